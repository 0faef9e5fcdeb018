#!/usr/bin/env python3
"""
Round-8 additions to the golden fixtures (run in the build container only; make_golden.py has the rules: the reference is IMPORTED
here, the fixtures hold inputs and the reference's OUTPUTS, never its source).

  track.npz   the reference's realtime path, executed here on seeded inputs:
                trk_*  HandDetector.track(com, size, dsize, doHandSize=False) (/root/reference/src/util/handdetector.py:504-544) with a
                       stub refineNet whose computeOutput returns seeded offsets and records what it is handed: windows inside the
                       frame, leaving it, and -- with a camera whose principal point is (0, 0) -- a centre that lands on (0, 0, 0),
                       once over a valid centre pixel and once over an all-zero window (the allclose fallback of :522-523);
                in*_   the three arrays refineCoM (:634-676) hands to the net for those calls;
                est_*  RealtimeHandposePipeline.estimatePose (/root/reference/src/util/realtimehandposepipeline.py:339-370) for all
                       eight (hand, invX, invY) combinations on a stub pose net, and the caller's pose * cube[2] / 2. + com3D (:198);
                det_*  RealtimeHandposePipeline.detect (:296-337) in tracking mode: its normalisation tail (:331-336) on a given crop.

The frames are not stored: tests regenerate them from `trk_seed` with oracle.augment.synthetic_frames (`trk_frame_sum` guards that).

What is stubbed, and why the pinned numbers do not depend on it.  cv2 is absent, so
  * HandDetector.resizeCrop (cv2.resize) is replaced by the oracle's resize_nn: the stub net ignores its input, so the centre that
    track returns does not depend on the resize; the recorded net inputs are refineCoM's construction on that resized window;
  * HandDetector.cropArea3D (cv2.resize inside) is replaced for the det_* case by a function returning a GIVEN crop in mm, so what
    is pinned there is exactly the tail of detect;
  * realtimehandposepipeline.py imports the Theano net classes and the matplotlib evaluation classes at module level: placeholder
    modules with empty classes satisfy those imports; the pipeline object is made with __new__ and given the attributes detect /
    estimatePose read (`.value` holders instead of multiprocessing.Value: the reference only reads `.value`).
Hand-size estimation (doHandSize=True) and HandDetector.detect need cv2.findContours and are not run.

NumPy 1 arithmetic.  The reference ran on NumPy 1, where `float32 scalar * Python float` is a float64; on NumPy 2 (this container) it
is a float32.  The importers' projections read self.fx / self.ux: the importer objects used here carry them as numpy.float64 scalars,
which makes every such product a float64 on NumPy 2 as well (float32 / float32 stays float32 on both) -- the arithmetic the reference
had.  The other expressions on the path (float32 array op Python float) have the same result type on both.
"""
import os
import sys
import types

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True


class _V(object):
    def __init__(self, value):
        self.value = value


class _Cfg(object):
    pass


class StubRefineNet(object):
    """computeOutput returns the next seeded offset and keeps what it was handed."""

    def __init__(self, offsets):
        self.offsets, self.k, self.seen = offsets, 0, []
        self.cfgParams = _Cfg()
        self.cfgParams.numInputs = 3

    def computeOutput(self, inputs):
        self.seen.append([numpy.array(a) for a in inputs])
        out = self.offsets[self.k][None].astype('float32')
        self.k += 1
        return out


class StubPoseNet(object):
    def __init__(self, out, size):
        self.out, self.seen = out, []
        self.cfgParams = _Cfg()
        self.cfgParams.inputDim = (1, 1, size, size)
        self.layers = [self]

    def computeOutput(self, inp):
        self.seen.append(numpy.array(inp))
        return self.out.copy()


def ref_importer(imp, name):
    cls, args = {'icvl': (imp.ICVLImporter, (241.42, 241.42, 160., 120.)), 'nyu': (imp.NYUImporter, (588.03, 587.07, 320., 240.)),
                 'origin': (imp.ICVLImporter, (241.42, 241.42, 0., 0.))}[name]
    o = cls.__new__(cls)
    imp.DepthImporter.__init__(o, *args)
    for a in ('fx', 'fy', 'ux', 'uy'):
        setattr(o, a, numpy.float64(getattr(o, a)))              # NumPy 1 arithmetic, see the header
    return o


def track_cases():
    """(camera name, frame index, centre, cube, net offset).  Frames: synthetic_frames(RandomState(trk_seed), 6, icvl, 120, 160)."""
    rng = numpy.random.RandomState(82)
    cases = []
    for cam in ('icvl', 'nyu'):
        for i in range(6):
            cases.append([cam, i, None, (250., 250., 250.) if i % 2 else (300., 280., 260.), rng.normal(0, 0.1, 3).astype('float32')])
    # the centre lands on (0, 0, 0): camera with its principal point at the origin, from (0, 0, 300) by (0, 0, -2) * 150
    cases.append(['origin', 0, numpy.float32([0., 0., 300.]), (300., 300., 300.), numpy.float32([0., 0., -2.])])      # valid centre pixel
    cases.append(['origin', 1, numpy.float32([0., 0., 300.]), (300., 300., 300.), numpy.float32([0., 0., -2.])])      # all-zero window
    return cases


def make_track():
    import make_golden as G                                    # placeholder modules, numpy shims, REF on sys.path
    from oracle import augment as A
    hd_mod = sys.modules.get('util.handdetector') or G.load_py2_module('util.handdetector', 'util/handdetector.py')
    imp = sys.modules.get('data.importers') or G.load_py2_module('data.importers', 'data/importers.py')
    for nm, names in (('net.poseregnet', ('PoseRegNet', 'PoseRegNetParams')), ('net.resnet', ('ResNet', 'ResNetParams')),
                      ('net.scalenet', ('ScaleNet', 'ScaleNetParams')),
                      ('util.handpose_evaluation', ('ICVLHandposeEvaluation', 'NYUHandposeEvaluation', 'MSRAHandposeEvaluation'))):
        if nm not in sys.modules:
            m = types.ModuleType(nm)
            for n in names:
                setattr(m, n, type(n, (object,), {}))
            sys.modules[nm] = m
    rt_mod = G.load_py2_module('util.realtimehandposepipeline', 'util/realtimehandposepipeline.py')
    HD, RTP = hd_mod.HandDetector, rt_mod.RealtimeHandposePipeline
    d = {}

    # ---- track ----
    seed, dsize = 81, (32, 32)
    frames, coms = A.synthetic_frames(numpy.random.RandomState(seed), 6, A.Camera.icvl(), 120, 160, (250., 250., 250.))
    frames[0][:40, :40] = 320.           # 'origin' case 0: a centre pixel inside the cube around (0, 0, 300)
    frames[1][:70, :70] = 0.             # 'origin' case 1: nothing there
    d['trk_seed'], d['trk_frame_sum'], d['trk_dsize'] = numpy.array(seed), numpy.float64(frames.astype('float64').sum()), numpy.array(dsize)
    cases = track_cases()
    names, idx, com_in, cubes, offs, com_out = [], [], [], [], [], []
    for k, (cam, i, com, cube, off) in enumerate(cases):
        com = coms[i] if com is None else com
        o = ref_importer(imp, cam)
        net = StubRefineNet([off])
        hd = HD(frames[i].copy(), abs(float(o.fx)), abs(float(o.fy)), importer=o, refineNet=net)
        hd.resizeCrop = lambda crop, sz: A.resize_nn(crop, sz)                    # stand-in for cv2.resize, see the header
        loc, size = hd.track(com.copy(), cube, dsize=dsize, doHandSize=False)
        assert size == cube and len(net.seen) == 1
        names.append(cam)
        idx.append(i)
        com_in.append(com)
        cubes.append(cube)
        offs.append(off)
        com_out.append(numpy.asarray(loc))
        for j in range(3):
            d['in%d_%d' % (j, k)] = net.seen[0][j]
    d['trk_cam'], d['trk_frame'] = numpy.array(names), numpy.array(idx)
    d['trk_com_in'], d['trk_cube'], d['trk_off'] = numpy.float32(com_in), numpy.float64(cubes), numpy.float32(offs)
    d['trk_com_out'] = numpy.stack(com_out)
    assert d['trk_com_out'].dtype == numpy.float32
    # without a refinement net the reference refuses
    try:
        HD(frames[0].copy(), 241.42, 241.42).track(coms[0], (250., 250., 250.), doHandSize=False)
        raise AssertionError("no RuntimeError")
    except RuntimeError as e:
        assert str(e) == "Need refineNet for this"

    # ---- estimatePose and the caller's de-normalisation ----
    rng = numpy.random.RandomState(83)
    crop = rng.uniform(-1., 1., (16, 16)).astype('float32')
    out = rng.normal(0, 0.4, (1, 42)).astype('float32')
    com3D = numpy.float32([12.5, -40.25, 512.3])
    cube = (300, 280, 250)
    d['est_crop'], d['est_out'], d['est_com3D'], d['est_cube'] = crop, out, com3D, numpy.array(cube)
    for k in range(8):
        hand, invX, invY = k & 1, bool(k & 2), bool(k & 4)
        p = RTP.__new__(RTP)
        p.poseNet = StubPoseNet(out, 16)
        p.hand = _V(RTP.HAND_RIGHT if hand else RTP.HAND_LEFT)
        cfg = {'fx': 241.42, 'fy': 241.42, 'cube': cube}
        if k & 6:                        # (the keys are optional in the reference: absent in case 0 / 1)
            cfg.update(invX=invX, invY=invY)
        p.sync = {'config': cfg}
        jj = p.estimatePose(crop, com3D)
        d['est_in_%d' % k], d['est_jj_%d' % k] = p.poseNet.seen[0], numpy.array(jj)
        d['est_pose_%d' % k] = jj * p.sync['config']['cube'][2] / 2. + com3D
        assert d['est_pose_%d' % k].dtype == numpy.float32

    # ---- the tail of detect ----
    o = ref_importer(imp, 'nyu')
    crop_mm = rng.uniform(480., 760., (16, 16)).astype('float32')
    crop_mm[rng.uniform(size=(16, 16)) < 0.3] = 0.
    off = numpy.float32([0.03, -0.02, 0.05])
    cfg = {'fx': 588., 'fy': 587., 'cube': (300, 300, 300)}
    orig = HD.cropArea3D
    HD.cropArea3D = lambda self, com=None, size=(250, 250, 250), dsize=(128, 128), docom=False: (crop_mm.copy(), numpy.eye(3), com)
    HD.resizeCrop = lambda self, crop, sz: A.resize_nn(crop, sz)
    try:
        p = RTP.__new__(RTP)
        p.importer, p.comrefNet, p.poseNet = o, StubRefineNet([off]), StubPoseNet(out, 16)
        p.sync = {'config': cfg}
        p.state, p.tracking, p.hand = _V(RTP.STATE_RUN), _V(True), _V(RTP.HAND_LEFT)
        p.lastcom = coms[2].copy()
        p.handsizes, p.numinitframes, p.verbose = [], 50, False
        got, M, c3 = p.detect(frames[2].copy())
    finally:
        HD.cropArea3D = orig
        del HD.resizeCrop
    d['det_frame'], d['det_lastcom'], d['det_off'], d['det_crop_mm'] = numpy.array(2), coms[2], off, crop_mm
    d['det_loc'], d['det_crop'], d['det_com3D'], d['det_cube'] = numpy.asarray(p.lastcom), got, numpy.asarray(c3), numpy.array(cfg['cube'])
    assert got.dtype == numpy.float32 and numpy.array_equal(M, numpy.eye(3))
    numpy.savez_compressed(os.path.join(HERE, 'track.npz'), **d)
    return d


if __name__ == '__main__':
    out = make_track()
    print('track.npz:', len(out), 'arrays,', os.path.getsize(os.path.join(HERE, 'track.npz')), 'bytes')
