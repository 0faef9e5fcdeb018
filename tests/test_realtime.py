"""The realtime path (hipdp/tracker.py, util/realtimehandposepipeline.py, util/cameradevice.py; ABI v13 kernels of csrc/crop.hip):
a depth frame in, the tracked hand's pose out, one device plan per frame.  Kernels against tests/track_ref.py (pinned to the
reference by tests/golden/track.npz) and against the crop kernels that are already pinned; the tracker plan stage by stage, free
running against the host-carried per-call API, its structure, a lost track, and the class API on an on-disk sequence.  Every kernel /
plan test runs on the emulator (CPU tier) and through libdpp_hip.so (-m gpu)."""
import os

import numpy as np
import pytest

from data.importers import ICVLImporter, NYUImporter
from hipdp import ops
from hipdp import runtime as R
from oracle import augment as A
from oracle import nets
from tests import track_ref as T
from tests.backends import BACKENDS, get_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
REC_BYTES = 76          # CropRec without its tail padding: 8 x int32, 2 x float64, 7 x float32


def _records(rt, buf, B):
    n = int(rt.lib.dpp_crop_record_bytes())
    return buf.get().reshape(B, n)[:, :REC_BYTES]


def _range_frames():
    """Frames for the range / prepare tests: the oracle's synthetic frames (centres inside, across and outside the frame, values
    beyond 1500 mm) with values below 10 mm added."""
    cam = A.Camera.icvl()
    cube = (250., 250., 250.)
    frames, coms = A.synthetic_frames(np.random.RandomState(11), 7, cam, 240, 320, cube)
    frames[1][np.random.RandomState(2).uniform(size=frames[1].shape) < 0.01] = 3.0
    frames[2][5, 7] = 0.5
    coms[3] = (-400., 120., 500.)            # window entirely outside the frame
    coms[4] = (160., 900., 450.)
    return cam, cube, frames, coms


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('shape', [(240, 320), (37, 45)])
def test_frame_range_and_ranged_prepare_equal_crop_prepare(backend, shape):
    rt = get_runtime(backend)
    cam, cube, frames, coms = _range_frames()
    H, W = shape
    frames = np.ascontiguousarray(frames[:, :H, :W])                      # 37 x 45: not a multiple of 4 pixels, the scalar path
    if (H, W) != (240, 320):
        coms = coms * np.float32([W / 320., H / 240., 1.])
    B = frames.shape[0]
    fr, co = rt.upload(frames), rt.upload(coms)
    cu = rt.upload(np.tile(np.float32(cube), (B, 1)))
    partial = ops.frame_range_workspace(rt, B)
    ops.frame_range(rt, fr, B, H, W, partial)(rt.stream)
    rt.synchronize()
    p = partial.get().reshape(B, -1, 2)
    for i in range(B):
        _, lo, hi = A.detector_preprocess(frames[i])
        assert max(10, p[i, :, 0].min()) == lo and min(1500, p[i, :, 1].max()) == hi
    nrec = int(rt.lib.dpp_crop_record_bytes())
    for stretch in (False, True):
        for dsz in (128, 96):
            r0, r1 = rt.alloc(B * nrec, np.uint8), rt.alloc(B * nrec, np.uint8)
            M0, M1 = rt.alloc((B, 9), zero=False), rt.alloc((B, 9), zero=False)
            ops.crop_prepare(rt, fr, B, H, W, co, cu, cam.fx, cam.fy, dsz, r0, M0, stretch=stretch)(rt.stream)
            ops.crop_prepare_ranged(rt, partial, B, co, cu, cam.fx, cam.fy, dsz, r1, M1, stretch=stretch)(rt.stream)
            rt.synchronize()
            assert np.array_equal(_records(rt, r0, B), _records(rt, r1, B))
            assert np.array_equal(M0.get(), M1.get())


@pytest.mark.parametrize('backend', BACKENDS)
def test_crop_flip_x_is_the_mirrored_crop(backend):
    rt = get_runtime(backend)
    cam, cube, frames, coms = _range_frames()
    B, H, W = frames.shape
    fr, co = rt.upload(frames), rt.upload(coms)
    cu = rt.upload(np.tile(np.float32(cube), (B, 1)))
    rec = rt.alloc(B * int(rt.lib.dpp_crop_record_bytes()), np.uint8)
    for dsz in (128, 50):
        ops.crop_prepare(rt, fr, B, H, W, co, cu, cam.fx, cam.fy, dsz, rec, None)(rt.stream)
        for flags, fill, pad in ((0, None, 0.), (ops.CROP_NORMALIZE, None, 0.), (ops.CROP_BILINEAR, None, 0.),
                                 (ops.CROP_NO_RANGE | ops.CROP_NO_THRESH, 7., 3.), (ops.CROP_NORMALIZE | ops.CROP_BILINEAR | ops.CROP_NO_RANGE, None, 0.)):
            a, b = rt.alloc((B, dsz, dsz), zero=False), rt.alloc((B, dsz, dsz), zero=False)
            ops.crop_warp_ex(rt, fr, rec, B, H, W, dsz, a, flags=flags, fill_value=fill, pad_value=pad)(rt.stream)
            ops.crop_warp_ex(rt, fr, rec, B, H, W, dsz, b, flags=flags | ops.CROP_FLIP_X, fill_value=fill, pad_value=pad)(rt.stream)
            rt.synchronize()
            plain, flipped = a.get(), b.get()
            assert np.array_equal(flipped, plain[:, :, ::-1]), (dsz, flags)
            assert not np.array_equal(flipped, plain)
    assert ops.CROP_FLIP_X == 16
    assert rt.lib.dpp_crop_warp_ex(fr.ptr, rec.ptr, B, H, W, 128, 32, 0., 0., 0., a.ptr, None) != 0      # unknown flag bits are refused


def _rec_fields(raw):
    dt = np.dtype([('xstart', 'i4'), ('ystart', 'i4'), ('cw', 'i4'), ('ch', 'i4'), ('szw', 'i4'), ('szh', 'i4'), ('xs', 'i4'), ('ys', 'i4'),
                   ('ifx', 'f8'), ('ify', 'f8'), ('min_depth', 'f4'), ('max_depth', 'f4'), ('zstart', 'f4'), ('zend', 'f4'), ('far_v', 'f4'),
                   ('norm_off', 'f4'), ('norm_div', 'f4')])
    assert dt.itemsize == REC_BYTES
    return np.ascontiguousarray(raw).view(dt).reshape(-1)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('camname', ['icvl', 'nyu', 'origin'])
def test_track_refine_equals_crop_refine_plus_prepare(backend, camname):
    """The fused kernel against the two pinned ones it replaces, and its status word.  Camera 'origin' has its principal point at
    (0, 0), so a centre at depth 0 projects to (0, 0, 0): numpy.allclose(com, 0) and the centre-pixel fallback."""
    rt = get_runtime(backend)
    cam = dict(icvl=A.Camera.icvl(), nyu=A.Camera.nyu(), origin=A.Camera(241.42, 241.42, 0., 0., False))[camname]
    camt = (cam.fx, cam.fy, cam.ux, cam.uy, int(cam.flip_y))
    cube = (300., 300., 300.)
    H, W = 240, 320
    frames, coms = A.synthetic_frames(np.random.RandomState(5), 8, A.Camera.icvl(), H, W, cube)
    B = frames.shape[0]
    rng = np.random.RandomState(6)
    net_out = rng.normal(0, 0.08, (B, 3)).astype(np.float32)
    # frames 6, 7: the net moves the centre to depth exactly 0 (-2 * 150 + 300), from the principal point so that x = y = 0 in 3-D
    for i in (6, 7):
        coms[i] = (cam.ux, cam.uy, 300.)
        net_out[i] = (0., 0., -2.)
    if camname == 'origin':
        frames[6][:60, :80] = 320.            # the window around (0, 0, 300) has a centre pixel inside the cube: the fallback finds a depth
        frames[7][:60, :80] = 0.              # ... and here it does not
    fr, co, no = rt.upload(frames), rt.upload(coms), rt.upload(net_out)
    cu = rt.upload(np.tile(np.float32(cube), (B, 1)))
    nrec = int(rt.lib.dpp_crop_record_bytes())
    rec0 = rt.alloc(B * nrec, np.uint8)
    ops.crop_prepare(rt, fr, B, H, W, co, cu, abs(cam.fx), abs(cam.fy), 128, rec0, None, stretch=True)(rt.stream)
    c_ref, c3_ref = rt.alloc((B, 3), zero=False), rt.alloc((B, 3), zero=False)
    ops.crop_refine(rt, fr, rec0, B, H, W, co, cu, no, camt, c_ref, com3d_out=c3_ref)(rt.stream)
    c_new, c3_new, rec1, M1 = rt.alloc((B, 3), zero=False), rt.alloc((B, 3), zero=False), rt.alloc(B * nrec, np.uint8), rt.alloc((B, 9), zero=False)
    status = rt.alloc((B,), np.int32)
    ops.track_refine(rt, fr, rec0, B, H, W, co, cu, no, camt, abs(cam.fx), abs(cam.fy), 96, c_new, c3_new, rec1, status, M_out=M1)(rt.stream)
    rt.synchronize()
    st, cn = status.get(), c_new.get()
    assert np.array_equal(cn, c_ref.get())                            # the centre: crop_refine's, lost or not
    want = [0] * 6 + ([1, 1] if camname != 'origin' else [0, 1])
    assert st.tolist() == want, st
    assert st.tolist() == [int(T.is_lost(c)) for c in cn]
    if camname == 'origin':
        assert cn[6].tolist() == [0., 0., 320.]                       # allclose(com, 0) -> centre pixel of the window
    ok = np.nonzero(st == 0)[0]
    assert np.array_equal(c3_new.get()[ok], c3_ref.get()[ok])
    rec2, M2 = rt.alloc(len(ok) * nrec, np.uint8), rt.alloc((len(ok), 9), zero=False)
    ops.crop_prepare(rt, rt.upload(frames[ok]), len(ok), H, W, rt.upload(cn[ok]), cu, abs(cam.fx), abs(cam.fy), 96, rec2, M2)(rt.stream)
    rt.synchronize()
    assert np.array_equal(_records(rt, rec1, B)[ok], _records(rt, rec2, len(ok)))
    assert np.array_equal(M1.get()[ok], M2.get())
    # a lost frame: an empty window, so that the crop is all zeros and nothing divides by zero, M = identity, com3D = 0
    lost = np.nonzero(st)[0]
    r = _rec_fields(_records(rt, rec1, B))
    out = rt.alloc((B, 96, 96), zero=False)
    ops.crop_warp_ex(rt, fr, rec1, B, H, W, 96, out, flags=ops.CROP_NORMALIZE)(rt.stream)
    rt.synchronize()
    for i in lost:
        assert r['cw'][i] == 0 and r['ch'][i] == 0 and r['szw'][i] == 0 and r['szh'][i] == 0
        assert np.array_equal(M1.get()[i], np.eye(3, dtype=np.float32).ravel()) and not c3_new.get()[i].any()
        assert not out.get()[i].any()
    # in place: the state buffer and the record buffer may be both input and output
    co2, rec3 = rt.upload(coms), rt.alloc(B * nrec, np.uint8)
    rt.copy(rec3, rec0)
    ops.track_refine(rt, fr, rec3, B, H, W, co2, cu, no, camt, abs(cam.fx), abs(cam.fy), 96, co2, c3_new, rec3, status)(rt.stream)
    rt.synchronize()
    assert np.array_equal(co2.get(), cn) and np.array_equal(_records(rt, rec3, B), _records(rt, rec1, B))


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('camname', ['icvl', 'nyu'])
def test_pose_finish_all_flag_combinations(backend, camname):
    rt = get_runtime(backend)
    cam = dict(icvl=A.Camera.icvl(), nyu=A.Camera.nyu())[camname]
    camt = (cam.fx, cam.fy, cam.ux, cam.uy, int(cam.flip_y))
    B, J = 3, 14
    rng = np.random.RandomState(8)
    net_out = rng.normal(0, 0.4, (B, J, 3)).astype(np.float32)
    cubes = np.float32([[250, 250, 250], [300, 300, 300], [233, 241, 287]])
    com3d = np.float32([[12.5, -40.25, 512.3], [-100.1, 33.3, 801.7], [0.3, 0.7, 333.3]])
    net_out[2, 3] = -com3d[2] / (cubes[2, 2] / np.float32(2.))        # a joint (nearly) at the camera centre
    no, cu, c3 = rt.upload(net_out), rt.upload(cubes), rt.upload(com3d)
    p3, pi = rt.alloc((B, J, 3), zero=False), rt.alloc((B, J, 3), zero=False)
    for flags in range(8):
        hand, invX, invY = flags & 1, bool(flags & 2), bool(flags & 4)
        assert (ops.POSE_HAND_RIGHT, ops.POSE_INV_X, ops.POSE_INV_Y) == (1, 2, 4)
        ops.pose_finish(rt, no, B, J, cu, c3, camt, flags, p3, pi)(rt.stream)
        rt.synchronize()
        got3, goti = p3.get(), pi.get()
        for b in range(B):
            want = T.denormalize(T.pose_signs(net_out[b], hand, invX, invY), cubes[b, 2], com3d[b])
            assert np.array_equal(got3[b], want), (flags, b)
            # the projection: exact against the oracle's joints3DToImg on the float32 pose -- the expression the crop kernels' shared
            # `toimg` is held to (float32 x / z, float64 scale and offset, one rounding)
            assert np.array_equal(goti[b], cam.joints3DToImg(want)), (flags, b)
    assert rt.lib.dpp_pose_finish(no.ptr, B, J, cu.ptr, c3.ptr, 1., 1., 0., 0., 0, 8, p3.ptr, pi.ptr, None) != 0


def _iter_ref(frames, coms, cube, fx, fy, n):
    out, ill = [], []
    for f, c in zip(frames, coms):
        d, lo, hi = A.detector_preprocess(f)
        r, bad = T.refine_com_iterative(d, c, n, cube, fx, fy, lo, hi)
        out.append(r.astype(np.float32))
        ill.append(bad)
    return np.stack(out), np.array(ill)


@pytest.mark.parametrize('backend', BACKENDS)
def test_refine_com_iterative_on_the_device(backend):
    from util.handdetector import refine_com_iterative
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    g = np.load(os.path.join(GOLD, 'crop.npz'))
    frames, coms = g['frames'], g['coms']
    cube = (250., 250., 250.)
    B = frames.shape[0]
    cubes = np.tile(np.float32(cube), (B, 1))
    got, st = refine_com_iterative(frames, coms, cubes, 241.42, 241.42, 3, runtime=rt, return_status=True)
    ref, ill = _iter_ref(frames, coms, cube, 241.42, 241.42, 3)
    assert not st.any() and not ill.any()
    assert np.array_equal(got, ref)
    np.testing.assert_allclose(got, g['com_it'], rtol=1e-5)           # the reference's own result (it sums depth in float32)
    for n in (0, 1, 5):
        got = refine_com_iterative(frames, coms, cubes, 241.42, 241.42, n, runtime=rt)
        assert np.array_equal(got, _iter_ref(frames, coms, cube, 241.42, 241.42, n)[0]), n
    # full-size frames, centres near and across the border
    cam = A.Camera.nyu()
    cube = (300., 300., 300.)
    frames, coms = A.synthetic_frames(np.random.RandomState(9), 6, cam, 480, 640, cube)
    cubes = np.tile(np.float32(cube), (6, 1))
    got, st = refine_com_iterative(frames, coms, cubes, cam.fx, cam.fy, 5, runtime=rt, return_status=True)
    ref, ill = _iter_ref(frames, coms, cube, abs(cam.fx), abs(cam.fy), 5)
    assert np.array_equal(st != 0, ill)
    assert np.array_equal(got[~ill], ref[~ill])
    assert np.isfinite(got).all()


# ---- the tracker plan ------------------------------------------------------------------------------------------------------
def _track_nets(rt, backend, J=14, zero_refine=False):
    """ScaleNet and a pose net at batch one: a small PoseRegNet on the emulator, the 128 x 128 ResNet on the GPU."""
    from tests.test_engine import make_net
    from tests.test_poseregnet import make as make_poseregnet
    from tests.test_scalenet import make as make_scalenet
    snet, sonet, sP = make_scalenet(rt, 1)
    if zero_refine:                     # the net regresses the constant offset (0, 0, -2): last layer W = 0, b = (0, 0, -2)
        W, b = snet.layers[-1].params
        W.set_value(np.zeros_like(W.get_value()))
        b.set_value(np.float32([0., 0., -2.]))
    if backend == 'hip':
        pnet, ponet, pP = make_net(rt, 1, 1, 128, J, 3)
    else:
        pnet, ponet, pP = make_poseregnet(rt, 0, 1, 128, J, 3)
    snet.setDeterministic()
    pnet.setDeterministic()
    return (snet, sonet, sP), (pnet, ponet, pP)


def _oracle_forward(onet, P):
    P64 = nets.cast_params(P, np.float64)

    def fwd(ins):
        ins = ins if isinstance(ins, list) else [ins]
        out, _ = nets.forward(onet, P64, [np.asarray(a, np.float64) for a in ins] if len(ins) > 1 else np.asarray(ins[0], np.float64), train=False)
        return out[:1]
    return fwd


def _sequence(backend):
    """240 x 320, 8 frames on the emulator; on the GPU also 480 x 640, 64 frames."""
    out = [(ICVLImporter('../data/ICVL/'), A.Camera.icvl(), (250., 250., 250.), 240, 320, 8)]
    if backend == 'hip':
        out.append((NYUImporter('../data/NYU/'), A.Camera.nyu(), (300., 300., 300.), 480, 640, 64))
    return out


@pytest.mark.parametrize('backend', BACKENDS)
def test_tracker_stages_match_restatement_teacher_forced(backend):
    from hipdp.tracker import HandTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, sonet, sP), (pnet, ponet, pP) = _track_nets(rt, backend)
    sfwd, pfwd = _oracle_forward(sonet, sP), _oracle_forward(ponet, pP)
    for di, cam, cube, H, W, n in _sequence(backend):
        frames, coms = T.drifting_sequence(np.random.RandomState(31), n, cam, H, W, cube)
        fx, fy = abs(cam.fx), abs(cam.fy)
        for hand in (T.HAND_LEFT, T.HAND_RIGHT):
            tr = HandTracker(rt, di, pnet, snet, H, W, cube, hand_right=hand == T.HAND_RIGHT)
            for i in range(1, n, 1 if n <= 8 else 9):
                tr.reset(coms[i - 1])                                  # teacher: the previous frame's true centre
                res = tr.process(frames[i], return_crop=True)
                assert res['status'] == 0
                d, lo, hi = A.detector_preprocess(frames[i])
                c_ref, rz, _ = T.track(d, coms[i - 1], cube, cam, fx, fy, sfwd)
                ins = T.refine_inputs(rz, cube, coms[i - 1])
                for t, a in zip(tr.ceng.x_ins, ins):                  # what the refinement net sees: exact
                    assert np.array_equal(t.buf.get().reshape(a.shape), a), i
                assert np.array_equal(ins[0][0, 0], A.normalize_crop(rz, coms[i - 1][2], cube[2]))
                np.testing.assert_allclose(res['com'], c_ref, rtol=0, atol=2e-4)      # float32 net vs float64 oracle net
                crop, M, com3D, _ = T.detect_tail(d, res['com'], cube, cam, fx, fy, (128, 128))
                want = T.pose_input(crop, hand)[0, 0]
                assert np.array_equal(res['crop'], want), i           # the final crop around the device's own centre: exact
                np.testing.assert_allclose(res['M'], M, rtol=1e-6, atol=1e-4)
                assert np.array_equal(res['com3D'], com3D)
                o = pfwd(want[None, None])[0].reshape(-1, 3).copy()      # the float64 oracle net on the device's own crop
                if hand == T.HAND_RIGHT:
                    o[:, 0] *= -1.
                pose64 = o * cube[2] / 2. + com3D.astype(np.float64)
                assert np.abs(res['pose'] - pose64).max() < 1e-3      # DESIGN section 2's bar: 1e-3 mm
                assert np.array_equal(res['pose_img'], cam.joints3DToImg(res['pose']))


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('hand', [T.HAND_LEFT, T.HAND_RIGHT], ids=['left', 'right'])
def test_free_running_device_state_equals_host_carried_state(backend, hand):
    """process_sequence (the centre never leaves the device) against the public per-call API with the centre carried by the host:
    bit-identical centres, crops and poses, every frame."""
    from hipdp.tracker import HandTracker
    from util.handdetector import HandDetector
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend)
    for di, cam, cube, H, W, n in _sequence(backend):
        frames, coms = T.drifting_sequence(np.random.RandomState(32), n, cam, H, W, cube)
        tr = HandTracker(rt, di, pnet, snet, H, W, cube, hand_right=hand == T.HAND_RIGHT)
        tr.reset(coms[0])
        seq = tr.process_sequence(frames, return_crops=True)
        assert len(seq) == n and all(r['status'] == 0 for r in seq)
        # frame by frame through process(): the same values
        tr.reset(coms[0])
        for i in range(n):
            r = tr.process(frames[i], return_crop=True)
            for k in ('pose', 'pose_img', 'com', 'com3D', 'M', 'crop'):
                assert np.array_equal(r[k], seq[i][k]), (i, k)
        com = coms[0].copy()
        moved = 0.
        for i in range(n):
            hd = HandDetector(frames[i].copy(), abs(di.fx), abs(di.fy), importer=di, refineNet=snet)
            loc, _ = hd.track(com, cube, dsize=(128, 128), doHandSize=False)
            crop, M, c = hd.cropArea3D(com=loc, size=cube, dsize=(128, 128))
            com3D = di.jointImgTo3D(c)
            sc = cube[2] / 2.
            crop[crop == 0] = com3D[2] + sc
            crop -= com3D[2]
            crop /= sc
            inp = np.ascontiguousarray(crop[None, None] if hand == T.HAND_LEFT else crop[None, None, :, ::-1]).astype(np.float32)
            jj = pnet.computeOutput(inp)[0].reshape(-1, 3)
            if hand == T.HAND_RIGHT:
                jj[:, 0] *= (-1.)
            pose = jj * cube[2] / 2. + com3D
            assert pose.dtype == np.float32
            assert np.array_equal(loc, seq[i]['com']), (i, loc, seq[i]['com'])
            assert np.array_equal(inp[0, 0], seq[i]['crop']), i
            assert np.array_equal(pose, seq[i]['pose']), i
            moved = max(moved, np.abs(loc - coms[0]).max())
            com = loc
        assert moved > 0.                                              # the state does change from frame to frame


@pytest.mark.parametrize('backend', BACKENDS)
def test_tracker_plan_structure(backend, monkeypatch):
    from hipdp.tracker import HandTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend)
    di, cam, cube, H, W, n = _sequence(backend)[0]
    frames, coms = T.drifting_sequence(np.random.RandomState(33), 3, cam, H, W, cube)
    tr = HandTracker(rt, di, pnet, snet, H, W, cube)
    plan = tr.plan(0)
    launches = plan.launches()
    whole_frame = [l for l in launches if (l.meta or {}).get('bytes', 0) >= 4.0 * H * W and (l.meta or {}).get('kernel') in ('frame_range', 'crop_prepare')]
    assert [l.name for l in whole_frame] == ['frame_range']          # exactly one launch reads the whole frame for the depth range
    assert not any(l.fn is rt.lib.dpp_crop_prepare or l.fn is rt.lib.dpp_crop_com for l in launches)
    assert [l.fn for l in launches].count(rt.lib.dpp_crop_prepare_ranged) == 1 and [l.fn for l in launches].count(rt.lib.dpp_track_refine) == 1
    assert len(launches) == 4 + (len(tr.ceng.x_ins) - 1) + len(tr.ceng.fwd.launches()) + 1 + len(tr.peng.fwd.launches()) + 1
    tr.reset(coms[0])
    tr.process(frames[0])                                              # records the plan
    calls = dict(h2d=[], run=0, d2h=[])
    real_in, real_out, real_run = rt.copy_in, rt.download, ops.Plan.run
    monkeypatch.setattr(rt, 'copy_in', lambda buf, arr: (calls['h2d'].append(buf.ptr), real_in(buf, arr))[1], raising=False)
    monkeypatch.setattr(rt, 'download', lambda buf: (calls['d2h'].append(buf.ptr), real_out(buf))[1], raising=False)
    monkeypatch.setattr(ops.Plan, 'run', lambda self, r: (calls.__setitem__('run', calls['run'] + 1), real_run(self, r))[1])
    r1 = tr.process(frames[1])
    assert calls['h2d'] == [tr.frames[0].ptr] and calls['run'] == 1   # one upload (the frame), one plan
    assert calls['d2h'] == [tr.res.ptr]                                # one download: the result block (the centre in it is reported, never fed back)
    r2 = tr.process(frames[2])
    assert calls['h2d'] == [tr.frames[0].ptr] * 2 and calls['run'] == 2 and calls['d2h'] == [tr.res.ptr] * 2
    assert not np.array_equal(r1['com'], r2['com'])
    monkeypatch.undo()
    with pytest.raises(ValueError):
        tr.process(frames[0][:10])
    with pytest.raises(ValueError):
        tr.reset((10., 10., 0.))


@pytest.mark.parametrize('backend', BACKENDS)
def test_lost_track_is_reported_and_refused_until_reset(backend):
    """A refinement net that always answers (0, 0, -2): from a centre at 300 mm with a 300 mm cube the new depth is exactly 0 in
    float32 (-2 * 150 + 300)."""
    from hipdp.tracker import LOST, HandTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend, zero_refine=True)
    di, cam = ICVLImporter('../data/ICVL/'), A.Camera.icvl()
    cube, H, W = (300., 300., 300.), 240, 320
    frames, coms = T.drifting_sequence(np.random.RandomState(34), 3, cam, H, W, cube)
    assert np.array_equal(snet.computeOutput(nets.scalenet_inputs(np.zeros((1, 1, 128, 128), np.float32))), np.float32([[0., 0., -2.]]))
    tr = HandTracker(rt, di, pnet, snet, H, W, cube)
    with pytest.raises(RuntimeError):
        tr.process(frames[0])                                          # never started
    tr.reset((150., 110., 300.))
    res = tr.process(frames[0], return_crop=True)
    assert res['status'] == LOST and res['com'][2] == 0.
    for k in ('pose', 'pose_img', 'com', 'com3D', 'M', 'crop'):
        assert np.isfinite(res[k]).all(), k
    assert not res['crop'].any() and np.array_equal(res['M'], np.eye(3, dtype=np.float32))
    with pytest.raises(RuntimeError):
        tr.process(frames[1])
    with pytest.raises(RuntimeError):
        tr.process_sequence(frames[1:])
    # from 700 mm the same net lands at 400 mm: the track goes on, and equals a fresh tracker's
    tr.reset((150., 110., 700.))
    a = tr.process(frames[1], return_crop=True)
    fresh = HandTracker(rt, di, pnet, snet, H, W, cube)
    fresh.reset((150., 110., 700.))
    b = fresh.process(frames[1], return_crop=True)
    assert a['status'] == 0 and a['com'][2] == 400.
    for k in ('pose', 'pose_img', 'com', 'com3D', 'M', 'crop'):
        assert np.array_equal(a[k], b[k]), k
    # in a sequence: the lost frame is the last one returned
    tr.reset((150., 110., 600.))                                       # 600 -> 300 -> 0
    seq = tr.process_sequence(frames)
    assert [r['status'] for r in seq] == [0, LOST] and tr.lost


# ---- the class API ---------------------------------------------------------------------------------------------------------
def _write_icvl_sequence(base, name, frames, coms, cam, J=16, seed=3):
    """A drifting sequence in the ICVL file format (labels file + 16-bit PNGs), the way tests/test_importers.py writes one; joint 0 (the
    importer's crop joint) is the blob's centre."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    frames = np.round(frames)
    lines, gt3D = [], []
    os.makedirs(os.path.join(base, 'Depth', '201403121135'), exist_ok=True)
    for i in range(len(frames)):
        c3 = cam.jointImgTo3D(coms[i])
        g = c3[None, :] + rng.normal(0, 30., (J, 3)).astype(np.float32)
        g[0] = c3
        uvd = np.stack([cam.joint3DToImg(j) for j in g]).astype(np.float32)
        gt3D.append(g.astype(np.float32))
        rel = '201403121135/%s_%04d.png' % (name, i)
        Image.fromarray(frames[i].astype(np.uint16)).save(os.path.join(base, 'Depth', rel))
        lines.append(rel + ' ' + ' '.join('%.4f' % v for v in uvd.reshape(-1)) + ' \n')
    with open(os.path.join(base, name + '.txt'), 'w') as f:
        f.writelines(lines)
    return frames.astype(np.float32), np.stack(gt3D)


@pytest.mark.parametrize('backend', BACKENDS)
def test_pipeline_api_on_a_file_sequence(backend, tmp_path):
    from util.cameradevice import CameraDevice, FileDevice
    from util.handdetector import HandDetector
    from util.realtimehandposepipeline import RealtimeHandposePipeline
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    cam, cube = A.Camera.icvl(), (250, 250, 250)
    frames, coms = T.drifting_sequence(np.random.RandomState(35), 5, cam, 240, 320, tuple(float(c) for c in cube))
    base = str(tmp_path / 'ICVL')
    frames, _ = _write_icvl_sequence(base, 'test_seq_1', frames, coms, cam)
    di = ICVLImporter(base, useCache=False)
    files = [os.path.join(base, 'Depth', '201403121135', 'test_seq_1_%04d.png' % i) for i in range(5)]
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend, J=16)
    config = {'fx': 241.42, 'fy': 241.42, 'cube': cube}

    with pytest.raises(ValueError):
        FileDevice(files[0], di)
    with pytest.raises(NotImplementedError):
        CameraDevice().getDepth()
    dev = FileDevice(files, di)
    ok, f0 = dev.getDepth()
    assert ok is True and np.array_equal(f0, frames[0]) and dev.getLastDepthNum() == 1

    # the fused plan per frame ...
    for hand in ('left', 'right'):
        rtp = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=coms[0])
        assert rtp.tracking.value is True and rtp.hand.value == rtp.HAND_LEFT and rtp.state.value == rtp.STATE_IDLE
        if hand == 'right':
            rtp.processKey(ord('h'))
            assert rtp.hand.value == rtp.HAND_RIGHT
        poses = rtp.processVideo(FileDevice(files, di))
        assert poses.shape == (5, 16, 3) and poses.dtype == np.float32 and np.isfinite(poses).all()
        assert len(rtp.frame_times) == 5
        # ... equals detect + estimatePose called separately
        rtp2 = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=coms[0])
        rtp2.initNets()
        if hand == 'right':
            rtp2.processKey(ord('h'))
        for i in range(5):
            crop, M, com3D = rtp2.detect(frames[i].copy())
            pose = rtp2.estimatePose(crop, com3D) * config['cube'][2] / 2. + com3D
            assert np.array_equal(pose, poses[i]), (hand, i)
        assert np.array_equal(np.asarray(rtp2.lastcom), np.asarray(rtp.lastcom))
    # max_frames, invX / invY, the cube keys and reset
    rtp = RealtimeHandposePipeline(pnet, dict(config, invX=True, invY=True), di, comrefNet=snet, init_com=coms[0])
    p2 = rtp.processVideo(FileDevice(files, di), max_frames=2)
    assert p2.shape == (2, 16, 3)
    rtp3 = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=coms[0])
    p3 = rtp3.processVideo(FileDevice(files, di), max_frames=2)
    assert not np.array_equal(p2, p3)
    rtp.processKey(ord('+'))
    assert rtp.sync['config']['cube'] == (260, 260, 260)
    rtp.processKey(ord('-'))
    rtp.processKey(ord('-'))
    assert rtp.sync['config']['cube'] == (240, 240, 240)
    rtp.processKey(ord('r'))
    assert rtp.sync['config']['cube'] == cube and np.array_equal(rtp.lastcom, coms[0])
    assert np.array_equal(rtp.processVideo(FileDevice(files, di), max_frames=2), p2)       # the same track again after reset
    rtp.processKey(ord('q'))
    assert rtp.stop.value is True
    with pytest.raises(NotImplementedError):
        rtp.processKey(ord('i'))                                       # hand-size calibration
    # without a seed, or with tracking off, the pipeline needs HandDetector.detect
    rtp = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet)
    rtp.initNets()
    with pytest.raises(NotImplementedError):
        rtp.detect(frames[0].copy())
    rtp = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=coms[0])
    rtp.processKey(ord('t'))
    with pytest.raises(NotImplementedError):
        rtp.processVideo(FileDevice(files, di))
    # the NON-reference seed: whole-frame centre of mass + refineCoMIterative(5)
    rtp = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, seed_com=True)
    ps = rtp.processVideo(FileDevice(files, di), max_frames=2)
    assert ps.shape == (2, 16, 3) and np.isfinite(ps).all()
    # HandDetector's own errors
    hd = HandDetector(frames[0].copy(), 241.42, 241.42, importer=di)
    with pytest.raises(RuntimeError, match="Need refineNet for this"):
        hd.track(coms[0], cube, doHandSize=False)
    hd = HandDetector(frames[0].copy(), 241.42, 241.42, importer=di, refineNet=snet)
    with pytest.raises(NotImplementedError):
        hd.track(coms[0], cube)                                        # doHandSize=True: cv2.findContours
    with pytest.raises(NotImplementedError):
        hd.detect(size=cube)
    loc, size = hd.track(coms[0], cube, doHandSize=False)
    assert size == cube and loc.dtype == np.float32 and loc.shape == (3,)


@pytest.mark.parametrize('backend', BACKENDS)
def test_realtime_example_runs_end_to_end(backend, tmp_path):
    import importlib.util
    R.set_default_runtime(get_runtime(backend))
    cam, cube = A.Camera.icvl(), (250., 250., 250.)
    frames, coms = T.drifting_sequence(np.random.RandomState(36), 4, cam, 240, 320, cube)
    base = str(tmp_path / 'ICVL')
    _write_icvl_sequence(base, 'test_seq_1', frames, coms, cam)
    spec = importlib.util.spec_from_file_location('realtime_driver', os.path.join(ROOT, 'examples', 'test_realtimepipeline.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = 'resnet' if backend == 'hip' else 'poseregnet'               # (the 128x128 ResNet is too slow for the SIMT emulator)
    poses, err = mod.main(['--dataset', 'icvl', '--data', base, '--net', net, '--cache', str(tmp_path / 'cache')])
    assert poses.shape == (4, 16, 3) and np.isfinite(poses).all() and np.isfinite(err) and err > 0
    poses2, _ = mod.main(['--dataset', 'icvl', '--data', base, '--net', net, '--seed', 'com', '--hand', 'right', '--max-frames', '2',
                          '--cache', str(tmp_path / 'cache')])
    assert poses2.shape == (2, 16, 3) and np.isfinite(poses2).all()


# ---- the restatement against the reference's own output ------------------------------------------------------------------------
def test_track_ref_reproduces_the_reference_fixture():
    """tests/golden/track.npz (make_golden_r8.py ran the reference's track / refineCoM / estimatePose / detect): tests/track_ref.py gives
    the same centres, net inputs, poses and normalised crop, exactly."""
    g = np.load(os.path.join(GOLD, 'track.npz'))
    frames, coms = A.synthetic_frames(np.random.RandomState(int(g['trk_seed'])), 6, A.Camera.icvl(), 120, 160, (250., 250., 250.))
    frames[0][:40, :40] = 320.
    frames[1][:70, :70] = 0.
    assert frames.astype(np.float64).sum() == float(g['trk_frame_sum'])
    cams = dict(icvl=A.Camera.icvl(), nyu=A.Camera.nyu(), origin=A.Camera(241.42, 241.42, 0., 0., False))
    dsize = tuple(int(v) for v in g['trk_dsize'])
    n = len(g['trk_cam'])
    assert n == 14
    fallback = 0
    for k in range(n):
        cam = cams[str(g['trk_cam'][k])]
        d, lo, hi = A.detector_preprocess(frames[int(g['trk_frame'][k])])
        cube, off = tuple(float(v) for v in g['trk_cube'][k]), g['trk_off'][k]
        com2, rz, _ = T.track(d, g['trk_com_in'][k], cube, cam, abs(cam.fx), abs(cam.fy), lambda ins: off[None], rsize=dsize)
        assert com2.dtype == np.float32 and np.array_equal(com2, g['trk_com_out'][k]), (k, com2, g['trk_com_out'][k])
        ins = T.refine_inputs(rz, cube, g['trk_com_in'][k])
        for j in range(3):
            assert np.array_equal(ins[j], g['in%d_%d' % (j, k)]), (k, j)
        fallback += int(com2[0] == 0. and com2[1] == 0.)
    assert fallback == 2 and g['trk_com_out'][12].tolist() == [0., 0., 320.] and T.is_lost(g['trk_com_out'][13])
    for k in range(8):
        hand, invX, invY = k & 1, bool(k & 2), bool(k & 4)
        assert np.array_equal(T.pose_input(g['est_crop'], hand), g['est_in_%d' % k])
        jj = T.pose_signs(g['est_out'], hand, invX, invY)
        assert np.array_equal(jj, g['est_jj_%d' % k]), k
        assert np.array_equal(T.denormalize(jj, g['est_cube'][2], g['est_com3D']), g['est_pose_%d' % k]), k
    cam = cams['nyu']
    d, lo, hi = A.detector_preprocess(frames[int(g['det_frame'])])
    cube = tuple(float(v) for v in g['det_cube'])
    loc, _, _ = T.track(d, g['det_lastcom'], cube, cam, 588., 587., lambda ins: g['det_off'][None], rsize=(16, 16))
    assert np.array_equal(loc, g['det_loc'])
    com3D = cam.jointImgTo3D(loc)
    assert np.array_equal(com3D, g['det_com3D'])
    assert np.array_equal(T.normalize_tail(g['det_crop_mm'], com3D, cube), g['det_crop'])
