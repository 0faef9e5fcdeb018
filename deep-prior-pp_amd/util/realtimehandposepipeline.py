"""
RealtimeHandposePipeline -- the headless part of /root/reference/src/util/realtimehandposepipeline.py: a depth frame goes in, the hand
is followed from the previous frame's centre, 3-D joints come out.

Built: the constants and constructor, initNets, detect (tracking mode, :296-337), estimatePose (:339-370), processKey's state
changes, reset, and a headless processVideo(device) that returns the poses in mm and runs every frame as ONE device plan
(hipdp.tracker.HandTracker).  detect() + estimatePose() called separately go through the per-call API (HandDetector.track,
cropArea3D, computeOutput) and give the same numbers as the fused plan.

Not built: HandDetector.detect as the reference has it (contour analysis of depth slabs with cv2.findContours, it cannot be pinned
without OpenCV) and with it the detection mode of detect(); the key-driven hand-size calibration (STATE_INIT, estimateHandsize: cv2
contours as well); show, addStatusBar and the cv2 windows; the producer / consumer processes of processVideoThreaded (their shared
state is plain attributes here: `.value` holders instead of multiprocessing.Value, a dict instead of Manager().dict()).

The first frame needs a SEED: init_com= (image coordinates, z in mm, e.g. a dataset's annotation of the first frame), which also
switches tracking on; or seed_detect=True, whole-frame detection by connected components on the device
(HandDetector.detectComponents / HandTracker.acquire: the nearest 8-connected object of more than 200 px, the centre of mass of its
window, refineCoMIterative(com, 5, cube) -- detect's steps with component labelling in the place of cv2's contours, see
util.handdetector for the three deviations), used again after every LOST frame; or seed_com=True, an explicitly NON-reference seed
-- the centre of mass of the whole range-limited frame (what cropArea3D(com=None) uses) refined the same way.  seed_detect takes
precedence over seed_com.  A frame in which seed_detect finds no hand (and seed_com, if set, nothing either) is answered like a LOST
one and the next frame is searched again.  With tracking off, or an all-zero last centre and no seed at all, detect raises the
NotImplementedError of HandDetector.detect.  calibrateHandsize(device) is the headless counterpart of STATE_INIT (:312-324) on the component hand size.

SENSOR frames: with sensor=dict(dtype='uint16' | 'float32', median=bool, mirror=bool) the frames handed to processFrame /
processVideo / calibrateHandsize (and to detect) are RAW sensor frames of that dtype; the mirror, the 3x3 median and the conversion
to float32 of the reference's CreativeCameraDevice.getDepth (cameradevice.py:189-200) run at the head of the frame's device plan
(hipdp.tracker.HandTracker(sensor=...)), and the per-call paths filter through util.cameradevice.filter_depth first, so that both
routes see the same frame.

BACKGROUND: with background=dict(margin=[, rel=, min_seen=]) learnBackground(device, frames=N) learns a per-pixel model of the scene
without the hand (hipdp/tracker.py, BACKGROUND), and the fused path removes it from every frame on the device before the detector of
seed_detect, the tracker and calibrateHandsize look at it: on a fixed camera the nearest object is then the hand, not the desk.  The
per-call API (detect) runs the host HandDetector and does not see the model.

A LOST track (the tracked centre's depth is close to 0: the reference would crop the middle of the frame through comToBounds'
"CoM ill-defined" branch, which is not built) gives a zero crop, eye(3) and a zero com3D -- the answer of :326-327 -- and clears
the last centre, so that the next frame needs a seed again.

SEVERAL cameras and hands: MultiStreamPipeline (below) plays a list of devices through hipdp.multitrack.MultiTracker -- one device
plan per tick for all tracks, with the same seeding rules per track.
"""
import copy
import time

import numpy

from net.poseregnet import PoseRegNet, PoseRegNetParams
from net.resnet import ResNet, ResNetParams
from net.scalenet import ScaleNet, ScaleNetParams
from util.handdetector import HandDetector, refine_com_iterative


class _Value(object):
    """Stand-in for multiprocessing.Value: the reference reads and writes `.value`."""

    def __init__(self, value):
        self.value = value


class _NoHand(Exception):
    """seed_detect looked at a frame and found no hand (and there is no other seed): the frame is treated like a lost one."""


def smoothing_figures(raw, filtered):
    """Sanity figures of a filtered pose sequence against the raw one, both (ticks, J, 3) over the same ticks, in mm: the mean
    frame-to-frame displacement of the raw joints, that of the filtered joints, and the mean raw-to-filtered distance (NaN where
    there are too few ticks).  No accuracy claim: with untrained nets they only show that the filter ran."""
    raw, filtered = numpy.asarray(raw, numpy.float64), numpy.asarray(filtered, numpy.float64)

    def step(p):
        return float(numpy.sqrt((numpy.diff(p, axis=0) ** 2).sum(-1)).mean()) if len(p) > 1 else float('nan')
    dist = float(numpy.sqrt(((raw - filtered) ** 2).sum(-1)).mean()) if len(raw) else float('nan')
    return dict(raw_step=step(raw), filtered_step=step(filtered), distance=dist)


def _stamp_of(device, what):
    """The stamp of the frame `device` delivered last; a device that does not stamp its frames cannot feed a timed pipeline."""
    stamp = device.getTimestamp() if hasattr(device, 'getTimestamp') else None
    if stamp is None:
        raise ValueError("timing needs stamped frames: %s returns no timestamp (FileDevice: stamps=)" % what)
    return stamp


class _Tick(list):
    """One frame (or None) per device, with the frames' stamps where the pipeline is timed."""
    stamps = None


class RealtimeHandposePipeline(object):
    """Realtime pipeline for handpose estimation"""

    # states of pipeline
    STATE_IDLE = 0
    STATE_INIT = 1
    STATE_RUN = 2

    # different hands
    HAND_LEFT = 0
    HAND_RIGHT = 1

    # different detectors
    DETECTOR_COM = 0

    def __init__(self, poseNet, config, di, verbose=False, comrefNet=None, init_com=None, seed_com=False, seed_detect=False, sensor=None,
                 smooth=None, visibility=None, timing=False, background=None):
        """
        :param poseNet:   network for pose estimation (a built net, or PoseRegNetParams / ResNetParams, with loadFile or not)
        :param config:    dict(fx=, fy=, cube=(x, y, z)[, invX=, invY=])
        :param di:        depth importer
        :param comrefNet: refinement network of the hand centre (a built net or ScaleNetParams)
        :param init_com:  seed of the track, image coordinates (switches tracking on)
        :param seed_com:  NON-reference seed from the frame's own centre of mass (module docstring)
        :param seed_detect: seed, and re-seed after a lost frame, by connected-component detection on the device (switches tracking on;
                          takes precedence over seed_com)
        :param sensor:    None (frames are float32 mm), or dict(dtype='uint16' | 'float32', median=bool, mirror=bool): frames are raw
                          sensor frames, converted / mirrored / median-filtered on the device (module docstring)
        :param smooth:    None, or HandTracker's dict(rate=, mincutoff=, beta=[, dcutoff=, max_hold=]): processFrame's result gains the
                          One-Euro-filtered pose_f / pose_img_f and the filter's word `smooth` beside the raw keys, and processVideo
                          leaves the filtered poses of the frames it returns in `poses_f`
        :param visibility: None, or HandTracker's dict(radius=, margin=, min_support=[, hidden_weight=]): processFrame's result gains
                          `vis` (the share of the pixels around each joint that lie at its depth) and `vis_class` (ops.VIS_* per joint),
                          and processVideo leaves the classes of the frames it returns in `vis_classes`
        :param timing:    True (needs smooth): HandTracker's -- the filter runs over the frames' stamps: processFrame takes stamp=
                          (seconds) and processVideo reads device.getTimestamp() behind every frame (a device that returns None raises)
        :param background: None, or HandTracker's dict(margin=[, rel=, min_seen=]): a per-pixel background learned by learnBackground(device)
                          is removed from every frame on the device before the fused path (processFrame / processVideo /
                          calibrateHandsize) looks at it; the per-call API (detect) works on the host and does not see it
        """
        self.importer = di
        self.poseNet = poseNet
        self.comrefNet = comrefNet
        self.initialconfig = copy.deepcopy(config)
        self.sync = dict(config=config, fid=0, crop=numpy.ones((128, 128), dtype='float32'),
                         com3D=numpy.asarray([0, 0, 300], dtype='float32'), frame=numpy.ones((240, 320), dtype='float32'), M=numpy.eye(3))
        self.stop = _Value(False)
        self.verbose = verbose
        self.hand = _Value(self.HAND_LEFT)
        self.state = _Value(self.STATE_IDLE)
        self.detection = _Value(self.DETECTOR_COM)
        self.handsizes = []
        self.numinitframes = 50
        self.tracking = _Value(init_com is not None or bool(seed_com) or bool(seed_detect))
        self.init_com = None if init_com is None else numpy.asarray(init_com, numpy.float32).copy()
        self.seed_com = bool(seed_com)
        self.seed_detect = bool(seed_detect)
        self.lastcom = (0, 0, 0) if init_com is None else self.init_com.copy()
        self.show_pose = False
        self.show_crop = False
        self._tracker = None
        self.sensor = None if sensor is None else dict(sensor)
        self.smooth = None if smooth is None else dict(smooth)
        self.poses_f = None
        self.visibility = None if visibility is None else dict(visibility)
        self.vis_classes = None
        self.timing = bool(timing)
        if self.timing and smooth is None:
            raise ValueError("timing needs smooth: with one camera the stamps are read by the filter alone")
        self.background = None if background is None else dict(background)

    def initNets(self):
        """Build the nets from their parameters (loading loadFile where set) and compile their forward plans (:118-141)."""
        if isinstance(self.poseNet, PoseRegNetParams):
            self.poseNet = PoseRegNet(numpy.random.RandomState(23455), cfgParams=self.poseNet)
        elif isinstance(self.poseNet, ResNetParams):
            self.poseNet = ResNet(numpy.random.RandomState(23455), cfgParams=self.poseNet)
        elif not isinstance(self.poseNet, (PoseRegNet, ResNet)):
            raise RuntimeError("Unknown pose estimation method!")
        self.poseNet.setDeterministic()
        self.poseNet.computeOutput(numpy.zeros(self.poseNet.cfgParams.inputDim, dtype='float32'))
        if self.comrefNet is not None:
            if isinstance(self.comrefNet, ScaleNetParams):
                self.comrefNet = ScaleNet(numpy.random.RandomState(23455), cfgParams=self.comrefNet)
            elif not isinstance(self.comrefNet, ScaleNet):
                raise RuntimeError("Unknown refine method!")
            self.comrefNet.setDeterministic()
            dims = self.comrefNet.cfgParams.inputDim
            dims = dims if isinstance(dims[0], (list, tuple)) else [dims]
            ins = [numpy.zeros(sz, dtype='float32') for sz in dims]
            self.comrefNet.computeOutput(ins if len(ins) > 1 else ins[0])

    # ---- sizes ------------------------------------------------------------------------------------------------------------
    def _pose_dsize(self):
        d = self.poseNet.cfgParams.inputDim
        return (int(d[2]), int(d[3]))

    def _refine_dsize(self):
        dims = self.comrefNet.cfgParams.inputDim
        d0 = dims[0] if isinstance(dims[0], (list, tuple)) else dims
        return (int(d0[2]), int(d0[3]))

    def _filtered(self, frame):
        """The float32 frame the per-call paths work on: a raw sensor frame through filter_depth, anything else as float32."""
        if self.sensor is None:
            return numpy.asarray(frame, numpy.float32)
        from hipdp import ops
        from util.cameradevice import filter_depth
        dt, median, mirror = ops.sensor_spec(self.sensor)
        frame = numpy.asarray(frame)
        if frame.dtype != dt:
            raise ValueError("frame dtype %s, the pipeline's sensor delivers %s" % (frame.dtype, dt))
        return filter_depth(frame, median=median, mirror=mirror)

    def _seed(self, frame, filtered=False):
        """The NON-reference seed: whole-frame centre of mass + refineCoMIterative(com, 5, cube).  filtered: `frame` has been through
        _filtered already."""
        frame = numpy.asarray(frame, numpy.float32) if filtered else self._filtered(frame)
        cfg = self.sync['config']
        hd = HandDetector(numpy.asarray(frame, numpy.float32).copy(), cfg['fx'], cfg['fy'], importer=self.importer)
        com = hd.calculateCoM(hd.dpt)
        if numpy.allclose(com, 0.):
            return numpy.zeros(3, numpy.float32)
        cube = numpy.asarray(cfg['cube'], numpy.float32)
        return refine_com_iterative(numpy.asarray(frame, numpy.float32)[None], com[None], cube[None], cfg['fx'], cfg['fy'], 5)[0]

    def _detect_seed(self, frame, filtered=False):
        """seed_detect for the per-call API: HandDetector.detectComponents' centre (doHandSize=False), zeros where there is no hand."""
        from util.handdetector import find_hands
        frame = numpy.asarray(frame, numpy.float32) if filtered else self._filtered(frame)
        cfg = self.sync['config']
        coms, _, found = find_hands(numpy.asarray(frame, numpy.float32)[None], numpy.asarray(cfg['cube'], numpy.float32)[None], cfg['fx'], cfg['fy'])
        return coms[0] if found[0] else numpy.zeros(3, numpy.float32)

    def _need_seed(self, frame, detect_tried=False, filtered=False):
        """The centre to track from, seeding it where there is none; without a seed: HandDetector.detect's NotImplementedError.
        filtered: `frame` is the float32 frame _filtered returned (detect has it already), not a raw sensor frame."""
        if self.state.value == self.STATE_INIT:
            raise NotImplementedError("hand-size calibration (STATE_INIT: estimateHandsize from cv2.findContours) is not built")
        if self.tracking.value and not numpy.allclose(self.lastcom, 0):
            return numpy.asarray(self.lastcom, numpy.float32)
        if self.tracking.value and self.seed_detect and not detect_tried:
            com = self._detect_seed(frame, filtered)
            if not numpy.isclose(com[2], 0.):
                return com
        if self.tracking.value and self.seed_com:
            com = self._seed(frame, filtered)
            if not numpy.isclose(com[2], 0.):
                return com
        if self.tracking.value and self.seed_detect:
            raise _NoHand()                            # nothing in view: not an error, the next frame is looked at again
        cfg = self.sync['config']
        return HandDetector(numpy.zeros((2, 2), numpy.float32), cfg['fx'], cfg['fy']).detect(size=cfg['cube'], doHandSize=False)

    # ---- the reference's per-call API ---------------------------------------------------------------------------------------
    def detect(self, frame):
        """Follow the hand into `frame` (:296-337, tracking mode): (normalised crop, transformation M, com3D)."""
        cfg = self.sync['config']
        if self.sensor is not None:                    # filtered ONCE: the seeds below get the same float32 frame
            frame = self._filtered(frame)
        try:
            lastcom = self._need_seed(frame, filtered=self.sensor is not None)
        except _NoHand:                                # the answer of :326-327, as for a lost track
            self.lastcom = (0, 0, 0)
            self.handsizes = []
            return numpy.zeros(self._pose_dsize()[::-1], dtype='float32'), numpy.eye(3), numpy.zeros(3, numpy.float32)
        hd = HandDetector(frame, cfg['fx'], cfg['fy'], importer=self.importer, refineNet=self.comrefNet)
        loc, handsz = hd.track(lastcom, cfg['cube'], dsize=self._refine_dsize(), doHandSize=False)
        self.lastcom = loc
        self.handsizes = []
        if numpy.allclose(loc, 0) or numpy.isclose(loc[2], 0.):
            self.lastcom = (0, 0, 0)                   # lost (module docstring)
            return numpy.zeros(self._pose_dsize()[::-1], dtype='float32'), numpy.eye(3), numpy.zeros(3, numpy.float32)
        crop, M, com = hd.cropArea3D(com=loc, size=cfg['cube'], dsize=self._pose_dsize())
        com3D = self.importer.jointImgTo3D(com)
        sc = (cfg['cube'][2] / 2.)
        crop[crop == 0] = com3D[2] + sc
        crop.clip(com3D[2] - sc, com3D[2] + sc)        # (the reference discards this result as well, :334)
        crop -= com3D[2]
        crop /= sc
        return crop, M, com3D

    def estimatePose(self, crop, com3D):
        """Estimate the hand pose (:339-370): normalised joint positions (J, 3); the caller forms pose * cube[2] / 2. + com3D."""
        if self.hand.value == self.HAND_LEFT:
            inp = crop[None, None, :, :].astype('float32')
        else:
            inp = crop[None, None, :, ::-1].astype('float32')
        jts = self.poseNet.computeOutput(numpy.ascontiguousarray(inp))
        jj = jts[0].reshape((-1, 3))
        cfg = self.sync['config']
        if 'invX' in cfg:
            if cfg['invX'] is True:
                jj[:, 1] *= (-1.)
        if 'invY' in cfg:
            if cfg['invY'] is True:
                jj[:, 0] *= (-1.)
        if self.hand.value == self.HAND_RIGHT:
            jj[:, 0] *= (-1.)
        return jj

    # ---- the fused path -----------------------------------------------------------------------------------------------------
    def tracker(self, H, W):
        """The device tracker for H x W frames, its state brought in line with the pipeline's (cube, hand, invX / invY)."""
        from hipdp.runtime import default_runtime
        from hipdp.tracker import HandTracker
        cfg = self.sync['config']
        t = self._tracker
        if t is None or (t.H, t.W) != (H, W) or (t.fx, t.fy) != (abs(float(cfg['fx'])), abs(float(cfg['fy']))):
            t = self._tracker = HandTracker(default_runtime(), self.importer, self.poseNet, self.comrefNet, H, W, cfg['cube'],
                                            fx=cfg['fx'], fy=cfg['fy'], sensor=self.sensor, smooth=self.smooth,
                                            visibility=self.visibility, timing=self.timing, background=self.background)
        if tuple(numpy.float32(cfg['cube'])) != tuple(t.cube_host):
            t.set_cube(cfg['cube'])
        t.set_hand(self.hand.value == self.HAND_RIGHT)
        t.set_inv(cfg.get('invX') is True, cfg.get('invY') is True)
        return t

    def _no_hand_result(self):
        """What processFrame answers for a frame in which seed_detect finds no hand: the shape of a LOST frame's result (status 1,
        zeros, M = identity); the pipeline keeps no centre, so the next frame is searched again."""
        from hipdp import ops
        J = self.poseNet.cfgParams.outputDim[1] // 3
        self.lastcom = (0, 0, 0)
        self._devcom = self.lastcom
        z3 = numpy.zeros(3, numpy.float32)
        self.sync.update(fid=self.sync['fid'] + 1, com3D=z3, M=numpy.eye(3, dtype=numpy.float32))
        res = dict(pose=numpy.zeros((J, 3), numpy.float32), pose_img=numpy.zeros((J, 3), numpy.float32), com=z3.copy(), com3D=z3.copy(),
                   M=numpy.eye(3, dtype=numpy.float32), status=1)
        if self.smooth is not None:                    # nothing ran: nothing was filtered
            res.update(pose_f=numpy.zeros((J, 3), numpy.float32), pose_img_f=numpy.zeros((J, 3), numpy.float32), smooth=ops.SMOOTH_EMPTY)
        if self.visibility is not None:                # nothing ran: the zeros of a row that is not OK
            res.update(vis=numpy.zeros(J, numpy.float32), vis_class=numpy.zeros(J, numpy.int32))
        return res

    def processFrame(self, frame, stamp=None):
        """detect + estimatePose + the de-normalisation of one frame as ONE device plan: the tracker's result dict (pose in mm).  With
        `timing`, stamp is the frame's time in seconds."""
        if self.timing and stamp is None:
            raise ValueError("a pipeline with timing needs every frame's stamp")
        frame = numpy.asarray(frame, numpy.float32) if self.sensor is None else numpy.asarray(frame)     # (a raw frame: the tracker checks its dtype)
        acquiring = self.seed_detect and self.tracking.value and self.state.value != self.STATE_INIT and numpy.allclose(self.lastcom, 0)
        if acquiring:                                  # the centre goes from the detector plan into the tracker's state on the device
            acq = self.tracker(*frame.shape).acquire(frame)
            if acq['found']:
                self.lastcom = acq['com'].copy()
                self._devcom = self.lastcom
        try:
            lastcom = self._need_seed(frame, detect_tried=acquiring)
        except _NoHand:
            return self._no_hand_result()
        t = self.tracker(*frame.shape)
        if t.lost or not numpy.array_equal(numpy.asarray(lastcom, numpy.float32), numpy.asarray(getattr(self, '_devcom', (0, 0, 0)), numpy.float32)):
            t.reset(lastcom)                           # the host's centre changed behind the device's back (seed, reset, detect())
        res = t.process(frame, stamp=stamp) if self.timing else t.process(frame)
        self.lastcom = (0, 0, 0) if res['status'] else res['com'].copy()
        self._devcom = self.lastcom
        self.sync.update(fid=self.sync['fid'] + 1, com3D=res['com3D'], M=res['M'])
        return res

    def processVideo(self, device, max_frames=None):
        """Headless processVideo (:235-294): every frame of `device` through the fused plan; returns the poses in mm, (frames, J, 3).
        Stops at the end of a FileDevice, after max_frames, on `q`, or at a lost track (whose frame is not returned); with seed_detect
        a lost frame, or one in which no hand is found, is skipped instead and the next frame is searched again."""
        self.initNets()
        device.start()
        poses, poses_f, vis_classes = [], [], []
        times = []
        while not self.stop.value and (max_frames is None or len(poses) < max_frames):
            try:
                ret, frame = device.getDepth()
            except IndexError:
                break
            if ret is False:
                print("Error while reading frame.")
                break
            stamp = _stamp_of(device, 'the device') if self.timing else None
            start = time.time()
            res = self.processFrame(frame, stamp) if self.timing else self.processFrame(frame)
            times.append(time.time() - start)
            if res['status']:
                print("Track lost (or no hand) in frame {}.".format(len(times) - 1))
                if self.seed_detect:
                    continue
                break
            poses.append(res['pose'].copy())
            if self.smooth is not None:
                poses_f.append(res['pose_f'].copy())
            if self.visibility is not None:
                vis_classes.append(res['vis_class'].copy())
            if self.verbose is True:
                print("{}ms frame".format(times[-1] * 1000.))
        device.stop()
        self.frame_times = times
        J = self.poseNet.cfgParams.outputDim[1] // 3
        self.poses_f = None if self.smooth is None else numpy.asarray(poses_f, numpy.float32).reshape(-1, J, 3)
        self.vis_classes = None if self.visibility is None else numpy.asarray(vis_classes, numpy.int32).reshape(-1, J)
        return numpy.asarray(poses, numpy.float32).reshape(-1, J, 3)

    def learnBackground(self, device, frames=None):
        """Headless, like calibrateHandsize: `frames` (default numinitframes) frames of `device`, showing the scene WITHOUT the hand,
        into the tracker's background model (raw frames with a sensor).  Raises RuntimeError if the device runs out of frames first.
        Returns the model, dict(near, seen, cut); tracker(H, W).set_background_model() of a later run takes it.  (A tracker for another
        frame size or other fx / fy is a new tracker: it starts without a model.)"""
        if self.background is None:
            raise RuntimeError("the pipeline was built without background=")
        n = self.numinitframes if frames is None else int(frames)
        self.initNets()
        device.start()
        t = None
        for i in range(n):
            try:
                ret, frame = device.getDepth()
            except IndexError:
                ret = False
            if ret is False:
                device.stop()
                raise RuntimeError("the device ran out of frames after %d of %d" % (i, n))
            frame = numpy.asarray(frame, numpy.float32) if self.sensor is None else numpy.asarray(frame)
            t = self.tracker(*frame.shape)
            t.learn_background(frame)
        device.stop()
        return None if t is None else t.background_model()

    def calibrateHandsize(self, device, num_frames=None):
        """Headless hand-size calibration, the counterpart of STATE_INIT (:312-324): `num_frames` (default numinitframes) frames of
        `device`; for each the component hand size (HandDetector.estimateHandsizeComponents, on the device) around the centre the
        detector acquires or, once there is one, the tracker follows; config['cube'] becomes the `int` median and the state
        STATE_RUN.  A frame without a hand, or whose track is lost, contributes the current cube, as detect's no-hand return does.
        Returns the new cube.  (processKey(ord('i')), the reference's cv2-contour calibration, stays not built.)"""
        n = self.numinitframes if num_frames is None else int(num_frames)
        self.initNets()
        device.start()
        self.handsizes = []
        while len(self.handsizes) < n:
            ret, frame = device.getDepth()
            if ret is False:
                raise RuntimeError("Error while reading frame.")
            frame = numpy.asarray(frame, numpy.float32) if self.sensor is None else numpy.asarray(frame)
            cfg = self.sync['config']
            t = self.tracker(*frame.shape)
            handsz = numpy.asarray(cfg['cube'], numpy.float32)
            if numpy.allclose(self.lastcom, 0):
                acq = t.acquire(frame, do_hand_size=True)
                if acq['found']:
                    handsz = acq['cube']
                    self.lastcom = acq['com'].copy()
                    self._devcom = self.lastcom
            elif not self.processFrame(frame)['status']:
                handsz = t.hand_size()
            self.handsizes.append(tuple(float(c) for c in handsz))
            if self.verbose is True:
                print(numpy.median(numpy.asarray(self.handsizes), axis=0))
        device.stop()
        cfg = self.sync['config']
        cfg['cube'] = tuple(int(c) for c in numpy.median(numpy.asarray(self.handsizes), axis=0).astype('int'))
        self.sync.update(config=cfg)
        self.state.value = self.STATE_RUN
        self.handsizes = []
        return cfg['cube']

    # ---- state ------------------------------------------------------------------------------------------------------------
    def processKey(self, key):
        """The state changes of the reference's keys (:493-525); `s` toggles flags that only its cv2 windows read."""
        if key == ord('q'):
            self.stop.value = True
        elif key == ord('h'):
            self.hand.value = self.HAND_RIGHT if self.hand.value == self.HAND_LEFT else self.HAND_LEFT
        elif key == ord('+'):
            cfg = self.sync['config']
            cfg['cube'] = tuple([lst + 10 for lst in list(cfg['cube'])])
            self.sync.update(config=cfg)
        elif key == ord('-'):
            cfg = self.sync['config']
            cfg['cube'] = tuple([lst - 10 for lst in list(cfg['cube'])])
            self.sync.update(config=cfg)
        elif key == ord('r'):
            self.reset()
        elif key == ord('i'):
            raise NotImplementedError("hand-size calibration (STATE_INIT: estimateHandsize from cv2.findContours) is not built")
        elif key == ord('t'):
            self.tracking.value = not self.tracking.value
        elif key == ord('s'):
            self.show_crop = not self.show_crop
            self.show_pose = not self.show_pose

    def reset(self):
        """Reset stateful parts (:527-536); the track starts again from init_com (or needs a new seed)."""
        self.state.value = self.STATE_IDLE
        self.sync.update(config=copy.deepcopy(self.initialconfig))
        self.detection.value = self.DETECTOR_COM
        self.lastcom = (0, 0, 0) if self.init_com is None else self.init_com.copy()


class MultiStreamPipeline(object):
    """Several cameras and hands through ONE device plan per tick (hipdp.multitrack.MultiTracker): the headless processVideo of
    RealtimeHandposePipeline for a list of CameraDevices.  `hands` names the tracks, one (device index, hand) each with hand
    HAND_LEFT / HAND_RIGHT: N cameras with one hand each, both hands of one camera, or a mixture.  Both nets are built for a batch
    of len(hands).  The devices may be unlike cameras: `di` is one importer for all devices or a list with one per device, config['fx'] /
    ['fy'] may be lists with one value per device, and every device may deliver frames of a size of its own (the tracker is built for
    the devices' frame shapes as they are first seen; MultiTracker keeps unlike sources in one plan through a per-source table).

    Seeds: init_com= one centre per track (image coordinates of its device, z in mm; None for a track without one), and / or
    seed_detect=True: a track without a centre -- never seeded, or lost -- is searched for in its device's next frame by the
    component detector, as RealtimeHandposePipeline's _need_seed does after a lost frame: ONE detector plan per device with lost
    tracks (MultiTracker.acquire_source) finds as many hands as the device has tracks and shares them out -- followed tracks keep
    theirs, the lost ones take the rest, nearest first -- so both hands of one camera start, and come back, without an init_com.
    max_extent (mm) keeps things larger than a hand (a wall behind one hand) from being taken for the second.

    Fusion (this project's own; hipdp/multitrack.py): with config['extrinsics'] -- one (R, t) per device, camera frame to world, mm --
    and groups= (lists of tracks that observe the same hand from different devices) every tick also fuses each group: processFrames'
    results carry MultiTracker's group / outlier / disagree / handed / peer_com per grouped track, `fused` holds the last tick's
    dict(pose, com, spread, n) per group, and processVideos leaves in `fused_poses` one (ticks, J, 3) array per group of the fused
    poses (world frame, mm) of the ticks in which at least one of its tracks was followed.  A grouped track that loses the hand is
    handed its peers' centre instead of waiting for a detection.

    Calibration (hipdp/multitrack.py, CALIBRATION): with calibrate=dict(anchor=, max_shape_dev=, min_cond=) config['extrinsics'] may
    hold None for devices whose pose nobody has measured; calibrateExtrinsics(ticks) finds them from the tracked hand itself.  Until
    then nothing is fused: `fused` is [].

    Smoothing (hipdp/multitrack.py, SMOOTHING): smooth=dict(rate=, mincutoff=, beta=[, dcutoff=, max_hold=]) goes to MultiTracker: the
    results carry pose_f / pose_img_f / smooth beside the raw keys, `fused` pose_f / smooth, and processVideos leaves in `poses_f` /
    `fused_poses_f` the filtered poses of exactly the ticks that its return value / `fused_poses` hold.

    Visibility (hipdp/multitrack.py, VISIBILITY): visibility=dict(radius=, margin=, min_support=[, hidden_weight=]) goes to MultiTracker:
    the results carry vis / vis_class per joint, the fusion is weighted by them, `fused` carries `weight`, and processVideos leaves
    in `vis_classes` the classes of exactly the ticks that its return value holds.

    Timing (hipdp/multitrack.py, TIMING): timing=dict(max_gap=, max_lead=) goes to MultiTracker: every tick carries the stamps that the
    devices report for their frames (CameraDevice.getTimestamp(); a device that returns None for a delivered frame raises), `now` is
    the latest of them, the results carry pose_t / pose_img_t / com3D_t / lead / align, `fused` refers to `now`, and processVideos
    leaves in `poses_t` the aligned poses of exactly the ticks that its return value holds."""

    HAND_LEFT, HAND_RIGHT = RealtimeHandposePipeline.HAND_LEFT, RealtimeHandposePipeline.HAND_RIGHT

    def __init__(self, poseNet, config, di, devices, hands, comrefNet, init_com=None, seed_detect=False, sensor=None, verbose=False,
                 max_extent=None, groups=None, max_dev=None, handover=True, calibrate=None, smooth=None, visibility=None, timing=None,
                 background=None):
        """
        :param poseNet, comrefNet: built nets or their parameters (as for RealtimeHandposePipeline), with batchSize == len(hands)
        :param config:    dict(fx=, fy=, cube=(x, y, z)[, invX=, invY=]); fx / fy: one value, or a list with one per device
        :param di:        depth importer (the one camera of all devices), or a list with one importer per device
        :param devices:   list of CameraDevice
        :param hands:     list of (device index, HAND_LEFT | HAND_RIGHT), one per track
        :param init_com:  None, or one centre (or None) per track
        :param seed_detect: acquire tracks without a centre by detection, again after they are lost
        :param sensor:    as for RealtimeHandposePipeline, for all devices
        :param max_extent: None, or the largest metric width / height (mm) of a component that seed_detect may take for a hand
        :param groups, max_dev, handover: MultiTracker's, with config['extrinsics'] (one (R, t) per device)
        :param calibrate: MultiTracker's: entries of config['extrinsics'] may then be None, to be found by calibrateExtrinsics
        :param smooth:    MultiTracker's: the One-Euro filter over the tracked and the fused poses
        :param visibility: MultiTracker's: every joint classified by the frame around it, the fusion weighted by that
        :param timing:    MultiTracker's: the devices' stamps carried through the plan, every track brought to the tick's instant
        :param background: MultiTracker's, for all devices: the per-pixel background learnBackground(ticks) learned is removed from every frame
        """
        self.background = None if background is None else dict(background)
        self.timing = None if timing is None else dict(timing)
        self.poses_t = None
        self.visibility = None if visibility is None else dict(visibility)
        self.vis_classes = None
        self.smooth = None if smooth is None else dict(smooth)
        self.poses_f, self.fused_poses_f = None, None
        self.max_extent = max_extent
        self.groups, self.max_dev, self.handover, self.calibrate = groups, max_dev, handover, calibrate
        self.fused, self.fused_poses = [], []
        self.config = copy.deepcopy(config)
        self.devices = list(devices)
        self.importers = list(di) if isinstance(di, (list, tuple)) else [di] * len(self.devices)
        if len(self.importers) != len(self.devices):
            raise ValueError("%d importers for %d devices" % (len(self.importers), len(self.devices)))
        self.poseNet, self.comrefNet, self.importer = poseNet, comrefNet, self.importers[0]
        self.hands = [(int(d), int(h)) for d, h in hands]
        if not self.hands or not self.devices:
            raise ValueError("MultiStreamPipeline needs at least one device and one track")
        if sorted(set(d for d, _ in self.hands)) != list(range(len(self.devices))):
            raise ValueError("every device needs a track, every track a device: %d devices, tracks on %r"
                             % (len(self.devices), sorted(set(d for d, _ in self.hands))))
        init_com = [None] * len(self.hands) if init_com is None else list(init_com)
        if len(init_com) != len(self.hands):
            raise ValueError("init_com has one entry per track")
        self.init_com = [None if c is None else numpy.asarray(c, numpy.float32).copy() for c in init_com]
        self.seed_detect = bool(seed_detect)
        if not self.seed_detect and any(c is None for c in self.init_com):
            raise ValueError("a track without init_com needs seed_detect=True")
        self.sensor = None if sensor is None else dict(sensor)
        self.verbose = verbose
        self.stop = _Value(False)
        self._tracker = None
        self._shapes = [None] * len(self.devices)                      # every device's frame shape, as first seen
        self._seeded = [False] * len(self.hands)

    def initNets(self):
        """Build the nets from their parameters and compile their forward plans: RealtimeHandposePipeline.initNets, at batch len(hands)."""
        one = RealtimeHandposePipeline(self.poseNet, self.config, self.importer, comrefNet=self.comrefNet)
        one.initNets()
        self.poseNet, self.comrefNet = one.poseNet, one.comrefNet

    def tracker(self, H, W=None):
        """The tracker for the devices' frame shapes: H a list with one (H, W) per device, or (H, W) the one shape of all devices."""
        from hipdp.multitrack import MultiTracker
        from hipdp.runtime import default_runtime
        shapes = tuple((int(h), int(w)) for h, w in H) if W is None else ((int(H), int(W)),) * len(self.devices)
        if self._tracker is None or self._tracker_key != shapes:
            cfg = self.config
            same = len(set(shapes)) == 1 and all(di is self.importer for di in self.importers)
            self._tracker = MultiTracker(default_runtime(), self.importer if same else self.importers, self.poseNet, self.comrefNet,
                                         shapes[0][0] if same else [s[0] for s in shapes], shapes[0][1] if same else [s[1] for s in shapes],
                                         cfg['cube'], [(d, h == self.HAND_RIGHT) for d, h in self.hands], sources=len(self.devices),
                                         invX=cfg.get('invX') is True, invY=cfg.get('invY') is True, fx=cfg['fx'], fy=cfg['fy'],
                                         sensor=self.sensor, extrinsics=cfg.get('extrinsics'), groups=self.groups, max_dev=self.max_dev,
                                         handover=self.handover, calibrate=self.calibrate, smooth=self.smooth,
                                         visibility=self.visibility, timing=self.timing, background=self.background)
            self._tracker_key = shapes
            self._seeded = [False] * len(self.hands)
        return self._tracker

    def _tracker_for(self, frames):
        """The tracker keyed by the tuple of the devices' frame shapes; a device that has not delivered yet counts with the shape of
        the first device that has (devices of one kind are the common case)."""
        for d, f in enumerate(frames):
            if f is not None and self._shapes[d] is None:
                self._shapes[d] = tuple(numpy.asarray(f).shape)
        first = next(s for s in self._shapes if s is not None)
        return self.tracker([first if s is None else s for s in self._shapes])

    def _to_seed(self, mt, frames):
        """The tracks that processFrames would seed before this tick (from init_com or by detection)."""
        return [t for t, (d, _) in enumerate(self.hands) if mt.lost[t] and frames[d] is not None and
                ((not self._seeded[t] and self.init_com[t] is not None) or self.seed_detect)]

    def _stamps_for(self, frames, stamps):
        """A timed tick's stamps: those given, else the ones _read() took from the devices with these frames."""
        if self.timing is None:
            if stamps is not None:
                raise ValueError("stamps need a pipeline with timing=")
            return None
        stamps = getattr(frames, 'stamps', None) if stamps is None else stamps
        if stamps is None:
            raise ValueError("a pipeline with timing needs one stamp per frame")
        return stamps

    def processFrames(self, frames, stamps=None):
        """One tick: one frame (or None) per device -> one result dict per track (MultiTracker.process).  Tracks without a centre are
        seeded first: from init_com once, else (seed_detect) by detection in their device's frame -- one detector plan per device
        for all its lost tracks.  With `timing`: stamps has one time (s) per frame (default: what the devices reported when _read()
        fetched these frames)."""
        stamps = self._stamps_for(frames, stamps)
        mt = self._tracker_for(frames)
        search = set()
        for t, (d, _) in enumerate(self.hands):
            if not mt.lost[t] or frames[d] is None:
                continue
            if not self._seeded[t] and self.init_com[t] is not None:
                mt.reset(t, self.init_com[t])
            elif self.seed_detect:
                search.add(d)
            self._seeded[t] = True
        for d in sorted(search):
            mt.acquire_source(d, frames[d], max_extent=self.max_extent)
        res = mt.process(frames) if stamps is None else mt.process(frames, stamps=stamps)
        self.fused = mt.fused
        return res

    def learnBackground(self, ticks):
        """`ticks` ticks of the devices, showing the scene WITHOUT hands, into the tracker's per-device background models (a device that
        delivers no frame in a tick sits that tick out).  Raises RuntimeError if the devices run out of frames first.  Returns the models,
        one dict(near, seen, cut) per device."""
        if self.background is None:
            raise RuntimeError("the pipeline was built without background=")
        self.initNets()
        for dev in self.devices:
            dev.start()
        for i in range(int(ticks)):
            frames = self._read()
            if frames is None:
                for dev in self.devices:
                    dev.stop()
                raise RuntimeError("the devices ran out of frames after %d of %d ticks" % (i, int(ticks)))
            self._tracker_for(frames).learn_background(list(frames))
        for dev in self.devices:
            dev.stop()
        return None if self._tracker is None else self._tracker.background_model()

    def calibrateExtrinsics(self, ticks):
        """Find the extrinsics that config['extrinsics'] leaves open (None entries; calibrate=) from the hand the devices see: `ticks`
        ticks from the devices through processFrames -- each adds its joint pairs to the sums on the device -- then
        MultiTracker.finish_calibration().  Returns its report, {device: dict(R, t, n, pairs, refused, rms, cond, ok)}.  Where every fit
        is ok the pipeline fuses from the next tick on (and config['extrinsics'] holds the fits); otherwise nothing has changed but
        the sums, and calling this again goes on from them."""
        self.initNets()
        for dev in self.devices:
            dev.start()
        for _ in range(int(ticks)):
            frames = self._read()
            if frames is None:
                break
            self.processFrames(frames)
        for dev in self.devices:
            dev.stop()
        if self._tracker is None or not self._tracker.calibrating:
            raise RuntimeError("nothing to calibrate: no frame was read, or config['extrinsics'] leaves no device open")
        report = self._tracker.finish_calibration()
        if not self._tracker.calibrating:
            ext = self._tracker.rig.extr_host
            self.config['extrinsics'] = [(ext[c, :9].reshape(3, 3).copy(), ext[c, 9:].copy()) for c in range(len(self.devices))]
        return report

    def _read(self):
        """One frame (or None) per device; None when a FileDevice has ended or no device delivered."""
        frames = _Tick()
        try:
            for dev in self.devices:
                ret, frame = dev.getDepth()
                frames.append(frame if ret is not False else None)
        except IndexError:
            return None
        if self.timing is not None:
            frames.stamps = [None if f is None else _stamp_of(dev, 'device %d' % d) for d, (dev, f) in enumerate(zip(self.devices, frames))]
        if all(f is None for f in frames):
            print("Error while reading frames.")
            return None
        return frames

    def processVideos(self, max_frames=None, overlapped=False):
        """Every tick one frame of every device through one plan, until a FileDevice ends, max_frames ticks, `stop`, or -- without
        seed_detect -- every track is lost.  Returns one (ticks followed, J, 3) float32 array of poses in mm per track: a tick in
        which a track is lost or idle is left out of that track's list.

        overlapped=True: stretches of ticks in which no track needs a seed go through MultiTracker.process_sequence (the uploads of
        the next tick under the plan of this one, the results read one tick late); a tick in which a track is to be seeded -- the
        first one, or after the host has learnt that a track was lost, with seed_detect -- is an ordinary tick.  The poses of the
        followed ticks are the same either way; frame_times then holds a stretch's mean for each of its ticks."""
        self.initNets()
        for dev in self.devices:
            dev.start()
        poses = [[] for _ in self.hands]
        times = []
        state = dict(ticks=0, carry=None, ended=False)

        def go_on():
            return not self.stop.value and (max_frames is None or state['ticks'] < max_frames) and not state['ended']

        fused_poses = [[] for _ in (self.groups or [])]
        poses_f, fused_poses_f = [[] for _ in self.hands], [[] for _ in (self.groups or [])]
        vis_classes, poses_t = [[] for _ in self.hands], [[] for _ in self.hands]

        def collect(res, tick, fused):
            for g, f in enumerate(fused):
                if f['n'] > 0:
                    fused_poses[g].append(f['pose'].copy())
                    if self.smooth is not None:
                        fused_poses_f[g].append(f['pose_f'].copy())
            for t, r in enumerate(res):
                if r['status'] == 0:
                    poses[t].append(r['pose'].copy())
                    if self.smooth is not None:
                        poses_f[t].append(r['pose_f'].copy())
                    if self.visibility is not None:
                        vis_classes[t].append(r['vis_class'].copy())
                    if self.timing is not None:
                        poses_t[t].append(r['pose_t'].copy())
                elif r['status'] == 1:
                    print("Track {} lost (or no hand) in tick {}.".format(t, tick))

        def stretch(mt):
            """The ticks handed to process_sequence: until the input ends or the host knows of a track to seed (that tick is carried
            over to the tick loop)."""
            while go_on():
                if not self.seed_detect and all(mt.lost):
                    return
                frames = self._read()
                if frames is None:
                    state['ended'] = True
                    return
                if self._to_seed(mt, frames) or self._tracker_for(frames) is not mt:
                    state['carry'] = frames
                    return
                state['ticks'] += 1
                yield frames if self.timing is None else (list(frames), frames.stamps)
        while go_on():
            frames, state['carry'] = (state['carry'], None) if state['carry'] is not None else (self._read(), None)
            if frames is None:
                break
            start = time.time()
            res = self.processFrames(frames)
            times.append(time.time() - start)
            collect(res, state['ticks'], self.fused)
            state['ticks'] += 1
            if not self.seed_detect and all(self._tracker.lost):
                break
            if self.verbose is True:
                print("{}ms tick".format(times[-1] * 1000.))
            if overlapped and go_on():
                first, start = state['ticks'], time.time()
                out = self._tracker.process_sequence(stretch(self._tracker))
                for i, res in enumerate(out):
                    collect(res, first + i, self._tracker.fused_ticks[i])
                self.fused = self._tracker.fused
                times.extend([(time.time() - start) / max(1, len(out))] * len(out))
                if not self.seed_detect and all(self._tracker.lost):
                    break
        for dev in self.devices:
            dev.stop()
        self.frame_times = times
        J = self.poseNet.cfgParams.outputDim[1] // 3
        self.fused_poses = [numpy.asarray(p, numpy.float32).reshape(-1, J, 3) for p in fused_poses]
        if self.smooth is not None:
            self.poses_f = [numpy.asarray(p, numpy.float32).reshape(-1, J, 3) for p in poses_f]
            self.fused_poses_f = [numpy.asarray(p, numpy.float32).reshape(-1, J, 3) for p in fused_poses_f]
        if self.visibility is not None:
            self.vis_classes = [numpy.asarray(c, numpy.int32).reshape(-1, J) for c in vis_classes]
        if self.timing is not None:
            self.poses_t = [numpy.asarray(p, numpy.float32).reshape(-1, J, 3) for p in poses_t]
        return [numpy.asarray(p, numpy.float32).reshape(-1, J, 3) for p in poses]
