"""
Realtime tracking on the device: a depth frame in, the followed hand's 3-D joints out, ONE launch plan per frame.

What the reference does per frame on the host in tracking mode (/root/reference/src/util/realtimehandposepipeline.py:296-370,
/root/reference/src/util/handdetector.py:504-544) -- HandDetector(frame), track(lastcom, cube, doHandSize=False),
cropArea3D(com=loc), the normalisation of :332-336, estimatePose and pose * cube_z / 2 + com3D -- is here

    frame_range                                   the frame's depth range, many workgroups, the ONE pass over the whole frame
    crop_prepare_ranged(lastcom, stretch)         track's window: getCrop + resizeCrop(cropped, dsize), handdetector.py:512-519
    crop_warp(normalised) -> crop_center x2       refineCoM's three inputs, :634-669
    the refinement net's forward plan
    track_refine                                  com' = joint3DToImg(out * cube_z/2 + jointImgTo3D(lastcom)), fallback, status; the
                                                  final crop's record, M and com3D; lastcom := com' (device state, in place)
    crop_warp_ex(normalised[, flipped])           cropArea3D(com=loc) + :332-336 (+ crop[:, ::-1] for HAND_RIGHT, :351)
    the pose net's forward plan
    pose_finish                                   the sign rules of :356-369, pose * cube_z / 2. + com3D (:198), joints3DToImg (:407)

track() has no calculateCoM re-centring: this is hipdp/cascade.py's chain minus crop_com.  Tracking is sequential (frame t is
cropped around the centre found in frame t - 1), so the centre never leaves the device between frames: the host uploads a frame,
runs the plan and downloads one small result block.

ACQUIRING the hand.  The plan above follows a hand from a centre somebody supplied.  acquire(frame) finds one: the detector plan of
hipdp/detect.py (connected components: the nearest object of more than 200 px, its window's centre of mass, refineCoMIterative(5))
runs on the tracker's own frame buffer and depth-range partials and writes its centre straight into the device state; the host
reads back the tracker's one result block (centre, seed, cube, found).  A process(frame) that follows gives the bits of reset(that centre) + process(frame).

LOST frames.  Where the refined centre's depth is numpy.isclose to 0 the reference takes comToBounds' "CoM ill-defined" branch
(handdetector.py:204-213) and crops the MIDDLE of the frame; no device kernel implements that branch.  track_refine flags such a
frame instead (status 1), gives it an empty crop window (an all-zero net input, finite outputs), and the tracker refuses further
frames until reset(com) or a successful acquire(frame).

SENSOR frames.  HandTracker(..., sensor=dict(dtype='uint16' | 'float32', median=bool, mirror=bool)) takes frames as a depth sensor
delivers them: the host uploads the RAW frame (half the bytes for uint16) and the plan starts with frame_ingest (csrc/ingest.hip:
mirror, 3x3 median with a replicated border, conversion to float32 -- what the reference's CreativeCameraDevice.getDepth does on the
host, src/util/cameradevice.py:189-200 of the reference) IN PLACE OF frame_range: it writes the float32 frame buffer everything
downstream reads and the same depth-range partials, so the launch count does not change.  sensor=None is the plan above, untouched.

BACKGROUND.  On a fixed camera a desk edge, a monitor or the user's torso is nearer than the hand: the detector starts from it, the
depth range feeds its slabs, the crop keeps what lies inside the cube.  HandTracker(..., background=dict(margin=, rel=0.0,
min_seen=1)) keeps a per-pixel model of the empty scene on the device -- near (the smallest non-zero depth seen while learning) and
seen (the learning frames with a depth) -- and from it a cut map, computed on the host once per model change: near - (margin + rel *
near) in float32 where seen >= min_seen, near != 0 and the result is > 0, +inf elsewhere.  frame_background (csrc/background.hip)
keeps a depth only where it is not 0 and strictly below its cut, IN PLACE in the frame buffer everything downstream reads, and writes
the depth-range partials of what it kept: without a sensor it stands in frame_range's place (the launch count does not change), with
one frame_ingest runs without partials and frame_background follows it (one launch more).  Both frame slots are masked against the
one cut map; the detector (acquire, hand_size) and joint_visibility see the masked frame.  learn_background(frame) is a plan of its
own (upload, [frame_ingest], background_learn, then the cut map); background_model() / set_background_model() / clear_background()
let a rig learn once and reload.  A model that was never learned is the neutral element: every output is that of a tracker without
the option.  background=None is the plan above, untouched.  Out of scope: per-source options, a cut inside the ingest kernel, the
host HandDetector API, morphological clean-up of the mask, mixed pixels at object edges, choosing margin / rel for a sensor.

ADAPTATION.  background=dict(..., adapt=dict(persist=, guard=, every=1)) keeps that model current while tracking (hipdp/multitrack.py,
ADAPTATION; tests/background_adapt_ref.py is the definition): frame_background_adapt stands in frame_background's place, cuts the
frame with the cut map as it stands and, from the raw depth, confirms the model, counts a depth that stays elsewhere for `persist`
adapting ticks before it replaces the model, and rewrites the cut map on the device where the model changed.  The pixels inside the
crop window track_refine left in the last tick, dilated by `guard`, are kept out.  The tracker adapts in every `every`-th tick, and
not in the tick after reset / acquire / a set_hand that changes the hand (the window on the device is stale there).  Known limits: a
lost track has no window, so a hand that rests for `persist` adapting ticks after the track was lost is absorbed; a forearm outside
the window can be absorbed and recedes once it moves; persist and guard have no default, none has been chosen for a sensor.
"""
import numpy as np

from . import ops
from .augmenter import camera_tuple

OK, LOST, IDLE = ops.TRACK_OK, ops.TRACK_LOST, ops.TRACK_IDLE


def _net_side(net):
    dims = net.cfgParams.inputDim
    d0 = dims[0] if isinstance(dims[0], (list, tuple)) else dims
    return int(d0[2])


def _engine(net, rt, what, batch, why):
    net.setDeterministic()
    eng = net._engine(rt)
    if eng.N != batch:
        raise ValueError("%s must be built for a batch of %s (batchSize=%d): %s" % (what, 'one' if batch == 1 else batch, eng.N, why))
    if any(t.shape[3] != 1 for t in eng.x_ins):
        raise ValueError("%s must take single-channel depth crops" % what)
    return eng


def _engine_b1(net, rt, what):
    return _engine(net, rt, what, 1, "one frame is one plan")


def refine_stage(rt, frame, H, W, partial, rec, com_in, cube, ceng, cam, fx, fy, dsz_final, com_out, com3d, rec_out, status, M=None, tracks=None):
    """The (op, side) list of HandDetector.track for ONE frame whose depth-range partials are in `partial`: window around com_in,
    the refinement net's inputs, its forward plan, track_refine.  Shared by HandTracker's plan and HandDetector.track -- and, with
    tracks = an ops.TrackSet (hipdp/multitrack.py), by MultiTracker's plan: the same steps for T tracks that each read frame src[t] of
    `frame` and its partials, through the indexed siblings of the three crop launches.  Where the TrackSet has a table the sources have
    cameras and frame sizes of their own, `frame` is the ragged frame buffer, the *_src siblings read (H, W, cam, fx, fy) per source
    from the table and the arguments of that name are unused."""
    nin = len(ceng.x_ins)
    if nin not in (1, 3):
        raise NotImplementedError("Number of inputs is {}".format(nin))
    if ceng.out_dim != 3:
        raise ValueError("the refinement net must regress one 3-D offset")
    rs = int(ceng.x_ins[0].shape[1])
    B = 1 if tracks is None else tracks.T
    in0 = ceng.x_ins[0].buf.reshape(B, rs, rs)
    out = [(ops.crop_prepare_ranged(rt, partial, B, com_in, cube, fx, fy, rs, rec, None, stretch=True, tracks=tracks), False),
           (ops.crop_warp(rt, frame, rec, B, H, W, rs, in0, normalize=True, nd_value=0.0, name='track_in0', tracks=tracks), False)]
    for k in range(1, nin):                        # 1/2 and 1/4 CENTRE crops, handdetector.py:657-669
        f = 2 ** k
        out.append((ops.crop_center(rt, in0, B, rs, rs, ceng.x_ins[k].buf, rs // f, rs // f, name='track_in%d' % k), False))
    out.extend(ceng.fwd.ops)
    out.append((ops.track_refine(rt, frame, rec, B, H, W, com_in, cube, ceng.out.buf, cam, fx, fy, dsz_final, com_out, com3d, rec_out, status,
                                 M_out=M, tracks=tracks), False))
    return out


def frame_stage(rt, fr, raw, B, H, W, partial, sensor, cut=None, table=None, adapt=None):
    """The launches that open a plan on B frames (with a table: on its sources): they leave the float32 frames in `fr` and their
    depth-range partials in `partial`.  frame_range; with a sensor (ops.sensor_spec's tuple) frame_ingest from `raw` in its place;
    with a background cut map frame_background in frame_range's place, behind a frame_ingest that then writes no partials.  adapt
    (dict(bg=, take=, records=, T=, src=); cut is then bg's): frame_background_adapt in frame_background's place, the same count."""
    out = []
    if sensor is not None:
        out.append(ops.frame_ingest(rt, raw, B, H, W, fr, partial if cut is None else None, median=sensor[1], mirror=sensor[2], table=table))
    elif cut is None:
        out.append(ops.frame_range(rt, fr, B, H, W, partial, table=table))
    if adapt is not None:
        out.append(ops.frame_background_adapt(rt, fr, adapt['bg'], adapt['take'], B, H, W, adapt['records'], adapt['T'], adapt['src'], partial,
                                              table=table))
    elif cut is not None:
        out.append(ops.frame_background(rt, fr, cut, B, H, W, partial, table=table))
    return out


class AdaptClock(object):
    """The host's side of background adaptation for a tracker of C sources: which sources adapt in a tick (`take`), kept per input set
    in a device array that is uploaded only when it changes.  Source c adapts when it delivered a fresh frame, the tick's number
    (counted over process() calls and sequence ticks alike) is a multiple of `every`, and no track on c was restarted from the host
    since c's last tick: such a track's window on the device is stale (or empty) for one tick."""

    def __init__(self, rt, C, every):
        self.rt, self.C, self.every, self.tick = rt, int(C), int(every), 0
        self.restarted = np.ones(self.C, bool)                  # nothing was tracked yet: no window to trust
        self.bufs, self.hosts = [rt.alloc((self.C,), np.int32)], [np.zeros(self.C, np.int32)]

    def buf(self, slot):
        if slot == len(self.bufs):                              # process_sequence's second set, made when first used
            self.bufs.append(self.rt.alloc((self.C,), np.int32))
            self.hosts.append(np.zeros(self.C, np.int32))
        return self.bufs[slot]

    def restart(self, c):
        self.restarted[c] = True

    def step(self, fresh, slot=0):
        """One tick with fresh[c] true where source c delivered a frame: the tick's take, uploaded into the slot's array if it differs
        from what that array holds (the slot's last plan is behind us, as for the gates)."""
        on = self.tick % self.every == 0
        take = np.array([int(bool(f) and on and not r) for f, r in zip(fresh, self.restarted)], np.int32)
        self.restarted &= ~np.asarray(fresh, bool)
        self.tick += 1
        buf = self.buf(slot)                                    # first: it makes the second set, hosts[slot] with it
        if not np.array_equal(take, self.hosts[slot]):
            buf.set(take)
            self.hosts[slot] = take
        return take


def valid_centre(com):
    """A centre (image coordinates, z in mm) a track can start from: finite, with a depth that is not numpy.isclose to 0."""
    return bool(np.all(np.isfinite(com))) and not np.isclose(com[2], 0.)


def check_frame(frame, sensor, shape, who):
    """`frame` as the array a tracker uploads: float32 without a sensor, else a raw frame of the sensor's dtype (taken as it is or not
    at all: no silent conversion), of `shape`; `who` words the shape error ("expected", "source 1 delivers")."""
    if sensor is None:
        frame = np.asarray(frame, np.float32)
    else:
        frame = np.asarray(frame)
        if frame.dtype != sensor[0]:
            raise ValueError("frame dtype %s, the tracker's sensor delivers %s" % (frame.dtype, sensor[0]))
    if frame.shape != shape:
        raise ValueError("frame shape %s, %s %s" % (frame.shape, who, shape))
    return frame


class ResultBlock(object):
    """Everything the host reads per frame as ONE float32 device allocation (`buf`): an ordered list of (name, shape, dtype) fields of
    4-byte elements.  `offsets`: name -> first word; view(name): the field on the device; split(host): name -> the field of a
    downloaded block, reshaped, an int32 field viewed as int32."""

    def __init__(self, rt, fields):
        self.fields, n = {}, 0                      # name -> (first word, one past the last, shape, dtype), in block order
        for name, shape, dtype in fields:
            assert np.dtype(dtype).itemsize == 4, (name, dtype)
            self.fields[name] = (n, n + int(np.prod(shape)), tuple(shape), np.dtype(dtype))
            n = self.fields[name][1]
        self.offsets = dict((name, f[0]) for name, f in self.fields.items())
        self.buf = rt.alloc(n, np.float32)

    def view(self, name):
        a, _, shape, dtype = self.fields[name]
        return self.buf.view(a, shape, dtype)

    def split(self, host):
        return dict((name, host[a:b].view(dtype).reshape(shape)) for name, (a, b, shape, dtype) in self.fields.items())


def track_fields(T, J):
    """The fields every tracker's block starts with, over T tracks: pose (mm), pose in image coordinates, centres (= the state), com3D,
    M, status -- and one detector's 8 words (seed, cube out, status: acquire)."""
    f32 = np.float32
    return [('pose', (T, J, 3), f32), ('pose_img', (T, J, 3), f32), ('com', (T, 3), f32), ('com3D', (T, 3), f32), ('M', (T, 3, 3), f32),
            ('status', (T,), np.int32), ('det', (8,), f32)]


def smooth_fields(T, J, G=0):
    """What a tracker with `smooth` appends to its block, behind every other field: the filtered poses, their projections and
    dpp_pose_smooth's word per track, and per group where the tracker has groups."""
    f32, i32 = np.float32, np.int32
    f = [('pose_f', (T, J, 3), f32), ('pose_img_f', (T, J, 3), f32), ('sstat', (T,), i32)]
    if G:
        f += [('fused_pose_f', (G, J, 3), f32), ('gstat', (G,), i32)]
    return f


def visibility_fields(T, J, G=0):
    """What a tracker with `visibility` appends to its block, behind every other field (smooth's included): dpp_joint_visibility's
    share of supporting pixels, weight and class per track and joint, and per group the largest weight that went into each fused joint."""
    f32 = np.float32
    f = [('vis', (T, J), f32), ('vis_weight', (T, J), f32), ('vis_class', (T, J), np.int32)]
    if G:
        f += [('fused_weight', (G, J), f32)]
    return f


def timing_fields(T, J):
    """What a MultiTracker with `timing` appends to its block, behind every other field (visibility's included): every track's pose, its
    projection and its centre at the tick's instant, the time it was moved over and dpp_pose_align's word."""
    f32 = np.float32
    return [('pose_t', (T, J, 3), f32), ('pose_img_t', (T, J, 3), f32), ('com3D_t', (T, 3), f32), ('lead', (T,), f32), ('astat', (T,), np.int32)]


class HandTracker(object):
    def __init__(self, rt, importer, poseNet, comrefNet, H, W, cube, hand_right=False, invX=False, invY=False, fx=None, fy=None, sensor=None,
                 smooth=None, visibility=None, timing=False, background=None):
        """
        :param importer:   the dataset importer (camera; NYU / MSRA flip the y axis)
        :param poseNet:    the pose regressor, built for a batch of one; its output is J x 3 normalised joints
        :param comrefNet:  a ScaleNet-like net (numInputs 1 or 3) regressing the normalised 3-D offset of the hand centre, batch of one
        :param H, W:       frame size
        :param cube:       metric cube (mm) around the hand
        :param hand_right, invX, invY: estimatePose's mirroring (realtimehandposepipeline.py:347-369)
        :param fx, fy:     what the reference hands to HandDetector (config['fx'], config['fy']); default: the importer's
        :param sensor:     None: frames are float32 millimetres, prepared by the host.  dict(dtype='uint16' | 'float32', median=bool,
                           mirror=bool): frames are RAW sensor frames of that dtype, converted (mirrored, median-filtered) on the device
        :param smooth:     None, or dict(rate=, mincutoff=, beta=, dcutoff=1.0, max_hold=0): the One-Euro filter over the pose as the last
                           launch of the plan (hipdp/multitrack.py, SMOOTHING): the result gains pose_f, pose_img_f and `smooth`
        :param visibility: None, or dict(radius=, margin=, min_support=, hidden_weight=0.0): one launch behind pose_finish classifies every
                           joint by the frame's depths around its pixel (hipdp/multitrack.py, VISIBILITY): the result gains `vis`
                           and `vis_class`
        :param timing:     True (needs `smooth`): every frame carries its stamp (s) and the filter runs over real elapsed time
                           (dpp_pose_smooth_t; smooth's `rate` is still validated but goes unread).  One camera has nothing to align:
                           there is no align launch (hipdp/multitrack.py, TIMING)
        :param background: None, or dict(margin=, rel=0.0, min_seen=1): a learned per-pixel background is removed from every frame as
                           the plan's first step (BACKGROUND above); margin (mm) has no default.  Nothing is removed until
                           learn_background() / set_background_model().  With adapt=dict(persist=, guard=, every=1) among its keys
                           the model is kept current while tracking, by the same launch (ADAPTATION above); persist (ticks) and
                           guard (pixels) have no default
        """
        self.rt, self.H, self.W = rt, int(H), int(W)
        self.importer = importer
        self.cam = camera_tuple(importer)
        self.fx = abs(float(importer.fx if fx is None else fx))
        self.fy = abs(float(importer.fy if fy is None else fy))
        self.ceng = _engine_b1(comrefNet, rt, 'comrefNet')
        self.peng = _engine_b1(poseNet, rt, 'poseNet')
        if len(self.peng.x_ins) != 1 or self.peng.out_dim % 3:
            raise ValueError("the pose net takes one crop and regresses J x 3 coordinates")
        self.rs, self.ds, self.J = int(self.ceng.x_ins[0].shape[1]), int(self.peng.x_in.shape[1]), self.peng.out_dim // 3
        f32 = np.float32
        self.frames = [rt.alloc((1, self.H, self.W), f32, zero=False) for _ in range(2)]      # t and t + 1 (process_sequence)
        self.sensor = None if sensor is None else ops.sensor_spec(sensor)                      # (dtype, median, mirror)
        # with a sensor the host uploads into `raw`, frame_ingest fills `frames`; without one `frames` IS what the host uploads into
        self.raw = None if sensor is None else [rt.alloc((1, self.H, self.W), self.sensor[0], zero=False) for _ in range(2)]
        self.inputs = self.frames if sensor is None else self.raw
        self.partial = ops.frame_range_workspace(rt, 1)
        self.background = None if background is None else ops.background_spec(background)
        self.bg = None if background is None else ops.BackgroundModel(rt, background, 1, self.H, self.W)   # near, seen, cut, take[, cand, run]
        self.adapt = None if self.bg is None or self.bg.adapt is None else AdaptClock(rt, 1, self.bg.adapt[2])
        self._learn = None
        self.rec = rt.alloc(rt.lib.dpp_crop_record_bytes(), np.uint8)
        self.cube = rt.alloc((1, 3), f32)
        # everything the host reads per frame is ONE block: pose (mm), pose in image coordinates, centre (= the state), com3D, M, status
        self.smooth = None if smooth is None else ops.smooth_spec(smooth)
        self.timing = bool(timing)
        if self.timing and smooth is None:
            raise ValueError("timing needs smooth: with one camera the stamps are read by the filter alone")
        self.sstate = None if smooth is None else ops.SmoothState(rt, 1, self.J, timed=self.timing)   # the filter's state: never downloaded
        # with `timing` one (stamp, now = stamp) pair per frame buffer, uploaded with the frame
        self.stamps = [rt.alloc((2,), np.float64) for _ in range(2)] if self.timing else None
        # (+ the detector's seed / cube / status words: acquire; with `smooth` the filtered pose, its projection and the filter's word follow)
        self.visibility = None if visibility is None else ops.visibility_spec(visibility)
        self.vsrc = None if visibility is None else rt.alloc((1,), np.int32)      # the one track's source: 0
        self.block = blk = ResultBlock(rt, track_fields(1, self.J) + (smooth_fields(1, self.J) if smooth is not None else []) +
                                       (visibility_fields(1, self.J) if visibility is not None else []))
        self.res = blk.buf
        self.pose3d, self.pose_img, self.com, self.com3d = blk.view('pose'), blk.view('pose_img'), blk.view('com'), blk.view('com3D')
        self.M, self.status = blk.view('M'), blk.view('status')
        self.crop = self.peng.x_in.buf.reshape(1, self.ds, self.ds)          # the pose net's input IS the final crop
        self.flags = 0
        self.set_hand(hand_right)
        self.set_inv(invX, invY)
        self._plans = {}
        self._detector = None
        self._slot = 0                                                         # frame buffer of the last frame
        self.lost = True                                                       # no centre yet
        self.set_cube(cube)
        self.runs = 0

    # ---- device state -----------------------------------------------------------------------------------------------------
    def reset(self, com):
        """Start (again) from the centre `com` (image coordinates, z in mm)."""
        com = np.asarray(com, np.float32).reshape(3)
        if not valid_centre(com):
            raise ValueError("reset needs a centre with a depth: %r" % (com,))
        self.com.set(com)
        self.lost = False
        self._clear_smooth()

    def _clear_smooth(self):
        """A restart or another hand: what is followed now is not what was filtered (one 4-byte upload), and the crop window the
        device holds is not this hand's: the background does not adapt in the next tick."""
        if self.sstate is not None:
            self.sstate.clear(0)
        if self.adapt is not None:
            self.adapt.restart(0)

    def detector(self):
        """The whole-frame detector on this tracker's buffers: frame slot 0 (and its raw buffer, with a sensor), the depth-range partials,
        the centre (its output) and the cube."""
        if self._detector is None:
            from .detect import FrameDetector
            self._detector = FrameDetector(self.rt, self.H, self.W, self.fx, self.fy, 1, frames=self.frames[0], partial=self.partial,
                                           com=self.com, cube=self.cube, res=self.block.view('det'), sensor=self.sensor,
                                           raw=None if self.sensor is None else self.raw[0],
                                           **({} if self.bg is None else dict(background=self.background, cut=self.bg.view(self.bg.cut, 0))))
        return self._detector

    # ---- the learned background ---------------------------------------------------------------------------------------------
    def _model(self):
        if self.bg is None:
            raise RuntimeError("the tracker was built without background=")
        return self.bg

    def learn_background(self, frame):
        """One frame of the scene WITHOUT the hand into the model (a raw one with a sensor: what is learned is frame_ingest's output):
        one upload, a plan of its own ([frame_ingest], background_learn), then the cut map -- a download of the model, the map on the
        host, one upload.  Not on the per-frame path."""
        bg = self._model()
        frame = self._frame(frame)
        if self._learn is None:
            rt, p = self.rt, ops.Plan('learn_background')
            if self.sensor is not None:
                p.add(ops.frame_ingest(rt, self.raw[0], 1, self.H, self.W, self.frames[0], None, median=self.sensor[1], mirror=self.sensor[2]))
            p.add(ops.background_learn(rt, self.frames[0], bg.take, 1, self.H, self.W, bg.near, bg.seen))
            self._learn = p
        self.inputs[0].set(frame)
        self._slot = 0
        self._learn.run(self.rt)
        self.rt.synchronize()
        bg.refresh()
        bg.forget_candidates()

    def background_model(self):
        """dict(near, seen, cut), (H, W) arrays: what set_background_model() of another tracker takes.  With adapt these are the
        adapted ones."""
        self.rt.synchronize()
        return self._model().get(0)

    def set_background_model(self, model):
        """Load dict(near=, seen=) as background_model() returned it (the cut map is computed from them with THIS tracker's options)."""
        self.rt.synchronize()
        self._model().set(0, model['near'], model['seen'])

    def clear_background(self):
        """Forget the model: the tracker is that of one without the option until something is learned again."""
        self.rt.synchronize()
        self._model().clear()

    def acquire(self, frame, do_hand_size=False):
        """Find the hand in `frame` (a raw one with a sensor: frame_ingest then opens the detector plan) and start (again) from it: one
        upload, the detector plan, one download of the tracker's result block.  Returns dict(com [3]
        image coordinates, cube [3] -- measured with do_hand_size, else the tracker's; the tracker's own cube is not changed --, found).
        Not found: the centre is (0, 0, 0) and the track is lost."""
        frame = self._frame(frame)
        det = self.detector()
        self.inputs[0].set(frame)
        self._slot = 0
        det.plan(do_hand_size).run(self.rt)
        self.rt.synchronize()
        res = self.block.split(self.res.get())                                  # the tracker's block: centre and detector words together
        coms, cubes, found, _, _ = det.parse(res['det'], res['com'], None if do_hand_size else self.cube_host)
        ok = bool(found[0]) and valid_centre(coms[0])
        self.lost = not ok
        if ok:                                                                 # a restart, as reset(com) is
            self._clear_smooth()
        elif self.adapt is not None:
            self.adapt.restart(0)
        return dict(com=coms[0], cube=cubes[0], found=ok)

    def hand_size(self, tol=0.0):
        """The hand's cube around the current centre in the frame last handed to process() or acquire():
        HandDetector.estimateHandsizeComponents on the device state (with a sensor: on the converted, filtered frame the plan left in
        the float32 frame buffer).  An empty depth range gives the tracker's cube.  After
        process_sequence the last frame may sit in the other frame buffer, which the detector does not see: RuntimeError."""
        if self._slot != 0:
            raise RuntimeError("hand_size measures the frame of the last process() / acquire(); the last frame came through process_sequence")
        cubes, _ = self.detector().hand_size(tol=tol)
        return cubes[0]

    def set_cube(self, cube):
        cube = np.asarray(cube, np.float32).reshape(3)
        if not (cube > 0).all():
            raise ValueError("the cube must have a positive size: %r" % (cube,))
        self.cube.set(cube)
        self.cube_host = cube

    def set_hand(self, right):
        """HAND_RIGHT mirrors the pose net's input and the x coordinate of its output.  (The mirroring is an argument of two
        launches, so each combination of hand / invX / invY has a plan of its own, recorded the first time it is used.)"""
        flags = (self.flags & ~ops.POSE_HAND_RIGHT) | (ops.POSE_HAND_RIGHT if right else 0)
        if flags != self.flags:                                                # the other hand: not what was filtered
            self._clear_smooth()
        self.flags = flags

    def set_inv(self, invX, invY):
        self.flags = (self.flags & ~(ops.POSE_INV_X | ops.POSE_INV_Y)) | (ops.POSE_INV_X if invX else 0) | (ops.POSE_INV_Y if invY else 0)

    # ---- the per-frame plan -----------------------------------------------------------------------------------------------
    def plan(self, slot=0):
        key = (slot, self.flags)
        if key not in self._plans:
            rt, H, W, fr = self.rt, self.H, self.W, self.frames[slot]
            p = ops.Plan('track')
            # frame_range; with a sensor raw -> fr and the same partials IN ITS PLACE; with a background the cut, which writes them
            # ... and with adapt the adapting cut in ITS place: the window track_refine left in `rec` in the last tick is kept out
            adapt = None if self.adapt is None else dict(bg=self.bg, take=self.adapt.buf(slot), records=self.rec, T=1, src=None)
            for op in frame_stage(rt, fr, None if self.sensor is None else self.raw[slot], 1, H, W, self.partial, self.sensor,
                                  None if self.bg is None else self.bg.cut, adapt=adapt):
                p.add(op)
            # the state buffer is read (prepare, track_refine) and then rewritten by ONE lane of track_refine: in place
            for op, side in refine_stage(rt, fr, H, W, self.partial, self.rec, self.com, self.cube, self.ceng, self.cam, self.fx, self.fy,
                                         self.ds, self.com, self.com3d, self.rec, self.status, self.M):
                p.add(op, side)
            wf = ops.CROP_NORMALIZE | (ops.CROP_FLIP_X if self.flags & ops.POSE_HAND_RIGHT else 0)
            p.add(ops.crop_warp_ex(rt, fr, self.rec, 1, H, W, self.ds, self.crop, flags=wf, nd_value=0.0, name='track_crop'))
            for op, side in self.peng.fwd.ops:
                p.add(op, side)
            p.add(ops.pose_finish(rt, self.peng.out.buf, 1, self.J, self.cube, self.com3d, self.cam, self.flags, self.pose3d, self.pose_img))
            if self.visibility is not None:         # reads the float32 frame of this slot, which the whole plan leaves as it is
                blk = self.block
                p.add(ops.joint_visibility(rt, self.pose_img, self.status, self.vsrc, 1, self.J, fr, 1, self.visibility, blk.view('vis'),
                                           blk.view('vis_weight'), blk.view('vis_class'), H=H, W=W))
            if self.smooth is not None:
                blk = self.block
                timed = dict(stamps=self.stamps[slot], C=1) if self.timing else {}
                p.add(ops.pose_smooth(rt, self.pose3d, self.status, 1, self.J, self.smooth, self.sstate, blk.view('pose_f'),
                                      blk.view('pose_img_f'), blk.view('sstat'), cam=self.cam, **timed))
            self._plans[key] = p
        return self._plans[key]

    def _result(self, res, crop=None):
        out = dict((k, v[0]) for k, v in self.block.split(res).items() if k != 'det')      # the one track's row of every field
        out['status'] = int(out['status'])
        if self.smooth is not None:
            out['smooth'] = int(out.pop('sstat'))
        if self.visibility is not None:
            del out['vis_weight']                                              # 1 where vis_class is VISIBLE, else hidden_weight
        if crop is not None:
            out['crop'] = crop
        return out

    def _check(self, frame):
        if self.lost:
            raise RuntimeError("the track is lost (or was never started): call reset(com) with a new centre")
        return self._frame(frame)

    def _frame(self, frame):
        return check_frame(frame, self.sensor, (self.H, self.W), 'expected')

    def _stamp(self, stamp):
        """The frame's stamp checked: None without `timing` (where passing one raises), else the two doubles to upload."""
        if not self.timing:
            if stamp is not None:
                raise ValueError("a stamp needs a tracker with timing=True")
            return None
        try:
            v = float(stamp)
        except (TypeError, ValueError):
            v = np.nan
        if not np.isfinite(v):
            raise ValueError("a timed frame needs a finite stamp in seconds: %r" % (stamp,))
        return np.float64([v, v])

    def process(self, frame, return_crop=False, stamp=None):
        """One frame, synchronously: one upload, one plan, one download.  Returns dict(pose [J][3] mm, pose_img [J][3], com [3] image
        coordinates, com3D [3], M [3][3], status[, crop]) -- `crop` as the pose net saw it (normalised; mirrored for HAND_RIGHT).
        status LOST: see the module docstring; the other entries are finite but meaningless and the tracker needs reset(com).  With
        `timing`, `stamp` is the frame's time in seconds: one more upload of 16 bytes."""
        frame = self._check(frame)
        when = self._stamp(stamp)
        self.inputs[0].set(frame)
        if when is not None:
            self.stamps[0].set(when)
        if self.adapt is not None:
            self.adapt.step([True], 0)
        self._slot = 0
        self.plan(0).run(self.rt)
        self.runs += 1
        self.rt.synchronize()
        out = self._result(self.res.get(), self.crop.get()[0] if return_crop else None)
        self.lost = out['status'] != OK
        return out

    def process_sequence(self, frames, return_crops=False):
        """A sequence of frames: the upload of frame t + 1 runs under the plan of frame t (two frame buffers, copy stream), the result
        of frame t is read while frame t + 1 is in flight.  Same values as process() frame by frame.  Stops at a lost frame (its
        result is the last one returned).  With `timing` the sequence's entries are (frame, stamp).

        With `adapt` a lost frame leaves more behind than the process() loop would: frame n + 1 was launched before the host learnt
        that frame n was lost, and only its RESULT is dropped.  Its tick has adapted the model, with an empty window, so nothing
        was kept out, and has advanced the adaptation's tick counter by one.  One such tick changes `near` nowhere through a candidate
        (persist >= 2), but it confirms, counts candidates and counts towards `every`.  After a lost frame neither the model nor the
        tick counter is what the loop leaves; reset(com) restarts the track either way, and the tick after it does not adapt."""
        rt = self.rt
        staged = hasattr(rt, 'staged_upload')
        results, pending, free = [], None, [None, None]

        def resolve(p):
            res, crop = p
            out = self._result(res.get(), crop.get()[0] if crop is not None else None)
            results.append(out)
            return out['status'] == OK
        for n, frame in enumerate(frames):
            when = None
            if self.timing:
                if not isinstance(frame, tuple) or len(frame) != 2:
                    raise ValueError("a timed sequence's entries are (frame, stamp)")
                frame, when = frame[0], self._stamp(frame[1])
            frame = self._check(frame)
            k = n & 1
            if staged:
                rt.wait_event(rt.staged_upload(self.inputs[k], frame[None], free[k]))
                if when is not None:
                    rt.wait_event(rt.staged_upload(self.stamps[k], when, free[k]))
            else:
                self.inputs[k].set(frame)
                if when is not None:
                    self.stamps[k].set(when)
            plan = self.plan(k)
            if self.adapt is not None:
                self.adapt.step([True], k)
            plan.run(rt)
            self._slot = k
            self.runs += 1
            free[k] = rt.record_event() if staged else None
            handle = (rt.read_async(self.res), rt.read_async(self.crop) if return_crops else None)
            if pending is not None and not resolve(pending):
                self.lost = True              # frame n ran on a meaningless centre: dropped
                rt.synchronize()
                return results
            pending = handle
        if pending is not None and not resolve(pending):
            self.lost = True
        rt.synchronize()
        return results
