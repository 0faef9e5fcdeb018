"""
Realtime tracking of several hands over several cameras: T tracks over C frame sources, ONE launch plan per tick.

hipdp/tracker.py's plan follows one hand in one camera's frames.  At a batch of one the two nets are bound by their launches, not
by arithmetic, so a second hand (or a second camera) served by a second HandTracker pays the whole plan, an upload and a download
again.  Here every launch of that plan runs once per tick for all tracks:

    frame_range (or frame_ingest)   at B = C       every source's depth range, the one pass over each frame
    crop_prepare_ranged_ix          at B = T       track t's window in frame src[t], from that frame's partials
    crop_warp_ix -> crop_center x2  at B = T       the refinement net's inputs
    the refinement net's forward plan, built for a batch of T
    track_refine_ix                 at B = T       centre update, final record, M, com3D, status; the T centres stay on the device
    crop_warp_ex_ix                 at B = T       the final crop, mirrored where tflags[t] has POSE_HAND_RIGHT
    the pose net's forward plan, built for a batch of T
    pose_finish_ix                  at B = T       the sign rules per track from tflags[t]
    joint_visibility                at T x J       only with `visibility`: every joint classified by the frame's depths around its pixel (below)
    pose_align                      at B = T       only with `timing`: every track brought to the tick's one instant (below)
    pose_fuse                       at G groups    only with `groups`: the tracks of one hand fused, lost tracks handed over (below)
    extrinsics_accumulate           per source     in pose_fuse's place while a source's extrinsics are being calibrated (below)
    pose_smooth                     at T + G rows  only with `smooth`: the One-Euro filter over the tracked and the fused poses (below)

so the launch count is HandTracker's whatever T and C are (plus one with `groups`, plus one with `smooth`, plus one with `visibility`, plus one with `timing`).  A track names its source (`src`), its hand side and invX / invY
(`tflags`) and whether it takes part in this tick (`gate`) in three small int32 device arrays; the hand side is data, not a launch
argument, so there is one plan, not one per flag combination.  C cameras with one hand each is tracks = [(c, False) for c in
range(C)]; both hands of one camera is tracks = [(0, False), (0, True)]; mixtures are allowed.

GATING.  A track sits a tick out (gate 0) when it is lost, was never started, or its source delivered no frame.  Its row still runs
through the nets (on an all-zero crop), its centre's bits stay as they are, and it is reported IDLE -- or LOST, when that is why it
was gated.  A lost track does not stop the others; it stays gated until reset(t, com) or a successful acquire(t, frame).

SOURCES.  With one importer and one (H, W) every source is the same camera: the camera and the frame size are launch arguments, the
frames one [C][H][W] buffer, the launches the *_ix ones above.  `importer`, `H`, `W`, `fx`, `fy` may instead be sequences with one
entry per source (a scalar anywhere: the same for all sources).  Where the entries differ -- a 640 x 480 camera beside a 320 x 240
one, or one model with per-unit calibration -- the tracker builds a per-source table on the device (ops.SourceTable: camera,
HandDetector's fx / fy, frame size, frame offsets), keeps the frames in ONE ragged buffer (every frame padded to 16 bytes) and
builds the same plan through the *_src siblings of the launches that read a frame or a camera (ABI v19): the same kernels with the
table in place of the scalars, the same launch count.  All entries equal is the homogeneous path, untouched.  The sensor options
(dtype / median / mirror) stay common to all sources.

FUSION (ABI v20; csrc/fuse.hip).  The reference has one device and one camera: what follows is THIS PROJECT'S OWN, stated in
include/dpp_hip.h, restated in NumPy by tests/fuse_ref.py and pinned to it bit for bit.  `extrinsics` gives every source an (R, t)
with w = R p + t from its camera frame (the frame of `pose` / `com3D`: the importer's jointImgTo3D frame, flip_y included) to one
world frame (mm); `groups` lists the tracks that observe the same physical hand from different sources.  One more launch at the end of
the plan, one workgroup per group, then
  - averages the group's OK tracks in the world frame: MultiTracker.fused[g] = dict(pose, com, spread, n) -- the fused joints, the
    fused centre, per joint the largest distance of a member's joint from the fused one, the number of tracks that went in;
  - with `max_dev` (mm) drops from the average a track whose world centre is farther than that from the componentwise median of
    three or more (`outlier`: it slid onto something else), and marks two that are farther apart than that (`disagree`: both still go in);
  - gives every member the centre its peers see, projected by its own camera (`peer_com`), and with `handover` writes that centre
    into a member that lost the hand in this tick or is an outlier (`handed`).  A handed track is reported LOST for the tick but is
    not marked lost: it runs ungated in the next tick from its peers' centre -- one tick of outage, no detector plan, no upload.
A track that is gated because it is lost (it lost the hand while no peer had it) is restarted by process() through reset(t, peer_com)
in the first tick in which its peers have the hand: one small upload, as acquire makes.  Tracks in no group are left entirely alone, and
without `groups` the tracker allocates, uploads, launches and returns exactly what it did before.  (Confidence weighting stood in
this list when fusion was written: see VISIBILITY below.)  Triangulation from 2-D alone, fusing the depth frames themselves, hand size for several hands and per-source sensor options
are out of scope.

CALIBRATION (ABI v21; csrc/calib.hip, hipdp/calib.py; this project's own as well, restated by tests/calib_ref.py).  The (R, t) that fusion
needs can come from the tracked hand itself: every tick gives the same J joints of one hand in each camera's frame, and a least-squares
rigid fit needs only running sums over those pairs.  With calibrate=dict(anchor=, max_shape_dev=, min_cond=) entries of `extrinsics` may
be None.  While such a source is pending (`calibrating`) the tick's last launch is extrinsics_accumulate in pose_fuse's place -- the same
launch count -- which adds, per pending source c and per group with an OK track on both the anchor source and c, the J pairs (joint in
c's frame, the anchor's joint in the world frame) to c's row of `acc`, a small float64 buffer of its own.  With max_shape_dev (mm) a pair
of tracks whose two skeletons differ in shape by more than that -- joint distances from the centroid; rigid motions keep them -- stays
out (a track that slid onto something else).  `fused` is [], nothing is handed over, the per-track results are the ungrouped tracker's
plus 'group'; process_sequence works unchanged.  calibration_report() downloads the sums and fits (calib.solve_rigid: Kabsch on the
host, with n, rms, cond = s2 / s1 and ok); finish_calibration() also installs the fits when all are ok and rebuilds the plan: from then
on the tracker builds the launches of one constructed with these extrinsics.  reset_calibration() zeroes the sums.  Without `timing` the pairs are taken as
simultaneous; with it they are the aligned poses of one instant (TIMING below).  Out of scope: intrinsics, chained calibration through a third camera (every pending
source must share a group with the anchor), weighting by joint, drift monitoring after calibration, and re-solving on the device.

SMOOTHING (ABI v22; csrc/smooth.hip; this project's own as well, restated by tests/smooth_ref.py).  The joints of a tick are what the
pose net regressed from that tick's crop: a resting hand jitters, a fused pose jumps when a member drops out.  With
smooth=dict(rate=, mincutoff=, beta=, dcutoff=1.0, max_hold=0) the LAST launch of the tick runs the One-Euro filter (Casiez et al., CHI
2012: a low-pass whose cut-off mincutoff + beta * speed rises with the filtered speed) over every track's `pose` and, with `groups`,
every group's fused pose: one workgroup per row, whatever T and G are.  Its state (ticks since the last valid sample, filtered value and
derivative in float64) lives on the device apart from the result block and is never downloaded.  A track's sample is valid when its
status on the device is OK; a LOST or IDLE tick is an invalid sample: the row returns its last filtered pose for up to max_hold ticks
(`smooth` == ops.SMOOTH_HELD) and the next valid sample is filtered with Te = (ticks since the last one) / rate, so a source that
delivers every second tick filters with 2 / rate; beyond max_hold the state is dropped (SMOOTH_EMPTY | SMOOTH_DROPPED, zeros) and the
next valid sample starts it again (SMOOTH_INIT: pose_f == pose).  A group's sample is valid when n >= 1.  Per-track results gain pose_f,
pose_img_f (pose_f through the track's own camera) and `smooth`, the row's word; fused[g] gains pose_f and `smooth`.  A restart from
the host -- reset(t, com), and through it acquire, acquire_source and the automatic reset from peer_com -- and a set_hand(t, ...) that changes the hand clear
the track's row (one 4-byte upload); a hand-over on the device does not: the hand is the same one.  While a source is being calibrated
nothing is fused: the group rows are left out of the launch (their outputs read as zeros) and start empty after finish_calibration().
`rate` is the tracker's one tick rate; with `timing` the elapsed time comes from the sources' stamps instead and `rate` goes unread
(TIMING below).  Out of scope: extrapolating a held pose by the filtered derivative, feeding the filtered centre
back into the crop, filtering com / com3D, and choosing mincutoff / beta for a dataset.  smooth=None:
allocation, uploads, plan, result block and keys are those of before.

VISIBILITY (ABI v23; csrc/visibility.hip, dpp_pose_fuse_w in csrc/fuse.hip; this project's own as well, restated by
tests/visibility_ref.py).  A second camera is pointed at a hand because the first does not see all of it, and a camera whose view of a
finger is blocked still regresses a joint there.  With visibility=dict(radius=, margin=, min_support=, hidden_weight=0.0) ONE launch behind
pose_finish looks, for every joint (u, v, z) of every OK track, at the frame's pixels within `radius` of the joint's pixel: a pixel within
`margin` mm of z is ON the joint, one more than `margin` nearer is in FRONT of it, a 0 is empty.  `vis` [J] is the share of ON pixels;
`vis_class` [J] is ops.VIS_VISIBLE with at least min_support ON pixels, else VIS_OCCLUDED with at least min_support in FRONT, else
VIS_UNSUPPORTED (guessed onto background or into a hole), or VIS_OFFFRAME for a joint outside its frame or without a depth.  A track that
is not OK on the device has zeros.  With `groups` the fusion launch becomes dpp_pose_fuse_w: a VISIBLE joint weighs 1, any other
hidden_weight, the fused joint is the weighted mean of the inliers' joints (the plain mean where nobody sees it), `spread` is taken over
those with a weight > 0, and fused[g] gains `weight` [J], the largest weight that went in (0: nobody saw the joint).  Membership, the
median test, fused `com`, peer_com and the hand-over do not read the weights; pose_smooth is untouched and filters the weighted fused
pose.  While a source is being calibrated the launch still runs and nothing is fused.  The new fields stand behind every other field of
the block, smooth's included.  radius, margin and min_support have no default: none has been chosen for a dataset.  Out of scope: a
per-joint hold in the smoother, weighting the calibration pairs by visibility, weighting fused `com`, gating the hand-over by visibility,
continuous weights from `vis`, and choosing `margin` for a dataset.  visibility=None: allocation, uploads, plan, result block and keys
are those of before.

TIMING (ABI v24; csrc/align.hip, dpp_pose_smooth_t in csrc/smooth.hip; this project's own as well, restated by tests/align_ref.py).
Everything above that combines tracks takes the cameras of a tick as simultaneous and the ticks as a clock.  Depth cameras without a
sync line are neither: two 30 Hz cameras are up to 17 ms apart, which a hand at 1 m / s turns into 17 mm between the two views -- a
systematic error of the size of the pose error itself, straight into `fused`, `spread`, the max_dev test and the calibration sums.  With
timing=dict(max_gap=, max_lead=) (seconds; no defaults: none has been chosen for a rig) process(frames, stamps=, now=) takes one stamp
per source that delivers a frame -- all on ONE clock -- and the instant `now` the tick's combined outputs refer to (default: the largest
stamp of the fresh frames; kept in `self.now`); the C + 1 doubles are the tick's one new upload.  ONE launch behind pose_finish (and
behind joint_visibility, which compares a joint with its own frame and keeps reading the unaligned pose_img) moves every OK track's pose
and centre from its stamp ts to `now` along the velocity between its previous sample and this one: y = x + (x - x_prev) / (ts - t_prev)
* (now - ts), when there is a previous sample no older than max_gap and |now - ts| <= max_lead; otherwise the sample goes through as it
is (`align` == ops.ALIGN_ASIS | NOPREV, GAP or FAR).  The state (the previous stamp, pose and centre per track) lives on the device apart
from the result block.  pose_fuse / pose_fuse_w and extrinsics_accumulate then read the aligned arrays -- the same kernels, other
pointers -- so fused[g], spread, the outlier test, peer_com, the centre of a hand-over and the calibration sums all refer to `now`.
With `smooth` the last launch is dpp_pose_smooth_t: the tracks' rows filter the UNALIGNED pose over the time between their own stamps,
the groups' rows the fused pose over the time between the ticks' instants; a sample whose stamp is not later than the row's last one is
refused (ops.SMOOTH_STALE beside HELD / DROPPED); smooth['rate'] is still validated but goes unread.  Per-track results gain pose_t,
pose_img_t, com3D_t, `lead` (now - ts, s) and `align`, behind every other field of the block.  reset(t, com) -- and through it acquire,
acquire_source and the automatic reset from peer_com -- and a set_hand that changes the hand clear the track's row (one 4-byte upload
beside smooth's); a hand-over on the device does not.  process_sequence takes (frames, stamps) or (frames, stamps, now) per tick and keeps
one stamps buffer per input set, uploaded with that set's frames.  Out of scope: estimating an unknown clock offset between cameras (the
stamps are taken as one clock), letting an IDLE track coast into the fusion, using the filtered derivative as the velocity, and per-source
sensor options.  timing=None: allocation, uploads, plans, result block and keys are those of before.

BACKGROUND (ABI v25; csrc/background.hip; this project's own as well, restated by tests/background_ref.py).  Everything above combines
tracks that were already found; finding the hand still needed an empty scene: the detector starts from the nearest object of more than
200 px, the depth range feeds its slabs and crop_warp keeps whatever lies inside the cube, so on a fixed camera a desk edge, a monitor
or the user's torso is what acquire / acquire_source return.  With background=dict(margin=, rel=0.0, min_seen=1) (common to all sources,
like `sensor`; margin in mm has no default) every source has a per-pixel model at its own frame size -- near (float32, the smallest
non-zero depth seen while learning; 0: none) and seen (int32, the learning frames with a depth) -- and a cut map computed on the HOST
once per model change, every operation rounded to float32: near - (margin + rel * near) where seen >= min_seen, near != 0 and the
result is > 0, +inf elsewhere.  frame_background keeps a depth only where it is not 0 and strictly below its cut, IN PLACE in the
frame buffer everything downstream reads, and writes the depth-range partials of what it kept: without a sensor in frame_range's place
(the launch count does not change), with one behind a frame_ingest that writes no partials (one launch more).  Both input sets of
process_sequence are masked against the one cut map; masking is idempotent, so the stale frame of a source that sits a tick out is
masked again to the same bits.  The per-track and per-source detectors take views of the cut map, so acquire, acquire_source, hand
size and joint_visibility see the masked frame.  learn_background(frames) (None where a source sits out) is a plan of its own: upload,
[frame_ingest], background_learn, then the cut maps of the sources that took part.  background_model(c) / set_background_model(c,
model) / clear_background([c]) let a rig learn once and reload.  A model that was never learned is the neutral element.  Out of scope:
per-source options, a cut inside the ingest kernel, the host HandDetector API, morphological clean-up of the mask, mixed pixels at
object edges, choosing margin / rel (or persist / guard) for a sensor.  background=None: allocation, uploads, plans, result block and
keys are those of before.

ADAPTATION (additive to ABI v25: dpp_frame_background_adapt; this project's own, restated by tests/background_adapt_ref.py).  A model
learned once goes stale: a cup put on the desk is the nearest object from then on, and something taken away leaves a cut that is too
near.  With background=dict(..., adapt=dict(persist=, guard=, every=1)) the plan's frame_background launch is frame_background_adapt,
the launch count unchanged: in the pass that cuts the frame it also confirms the model where the raw depth lies in its band
(near = min, seen += 1), counts a depth that stays elsewhere as a candidate (cand, run; the model's own band around cand) and
replaces the model with it after `persist` adapting ticks, and rewrites the cut map on the device, in the host's float32 arithmetic,
where the model changed; the new cut holds from the next tick on.  What must not be learned is on the device already: track_refine
left every track's final crop window in the records buffer, and the pixels inside a window of the source, dilated by `guard`, only
lose their candidate.  The host sets take[c] = 1 when source c delivered a fresh frame, the tick's number (process() calls and
sequence ticks alike) is a multiple of `every`, and no track on c was restarted from the host since c's last tick -- reset, acquire,
acquire_source, the automatic peer_com reset, a set_hand that changes the hand: such a track's window is stale for one tick; take is
uploaded only when it changes, one array per input set.  A source with take 0 runs the plain cut and reads no model array; its
stale frame is cut again, possibly by a newer cut.  set / clear / learn_background zero the candidates of the sources they touch;
background_model(c) returns the adapted model; the detectors take views of the cut map and do not adapt.  Known limits: a lost or
gated track has no window, so its hand is absorbed if it stays still for `persist` adapting ticks; a forearm outside the crop window
can be absorbed, and recedes again once it moves; a hand handed over on the device is unprotected for one tick (persist >= 2 keeps
that tick from changing `near` through a candidate); no per-source options, and no persist / guard chosen for a sensor.  adapt absent:
allocation, uploads, plans, result block and keys are those of before.

acquire_source(c, frame) finds ALL hands of a source in one detector plan and starts the source's tracks from them; the detectors
are built per source, at that source's size and focal lengths, on views of its frame slice.

SEQUENCES.  process_sequence(ticks) is HandTracker.process_sequence for several sources: two sets of input buffers, the uploads of
tick n + 1 on the copy stream under the plan of tick n, the result block of tick n read while tick n + 1 is in flight.  The host
therefore learns one tick late that a track was lost: the track runs ungated for one more tick (track_refine reports it LOST there:
a frame queued behind a lost one stays lost) and is gated from the tick after.  Nothing is detected inside a sequence, and nothing is
reset from the host inside one: the hand-over on the device needs no host knowledge, so a track lost and handed in tick n is OK again
in tick n + 1 as in the process() loop, but a track that is gated because it is lost stays gated until the sequence ends.
"""
import numpy as np

from . import ops
from .augmenter import camera_tuple
from .tracker import IDLE, LOST, OK, AdaptClock, ResultBlock, _engine, check_frame, frame_stage, refine_stage, smooth_fields, timing_fields, track_fields, valid_centre, visibility_fields


class MultiTracker(object):
    def __init__(self, rt, importer, poseNet, comrefNet, H, W, cube, tracks, sources=None, invX=False, invY=False, fx=None, fy=None,
                 sensor=None, extrinsics=None, groups=None, max_dev=None, handover=True, calibrate=None, smooth=None, visibility=None, timing=None,
                 background=None):
        """
        :param importer:   the dataset importer (the camera) of all sources, or a sequence of C importers, one per source
        :param poseNet, comrefNet: as for HandTracker, but built for a batch of T, the number of tracks: row t is track t
        :param H, W:       frame size of all sources, or sequences of C ints
        :param cube:       metric cube (mm) every track starts with (set_cube(t, cube) changes one)
        :param tracks:     list of (source, hand_right): track t follows one hand in the frames of source `source`
        :param sources:    number of frame sources C (default: the largest source named, plus one); C <= T, every track reads one source
        :param invX, invY: estimatePose's mirroring, for all tracks
        :param fx, fy:     what the reference hands to HandDetector (a value for all sources or a sequence of C; None entries
                           and the default: the source's importer's)
        :param sensor:     as for HandTracker, for ALL sources: frames are raw sensor frames and frame_ingest runs at B = C
        :param extrinsics: one (R, t) per source: R a 3 x 3 rotation, t in mm, w = R p + t from the source's camera frame to the world
        :param groups:     list of lists of track indices: the tracks of a group observe the same hand from pairwise distinct sources
                           (disjoint, 1 .. 16 members each; needs `extrinsics`).  None: no fusion, the tracker of before
        :param max_dev:    None, or the distance (mm) beyond which a member's world centre is an outlier / two members disagree
        :param handover:   a member that lost the hand (or is an outlier) goes on from its peers' centre; False: fusion reports only
        :param calibrate:  None, or dict(anchor=0, max_shape_dev=None, min_cond=0.) (any subset): entries of `extrinsics` may then be
                           None, and those sources are calibrated against the source `anchor` from the tracked hand (CALIBRATION above)
        :param smooth:     None, or dict(rate=, mincutoff=, beta=, dcutoff=1.0, max_hold=0): the One-Euro filter over the poses
                           (SMOOTHING above); rate (ticks / s), mincutoff (Hz) and beta (Hz per mm / s) have no default
        :param visibility: None, or dict(radius=, margin=, min_support=, hidden_weight=0.0): every joint classified by the frame's depths
                           around its pixel, and with `groups` the fusion weighted by it (VISIBILITY above); radius (pixels), margin (mm)
                           and min_support (pixels) have no default
        :param timing:     None, or dict(max_gap=, max_lead=) (seconds; neither has a default): every tick carries one stamp per source and
                           an instant `now`; every track is brought to `now` before tracks are combined, and `smooth` filters over the
                           stamps -- its `rate` is still validated but goes unread (TIMING above)
        :param background: None, or dict(margin=, rel=0.0, min_seen=1), for ALL sources: a learned per-pixel background is removed from
                           every frame as the plan's first step (BACKGROUND above); margin (mm) has no default.  With
                           adapt=dict(persist=, guard=, every=1) among its keys the models are kept current while tracking, by the
                           same launch (ADAPTATION above); persist (ticks) and guard (pixels) have no default
        """
        self.rt = rt
        tracks = [(int(s), bool(r)) for s, r in tracks]
        if not tracks:
            raise ValueError("MultiTracker needs at least one track")
        srcs = [s for s, _ in tracks]
        self.T = T = len(srcs)
        self.C = C = int(max(srcs) + 1 if sources is None else sources)
        self.src_host = ops.track_index(srcs, C)                             # the kernels trust it: checked here
        if C > T:
            raise ValueError("%d sources for %d tracks: every source needs a track that reads it" % (C, T))
        if groups is not None and extrinsics is None:
            raise ValueError("groups needs extrinsics: one (R, t) per source")
        if max_dev is not None and not (np.isfinite(max_dev) and max_dev > 0.):
            raise ValueError("max_dev is None or a distance > 0 (mm): %r" % (max_dev,))
        cal = None
        if calibrate is not None:
            cal = dict(anchor=0, max_shape_dev=None, min_cond=0.)
            if set(calibrate) - set(cal):
                raise ValueError("calibrate takes anchor, max_shape_dev and min_cond, not %r" % sorted(set(calibrate) - set(cal)))
            cal.update(calibrate)
            if groups is None:
                raise ValueError("calibrate needs groups: the pairs come from the tracks of one hand in two sources")
            if cal['max_shape_dev'] is not None and not (np.isfinite(cal['max_shape_dev']) and cal['max_shape_dev'] > 0.):
                raise ValueError("max_shape_dev is None or a distance > 0 (mm): %r" % (cal['max_shape_dev'],))
            if not (np.isfinite(cal['min_cond']) and cal['min_cond'] >= 0.):
                raise ValueError("min_cond is a ratio >= 0: %r" % (cal['min_cond'],))
        self.max_dev, self.handover = None if max_dev is None else float(max_dev), bool(handover)
        self.smooth = None if smooth is None else ops.smooth_spec(smooth)
        self.visibility = None if visibility is None else ops.visibility_spec(visibility)
        self.timing = None if timing is None else ops.timing_spec(timing)
        importers = self._per_source(importer, C, 'importer')
        Hs, Ws = self._per_source(H, C, 'H'), self._per_source(W, C, 'W')
        if any(int(h) != h or int(w) != w or h < 1 or w < 1 for h, w in zip(Hs, Ws)):
            raise ValueError("frame sizes must be positive integers: H %r, W %r" % (Hs, Ws))
        self.sizes = [(int(h), int(w)) for h, w in zip(Hs, Ws)]
        self.importers, self.cams = importers, [camera_tuple(di) for di in importers]
        self.fxs = [abs(float(di.fx if f is None else f)) for di, f in zip(importers, self._per_source(fx, C, 'fx'))]
        self.fys = [abs(float(di.fy if f is None else f)) for di, f in zip(importers, self._per_source(fy, C, 'fy'))]
        if any(v == 0. or not np.isfinite(v) for cam in self.cams for v in cam[:2]) or any(v == 0. or not np.isfinite(v) for v in self.fxs + self.fys):
            raise ValueError("a source needs focal lengths other than zero: cameras %r, fx %r, fy %r" % (self.cams, self.fxs, self.fys))
        # all entries equal: the homogeneous path -- the camera and the frame size as launch arguments, no table
        self.hetero = len(set(zip(self.sizes, self.cams, self.fxs, self.fys))) > 1
        self.importer, self.cam, self.fx, self.fy = importers[0], self.cams[0], self.fxs[0], self.fys[0]
        self.H, self.W = (None, None) if self.hetero else self.sizes[0]
        self.ceng = _engine(comrefNet, rt, 'comrefNet', T, "one row per track")
        self.peng = _engine(poseNet, rt, 'poseNet', T, "one row per track")
        if len(self.peng.x_ins) != 1 or self.peng.out_dim % 3:
            raise ValueError("the pose net takes one crop and regresses J x 3 coordinates")
        self.rs, self.ds, self.J = int(self.ceng.x_ins[0].shape[1]), int(self.peng.x_in.shape[1]), self.peng.out_dim // 3
        f32, i32 = np.float32, np.int32
        self.sensor = None if sensor is None else ops.sensor_spec(sensor)
        if self.hetero:                                                            # ragged buffers; _slice(buf, c) is source c's frame
            self.table = ops.SourceTable(rt, self.cams, list(zip(self.fxs, self.fys)), self.sizes,
                                         None if sensor is None else self.sensor[0].itemsize)
            self.frames = self._ragged(False)
            self.raw = None if sensor is None else self._ragged(True)
        else:
            self.table = None
            self.frames = rt.alloc((C, self.H, self.W), f32, zero=False)
            self.raw = None if sensor is None else rt.alloc((C, self.H, self.W), self.sensor[0], zero=False)
        self.inputs = self.frames if sensor is None else self.raw                 # what the host uploads into
        self._inputs2 = self._frames2 = self._gate2 = None                         # process_sequence's second set, made when first used
        self.partial = ops.frame_range_workspace(rt, C)
        self._pstride = self.partial.size // C
        self.background = None if background is None else ops.background_spec(background)
        # near, seen, cut and take in the frames' own layout (with a table: the ragged one)
        self.bg = None if background is None else ops.BackgroundModel(rt, background, C, self.H, self.W, table=self.table)
        self.adapt = None if self.bg is None or self.bg.adapt is None else AdaptClock(rt, C, self.bg.adapt[2])
        self._learn = None
        self.rec = rt.alloc(T * rt.lib.dpp_crop_record_bytes(), np.uint8)
        self.cube = rt.alloc((T, 3), f32)
        ix = rt.alloc((3, T), i32)                                                 # src, gate (all zero: nobody has started), tflags
        self.src, self.gate, self.tflags = ix.view(0, (T,)), ix.view(T, (T,)), ix.view(2 * T, (T,))
        self.src.set(self.src_host)
        self.trackset = ops.TrackSet(T, self.src, self.gate, self.tflags, self.table)    # what the plan's launches know about their rows
        # everything the host reads per tick is ONE block, every entry an array over the tracks (the launches write [T][...] arrays)
        fields = track_fields(T, self.J)
        self.rig = None if groups is None else ops.FuseRig(rt, extrinsics, groups, self.src_host, C,   # validated there, uploaded once
                                                           anchor=None if cal is None else cal['anchor'])
        self.cal_src, self.acc = [], None
        if cal is not None and self.rig.pending:        # the sums are a buffer of their own: the per-tick download does not grow
            self.anchor, self.max_shape_dev, self.min_cond = self.rig.anchor, cal['max_shape_dev'], float(cal['min_cond'])
            self.cal_src = list(self.rig.pending)
            self.acc = rt.alloc((len(self.cal_src), ops.CALIB_SLOTS), np.float64)
        if self.rig is not None:                                                   # the fused arrays follow: every offset above keeps its value
            G = self.rig.G
            fields += [('fused_pose', (G, self.J, 3), f32), ('fused_com', (G, 3), f32), ('spread', (G, self.J), f32), ('n', (G,), i32),
                       ('peer_com', (T, 3), f32), ('fstat', (T,), i32)]
        self.sstate = None
        if self.smooth is not None:                                                # behind everything else; the state is a buffer of its own
            G = 0 if self.rig is None else self.rig.G
            fields += smooth_fields(T, self.J, G)
            self.sstate = ops.SmoothState(rt, T + G, self.J, timed=self.timing is not None)
        if self.visibility is not None:                                            # behind smooth's as well
            fields += visibility_fields(T, self.J, 0 if self.rig is None else self.rig.G)
        self.astate = self.stamps = self._stamps2 = self.now = None
        if self.timing is not None:                                                # behind visibility's as well; the state is a buffer of its own
            fields += timing_fields(T, self.J)
            self.astate = ops.AlignState(rt, T, self.J)
            self.stamps = rt.alloc((C + 1,), np.float64)                           # one stamp per source, then `now`: the tick's one new upload
        self.block = blk = ResultBlock(rt, fields)
        self.res, self._off = blk.buf, blk.offsets
        self.fused = []
        if self.rig is not None:
            self.fused_pose, self.fused_com, self.spread = blk.view('fused_pose'), blk.view('fused_com'), blk.view('spread')
            self.fused_n, self.peer_com, self.fstat = blk.view('n'), blk.view('peer_com'), blk.view('fstat')
        self.pose3d, self.pose_img, self.com, self.com3d = blk.view('pose'), blk.view('pose_img'), blk.view('com'), blk.view('com3D')
        self.M, self.status = blk.view('M'), blk.view('status')
        self.crop = self.peng.x_in.buf.reshape(T, self.ds, self.ds)             # the pose net's input IS the final crops
        self.flags_host = np.zeros(T, i32)
        self.flags_host[:] = (ops.POSE_INV_X if invX else 0) | (ops.POSE_INV_Y if invY else 0)
        for t, (_, right) in enumerate(tracks):
            if right:
                self.flags_host[t] |= ops.POSE_HAND_RIGHT
        self.tflags.set(self.flags_host)
        self.gate_host = np.zeros(T, i32)                                          # what the device holds
        self.lost = np.ones(T, bool)                                               # no centre yet
        self.cube_host = np.zeros((T, 3), f32)
        self.com_host = np.zeros((T, 3), f32)                                      # the centres as last downloaded (or reset)
        for t in range(T):
            self.set_cube(t, cube)
        self._plans = {}
        self._detectors = {}
        self.runs = 0

    @staticmethod
    def _per_source(v, C, what):
        """A scalar means "the same for all sources"; a sequence has one entry per source."""
        if isinstance(v, (list, tuple, np.ndarray)):
            if len(v) != C:
                raise ValueError("%d entries of %s for %d sources" % (len(v), what, C))
            return list(v)
        return [v] * C

    def _ragged(self, raw, zero=False):
        """A ragged buffer for one frame of every source: float32 frames, or (raw) frames of the sensor's type."""
        if raw:
            return self.rt.alloc((self.table.raw_elems,), self.sensor[0], zero=zero)
        return self.rt.alloc((self.table.frame_elems,), np.float32, zero=zero)

    def _slice(self, buf, c, raw=False):
        """Source c's frame in a frame buffer as a (1, H, W) view (raw: the buffer is a raw sensor buffer, whose offsets differ)."""
        H, W = self.sizes[c]
        if not self.hetero:
            return buf.view(c * H * W, (1, H, W))
        return buf.view(int(self.table.host['raw_off' if raw else 'frame_off'][c]), (1, H, W))

    def _input(self, c, slot=0):
        return self._slice(self.inputs if slot == 0 else self._inputs2, c, raw=self.sensor is not None)

    # ---- device state -----------------------------------------------------------------------------------------------------
    def _track(self, t):
        t = int(t)
        if not 0 <= t < self.T:
            raise IndexError("track %d of %d" % (t, self.T))
        return t

    def reset(self, t, com):
        """Start track t (again) from the centre `com` (image coordinates of its source, z in mm)."""
        t = self._track(t)
        com = np.asarray(com, np.float32).reshape(3)
        if not valid_centre(com):
            raise ValueError("reset needs a centre with a depth: %r" % (com,))
        self.com.view(3 * t, (1, 3)).set(com)
        self.com_host[t] = com
        self.lost[t] = False
        self._clear_row(t)

    def _clear_row(self, t):
        """A restart or another hand: what track t follows now is not what was filtered (one 4-byte upload of since[t] = -1) nor what
        its velocity was taken from (with `timing`, one of have[t] = 0)."""
        if self.sstate is not None:
            self.sstate.clear(t)
        if self.astate is not None:
            self.astate.clear(t)
        if self.adapt is not None:                      # the window the device holds for t is not this hand's: its source sits one tick out
            self.adapt.restart(self.src_host[t])

    def drop(self, t):
        """Mark track t lost: the application knows what the tracker cannot see (the only loss test is a centre at depth 0) -- its
        camera is covered, the hand left.  The track is gated until reset / acquire, or, in a group, until its peers have the hand."""
        self.lost[self._track(t)] = True

    def set_cube(self, t, cube):
        t = self._track(t)
        cube = np.asarray(cube, np.float32).reshape(3)
        if not (cube > 0).all():
            raise ValueError("the cube must have a positive size: %r" % (cube,))
        self.cube.view(3 * t, (1, 3)).set(cube)
        self.cube_host[t] = cube

    def set_hand(self, t, right):
        """HAND_RIGHT mirrors track t's pose-net input and the x coordinate of its output: a rewrite of tflags[t], not a new plan."""
        t = self._track(t)
        flags = (self.flags_host[t] & ~ops.POSE_HAND_RIGHT) | (ops.POSE_HAND_RIGHT if right else 0)
        if flags != self.flags_host[t]:
            self._clear_row(t)
        self.flags_host[t] = flags
        self.tflags.set(self.flags_host)

    def detector(self, t):
        """The whole-frame detector at B = 1 on views of track t's buffers: its source's frame (and raw frame), that frame's
        depth-range partials, the track's centre (the detector's output) and cube."""
        t = self._track(t)
        if t not in self._detectors:
            from .detect import FrameDetector
            c = int(self.src_host[t])
            (H, W) = self.sizes[c]
            self._detectors[t] = FrameDetector(
                self.rt, H, W, self.fxs[c], self.fys[c], 1, frames=self._slice(self.frames, c),
                partial=self.partial.view(c * self._pstride, (self._pstride,)), com=self.com.view(3 * t, (1, 3)),
                cube=self.cube.view(3 * t, (1, 3)), res=self.block.view('det'), sensor=self.sensor,
                raw=None if self.sensor is None else self._slice(self.raw, c, raw=True), **self._cut(c))
        return self._detectors[t]

    def _cut(self, c):
        """What a detector of source c is handed beside its frame: the background options and a view of the source's cut map."""
        return {} if self.bg is None else dict(background=self.background, cut=self.bg.view(self.bg.cut, c))

    # ---- the learned background ---------------------------------------------------------------------------------------------
    def _model(self):
        if self.bg is None:
            raise RuntimeError("the tracker was built without background=")
        return self.bg

    def learn_background(self, frames):
        """One frame per source of the scene WITHOUT hands into the sources' models, None where a source sits out (raw frames with a
        sensor: what is learned is frame_ingest's output): one upload per frame (and of `take`, when it differs from the last call's),
        a plan of its own ([frame_ingest], background_learn), then the cut maps of the sources that took part -- a download of the
        model, the map on the host, an upload.  Not on the per-tick path."""
        bg = self._model()
        if len(frames) != self.C:
            raise ValueError("%d frames for %d sources" % (len(frames), self.C))
        fresh = [None if f is None else self._frame(f, c) for c, f in enumerate(frames)]
        if self._learn is None:
            rt, p = self.rt, ops.Plan('learn_background')
            if self.sensor is not None:
                p.add(ops.frame_ingest(rt, self.raw, self.C, self.H, self.W, self.frames, None, median=self.sensor[1], mirror=self.sensor[2],
                                       table=self.table))
            p.add(ops.background_learn(rt, self.frames, bg.take, self.C, self.H, self.W, bg.near, bg.seen, table=self.table))
            self._learn = p
        for c, f in enumerate(fresh):
            if f is not None:
                self._input(c).set(f)
        bg.set_take([int(f is not None) for f in fresh])
        self._learn.run(self.rt)
        self.rt.synchronize()
        for c, f in enumerate(fresh):
            if f is not None:
                bg.refresh(c)
                bg.forget_candidates(c)

    def background_model(self, c=None):
        """dict(near, seen, cut) of source c ((H, W) arrays of its size), or the list of all sources' without c.  With adapt these are
        the adapted ones."""
        self.rt.synchronize()
        bg = self._model()
        return [bg.get(s) for s in range(self.C)] if c is None else bg.get(c)

    def set_background_model(self, c, model):
        """Load dict(near=, seen=) as background_model(c) returned it into source c (the cut map is computed with THIS tracker's options)."""
        self.rt.synchronize()
        self._model().set(c, model['near'], model['seen'])

    def clear_background(self, c=None):
        """Forget the model of source c (or of all): until something is learned again the source is that of a tracker without the option."""
        self.rt.synchronize()
        self._model().clear(c)

    def acquire(self, t, frame, do_hand_size=False):
        """Find a hand in `frame` of track t's source and start track t (again) from it, as HandTracker.acquire does: one upload, the
        detector plan, one download of the result block.  The detector finds the NEAREST object of the frame: of two hands on one
        source it finds the same one for both tracks; acquire_source(c, frame) finds both and shares them out.  Returns
        dict(com, cube, found); not found: the centre is (0, 0, 0) and the track stays lost."""
        t = self._track(t)
        c = int(self.src_host[t])
        frame = self._frame(frame, c)
        det = self.detector(t)
        self._input(c).set(frame)
        det.plan(do_hand_size).run(self.rt)
        self.rt.synchronize()
        res = self.block.split(self.res.get())
        coms, cubes, found, _, _ = det.parse(res['det'], res['com'][t], None if do_hand_size else self.cube_host[t])
        ok = bool(found[0]) and valid_centre(coms[0])
        self.lost[t] = not ok
        self.com_host[t] = coms[0]
        if ok:                                                                     # a restart, as reset(t, com) is
            self._clear_row(t)
        elif self.adapt is not None:
            self.adapt.restart(c)
        return dict(com=coms[0], cube=cubes[0], found=ok)

    def source_detector(self, c, max_extent=None):
        """(detector, tracks of source c).  The several-hands detector of source c at B = 1, hands = the number of tracks that read c: on views of the source's frame
        (and raw frame) and partials, with a result block of its own that also holds the K centres -- they go to the tracks through
        reset(t, com), not through the plan.  The K detections share ONE cube, that of the source's first track."""
        c = int(c)
        ts = [t for t in range(self.T) if self.src_host[t] == c]
        if not 0 <= c < self.C or not ts:
            raise IndexError("source %d of %d" % (c, self.C))
        key = ('source', c, float(max_extent) if max_extent else 0.0)
        if len(ts) == 1 and not max_extent:                                   # nothing to share out: track ts[0]'s own detector
            return self.detector(ts[0]), ts
        if key not in self._detectors:
            from .detect import FrameDetector
            (H, W) = self.sizes[c]
            self._detectors[key] = FrameDetector(
                self.rt, H, W, self.fxs[c], self.fys[c], 1, frames=self._slice(self.frames, c),
                partial=self.partial.view(c * self._pstride, (self._pstride,)), cube=self.cube.view(3 * ts[0], (1, 3)), sensor=self.sensor,
                raw=None if self.sensor is None else self._slice(self.raw, c, raw=True), hands=len(ts), max_extent=max_extent,
                **self._cut(c))
        return self._detectors[key], ts

    def acquire_source(self, c, frame, max_extent=None, order='near'):
        """Find the hands of source c in `frame` and start its tracks from them: one upload, ONE detector plan at K = the number of
        tracks that read c, one download.  The detections (hipdp.detect, hands=K: nearest slab first, then raster-first; max_extent
        as there) are refined with the cube of the source's first track and handed out on the host:
          - a track that is being followed keeps its centre and claims the found detection nearest to its last downloaded centre in
            image (x, y) (Euclidean, float64, ties to the lower slot), so that its hand is not given to another track;
          - the lost tracks, in ascending t, take the remaining found detections in slot order (order='near') or in ascending
            refined-centre x (order='x': left to right); each is started with reset(t, com);
          - a track left without a detection stays lost.
        Returns one dict(com, cube, found) per track of the source, in ascending t (a followed track: its own centre, found True)."""
        if order not in ('near', 'x'):
            raise ValueError("order is 'near' or 'x', not %r" % (order,))
        det, ts = self.source_detector(c, max_extent)
        c = int(c)
        frame = self._frame(frame, c)
        if not det.multi:                                                     # one track, no extent filter: acquire's plan, acquire's bits
            t = ts[0]
            if self.lost[t]:
                return [self.acquire(t, frame)]
            self._input(c).set(frame)
            return [dict(com=self.com_host[t].copy(), cube=self.cube_host[t].copy(), found=True)]
        self._input(c).set(frame)
        det.plan(False).run(self.rt)
        self.rt.synchronize()
        coms, _, found = det.parse(det.res.get(), None, self.cube_host[ts[0]])[:3]
        coms, found = coms[0], found[0]
        ok = [bool(found[k]) and valid_centre(coms[k]) for k in range(len(ts))]
        free = [k for k in range(len(ts)) if ok[k]]
        out = {}
        followed = [t for t in ts if not self.lost[t]]
        if followed:
            last = self.com_host.astype(np.float64)
            for t in followed:
                if free:
                    d = [np.hypot(np.float64(coms[k][0]) - last[t][0], np.float64(coms[k][1]) - last[t][1]) for k in free]
                    free.pop(int(np.argmin(d)))                               # argmin: the first (lowest slot) of equal distances
                out[t] = dict(com=last[t].astype(np.float32), cube=self.cube_host[t].copy(), found=True)
        if order == 'x':
            free.sort(key=lambda k: (float(coms[k][0]), k))
        for t in ts:
            if t in out:
                continue
            if free:
                k = free.pop(0)
                self.reset(t, coms[k])
                out[t] = dict(com=coms[k].copy(), cube=self.cube_host[t].copy(), found=True)
            else:
                out[t] = dict(com=np.zeros(3, np.float32), cube=self.cube_host[t].copy(), found=False)
        return [out[t] for t in ts]

    # ---- calibration ------------------------------------------------------------------------------------------------------
    @property
    def calibrating(self):
        """A source still waits for its (R, t): the tick ends in extrinsics_accumulate, nothing is fused or handed over."""
        return self.rig is not None and bool(self.rig.pending)

    def calibration_report(self):
        """{source: calib.solve_rigid of its sums so far} for every source that is being calibrated: one download of
        len(cal_src) x 160 bytes, one 3 x 3 SVD each.  Nothing changes."""
        from .calib import solve_rigid
        if not self.calibrating:
            raise RuntimeError("no source is being calibrated")
        self.rt.synchronize()
        rows = self.acc.get()
        return dict((c, solve_rigid(rows[k], self.min_cond)) for k, c in enumerate(self.cal_src))

    def finish_calibration(self):
        """calibration_report(), and where EVERY source's fit is ok: the fits become the rig's extrinsics (one small upload each) and the
        plan is rebuilt -- from the next tick on this is the tracker that was constructed with them.  Otherwise nothing changes, and the
        caller goes on feeding ticks (or reset_calibration()).  Returns the report."""
        report = self.calibration_report()
        if all(r['ok'] for r in report.values()):
            for c in list(self.cal_src):
                self.rig.set_extrinsics(c, report[c]['R'], report[c]['t'])
            self._plans = {}
        return report

    def reset_calibration(self):
        """Forget the pairs summed so far."""
        if self.acc is None:
            raise RuntimeError("no source is being calibrated")
        self.rt.synchronize()
        self.acc.set(np.zeros(self.acc.shape, np.float64))

    # ---- the per-tick plan --------------------------------------------------------------------------------------------------
    def _second_set(self):
        """process_sequence's second set of input buffers (and of gates): made the first time a sequence runs, so a tracker that only
        ever ticks allocates what it always did.  Zeroed: an idle source's slice is read by the depth-range pass before anything
        was uploaded into it."""
        if self._inputs2 is None:
            if self.hetero:
                self._inputs2 = self._ragged(self.sensor is not None, zero=True)
            else:
                self._inputs2 = self.rt.alloc((self.C, self.H, self.W), np.float32 if self.sensor is None else self.sensor[0])
            self._gate2 = self.rt.alloc((self.T,), np.int32)
            self._gate2_host = np.zeros(self.T, np.int32)
            self._trackset2 = ops.TrackSet(self.T, self.src, self._gate2, self.tflags, self.table)
            if self.timing is not None:                                            # the set's own stamps, uploaded with its frames
                self._stamps2 = self.rt.alloc((self.C + 1,), np.float64)

    def plan(self, slot=0):
        """The plan of one tick on input set `slot` (1: process_sequence's second set; without a sensor the second set IS a second
        frame buffer, with one the raw frames alone are doubled: the float32 frames are written and read inside one plan)."""
        if slot not in self._plans:
            rt, H, W, T, C = self.rt, self.H, self.W, self.T, self.C
            if slot:
                self._second_set()
            tracks = self._trackset2 if slot else self.trackset           # the slot's own gates; with a table H, W, cam, fx, fy go unread
            fr = self._inputs2 if slot and self.sensor is None else self.frames
            raw = self._inputs2 if slot else self.raw
            p = ops.Plan('multitrack')
            # frame_range; with a sensor frame_ingest in its place; with a background frame_background, which then writes the partials
            # ... and with adapt the adapting cut in ITS place: the windows track_refine left in `rec` in the last tick are kept out
            adapt = None if self.adapt is None else dict(bg=self.bg, take=self.adapt.buf(slot), records=self.rec, T=T, src=self.src)
            for op in frame_stage(rt, fr, raw, C, H, W, self.partial, self.sensor, None if self.bg is None else self.bg.cut, table=self.table,
                                  adapt=adapt):
                p.add(op)
            # the T centres are read (prepare, track_refine) and then rewritten by one lane per track of track_refine: in place
            for op, side in refine_stage(rt, fr, H, W, self.partial, self.rec, self.com, self.cube, self.ceng, self.cam, self.fx, self.fy,
                                         self.ds, self.com, self.com3d, self.rec, self.status, self.M, tracks=tracks):
                p.add(op, side)
            p.add(ops.crop_warp_ex(rt, fr, self.rec, T, H, W, self.ds, self.crop, flags=ops.CROP_NORMALIZE, nd_value=0.0, name='track_crop',
                                   tracks=tracks))
            for op, side in self.peng.fwd.ops:
                p.add(op, side)
            p.add(ops.pose_finish(rt, self.peng.out.buf, T, self.J, self.cube, self.com3d, self.cam, None, self.pose3d, self.pose_img,
                                  tracks=tracks))
            weighted = {}
            if self.visibility is not None:             # reads the slot's float32 frames, which nothing in the plan writes behind the first launch
                blk = self.block
                p.add(ops.joint_visibility(rt, self.pose_img, self.status, self.src, T, self.J, fr, C, self.visibility, blk.view('vis'),
                                           blk.view('vis_weight'), blk.view('vis_class'), table=self.table, H=H, W=W))
                if self.rig is not None:
                    weighted = dict(weight=blk.view('vis_weight'), fused_weight=blk.view('fused_weight'), name='pose_fuse_w')
            pose3d, com3d, timed = self.pose3d, self.com3d, {}      # what the launches that COMBINE tracks read
            if self.timing is not None:                 # every track at the tick's instant; both slots move on the ONE state
                blk, stamps = self.block, self._stamps2 if slot else self.stamps
                pose3d, com3d, timed = blk.view('pose_t'), blk.view('com3D_t'), dict(stamps=stamps, C=C)
                p.add(ops.pose_align(rt, self.pose3d, self.com3d, self.status, self.src, T, self.J, stamps, C, self.timing, self.astate,
                                     pose3d, blk.view('pose_img_t'), com3d, blk.view('lead'), blk.view('astat'), cam=self.cam,
                                     table=self.table))
            if self.calibrating:                        # in the fusion launch's place: nothing can be fused or handed over yet
                p.add(ops.extrinsics_accumulate(rt, pose3d, self.status, self.src, T, self.J, self.rig, self.anchor, self.cal_src,
                                                self.max_shape_dev, self.acc))
            elif self.rig is not None:                  # the last launch of the main lane: the next tick's prepare is ordered behind it
                p.add(ops.pose_fuse(rt, pose3d, com3d, self.status, self.src, T, self.J, self.rig, self.table, H, W, self.cam,
                                    self.max_dev, self.handover, self.com, self.fused_pose, self.fused_com, self.spread, self.fused_n,
                                    self.peer_com, self.fstat, **weighted))
            if self.smooth is not None:                 # the last launch of the main lane; both slots filter into the ONE state
                blk, fusing = self.block, self.rig is not None and not self.calibrating
                grp = {}
                if fusing:
                    grp = dict(fused_pose=self.fused_pose, n=self.fused_n, G=self.rig.G, fused_pose_f=blk.view('fused_pose_f'),
                               gstat=blk.view('gstat'))
                p.add(ops.pose_smooth(rt, self.pose3d, self.status, T, self.J, self.smooth, self.sstate, blk.view('pose_f'),
                                      blk.view('pose_img_f'), blk.view('sstat'), cam=self.cam, src=self.src, table=self.table,
                                      **dict(grp, **timed)))  # the tracks' rows filter the UNALIGNED pose at their own stamps
            self._plans[slot] = p
        return self._plans[slot]

    def _frame(self, frame, c=0):
        """`frame` checked against the size of source c (ITS source) and the sensor's dtype."""
        return check_frame(frame, self.sensor, self.sizes[c], 'source %d delivers' % c)

    def _gates(self, fresh):
        """The tick's gate vector: a track takes part when the host does not know it lost and its source has a fresh frame."""
        return np.array([int(not self.lost[t] and fresh[self.src_host[t]] is not None) for t in range(self.T)], np.int32)

    def _results(self, res, gate, crops=None):
        f = self.block.split(res)
        st, pose, pimg, com, com3d, M = f['status'], f['pose'], f['pose_img'], f['com'], f['com3D'], f['M']
        self.com_host[:] = com
        rig = self.rig
        fusing = rig is not None and not rig.pending
        self.fused = []
        if fusing:
            fstat, peer = f['fstat'], f['peer_com']
            self.fused = [dict(pose=f['fused_pose'][g], com=f['fused_com'][g], spread=f['spread'][g], n=int(f['n'][g])) for g in range(rig.G)]
            if self.smooth is not None:
                for g, d in enumerate(self.fused):
                    d.update(pose_f=f['fused_pose_f'][g], smooth=int(f['gstat'][g]))
            if self.visibility is not None:
                for g, d in enumerate(self.fused):
                    d.update(weight=f['fused_weight'][g])
            self._peer_ok = (fstat & ops.FUSE_PEER_OK) != 0
        out = []
        for t in range(self.T):
            status = int(st[t])
            grouped = rig is not None and rig.group_of[t] >= 0
            handed = grouped and fusing and bool(fstat[t] & ops.FUSE_HANDED)
            if not gate[t]:                          # gated because it is lost (or never started): LOST; because its source idles: IDLE
                status = LOST if self.lost[t] else IDLE
            else:
                # handed over on the device: LOST in this tick, but it goes on from its peers' centre.  (Not in the tick that
                # process_sequence runs ungated behind a loss the host had not seen yet: that track is gated in a process() loop.)
                self.lost[t] = status != OK and (bool(self.lost[t]) or not handed)
            d = dict(pose=pose[t], pose_img=pimg[t], com=com[t], com3D=com3d[t], M=M[t], status=status)
            if grouped and not fusing:
                d.update(group=int(rig.group_of[t]))
            elif grouped:
                d.update(group=int(rig.group_of[t]), outlier=bool(fstat[t] & ops.FUSE_OUTLIER), disagree=bool(fstat[t] & ops.FUSE_DISAGREE),
                         handed=handed, peer_com=peer[t])
            if self.smooth is not None:
                d.update(pose_f=f['pose_f'][t], pose_img_f=f['pose_img_f'][t], smooth=int(f['sstat'][t]))
            if self.visibility is not None:
                d.update(vis=f['vis'][t], vis_class=f['vis_class'][t])
            if self.timing is not None:
                d.update(pose_t=f['pose_t'][t], pose_img_t=f['pose_img_t'][t], com3D_t=f['com3D_t'][t], lead=f['lead'][t], align=int(f['astat'][t]))
            if crops is not None:
                d['crop'] = crops[t]
            out.append(d)
        return out

    def _stamps(self, stamps, now, fresh):
        """The tick's stamps checked: None without `timing` (where passing any raises), else the float64 [C + 1] array to upload."""
        if self.timing is None:
            if stamps is not None or now is not None:
                raise ValueError("stamps need a tracker with timing=dict(max_gap=, max_lead=)")
            return None
        return ops.tick_stamps(stamps, now, fresh, self.C)

    def process(self, frames, return_crop=False, stamps=None, now=None):
        """One tick: `frames` has one entry per source, None where that source has no new frame.  The fresh frames are uploaded (one
        upload each; `gate` too, only when it differs from the last tick's), ONE plan runs, ONE block is downloaded.  Returns one
        dict per track with HandTracker.process's keys.  status OK: the track was followed.  IDLE: its source had no frame, its
        centre is unchanged.  LOST: it lost the hand in this tick, or is refused (lost before, or never started) until reset(t,
        com) / acquire(t, frame).  For IDLE and LOST the other entries are finite but meaningless.  With `timing`: `stamps` has one
        finite time (s) per source that delivers a frame, `now` is the instant the combined outputs refer to (default: the largest
        stamp of the fresh frames; kept in self.now), and the C + 1 doubles are the tick's one additional upload."""
        if len(frames) != self.C:
            raise ValueError("%d frames for %d sources" % (len(frames), self.C))
        fresh = [None if f is None else self._frame(f, c) for c, f in enumerate(frames)]
        when = self._stamps(stamps, now, fresh)
        gate = self._gates(fresh)
        for c, f in enumerate(fresh):
            if f is not None:
                self._input(c).set(f)
        if when is not None:
            self.stamps.set(when)
            self.now = float(when[self.C])
        if not np.array_equal(gate, self.gate_host):
            self.gate.set(gate)
            self.gate_host = gate
        if self.adapt is not None:
            self.adapt.step([f is not None for f in fresh], 0)
        self.plan().run(self.rt)
        self.runs += 1
        self.rt.synchronize()
        out = self._results(self.res.get(), gate, self.crop.get() if return_crop else None)
        if self.rig is not None and self.handover and not self.calibrating:
            for t in np.flatnonzero(self.rig.group_of >= 0):
                # gated BECAUSE it is lost, and its peers have the hand now: start it again from their centre (one small upload)
                if not gate[t] and self.lost[t] and self._peer_ok[t]:
                    self.reset(t, out[t]['peer_com'])
        return out

    def process_sequence(self, ticks, return_crops=False):
        """A sequence of ticks (an iterable of per-source frame lists, None for "no frame", as process takes them; with `timing` an
        iterable of (frames, stamps) or (frames, stamps, now), each set's stamps uploaded with its frames): the uploads of
        tick n + 1 run on the copy stream under the plan of tick n (two sets of input buffers, one plan and one `gate` array per
        set, so a plan in flight never sees the next tick's frames or gates), and the result block of tick n is read while tick
        n + 1 is in flight.  Returns one list of per-track dicts per tick, as a process() loop would.

        The host learns one tick late that a track was lost in tick n: the track runs ungated in tick n + 1, where track_refine
        reports it LOST again (its centre is ill-defined), and is gated from tick n + 2 on, as in process().  A lost track stops
        neither the sequence nor the other tracks; nothing is detected inside a sequence.  For every track-tick whose status is OK
        or IDLE every key has the bits of the process() loop; for LOST only the status is promised.  self.lost, com_host, gate_host
        and runs are afterwards what the loop would have left (a lost track's centre is put back to the one it was lost with; a track
        that was handed its peers' centre is not lost and keeps it).  With `groups`, self.fused_ticks holds self.fused of every tick."""
        rt = self.rt
        staged = hasattr(rt, 'staged_upload')
        self._second_set()
        results, pending, free = [], None, [None, None]
        gates = [self.gate, self._gate2]
        lost_com = {}                                   # track -> the centre it was lost with (the tick after overwrites it)

        def resolve(p):
            res, crops, gate = p
            was = self.lost.copy()
            out = self._results(res.get(), gate, crops.get() if crops is not None else None)
            for t in range(self.T):
                if self.lost[t] and not was[t]:
                    lost_com[t] = out[t]['com'].copy()
            results.append(out)
            self.fused_ticks.append(self.fused)
        last = None
        self.fused_ticks = []                           # MultiTracker.fused of every tick of this sequence (empty lists without groups)
        for n, frames in enumerate(ticks):
            stamps = now = None
            if self.timing is not None:
                if not isinstance(frames, tuple) or len(frames) not in (2, 3):
                    raise ValueError("a timed sequence's ticks are (frames, stamps) or (frames, stamps, now)")
                frames, stamps, now = frames if len(frames) == 3 else frames + (None,)
            if len(frames) != self.C:
                raise ValueError("%d frames for %d sources" % (len(frames), self.C))
            fresh = [None if f is None else self._frame(f, c) for c, f in enumerate(frames)]
            when = self._stamps(stamps, now, fresh)
            k = n & 1
            # self.lost is what the host knows: the results up to tick n - 2
            gate = self._gates(fresh)
            events = []
            for c, f in enumerate(fresh):
                if f is not None:
                    if staged:
                        events.append(rt.staged_upload(self._input(c, k), f[None], free[k]))
                    else:
                        self._input(c, k).set(f)
            if when is not None:
                if staged:
                    events.append(rt.staged_upload(self._stamps2 if k else self.stamps, when, free[k]))
                else:
                    (self._stamps2 if k else self.stamps).set(when)
                self.now = float(when[self.C])
            if not np.array_equal(gate, self._gate2_host if k else self.gate_host):   # the set's own gates: its last plan is behind us
                gates[k].set(gate)
                if k:
                    self._gate2_host = gate
                else:
                    self.gate_host = gate
            plan = self.plan(k)
            if self.adapt is not None:
                self.adapt.step([f is not None for f in fresh], k)
            for ev in events:
                rt.wait_event(ev)
            plan.run(rt)
            self.runs += 1
            free[k] = rt.record_event() if staged else None
            handle = (rt.read_async(self.res), rt.read_async(self.crop) if return_crops else None, gate)
            if pending is not None:
                resolve(pending)
            pending = handle
            # the gates a process() loop would have used for this tick: it knows tick n - 1's losses already
            last = self._gates(fresh)
        if pending is not None:
            resolve(pending)
        rt.synchronize()
        if last is not None and not np.array_equal(last, self.gate_host):      # process() reads set 0: leave it what the loop would have
            self.gate.set(last)
            self.gate_host = last
        for t, com in lost_com.items():
            if self.lost[t]:
                self.com.view(3 * t, (1, 3)).set(com)
                self.com_host[t] = com
        return results
