"""
Whole-frame hand detection on the device: a depth frame in, the centre of the nearest sufficiently large object (and, on request,
the metric cube of the hand) out, ONE launch plan per batch of frames, no host round trip inside it.

What the reference's HandDetector.detect (/root/reference/src/util/handdetector.py:569-632) takes from cv2.findContours is restated
with 8-connected component labelling (csrc/components.hip):

    frame_range                                   the frames' depth ranges (shared with the tracker's plan)
    slab_keys                                     the 20 depth slabs of :576-582 as one uint8 key per pixel
    label_components (+ statistics)               canonical labels: the smallest linear index of each component; count, box, sums
    detect_seed                                   nearest slab's raster-first component of more than 200 px; calculateCoM of the
                                                  +-100 px window around its centroid inside that slab (:589-607)
    refine_com_iterative(5)                       :610, the tracker's kernel, unchanged
    -- with do_hand_size --
    mask_keys                                     d != 0 and com_z - cube_z / 2 <= d <= com_z + cube_z / 2 (:616-619)
    label_components (+ statistics)               the same kernels on the binary key
    hand_size                                     the largest component's bounding box through estimateHandsize (:911-937)

Three deviations from the reference, all forced by leaving cv2 out: pixel count instead of contourArea; raster-first instead of
cv2's contour order; a depth exactly on a slab boundary belongs to the nearer slab only.

SEVERAL HANDS.  FrameDetector(hands=K, max_extent=) returns up to K hands per frame from the SAME labelling, in a plan of one launch
more: comp_candidates + detect_select + detect_seeds (ops.detect_seeds) stand where comp_select + detect_seed stood, and
refine_com_iterative_ix refines the K seeds of a frame against the frame's cube.

    candidates      the components of more than 200 px in (key, root) order: nearest slab first, then raster-first
    extent filter   (this project's rule) with max_extent (mm) a candidate wider or higher than that at its slab's far bound is dropped:
                    (xmax - xmin + 1) * b_{key+1} / fx > max_extent, likewise in y -- a far wall is not the second hand
    selection       (this project's rule) greedy in that order: a candidate whose centroid lies in the +-100 px seed window of an accepted
                    one is suppressed -- one hand reaching across a slab boundary is two components -- and suppresses nothing itself
    seeds, centres  per accepted candidate exactly what detect_seed / refine_com_iterative(5) give for the one winner

hands=1 without max_extent is the one-hand plan above, launch for launch.  Hand size is a one-hand procedure (it would take K labelling
passes and K workspaces of 40 bytes per pixel): do_hand_size with hands > 1 raises ValueError.

With sensor=dict(dtype=, median=, mirror=) the frames handed to run() are RAW sensor frames: frame_ingest (csrc/ingest.hip) converts,
mirrors and median-filters them into the float32 frame buffer and writes the depth-range partials, in frame_range's place.

BACKGROUND.  The nearest object of more than 200 px is a desk edge, a monitor or the user's torso wherever one is nearer than the hand.
FrameDetector(background=dict(margin=, rel=0.0, min_seen=1)) cuts a learned per-pixel background from the frames first (hipdp/tracker.py,
BACKGROUND; csrc/background.hip): frame_background keeps a depth only where it is not 0 and strictly below its cut, in place, and
writes the depth-range partials of what it kept, so the slabs, the labelling, the seed window, the refinement and the hand size all
work on the masked frame.  stage(with_range=True) opens with frame_background instead of frame_range -- behind a frame_ingest without
partials where there is a sensor.  A tracker's detectors take views of the tracker's cut map (cut=); a detector of its own owns a model
(self.bg) whose cut map is +inf, the neutral element, until something was learned.  Out of scope: updating the model while tracking,
per-source options, a cut inside the ingest kernel, the host HandDetector API, morphological clean-up of the mask, mixed pixels at
object edges, choosing margin / rel for a sensor.
"""
import numpy as np

from . import ops

NUM_REFINE_ITER = 5                 # handdetector.py:610


class FrameDetector(object):
    def __init__(self, rt, H, W, fx, fy, B=1, frames=None, partial=None, com=None, cube=None, res=None, sensor=None, raw=None, hands=1,
                 max_extent=None, background=None, cut=None):
        """
        :param H, W:    frame size
        :param fx, fy:  what the reference hands to HandDetector
        :param B:       frames per run
        :param frames, partial, com, cube: device buffers of an owner whose state the plan works on (HandTracker: its frame buffer,
                        its depth-range partials, its centre -- the plan's final centre lands there -- and its cube); by default own
        :param res:     8 * B float32 of an owner's result block for seed / cube out / status (so that the owner reads ONE block)
        :param sensor:  None, or dict(dtype='uint16' | 'float32', median=bool, mirror=bool): run() takes raw frames of that dtype
        :param raw:     with a sensor: the owner's raw frame buffer (B, H, W) of the sensor's dtype; by default own
        :param hands:   K, the number of hands looked for per frame (1 .. 16).  With K > 1 (or a max_extent) centres and seeds are
                        (B * K, 3), row b * K + k the k-th hand of frame b; the cubes stay (B, 3): the hands of a frame share its cube;
                        an own result block then also holds the centres and the per-slot report (key, count, box), so that the host
                        reads ONE block; res, when given, has 14 * B * K words, com (B * K, 3).  Hand size is measured for one hand only
        :param max_extent: None / 0, or the largest metric width and height (mm) a component may have to be a hand
        :param background: None, or dict(margin=, rel=0.0, min_seen=1): a learned background is cut from the frames first (BACKGROUND above)
        :param cut:     with a background: the owner's cut map (B, H, W) (a tracker hands a view of its own); by default the map of an own
                        model, self.bg (an ops.BackgroundModel: learn through ops.background_learn, then bg.refresh())
        """
        self.rt, self.B, self.H, self.W = rt, int(B), int(H), int(W)
        self.K = int(hands)
        if not 1 <= self.K <= ops.DETECT_MAX_HANDS:
            raise ValueError("hands must be 1 .. %d, not %r" % (ops.DETECT_MAX_HANDS, hands))
        self.max_extent = float(max_extent) if max_extent else 0.0
        if not 0.0 <= self.max_extent < np.inf:
            raise ValueError("max_extent must be a finite size in mm, not %r" % (max_extent,))
        self.multi = self.K > 1 or self.max_extent > 0.0                  # the several-hands launches and result block
        self.fx, self.fy = abs(float(fx)), abs(float(fy))
        f32 = np.float32
        self.frames = frames if frames is not None else rt.alloc((self.B, self.H, self.W), f32, zero=False)
        self.sensor = None if sensor is None else ops.sensor_spec(sensor)
        self.raw = None
        if self.sensor is not None:
            self.raw = raw if raw is not None else rt.alloc((self.B, self.H, self.W), self.sensor[0], zero=False)
        self.partial = partial if partial is not None else ops.frame_range_workspace(rt, self.B)
        self.background = None if background is None else ops.background_spec(background)
        self.bg = self.cut = None
        if self.background is not None:
            if cut is None:
                self.bg = ops.BackgroundModel(rt, self.background, self.B, self.H, self.W)
            self.cut = cut if cut is not None else self.bg.cut
        elif cut is not None:
            raise ValueError("a cut map needs the background options it was computed with")
        self.cube = cube if cube is not None else rt.alloc((self.B, 3), f32)
        self.ws = ops.ComponentWorkspace(rt, self.B, self.H, self.W, candidates=self.multi)
        self._plans = {}
        if self.multi:
            # ONE block: seeds, cubes out, found / hand-size status, refinement status, report -- and, unless an owner holds them, the centres
            N = self.N = self.B * self.K
            self._com_in_res = com is None and res is None
            self.res = res if res is not None else rt.alloc((17 if com is None else 14) * N, f32)
            self.com = com if com is not None else (self.res.view(14 * N, (N, 3)) if self._com_in_res else rt.alloc((N, 3), f32))
            self.seed, self.cube_out = self.res.view(0, (N, 3)), self.res.view(3 * N, (N, 3))
            self.status, self.rstatus = self.res.view(6 * N, (N,), np.int32), self.res.view(7 * N, (N,), np.int32)
            self.report = self.res.view(8 * N, (N, 6), np.int32)
            self.src = None
            if self.K > 1:                                                   # row r works on frame r // K: uploaded once
                self.src = rt.alloc((N,), np.int32, zero=False)
                self.src.set(ops.track_index(np.arange(N) // self.K, self.B))
            return
        self.N = self.B
        self.com = com if com is not None else rt.alloc((self.B, 3), f32)
        # what the host reads per run besides the centre, ONE block: seed, cube out, found / hand-size status, refinement status
        self.res = res if res is not None else rt.alloc(8 * self.B, f32)
        self.seed, self.cube_out = self.res.view(0, (self.B, 3)), self.res.view(3 * self.B, (self.B, 3))
        self.status, self.rstatus = self.res.view(6 * self.B, (self.B,), np.int32), self.res.view(7 * self.B, (self.B,), np.int32)

    def stage(self, do_hand_size=False, with_range=True):
        """The detector's launches in order (steps a-f of the module docstring); with_range=False when the caller's plan has already
        run frame_range (or frame_ingest) on these frames."""
        rt, B, H, W, fr, ws = self.rt, self.B, self.H, self.W, self.frames, self.ws
        if do_hand_size and self.K > 1:
            raise ValueError("hand size is measured for one hand per frame: do_hand_size needs hands=1")
        out = [ops.frame_range(rt, fr, B, H, W, self.partial)] if with_range else []
        if with_range and self.cut is not None:     # the same launch(es) a tracker's plan opens with: [frame_ingest,] frame_background
            from .tracker import frame_stage
            out = frame_stage(rt, fr, self.raw, B, H, W, self.partial, self.sensor, self.cut)
        if self.multi:
            out += [ops.slab_keys(rt, fr, self.partial, ws),
                    ops.label_components(rt, ws),
                    ops.detect_seeds(rt, fr, self.partial, ws, self.K, self.seed, self.status, self.report, max_extent=self.max_extent,
                                     fx=self.fx, fy=self.fy),
                    ops.refine_com_iterative_ix(rt, fr, self.partial, self.N, self.src, H, W, self.seed, self.cube, self.fx, self.fy,
                                                NUM_REFINE_ITER, self.com, self.rstatus, name='detect_refine')]
            return out + (self.hand_size_stage() if do_hand_size else [])
        out += [ops.slab_keys(rt, fr, self.partial, ws),
                ops.label_components(rt, ws),
                ops.detect_seed(rt, fr, self.partial, ws, self.seed, self.status),
                ops.refine_com_iterative(rt, fr, self.partial, B, H, W, self.seed, self.cube, self.fx, self.fy, NUM_REFINE_ITER, self.com,
                                         self.rstatus, name='detect_refine')]
        if do_hand_size:
            out += self.hand_size_stage()
        return out

    def hand_size_stage(self, tol=0.0):
        """Step f alone: the hand's cube from the centre in self.com (status bit DETECT_FOUND must be set for a frame to be measured)."""
        rt, ws = self.rt, self.ws
        if self.K > 1:
            raise ValueError("hand size is measured for one hand per frame: it needs hands=1")
        return [ops.mask_keys(rt, self.frames, self.com, self.cube, ws),
                ops.label_components(rt, ws),
                ops.hand_size(rt, ws, self.com, self.cube, self.fx, self.fy, self.cube_out, self.status, tol=tol)]

    def hand_size(self, tol=0.0):
        """Run step f on the frames and centres the buffers hold: (cubes (B, 3) float32, status (B,)) -- a frame with an empty depth
        range has DETECT_NO_SIZE set and its input cube."""
        host = self.res.get() if self.multi else np.zeros(8 * self.B, np.float32)
        host[6 * self.B:7 * self.B].view(np.int32)[:] = ops.DETECT_FOUND
        self.res.set(host)
        for op in self.hand_size_stage(tol=tol):
            op(self.rt.stream)
        self.rt.synchronize()
        out = self.result(True)
        return out[1], out[4]

    def plan(self, do_hand_size=False):
        key = bool(do_hand_size)
        if key not in self._plans:
            p = ops.Plan('detect')
            if self.sensor is not None and self.cut is None:     # raw -> frames and the partials, then the stage without its range pass
                p.add(ops.frame_ingest(self.rt, self.raw, self.B, self.H, self.W, self.frames, self.partial, median=self.sensor[1],
                                       mirror=self.sensor[2]))
            for op in self.stage(key, with_range=self.sensor is None or self.cut is not None):
                p.add(op)
            self._plans[key] = p
        return self._plans[key]

    def result(self, do_hand_size=False):
        """Download (coms, cubes, found, seeds, status): a frame that was not found has com (0, 0, 0) and its input cube.
        With hands > 1 (or a max_extent) there is a K axis -- coms and seeds (B, K, 3), found and status (B, K), cubes (B, K, 3) (the
        frame's cube in every slot) -- and a sixth entry: report = dict(key, count, xmin, xmax, ymin, ymax, refine_status), (B, K)
        int32 each; an empty slot is all zero with refine_status 1."""
        if self.multi and self._com_in_res:
            return self.parse(self.res.get(), None, None if do_hand_size else self.cube.get())
        return self.parse(self.res.get(), self.com.get(), None if do_hand_size else self.cube.get())

    def parse(self, res, com, cube):
        """result() from downloaded blocks: this detector's 8 * B floats, the centres, the input cubes (None: the measured ones)."""
        if self.multi:
            return self._parse_multi(res, com, cube)
        B = self.B
        status = res[6 * B:7 * B].view(np.int32).copy()
        found = (status & ops.DETECT_FOUND) != 0
        coms = np.asarray(com, np.float32).reshape(B, 3).copy()
        cubes = res[3 * B:6 * B].reshape(B, 3).copy() if cube is None else np.asarray(cube, np.float32).reshape(B, 3).copy()
        return coms, cubes, found, res[:3 * B].reshape(B, 3).copy(), status

    def _parse_multi(self, res, com, cube):
        """parse() of the several-hands block; com None: the centres are the block's own."""
        B, K, N = self.B, self.K, self.N
        res = np.asarray(res, np.float32)
        status = res[6 * N:7 * N].view(np.int32).reshape(B, K).copy()
        found = (status & ops.DETECT_FOUND) != 0
        coms = (res[14 * N:17 * N] if com is None else np.asarray(com, np.float32)).reshape(B, K, 3).copy()
        if cube is None:
            cubes = res[3 * N:6 * N].reshape(B, K, 3).copy()
        else:
            cubes = np.repeat(np.asarray(cube, np.float32).reshape(B, 1, 3), K, axis=1)
        rep = res[8 * N:14 * N].view(np.int32).reshape(B, K, 6)
        report = dict((n, rep[:, :, i].copy()) for i, n in enumerate(ops.DETECT_REPORT))
        report['refine_status'] = res[7 * N:8 * N].view(np.int32).reshape(B, K).copy()
        return coms, cubes, found, res[:3 * N].reshape(B, K, 3).copy(), status, report

    def run(self, frames, cubes, do_hand_size=False):
        """Upload B frames (raw ones of the sensor's dtype, with a sensor) and their cubes, run the plan, download the result (see result())."""
        if self.sensor is None:
            self.frames.set(np.ascontiguousarray(frames, np.float32).reshape(self.B, self.H, self.W))
        else:
            frames = np.asarray(frames)
            if frames.dtype != self.sensor[0]:
                raise ValueError("frame dtype %s, the detector's sensor delivers %s" % (frames.dtype, self.sensor[0]))
            self.raw.set(np.ascontiguousarray(frames).reshape(self.B, self.H, self.W))
        self.cube.set(np.ascontiguousarray(cubes, np.float32).reshape(self.B, 3))
        self.plan(do_hand_size).run(self.rt)
        self.rt.synchronize()
        return self.result(do_hand_size)
