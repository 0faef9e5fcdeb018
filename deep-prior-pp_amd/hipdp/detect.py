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

With sensor=dict(dtype=, median=, mirror=) the frames handed to run() are RAW sensor frames: frame_ingest (csrc/ingest.hip) converts,
mirrors and median-filters them into the float32 frame buffer and writes the depth-range partials, in frame_range's place.
"""
import numpy as np

from . import ops

NUM_REFINE_ITER = 5                 # handdetector.py:610


class FrameDetector(object):
    def __init__(self, rt, H, W, fx, fy, B=1, frames=None, partial=None, com=None, cube=None, res=None, sensor=None, raw=None):
        """
        :param H, W:    frame size
        :param fx, fy:  what the reference hands to HandDetector
        :param B:       frames per run
        :param frames, partial, com, cube: device buffers of an owner whose state the plan works on (HandTracker: its frame buffer,
                        its depth-range partials, its centre -- the plan's final centre lands there -- and its cube); by default own
        :param res:     8 * B float32 of an owner's result block for seed / cube out / status (so that the owner reads ONE block)
        :param sensor:  None, or dict(dtype='uint16' | 'float32', median=bool, mirror=bool): run() takes raw frames of that dtype
        :param raw:     with a sensor: the owner's raw frame buffer (B, H, W) of the sensor's dtype; by default own
        """
        self.rt, self.B, self.H, self.W = rt, int(B), int(H), int(W)
        self.fx, self.fy = abs(float(fx)), abs(float(fy))
        f32 = np.float32
        self.frames = frames if frames is not None else rt.alloc((self.B, self.H, self.W), f32, zero=False)
        self.sensor = None if sensor is None else ops.sensor_spec(sensor)
        self.raw = None
        if self.sensor is not None:
            self.raw = raw if raw is not None else rt.alloc((self.B, self.H, self.W), self.sensor[0], zero=False)
        self.partial = partial if partial is not None else ops.frame_range_workspace(rt, self.B)
        self.com = com if com is not None else rt.alloc((self.B, 3), f32)
        self.cube = cube if cube is not None else rt.alloc((self.B, 3), f32)
        self.ws = ops.ComponentWorkspace(rt, self.B, self.H, self.W)
        # what the host reads per run besides the centre, ONE block: seed, cube out, found / hand-size status, refinement status
        self.res = res if res is not None else rt.alloc(8 * self.B, f32)
        self.seed, self.cube_out = self.res.view(0, (self.B, 3)), self.res.view(3 * self.B, (self.B, 3))
        self.status, self.rstatus = self.res.view(6 * self.B, (self.B,), np.int32), self.res.view(7 * self.B, (self.B,), np.int32)
        self._plans = {}

    def stage(self, do_hand_size=False, with_range=True):
        """The detector's launches in order (steps a-f of the module docstring); with_range=False when the caller's plan has already
        run frame_range (or frame_ingest) on these frames."""
        rt, B, H, W, fr, ws = self.rt, self.B, self.H, self.W, self.frames, self.ws
        out = [ops.frame_range(rt, fr, B, H, W, self.partial)] if with_range else []
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
        return [ops.mask_keys(rt, self.frames, self.com, self.cube, ws),
                ops.label_components(rt, ws),
                ops.hand_size(rt, ws, self.com, self.cube, self.fx, self.fy, self.cube_out, self.status, tol=tol)]

    def hand_size(self, tol=0.0):
        """Run step f on the frames and centres the buffers hold: (cubes (B, 3) float32, status (B,)) -- a frame with an empty depth
        range has DETECT_NO_SIZE set and its input cube."""
        host = np.zeros(8 * self.B, np.float32)
        host[6 * self.B:7 * self.B].view(np.int32)[:] = ops.DETECT_FOUND
        self.res.set(host)
        for op in self.hand_size_stage(tol=tol):
            op(self.rt.stream)
        self.rt.synchronize()
        _, cubes, _, _, status = self.result(True)
        return cubes, status

    def plan(self, do_hand_size=False):
        key = bool(do_hand_size)
        if key not in self._plans:
            p = ops.Plan('detect')
            if self.sensor is not None:             # raw -> frames and the partials, then the stage without its range pass
                p.add(ops.frame_ingest(self.rt, self.raw, self.B, self.H, self.W, self.frames, self.partial, median=self.sensor[1],
                                       mirror=self.sensor[2]))
            for op in self.stage(key, with_range=self.sensor is None):
                p.add(op)
            self._plans[key] = p
        return self._plans[key]

    def result(self, do_hand_size=False):
        """Download (coms, cubes, found, seeds, status): a frame that was not found has com (0, 0, 0) and its input cube."""
        return self.parse(self.res.get(), self.com.get(), None if do_hand_size else self.cube.get())

    def parse(self, res, com, cube):
        """result() from downloaded blocks: this detector's 8 * B floats, the centres, the input cubes (None: the measured ones)."""
        B = self.B
        status = res[6 * B:7 * B].view(np.int32).copy()
        found = (status & ops.DETECT_FOUND) != 0
        coms = np.asarray(com, np.float32).reshape(B, 3).copy()
        cubes = res[3 * B:6 * B].reshape(B, 3).copy() if cube is None else np.asarray(cube, np.float32).reshape(B, 3).copy()
        return coms, cubes, found, res[:3 * B].reshape(B, 3).copy(), status

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
