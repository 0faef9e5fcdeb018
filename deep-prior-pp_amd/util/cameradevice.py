"""
Camera devices of the realtime demo (/root/reference/src/util/cameradevice.py): the abstract CameraDevice and FileDevice, which plays
a list of depth files through an importer.  The SDK-backed devices of the reference (CreativeCameraDevice, DepthSenseCameraDevice:
vendor libraries) and saveDepth / saveRGB (scipy.misc image writers) are not built.

What CreativeCameraDevice.getDepth does to every frame AFTER the SDK has delivered it (:189-200) is built, on the device: the
optional mirror, cv2.medianBlur(depth, 3) on the 16-bit map and the conversion to float32 are one kernel launch (csrc/ingest.hip,
bit for bit cv2's replicated-border median).  filter_depth(frames) is that arithmetic as a function; FilteredDevice(device) applies it
to whatever another CameraDevice delivers -- the place a vendor binding's raw uint16 frames go through.  A realtime user does not
need either: RealtimeHandposePipeline(sensor=...) / HandTracker(sensor=...) take the RAW frames and run the same launch at the head of
the frame's plan (half the upload for uint16, no extra launch).
"""
import numpy


class CameraDevice(object):
    """Abstract class that handles all camera devices (cameradevice.py:43-128)."""

    def __init__(self, mirror=False):
        self.mirror = mirror

    def start(self):
        raise NotImplementedError("!")

    def stop(self):
        raise NotImplementedError("!")

    def getDepth(self):
        """(ok, depth frame in mm as float32)"""
        raise NotImplementedError("!")

    def getRGB(self):
        raise NotImplementedError("!")

    def getGrayScale(self):
        raise NotImplementedError("!")

    def getRGBD(self):
        raise NotImplementedError("!")

    def getLastColorNum(self):
        raise NotImplementedError("!")

    def getLastDepthNum(self):
        raise NotImplementedError("!")

    def getDepthIntrinsics(self):
        raise NotImplementedError("!")

    def getColorIntrinsics(self):
        raise NotImplementedError("!")

    def getExtrinsics(self):
        raise NotImplementedError("!")

    def getTimestamp(self):
        """The time in seconds at which the frame last delivered by getDepth() was taken, on the clock all devices of a rig share, or
        None: the device does not stamp its frames.  (Not in the reference, which has one camera: hipdp/multitrack.py, TIMING.)"""
        return None


class FileDevice(CameraDevice):
    """Loads the frames of a list of files through importer.loadDepthMap (cameradevice.py:348-397).  getDepth() returns
    (True, next frame) and raises IndexError past the last file, as the reference's list indexing does.  The reference sleeps 10 ms
    per frame (:394) to pace its GUI; a headless player has nothing to pace, so that sleep is left out.  stamps: None, or a sequence of
    seconds, one per file -- what a recording's sensor stamped its frames with; getTimestamp() then returns the stamp of the frame last
    delivered."""

    def __init__(self, filenames, importer, mirror=False, stamps=None):
        super(FileDevice, self).__init__(mirror)
        if not isinstance(filenames, list):
            raise ValueError("Files must be list of filenames.")
        if stamps is not None:
            stamps = [float(s) for s in stamps]
            if len(stamps) != len(filenames) or not numpy.isfinite(stamps).all():
                raise ValueError("stamps must be one finite time in seconds per file")
        self.stamps = stamps
        self.filenames = filenames
        self.importer = importer
        if hasattr(importer, 'getCameraIntrinsics'):
            self.depth_intrinsics = importer.getCameraIntrinsics()
        else:
            self.depth_intrinsics = numpy.array([[importer.fx, 0., importer.ux], [0., importer.fy, importer.uy], [0., 0., 1.]], numpy.float32)
        self.color_intrinsics = numpy.zeros((3, 3))
        self.extrinsics = numpy.zeros((3, 4))
        self.last_color_num = 0
        self.last_depth_num = 0

    def start(self):
        pass

    def stop(self):
        pass

    def getDepth(self):
        frame = self.importer.loadDepthMap(self.filenames[self.last_depth_num])
        self.last_depth_num += 1
        return True, frame

    def getTimestamp(self):
        if self.stamps is None or self.last_depth_num == 0:
            return None
        return self.stamps[self.last_depth_num - 1]

    def getLastDepthNum(self):
        return self.last_depth_num

    def getLastColorNum(self):
        return self.last_color_num

    def getDepthIntrinsics(self):
        return self.depth_intrinsics

    def getColorIntrinsics(self):
        return self.color_intrinsics

    def getExtrinsics(self):
        return self.extrinsics


def filter_depth(frames, median=True, mirror=False, runtime=None, return_range=False):
    """What CreativeCameraDevice.getDepth does to a frame (cameradevice.py:189-200) on the device: optional mirror ([:, ::-1]),
    cv2.medianBlur(depth, 3) (replicated border), float32.  frames: (H, W) or (B, H, W), uint16 or float32 (free of NaN) -> float32
    frames of the same shape; with return_range also the per-frame (min, max) of the result, (B, 2) float32 ((2,) for one frame).
    The device buffers are kept per shape and dtype and used again by later calls."""
    from hipdp import ops
    from hipdp.runtime import default_runtime
    from util.handdetector import _cached
    rt = runtime or default_runtime()
    frames = numpy.asarray(frames)
    if frames.dtype.name not in ops.INGEST_TYPES:
        raise ValueError("filter_depth takes uint16 or float32 frames, not %s" % frames.dtype)
    if frames.ndim not in (2, 3):
        raise ValueError("frames must be (H, W) or (B, H, W)")
    single = frames.ndim == 2
    B, H, W = (1,) + frames.shape if single else frames.shape
    raw, out, partial = _cached(('filter_depth', rt, B, H, W, frames.dtype.name),
                                lambda: (rt.alloc((B, H, W), frames.dtype, zero=False), rt.alloc((B, H, W), numpy.float32, zero=False),
                                         ops.frame_range_workspace(rt, B)))
    raw.set(numpy.ascontiguousarray(frames).reshape(B, H, W))
    ops.frame_ingest(rt, raw, B, H, W, out, partial, median=median, mirror=mirror)(rt.stream)
    rt.synchronize()
    res = out.get().reshape(frames.shape)
    if not return_range:
        return res
    p = partial.get().reshape(B, -1, 2)                                # frame_range's layout: FR_BANDS (min, max) pairs per frame
    rng = numpy.stack([p[:, :, 0].min(axis=1), p[:, :, 1].max(axis=1)], axis=1)
    return res, (rng[0] if single else rng)


class FilteredDevice(CameraDevice):
    """Any CameraDevice with CreativeCameraDevice.getDepth's frame arithmetic (filter_depth) applied to what it delivers: getDepth()
    returns (count_nonzero != 0, filtered float32 frame), as :199-200 does -- the flag from the filtered frame's depth range, no second
    pass.  The wrapped device must deliver uint16 or float32 frames (anything else is filter_depth's ValueError: no silent
    conversion).  mirror=None takes the wrapped device's `mirror`.  Every other method and attribute is the wrapped device's."""

    def __init__(self, device, median=True, mirror=None, runtime=None):
        super(FilteredDevice, self).__init__(bool(device.mirror) if mirror is None else bool(mirror))
        self.device = device
        self.median = bool(median)
        self.runtime = runtime

    def getDepth(self):
        ret, frame = self.device.getDepth()
        if ret is False:
            return ret, frame
        out, (lo, hi) = filter_depth(frame, median=self.median, mirror=self.mirror, runtime=self.runtime, return_range=True)
        return bool(lo != 0 or hi != 0), out                          # numpy.count_nonzero(depth) != 0

    def start(self):
        return self.device.start()

    def stop(self):
        return self.device.stop()

    def getRGB(self):
        return self.device.getRGB()

    def getGrayScale(self):
        return self.device.getGrayScale()

    def getRGBD(self):
        return self.device.getRGBD()

    def getLastColorNum(self):
        return self.device.getLastColorNum()

    def getLastDepthNum(self):
        return self.device.getLastDepthNum()

    def getDepthIntrinsics(self):
        return self.device.getDepthIntrinsics()

    def getColorIntrinsics(self):
        return self.device.getColorIntrinsics()

    def getExtrinsics(self):
        return self.device.getExtrinsics()

    def getTimestamp(self):
        return self.device.getTimestamp()

    def __getattr__(self, name):                                       # attributes of the wrapped device (filenames, importer, ...)
        if name == 'device':
            raise AttributeError(name)
        return getattr(self.device, name)
