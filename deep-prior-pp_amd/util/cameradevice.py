"""
Camera devices of the realtime demo (/root/reference/src/util/cameradevice.py): the abstract CameraDevice and FileDevice, which plays
a list of depth files through an importer.  The SDK-backed devices of the reference (CreativeCameraDevice, DepthSenseCameraDevice:
vendor libraries) and saveDepth / saveRGB (scipy.misc image writers) are not built.
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


class FileDevice(CameraDevice):
    """Loads the frames of a list of files through importer.loadDepthMap (cameradevice.py:348-397).  getDepth() returns
    (True, next frame) and raises IndexError past the last file, as the reference's list indexing does.  The reference sleeps 10 ms
    per frame (:394) to pace its GUI; a headless player has nothing to pace, so that sleep is left out."""

    def __init__(self, filenames, importer, mirror=False):
        super(FileDevice, self).__init__(mirror)
        if not isinstance(filenames, list):
            raise ValueError("Files must be list of filenames.")
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
