#!/usr/bin/env python3
"""
examples/test_realtimepipeline.py fed the way a depth sensor delivers frames: the recorded sequence is handed to the pipeline RAW and
what the reference's CreativeCameraDevice.getDepth does on the host -- mirror, cv2.medianBlur(depth, 3), conversion to float32 -- runs
as the first launch of every frame's device plan (RealtimeHandposePipeline(sensor=...), csrc/ingest.hip).

    --sensor-u16   the recorded frames rounded to uint16 millimetres and fed as such (half the upload); converted on the device
    --median       the 3x3 median filter (cv2's replicated border, bit for bit) on the device
    --mirror       every frame mirrored on the device; the seed annotation is mirrored with it (the error printed is then
                   meaningless: the annotations are those of the recorded frames)

All three default to off, and without them this IS examples/test_realtimepipeline.py: there is no second main here.  The options
are taken off the command line, everything else goes to that example's own main(), which runs with a pipeline class that carries the
sensor description and a device class that delivers uint16 frames.  examples/realtime_detect.py takes the same options from here.

    python examples/realtime_sensor.py --dataset nyu --data ../data/NYU/ --sensor-u16 --median
"""
import argparse
import importlib.util
import os

_spec = importlib.util.spec_from_file_location('realtime_driver_base', os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                  'test_realtimepipeline.py'))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)                           # a private copy of the example: sets sys.path; its names are replaced below
numpy = base.numpy
FileDevice, Pipeline = base.FileDevice, base.RealtimeHandposePipeline


class SensorFileDevice(FileDevice):
    """A FileDevice that delivers its frames as a 16-bit sensor would: rounded to uint16 millimetres."""

    def getDepth(self):
        ret, frame = super(SensorFileDevice, self).getDepth()
        return ret, numpy.clip(numpy.rint(frame), 0, 65535).astype(numpy.uint16)


def add_sensor_options(ap):
    ap.add_argument('--sensor-u16', action='store_true', help='feed raw uint16 frames (the recorded ones, rounded); converted on the device')
    ap.add_argument('--median', action='store_true', help='3x3 median filter of every frame on the device (cv2.medianBlur(depth, 3))')
    ap.add_argument('--mirror', action='store_true', help='mirror every frame on the device')


def sensor_of(args):
    """(the pipeline's sensor description or None, the device class) for the parsed options."""
    if not (args.sensor_u16 or args.median or args.mirror):
        return None, FileDevice
    sensor = dict(dtype='uint16' if args.sensor_u16 else 'float32', median=args.median, mirror=args.mirror)
    return sensor, SensorFileDevice if args.sensor_u16 else FileDevice


def main(argv=None):
    ap = argparse.ArgumentParser(add_help=False)
    add_sensor_options(ap)
    args, rest = ap.parse_known_args(argv)
    sensor, Device = sensor_of(args)
    made = []

    def pipeline(*a, **k):                               # the example's pipeline, with the sensor description
        made.append(Pipeline(*a, sensor=sensor, **k))
        return made[-1]

    def device(filenames, di):                           # the example's device; the seed follows the mirror (it is set before the first frame)
        rtp = made[-1]
        if args.mirror and rtp.init_com is not None:
            rtp.init_com[0] = di.loadDepthMap(filenames[0]).shape[1] - 1 - rtp.init_com[0]
            rtp.lastcom = rtp.init_com.copy()
        return Device(filenames, di)
    base.RealtimeHandposePipeline, base.FileDevice = pipeline, device
    try:
        return base.main(rest)
    finally:
        base.RealtimeHandposePipeline, base.FileDevice = Pipeline, FileDevice


if __name__ == '__main__':
    main()
