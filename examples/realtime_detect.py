#!/usr/bin/env python3
"""
examples/test_realtimepipeline.py with the hand FOUND instead of seeded: no annotation starts the track, the hand is detected on the
device by connected components (RealtimeHandposePipeline(seed_detect=True): the nearest 8-connected object of more than 200 px, see
util.handdetector.HandDetector.detectComponents) in the first frame and again after every lost frame.  --calibrate N first measures
the hand over N frames (calibrateHandsize, the headless STATE_INIT) and runs with that cube.  Same data sets, nets and options
otherwise (--sensor-u16 / --median / --mirror of examples/realtime_sensor.py included: raw sensor frames, filtered on the device); prints the time per frame.

    python examples/realtime_detect.py --dataset nyu --data ../data/NYU/ --pose-net ./eval/NYU_network_prior.pkl \\
        --comref-net ./eval/net_NYU_COM_AUGMENT.pkl
"""
import argparse
import importlib.util
import os

_spec = importlib.util.spec_from_file_location('realtime_driver_base', os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                  'test_realtimepipeline.py'))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)                           # sets sys.path; DATASETS, the importers and the net parameter classes
_spec = importlib.util.spec_from_file_location('realtime_sensor_options', os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                     'realtime_sensor.py'))
sensor = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sensor)                         # --sensor-u16 / --median / --mirror and the uint16 file device


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--dataset', choices=sorted(base.DATASETS), default='nyu')
    ap.add_argument('--data', default=None, help='dataset directory (default: ../data/<NAME>/)')
    ap.add_argument('--seq', default=None)
    ap.add_argument('--net', choices=['resnet', 'poseregnet'], default='resnet')
    ap.add_argument('--joints', type=int, default=None, help="the pose net's joints (default: the sequence's)")
    ap.add_argument('--pose-net', default=None, help='checkpoint of the pose net')
    ap.add_argument('--comref-net', default=None, help='checkpoint of the ScaleNet centre refinement')
    ap.add_argument('--calibrate', type=int, default=0, help='measure the hand size over this many frames first')
    ap.add_argument('--max-frames', type=int, default=None)
    ap.add_argument('--cache', default='./cache/')
    sensor.add_sensor_options(ap)
    args = ap.parse_args(argv)
    Importer, seq_name, config = base.DATASETS[args.dataset]
    data = args.data or {'icvl': '../data/ICVL/', 'nyu': '../data/NYU/', 'msra': '../data/MSRA15/'}[args.dataset]
    di = Importer(data, useCache=False, cacheDir=args.cache)
    seq = di.loadSequence(args.seq or seq_name, Nmax=args.max_frames if args.max_frames else float('inf'))
    frames = seq.data
    if not frames:
        raise SystemExit("no frames in %s" % (args.seq or seq_name))
    J = args.joints or int(frames[0].gt3Dorig.shape[0])
    if args.net == 'resnet':
        poseNetParams = base.ResNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=1, numJoints=J, nDims=3)
    else:
        poseNetParams = base.PoseRegNetParams(type=0, nChan=1, wIn=128, hIn=128, batchSize=1, numJoints=J, nDims=3)
    poseNetParams.loadFile = args.pose_net
    comrefNetParams = base.ScaleNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=1, resizeFactor=2, numJoints=1, nDims=3)
    comrefNetParams.loadFile = args.comref_net
    config = dict(config, cube=tuple(seq.config['cube']))
    sensor_desc, Device = sensor.sensor_of(args)
    rtp = base.RealtimeHandposePipeline(poseNetParams, config, di, verbose=False, comrefNet=comrefNetParams, seed_detect=True, sensor=sensor_desc)
    files = [f.fileName for f in frames]
    if args.calibrate:
        print("hand size over {} frames: {}".format(args.calibrate, rtp.calibrateHandsize(Device(files, di), args.calibrate)))
        rtp.lastcom = (0, 0, 0)                          # the run below starts from the first frame again
    poses = rtp.processVideo(Device(files, di), max_frames=args.max_frames)
    t = base.numpy.asarray(rtp.frame_times[1:] or rtp.frame_times)
    print("{} of {} frames with a pose, {:.3f} ms per frame (median)".format(len(poses), len(rtp.frame_times), base.numpy.median(t) * 1000.))
    return poses, rtp.sync['config']['cube']


if __name__ == '__main__':
    main()
