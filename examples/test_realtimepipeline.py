#!/usr/bin/env python3
"""
The realtime hand-pose pipeline on a recorded sequence, headless -- the Python-3 counterpart of the reference's
/root/reference/src/test_realtimepipeline.py written against the class API of deep-prior-pp_amd/: the frames of a dataset sequence
are played through a FileDevice, the hand is followed from frame to frame (ScaleNet centre refinement) and the pose net regresses the
joints; every frame is ONE device plan (hipdp/tracker.py).  Prints the time per frame and, where the sequence has annotations that
match the pose net's joints, the mean joint error.

The reference finds the hand in the first frame with HandDetector.detect (cv2 contour analysis, not built); here the track is seeded
with the first frame's annotated centre (or --seed com: the frame's own centre of mass, a NON-reference seed).  Its cv2 windows,
keyboard handling and producer / consumer processes are not built either.  Checkpoints are optional: without them the nets have
random weights (a dry run of the machinery).

    python examples/test_realtimepipeline.py --dataset nyu --data ../data/NYU/ --pose-net ./eval/NYU_network_prior.pkl \\
        --comref-net ./eval/net_NYU_COM_AUGMENT.pkl
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-prior-pp_amd'))

import numpy  # noqa: E402

from data.importers import ICVLImporter, MSRA15Importer, NYUImporter  # noqa: E402
from net.poseregnet import PoseRegNetParams  # noqa: E402
from net.resnet import ResNetParams  # noqa: E402
from net.scalenet import ScaleNetParams  # noqa: E402
from util.cameradevice import FileDevice  # noqa: E402
from util.handpose_evaluation import HandposeEvaluation  # noqa: E402
from util.realtimehandposepipeline import RealtimeHandposePipeline  # noqa: E402

# importer, default sequence, the config of the reference's script (test_realtimepipeline.py:70-72)
DATASETS = {'icvl': (ICVLImporter, 'test_seq_1', {'fx': 241.42, 'fy': 241.42, 'cube': (250, 250, 250)}),
            'nyu': (NYUImporter, 'test_1', {'fx': 588., 'fy': 587., 'cube': (300, 300, 300)}),
            'msra': (MSRA15Importer, 'P0', {'fx': 241.42, 'fy': 241.42, 'cube': (200, 200, 200)})}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--dataset', choices=sorted(DATASETS), default='nyu')
    ap.add_argument('--data', default=None, help='dataset directory (default: ../data/<NAME>/)')
    ap.add_argument('--seq', default=None)
    ap.add_argument('--net', choices=['resnet', 'poseregnet'], default='resnet', help='pose net: ResNet type 1 (the reference) or PoseRegNet type 0')
    ap.add_argument('--joints', type=int, default=None, help="the pose net's joints (default: the sequence's)")
    ap.add_argument('--pose-net', default=None, help='checkpoint of the pose net')
    ap.add_argument('--comref-net', default=None, help='checkpoint of the ScaleNet centre refinement')
    ap.add_argument('--seed', choices=['gt', 'com'], default='gt', help="first frame's centre: its annotation, or the frame's centre of mass")
    ap.add_argument('--hand', choices=['left', 'right'], default='left')
    ap.add_argument('--max-frames', type=int, default=None)
    ap.add_argument('--cache', default='./cache/')
    args = ap.parse_args(argv)
    Importer, seq_name, config = DATASETS[args.dataset]
    base = args.data or {'icvl': '../data/ICVL/', 'nyu': '../data/NYU/', 'msra': '../data/MSRA15/'}[args.dataset]
    di = Importer(base, useCache=False, cacheDir=args.cache)
    seq = di.loadSequence(args.seq or seq_name, Nmax=args.max_frames if args.max_frames else float('inf'))
    frames = seq.data
    if not frames:
        raise SystemExit("no frames in %s" % (args.seq or seq_name))
    J = args.joints or int(frames[0].gt3Dorig.shape[0])
    if args.net == 'resnet':
        poseNetParams = ResNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=1, numJoints=J, nDims=3)
    else:
        poseNetParams = PoseRegNetParams(type=0, nChan=1, wIn=128, hIn=128, batchSize=1, numJoints=J, nDims=3)
    poseNetParams.loadFile = args.pose_net
    comrefNetParams = ScaleNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=1, resizeFactor=2, numJoints=1, nDims=3)
    comrefNetParams.loadFile = args.comref_net
    config = dict(config, cube=tuple(seq.config['cube']))
    init = frames[0].gtorig[di.crop_joint_idx] if args.seed == 'gt' else None
    rtp = RealtimeHandposePipeline(poseNetParams, config, di, verbose=False, comrefNet=comrefNetParams, init_com=init, seed_com=args.seed == 'com')
    if args.hand == 'right':
        rtp.processKey(ord('h'))
    dev = FileDevice([f.fileName for f in frames], di)
    poses = rtp.processVideo(dev, max_frames=args.max_frames)
    t = numpy.asarray(rtp.frame_times[1:] or rtp.frame_times)          # the first frame records the plan
    print("{} frames, {:.3f} ms per frame (median; {:.3f} ms mean)".format(len(poses), numpy.median(t) * 1000., t.mean() * 1000.))
    err = None
    if len(poses) and poses.shape[1] == frames[0].gt3Dorig.shape[0]:
        gt3D = [f.gt3Dorig for f in frames[:len(poses)]]
        err = HandposeEvaluation(gt3D, list(poses)).getMeanError()
        print("Mean error: {}mm".format(err))
    return poses, err


if __name__ == '__main__':
    main()
