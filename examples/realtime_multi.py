#!/usr/bin/env python3
"""
Several hands and cameras through ONE device plan per tick, headless: two recorded sequences are played through two FileDevices as two
cameras, and three hands are followed at once -- the left- and the right-hand view of the first camera and the left-hand view of the
second (util.realtimehandposepipeline.MultiStreamPipeline on hipdp/multitrack.py).  The nets are built for a batch of three; a tick
costs the launches of ONE single-hand tracker (examples/test_realtimepipeline.py), whatever the number of hands.

Every track is seeded with its sequence's annotated centre of the first frame (both views of the first camera with the same one),
or, with --seed detect, the tracks that are alone on their camera by connected-component detection.  With --seed detect-all no
annotation is used at all: both tracks of the first camera are started by ONE detector plan that returns two hands of a frame
(nearest first; --max-extent MM keeps a wall behind a single hand from being taken for the second -- without a second hand in view
the second track then stays lost).  Prints the time per tick and, where the annotations match the pose net's joints, the mean joint error
of every left-hand track.  Checkpoints are optional: without them the nets have random weights (a dry run of the machinery).

--half-res-second plays the second sequence at half resolution (every second row and column) through an importer whose fx, fy, ux, uy
are halved: the same scene through a different camera, in the same plan as the full-resolution first camera (MultiTracker's
per-source table).  The second camera's 3-D poses must then land near those of the all-full-resolution run, which is made as well;
the mean difference is printed -- a sanity figure, not a bar.  --overlapped runs the ticks through MultiTracker.process_sequence.

--fuse plays the SAME sequence through two cameras and fuses the two tracks of its one hand (hipdp/multitrack.py `groups=`, this
project's own semantics): camera 0 is the recording, camera 1 delivers it at half resolution AND upside down (rotated by 180 degrees
about the optical axis) through the importer that fits -- a known rigid transform of the camera, whose inverse is handed to the tracker
as camera 1's extrinsics (camera 0: the identity), so that both see one world.  Prints the mean spread of the fused joints and the
mean distance of the fused pose from each camera's own -- sanity figures, not bars.  --drop-second A:B covers camera 1 in ticks A ..
B - 1: its frames are all zero and the example marks its track lost (an empty frame moves no centre to depth 0, which is the tracker's
only loss test; the application knows that its camera sees nothing).  In every covered tick the track is handed the centre camera 0
sees, so it is followed again in the first tick in which the frames are back, without a detector plan; the ticks are printed.
--calibrate-extrinsics N withholds camera 1's extrinsics from the tracker: the first N ticks add the hand's joints, as both cameras see
them, to running sums on the device (MultiTracker calibrate=), then a rigid fit on the host gives camera 1 its (R, t) and the run goes on
fusing with it.  Printed per calibrated camera: the joint pairs n, the fit's rms and cond, and how far (degrees, mm) the fit is from the
withheld extrinsics.  The example prints what it gets: with untrained nets the two poses are unrelated and the figures mean nothing.

--smooth RATE MINCUTOFF BETA [--hold N] runs the One-Euro filter over every track's joints (with --fuse: over the fused joints too) as
the plan's last launch (MultiTracker smooth=, this project's own) and prints two sanity figures, not bars: the mean frame-to-frame
displacement of the raw and of the filtered joints, and the mean raw-to-filtered distance -- of the fused pose with --fuse, else of
every track.

--visibility RADIUS MARGIN MIN_SUPPORT [--hidden-weight W] classifies every joint of every track by the frame's depths within RADIUS
pixels of it (MultiTracker visibility=, this project's own: at least MIN_SUPPORT pixels within MARGIN mm of the joint's depth: visible;
else that many nearer ones: occluded; else unsupported; outside the frame: off-frame) and prints the share of joints per class per
track; with --fuse the fusion is weighted by it (a joint that is not visible weighs W, default 0).  With --fuse and --visibility,
--occlude-second X0:Y0:X1:Y1:DEPTH writes a rectangle of DEPTH mm -- something nearer than the hand -- into camera 1's frames (its own
pixel coordinates) and makes two more runs without output, the unoccluded one and the occluded one without --visibility, to print the
mean distance of the fused joints from the unoccluded run's, weighted and unweighted: sanity figures, not bars.

--fuse --stamps RATE [--lag-second N] stamps the frames: camera 0 delivers frame i in tick i with the stamp i / RATE, camera 1 frame
max(i - N, 0) with the stamp (i - N) / RATE -- a camera that runs N frames behind and says so.  The tracker carries the stamps through the
plan (MultiTracker timing=, this project's own): every track is moved to the tick's instant along its own velocity before the two are
fused (max_gap = 4 / RATE, max_lead = (N + 1) / RATE: the example's choice, no default exists).  Two more runs without output, the
synchronous one (N = 0, no timing) and the lagging one without timing, give the mean distance of the fused joints from the synchronous
run's with and without timing: sanity figures, not bars.

--background MARGIN REL [--learn N] [--clutter X0:Y0:X1:Y1:DEPTH] removes a learned per-pixel background from every camera's frames
as the plan's first step (MultiTracker background=, this project's own; the options and the devices of examples/realtime_background.py):
the static rectangle is pasted into every frame of both cameras, the models are learned from the first N ticks (default 5) with the
hand taken out around each sequence's annotated first centre, and with --seed detect / detect-all the detector then starts from the
hand and not from the rectangle.  Prints the share of pixels at which each camera's model knows a background.  Not with --fuse or
--half-res-second.  --clutter ...:DEPTH:START pastes the rectangle only from tick START of the played sequences on (an object put down
after learning), and --adapt PERSIST GUARD [--adapt-every N] keeps the models current while tracking (MultiTracker's adapt=): the
rectangle is absorbed PERSIST adapting ticks later; prints the share of the rectangle each camera's model has taken over at the end.

    python examples/realtime_multi.py --dataset icvl --data ../data/ICVL/ --seqs test_seq_1 test_seq_2
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-prior-pp_amd'))

import numpy  # noqa: E402

from data.importers import DepthImporter, ICVLImporter, MSRA15Importer, NYUImporter  # noqa: E402
from net.poseregnet import PoseRegNetParams  # noqa: E402
from net.resnet import ResNetParams  # noqa: E402
from net.scalenet import ScaleNetParams  # noqa: E402
from util.cameradevice import FileDevice  # noqa: E402
from util.handpose_evaluation import HandposeEvaluation  # noqa: E402
from util.realtimehandposepipeline import MultiStreamPipeline, smoothing_figures  # noqa: E402


def background_example():
    """examples/realtime_background.py as a module: its options' parser and its devices are used here as they are."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('realtime_background_example', os.path.join(ROOT, 'examples', 'realtime_background.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


DATASETS = {'icvl': (ICVLImporter, ('test_seq_1', 'test_seq_2'), {'fx': 241.42, 'fy': 241.42, 'cube': (250, 250, 250)}),
            'nyu': (NYUImporter, ('test_1', 'test_2'), {'fx': 588., 'fy': 587., 'cube': (300, 300, 300)}),
            'msra': (MSRA15Importer, ('P0', 'P1'), {'fx': 241.42, 'fy': 241.42, 'cube': (200, 200, 200)})}


class HalfResFileDevice(FileDevice):
    """A FileDevice that delivers every second row and column of its frames: the camera whose fx, fy, ux, uy are half the recorded one's."""

    def getDepth(self):
        ret, frame = super(HalfResFileDevice, self).getDepth()
        return ret, numpy.ascontiguousarray(frame[::2, ::2])


def half_res_importer(di):
    from hipdp.augmenter import camera_tuple
    half = DepthImporter(di.fx / 2., di.fy / 2., di.ux / 2., di.uy / 2.)
    half.flip_y = camera_tuple(di)[4]
    return half


class UpsideDownHalfResFileDevice(FileDevice):
    """Every second row and column, rotated by 180 degrees: the half-resolution camera mounted upside down."""

    def getDepth(self):
        ret, frame = super(UpsideDownHalfResFileDevice, self).getDepth()
        return ret, numpy.ascontiguousarray(frame[::2, ::2][::-1, ::-1])


def upside_down_half_res_importer(di, H2, W2):
    """The camera of UpsideDownHalfResFileDevice: pixel (u, v) of the half-resolution frame lands at (W2 - 1 - u, H2 - 1 - v), so with the
    principal point mirrored in the same way x and y change sign: its frame is the recorded camera's rotated by diag(-1, -1, 1)."""
    half = half_res_importer(di)
    half.ux, half.uy = (W2 - 1) - half.ux, (H2 - 1) - half.uy
    return half


def smooth_arg(args):
    """{} without --smooth, else the smooth= keyword of the pipeline."""
    if args.smooth is None:
        return {}
    return dict(smooth=dict(rate=args.smooth[0], mincutoff=args.smooth[1], beta=args.smooth[2], max_hold=args.hold))


def print_smoothing(what, fig):
    print("{}, smoothing (sanity figures): mean frame-to-frame displacement {raw_step:.3f} mm raw, {filtered_step:.3f} mm filtered; "
          "mean raw-to-filtered distance {distance:.3f} mm".format(what, **fig))


CLASSES = (('visible', 1), ('occluded', 2), ('unsupported', 4), ('off-frame', 8))          # ops.VIS_*


def visibility_arg(args):
    """{} without --visibility, else the visibility= keyword of the pipeline."""
    if args.visibility is None:
        return {}
    r, margin, support = args.visibility
    return dict(visibility=dict(radius=int(r), margin=margin, min_support=int(support), hidden_weight=args.hidden_weight))


def class_shares(classes):
    """{class name: share} of the joints of one track over its followed ticks: classes is (ticks, J) of ops.VIS_* words."""
    c = numpy.asarray(classes, numpy.int32).reshape(-1)
    return dict((name, float((c == v).mean()) if c.size else float('nan')) for name, v in CLASSES)


def print_visibility(t, shares):
    print("track {}, visibility: ".format(t) + ', '.join("{} {:.3f}".format(name, shares[name]) for name, _ in CLASSES))


def fuse_demo(args, di, seqs, config, poseNetParams, comrefNetParams, hands, occlude=None, visibility=True, lag=0, timing=False):
    """--fuse: one sequence through two cameras, the two tracks of its hand fused; returns a dict of what is printed.  occlude: None or
    (x0, y0, x1, y1, depth), the rectangle written into camera 1's frames; visibility False: without --visibility whatever args say.
    lag: camera 1 delivers frame max(i - lag, 0) in tick i; timing: the frames are stamped (--stamps) and the tracker reads the stamps."""
    files = [f.fileName for f in seqs[0].data]
    files1, stamped, time_kw = [files[max(i - lag, 0)] for i in range(len(files))], [{}, {}], {}
    if timing:
        rate = float(args.stamps)
        stamped = [dict(stamps=[i / rate for i in range(len(files))]), dict(stamps=[(i - lag) / rate for i in range(len(files))])]
        time_kw = dict(timing=dict(max_gap=4. / rate, max_lead=(lag + 1.) / rate))
    H, W = numpy.asarray(di.loadDepthMap(files[0])).shape
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    di2 = upside_down_half_res_importer(di, H2, W2)
    Rz = numpy.diag([-1., -1., 1.])                                    # camera 1's frame -> world (= camera 0's frame): its own inverse
    true_ext = [(numpy.eye(3), numpy.zeros(3)), (Rz, numpy.zeros(3))]
    n_cal = args.calibrate_extrinsics or 0
    vis_kw = visibility_arg(args) if visibility else {}
    cfg = dict(config, fx=[config['fx'], config['fx'] / 2.], fy=[config['fy'], config['fy'] / 2.],
               extrinsics=[true_ext[0], None] if n_cal else true_ext)        # calibrating: camera 1's pose is withheld from the tracker
    c0 = numpy.asarray(seqs[0].data[0].gtorig[di.crop_joint_idx], numpy.float32)
    seeds = [c0, numpy.float32([(W2 - 1) - c0[0] / 2., (H2 - 1) - c0[1] / 2., c0[2]])]
    devices = [FileDevice(files, di, **stamped[0]), UpsideDownHalfResFileDevice(files1, di, **stamped[1])]
    msp = MultiStreamPipeline(poseNetParams, cfg, [di, di2], devices, hands, comrefNetParams, init_com=seeds, groups=[[0, 1]],
                              max_dev=args.max_dev, calibrate=dict(anchor=0) if n_cal else None,
                              **dict(smooth_arg(args), **dict(vis_kw, **time_kw)))
    drop = range(0)
    if args.drop_second:
        a, b = (int(v) for v in args.drop_second.split(':'))
        drop = range(a, b)
    msp.initNets()
    for dev in devices:
        dev.start()
    status, spread, dist, fused, calibration, fused_f = [], [], [[], []], [], [], []
    classes, fused_at = [[], []], []
    tick = 0
    while args.max_frames is None or tick < args.max_frames:
        frames = msp._read()
        if frames is None:
            break
        if tick in drop:                                               # camera 1 is covered: no depth at all, so no hand
            frames[1] = numpy.zeros_like(frames[1])
            if msp._tracker is not None:
                msp._tracker.drop(1)
        if occlude is not None:                                        # something nearer than the hand in front of camera 1
            x0, y0, x1, y1, depth = occlude
            frames[1] = numpy.array(frames[1])
            frames[1][int(y0):int(y1), int(x0):int(x1)] = depth
        res = msp.processFrames(frames)
        status.append([r['status'] for r in res])
        if vis_kw:
            for t, r in enumerate(res):
                if r['status'] == 0:
                    classes[t].append(r['vis_class'].copy())
        tick += 1
        mt = msp._tracker
        if mt.calibrating:                                             # the tick added its joint pairs to the sums; nothing is fused yet
            if tick >= n_cal:
                for c, r in sorted(mt.finish_calibration().items()):
                    Rt, tt = true_ext[c]
                    cosa = (numpy.trace(r['R'].T.dot(Rt)) - 1.) / 2.
                    r = dict(r, source=c, angle=float(numpy.degrees(numpy.arccos(numpy.clip(cosa, -1., 1.)))),
                             shift=float(numpy.linalg.norm(r['t'] - tt)))
                    calibration.append(r)
                    print("camera {} after {} ticks: n {} joint pairs, rms {:.3f} mm, cond {:.4f}, ok {}; {:.3f} degrees and {:.3f} mm from "
                          "the extrinsics it was given up with".format(c, tick, r['n'], r['rms'], r['cond'], r['ok'], r['angle'], r['shift']))
            continue
        f = msp.fused[0]
        if f['n'] == 2:
            spread.append(float(f['spread'].mean()))
            ext = mt.rig.extr_host
            for t in range(2):
                Rm, tv = ext[t, :9].reshape(3, 3), ext[t, 9:]
                world = res[t]['pose'].astype(numpy.float64).dot(Rm.T) + tv
                dist[t].append(float(numpy.sqrt(((world - f['pose']) ** 2).sum(1)).mean()))
        if f['n'] > 0:
            fused.append(f['pose'].copy())
            fused_at.append(tick - 1)
            if args.smooth is not None:
                fused_f.append(f['pose_f'].copy())
    for dev in devices:
        dev.stop()
    out = dict(status=status, spread=float(numpy.mean(spread)) if spread else float('nan'),
               dist=[float(numpy.mean(d)) if d else float('nan') for d in dist], fused=numpy.asarray(fused, numpy.float32), dropped=list(drop),
               back=None, calibration=calibration, fused_at=fused_at)
    print("{} ticks, both cameras followed in {}: mean spread {:.3f} mm, fused pose {:.3f} mm from camera 0's, {:.3f} mm from camera 1's"
          .format(tick, len(spread), out['spread'], out['dist'][0], out['dist'][1]))
    if len(drop):
        after = [i for i in range(drop[-1] + 1, tick) if status[i][1] == 0]
        out['back'] = after[0] if after else None
        print("camera 1 covered in ticks {} .. {}; its track is followed again in tick {} (expected: {}, the tick after the last covered one)"
              .format(drop[0], drop[-1], out['back'], drop[-1] + 1))
    if args.smooth is not None:
        out['smooth'] = smoothing_figures(fused, fused_f)
        print_smoothing("fused pose", out['smooth'])
    if vis_kw:
        out['visibility'] = [class_shares(c) for c in classes]
        for t, shares in enumerate(out['visibility']):
            print_visibility(t, shares)
    return out


def fused_distance(a, b):
    """Mean distance (mm) of the fused joints of run a from those of run b over the ticks in which both have a fused pose."""
    ia, ib = dict(zip(a['fused_at'], a['fused'])), dict(zip(b['fused_at'], b['fused']))
    both = sorted(set(ia) & set(ib))
    if not both:
        return float('nan')
    return float(numpy.mean([numpy.sqrt(((ia[i].astype(numpy.float64) - ib[i]) ** 2).sum(1)).mean() for i in both]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--dataset', choices=sorted(DATASETS), default='nyu')
    ap.add_argument('--data', default=None, help='dataset directory (default: ../data/<NAME>/)')
    ap.add_argument('--seqs', nargs=2, default=None, help='the two sequences played as camera 0 and camera 1')
    ap.add_argument('--net', choices=['resnet', 'poseregnet'], default='resnet', help='pose net: ResNet type 1 (the reference) or PoseRegNet type 0')
    ap.add_argument('--joints', type=int, default=None, help="the pose net's joints (default: the sequences')")
    ap.add_argument('--pose-net', default=None, help='checkpoint of the pose net')
    ap.add_argument('--comref-net', default=None, help='checkpoint of the ScaleNet centre refinement')
    ap.add_argument('--seed', choices=['gt', 'detect', 'detect-all'], default='gt',
                    help="first centres: the annotations, detection where a camera has one track, or detection for every track")
    ap.add_argument('--max-extent', type=float, default=None, help='with detection: the largest width / height (mm) of a hand candidate')
    ap.add_argument('--max-frames', type=int, default=None)
    ap.add_argument('--half-res-second', action='store_true', help='camera 1 at half resolution through a camera of its own')
    ap.add_argument('--overlapped', action='store_true', help='upload tick n + 1 under the plan of tick n (process_sequence)')
    ap.add_argument('--fuse', action='store_true', help='one sequence through two cameras, the two tracks of its hand fused in the world frame')
    ap.add_argument('--drop-second', default=None, metavar='A:B', help='with --fuse: camera 1 delivers all-zero frames in ticks A .. B - 1')
    ap.add_argument('--max-dev', type=float, default=None, help='with --fuse: MultiTracker max_dev (mm)')
    ap.add_argument('--calibrate-extrinsics', type=int, default=None, metavar='N',
                    help="with --fuse: camera 1's extrinsics are withheld and found again from the tracked hand in the first N ticks")
    ap.add_argument('--smooth', nargs=3, type=float, default=None, metavar=('RATE', 'MINCUTOFF', 'BETA'),
                    help='One-Euro filter over the joints: ticks per second, Hz, Hz per mm/s')
    ap.add_argument('--hold', type=int, default=0, metavar='N', help='with --smooth: ticks a lost track keeps its last filtered pose (max_hold)')
    ap.add_argument('--visibility', nargs=3, type=float, default=None, metavar=('RADIUS', 'MARGIN', 'MIN_SUPPORT'),
                    help="classify every joint by the frame's depths around it: pixels, mm, pixels; with --fuse the fusion is weighted by it")
    ap.add_argument('--hidden-weight', type=float, default=0., metavar='W', help='with --visibility: what a joint that is not visible weighs in the fusion')
    ap.add_argument('--occlude-second', default=None, metavar='X0:Y0:X1:Y1:DEPTH',
                    help="with --fuse --visibility: a rectangle of DEPTH mm written into camera 1's frames")
    ap.add_argument('--stamps', type=float, default=None, metavar='RATE',
                    help='with --fuse: the frames are stamped at RATE per second and the tracker aligns the tracks in time before it fuses them')
    ap.add_argument('--lag-second', type=int, default=0, metavar='N', help='with --fuse --stamps: camera 1 runs N frames behind camera 0')
    ap.add_argument('--background', nargs=2, type=float, default=None, metavar=('MARGIN', 'REL'),
                    help="remove a learned per-pixel background from every camera's frames: mm, and a share of the depth")
    ap.add_argument('--learn', type=int, default=5, metavar='N', help='with --background: the ticks the models are learned from')
    ap.add_argument('--clutter', default=None, metavar='X0:Y0:X1:Y1:DEPTH[:START]',
                    help='with --background: a static rectangle pasted into every frame (from tick START of the sequences on, and not while learning)')
    ap.add_argument('--adapt', nargs=2, type=int, default=None, metavar=('PERSIST', 'GUARD'),
                    help='with --background: keep the models current while tracking: ticks until a depth that stays is background, guard pixels')
    ap.add_argument('--adapt-every', type=int, default=None, metavar='N', help='with --adapt: adapt in every N-th tick')
    ap.add_argument('--cache', default='./cache/')
    args = ap.parse_args(argv)
    Importer, seq_names, config = DATASETS[args.dataset]
    base = args.data or {'icvl': '../data/ICVL/', 'nyu': '../data/NYU/', 'msra': '../data/MSRA15/'}[args.dataset]
    di = Importer(base, useCache=False, cacheDir=args.cache)
    seqs = [di.loadSequence(name, Nmax=args.max_frames if args.max_frames else float('inf')) for name in (args.seqs or seq_names)]
    if not all(s.data for s in seqs):
        raise SystemExit("no frames in one of %s" % (args.seqs or seq_names,))
    L, R = MultiStreamPipeline.HAND_LEFT, MultiStreamPipeline.HAND_RIGHT
    hands = [(0, L), (0, R), (1, L)]                                   # both hands of camera 0, one hand of camera 1
    if args.fuse:
        hands = [(0, L), (1, L)]                                       # ONE hand, seen by both cameras
    T = len(hands)
    J = args.joints or int(seqs[0].data[0].gt3Dorig.shape[0])
    if args.net == 'resnet':
        poseNetParams = ResNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=T, numJoints=J, nDims=3)
    else:
        poseNetParams = PoseRegNetParams(type=0, nChan=1, wIn=128, hIn=128, batchSize=T, numJoints=J, nDims=3)
    poseNetParams.loadFile = args.pose_net
    comrefNetParams = ScaleNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=T, resizeFactor=2, numJoints=1, nDims=3)
    comrefNetParams.loadFile = args.comref_net
    config = dict(config, cube=tuple(seqs[0].config['cube']))
    if args.occlude_second and not (args.fuse and args.visibility is not None):
        raise SystemExit("--occlude-second compares the weighted with the unweighted fusion: it needs --fuse and --visibility")
    if args.stamps is not None and not (args.fuse and numpy.isfinite(args.stamps) and args.stamps > 0. and not args.occlude_second):
        raise SystemExit("--stamps RATE (> 0) stamps the two cameras of --fuse (not together with --occlude-second)")
    if args.lag_second and (args.stamps is None or args.lag_second < 0):
        raise SystemExit("--lag-second N (>= 0) needs --stamps")
    if args.background is not None and (args.fuse or args.half_res_second):
        raise SystemExit("--background is not combined with --fuse or --half-res-second")
    if (args.clutter is not None or args.adapt is not None or args.adapt_every is not None) and args.background is None:
        raise SystemExit("--clutter and --adapt need --background")
    if args.fuse:
        import contextlib
        import io
        demo = (args, di, seqs, config, poseNetParams, comrefNetParams, hands)
        if args.stamps is not None:
            out = fuse_demo(*demo, lag=args.lag_second, timing=True)
            with contextlib.redirect_stdout(io.StringIO()):            # the two runs to compare with: their own output is not repeated
                sync, untimed = fuse_demo(*demo), fuse_demo(*demo, lag=args.lag_second)
            out['lagging'] = dict(timed=fused_distance(out, sync), untimed=fused_distance(untimed, sync))
            print("camera 1 lagging by {} frames (sanity figures): fused joints {timed:.3f} mm from the synchronous run's with timing, "
                  "{untimed:.3f} mm without".format(args.lag_second, **out['lagging']))
            return out
        if not args.occlude_second:
            return fuse_demo(*demo)
        occlude = tuple(float(v) for v in args.occlude_second.split(':'))
        if len(occlude) != 5:
            raise SystemExit("--occlude-second takes X0:Y0:X1:Y1:DEPTH")
        out = fuse_demo(*demo, occlude=occlude)
        with contextlib.redirect_stdout(io.StringIO()):                # the two runs to compare with: their own output is not repeated
            clear, plain = fuse_demo(*demo, visibility=False), fuse_demo(*demo, occlude=occlude, visibility=False)
        out['occluded'] = dict(weighted=fused_distance(out, clear), unweighted=fused_distance(plain, clear))
        print("camera 1 occluded (sanity figures): fused joints {weighted:.3f} mm from the unoccluded run's with the weights, "
              "{unweighted:.3f} mm without".format(**out['occluded']))
        return out
    init = [seqs[d].data[0].gtorig[di.crop_joint_idx] for d, _ in hands]
    if args.seed == 'detect':
        init[2] = None                                                 # alone on its camera: found by the detector
    elif args.seed == 'detect-all':
        init = [None] * T                                              # both hands of camera 0 from one detector plan
    files = [[f.fileName for f in s.data] for s in seqs]

    def run(half):
        if half:
            dis, cfg = [di, half_res_importer(di)], dict(config, fx=[config['fx'], config['fx'] / 2.], fy=[config['fy'], config['fy'] / 2.])
            devices = [FileDevice(files[0], di), HalfResFileDevice(files[1], di)]
            seeds = [c if c is None or d == 0 else numpy.asarray(c, numpy.float32) * numpy.float32([.5, .5, 1.]) for c, (d, _) in zip(init, hands)]
        else:
            dis, cfg, devices, seeds = di, config, [FileDevice(f, di) for f in files], init
        bg_kw = {}
        if args.background is not None:                                # the rooms are not empty: the rectangle in every frame of both cameras
            bg = background_example()
            clutter, start = bg.parse_clutter(args.clutter, with_start=True)
            devices = [bg.ClutterDevice(f, di, clutter, first=start or 0) for f in files]
            bg_kw = dict(background=dict(margin=args.background[0], rel=args.background[1]))
            if bg.parse_adapt(args) is not None:
                bg_kw['background']['adapt'] = bg.parse_adapt(args)
        msp = MultiStreamPipeline(poseNetParams, cfg, dis, devices, hands, comrefNetParams, init_com=seeds, seed_detect=args.seed != 'gt',
                                  max_extent=args.max_extent, **dict(smooth_arg(args), **dict(visibility_arg(args), **bg_kw)))
        if bg_kw:                                                      # learn the rooms without the hand, then play the sequences
            n = min([max(1, args.learn)] + [len(f) for f in files])
            cz = float(config['cube'][2])
            msp.devices = [bg.ClutterDevice(f[:n], di, None if start is not None else clutter,
                                            hand=(float(s.data[0].gtorig[di.crop_joint_idx][2]), cz)) for f, s in zip(files, seqs)]
            models = msp.learnBackground(n)
            msp.devices = devices
            msp.background_known = [float(numpy.isfinite(m['cut']).mean()) for m in models]
            print("background learned from {} ticks: known at {} of the pixels".format(
                n, ', '.join("{:.1%} (camera {})".format(k, c) for c, k in enumerate(msp.background_known))))
        poses = msp.processVideos(max_frames=args.max_frames, overlapped=args.overlapped)
        if bg_kw and clutter is not None and start is not None:        # how much of the late rectangle each camera's model has taken over
            x0, y0, x1, y1, d = clutter
            msp.background_absorbed = [float((numpy.abs(m['near'][y0:y1, x0:x1] - d) < 25.).mean()) for m in msp._tracker.background_model()]
            print("background: the rectangle appeared in tick {}; absorbed at the end: {}".format(
                start, ', '.join("{:.1%} (camera {})".format(k, c) for c, k in enumerate(msp.background_absorbed))))
        return msp, poses
    msp, poses = run(args.half_res_second)
    t = numpy.asarray(msp.frame_times[1:] or msp.frame_times)         # the first tick records the plan
    print("{} ticks, {} tracks, {:.3f} ms per tick (median; {:.3f} ms mean)".format(len(msp.frame_times), T, numpy.median(t) * 1000., t.mean() * 1000.))
    errs = []
    for (d, hand), p in zip(hands, poses):
        err = None
        if hand == L and len(p) and p.shape[1] == seqs[d].data[0].gt3Dorig.shape[0]:
            err = HandposeEvaluation([f.gt3Dorig for f in seqs[d].data[:len(p)]], list(p)).getMeanError()
            print("camera {} left hand, mean error: {}mm".format(d, err))
        errs.append(err)
    if args.half_res_second:                                           # the same scene through the other camera: the poses must be near
        _, full = run(False)
        n = min(len(full[2]), len(poses[2]))
        diff = float(numpy.abs(full[2][:n] - poses[2][:n]).mean()) if n else float('nan')
        print("camera 1 at half resolution against full resolution, mean difference over {} ticks: {:.3f} mm".format(n, diff))
        return poses, errs, diff
    if args.smooth is not None:
        figs = [smoothing_figures(p, pf) for p, pf in zip(poses, msp.poses_f)]
        for t, fig in enumerate(figs):
            print_smoothing("track {}".format(t), fig)
        return poses, errs, figs
    if args.visibility is not None:
        shares = [class_shares(c) for c in msp.vis_classes]
        for t, sh in enumerate(shares):
            print_visibility(t, sh)
        return poses, errs, shares
    return poses, errs


if __name__ == '__main__':
    main()
