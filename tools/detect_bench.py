#!/usr/bin/env python3
"""Latency of finding the hand in a whole frame: 480x640 synthetic depth frames, the 128x128 ResNet (type 1, 14 joints) and ScaleNet
at batch one (the tracker the detector plan belongs to), fp32.  Needs the GPU.

    python tools/detect_bench.py [--frames 200] [--reps 5]

Measured in ONE process, after warm-up, the routes alternating repetition by repetition (median and spread = max - min of the
repetitions' per-frame means):
  (a) HandTracker.acquire(frame)                       wall clock per frame: one upload, the detector plan, one download (the tracker's result block)
  (b) HandTracker.acquire(frame, do_hand_size=True)    the same with the hand-size stage
  (c) the detector plan alone                          device time from HIP events around back-to-back plan runs (no transfers),
      without and with the hand-size stage
  (d) seed_com, the only automatic seed there was before: RealtimeHandposePipeline._seed = host calculateCoM of the whole frame
      + refine_com_iterative (upload, two launches, download), wall clock per frame
(d) finds the centre of mass of everything in view and (a) the nearest object: they are not the same answer; what is compared is the
cost of seeding a track.  There is no pass mark.

    python tools/detect_bench.py --hands 1 2 4 [--parent DIR] [--frames 200] [--reps 5] [--rounds 2]

The several-hands leg: frames with four hand-sized objects at different depths, more than a seed window apart.  Per K:
  device     the detector plan of FrameDetector(hands=K) (K = 1: today's plan), device time from HIP events, back to back
  acquire    wall clock of one acquisition: K = 1 HandTracker.acquire(frame); K > 1 MultiTracker.acquire_source(0, frame) with K lost
             tracks on one source -- one upload, one plan, one download, K reset()s
  parent     HandTracker.acquire(frame) and its detector plan on the tree given with --parent (a built checkout of the parent commit;
             without it: this tree), the alternative a user had: one call per hand
Every leg runs in a child process of its own, the legs alternating --rounds times.  Verdicts, both against the parent's numbers of
the same job: K = 1 acquisition within the larger spread of the parent's; one K = 2 acquisition below TWO parent acquisitions by
more than the larger spread."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'deep-prior-pp_amd'))


def _stat(vals):
    s = sorted(vals)
    n = len(s)
    med = s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])
    return med, s[-1] - s[0]


def _hand_frames(n):
    """tools/track_bench.py's frames (a blob at 600 mm before a noisy wall) with three more hand-sized discs at 700, 800 and 900 mm."""
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from track_bench import _frames
    frames, _ = _frames(n)
    yy, xx = np.mgrid[0:480, 0:640]
    rng = np.random.RandomState(9)
    for f in frames:
        for (u, v, d) in ((90., 90., 700.), (540., 100., 800.), (520., 380., 900.)):
            r = 150. * 588.03 / d * 0.7
            disc = (xx - u) ** 2 + (yy - v) ** 2 < r * r
            f[disc] = (d + rng.normal(0, 10., f.shape))[disc].astype(np.float32)
    return frames


def hands_child(args):
    """One leg of the several-hands measurement in this process, on the tree args.tree: prints one DETECT_BENCH json line."""
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, 'deep-prior-pp_amd'))
    import numpy as np
    import torch
    from data.importers import NYUImporter
    from hipdp import runtime as R
    from hipdp.runtime import TorchHipRuntime
    from hipdp.tracker import HandTracker
    from net.resnet import ResNet, ResNetParams
    from net.scalenet import ScaleNet, ScaleNetParams
    rt = TorchHipRuntime()
    R.set_default_runtime(rt)
    di = NYUImporter('../data/NYU/')
    cube = (300., 300., 300.)

    def nets(B):
        pnet = ResNet(np.random.RandomState(23455), cfgParams=ResNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=B, numJoints=14, nDims=3))
        snet = ScaleNet(np.random.RandomState(23455), cfgParams=ScaleNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=B, resizeFactor=2,
                                                                             numJoints=1, nDims=3))
        pnet.setDeterministic()
        snet.setDeterministic()
        return pnet, snet
    nfr = 16
    frames = _hand_frames(nfr)
    N, reps = args.frames, args.reps
    out = dict(leg=args.leg, tree=tree)

    def wall(fn):
        vals = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(N):
                fn(frames[i % nfr])
            torch.cuda.synchronize()
            vals.append((time.perf_counter() - t0) / N * 1e3)
        return vals

    def device(plan):
        vals = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(torch.cuda.current_stream())
            for _ in range(N):
                plan.run(rt)
            e1.record(torch.cuda.current_stream())
            torch.cuda.synchronize()
            vals.append(e0.elapsed_time(e1) / N)
        return vals

    pnet, snet = nets(1)
    tr = HandTracker(rt, di, pnet, snet, 480, 640, cube)
    assert all(tr.acquire(frames[i])['found'] for i in range(nfr))
    if args.leg == 'parent':
        out['parent_acquire_ms'] = wall(lambda f: tr.acquire(f))
        out['parent_device_ms'] = device(tr.detector().plan(False))
    else:
        from hipdp.detect import FrameDetector
        from hipdp.multitrack import MultiTracker
        for K in args.hands:
            det = FrameDetector(rt, 480, 640, di.fx, di.fy, 1, hands=K)
            det.run(frames[:1], [cube])
            out['device_ms_K%d' % K] = device(det.plan(False))
            out['launches_K%d' % K] = sum(op.kernels for op in det.plan(False).launches())
            if K == 1:
                out['acquire_ms_K1'] = wall(lambda f: tr.acquire(f))
                continue
            pk, sk = nets(K)
            mt = MultiTracker(rt, di, pk, sk, 480, 640, cube, [(0, False)] * K)

            def acquire(f):
                mt.lost[:] = True
                return mt.acquire_source(0, f)
            out['found_K%d' % K] = int(sum(a['found'] for a in acquire(frames[0])))
            out['acquire_ms_K%d' % K] = wall(acquire)
    print('DETECT_BENCH ' + json.dumps(out))
    return 0


def hands_main(args):
    ptree = os.path.abspath(args.parent) if args.parent else ROOT
    res = {}
    for _ in range(args.rounds):
        for leg, tree in (('parent', ptree), ('hands', ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg, '--tree', tree, '--frames', str(args.frames), '--reps', str(args.reps),
                   '--hands'] + [str(k) for k in args.hands]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=420, cwd=tree)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith('DETECT_BENCH ')]
            if p.returncode != 0 or not lines:
                sys.stdout.write(p.stdout[-4000:])
                raise SystemExit("%s leg in %s failed (exit %d)" % (leg, tree, p.returncode))
            for k, v in json.loads(lines[-1][len('DETECT_BENCH '):]).items():
                if isinstance(v, list):
                    res.setdefault(k, []).extend(v)
                else:
                    res[k] = v
    print("several hands of one frame, 480x640 frames with four hand-sized objects, fp32; %d frames x %d repetitions x %d processes per leg, "
          "legs alternating" % (args.frames, args.reps, args.rounds))
    print("parent leg (HandTracker.acquire: one hand per call) measured on: %s" % ('the parent checkout' if args.parent else 'this tree'))
    print("all times in ms: median (spread = max - min over the repetitions)")
    pa, pd = _stat(res['parent_acquire_ms']), _stat(res['parent_device_ms'])
    print("%-8s %-26s %-26s %-10s %s" % ('K', 'detector plan, device', 'one acquisition, wall', 'launches', 'hands found'))
    print("%-8s %-26s %-26s %-10s %s" % ('parent', '%.4f (%.4f)' % pd, '%.4f (%.4f)' % pa, '', '1'))
    st = {}
    for K in args.hands:
        d, a = _stat(res['device_ms_K%d' % K]), _stat(res['acquire_ms_K%d' % K])
        st[K] = a
        print("%-8d %-26s %-26s %-10d %s" % (K, '%.4f (%.4f)' % d, '%.4f (%.4f)' % a, res['launches_K%d' % K],
                                             res.get('found_K%d' % K, 1)))
    ok = True
    if 1 in st:
        a = st[1]
        ok1 = abs(a[0] - pa[0]) <= max(a[1], pa[1])
        ok = ok and ok1
        print("verdict K = 1: acquisition %.4f ms against the parent's %.4f ms; difference %+.4f ms, larger spread %.4f ms -> %s"
              % (a[0], pa[0], a[0] - pa[0], max(a[1], pa[1]), 'PASS' if ok1 else 'FAIL'))
    if 2 in st:
        a = st[2]
        ok2 = 2 * pa[0] - a[0] > max(a[1], pa[1])
        ok = ok and ok2
        print("verdict K = 2: one acquisition %.4f ms against two of the parent's, %.4f ms; gap %.4f ms, larger spread %.4f ms -> %s"
              % (a[0], 2 * pa[0], 2 * pa[0] - a[0], max(a[1], pa[1]), 'PASS' if ok2 else 'FAIL'))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--hands', type=int, nargs='+', default=None, help='the several-hands leg: the K to measure, e.g. 1 2 4')
    ap.add_argument('--parent', default=None, help='with --hands: a built checkout of the parent commit, whose acquire is the yardstick')
    ap.add_argument('--rounds', type=int, default=2, help='with --hands: alternations of the two legs')
    ap.add_argument('--leg', choices=['parent', 'hands'], default=None, help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return hands_child(args)
    if args.hands:
        return hands_main(args)
    import numpy as np
    import torch
    from data.importers import NYUImporter
    from hipdp import runtime as R
    from hipdp.runtime import TorchHipRuntime
    from hipdp.tracker import HandTracker
    from net.resnet import ResNet, ResNetParams
    from net.scalenet import ScaleNet, ScaleNetParams
    from tools.track_bench import _frames
    from util.realtimehandposepipeline import RealtimeHandposePipeline
    rt = TorchHipRuntime()
    R.set_default_runtime(rt)
    di = NYUImporter('../data/NYU/')
    cube = (300., 300., 300.)
    pnet = ResNet(np.random.RandomState(23455), cfgParams=ResNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=1, numJoints=14, nDims=3))
    snet = ScaleNet(np.random.RandomState(23455), cfgParams=ScaleNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=1, resizeFactor=2,
                                                                         numJoints=1, nDims=3))
    pnet.setDeterministic()
    snet.setDeterministic()
    nfr = 16
    frames, _ = _frames(nfr)
    N, reps = args.frames, args.reps
    tr = HandTracker(rt, di, pnet, snet, 480, 640, cube)
    rtp = RealtimeHandposePipeline(pnet, {'fx': di.fx, 'fy': di.fy, 'cube': cube}, di, comrefNet=snet, seed_com=True)
    det = tr.detector()
    found = sum(bool(tr.acquire(frames[i])['found']) for i in range(nfr))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(N):
            fn(frames[i % nfr])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / N * 1e3

    def device(plan):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(torch.cuda.current_stream())
        for _ in range(N):
            plan.run(rt)
        e1.record(torch.cuda.current_stream())
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / N

    routes = (('acquire_ms', lambda: wall(lambda f: tr.acquire(f))),
              ('acquire_hs_ms', lambda: wall(lambda f: tr.acquire(f, do_hand_size=True))),
              ('plan_device_ms', lambda: device(det.plan(False))),
              ('plan_hs_device_ms', lambda: device(det.plan(True))),
              ('seed_com_ms', lambda: wall(lambda f: rtp._seed(f))))
    for _, fn in routes:                                   # warm-up: every plan recorded, every shape seen
        fn()
    res = dict((k, []) for k, _ in routes)
    for _ in range(reps):
        for k, fn in routes:
            res[k].append(fn())
    print("hand detection latency, 480x640 frames, fp32; %d frames x %d repetitions per route, one process, routes alternating; "
          "%d of %d distinct frames found" % (N, reps, found, nfr))
    rows = (('acquire_ms', '(a) HandTracker.acquire, wall ms / frame'),
            ('acquire_hs_ms', '(b) HandTracker.acquire(do_hand_size=True), wall ms / frame'),
            ('plan_device_ms', '(c) detector plan, device ms / plan (HIP events, back to back)'),
            ('plan_hs_device_ms', '    with the hand-size stage, device ms / plan'),
            ('seed_com_ms', '(d) seed_com: host calculateCoM + refine_com_iterative, wall ms / frame'))
    for k, label in rows:
        med, spread = _stat(res[k])
        print("%-76s median %.4f  spread %.4f  (min %.4f, max %.4f, n=%d)" % (label, med, spread, min(res[k]), max(res[k]), len(res[k])))
    print("detector plan launches: %d (%d with the hand-size stage)" % (sum(op.kernels for op in det.plan(False).launches()),
                                                                       sum(op.kernels for op in det.plan(True).launches())))
    return 0


if __name__ == '__main__':
    sys.exit(main())
