#!/usr/bin/env python3
"""Latency of one tick of T tracks over C cameras: 480x640 synthetic depth frames, the 128x128 ResNet (type 1, 14 joints) and ScaleNet,
fp32 -- MultiTracker.process (one plan, nets at batch T) against T sequential HandTracker.process calls (T plans, nets at batch one).

    python tools/multitrack_bench.py [--ticks 300] [--reps 5] [--parent DIR]

Configurations: T = C in {1, 2, 4, 8, 16} (one hand per camera) and T = 2, C = 1 (both hands of one camera).  Measured per
configuration, after warm-up, five repetitions per process (median and spread = max - min of the repetitions' per-tick means):
  multi      MultiTracker.process(frames): wall clock per tick, the C uploads and the one download included
  device     device time of the tick's plan from HIP events around back-to-back plan runs (no transfers)
  yardstick  T HandTrackers (sharing the batch-one nets) called one after the other with their camera's frame: wall clock per tick,
             T uploads, T plans, T downloads

--parent DIR: a checkout of the parent tree (with its own built library) that runs the yardstick.  Every leg runs in a child process
of its own, the legs alternating.  Verdicts: at T = C = 8 the median tick lies below HALF the yardstick's median and the gap exceeds the
larger of the two spreads; at T = C = 1 the tick is not slower than HandTracker.process by more than the larger spread.

As in tools/track_bench.py the refinement net's last layer is zeroed, so every track stays on its seed whatever the random weights
are; no timing depends on the values."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from track_bench import _frames, _stat  # noqa: E402

CONFIGS = [(1, 1), (2, 2), (4, 4), (8, 8), (16, 16), (2, 1)]          # (T, C)


def _key(T, C):
    return 'T%d_C%d' % (T, C)


def child(args):
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, 'deep-prior-pp_amd'))
    import numpy as np
    import torch
    from data.importers import NYUImporter
    from hipdp import runtime as R
    from hipdp.runtime import TorchHipRuntime
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
        W, b = snet.layers[-1].params
        W.set_value(np.zeros_like(W.get_value()))
        b.set_value(np.zeros_like(b.get_value()))
        pnet.setDeterministic()
        snet.setDeterministic()
        return pnet, snet
    nfr = 16
    frames, com0 = _frames(nfr)
    N, reps = args.ticks, args.reps
    out = dict(leg=args.leg, tree=tree, ticks=N, reps=reps)

    def timed(fn):
        vals = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(N):
                fn(i)
            torch.cuda.synchronize()
            vals.append((time.perf_counter() - t0) / N * 1e3)
        return vals

    def tick_frames(i, C):
        return [frames[(i + c) % nfr] for c in range(C)]

    if args.leg == 'yardstick':
        from hipdp.tracker import HandTracker
        pnet, snet = nets(1)
        for T, C in CONFIGS:
            trs = [HandTracker(rt, di, pnet, snet, 480, 640, cube, hand_right=bool(t % 2) and C < T) for t in range(T)]
            for tr in trs:
                tr.reset(com0)

            def tick(i):
                fr = tick_frames(i, C)
                for t, tr in enumerate(trs):
                    assert tr.process(fr[t % C])['status'] == 0
            for i in range(10):
                tick(i)
            out['yardstick_ms_' + _key(T, C)] = timed(tick)
    else:
        from hipdp.multitrack import MultiTracker
        for T, C in CONFIGS:
            pnet, snet = nets(T)
            mt = MultiTracker(rt, di, pnet, snet, 480, 640, cube, [(t % C, bool(t // C)) for t in range(T)])
            for t in range(T):
                mt.reset(t, com0)

            def tick(i):
                assert all(r['status'] == 0 for r in mt.process(tick_frames(i, C)))
            for i in range(10):
                tick(i)
            out['multi_ms_' + _key(T, C)] = timed(tick)
            plan = mt.plan()
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
            out['device_ms_' + _key(T, C)] = vals
            out['launches_' + _key(T, C)] = len(plan.launches())
            assert not mt.lost.any()
    print('MULTITRACK_BENCH ' + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=300)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--parent', default=None, help='checkout of the parent tree (built): it runs the yardstick')
    ap.add_argument('--rounds', type=int, default=2, help='alternations of the two legs')
    ap.add_argument('--leg', choices=['multi', 'yardstick'], default=None, help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return child(args)
    ytree = os.path.abspath(args.parent) if args.parent else ROOT
    res = {}
    for r in range(args.rounds):
        for leg, tree in (('yardstick', ytree), ('multi', ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg, '--tree', tree, '--ticks', str(args.ticks), '--reps', str(args.reps)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=420, cwd=tree)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith('MULTITRACK_BENCH ')]
            if p.returncode != 0 or not lines:
                sys.stdout.write(p.stdout[-4000:])
                raise SystemExit("%s leg in %s failed (exit %d)" % (leg, tree, p.returncode))
            for k, v in json.loads(lines[-1][len('MULTITRACK_BENCH '):]).items():
                if isinstance(v, list):
                    res.setdefault(k, []).extend(v)
                else:
                    res[k] = v
    print("one tick of T tracks over C cameras, 480x640 frames, ResNet type 1 (14 joints) + ScaleNet, fp32; %d ticks x %d repetitions x %d "
          "processes per leg" % (args.ticks, args.reps, args.rounds))
    print("yardstick (T sequential HandTracker.process calls, nets at batch one) measured on: %s" % ('the parent checkout' if args.parent else 'this tree'))
    print("all times in ms per tick: median (spread = max - min over the repetitions)")
    print("%-10s %-22s %-22s %-8s %-22s %s" % ('T, C', 'MultiTracker.process', 'yardstick', 'ratio', 'plan, device time', 'launches'))
    st = {}
    for T, C in CONFIGS:
        k = _key(T, C)
        m, y, d = _stat(res['multi_ms_' + k]), _stat(res['yardstick_ms_' + k]), _stat(res['device_ms_' + k])
        st[k] = (m, y)
        print("%-10s %-22s %-22s %-8s %-22s %d" % ('%d, %d' % (T, C), '%.4f (%.4f)' % m, '%.4f (%.4f)' % y, '%.2fx' % (y[0] / m[0]),
                                                 '%.4f (%.4f)' % d, res['launches_' + k]))
    (m8, y8), (m1, y1) = st[_key(8, 8)], st[_key(1, 1)]
    ok8 = m8[0] < 0.5 * y8[0] and y8[0] - m8[0] > max(m8[1], y8[1])
    print("verdict T = C = 8: tick %.4f ms against %.4f ms for eight calls (half: %.4f); gap %.4f ms, larger spread %.4f ms -> %s"
          % (m8[0], y8[0], 0.5 * y8[0], y8[0] - m8[0], max(m8[1], y8[1]), 'PASS' if ok8 else 'FAIL'))
    ok1 = m1[0] - y1[0] <= max(m1[1], y1[1])
    print("verdict T = C = 1: tick %.4f ms against %.4f ms for HandTracker.process; difference %+.4f ms, larger spread %.4f ms -> %s"
          % (m1[0], y1[0], m1[0] - y1[0], max(m1[1], y1[1]), 'PASS' if ok1 else 'FAIL'))
    return 0 if ok8 and ok1 else 1


if __name__ == '__main__':
    sys.exit(main())
