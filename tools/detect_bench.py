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
cost of seeding a track.  There is no pass mark."""
import argparse
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
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
