#!/usr/bin/env python3
"""Latency of the frame -> pose routes: 480x640 synthetic depth frames, the 128x128 ResNet (type 1, 14 joints) and ScaleNet at batch
one, fp32.

    python tools/track_bench.py [--frames 200] [--reps 5] [--parent DIR]

Measured, after warm-up, five repetitions each (median and spread = max - min of the repetitions' per-frame means):
  (a) HandTracker.process          wall clock per frame, upload and download included (one upload, one plan, one download)
  (b) HandTracker.process_sequence frames per second (the upload of frame t + 1 under the plan of frame t)
  (c) device time per tracker plan from HIP events around back-to-back plan runs (no transfers), next to the two nets' own
      single-frame forward plans measured the same way: the difference is what the crop / tracking kernels cost
  (d) the per-call route: per frame HandDetector(frame, fx, fy, importer, refineNet).cropArea3D(com=previous centre, size, dsize,
      docom=True), the NumPy normalisation and poseNet.computeOutput -- what a user could do before the tracker existed.

--parent DIR: a checkout of an older tree (with its own built library) whose per-call route (d) is the yardstick.  Every measurement
runs in a child process of its own (one tree per process), the trees alternating, and the verdict line says whether the median of (a)
lies below the median of the parent's (d) by more than the larger of the two spreads.  Without --parent, (d) is measured on this tree.

The refinement net's last layer is zeroed (it answers "no offset"), so the track stays on its seed whatever the random weights of
the nets are; no timing depends on the values.  The per-call route copies the frame (HandDetector zeroes out-of-range depth in place,
and the reference's processVideo hands it frame.copy() as well)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frames(n, H=480, W=640, seed=5):
    import numpy as np
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.float32)
    u, v, d = W * 0.45, H * 0.5, 600.
    for i in range(n):
        f = np.full((H, W), 1400., np.float32) + rng.normal(0, 3., (H, W)).astype(np.float32)
        f[rng.uniform(size=(H, W)) < 0.05] = 0.
        r = 150. * 588.03 / d * 0.7
        blob = (xx - u) ** 2 + (yy - v) ** 2 < r * r
        f[blob] = (d + rng.normal(0, 30., (H, W)))[blob].astype(np.float32)
        f[rng.uniform(size=(H, W)) < 0.01] = 2500.
        out[i] = f
        u, v = u + rng.uniform(-3, 3), v + rng.uniform(-3, 3)
    return out, np.float32([W * 0.45, H * 0.5, 600.])


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
    from util.handdetector import HandDetector
    rt = TorchHipRuntime()
    R.set_default_runtime(rt)
    di = NYUImporter('../data/NYU/')
    cube = (300., 300., 300.)
    pnet = ResNet(np.random.RandomState(23455), cfgParams=ResNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=1, numJoints=14, nDims=3))
    snet = ScaleNet(np.random.RandomState(23455), cfgParams=ScaleNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=1, resizeFactor=2,
                                                                         numJoints=1, nDims=3))
    W, b = snet.layers[-1].params
    W.set_value(np.zeros_like(W.get_value()))
    b.set_value(np.zeros_like(b.get_value()))
    pnet.setDeterministic()
    snet.setDeterministic()
    nfr = 16
    frames, com0 = _frames(nfr)
    N, reps = args.frames, args.reps
    out = dict(route=args.route, tree=tree, frames=N, reps=reps)

    def timed(fn):
        vals = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            vals.append((time.perf_counter() - t0) / N * 1e3)
        return vals

    if args.route == 'percall':
        fx, fy = abs(di.fx), abs(di.fy)
        state = dict(com=com0.copy())

        def one(i):
            hd = HandDetector(frames[i % nfr].copy(), fx, fy, importer=di, refineNet=snet)
            crop, M, com = hd.cropArea3D(com=state['com'], size=cube, dsize=(128, 128), docom=True)
            com3D = di.jointImgTo3D(com)
            sc = cube[2] / 2.
            crop[crop == 0] = com3D[2] + sc
            crop -= com3D[2]
            crop /= sc
            pose = pnet.computeOutput(np.ascontiguousarray(crop[None, None], np.float32))[0].reshape(-1, 3) * cube[2] / 2. + com3D
            state['com'] = np.asarray(com, np.float32)
            return pose
        for i in range(20):
            one(i)
        out['percall_ms'] = timed(lambda: [one(i) for i in range(N)])
    else:
        from hipdp.tracker import HandTracker
        tr = HandTracker(rt, di, pnet, snet, 480, 640, cube)
        tr.reset(com0)
        seq = [frames[i % nfr] for i in range(N)]
        for i in range(20):
            assert tr.process(frames[i % nfr])['status'] == 0
        tr.process_sequence(seq[:20])
        out['process_ms'] = timed(lambda: [tr.process(f) for f in seq])
        out['sequence_ms'] = timed(lambda: tr.process_sequence(seq))

        def device_ms(run):
            vals = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(torch.cuda.current_stream())
                for _ in range(N):
                    run()
                e1.record(torch.cuda.current_stream())
                torch.cuda.synchronize()
                vals.append(e0.elapsed_time(e1) / N)
            return vals
        plan = tr.plan(0)
        out['plan_device_ms'] = device_ms(lambda: plan.run(rt))
        out['posenet_device_ms'] = device_ms(lambda: tr.peng.fwd.run(rt))
        out['comref_device_ms'] = device_ms(lambda: tr.ceng.fwd.run(rt))
        out['plan_launches'] = len(plan.launches())
        out['net_launches'] = [len(tr.peng.fwd.launches()), len(tr.ceng.fwd.launches())]
        assert not tr.lost
    print('TRACK_BENCH ' + json.dumps(out))


def _stat(vals):
    s = sorted(vals)
    n = len(s)
    med = s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])
    return med, s[-1] - s[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--parent', default=None, help='checkout of the tree whose per-call route is the yardstick (built)')
    ap.add_argument('--rounds', type=int, default=2, help='alternations of the two trees')
    ap.add_argument('--route', choices=['fused', 'percall'], default=None, help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.route:
        return child(args)
    ytree = os.path.abspath(args.parent) if args.parent else ROOT
    res = {}
    for r in range(args.rounds):
        for route, tree in (('percall', ytree), ('fused', ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), '--route', route, '--tree', tree, '--frames', str(args.frames), '--reps', str(args.reps)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=420, cwd=tree)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith('TRACK_BENCH ')]
            if p.returncode != 0 or not lines:
                sys.stdout.write(p.stdout[-4000:])
                raise SystemExit("%s route in %s failed (exit %d)" % (route, tree, p.returncode))
            d = json.loads(lines[-1][len('TRACK_BENCH '):])
            for k, v in d.items():
                if isinstance(v, list) and k.endswith('_ms'):
                    res.setdefault(k, []).extend(v)
                else:
                    res[k if k not in ('tree', 'route') else '%s_%s' % (route, k)] = v
    print("frame -> pose latency, 480x640 frames, ResNet type 1 (14 joints) + ScaleNet at batch one, fp32; %d frames x %d repetitions x %d "
          "processes per route" % (args.frames, args.reps, args.rounds))
    print("per-call route measured on: %s" % ('the parent checkout' if args.parent else 'this tree'))
    rows = (('percall_ms', '(d) per-call route (cropArea3D docom + normalise + computeOutput), wall ms / frame'),
            ('process_ms', '(a) HandTracker.process, wall ms / frame'),
            ('sequence_ms', '(b) HandTracker.process_sequence, wall ms / frame'),
            ('plan_device_ms', '(c) tracker plan, device ms / plan (HIP events, back to back)'),
            ('posenet_device_ms', '    pose net forward alone, device ms'),
            ('comref_device_ms', '    refinement net forward alone, device ms'))
    st = {}
    for k, label in rows:
        st[k] = _stat(res[k])
        print("%-86s median %.4f  spread %.4f  (min %.4f, max %.4f, n=%d)" % (label, st[k][0], st[k][1], min(res[k]), max(res[k]), len(res[k])))
    print("(b) as a rate: %.0f frames / s" % (1e3 / st['sequence_ms'][0]))
    print("plan launches: %d (pose net %d, refinement net %d); crop / tracking kernels cost %.4f ms of device time per frame "
          "(plan - the two nets)" % (res['plan_launches'], res['net_launches'][0], res['net_launches'][1],
                                     st['plan_device_ms'][0] - st['posenet_device_ms'][0] - st['comref_device_ms'][0]))
    gap, noise = st['percall_ms'][0] - st['process_ms'][0], max(st['percall_ms'][1], st['process_ms'][1])
    ok = gap > noise
    print("verdict: (a) is %.4f ms below the per-call route; larger spread %.4f ms -> %s" % (gap, noise, 'PASS' if ok else 'FAIL'))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
