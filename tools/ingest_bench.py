#!/usr/bin/env python3
"""What taking sensor frames on the device costs: 480x640 frames, the 128x128 ResNet (type 1, 14 joints) and ScaleNet at batch one, fp32
(the set-up of tools/track_bench.py).

    python tools/ingest_bench.py [--frames 200] [--reps 5] [--rounds 2] [--parent DIR]

All legs of this tree run in ONE process and ALTERNATE (repetition r of every leg before repetition r + 1 of any), so that drift of
the machine lands on all of them alike; per leg: median and spread (max - min) of the repetitions' per-frame means, after warm-up.
  (a) HandTracker.process, float32 frames prepared by the host              wall ms / frame (one upload, one plan, one download)
  (b) HandTracker(sensor=uint16).process, raw frames, no median             the same, half the upload, frame_ingest for frame_range
  (c) HandTracker(sensor=uint16, median).process                            ... with the 3x3 median in that launch
  (d) acquire() of the three trackers                                       wall ms / frame (the detector plan)
  (e) the launch alone: frame_range against frame_ingest (uint16 / float32, with and without median, mirrored), device ms per
      launch from HIP events around back-to-back launches; and the device time of the three tracking plans measured the same way
  (h) what a host pays without the kernel: scipy.ndimage.median_filter(size=3) of one uint16 frame + astype(float32), ms (if scipy imports)

--parent DIR: a built checkout of the parent commit.  Its HandTracker.process() is measured in child processes of its own that
alternate with this tree's process ((p) below) in the same job: THE baseline for (a)-(c); (a) against (p) shows that sensor=None
costs what it cost.  Every process that opens the GPU runs under a timeout of its own.

The refinement net's last layer is zeroed (track_bench.py: the track stays on its seed, no timing depends on values)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300


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
        out[i] = np.rint(f)                              # whole millimetres: the float32 and the uint16 legs see the same values
        u, v = u + rng.uniform(-3, 3), v + rng.uniform(-3, 3)
    return out, np.float32([W * 0.45, H * 0.5, 600.])


def child(args):
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, 'deep-prior-pp_amd'))
    import numpy as np
    import torch
    from data.importers import NYUImporter
    from hipdp import ops
    from hipdp import runtime as R
    from hipdp.runtime import TorchHipRuntime
    from hipdp.tracker import HandTracker
    from net.resnet import ResNet, ResNetParams
    from net.scalenet import ScaleNet, ScaleNetParams
    rt = TorchHipRuntime()
    R.set_default_runtime(rt)
    di = NYUImporter('../data/NYU/')
    cube = (300., 300., 300.)
    H, W = 480, 640
    pnet = ResNet(np.random.RandomState(23455), cfgParams=ResNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=1, numJoints=14, nDims=3))
    snet = ScaleNet(np.random.RandomState(23455), cfgParams=ScaleNetParams(type=1, nChan=1, wIn=128, hIn=128, batchSize=1, resizeFactor=2,
                                                                         numJoints=1, nDims=3))
    Wl, bl = snet.layers[-1].params
    Wl.set_value(np.zeros_like(Wl.get_value()))
    bl.set_value(np.zeros_like(bl.get_value()))
    pnet.setDeterministic()
    snet.setDeterministic()
    nfr = 16
    frames, com0 = _frames(nfr)
    N, reps = args.frames, args.reps
    out = dict(route=args.route, tree=tree, frames=N, reps=reps)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / N * 1e3

    def device(run):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(torch.cuda.current_stream())
        for _ in range(N):
            run()
        e1.record(torch.cuda.current_stream())
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / N

    if args.route == 'parent':                       # only what the parent commit has: HandTracker.process on float32 frames
        tr = HandTracker(rt, di, pnet, snet, H, W, cube)
        tr.reset(com0)
        seq = [frames[i % nfr] for i in range(N)]
        for i in range(20):
            assert tr.process(frames[i % nfr])['status'] == 0
        out['parent_process_ms'] = [wall(lambda: [tr.process(f) for f in seq]) for _ in range(reps)]
        assert not tr.lost
        print('INGEST_BENCH ' + json.dumps(out))
        return 0

    raw = frames.astype(np.uint16)
    assert np.array_equal(raw.astype(np.float32), frames)
    trackers = dict(a=(HandTracker(rt, di, pnet, snet, H, W, cube), frames),
                    b=(HandTracker(rt, di, pnet, snet, H, W, cube, sensor=dict(dtype='uint16', median=False, mirror=False)), raw),
                    c=(HandTracker(rt, di, pnet, snet, H, W, cube, sensor=dict(dtype='uint16', median=True, mirror=False)), raw))
    legs = {}
    for k, (tr, src) in trackers.items():
        tr.reset(com0)
        seq = [src[i % nfr] for i in range(N)]
        for i in range(20):
            assert tr.process(src[i % nfr])['status'] == 0
        out['acquire_found_' + k] = bool(tr.acquire(src[0])['found'])
        # (order: acquire moves the centre or loses the track, so every process leg starts from the seed again and the plan runs behind it)
        legs['acquire_' + k] = (wall, lambda tr=tr, seq=seq: [tr.acquire(f) for f in seq])
        legs['process_' + k] = (wall, lambda tr=tr, seq=seq: (tr.reset(com0), [tr.process(f) for f in seq]))
        legs['plan_device_' + k] = (device, lambda tr=tr: tr.plan(0).run(rt))
        tr.reset(com0)
    a, b, c = trackers['a'][0], trackers['b'][0], trackers['c'][0]
    assert len(a.plan(0).launches()) == len(b.plan(0).launches()) == len(c.plan(0).launches())
    out['plan_launches'] = len(a.plan(0).launches())
    # (e) the launches alone, on buffers of their own
    fr32, fr16 = rt.upload(frames[:1]), rt.upload(raw[:1])
    dst, part = rt.alloc((1, H, W), np.float32, zero=False), ops.frame_range_workspace(rt, 1)
    alone = dict(frame_range=ops.frame_range(rt, fr32, 1, H, W, part),
                 ingest_u16=ops.frame_ingest(rt, fr16, 1, H, W, dst, part),
                 ingest_u16_median=ops.frame_ingest(rt, fr16, 1, H, W, dst, part, median=True),
                 ingest_u16_median_mirror=ops.frame_ingest(rt, fr16, 1, H, W, dst, part, median=True, mirror=True),
                 ingest_f32=ops.frame_ingest(rt, fr32, 1, H, W, dst, part),
                 ingest_f32_median=ops.frame_ingest(rt, fr32, 1, H, W, dst, part, median=True))
    for k, op in alone.items():
        op(rt.stream)
        legs['launch_' + k] = (device, lambda op=op: op(rt.stream))
    rt.synchronize()
    for k in legs:
        out[k + '_ms'] = []
    for _ in range(reps):                                # the legs alternate
        for k, (how, fn) in legs.items():
            out[k + '_ms'].append(how(fn))
    try:
        from scipy import ndimage
        vals = []
        for i in range(5):
            t0 = time.perf_counter()
            ndimage.median_filter(raw[i], size=3, mode='nearest').astype(np.float32)
            vals.append((time.perf_counter() - t0) * 1e3)
        out['host_median_ms'] = vals
    except ImportError:
        pass
    print('INGEST_BENCH ' + json.dumps(out))
    return 0


def _stat(vals):
    s = sorted(vals)
    n = len(s)
    med = s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])
    return med, s[-1] - s[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=2, help='processes per tree, the trees alternating')
    ap.add_argument('--parent', default=None, help="a built checkout of the parent commit: its process() is the baseline")
    ap.add_argument('--route', choices=['legs', 'parent'], default=None, help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.route:
        return child(args)
    res = {}
    jobs = ([('parent', os.path.abspath(args.parent))] if args.parent else []) + [('legs', ROOT)]
    for r in range(args.rounds):
        for route, tree in jobs:
            cmd = [sys.executable, os.path.abspath(__file__), '--route', route, '--tree', tree, '--frames', str(args.frames), '--reps', str(args.reps)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=CHILD_TIMEOUT, cwd=tree)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith('INGEST_BENCH ')]
            if p.returncode != 0 or not lines:
                sys.stdout.write(p.stdout[-4000:])
                raise SystemExit("%s in %s failed (exit %d)" % (route, tree, p.returncode))      # nothing more is started on the GPU
            d = json.loads(lines[-1][len('INGEST_BENCH '):])
            for k, v in d.items():
                if isinstance(v, list) and k.endswith('_ms'):
                    res.setdefault(k, []).extend(v)
                elif k == 'plan_launches':
                    res[k] = v
    print("sensor frames on the device, 480x640, ResNet type 1 (14 joints) + ScaleNet at batch one, fp32; %d frames x %d repetitions x %d "
          "processes; legs of one process alternate" % (args.frames, args.reps, args.rounds))
    rows = (('parent_process_ms', "(p) the PARENT commit's HandTracker.process, float32 frames, wall ms / frame"),
            ('process_a_ms', '(a) HandTracker.process, float32 frames (sensor=None), wall ms / frame'),
            ('process_b_ms', '(b) sensor uint16, no median: process, wall ms / frame'),
            ('process_c_ms', '(c) sensor uint16, 3x3 median: process, wall ms / frame'),
            ('acquire_a_ms', '(d) acquire, float32 frames, wall ms / frame'),
            ('acquire_b_ms', '    acquire, sensor uint16, no median'),
            ('acquire_c_ms', '    acquire, sensor uint16, 3x3 median'),
            ('launch_frame_range_ms', '(e) frame_range alone, device ms / launch (HIP events, back to back)'),
            ('launch_ingest_u16_ms', '    frame_ingest uint16'),
            ('launch_ingest_u16_median_ms', '    frame_ingest uint16 + median'),
            ('launch_ingest_u16_median_mirror_ms', '    frame_ingest uint16 + median + mirror'),
            ('launch_ingest_f32_ms', '    frame_ingest float32'),
            ('launch_ingest_f32_median_ms', '    frame_ingest float32 + median'),
            ('plan_device_a_ms', '    tracking plan, float32 frames, device ms / plan'),
            ('plan_device_b_ms', '    tracking plan, sensor uint16'),
            ('plan_device_c_ms', '    tracking plan, sensor uint16 + median'),
            ('host_median_ms', '(h) host: scipy median_filter(size=3) of one uint16 frame + astype(float32), ms'))
    st = {}
    for k, label in rows:
        if k not in res:
            continue
        st[k] = _stat(res[k])
        print("%-88s median %.4f  spread %.4f  (min %.4f, max %.4f, n=%d)" % (label, st[k][0], st[k][1], min(res[k]), max(res[k]), len(res[k])))
    base_key = 'parent_process_ms' if 'parent_process_ms' in st else 'process_a_ms'
    base = st[base_key]
    print("baseline: %s" % ("the parent commit's process() from this job" if base_key == 'parent_process_ms' else "(a) of this tree (no --parent)"))
    per_launch = st['plan_device_a_ms'][0] / res['plan_launches']
    print("tracking plan: %d launches, %.4f ms of device time per launch on average" % (res['plan_launches'], per_launch))
    for k, name in (('process_a_ms', '(a)'), ('process_b_ms', '(b)'), ('process_c_ms', '(c)')):
        if k == base_key:
            continue
        gap, noise = base[0] - st[k][0], max(base[1], st[k][1])
        word = 'below' if gap > noise else ('above' if -gap > noise else 'within the spread of')
        print("%s is %+.4f ms against the baseline (larger spread %.4f ms): %s the baseline" % (name, -gap, noise, word))
    extra = st['plan_device_c_ms'][0] - st['plan_device_a_ms'][0]
    print("the median costs %.4f ms of device time per plan over the float32 plan: %s one average plan launch (%.4f ms)"
          % (extra, 'more than' if extra > per_launch else 'no more than', per_launch))
    return 0


if __name__ == '__main__':
    sys.exit(main())
