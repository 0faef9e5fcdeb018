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

Further legs, same protocol (a child process per leg, the legs alternating, 2 processes per leg, median and spread = max - min):
  --homogeneous --parent DIR   MultiTracker.process of this tree against the PARENT's at T = C = 1 and 8: the homogeneous tick must be
                               within the larger of the two spreads (two-sided verdict: which side a miss falls on)
  --mixed                      C sources alternating 480x640 (NYU camera) / 240x320 (the camera of half the intrinsics, every second
                               row and column of the same frames) in ONE plan through the per-source table, against C homogeneous
                               480x640 sources of this tree, at T = C = 8: wall clock per tick and the plans' device time
  --sequence                   MultiTracker.process_sequence (uploads of tick n + 1 under the plan of tick n) against the process()
                               loop of this tree at T = C = 1, 8, 16
  --fuse --parent DIR          the grouped tick (two groups of T / 2 tracks, identity extrinsics, max_dev 50 mm: one more launch,
                               dpp_pose_fuse) at T = C = 8 against this tree's ungrouped tick and against the PARENT's tick.  Claims:
                               the ungrouped tick is within the larger spread of the parent's; the grouped tick exceeds the ungrouped
                               one by no more than the larger spread plus ONE launch's device time (the grouped plan's back-to-back
                               device time over its launch count, from the same run).  And the recovery of a track that lost its hand:
                               wall clock of the two ticks after the frames return by hand-over (tick: gated, restarted from its
                               peers' centre; tick: followed) against the same two ticks through acquire(t, frame) (the detector
                               plan) in the same process: the gap must exceed the larger spread.
  --calibrate --parent DIR     the calibrating tick (calibrate=dict(anchor=0), the extrinsics of the anchor's group withheld: the plan ends in
                               dpp_extrinsics_accumulate in dpp_pose_fuse's place) and the grouped tick after finish_calibration() at T = C =
                               8 in two groups of four, against this tree's ungrouped tick and the PARENT's ungrouped and grouped ticks.
                               Claims: (1) the ungrouped tick and the calibrated grouped tick are each within the larger spread of the
                               parent's same tick; (2) the calibrating plan's device time minus the ungrouped plan's is no more than the
                               grouped plan's minus the ungrouped plan's plus the larger spread: accumulating costs no more than the
                               fusion launch it stands in for.  The wall clock of finish_calibration() is reported without a claim.
  --smooth --parent DIR        the grouped tick with smooth=dict(rate=30, mincutoff=1, beta=0.007, max_hold=2) (one more launch,
                               dpp_pose_smooth, over T + 2 rows) at T = C = 8 in two groups of four, against this tree's grouped tick
                               without `smooth` and the PARENT's grouped tick.  Claims: (1) without `smooth` the tick and the plan's
                               back-to-back device time are each within the larger spread of the parent's; (2) the plan with `smooth`
                               costs at most ONE launch more in device time than the plan without: the bar is the average launch of the
                               smoothing plan (its device time over its launch count, from the same job) plus the larger spread of the
                               two device-time legs.
  --visibility --parent DIR    the grouped tick with visibility=dict(radius=2, margin=40, min_support=6) (one more launch,
                               dpp_joint_visibility, at T x J workgroups behind pose_finish; the fusion launch becomes dpp_pose_fuse_w) at
                               T = C = 8 in two groups of four, against this tree's grouped tick without `visibility` and the PARENT's
                               grouped tick.  Claims, as for --smooth: (1) without `visibility` the tick and the plan's device time are
                               each within the larger spread of the parent's; (2) the plan with `visibility` costs at most ONE average
                               launch of that plan plus the larger spread of the two device-time legs more than the plan without.
  --timing --parent DIR        the grouped tick with timing=dict(max_gap=0.1, max_lead=0.02) (one more launch, dpp_pose_align, at T
                               workgroups behind pose_finish; the fusion launch reads the aligned poses; every tick uploads C + 1 stamps,
                               source c stamped 2 c ms before source 0) at T = C = 8 in two groups of four, against this tree's grouped
                               tick without `timing` and the PARENT's grouped tick.  Claims, as for --smooth: (1) without `timing` the
                               tick and the plan's device time are each within the larger spread of the parent's; (2) the plan with
                               `timing` costs at most ONE average launch of that plan plus the larger spread of the two device-time legs
                               more than the plan without.  No wall-clock claim: the tick gains one small upload and a larger download.
  --background [--parent DIR]  the tick with background=dict(margin=50, rel=0.01) at T = C = 8 (a model that knows a background behind
                               everything at every pixel, loaded through set_background_model: no timing depends on the values).
                               Without a sensor dpp_frame_background stands in dpp_frame_range's place (three frames' worth of bytes
                               for one); with sensor=dict(dtype='uint16', median=True) it follows dpp_frame_ingest (one launch more),
                               measured against the same sensor without `background`.  Claim (two-sided, needs --parent): with
                               background=None the tick and the plan's device time are each within the larger spread of the parent's.
                               The two deltas are reported against the average launch of their plan, without a claim.
  --adapt [--parent DIR]       the tick with background=dict(margin=50, rel=0.01, adapt=dict(persist=5, guard=8, every=1 | 8)) at
                               T = C = 8: dpp_frame_background_adapt in dpp_frame_background's place.  The cut is written in place, so a
                               plan run again on its own frame buffer adapts from nothing (the wall is holes by then).  The adapting tick
                               (take all 1) is therefore timed with a device-to-device copy in front of every run that puts the raw frames
                               of that tick back; so are, for the difference, the same plan with take all 0 and background alone, and the
                               copies alone.  The share of pixels that confirm in such a tick is reported with it.  The back-to-back time
                               with take all 1 is reported as what it is, a lower bound.  Claims (two-sided, on back-to-back runs): with
                               background alone the tick and the plan's device time are each within the larger spread of the parent's
                               (needs --parent); a non-adapting tick's plan (take all 0) within the larger spread of background alone.
                               The cost of an adapting tick is reported, not bounded.
--configs 1x1,8x8 overrides a leg's (T, C) list.

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
    configs = [tuple(int(v) for v in c.split('x')) for c in args.configs.split(',')] if args.configs else CONFIGS

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

    def device_time(plan):
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

    if args.leg in ('mixed', 'sequence'):
        from data.importers import DepthImporter
        from hipdp.multitrack import MultiTracker
        half = DepthImporter(di.fx / 2., di.fy / 2., di.ux / 2., di.uy / 2.)
        half.flip_y = True                                             # the NYU convention, as the full-size camera
        small, com_small = np.ascontiguousarray(frames[:, ::2, ::2]), com0 * np.float32([.5, .5, 1.])
        for T, C in configs:
            pnet, snet = nets(T)
            mixed = args.leg == 'mixed'
            tracks = [(t % C, bool(t // C)) for t in range(T)]
            if mixed:                                                  # even sources 480x640, odd ones 240x320 with their own camera
                mt = MultiTracker(rt, [half if c % 2 else di for c in range(C)], pnet, snet, [240 if c % 2 else 480 for c in range(C)],
                                  [320 if c % 2 else 640 for c in range(C)], cube, tracks)
                assert mt.hetero == (C > 1)
            else:
                mt = MultiTracker(rt, di, pnet, snet, 480, 640, cube, tracks)
            for t, (c, _) in enumerate(tracks):
                mt.reset(t, com_small if mixed and c % 2 else com0)

            def tick_of(i):
                return [(small if mixed and c % 2 else frames)[(i + c) % nfr] for c in range(C)]
            if mixed:
                def run(i0):
                    for i in range(N):
                        assert all(r['status'] == 0 for r in mt.process(tick_of(i0 + i)))
            else:
                def run(i0):
                    res = mt.process_sequence(tick_of(i0 + i) for i in range(N))
                    assert len(res) == N and all(r['status'] == 0 for r in res[-1])
            run(0)
            vals = []
            for r in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(r)
                torch.cuda.synchronize()
                vals.append((time.perf_counter() - t0) / N * 1e3)
            out[args.leg + '_ms_' + _key(T, C)] = vals
            if mixed:
                out['mixed_device_ms_' + _key(T, C)] = device_time(mt.plan())
                out['mixed_launches_' + _key(T, C)] = len(mt.plan().launches())
            assert not mt.lost.any()
    elif args.leg == 'calib':
        from hipdp.multitrack import MultiTracker
        eye = (np.eye(3), np.zeros(3))
        for T, C in configs:
            pnet, snet = nets(T)
            tracks = [(t % C, bool(t // C)) for t in range(T)]
            half = max(1, T // 2)
            groups = [g for g in (list(range(half)), list(range(half, T))) if g]
            # the sources of the anchor's group are withheld; the other group's cannot be found from this anchor and are given
            withheld = sorted(set(tracks[t][0] for t in groups[0]) - {0})
            mt = MultiTracker(rt, di, pnet, snet, 480, 640, cube, tracks, extrinsics=[None if c in withheld else eye for c in range(C)],
                              groups=groups, max_dev=50., calibrate=dict(anchor=0))
            for t in range(T):
                mt.reset(t, com0)

            # every camera plays the SAME frame here: the nets are untrained, and only equal views give pairs that a rigid motion fits
            # (the identity), so that the calibrated tick fuses consistent tracks as the parent's grouped tick does; no time depends on it
            def tick(i):
                assert all(r['status'] == 0 for r in mt.process([frames[i % nfr]] * C))
            for i in range(10):
                tick(i)
            assert mt.calibrating and mt.cal_src == withheld and mt.fused == []
            out['calibrating_ms_' + _key(T, C)] = timed(tick)
            out['calibrating_device_ms_' + _key(T, C)] = device_time(mt.plan())
            out['calibrating_launches_' + _key(T, C)] = len(mt.plan().launches())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            report = mt.finish_calibration()
            torch.cuda.synchronize()
            out['finish_ms_' + _key(T, C)] = [(time.perf_counter() - t0) * 1e3]
            out['finish_pairs_' + _key(T, C)] = int(min(r['pairs'] for r in report.values()))
            assert all(r['ok'] for r in report.values()) and not mt.calibrating, report
            for i in range(10):
                tick(i)
            assert len(mt.fused) == len(groups)
            out['calibrated_ms_' + _key(T, C)] = timed(tick)
            out['calibrated_device_ms_' + _key(T, C)] = device_time(mt.plan())
            out['calibrated_launches_' + _key(T, C)] = len(mt.plan().launches())
    elif args.leg == 'smooth':
        from hipdp import ops
        from hipdp.multitrack import MultiTracker
        eye = (np.eye(3), np.zeros(3))
        for T, C in configs:
            pnet, snet = nets(T)
            tracks = [(t % C, bool(t // C)) for t in range(T)]
            half = max(1, T // 2)
            groups = [g for g in (list(range(half)), list(range(half, T))) if g]
            mt = MultiTracker(rt, di, pnet, snet, 480, 640, cube, tracks, extrinsics=[eye] * C, groups=groups, max_dev=50.,
                              smooth=dict(rate=30., mincutoff=1., beta=0.007, max_hold=2))
            for t in range(T):
                mt.reset(t, com0)

            def tick(i):
                res = mt.process(tick_frames(i, C))
                assert all(r['status'] == 0 and r['smooth'] == ops.SMOOTH_OK for r in res) and all(f['smooth'] == ops.SMOOTH_OK for f in mt.fused)
            mt.process(tick_frames(0, C))                               # the tick that starts every row
            for i in range(10):
                tick(i)
            assert mt.plan().launches()[-1].name == 'pose_smooth'
            out['smooth_ms_' + _key(T, C)] = timed(tick)
            out['smooth_device_ms_' + _key(T, C)] = device_time(mt.plan())
            out['smooth_launches_' + _key(T, C)] = len(mt.plan().launches())
            out['smooth_block_bytes_' + _key(T, C)] = 4 * int(mt.res.size)
    elif args.leg == 'bg':
        from hipdp.multitrack import MultiTracker
        sensor = dict(dtype='uint16', median=True)
        raw = np.rint(frames).astype(np.uint16)
        far = dict(near=np.full((480, 640), 5000., np.float32), seen=np.ones((480, 640), np.int32))      # behind everything: nothing is cut
        for T, C in configs:
            pnet, snet = nets(T)
            tracks = [(t % C, bool(t // C)) for t in range(T)]
            for name, kw, src in (('bg', dict(background=dict(margin=50., rel=0.01)), frames), ('sensor', dict(sensor=sensor), raw),
                                  ('sensor_bg', dict(sensor=sensor, background=dict(margin=50., rel=0.01)), raw)):
                mt = MultiTracker(rt, di, pnet, snet, 480, 640, cube, tracks, **kw)
                if 'background' in kw:
                    for c in range(C):
                        mt.set_background_model(c, far)
                    assert np.isfinite(mt.background_model(0)['cut']).all()
                for t in range(T):
                    mt.reset(t, com0)

                def tick(i):
                    assert all(r['status'] == 0 for r in mt.process([src[(i + c) % nfr] for c in range(C)]))
                for i in range(10):
                    tick(i)
                names = [l.name for l in mt.plan().launches()]
                assert names[:2] == dict(bg=['frame_background', 'crop_prepare_ranged'], sensor=['frame_ingest', 'crop_prepare_ranged'],
                                         sensor_bg=['frame_ingest', 'frame_background'])[name], names[:3]
                out[name + '_ms_' + _key(T, C)] = timed(tick)
                out[name + '_device_ms_' + _key(T, C)] = device_time(mt.plan())
                out[name + '_launches_' + _key(T, C)] = len(names)
                assert not mt.lost.any()
    elif args.leg == 'adapt':
        from hipdp.multitrack import MultiTracker
        far = dict(near=np.full((480, 640), 5000., np.float32), seen=np.ones((480, 640), np.int32))      # behind everything: nothing is cut
        for T, C in configs:
            pnet, snet = nets(T)
            tracks = [(t % C, bool(t // C)) for t in range(T)]
            # the frames of tick i as one device array per i: the raw depths are gone after the in-place cut, so a plan that is run
            # again on its own frame buffer sees the holes the cut left and adapts nothing.  Every timed run is therefore preceded by a
            # device-to-device copy that puts the raw frames of its tick back (in stream order, no host in between).
            keep = [rt.upload(np.stack(tick_frames(i, C))) for i in range(nfr)]

            def fresh_time(mt, copy_only=False):
                """Device time per tick of [restore the raw frames of tick i; run the plan], i going round the nfr ticks; copy_only:
                of the restoring copies alone."""
                plan, vals = mt.plan(), []
                assert mt.frames.size == keep[0].size and mt.sensor is None
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record(torch.cuda.current_stream())
                    for i in range(N):
                        rt.copy(mt.frames, keep[i % nfr])
                        if not copy_only:
                            plan.run(rt)
                    e1.record(torch.cuda.current_stream())
                    torch.cuda.synchronize()
                    vals.append(e0.elapsed_time(e1) / N)
                return vals

            def set_take(mt, v):
                take = np.full(C, v, np.int32)
                mt.adapt.buf(0).set(take)
                mt.adapt.hosts[0] = take

            def share_confirmed(mt):
                """Share of source 0's pixels that one more adapting tick on raw frames confirms (seen goes up)."""
                set_take(mt, 1)
                before = mt.bg.view(mt.bg.seen, 0).get()
                rt.copy(mt.frames, keep[0])
                mt.plan().run(rt)
                rt.synchronize()
                return float((mt.bg.view(mt.bg.seen, 0).get() != before).mean())
            # background alone, by the same method: the reference of the two adapting plans
            mt = MultiTracker(rt, di, pnet, snet, 480, 640, cube, tracks, background=dict(margin=50., rel=0.01))
            for c in range(C):
                mt.set_background_model(c, far)
            for t in range(T):
                mt.reset(t, com0)
            for i in range(10):
                assert all(r['status'] == 0 for r in mt.process(tick_frames(i, C)))
            out['alone_fresh_device_ms_' + _key(T, C)] = fresh_time(mt)
            out['copy_device_ms_' + _key(T, C)] = fresh_time(mt, copy_only=True)
            for name, every in (('adapt1', 1), ('adapt8', 8)):
                mt = MultiTracker(rt, di, pnet, snet, 480, 640, cube, tracks,
                                  background=dict(margin=50., rel=0.01, adapt=dict(persist=5, guard=8, every=every)))
                for c in range(C):
                    mt.set_background_model(c, far)
                for t in range(T):
                    mt.reset(t, com0)

                def tick(i):
                    assert all(r['status'] == 0 for r in mt.process(tick_frames(i, C)))
                for i in range(10 * every):                             # past persist adapting ticks: the scene has replaced the far model
                    tick(i)
                names = [l.name for l in mt.plan().launches()]
                assert names[:2] == ['frame_background_adapt', 'crop_prepare_ranged'], names[:3]
                out[name + '_ms_' + _key(T, C)] = timed(tick)
                out[name + '_launches_' + _key(T, C)] = len(names)
                # the take array as the host leaves it for an adapting (all 1) and for a non-adapting tick (all 0)
                for key, v in (('on', 1), ('off', 0)):
                    set_take(mt, v)
                    # on raw frames: with take 1 the wall confirms in every run, as in a real adapting tick
                    out['%s_%s_fresh_device_ms_%s' % (name, key, _key(T, C))] = fresh_time(mt)
                    # the plan run again on the frame it has already cut (device_time's way): with take 1 a LOWER BOUND of an adapting
                    # tick, the six arrays are read but nothing confirms and `seen` is not stored
                    out['%s_%s_device_ms_%s' % (name, key, _key(T, C))] = device_time(mt.plan())
                out[name + '_confirmed_' + _key(T, C)] = share_confirmed(mt)
                assert out[name + '_confirmed_' + _key(T, C)] > 0.5, "the timed adapting ticks must confirm the scene"
                assert not mt.lost.any()
    elif args.leg == 'timing':
        from hipdp import ops
        from hipdp.multitrack import MultiTracker
        eye = (np.eye(3), np.zeros(3))
        for T, C in configs:
            pnet, snet = nets(T)
            tracks = [(t % C, bool(t // C)) for t in range(T)]
            half = max(1, T // 2)
            groups = [g for g in (list(range(half)), list(range(half, T))) if g]
            mt = MultiTracker(rt, di, pnet, snet, 480, 640, cube, tracks, extrinsics=[eye] * C, groups=groups, max_dev=50.,
                              timing=dict(max_gap=0.1, max_lead=0.02))
            for t in range(T):
                mt.reset(t, com0)
            clock = [0]

            def tick(i):
                clock[0] += 1                                           # the stamps go on over the repetitions: every tick is MOVED
                res = mt.process(tick_frames(i, C), stamps=[clock[0] / 30. - 0.002 * c for c in range(C)])
                assert all(r['status'] == 0 and r['align'] == ops.ALIGN_MOVED for r in res) and all(f['n'] == len(g) for f, g in zip(mt.fused, groups))
            mt.process(tick_frames(0, C), stamps=[-0.002 * c for c in range(C)])    # the tick that starts every row
            for i in range(10):
                tick(i)
            names = [l.name for l in mt.plan().launches()]
            assert names[-2:] == ['pose_align', 'pose_fuse'], names[-3:]
            out['timing_ms_' + _key(T, C)] = timed(tick)
            out['timing_device_ms_' + _key(T, C)] = device_time(mt.plan())
            out['timing_launches_' + _key(T, C)] = len(mt.plan().launches())
            out['timing_block_bytes_' + _key(T, C)] = 4 * int(mt.res.size)
    elif args.leg == 'vis':
        from hipdp import ops
        from hipdp.multitrack import MultiTracker
        eye = (np.eye(3), np.zeros(3))
        for T, C in configs:
            pnet, snet = nets(T)
            tracks = [(t % C, bool(t // C)) for t in range(T)]
            half = max(1, T // 2)
            groups = [g for g in (list(range(half)), list(range(half, T))) if g]
            mt = MultiTracker(rt, di, pnet, snet, 480, 640, cube, tracks, extrinsics=[eye] * C, groups=groups, max_dev=50.,
                              visibility=dict(radius=2, margin=40., min_support=6))
            for t in range(T):
                mt.reset(t, com0)

            def tick(i):
                res = mt.process(tick_frames(i, C))
                assert all(r['status'] == 0 and r['vis_class'].all() for r in res) and all(f['n'] == len(g) for f, g in zip(mt.fused, groups))
            for i in range(10):
                tick(i)
            names = [l.name for l in mt.plan().launches()]
            assert names[-2:] == ['joint_visibility', 'pose_fuse_w'], names[-3:]
            out['vis_ms_' + _key(T, C)] = timed(tick)
            out['vis_device_ms_' + _key(T, C)] = device_time(mt.plan())
            out['vis_launches_' + _key(T, C)] = len(mt.plan().launches())
            out['vis_block_bytes_' + _key(T, C)] = 4 * int(mt.res.size)
            blk = mt.block.split(mt.res.get())
            out['vis_visible_share_' + _key(T, C)] = float((blk['vis_class'] == ops.VIS_VISIBLE).mean())
    elif args.leg in ('fuse', 'fuse_tick'):
        from hipdp.multitrack import MultiTracker
        eye = (np.eye(3), np.zeros(3))
        for T, C in configs:
            pnet, snet = nets(T)
            tracks = [(t % C, bool(t // C)) for t in range(T)]
            half = max(1, T // 2)
            groups = [g for g in (list(range(half)), list(range(half, T))) if g]
            mt = MultiTracker(rt, di, pnet, snet, 480, 640, cube, tracks, extrinsics=[eye] * C, groups=groups, max_dev=50.)
            plain = MultiTracker(rt, di, pnet, snet, 480, 640, cube, tracks)
            for t in range(T):
                mt.reset(t, com0)
                plain.reset(t, com0)

            def tick(i):
                assert all(r['status'] == 0 for r in mt.process(tick_frames(i, C)))
            for i in range(10):
                tick(i)
            assert all(f['n'] == len(g) for f, g in zip(mt.fused, groups)) and len(mt.plan().launches()) == len(plain.plan().launches()) + 1
            out['fuse_ms_' + _key(T, C)] = timed(tick)
            out['fuse_device_ms_' + _key(T, C)] = device_time(mt.plan())
            out['fuse_launches_' + _key(T, C)] = len(mt.plan().launches())
            out['fuse_block_bytes_' + _key(T, C)] = 4 * int(mt.res.size)
            if T < 2 or args.leg == 'fuse_tick':
                continue
            # recovery of track 0: the two ticks after the frames return, by hand-over and through the detector
            n_rec = max(1, N // 10)

            def recover(tr, acquire):
                vals = []
                for _ in range(reps):
                    total = 0.0
                    for i in range(n_rec):
                        fr = tick_frames(i, C)
                        tr.drop(0)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        if acquire:
                            assert tr.acquire(0, fr[0])['found']
                        first = tr.process(fr)
                        second = tr.process(fr)
                        torch.cuda.synchronize()
                        total += time.perf_counter() - t0
                        assert second[0]['status'] == 0 and first[0]['status'] == (0 if acquire else 1)
                    vals.append(total / n_rec * 1e3)
                return vals
            recover(mt, False), recover(plain, True)
            out['recover_handover_ms_' + _key(T, C)] = recover(mt, False)
            out['recover_acquire_ms_' + _key(T, C)] = recover(plain, True)
            assert not mt.lost.any() and not plain.lost.any() and mt._detectors == {}
    elif args.leg == 'yardstick':
        from hipdp.tracker import HandTracker
        pnet, snet = nets(1)
        for T, C in configs:
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
        for T, C in configs:
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
            out['device_ms_' + _key(T, C)] = device_time(plan)
            out['launches_' + _key(T, C)] = len(plan.launches())
            assert not mt.lost.any()
    print('MULTITRACK_BENCH ' + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=300)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--parent', default=None, help='checkout of the parent tree (built): it runs the yardstick')
    ap.add_argument('--rounds', type=int, default=2, help='alternations of the two legs')
    ap.add_argument('--homogeneous', action='store_true', help="this tree's process() against the parent's (needs --parent)")
    ap.add_argument('--mixed', action='store_true', help='sources of unlike sizes and cameras against homogeneous ones')
    ap.add_argument('--sequence', action='store_true', help='process_sequence against the process() loop')
    ap.add_argument('--configs', default=None, help='T x C list of a leg, e.g. 1x1,8x8')
    ap.add_argument('--fuse', action='store_true', help="the grouped tick against this tree's and the parent's ungrouped tick; recovery (needs --parent)")
    ap.add_argument('--calibrate', action='store_true', help="the calibrating and the calibrated tick against this tree's and the parent's ticks (needs --parent)")
    ap.add_argument('--smooth', action='store_true', help="the grouped tick with the One-Euro filter against this tree's and the parent's grouped tick (needs --parent)")
    ap.add_argument('--visibility', action='store_true', help="the grouped tick with joint visibility and the weighted fusion against this tree's and the parent's grouped tick (needs --parent)")
    ap.add_argument('--timing', action='store_true', help="the grouped tick with stamps and the alignment launch against this tree's and the parent's grouped tick (needs --parent)")
    ap.add_argument('--background', action='store_true', help="the tick with a learned background, without and with a sensor, against this tree's and the parent's tick")
    ap.add_argument('--adapt', action='store_true', help="the tick with background adapt= (every 1 and 8; adapting and non-adapting ticks) against the tick with background alone of this tree and of the parent")
    ap.add_argument('--leg', choices=['multi', 'yardstick', 'mixed', 'sequence', 'fuse', 'fuse_tick', 'calib', 'smooth', 'vis', 'timing', 'bg', 'adapt'], default=None, help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return child(args)
    ytree = os.path.abspath(args.parent) if args.parent else ROOT

    def run_legs(legs, configs):
        """legs: (leg, tree, key prefix); every leg a child process of its own, alternating, args.rounds times."""
        res = {}
        for r in range(args.rounds):
            for leg, tree, prefix in legs:
                cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg, '--tree', tree, '--ticks', str(args.ticks), '--reps', str(args.reps)]
                if configs:
                    cmd += ['--configs', configs]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=420, cwd=tree)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith('MULTITRACK_BENCH ')]
                if p.returncode != 0 or not lines:
                    sys.stdout.write(p.stdout[-4000:])
                    raise SystemExit("%s leg in %s failed (exit %d)" % (leg, tree, p.returncode))
                sys.stderr.write("round %d: %s leg in %s done\n" % (r, leg, tree))
                sys.stderr.flush()
                for k, v in json.loads(lines[-1][len('MULTITRACK_BENCH '):]).items():
                    if isinstance(v, list):
                        res.setdefault(prefix + k, []).extend(v)
                    else:
                        res[prefix + k] = v
        return res

    def two_sided(what, a, b, na, nb):
        """`a` against `b` (median, spread): within the larger spread, or which side the miss falls on."""
        d, bar = a[0] - b[0], max(a[1], b[1])
        side = 'within the larger spread' if abs(d) <= bar else ('%s is SLOWER' % na if d > 0 else '%s is FASTER' % na)
        print("verdict %s: %s %.4f ms against %s %.4f ms; difference %+.4f ms, larger spread %.4f ms -> %s" % (what, na, a[0], nb, b[0], d, bar, side))
        return d <= bar

    head = "480x640 frames, ResNet type 1 (14 joints) + ScaleNet, fp32; %d ticks x %d repetitions x %d processes per leg" % (args.ticks, args.reps, args.rounds)
    if args.homogeneous:
        if not args.parent:
            raise SystemExit("--homogeneous compares against --parent DIR")
        cfgs = args.configs or '1x1,8x8'
        res = run_legs([('multi', ytree, 'parent_'), ('multi', ROOT, '')], cfgs)
        print("the homogeneous tick, MultiTracker.process of this tree against the parent checkout's; " + head)
        print("all times in ms per tick: median (spread = max - min over the repetitions)")
        ok = True
        for c in cfgs.split(','):
            T, C = (int(v) for v in c.split('x'))
            k = _key(T, C)
            m, y = _stat(res['multi_ms_' + k]), _stat(res['parent_multi_ms_' + k])
            d, dy = _stat(res['device_ms_' + k]), _stat(res['parent_device_ms_' + k])
            print("T = C = %d: this tree %.4f (%.4f), parent %.4f (%.4f); plan, device time: %.4f (%.4f), parent %.4f (%.4f)" % ((T,) + m + y + d + dy))
            ok = two_sided('T = C = %d' % T, m, y, 'this tree', 'the parent') and ok
        return 0 if ok else 1
    if args.fuse:
        if not args.parent:
            raise SystemExit("--fuse compares against --parent DIR")
        cfgs = args.configs or '8x8'
        res = run_legs([('multi', ytree, 'parent_'), ('multi', ROOT, ''), ('fuse', ROOT, '')], cfgs)
        print("the grouped tick (two groups of T / 2 tracks fused by one more launch) against the ungrouped tick of this tree and of the parent "
              "checkout; " + head)
        print("all times in ms per tick: median (spread = max - min over the repetitions)")
        ok = True
        for c in cfgs.split(','):
            T, C = (int(v) for v in c.split('x'))
            k = _key(T, C)
            f, m, y = _stat(res['fuse_ms_' + k]), _stat(res['multi_ms_' + k]), _stat(res['parent_multi_ms_' + k])
            df, dm, dy = _stat(res['fuse_device_ms_' + k]), _stat(res['device_ms_' + k]), _stat(res['parent_device_ms_' + k])
            nl = res['fuse_launches_' + k]
            per = df[0] / nl
            print("T = C = %d: grouped %.4f (%.4f), ungrouped %.4f (%.4f), parent %.4f (%.4f); plan, device time: grouped %.4f (%.4f), ungrouped "
                  "%.4f (%.4f), parent %.4f (%.4f); launches %d / %d; device time per launch of the grouped plan %.2f us"
                  % ((T,) + f + m + y + df + dm + dy + (nl, res['launches_' + k], per * 1e3)))
            ok = two_sided('T = C = %d, nothing existing got slower' % T, m, y, 'the ungrouped tick', "the parent's tick") and ok
            bar = max(f[1], m[1]) + per
            fits = f[0] - m[0] <= bar
            print("verdict T = C = %d, the grouped tick: %+.4f ms over the ungrouped one; larger spread %.4f ms + one launch %.4f ms = %.4f ms -> %s"
                  % (T, f[0] - m[0], max(f[1], m[1]), per, bar, 'holds' if fits else 'DOES NOT hold'))
            print("  plan device time, grouped - ungrouped: %+.2f us" % ((df[0] - dm[0]) * 1e3))
            ok = fits and ok
            if 'recover_handover_ms_' + k in res:
                h, a = _stat(res['recover_handover_ms_' + k]), _stat(res['recover_acquire_ms_' + k])
                gap = a[0] - h[0]
                wins = gap > max(h[1], a[1])
                print("recovery T = C = %d, the two ticks after the frames return: hand-over %.4f (%.4f), acquire + the same ticks %.4f (%.4f); gap "
                      "%.4f ms, larger spread %.4f ms -> %s" % ((T,) + h + a + (gap, max(h[1], a[1]), 'holds' if wins else 'DOES NOT hold')))
                ok = wins and ok
        return 0 if ok else 1
    if args.smooth:
        if not args.parent:
            raise SystemExit("--smooth compares against --parent DIR")
        cfgs = args.configs or '8x8'
        res = run_legs([('fuse_tick', ytree, 'parent_'), ('fuse_tick', ROOT, ''), ('smooth', ROOT, '')], cfgs)
        print("the grouped tick with smooth= (two groups of T / 2 tracks; one more launch, dpp_pose_smooth, over T + 2 rows) against the grouped "
              "tick without it of this tree and of the parent checkout; " + head)
        print("all times in ms per tick: median (spread = max - min over the repetitions)")
        ok = True
        for c in cfgs.split(','):
            T, C = (int(v) for v in c.split('x'))
            k = _key(T, C)
            s, f, y = _stat(res['smooth_ms_' + k]), _stat(res['fuse_ms_' + k]), _stat(res['parent_fuse_ms_' + k])
            ds, df, dy = _stat(res['smooth_device_ms_' + k]), _stat(res['fuse_device_ms_' + k]), _stat(res['parent_fuse_device_ms_' + k])
            nl = res['smooth_launches_' + k]
            per = ds[0] / nl
            print("T = C = %d, wall clock: with smooth %.4f (%.4f), without %.4f (%.4f), parent %.4f (%.4f)" % ((T,) + s + f + y))
            print("T = C = %d, plan device time: with smooth %.4f (%.4f), without %.4f (%.4f), parent %.4f (%.4f); launches %d / %d / %d; device "
                  "time per launch of the smoothing plan %.2f us" % ((T,) + ds + df + dy + (nl, res['fuse_launches_' + k], res['parent_fuse_launches_' + k], per * 1e3)))
            ok = two_sided('T = C = %d, claim 1, the tick without smooth' % T, f, y, 'this tree', 'the parent') and ok
            ok = two_sided('T = C = %d, claim 1, the plan device time without smooth' % T, df, dy, 'this tree', 'the parent') and ok
            extra, bar = (ds[0] - df[0]) * 1e3, (per + max(ds[1], df[1])) * 1e3
            fits = extra <= bar
            print("verdict T = C = %d, claim 2, plan device time with smooth over the plan without: %+.2f us; one average launch %.2f us + larger "
                  "spread %.2f us = %.2f us -> %s" % (T, extra, per * 1e3, max(ds[1], df[1]) * 1e3, bar, 'holds' if fits else 'DOES NOT hold'))
            if not fits:
                print("  claim 2 is missed by %.2f us" % (extra - bar))
            print("  wall clock with smooth over without: %+.4f ms (no claim: the download grows by %d bytes)" % (s[0] - f[0], res['smooth_block_bytes_' + k] - res['fuse_block_bytes_' + k]))
            ok = fits and ok
        return 0 if ok else 1
    if args.visibility:
        if not args.parent:
            raise SystemExit("--visibility compares against --parent DIR")
        cfgs = args.configs or '8x8'
        res = run_legs([('fuse_tick', ytree, 'parent_'), ('fuse_tick', ROOT, ''), ('vis', ROOT, '')], cfgs)
        print("the grouped tick with visibility= (two groups of T / 2 tracks; one more launch, dpp_joint_visibility, at T x J workgroups behind "
              "pose_finish, and dpp_pose_fuse_w in dpp_pose_fuse's place) against the grouped tick without it of this tree and of the parent "
              "checkout; " + head)
        print("all times in ms per tick: median (spread = max - min over the repetitions)")
        ok = True
        for c in cfgs.split(','):
            T, C = (int(v) for v in c.split('x'))
            k = _key(T, C)
            s, f, y = _stat(res['vis_ms_' + k]), _stat(res['fuse_ms_' + k]), _stat(res['parent_fuse_ms_' + k])
            ds, df, dy = _stat(res['vis_device_ms_' + k]), _stat(res['fuse_device_ms_' + k]), _stat(res['parent_fuse_device_ms_' + k])
            nl = res['vis_launches_' + k]
            per = ds[0] / nl
            print("T = C = %d, wall clock: with visibility %.4f (%.4f), without %.4f (%.4f), parent %.4f (%.4f)" % ((T,) + s + f + y))
            print("T = C = %d, plan device time: with visibility %.4f (%.4f), without %.4f (%.4f), parent %.4f (%.4f); launches %d / %d / %d; "
                  "device time per launch of the visibility plan %.2f us; share of joints VISIBLE in the last tick %.3f"
                  % ((T,) + ds + df + dy + (nl, res['fuse_launches_' + k], res['parent_fuse_launches_' + k], per * 1e3, res['vis_visible_share_' + k])))
            ok = two_sided('T = C = %d, claim 1, the tick without visibility' % T, f, y, 'this tree', 'the parent') and ok
            ok = two_sided('T = C = %d, claim 1, the plan device time without visibility' % T, df, dy, 'this tree', 'the parent') and ok
            extra, bar = (ds[0] - df[0]) * 1e3, (per + max(ds[1], df[1])) * 1e3
            fits = extra <= bar
            print("verdict T = C = %d, claim 2, plan device time with visibility over the plan without: %+.2f us; one average launch %.2f us + "
                  "larger spread %.2f us = %.2f us -> %s" % (T, extra, per * 1e3, max(ds[1], df[1]) * 1e3, bar, 'holds' if fits else 'DOES NOT hold'))
            if not fits:
                print("  claim 2 is missed by %.2f us" % (extra - bar))
            print("  wall clock with visibility over without: %+.4f ms (no claim: the download grows by %d bytes)"
                  % (s[0] - f[0], res['vis_block_bytes_' + k] - res['fuse_block_bytes_' + k]))
            ok = fits and ok
        return 0 if ok else 1
    if args.timing:
        if not args.parent:
            raise SystemExit("--timing compares against --parent DIR")
        cfgs = args.configs or '8x8'
        res = run_legs([('fuse_tick', ytree, 'parent_'), ('fuse_tick', ROOT, ''), ('timing', ROOT, '')], cfgs)
        print("the grouped tick with timing= (two groups of T / 2 tracks; one more launch, dpp_pose_align, at T workgroups behind pose_finish; "
              "the fusion reads the aligned poses; C + 1 stamps uploaded per tick) against the grouped tick without it of this tree and of the "
              "parent checkout; " + head)
        print("all times in ms per tick: median (spread = max - min over the repetitions)")
        ok = True
        for c in cfgs.split(','):
            T, C = (int(v) for v in c.split('x'))
            k = _key(T, C)
            s, f, y = _stat(res['timing_ms_' + k]), _stat(res['fuse_ms_' + k]), _stat(res['parent_fuse_ms_' + k])
            ds, df, dy = _stat(res['timing_device_ms_' + k]), _stat(res['fuse_device_ms_' + k]), _stat(res['parent_fuse_device_ms_' + k])
            nl = res['timing_launches_' + k]
            per = ds[0] / nl
            print("T = C = %d, wall clock: with timing %.4f (%.4f), without %.4f (%.4f), parent %.4f (%.4f)" % ((T,) + s + f + y))
            print("T = C = %d, plan device time: with timing %.4f (%.4f), without %.4f (%.4f), parent %.4f (%.4f); launches %d / %d / %d; device "
                  "time per launch of the timed plan %.2f us" % ((T,) + ds + df + dy + (nl, res['fuse_launches_' + k], res['parent_fuse_launches_' + k], per * 1e3)))
            ok = two_sided('T = C = %d, claim 1, the tick without timing' % T, f, y, 'this tree', 'the parent') and ok
            ok = two_sided('T = C = %d, claim 1, the plan device time without timing' % T, df, dy, 'this tree', 'the parent') and ok
            extra, bar = (ds[0] - df[0]) * 1e3, (per + max(ds[1], df[1])) * 1e3
            fits = extra <= bar
            print("verdict T = C = %d, claim 2, plan device time with timing over the plan without: %+.2f us; one average launch %.2f us + larger "
                  "spread %.2f us = %.2f us -> %s" % (T, extra, per * 1e3, max(ds[1], df[1]) * 1e3, bar, 'holds' if fits else 'DOES NOT hold'))
            if not fits:
                print("  claim 2 is missed by %.2f us" % (extra - bar))
            print("  wall clock with timing over without: %+.4f ms (no claim: one upload of %d bytes more, the download grows by %d bytes)"
                  % (s[0] - f[0], 8 * (C + 1), res['timing_block_bytes_' + k] - res['fuse_block_bytes_' + k]))
            ok = fits and ok
        return 0 if ok else 1
    if args.background:
        cfgs = args.configs or '8x8'
        legs = ([('multi', ytree, 'parent_')] if args.parent else []) + [('multi', ROOT, ''), ('bg', ROOT, '')]
        res = run_legs(legs, cfgs)
        print("the tick with background= (dpp_frame_background in dpp_frame_range's place; with a uint16 sensor and the 3x3 median: behind "
              "dpp_frame_ingest, one launch more) against the tick without it of this tree%s; " % (' and of the parent checkout' if args.parent else '') + head)
        print("all times in ms per tick: median (spread = max - min over the repetitions)")
        ok = True
        for c in cfgs.split(','):
            T, C = (int(v) for v in c.split('x'))
            k = _key(T, C)
            m, dm = _stat(res['multi_ms_' + k]), _stat(res['device_ms_' + k])
            b, db = _stat(res['bg_ms_' + k]), _stat(res['bg_device_ms_' + k])
            s_, ds = _stat(res['sensor_ms_' + k]), _stat(res['sensor_device_ms_' + k])
            sb, dsb = _stat(res['sensor_bg_ms_' + k]), _stat(res['sensor_bg_device_ms_' + k])
            print("T = C = %d, wall clock: background=None %.4f (%.4f), with background %.4f (%.4f); sensor %.4f (%.4f), sensor with background "
                  "%.4f (%.4f)" % ((T,) + m + b + s_ + sb))
            print("T = C = %d, plan device time: background=None %.4f (%.4f), with background %.4f (%.4f); sensor %.4f (%.4f), sensor with "
                  "background %.4f (%.4f); launches %d / %d / %d / %d" % ((T,) + dm + db + ds + dsb + (
                      res['launches_' + k], res['bg_launches_' + k], res['sensor_launches_' + k], res['sensor_bg_launches_' + k])))
            if args.parent:
                y, dy = _stat(res['parent_multi_ms_' + k]), _stat(res['parent_device_ms_' + k])
                print("T = C = %d, the parent's tick %.4f (%.4f), its plan's device time %.4f (%.4f)" % ((T,) + y + dy))
                ok = two_sided('T = C = %d, the tick with background=None' % T, m, y, 'this tree', 'the parent') and ok
                ok = two_sided('T = C = %d, the plan device time with background=None' % T, dm, dy, 'this tree', 'the parent') and ok
            per, per_s = db[0] / res['bg_launches_' + k] * 1e3, dsb[0] / res['sensor_bg_launches_' + k] * 1e3
            mb = 4. * C * 480 * 640 / 1e6
            print("  without a sensor, frame_background for frame_range (%.1f MB moved for %.1f MB): plan device time %+.2f us (spreads %.2f / %.2f "
                  "us); the plan's average launch is %.2f us; wall clock %+.4f ms" % (3 * mb, mb, (db[0] - dm[0]) * 1e3, db[1] * 1e3, dm[1] * 1e3,
                                                                                     per, b[0] - m[0]))
            print("  with the sensor, one launch more: plan device time %+.2f us (spreads %.2f / %.2f us); the plan's average launch is %.2f us; "
                  "wall clock %+.4f ms" % ((dsb[0] - ds[0]) * 1e3, dsb[1] * 1e3, ds[1] * 1e3, per_s, sb[0] - s_[0]))
        return 0 if ok else 1
    if args.adapt:
        cfgs = args.configs or '8x8'
        res = run_legs(([('bg', ytree, 'parent_')] if args.parent else []) + [('bg', ROOT, ''), ('adapt', ROOT, '')], cfgs)
        print("the tick with background=dict(..., adapt=) (dpp_frame_background_adapt in dpp_frame_background's place, the launch count unchanged) "
              "against the tick with background alone of this tree%s; " % (' and of the parent checkout' if args.parent else '') + head)
        print("all times in ms per tick: median (spread = max - min over the repetitions)")
        ok = True
        for c in cfgs.split(','):
            T, C = (int(v) for v in c.split('x'))
            k = _key(T, C)
            b, db = _stat(res['bg_ms_' + k]), _stat(res['bg_device_ms_' + k])
            a1, a8 = _stat(res['adapt1_ms_' + k]), _stat(res['adapt8_ms_' + k])
            rp1, rp8, off8 = (_stat(res[n + '_device_ms_' + k]) for n in ('adapt1_on', 'adapt8_on', 'adapt8_off'))
            al, cp = _stat(res['alone_fresh_device_ms_' + k]), _stat(res['copy_device_ms_' + k])
            on1, of1, on8, of8 = (_stat(res[n + '_fresh_device_ms_' + k]) for n in ('adapt1_on', 'adapt1_off', 'adapt8_on', 'adapt8_off'))
            print("T = C = %d, wall clock: background alone %.4f (%.4f); adapt every=1 %.4f (%.4f); adapt every=8 %.4f (%.4f)" % ((T,) + b + a1 + a8))
            print("T = C = %d, plan device time, the plan run again on the frames it has cut: background alone %.4f (%.4f); take all 0 "
                  "(a non-adapting tick) %.4f (%.4f); launches %d / %d / %d" % ((T,) + db + off8 + (
                      res['bg_launches_' + k], res['adapt1_launches_' + k], res['adapt8_launches_' + k])))
            if args.parent:
                y, dy = _stat(res['parent_bg_ms_' + k]), _stat(res['parent_bg_device_ms_' + k])
                print("T = C = %d, the parent's tick with background %.4f (%.4f), its plan's device time %.4f (%.4f)" % ((T,) + y + dy))
                ok = two_sided('T = C = %d, the tick with background alone' % T, b, y, 'this tree', 'the parent') and ok
                ok = two_sided('T = C = %d, the plan device time with background alone' % T, db, dy, 'this tree', 'the parent') and ok
            ok = two_sided('T = C = %d, the plan device time of a non-adapting tick' % T, off8, db, 'adapt (take 0)', 'background alone') and ok
            mb = 4. * C * 480 * 640 / 1e6
            print("T = C = %d, device time of [a device copy puts the tick's raw frames back (%.1f MB read, %.1f MB written); the plan], so "
                  "that every run sees depths to adapt from: the copies alone %.4f (%.4f); background alone %.4f (%.4f); every=1: take all "
                  "0 %.4f (%.4f), take all 1 (an adapting tick) %.4f (%.4f); every=8: take all 0 %.4f (%.4f), take all 1 %.4f (%.4f)"
                  % ((T, mb, mb) + cp + al + of1 + on1 + of8 + on8))
            print("  share of source 0's pixels that one such adapting tick confirms: %.3f (every=1), %.3f (every=8)"
                  % (res['adapt1_confirmed_' + k], res['adapt8_confirmed_' + k]))
            two_sided('T = C = %d, take all 0 on raw frames (reported)' % T, of8, al, 'adapt (take 0)', 'background alone')
            for nm, on, of in (('every=1', on1, of1), ('every=8', on8, of8)):
                print("  an adapting tick, %s (six arrays read, the frame and `seen` stored, the rest where it changed; up to %.1f MB for "
                      "%.1f MB): %+.2f us over the same plan with take all 0, %+.2f us over background alone (spreads %.2f / %.2f / %.2f us; "
                      "no claim: reported)" % (nm, 12 * mb, 3 * mb, (on[0] - of[0]) * 1e3, (on[0] - al[0]) * 1e3, on[1] * 1e3, of[1] * 1e3, al[1] * 1e3))
            print("  a LOWER BOUND, not an adapting tick: take all 1 with the plan run again on the frames it has cut (the wall is holes by "
                  "then: the six arrays are read, nothing confirms, `seen` is not stored): %.4f (%.4f) at every=1, %.4f (%.4f) at every=8, "
                  "%+.2f / %+.2f us over background alone" % (rp1 + rp8 + ((rp1[0] - db[0]) * 1e3, (rp8[0] - db[0]) * 1e3)))
            print("  wall clock of the tick over background alone: %+.4f ms at every=1, %+.4f ms at every=8" % (a1[0] - b[0], a8[0] - b[0]))
        return 0 if ok else 1
    if args.calibrate:
        if not args.parent:
            raise SystemExit("--calibrate compares against --parent DIR")
        cfgs = args.configs or '8x8'
        res = run_legs([('multi', ytree, 'parent_'), ('fuse_tick', ytree, 'parent_'), ('multi', ROOT, ''), ('calib', ROOT, '')], cfgs)
        print("the calibrating tick (dpp_extrinsics_accumulate in dpp_pose_fuse's place) and the grouped tick after finish_calibration(), two "
              "groups of T / 2 tracks, against the ungrouped tick of this tree and the ungrouped and grouped ticks of the parent checkout; " + head)
        print("all times in ms per tick: median (spread = max - min over the repetitions)")
        ok = True
        for c in cfgs.split(','):
            T, C = (int(v) for v in c.split('x'))
            k = _key(T, C)
            m, y, fy = _stat(res['multi_ms_' + k]), _stat(res['parent_multi_ms_' + k]), _stat(res['parent_fuse_ms_' + k])
            a, f = _stat(res['calibrating_ms_' + k]), _stat(res['calibrated_ms_' + k])
            dm, dy, dfy = _stat(res['device_ms_' + k]), _stat(res['parent_device_ms_' + k]), _stat(res['parent_fuse_device_ms_' + k])
            da, df = _stat(res['calibrating_device_ms_' + k]), _stat(res['calibrated_device_ms_' + k])
            print("T = C = %d, wall clock: ungrouped %.4f (%.4f), parent %.4f (%.4f); calibrating %.4f (%.4f); calibrated grouped %.4f (%.4f), "
                  "parent's grouped %.4f (%.4f)" % ((T,) + m + y + a + f + fy))
            print("T = C = %d, plan device time: ungrouped %.4f (%.4f), parent %.4f (%.4f); calibrating %.4f (%.4f); calibrated grouped %.4f "
                  "(%.4f), parent's grouped %.4f (%.4f); launches %d / %d / %d" % ((T,) + dm + dy + da + df + dfy + (
                      res['launches_' + k], res['calibrating_launches_' + k], res['calibrated_launches_' + k])))
            ok = two_sided('T = C = %d, claim 1, the ungrouped tick' % T, m, y, 'this tree', 'the parent') and ok
            ok = two_sided('T = C = %d, claim 1, the calibrated grouped tick' % T, f, fy, 'this tree', "the parent's grouped tick") and ok
            acc_us, fuse_us = (da[0] - dm[0]) * 1e3, (df[0] - dm[0]) * 1e3
            bar = max(da[1], df[1], dm[1]) * 1e3
            fits = acc_us <= fuse_us + bar
            print("verdict T = C = %d, claim 2, plan device time over the ungrouped plan: accumulating %+.2f us, fusing %+.2f us, larger spread "
                  "%.2f us -> %s" % (T, acc_us, fuse_us, bar, 'holds' if fits else 'DOES NOT hold'))
            ok = fits and ok
            fin = res['finish_ms_' + k]
            print("finish_calibration() (one download of %d bytes per source, a 3 x 3 SVD each, one upload each, the plan dropped), wall clock: "
                  "%s ms after %d pairs per source (no claim)" % (20 * 8, ', '.join('%.3f' % v for v in fin), res['finish_pairs_' + k]))
        return 0 if ok else 1
    if args.mixed:
        cfgs = args.configs or '8x8'
        res = run_legs([('multi', ROOT, ''), ('mixed', ROOT, '')], cfgs)
        print("sources alternating 480x640 / 240x320 with cameras of their own (one plan, per-source table) against homogeneous 480x640 "
              "sources; " + head)
        print("all times in ms per tick: median (spread = max - min over the repetitions)")
        ok = True
        for c in cfgs.split(','):
            T, C = (int(v) for v in c.split('x'))
            k = _key(T, C)
            m, h = _stat(res['mixed_ms_' + k]), _stat(res['multi_ms_' + k])
            dm, dh = _stat(res['mixed_device_ms_' + k]), _stat(res['device_ms_' + k])
            print("T = %d, C = %d: mixed tick %.4f (%.4f), homogeneous tick %.4f (%.4f); plan, device time: mixed %.4f (%.4f), homogeneous %.4f "
                  "(%.4f); launches %d / %d" % ((T, C) + m + h + dm + dh + (res['mixed_launches_' + k], res['launches_' + k])))
            ok = two_sided('T = %d, C = %d' % (T, C), m, h, 'the mixed tick', 'the homogeneous tick') and ok
        return 0 if ok else 1
    if args.sequence:
        cfgs = args.configs or '1x1,8x8,16x16'
        res = run_legs([('multi', ROOT, ''), ('sequence', ROOT, '')], cfgs)
        print("MultiTracker.process_sequence (uploads of tick n + 1 under the plan of tick n) against the process() loop; " + head)
        print("all times in ms per tick: median (spread = max - min over the repetitions)")
        ok = True
        for c in cfgs.split(','):
            T, C = (int(v) for v in c.split('x'))
            k = _key(T, C)
            q, m, d = _stat(res['sequence_ms_' + k]), _stat(res['multi_ms_' + k]), _stat(res['device_ms_' + k])
            print("T = C = %d: process_sequence %.4f (%.4f), process loop %.4f (%.4f), plan device time %.4f (%.4f)" % ((T,) + q + m + d))
            within = two_sided('T = C = %d' % T, q, m, 'process_sequence', 'the process loop')
            faster = m[0] - q[0] > max(q[1], m[1])
            ok = (faster if C >= 8 else within) and ok
            if C >= 8:
                print("  claim at C >= 8 (faster by more than the larger spread): %s" % ('holds' if faster else 'DOES NOT hold'))
        return 0 if ok else 1
    res = run_legs([('yardstick', ytree, ''), ('multi', ROOT, '')], None)
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
