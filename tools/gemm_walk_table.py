#!/usr/bin/env python3
"""Every dpp_gemm variant-0 launch of the bs128 train step, joined with a single-stream kernel trace of that step:
   DPP_NO_SIDE_STREAM=1 rocprofv3 --kernel-trace -d DIR -o run -- python tools/step_profile.py 6 [size] [f32|bf16]
   python tools/gemm_walk_table.py DIR/.../run_results.db [size] [f32|bf16] > profiles/gemm_walk_after.txt
Per launch: role (forward / data gradient / filter gradient), the stream the step plan puts it on (the trace itself is single-stream), (M, N, K),
the stride of the row maps of A / B / C, tile, the grid dpp_gemm launches (dpp_gemm_walk_grid: the walking grid, or one workgroup per tile; with
DPP_GEMM_WALK=0 in the environment: the one-tile grids, to read a trace of a build without the walk), avg / min / max us of the matching
(kernel, grid) of the trace, the ALGORITHMIC bytes of the launch (operands + output + residual + BatchNorm input, from the shapes -- not a counter
reading) and those bytes per avg us.  Needs the GPU (the plan is built on the product runtime; the walking grid is the device's occupancy)."""
import ctypes as C
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'deep-prior-pp_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
from _names import pretty  # noqa: E402
from hipdp import engine  # noqa: E402
from hipdp.runtime import TorchHipRuntime  # noqa: E402
from net.resnet import ResNet, ResNetParams  # noqa: E402

db = sqlite3.connect(sys.argv[1])
size = int(sys.argv[2]) if len(sys.argv) > 2 else 128
bf16 = len(sys.argv) > 3 and sys.argv[3] == 'bf16'

# (family, BM, BN, BK, b_kc, grid) -> [durations in us]
trace = {}
for name, gx, gy, gz, us in db.execute("select name, grid_x/workgroup_x, grid_y/workgroup_y, grid_z/workgroup_z, (end-start)/1e3 from kernels"):
    m = re.match(r'gemm_(walk_)?kernel<(\d+), (\d+), (\d+), (\d+), (true|false), (true|false)', pretty(name))
    if not m:
        continue
    walk = m.group(1) is not None
    if not walk and m.group(6) != 'true':
        bkc, akc = m.group(7) == 'true', False
    else:
        bkc, akc = (m.group(6) if walk else m.group(7)) == 'true', True
    trace.setdefault((walk, akc, int(m.group(2)), int(m.group(3)), int(m.group(5)), bkc, (gx, gy, gz)), []).append(us)

rt = TorchHipRuntime()
net = ResNet(np.random.RandomState(23455), cfgParams=ResNetParams(type=0, wIn=size, hIn=size, batchSize=128, numJoints=1, nDims=30))
eng = engine.CompiledNet(net, train=True, runtime=rt, loss=dict(kind='embedding'), bf16=bf16)
lib = rt.lib
print("dpp_gemm variant-0 launches of the bs128 %d x %d %s train step (DPP_GEMM_WALK=%s)" % (size, size, 'bf16' if bf16 else 'f32', os.environ.get('DPP_GEMM_WALK', 'unset')))
print("%-16s %-5s %-6s %22s %-7s %-10s %-6s %-13s %6s %8s %8s %8s %8s %7s" %
      ('launch', 'role', 'stream', '(M, N, K)', 'maps', 'tile', 'kernel', 'grid', 'til/wg', 'avg_us', 'min_us', 'max_us', 'alg_MB', 'TB/s'))
for pname, plan in (('fwd', eng.fwd), ('bwd', eng.bwd)):
    for op, side in plan.ops:
        if getattr(op, 'fn', None) is not lib.dpp_gemm or op.keep[0].variant != 0:
            continue
        d = op.keep[0]
        role = 'wgrad' if not d.a_kc else ('fwd' if pname == 'fwd' else 'dgrad')
        gx, gy = C.c_int(0), C.c_int(0)
        walk = bool(lib.dpp_gemm_walk_grid(C.byref(d), C.byref(gx), C.byref(gy)))
        ntiles, ncol = -(-d.M // d.bm), -(-d.N // d.bn)
        grid = (gx.value, gy.value, 1) if walk else (ntiles, ncol, d.splitk)
        bk = 64 if not d.a_kc else (64 if d.K // d.splitk >= 128 else (32 if d.K > 16 else 16))
        us = trace.get((walk, bool(d.a_kc), d.bm, d.bn, bk, bool(d.b_kc), grid))
        esz = lambda bit: 2.0 if d.store & bit else 4.0            # noqa: E731
        mb = (esz(1) * d.M * d.K + esz(2) * d.K * d.N + (4.0 * d.splitk if d.splitk > 1 else esz(4)) * d.M * d.N +
              (esz(4) * d.M * d.N if d.residual else 0) + (esz(8) * d.M * d.N if d.epi.bn_x else 0)) / 1e6
        line = "%-16s %-5s %-6s %22s %-7s %-10s %-6s %-13s %6.2f" % (
            op.name[:16], role, 'branch' if side else 'main', '(%d, %d, %d)' % (d.M, d.N, d.K), '%d/%d/%d' % (d.mapA.s, d.mapB.s, d.mapC.s),
            '%dx%d/%d' % (d.bm, d.bn, bk), 'walk' if walk else 'tile', '<%d,%d,%d>' % grid, float(ntiles * ncol * d.splitk) / max(1, grid[0] * grid[1] * grid[2]))
        if us:
            avg = sum(us) / len(us)
            line += " %8.2f %8.2f %8.2f %8.1f %7.2f" % (avg, min(us), max(us), mb, mb / avg)
        else:
            line += "   (no such launch in the trace)"
        print(line)
print()
print("til/wg = tiles of the problem per workgroup of the launch.  Several launches of one (kernel, grid) share one avg / min / max (all its")
print("dispatches of the trace).")
