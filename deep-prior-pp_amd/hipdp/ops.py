"""
Prepared kernel launches ("ops") over the C ABI.  An op is built once (descriptor structs filled, device
pointers resolved) and then replayed every step with `op(stream)`; a `Plan` is an ordered list of ops.
Building is host logic only; nothing here computes on the CPU.
"""
import ctypes as C
import os

import numpy as np

from .lib import ST_A, ST_B, ST_BNX, ST_C, Act, BnEval, DppError, Epilogue, GemmDesc, ResblockDesc, RowMap, check


class Launch(object):
    """One prepared kernel launch.  `meta` = dict(kernel=<family>, flops=<algorithmic flops>, bytes=<algorithmic HBM
    bytes>) is what bench.py's roofline accounting reads."""
    __slots__ = ('fn', 'args', 'keep', 'name', 'meta', 'kernels')

    def __init__(self, fn, args, keep, name, meta=None, kernels=1):
        self.fn, self.args, self.keep, self.name, self.meta = fn, args, keep, name, meta
        self.kernels = kernels         # kernels the entry point issues (the plan recorder checks what it captured against this)

    def __call__(self, stream):
        st = self.fn(*self.args, stream)
        if st != 0:
            check(st, self.name)


class Fork(object):
    """Marker: from here on, launches added with side=True run on the side stream, which first waits for everything
    issued so far on the main stream."""
    name = 'fork'
    meta = None


class Join(object):
    """Marker: the main stream waits for everything issued so far on the side stream."""
    name = 'join'
    meta = None


# How a Plan issues its launches when it runs on a runtime:
#   native (default)  recorded once into a dpp_plan (include/dpp_hip.h) and re-issued from C++ on the two HIP streams;
#   graph             the same recording replayed as an explicit hipGraph (lanes = parallel branches);
#   graph1            one-lane hipGraph (everything chained in recorded order);
#   python            every launch is a ctypes call from the interpreter (what round 1 measured: host-bound).
LAUNCH_MODE = os.environ.get('DPP_LAUNCH_MODE', 'native')


def _side_streams():
    try:
        return max(1, min(8, int(os.environ.get('DPP_SIDE_STREAMS', '1'))))
    except ValueError:
        return 1


# Side streams of the native runner (csrc/plan.hip reads the same variable).  With S > 1 the launches between two forks are a group,
# groups are dealt round-robin to S streams that are NOT ordered against each other: a plan is only valid there if no side launch
# depends on a side launch of an earlier group.  The engine checks this number where it builds a plan that has such a dependency.
SIDE_STREAMS = _side_streams()


def one_side_stream_only(what):
    """Called where a plan is built whose gradient-branch groups depend on each other: refuse it for DPP_SIDE_STREAMS > 1."""
    if SIDE_STREAMS > 1:
        raise NotImplementedError("%s puts launches on the gradient branch that read what an EARLIER fork group of the branch wrote; with "
                                  "DPP_SIDE_STREAMS=%d the groups run on streams that are not ordered against each other.  Use one side "
                                  "stream (DPP_SIDE_STREAMS=1) or turn the knob off." % (what, SIDE_STREAMS))


class NativePlan(object):
    """A run of launches / fork / join markers recorded into a dpp_plan.  Recording calls every prepared op once with the
    library in recording mode: the C side keeps the resolved kernel, grid and a private copy of the arguments."""

    def __init__(self, rt, items, mode='native'):
        self.rt, self.lib, self.items, self.mode = rt, rt.lib, items, mode       # items keep the device buffers alive
        h = C.c_void_p()
        check(self.lib.dpp_plan_create(C.byref(h)), 'dpp_plan_create')
        self.handle = h
        lib = self.lib
        check(lib.dpp_plan_record_begin(h), 'dpp_plan_record_begin')
        try:
            lane = 0
            for op, side in items:
                if isinstance(op, Fork):
                    check(lib.dpp_plan_fork(h), 'dpp_plan_fork')
                elif isinstance(op, Join):
                    check(lib.dpp_plan_join(h), 'dpp_plan_join')
                else:
                    if int(bool(side)) != lane:
                        lane = int(bool(side))
                        check(lib.dpp_plan_record_lane(h, lane), 'dpp_plan_record_lane')
                    op(None)
        finally:
            check(lib.dpp_plan_record_end(h), 'dpp_plan_record_end')
        n = C.c_int()
        check(lib.dpp_plan_count(h, C.byref(n), None, None), 'dpp_plan_count')
        want = sum(op.kernels for op, _ in items if isinstance(op, Launch))
        if n.value != want:
            raise DppError("plan recording captured %d launches, expected %d" % (n.value, want))
        self.graph_ready = False

    def run(self, rt):
        two = getattr(rt, 'has_side_stream', False)
        if self.mode in ('graph', 'graph1') and not getattr(rt, 'is_emulator', False):
            if not self.graph_ready:
                check(self.lib.dpp_plan_graph_build(self.handle, 1 if (self.mode == 'graph' and two) else 0), 'dpp_plan_graph_build')
                self.graph_ready = True
            check(self.lib.dpp_plan_graph_launch(self.handle, rt.stream), 'dpp_plan_graph_launch')
            return
        st = self.lib.dpp_plan_run(self.handle, rt.stream, rt.side_stream if two else None)
        if st != 0:
            check(st, 'dpp_plan_run')

    def __del__(self):
        try:
            if self.handle:
                self.lib.dpp_plan_destroy(self.handle)
                self.handle = None
        except Exception:          # noqa: BLE001  (interpreter shutdown)
            pass


class _OpList(list):
    """The (op, side) list of a Plan.  Every mutation bumps `version`: a compiled plan stays valid exactly as long as the list it was
    recorded from is untouched -- the engine splices plans in place (Plan.ops[0:0] = ..., pop / insert) -- without rebuilding a
    400-tuple identity key on every step."""
    version = 0

    def _bump(name):
        base = getattr(list, name)

        def method(self, *a, **k):
            self.version += 1
            return base(self, *a, **k)
        method.__name__ = name
        return method

    for _n in ('append', 'extend', 'insert', 'pop', 'remove', 'clear', 'sort', 'reverse', '__setitem__', '__delitem__', '__iadd__', '__imul__'):
        locals()[_n] = _bump(_n)
    del _n, _bump


class Plan(object):
    """An ordered list of launches.  Every launch belongs to the main stream or (side=True) to an auxiliary stream that
    the runtime provides; Fork / Join markers order the two (event wait).  Run on a runtime, consecutive launches are
    compiled into NativePlans (one C call each); steps that are not kernel launches (collectives) stay Python calls
    between them."""

    def __init__(self, name=''):
        self.name = name
        self._ops = _OpList()  # (op, side)
        self.uses_side = False
        self._compiled = None

    @property
    def ops(self):
        return self._ops

    @ops.setter
    def ops(self, value):          # assigning a new list replaces the recording's source as well
        new = _OpList(value)
        new.version = self._ops.version + 1
        self._ops = new

    @staticmethod
    def concat(name, plans):
        out = Plan(name)
        for p in plans:
            out.ops.extend(p.ops)
            out.uses_side = out.uses_side or p.uses_side
        return out

    def add(self, op, side=False):
        if op is not None:
            self.ops.append((op, side))
            self.uses_side = self.uses_side or side
        return op

    def fork(self):
        self.ops.append((Fork(), False))

    def join(self):
        self.ops.append((Join(), False))

    def launches(self):
        return [o for (o, _) in self.ops if isinstance(o, Launch)]

    def steps(self):
        return [o for (o, _) in self.ops if not isinstance(o, (Fork, Join))]

    def _compile(self, rt):
        # keyed on the identity of the ops: a plan whose ops are replaced or reordered (the engine splices plans) must be re-recorded,
        # a recording freezes each launch's grid and arguments
        key = (id(rt), LAUNCH_MODE, id(self._ops), self._ops.version)
        if self._compiled is not None and self._compiled[0] == key:
            return self._compiled[1]
        segs, cur = [], []
        for op, side in self.ops:
            if isinstance(op, (Launch, Fork, Join)):
                cur.append((op, side))
            else:
                if cur:
                    segs.append(NativePlan(rt, cur, LAUNCH_MODE))
                    cur = []
                segs.append(op)
        if cur:
            segs.append(NativePlan(rt, cur, LAUNCH_MODE))
        self._compiled = (key, segs)
        return segs

    def segment_counts(self):
        """(native launch segments, host-issued steps) of this plan: a step that is not a kernel launch -- an RCCL collective -- ends the
        native segment in front of it and is issued from Python between two dpp_plan_run calls."""
        native, host, open_ = 0, 0, False
        for op, _ in self.ops:
            if isinstance(op, (Launch, Fork, Join)):
                if not open_:
                    native, open_ = native + 1, True
            else:
                host, open_ = host + 1, False
        return native, host

    def run(self, rt_or_stream):
        """rt_or_stream: a runtime (multi-stream aware) or a raw stream handle (single stream, side ops inline)."""
        rt = rt_or_stream if hasattr(rt_or_stream, 'stream') else None
        if rt is not None and LAUNCH_MODE != 'python':
            for seg in self._compile(rt):
                if isinstance(seg, NativePlan):
                    seg.run(rt)
                else:
                    seg(rt.stream)
            return
        if rt is None or not self.uses_side or not getattr(rt, 'has_side_stream', False):
            st = rt.stream if rt is not None else rt_or_stream
            for op, _ in self.ops:
                if not isinstance(op, (Fork, Join)):
                    op(st)
            return
        main, side = rt.stream, rt.side_stream
        for op, on_side in self.ops:
            if isinstance(op, Fork):
                rt.side_wait_main()
            elif isinstance(op, Join):
                rt.main_wait_side()
            else:
                op(side if on_side else main)

    def __len__(self):
        return len(self.launches())


def _p(buf):
    return None if buf is None else buf.ptr


BF16 = np.dtype(np.uint16)          # storage dtype of a bf16 activation tensor (runtime buffers have no bfloat16: the bits travel as uint16)


def _is16(buf):
    """Does this buffer hold a bf16-stored activation tensor (DPP_ST_* of include/dpp_hip.h)?"""
    return buf is not None and getattr(buf, 'dtype', None) == BF16


def _store(a=None, b=None, c=None, bnx=None):
    """DPP_ST_* mask of a call from the dtypes of the buffers in its A / B / C (+ residual) / epilogue.bn_x roles."""
    return (ST_A if _is16(a) else 0) | (ST_B if _is16(b) else 0) | (ST_C if _is16(c) else 0) | (ST_BNX if _is16(bnx) else 0)


def _esz(buf):
    return 2.0 if _is16(buf) else 4.0


def act(mode=0, mean=None, scale=None, beta=None, cmod=1, x2=None, aux=None, out=None):
    a = Act(_p(mean), _p(scale), _p(beta), int(mode), int(cmod), _p(x2), _p(aux), _p(out))
    a._keep = (mean, scale, beta, x2, aux, out)
    return a


def act_bn_bwd(bn, q, p, x, C, out=None):
    """Operand prologue of dpp_gemm's A in mode 4: the operand is the masked gradient G of BatchNorm `bn`, and the value used
    is dX = scale*G - p*(x - mean) - q (q = scale*c1, p = scale*inv_std*c2 from bn_bwd_finalize): bn_bwd_apply on the fly."""
    return act(Act.BN_BWD, mean=bn.mean, scale=bn.scale, beta=q, cmod=C, x2=x, aux=p, out=out)


def epilogue(stats=None, bn=None, bn_x=None, bn_relu=True, bn_partial=None):
    """dpp_epilogue: fused BatchNorm statistics (`stats`) and/or BatchNorm-backward mask + sums (`bn` = an object with
    mean / inv_std / scale / beta_buf buffers, `bn_x` the BatchNorm input, `bn_partial` the per-block sums)."""
    e = Epilogue()
    e.stats = _p(stats)
    if bn is not None:
        e.bn_x, e.bn_mean, e.bn_inv_std, e.bn_scale, e.bn_beta = bn_x.ptr, bn.mean.ptr, bn.inv_std.ptr, bn.scale.ptr, bn.beta_buf.ptr
        e.bn_relu, e.bn_partial = int(bn_relu), bn_partial.ptr
    e._bn_x = bn_x
    e._keep = (stats, bn, bn_x, bn_partial)
    return e


def gemm(rt, A, B, Cbuf, M, N, K, a_kc, b_kc, lda, ldb, ldc=0, mapA=None, mapB=None, mapC=None, actA=None, actB=None,
         bias=None, residual=None, splitk=1, partial=None, tile=(0, 0, 0), epi=None, variant=0, name='gemm', precision=0):
    """C = A_op . B_op, see dpp_gemm in include/dpp_hip.h."""
    d = GemmDesc()
    d.A, d.lda, d.a_kc = A.ptr, lda, int(a_kc)
    d.mapA = mapA or RowMap.identity()
    d.actA = actA or Act.none()
    d.B, d.ldb, d.b_kc = B.ptr, ldb, int(b_kc)
    d.mapB = mapB or RowMap.identity()
    d.actB = actB or Act.none()
    d.C, d.ldc = _p(Cbuf), ldc
    d.mapC = mapC or RowMap.identity()
    d.bias, d.residual = _p(bias), _p(residual)
    d.M, d.N, d.K = int(M), int(N), int(K)
    d.splitk, d.partial = int(splitk), _p(partial)
    d.bm, d.bn, d.wm = tile
    d.variant = int(variant)
    if epi is not None:
        d.epi = epi
    if _is16(residual) != _is16(Cbuf) and residual is not None and Cbuf is not None:
        raise ValueError("dpp_gemm: C and residual must be stored alike")
    d.store = _store(A, B, Cbuf, getattr(epi, '_bn_x', None) if epi is not None else None)
    d.precision = int(precision)
    meta = dict(kernel='gemm_mfma_bf16' if precision else 'gemm_mfma_f32', flops=2.0 * M * N * K,
                bytes=_esz(A) * M * K + _esz(B) * K * N + (4.0 * M * N * max(1, splitk) if splitk > 1 else _esz(Cbuf) * M * N) +
                (_esz(residual) * M * N if residual is not None else 0))
    return Launch(rt.lib.dpp_gemm, (C.byref(d),), (d, A, B, Cbuf, bias, residual, partial, actA, actB, epi), name, meta)


def gemm_variant_rows(rt, launch):
    """dpp_gemm_variant_rows for a launch built by gemm(): rows per workgroup of the kernel its `variant` asks for, or 0 when the C
    side would answer DPP_E_UNSUPPORTED (alignment, prologue mode, epilogue) -- the caller then describes it with variant 0."""
    return int(rt.lib.dpp_gemm_variant_rows(C.byref(launch.keep[0])))


def wgrad_stream(rt, dY, Co, X, Ci, M, rows_per_wave, partial, mapX=None, actX=None, name='wgrad_stream', precision=0):
    """dpp_wgrad_stream: the filter gradient of a 1x1 convolution as per-slice partials [slices][Co][Ci] (precision 1: bf16 MFMA operands,
    dpp_wgrad_stream_bf16, the shapes dpp_wgrad_stream_bf16_ok accepts)."""
    nsl = rt.lib.dpp_wgrad_stream_slices(Co, Ci, M, rows_per_wave)
    meta = dict(kernel='gemm_mfma_bf16' if precision else 'gemm_mfma_f32', flops=2.0 * M * Co * Ci,
                bytes=_esz(dY) * M * Co + 4.0 * nsl * Co * Ci + _esz(X) * M * Ci)
    return Launch(rt.lib.dpp_wgrad_stream_bf16 if precision else rt.lib.dpp_wgrad_stream, (dY.ptr, int(Co), X.ptr, int(Ci), C.byref(mapX) if mapX is not None else None, _actp(actX), int(M),
                                            int(rows_per_wave), partial.ptr, _store(a=dY, b=X)), (dY, X, partial, mapX, actX), name, meta)


def wgrad3_stream(rt, dY, Co, X, Ci, N, H, W, rows_per_wave, partial, actX=None, name='conv3x3_wgrad_stream'):
    """dpp_wgrad3_stream: the filter gradient of a 3x3 convolution as per-slice partials [slices][Co][9][Ci]."""
    nsl = rt.lib.dpp_wgrad3_stream_slices(Co, Ci, N, H, W, rows_per_wave)
    px = float(N) * H * W
    meta = dict(kernel='conv3x3_wgrad_mfma_f32', flops=2.0 * px * 9 * Ci * Co, bytes=4.0 * (px * Co + nsl * 9.0 * Ci * Co) + _esz(X) * px * Ci)
    return Launch(rt.lib.dpp_wgrad3_stream, (dY.ptr, int(Co), X.ptr, int(Ci), int(N), int(H), int(W), _actp(actX), int(rows_per_wave),
                                             partial.ptr, _store(a=dY, b=X)), (dY, X, partial, actX), name, meta)


def fc_gemm(rt, A, B, Cbuf, M, N, K, a_kc, b_kc, lda, ldb, ldc=0, actA=None, actB=None, bias=None, residual=None, splitk=1, partial=None,
            precision=0, kchunk=0, name='fc_gemm'):
    """dpp_fc_gemm: dpp_gemm's contract on the weight-streaming kernel (f32 or bf16 operands), see include/dpp_hip.h."""
    d = GemmDesc()
    d.A, d.lda, d.a_kc = A.ptr, lda, int(a_kc)
    d.mapA, d.mapB, d.mapC = RowMap.identity(), RowMap.identity(), RowMap.identity()
    d.actA = actA or Act.none()
    d.B, d.ldb, d.b_kc = B.ptr, ldb, int(b_kc)
    d.actB = actB or Act.none()
    d.C, d.ldc = _p(Cbuf), ldc
    d.bias, d.residual = _p(bias), _p(residual)
    d.M, d.N, d.K = int(M), int(N), int(K)
    d.splitk, d.partial = int(splitk), _p(partial)
    d.store = _store(A, B, Cbuf)
    if _is16(residual) != _is16(Cbuf) and residual is not None and Cbuf is not None:
        raise ValueError("dpp_fc_gemm: C and residual must be stored alike")
    meta = dict(kernel='fc_gemm_mfma_bf16' if precision else 'gemm_mfma_f32', flops=2.0 * M * N * K,
                bytes=4.0 * (M * K + K * N + M * N * (max(1, splitk) if splitk > 1 else 1) + (M * N if residual is not None else 0)))
    return Launch(rt.lib.dpp_fc_gemm, (C.byref(d), int(precision), int(kchunk)), (d, A, B, Cbuf, bias, residual, partial, actA, actB), name, meta)


def fc_wgrad_stream(rt, X, dY, dW, Nb, K, N, actX=None, name='fc_wgrad_stream'):
    """dpp_fc_wgrad_stream: dW [K][N] = act(X)^T . dY over the Nb rows, each output block owned by one wave (no partials)."""
    meta = dict(kernel='gemm_mfma_f32', flops=2.0 * Nb * K * N, bytes=4.0 * (Nb * K + Nb * N + K * N))
    return Launch(rt.lib.dpp_fc_wgrad_stream, (X.ptr, dY.ptr, dW.ptr, int(Nb), int(K), int(N), _actp(actX), _store(b=X)), (X, dY, dW, actX), name, meta)


def reduce_partials(rt, partial, nz, n, out, bias=None, nbias=1, name='reduce_partials'):
    return Launch(rt.lib.dpp_reduce_partials, (partial.ptr, int(nz), int(n), _p(bias), int(nbias), out.ptr),
                  (partial, out, bias), name, dict(kernel='reduce_partials', flops=float(nz) * n, bytes=4.0 * (nz + 1) * n))


def _actp(a):
    return C.byref(a) if a is not None else None


def conv3x3(rt, X, N, H, W, Ci, Wk, Co, Y, actX=None, bias=None, residual=None, bm=0, epi=None, name='conv3x3', precision=0):
    px = float(N) * H * W
    meta = dict(kernel='conv3x3_mfma_bf16' if precision else 'conv3x3_mfma_f32', flops=2.0 * px * 9 * Ci * Co,
                bytes=px * (_esz(X) * Ci + _esz(Y) * Co + (_esz(residual) * Co if residual is not None else 0)) + 4.0 * 9 * Ci * Co)
    if residual is not None and _is16(residual) != _is16(Y):
        raise ValueError("dpp_conv3x3: Y and residual must be stored alike")
    st = _store(X, None, Y, getattr(epi, '_bn_x', None) if epi is not None else None)
    return Launch(rt.lib.dpp_conv3x3_bf16 if precision else rt.lib.dpp_conv3x3, (X.ptr, N, H, W, Ci, _actp(actX), Wk.ptr, Co, _p(bias), _p(residual), Y.ptr, bm,
                                       C.byref(epi) if epi is not None else None, st),
                  (X, Wk, Y, actX, bias, residual, epi), name, meta)


def conv3x3_stream(rt, X, N, H, W, Cc, Wk, Y, actX=None, bias=None, epi=None, name='conv3x3'):
    """dpp_conv3x3_stream: the 3x3 convolution of a narrow square layer on the barrier-free kernel (float32 tensors only)."""
    _f32_only('dpp_conv3x3_stream', X, Y, getattr(epi, '_bn_x', None) if epi is not None else None)
    px = float(N) * H * W
    meta = dict(kernel='conv3x3_mfma_f32', flops=2.0 * px * 9 * Cc * Cc, bytes=px * 8.0 * Cc + 4.0 * 9 * Cc * Cc)
    return Launch(rt.lib.dpp_conv3x3_stream, (X.ptr, N, H, W, Cc, _actp(actX), Wk.ptr, _p(bias), Y.ptr, C.byref(epi) if epi is not None else None),
                  (X, Wk, Y, actX, bias, epi), name, meta)


def conv3x3_wtrans(rt, Wk, Co, Ci, Wd, name='conv3x3_wtrans'):
    return Launch(rt.lib.dpp_conv3x3_wtrans, (Wk.ptr, Co, Ci, Wd.ptr), (Wk, Wd), name)


def conv3x3_wtrans_multi(rt, jobs, name='conv3x3_wtrans'):
    """jobs: [(Wk buffer, Co, Ci, Wd buffer)]: the mirrored data-gradient weights of every 3x3 layer in ONE launch."""
    import struct
    assert rt.lib.dpp_wtrans_job_bytes() == 32
    raw, block0 = b'', 0
    for (Wk, Co, Ci, Wd) in jobs:
        raw += struct.pack('<QQiiii', Wk.ptr, Wd.ptr, int(Co), int(Ci), block0, 0)
        block0 += -(-(Co * 9 * Ci) // 256)
    table = rt.upload(np.frombuffer(raw, np.uint8).copy())
    return Launch(rt.lib.dpp_conv3x3_wtrans_multi, (table.ptr, len(jobs), block0), (table, list(jobs)), name)


def conv3x3_wgrad(rt, X, N, H, W, Ci, dY, Co, partial, actX=None, bm=64, name='conv3x3_wgrad', precision=0):
    """precision 1: bf16 MFMA operands (dpp_conv3x3_wgrad_bf16; layers dpp_conv3x3_wgrad_bf16_ok accepts)."""
    px = float(N) * H * W
    nblk = rt.lib.dpp_conv3x3_wgrad_blocks(N, H, W, Ci, Co, bm)
    meta = dict(kernel='conv3x3_wgrad_mfma_bf16' if precision else 'conv3x3_wgrad_mfma_f32', flops=2.0 * px * 9 * Ci * Co,
                bytes=_esz(dY) * px * Co + 4.0 * nblk * 9.0 * Ci * Co + _esz(X) * px * Ci)
    fn = rt.lib.dpp_conv3x3_wgrad_bf16 if precision else rt.lib.dpp_conv3x3_wgrad
    return Launch(fn, (X.ptr, N, H, W, Ci, _actp(actX), dY.ptr, Co, partial.ptr, bm, _store(a=X, b=dY)),
                  (X, dY, partial, actX), name, meta)


def stem_fwd(rt, X, N, H, W, Wk, bias, Co, Y, argmax, stats=None, name='stem_fwd'):
    px = float(N) * H * W
    return Launch(rt.lib.dpp_stem_fwd, (X.ptr, N, H, W, Wk.ptr, bias.ptr, Co, Y.ptr, _p(argmax), _p(stats), _store(c=Y)), (X, Wk, bias, Y, argmax, stats), name,
                  dict(kernel='stem_fwd_mfma_f32', flops=2.0 * px * 25 * Co, bytes=4.0 * px + px / 4 * Co * (1.0 + _esz(Y))))


def stem_wgrad(rt, X, N, H, W, dY, argmax, Co, partial, tiles_per_block, name='stem_wgrad'):
    px = float(N) * H * W
    return Launch(rt.lib.dpp_stem_wgrad, (X.ptr, N, H, W, dY.ptr, argmax.ptr, Co, partial.ptr, tiles_per_block),
                  (X, dY, argmax, partial), name, dict(kernel='stem_wgrad', flops=2.0 * px / 4 * Co * 25, bytes=4.0 * px + px / 4 * Co * 5.0))


def convpool_fwd(rt, X, N, H, W, Ci, Wk, kh, kw, pad, Co, pool, bias, Y, ties=None, actX=None, name='convpool_fwd'):
    px = float(N) * (H + 2 * pad - kh + 1) * (W + 2 * pad - kw + 1)
    return Launch(rt.lib.dpp_convpool_fwd, (X.ptr, N, H, W, Ci, _actp(actX), Wk.ptr, kh, kw, pad, Co, pool, bias.ptr, Y.ptr, _p(ties)),
                  (X, Wk, bias, Y, ties, actX), name,
                  dict(kernel='convpool_fwd', flops=2.0 * px * kh * kw * Ci * Co, bytes=4.0 * N * H * W * Ci + 6.0 * px / (pool * pool) * Co))


def convpool_wgrad(rt, X, N, H, W, Ci, dY, ties, kh, kw, pad, Co, pool, partial, actX=None, name='convpool_wgrad'):
    px = float(N) * (H + 2 * pad - kh + 1) * (W + 2 * pad - kw + 1) / (pool * pool)
    return Launch(rt.lib.dpp_convpool_wgrad, (X.ptr, N, H, W, Ci, _actp(actX), dY.ptr, _p(ties), kh, kw, pad, Co, pool, partial.ptr),
                  (X, dY, ties, partial, actX), name,
                  dict(kernel='convpool_wgrad', flops=2.0 * px * kh * kw * Ci * Co, bytes=4.0 * N * H * W * Ci + 6.0 * px * Co))


def convpool_dgrad(rt, dY, ties, N, H, W, Ci, Wk, kh, kw, pad, Co, pool, dX, name='convpool_dgrad'):
    px = float(N) * (H + 2 * pad - kh + 1) * (W + 2 * pad - kw + 1) / (pool * pool)
    return Launch(rt.lib.dpp_convpool_dgrad, (dY.ptr, _p(ties), N, H, W, Ci, Wk.ptr, kh, kw, pad, Co, pool, dX.ptr), (dY, ties, Wk, dX), name,
                  dict(kernel='convpool_dgrad', flops=2.0 * px * kh * kw * Ci * Co, bytes=4.0 * N * H * W * Ci + 6.0 * px * Co))


def bn_stats_partial(rt, X, M, Cc, rpb, partial, name='bn_stats_partial'):
    return Launch(rt.lib.dpp_bn_stats_partial, (X.ptr, M, Cc, rpb, partial.ptr, _store(a=X)), (X, partial), name,
                  dict(kernel='bn_stats_partial', flops=3.0 * M * Cc, bytes=_esz(X) * M * Cc))


def bn_finalize(rt, partial, nb, M, rpb, Cc, gamma, eps, mean, inv_std, scale, run_mean=None, run_inv_std=None, alpha=0.0,
                nseg=1, name='bn_finalize'):
    """partial: nseg segments of [2][Cc][nb] (nb blocks per segment), M rows over all segments."""
    return Launch(rt.lib.dpp_bn_finalize, (partial.ptr, nb, int(nseg), M, rpb, Cc, gamma.ptr, float(eps), mean.ptr, inv_std.ptr, scale.ptr,
                                           _p(run_mean), _p(run_inv_std), float(alpha)),
                  (partial, gamma, mean, inv_std, scale, run_mean, run_inv_std), name,
                  dict(kernel='bn_finalize', flops=0.0, bytes=8.0 * nb * Cc))


def bn_eval_coeffs(rt, gamma, run_mean, run_inv_std, Cc, mean, inv_std, scale, name='bn_eval_coeffs'):
    return Launch(rt.lib.dpp_bn_eval_coeffs, (gamma.ptr, run_mean.ptr, run_inv_std.ptr, Cc, mean.ptr, inv_std.ptr, scale.ptr),
                  (gamma, run_mean, run_inv_std, mean, inv_std, scale), name)


def bn_eval_coeffs_multi(rt, jobs, name='bn_eval_coeffs'):
    """jobs: [(gamma, run_mean, run_inv_std, C, mean, inv_std, scale)] -- dpp_bn_eval_coeffs for every BatchNorm of a net in ONE launch."""
    import struct
    assert rt.lib.dpp_bn_eval_job_bytes() == 56
    raw, block0 = b'', 0
    for (gamma, rm, ris, Cc, mean, inv_std, scale) in jobs:
        raw += struct.pack('<QQQQQQii', gamma.ptr, rm.ptr, ris.ptr, mean.ptr, inv_std.ptr, scale.ptr, int(Cc), block0)
        block0 += -(-int(Cc) // 256)
    table = rt.upload(np.frombuffer(raw, np.uint8).copy())
    return Launch(rt.lib.dpp_bn_eval_coeffs_multi, (table.ptr, len(jobs), block0), (table, list(jobs)), name,
                  dict(kernel='bn_eval_coeffs', flops=0.0, bytes=24.0 * sum(int(j[3]) for j in jobs)))


def bn_eval(mean, inv_std, gamma, beta):
    """dpp_bn_eval: a BatchNorm in deterministic mode as the fused block kernel reads it (stored statistics + affine parameters)."""
    b = BnEval(mean.ptr, inv_std.ptr, gamma.ptr, beta.ptr)
    b._keep = (mean, inv_std, gamma, beta)
    return b


def resblock_eval(rt, X, N, H, W, Cin, stride, Cout, Nb, bn0, bn1, bn2, W1, b1, W2, b2, W3, b3, Y, Wsc=None, bsc=None, name='resblock_eval'):
    """dpp_resblock_eval: one pre-activation bottleneck block of the deterministic forward pass in one launch (csrc/resblock.hip)."""
    d = ResblockDesc()
    d.store = _store(a=X, c=Y)
    Ho, Wo = -(-H // stride), -(-W // stride)
    d.X, d.N, d.H, d.W, d.Cin = X.ptr, int(N), int(H), int(W), int(Cin)
    d.stride, d.Ho, d.Wo, d.Cout, d.Nb = int(stride), Ho, Wo, int(Cout), int(Nb)
    d.bn0, d.bn1, d.bn2 = bn0, bn1, bn2
    d.W1, d.b1, d.W2, d.b2, d.W3, d.b3 = W1.ptr, b1.ptr, W2.ptr, b2.ptr, W3.ptr, b3.ptr
    d.Wsc, d.bsc, d.Y = _p(Wsc), _p(bsc), Y.ptr
    px = float(N) * Ho * Wo
    flops = 2.0 * px * (Cin * Nb + 9.0 * Nb * Nb + Nb * Cout + (Cin * Cout if Wsc is not None else 0))
    byts = _esz(X) * (float(N) * H * W * Cin + (px * Cout if Wsc is None else 0)) + _esz(Y) * px * Cout + 4.0 * (Cin * Nb + 9.0 * Nb * Nb + Nb * Cout)
    return Launch(rt.lib.dpp_resblock_eval, (C.byref(d),), (d, X, Y, bn0, bn1, bn2, W1, b1, W2, b2, W3, b3, Wsc, bsc), name,
                  dict(kernel='resblock_eval_mfma_f32', flops=flops, bytes=byts))


def bn_bwd_reduce(rt, dA, X, M, Cc, mean, inv_std, scale, beta, relu, G, rpb, partial, name='bn_bwd_reduce'):
    return Launch(rt.lib.dpp_bn_bwd_reduce, (dA.ptr, X.ptr, M, Cc, mean.ptr, inv_std.ptr, scale.ptr, beta.ptr, int(relu), G.ptr, rpb,
                                             partial.ptr, _store(a=dA, c=G, bnx=X)), (dA, X, mean, inv_std, scale, beta, G, partial), name,
                  dict(kernel='bn_bwd_reduce', flops=8.0 * M * Cc, bytes=(8.0 + _esz(X)) * M * Cc))


def bn_bwd_finalize(rt, partial, nb, M, Cc, dbeta, dgamma, c1, c2, nseg=1, bn=None, q=None, p=None, name='bn_bwd_finalize'):
    """q, p (with bn): also write the constants of the mode-4 operand prologue (act_bn_bwd)."""
    return Launch(rt.lib.dpp_bn_bwd_finalize, (partial.ptr, nb, int(nseg), M, Cc, dbeta.ptr, dgamma.ptr, c1.ptr, c2.ptr,
                                               _p(bn.inv_std) if q is not None else None, _p(bn.scale) if q is not None else None,
                                               _p(q), _p(p)),
                  (partial, dbeta, dgamma, c1, c2, bn, q, p), name, dict(kernel='bn_bwd_finalize', flops=0.0, bytes=8.0 * nb * Cc))


def bn_bwd_apply(rt, G, X, M, Cc, mean, inv_std, scale, c1, c2, dX, add=None, rpb=None, colsum=None, name='bn_bwd_apply'):
    rpb = rpb or max(32, -(-M // 1024))
    if add is not None and _is16(add) != _is16(dX):
        raise ValueError("dpp_bn_bwd_apply: dX and the gradient added to it must be stored alike")
    return Launch(rt.lib.dpp_bn_bwd_apply, (G.ptr, X.ptr, M, Cc, mean.ptr, inv_std.ptr, scale.ptr, c1.ptr, c2.ptr, _p(add), dX.ptr,
                                            int(rpb), _p(colsum), _store(a=G, c=dX, bnx=X)),
                  (G, X, mean, inv_std, scale, c1, c2, add, dX, colsum), name,
                  dict(kernel='bn_bwd_apply', flops=6.0 * M * Cc, bytes=((12.0 if add is not None else 8.0) + _esz(X)) * M * Cc))


def bn_bwd_finalize_apply(rt, G, X, M, Cc, mean, inv_std, scale, partial, nb, dX, dbeta, dgamma, add=None, rpb=32, colsum=None,
                          name='bn_bwd_finalize_apply'):
    """dpp_bn_bwd_finalize_apply: the finalize of the per-block sums and the apply pass of a BatchNorm backward in one launch."""
    if add is not None and _is16(add) != _is16(dX):
        raise ValueError("dpp_bn_bwd_finalize_apply: dX and the gradient added to it must be stored alike")
    return Launch(rt.lib.dpp_bn_bwd_finalize_apply, (G.ptr, X.ptr, M, Cc, mean.ptr, inv_std.ptr, scale.ptr, partial.ptr, int(nb), _p(add), dX.ptr,
                                                     int(rpb), _p(colsum), dbeta.ptr, dgamma.ptr, _store(a=G, c=dX, bnx=X)),
                  (G, X, mean, inv_std, scale, partial, add, dX, colsum, dbeta, dgamma), name,
                  dict(kernel='bn_bwd_apply', flops=6.0 * M * Cc, bytes=((12.0 if add is not None else 8.0) + _esz(X)) * M * Cc))


def colsum_partial(rt, X, M, Cc, rpb, partial, name='colsum_partial'):
    if _is16(X):
        raise NotImplementedError("dpp_colsum_partial reads float32 gradients")
    return Launch(rt.lib.dpp_colsum_partial, (X.ptr, M, Cc, rpb, partial.ptr), (X, partial), name,
                  dict(kernel='colsum_partial', flops=1.0 * M * Cc, bytes=4.0 * M * Cc))


def loss_sse(rt, out, y, rows, d, denom, cost, dout=None, name='loss_sse'):
    return Launch(rt.lib.dpp_loss_sse, (out.ptr, y.ptr, rows, d, denom, cost.ptr, _p(dout)), (out, y, cost, dout), name)


def reduce_partials_loss(rt, partial, nz, rows, d, out, bias, y, denom, cost, dout=None, name='reduce_partials_loss'):
    """reduce_partials (+ bias) of the net's last HiddenLayer and loss_sse on its output in one launch."""
    n = rows * d
    return Launch(rt.lib.dpp_reduce_partials_loss, (partial.ptr, nz, rows, d, _p(bias), out.ptr, y.ptr, denom, cost.ptr, _p(dout)),
                  (partial, out, bias, y, cost, dout), name, dict(kernel='reduce_partials', flops=float(nz) * n, bytes=4.0 * (nz + 3) * n))


def loss_sse_bcast(rt, out, y, n, cost, dout=None, err=None, name='loss_sse_bcast'):
    return Launch(rt.lib.dpp_loss_sse_bcast, (out.ptr, y.ptr, n, cost.ptr, _p(dout), _p(err)), (out, y, cost, dout, err), name)


def error_l2(rt, out, y, rows, d, err, name='error_l2'):
    return Launch(rt.lib.dpp_error_l2, (out.ptr, y.ptr, rows, d, err.ptr), (out, y, err), name)


def adam(rt, w, g, m, v, n, hyper, name='adam', tick=False):
    """tick: the launch also advances the step count t (dpp_adam_ticked) -- no dpp_adam_tick launch behind it."""
    return Launch(rt.lib.dpp_adam_ticked if tick else rt.lib.dpp_adam, (w.ptr, g.ptr, m.ptr, v.ptr, n, hyper.ptr), (w, g, m, v, hyper), name,
                  dict(kernel='adam', flops=12.0 * n, bytes=28.0 * n))


def _f32_only(what, *bufs):
    if any(_is16(b) for b in bufs):
        raise NotImplementedError("%s reads / writes float32 tensors only (a bf16-stored tensor reached it)" % what)


def axpy(rt, y, x, alpha, n, name='axpy'):
    _f32_only('dpp_axpy', y, x)
    return Launch(rt.lib.dpp_axpy, (y.ptr, x.ptr, float(alpha), n), (y, x), name)


def sumsq(rt, x, n, alpha, out, accumulate, name='sumsq'):
    return Launch(rt.lib.dpp_sumsq, (x.ptr, n, float(alpha), out.ptr, int(accumulate)), (x, out), name)


def segment_table(rt, base, views):
    """(offset, length) pairs of `views` inside the flat buffer `base`, as a device array for sumsq_multi / axpy_multi."""
    seg = []
    for v in views:
        off = (v.ptr - base.ptr) // 4
        assert 0 <= off and off + v.size <= base.size and (v.ptr - base.ptr) % 4 == 0, "view outside the flat buffer"
        seg += [off, v.size]
    return rt.upload(np.asarray(seg, np.int64)), len(seg) // 2


def sumsq_multi(rt, base, seg, nseg, alpha, out, accumulate, name='sumsq_multi'):
    ws = rt.alloc(int(rt.lib.dpp_sumsq_multi_workspace_bytes()) // 8, np.float64, zero=False)
    return Launch(rt.lib.dpp_sumsq_multi, (base.ptr, seg.ptr, int(nseg), float(alpha), ws.ptr, out.ptr, int(accumulate)),
                  (base, seg, ws, out), name, kernels=2)


def axpy_multi(rt, ybase, xbase, seg, nseg, alpha, name='axpy_multi'):
    return Launch(rt.lib.dpp_axpy_multi, (ybase.ptr, xbase.ptr, seg.ptr, int(nseg), float(alpha)), (ybase, xbase, seg), name)


def scale(rt, x, y, n, a=1.0, relu=False, mask=None, name='scale'):
    return Launch(rt.lib.dpp_scale, (x.ptr, _p(mask), float(a), int(relu), y.ptr, n), (x, y, mask), name)


def relu_bwd(rt, dy, pre, g, n, a=1.0, mask=None, name='relu_bwd'):
    _f32_only('dpp_relu_bwd', dy, pre, g)
    return Launch(rt.lib.dpp_relu_bwd, (dy.ptr, pre.ptr, _p(mask), float(a), g.ptr, n), (dy, pre, g, mask), name)


def augment_prepare(rt, img, com3d, cube, Mcrop, gt3d, B, J, dsz, cam, records, out_y, mode=None, off=None, rot=None, sc=None,
                    mode_table=None, n_modes=0, seed=0, counter=0, sigma_com=5., sigma_sc=0.02, rot_range=180.,
                    pca_mean=None, pca_comp=None, E=0, out_mode=None, counter_dev=None, norm_zero_one=False, name='augment_prepare'):
    fx, fy, ux, uy, flip = cam
    return Launch(rt.lib.dpp_augment_prepare,
                  (img.ptr, com3d.ptr, cube.ptr, Mcrop.ptr, gt3d.ptr, B, J, dsz, _p(mode), _p(off), _p(rot), _p(sc), _p(mode_table),
                   n_modes, seed, counter, float(sigma_com), float(sigma_sc), float(rot_range), float(fx), float(fy), float(ux),
                   float(uy), int(flip), int(bool(norm_zero_one)), _p(pca_mean), _p(pca_comp), E, records.ptr, out_y.ptr, _p(out_mode),
                   _p(counter_dev)),
                  (img, com3d, cube, Mcrop, gt3d, mode, off, rot, sc, mode_table, pca_mean, pca_comp, records, out_y, out_mode,
                   counter_dev), name)


def augment_warp(rt, img, records, B, dsz, out, name='augment_warp'):
    return Launch(rt.lib.dpp_augment_warp, (img.ptr, records.ptr, B, dsz, out.ptr), (img, records, out), name,
                  dict(kernel='augment_warp', flops=40.0 * B * dsz * dsz, bytes=8.0 * B * dsz * dsz))


def augment(rt, img, com3d, cube, Mcrop, gt3d, B, J, dsz, cam, out_x, out_y, records=None, mode=None, off=None, rot=None, sc=None,
            mode_table=None, n_modes=0, seed=0, counter=0, sigma_com=5., sigma_sc=0.02, rot_range=180., pca_mean=None, pca_comp=None,
            E=0, out_mode=None, counter_dev=None, ticket=None, sample0=0, global_batch=0, splits=0, norm_zero_one=False, binarize=False,
            name='augment'):
    """prepare + warp as one launch (dpp_augment); with `ticket` it also advances the device draw counter."""
    fx, fy, ux, uy, flip = cam
    return Launch(rt.lib.dpp_augment,
                  (img.ptr, com3d.ptr, cube.ptr, Mcrop.ptr, gt3d.ptr, B, J, dsz, _p(mode), _p(off), _p(rot), _p(sc), _p(mode_table),
                   n_modes, seed, counter, float(sigma_com), float(sigma_sc), float(rot_range), float(fx), float(fy), float(ux),
                   float(uy), int(flip), int(bool(norm_zero_one)) | (2 if binarize else 0), _p(pca_mean), _p(pca_comp), E, _p(records), out_x.ptr, out_y.ptr,
                   _p(out_mode), _p(counter_dev), _p(ticket), int(sample0), int(global_batch), int(splits)),
                  (img, com3d, cube, Mcrop, gt3d, mode, off, rot, sc, mode_table, pca_mean, pca_comp, records, out_x, out_y, out_mode,
                   counter_dev, ticket), name, dict(kernel='augment', flops=40.0 * B * dsz * dsz, bytes=8.0 * B * dsz * dsz))


class AugmentState(object):
    """The device-resident draw counter (+ the ticket word that advances it) of one augmentation stream, shared by the
    launches over all data slices; sample0 / global_batch key the draws by the GLOBAL sample index (data parallelism)."""

    def __init__(self, rt, B, seed=0, sample0=0, global_batch=0):
        self.rt, self.B, self.seed, self.sample0, self.global_batch = rt, int(B), int(seed), int(sample0), int(global_batch or B)
        self.counter = rt.alloc(1, np.int64)
        self.ticket = rt.alloc(1, np.int32)

    def ops(self, img, com3d, cube, Mcrop, gt3d, J, dsz, cam, out_x, out_y, **kw):
        return [augment(self.rt, img, com3d, cube, Mcrop, gt3d, self.B, J, dsz, cam, out_x, out_y, seed=self.seed, counter=0,
                        counter_dev=self.counter, ticket=self.ticket, sample0=self.sample0, global_batch=self.global_batch, **kw)]


def crop_prepare(rt, frames, B, H, W, com, cube, fx, fy, dsz, records, M_out=None, stretch=False, name='crop_prepare'):
    return Launch(rt.lib.dpp_crop_prepare, (frames.ptr, B, H, W, com.ptr, cube.ptr, float(fx), float(fy), dsz, int(bool(stretch)), records.ptr,
                                            _p(M_out)),
                  (frames, com, cube, records, M_out), name, dict(kernel='crop_prepare', flops=2.0 * B * H * W, bytes=4.0 * B * H * W))


def crop_com(rt, frames, records, B, H, W, com_out, name='crop_com'):
    ws = rt.alloc(max(1, int(rt.lib.dpp_crop_com_workspace_bytes(B)) // 8), np.float64, zero=False)     # per-band partial sums
    return Launch(rt.lib.dpp_crop_com, (frames.ptr, records.ptr, B, H, W, ws.ptr, com_out.ptr), (frames, records, ws, com_out), name,
                  kernels=2)


# The launches that take `tracks=` (and frame_range / frame_ingest, which take `table=`) are ONE op over a family of C entry points
# (include/dpp_hip.h): without a TrackSet the plain symbol on B frames; with one (below) the *_ix symbol on tracks.T rows, row t in
# frame src[t] (B is not read); with one that has a SourceTable the *_src symbol, which reads the frame size, the camera and fx / fy
# per source from the table (H, W, cam, fx, fy are not read: pass None).
def crop_warp(rt, frames, records, B, H, W, dsz, out, normalize=True, nd_value=0.0, name='crop_warp', tracks=None):
    tail = (dsz, int(bool(normalize)), float(nd_value), out.ptr)
    if tracks is None:
        fn, args, keep = rt.lib.dpp_crop_warp, (frames.ptr, records.ptr, B, H, W) + tail, (frames, records, out)
    elif tracks.table is None:
        B = tracks.T
        fn, args, keep = rt.lib.dpp_crop_warp_ix, (frames.ptr, records.ptr, B, tracks.src.ptr, H, W) + tail, (frames, records, tracks.src, out)
    else:
        B, tab = tracks.T, tracks.table.dev
        fn, args, keep = rt.lib.dpp_crop_warp_src, (frames.ptr, records.ptr, B, tracks.src.ptr, tab.ptr) + tail, (frames, records, tracks.src, tab, out)
    return Launch(fn, args, keep, name, dict(kernel='crop_warp', flops=10.0 * B * dsz * dsz, bytes=8.0 * B * dsz * dsz))


CROP_NORMALIZE, CROP_BILINEAR, CROP_NO_RANGE, CROP_NO_THRESH, CROP_FLIP_X = 1, 2, 4, 8, 16      # dpp_crop_warp_ex flags


def crop_warp_ex(rt, frames, records, B, H, W, dsz, out, flags=0, nd_value=0.0, fill_value=None, pad_value=0.0, name='crop_warp_ex',
                 tracks=None):
    """dpp_crop_warp_ex: the initial crop with the bilinear mode and applyCrop3D's options (fill_value defaults to nd_value).  With
    tracks, CROP_FLIP_X comes per track from tflags[t] & POSE_HAND_RIGHT, the other flags hold for all tracks."""
    fill = float(nd_value) if fill_value is None else float(fill_value)
    taps = 4 if flags & CROP_BILINEAR else 1
    tail = (dsz, int(flags), float(nd_value), fill, float(pad_value), out.ptr)
    if tracks is None:
        fn, args, keep = rt.lib.dpp_crop_warp_ex, (frames.ptr, records.ptr, B, H, W) + tail, (frames, records, out)
    elif tracks.table is None:
        B, src, tf = tracks.T, tracks.src, tracks.tflags
        fn, args, keep = rt.lib.dpp_crop_warp_ex_ix, (frames.ptr, records.ptr, B, src.ptr, tf.ptr, H, W) + tail, (frames, records, src, tf, out)
    else:
        B, src, tf, tab = tracks.T, tracks.src, tracks.tflags, tracks.table.dev
        fn, args = rt.lib.dpp_crop_warp_ex_src, (frames.ptr, records.ptr, B, src.ptr, tf.ptr, tab.ptr) + tail
        keep = (frames, records, src, tf, tab, out)
    return Launch(fn, args, keep, name,
                  dict(kernel='crop_warp', flops=(30.0 if taps == 4 else 10.0) * B * dsz * dsz, bytes=(4.0 * taps + 4.0) * B * dsz * dsz))


def resize_crops(rt, src, B, sh, sw, dh, dw, out, bilinear=False, nd_value=0.0, name='resize_crops'):
    """dpp_resize_crops: resizeCrop of B same-size crops, nearest neighbour or bilinearResize."""
    return Launch(rt.lib.dpp_resize_crops, (src.ptr, B, sh, sw, dh, dw, int(bool(bilinear)), float(nd_value), out.ptr), (src, out), name,
                  dict(kernel='resize_crops', flops=(30.0 if bilinear else 2.0) * B * dh * dw, bytes=4.0 * B * (sh * sw + dh * dw)))


def recrop(rt, crops, B, h, w, M, Mnew, th, tw, out, background=0.0, nv_val=0.0, zrange=None, name='recrop'):
    """dpp_recrop: recropHand of B crops (M, Mnew [B][9] float64; zrange [B][2] float32 or None for thresh_z=False)."""
    return Launch(rt.lib.dpp_recrop, (crops.ptr, B, h, w, M.ptr, Mnew.ptr, th, tw, float(background), float(nv_val), int(zrange is not None),
                                      _p(zrange), out.ptr),
                  (crops, M, Mnew, zrange, out), name, dict(kernel='recrop', flops=20.0 * B * th * tw, bytes=4.0 * B * (h * w + th * tw)))


def inverse_crop(rt, crops, B, ch, cw, bounds, H, W, out, bilinear=False, nd_value=0.0, background=0.0, zrange=None, name='inverse_crop'):
    """dpp_inverse_crop: getInverseCrop of B crops into [B][H][W] frames (bounds [B][4] int32; zrange [B][2] float32 or None)."""
    return Launch(rt.lib.dpp_inverse_crop, (crops.ptr, B, ch, cw, bounds.ptr, _p(zrange), H, W, int(bool(bilinear)), float(nd_value),
                                            float(background), int(zrange is not None), out.ptr),
                  (crops, bounds, zrange, out), name,
                  dict(kernel='inverse_crop', flops=(30.0 if bilinear else 4.0) * B * H * W, bytes=4.0 * B * (ch * cw + H * W)))


def crop_refine(rt, frames, records, B, H, W, com_in, cube, net_out, cam, com_out, gt3d_orig=None, J=0, pca_mean=None, pca_comp=None, E=0,
                com3d_out=None, gt3d_crop=None, out_y=None, name='crop_refine'):
    """dpp_crop_refine: the refined crop centre from a refinement net's output (+ optionally the labels of the re-cropped frame)."""
    fx, fy, ux, uy, flip = cam
    return Launch(rt.lib.dpp_crop_refine,
                  (frames.ptr, records.ptr, B, H, W, com_in.ptr, cube.ptr, net_out.ptr, float(fx), float(fy), float(ux), float(uy), int(flip),
                   _p(gt3d_orig), int(J), _p(pca_mean), _p(pca_comp), int(E), com_out.ptr, _p(com3d_out), _p(gt3d_crop), _p(out_y)),
                  (frames, records, com_in, cube, net_out, gt3d_orig, pca_mean, pca_comp, com_out, com3d_out, gt3d_crop, out_y), name)


def frame_range_workspace(rt, B):
    """The per-band (min, max) partials of B frames: what frame_range writes and crop_prepare_ranged / refine_com_iterative read."""
    return rt.alloc(max(1, int(rt.lib.dpp_frame_range_bytes(B)) // 4), np.float32, zero=False)


def frame_range(rt, frames, B, H, W, partial, name='frame_range', table=None):
    """dpp_frame_range: the depth range of every frame, many workgroups per frame -- the ONE pass over the whole frame of a tracked frame.
    table (a SourceTable): dpp_frame_range_src on the ragged buffer of the table's sources; B, H, W are not read."""
    if table is None:
        fn, args, keep, npx = rt.lib.dpp_frame_range, (frames.ptr, B, H, W, partial.ptr), (frames, partial), float(B) * H * W
    else:
        fn, args, keep, npx = rt.lib.dpp_frame_range_src, (frames.ptr, table.dev.ptr, table.C, partial.ptr), (frames, table.dev, partial), table.npx
    return Launch(fn, args, keep, name, dict(kernel='frame_range', flops=2.0 * npx, bytes=4.0 * npx))


INGEST_U16, INGEST_F32 = 1, 2                 # DPP_INGEST_*: source types of dpp_frame_ingest
INGEST_MEDIAN3, INGEST_MIRROR_X = 1, 2        # ... and its flags
INGEST_TYPES = {'uint16': INGEST_U16, 'float32': INGEST_F32}


def sensor_spec(sensor):
    """A sensor description dict(dtype='uint16' | 'float32', median=bool, mirror=bool) checked and normalised to (numpy dtype, median,
    mirror); such a tuple (a tracker hands its own to its detectors) passes through."""
    if isinstance(sensor, tuple):
        return sensor
    unknown = set(sensor) - {'dtype', 'median', 'mirror'}
    if unknown:
        raise ValueError("unknown sensor options: %s" % sorted(unknown))
    dt = np.dtype(sensor.get('dtype', 'uint16'))
    if dt.name not in INGEST_TYPES:
        raise ValueError("a sensor delivers uint16 or float32 frames, not %s" % dt.name)
    return dt, bool(sensor.get('median', False)), bool(sensor.get('mirror', False))


def frame_ingest(rt, raw, B, H, W, frames, partial, median=False, mirror=False, name='frame_ingest', table=None):
    """dpp_frame_ingest: raw sensor frames (uint16 or float32, by raw.dtype) -> float32 frames, optionally mirrored and 3x3-median
    filtered, and frame_range's partials of the result (partial may be None) -- in a plan it stands where frame_range stood.
    table (a SourceTable): dpp_frame_ingest_src on the ragged buffers of the table's sources; B, H, W are not read."""
    if raw.dtype.name not in INGEST_TYPES:
        raise ValueError("frame_ingest reads uint16 or float32 frames, not %s" % raw.dtype.name)
    flags = (INGEST_MEDIAN3 if median else 0) | (INGEST_MIRROR_X if mirror else 0)
    head, tail = (raw.ptr, INGEST_TYPES[raw.dtype.name]), (flags, frames.ptr, _p(partial))
    if table is None:
        fn, args, keep, npx = rt.lib.dpp_frame_ingest, head + (B, H, W) + tail, (raw, frames, partial), float(B) * H * W
    else:
        fn, args, keep, npx = rt.lib.dpp_frame_ingest_src, head + (table.dev.ptr, table.C) + tail, (raw, table.dev, frames, partial), table.npx
    # a median output takes 8 compare-exchanges' worth of its columns' sorts (shared by three outputs) + 12 of its own; min / max: 2
    return Launch(fn, args, keep, name, dict(kernel='frame_ingest', flops=(22.0 if median else 2.0) * npx, bytes=(raw.dtype.itemsize + 4.0) * npx))


# ---- a learned static background removed from the frame (include/dpp_hip.h, ABI v25; csrc/background.hip) -------------------------------
def background_spec(background):
    """dict(margin=, rel=0.0, min_seen=1[, adapt=dict(persist=, guard=, every=1)]) checked on the host -> (margin, rel, min_seen); such
    a tuple (a tracker hands its own to its detectors, which never adapt) passes through.  margin (mm, finite, >= 0) is required: none
    has been chosen for a sensor.  0 <= rel < 1; min_seen an int >= 1.  adapt is checked here and read by background_adapt_spec."""
    if isinstance(background, tuple):
        return background
    known = ('margin', 'rel', 'min_seen', 'adapt')
    if not isinstance(background, dict) or set(background) - set(known):
        raise ValueError("background takes margin, rel, min_seen and adapt, not %r" %
                         (sorted(set(background) - set(known)) if isinstance(background, dict) else background,))
    s = dict(rel=0.0, min_seen=1)
    s.update(background)
    if 'margin' not in s:
        raise ValueError("background needs margin (mm): no default has been chosen for a sensor")
    try:
        margin, rel, seen = float(s['margin']), float(s['rel']), int(s['min_seen'])
    except (TypeError, ValueError):
        raise ValueError("background takes numbers: %r" % (background,))
    if not (np.isfinite(margin) and margin >= 0.):
        raise ValueError("margin (mm) is finite and >= 0: %r" % (s['margin'],))
    if not 0. <= rel < 1.:
        raise ValueError("rel is a share of the depth, 0 <= rel < 1: %r" % (s['rel'],))
    if seen != s['min_seen'] or not 1 <= seen < 2 ** 31:
        raise ValueError("min_seen is a number of frames >= 1: %r" % (s['min_seen'],))
    _adapt_spec(s.get('adapt'), seen)
    return margin, rel, seen


def _adapt_spec(adapt, min_seen):
    if adapt is None:
        return None
    known = ('persist', 'guard', 'every')
    if not isinstance(adapt, dict) or set(adapt) - set(known):
        raise ValueError("adapt takes persist, guard and every, not %r" % (sorted(set(adapt) - set(known)) if isinstance(adapt, dict) else adapt,))
    a = dict(every=1)
    a.update(adapt)
    for k in ('persist', 'guard'):
        if k not in a:
            raise ValueError("adapt needs %s: no default has been chosen for a sensor" % k)
    out = []
    for k, low in (('persist', max(2, min_seen)), ('guard', 0), ('every', 1)):
        try:
            v = int(a[k])
        except (TypeError, ValueError):
            raise ValueError("adapt takes integers: %s = %r" % (k, a[k]))
        if isinstance(a[k], bool) or v != a[k] or not low <= v < 2 ** 31:
            raise ValueError("adapt's %s is an integer >= %d%s: %r" % (k, low, " (max(2, min_seen))" if k == 'persist' else "", a[k]))
        out.append(v)
    return tuple(out)


def background_adapt_spec(background):
    """None, or (persist, guard, every) of background=dict(..., adapt=dict(persist=, guard=, every=1)): the model is kept current while
    tracking.  persist (adapting ticks until a depth that stays becomes the background, an int >= max(2, min_seen)) and guard (pixels
    around a track's crop window that are kept out, an int >= 0) have no default; every (ticks, an int >= 1): the tracker adapts in
    the ticks whose number is a multiple of it.  A tuple (background_spec's own result) has no adapt."""
    if isinstance(background, tuple):
        return None
    min_seen = background_spec(background)[2]              # first: whatever is no dict of the known keys is its ValueError
    return _adapt_spec(background.get('adapt'), min_seen)


def background_cut(near, seen, spec):
    """The cut map of a model on the host, every operation rounded to float32: near - (margin + rel * near) where seen >= min_seen,
    near != 0 and the result is > 0; +inf elsewhere (no background is known there: every depth is foreground)."""
    margin, rel, min_seen = spec
    near = np.asarray(near, np.float32)
    cut = near - (np.float32(margin) + np.float32(rel) * near)
    known = (np.asarray(seen) >= min_seen) & (near != 0) & (cut > 0)
    return np.where(known, cut, np.float32(np.inf)).astype(np.float32)


def frame_background(rt, frames, cut, B, H, W, partial, name='frame_background', table=None):
    """dpp_frame_background: frames = (f != 0 and f < cut) ? f : 0 IN PLACE, and frame_range's partials of the result (partial may be
    None) -- in a plan it stands where frame_range stood.  table (a SourceTable): dpp_frame_background_src on the ragged buffers of the
    table's sources (cut has the frames' layout); B, H, W are not read."""
    if table is None:
        fn, args, keep, npx = rt.lib.dpp_frame_background, (frames.ptr, cut.ptr, B, H, W, _p(partial)), (frames, cut, partial), float(B) * H * W
    else:
        fn, args, npx = rt.lib.dpp_frame_background_src, (frames.ptr, cut.ptr, table.dev.ptr, table.C, _p(partial)), table.npx
        keep = (frames, cut, table.dev, partial)
    # per pixel: the frame read and written, the cut read; two compares and a select, min / max
    return Launch(fn, args, keep, name, dict(kernel='frame_background', flops=4.0 * npx, bytes=3 * 4.0 * npx))


def frame_background_adapt(rt, frames, bg, take, B, H, W, records, T, src, partial, name='frame_background_adapt', table=None):
    """dpp_frame_background_adapt: frame_background on `frames` with bg's cut map as it stands, and in the same pass bg (a
    BackgroundModel with adapt=) adapted from the raw depths of the sources with take[c] != 0 (tests/background_adapt_ref.py):
    near / seen confirmed, cand / run counted, the model replaced at persist, the cut map rewritten where the model changed.
    records: the crop records of T tracks as track_refine left them (their windows, dilated by guard, are kept out), src [T] int32
    their sources (None: track t reads frame t); records None: nothing is kept out."""
    margin, rel, min_seen = bg.spec
    persist, guard, _ = bg.adapt
    head = (frames.ptr, bg.cut.ptr, bg.near.ptr, bg.seen.ptr, bg.cand.ptr, bg.run.ptr, take.ptr)
    tail = (_p(records), int(T) if records is not None else 0, _p(src), margin, rel, min_seen, persist, guard, _p(partial))
    keep = (frames, bg.cut, bg.near, bg.seen, bg.cand, bg.run, take, records, src, partial)
    if table is None:
        fn, args, npx = rt.lib.dpp_frame_background_adapt, head + (B, H, W) + tail, float(B) * H * W
    else:
        fn, args, npx, keep = rt.lib.dpp_frame_background_adapt_src, head + (table.dev.ptr, table.C) + tail, table.npx, keep + (table.dev,)
    # per pixel at the most: six arrays read and written; the cut's compares, two bands and a cut map's three operations, min / max
    return Launch(fn, args, keep, name, dict(kernel='frame_background_adapt', flops=16.0 * npx, bytes=12 * 4.0 * npx))


def background_learn(rt, frames, take, B, H, W, near, seen, name='background_learn', table=None):
    """dpp_background_learn: one float32 frame per source into the model (near: the smallest non-zero depth; seen: the frames with a
    depth); take (int32 per source): 0 leaves that source's model untouched.  table: dpp_background_learn_src, as frame_background."""
    if table is None:
        fn, args, npx = rt.lib.dpp_background_learn, (frames.ptr, take.ptr, B, H, W, near.ptr, seen.ptr), float(B) * H * W
        keep = (frames, take, near, seen)
    else:
        fn, args, npx = rt.lib.dpp_background_learn_src, (frames.ptr, take.ptr, table.dev.ptr, table.C, near.ptr, seen.ptr), table.npx
        keep = (frames, take, table.dev, near, seen)
    return Launch(fn, args, keep, name, dict(kernel='background_learn', flops=3.0 * npx, bytes=5 * 4.0 * npx))


class BackgroundModel(object):
    """The background model of C frame sources and what is derived from it, in the layout of the frames they are applied to ((C, H, W),
    or with a SourceTable the ragged one): `near` (float32), `seen` (int32), `cut` (float32, what frame_background reads; +inf until
    refresh() after something was learned or set) and `take` (int32 [C], background_learn's per-source switch).  The model lives on
    the device; refresh() downloads it, computes the cut map on the host (background_cut) and uploads it: once per model change, never
    per tick.  With spec's adapt= (background_adapt_spec) the model is also kept current by the plan's own cut launch
    (frame_background_adapt), which rewrites the cut map on the device; `cand` (float32) and `run` (int32) are its candidate state in
    the same layout (None without adapt), zeroed by set / clear / forget for the sources they touch."""

    def __init__(self, rt, spec, C, H=None, W=None, table=None):
        self.rt, self.spec, self.C, self.table = rt, background_spec(spec), int(C), table
        self.adapt = background_adapt_spec(spec)
        if table is None:
            self.sizes, self.offs, n = [(int(H), int(W))] * self.C, [c * int(H) * int(W) for c in range(self.C)], self.C * int(H) * int(W)
        else:
            self.sizes, self.offs, n = [table.size(c) for c in range(self.C)], [int(o) for o in table.host['frame_off']], table.frame_elems
        self.near, self.seen = rt.alloc((n,), np.float32), rt.alloc((n,), np.int32)
        self.cut = rt.upload(np.full(n, np.inf, np.float32))
        self.take_host = np.ones(self.C, np.int32)
        self.take = rt.upload(self.take_host)
        self.cand = self.run = None
        if self.adapt is not None:
            self.cand, self.run = rt.alloc((n,), np.float32), rt.alloc((n,), np.int32)

    def forget_candidates(self, c=None):
        """Zero cand / run (of source c, or of all): what was counted belongs to a model that was set, cleared or learned since."""
        if self.adapt is not None:
            for s in self._sources(c):
                H, W = self.sizes[s]
                self.view(self.cand, s).set(np.zeros((H, W), np.float32))
                self.view(self.run, s).set(np.zeros((H, W), np.int32))

    def view(self, buf, c):
        """Source c's (1, H, W) part of one of the model's buffers."""
        H, W = self.sizes[c]
        return buf.view(self.offs[c], (1, H, W))

    def set_take(self, take):
        take = np.asarray(take, np.int32).reshape(self.C)
        if not np.array_equal(take, self.take_host):
            self.take.set(take)
            self.take_host = take.copy()

    def _sources(self, c):
        if c is None:
            return list(range(self.C))
        if not 0 <= int(c) < self.C:
            raise IndexError("source %r of %d" % (c, self.C))
        return [int(c)]

    def refresh(self, c=None):
        """Recompute and upload the cut map (of source c alone, or of every source)."""
        for s in self._sources(c):
            cut = background_cut(self.view(self.near, s).get(), self.view(self.seen, s).get(), self.spec)
            self.view(self.cut, s).set(cut)

    def clear(self, c=None):
        """Forget what was learned (for source c, or for all): the cut map is +inf again, the tracker that of one without the option."""
        for s in self._sources(c):
            H, W = self.sizes[s]
            self.view(self.near, s).set(np.zeros((H, W), np.float32))
            self.view(self.seen, s).set(np.zeros((H, W), np.int32))
            self.view(self.cut, s).set(np.full((H, W), np.inf, np.float32))
        self.forget_candidates(c)

    def get(self, c):
        """dict(near, seen, cut) of source c, (H, W) each, downloaded."""
        (s,) = self._sources(int(c))
        return dict(near=self.view(self.near, s).get()[0], seen=self.view(self.seen, s).get()[0], cut=self.view(self.cut, s).get()[0])

    def set(self, c, near, seen):
        """Load a model learned earlier into source c and refresh its cut map."""
        (s,) = self._sources(int(c))
        near, seen = np.asarray(near), np.asarray(seen)
        if near.shape != self.sizes[s] or seen.shape != self.sizes[s]:
            raise ValueError("background model shapes %s / %s, source %d delivers %s" % (near.shape, seen.shape, s, self.sizes[s]))
        if not np.issubdtype(seen.dtype, np.integer) or (seen < 0).any() or not np.all(np.isfinite(near)) or (near < 0).any():
            raise ValueError("near holds finite depths >= 0 (0: none seen), seen counts of frames")
        self.view(self.near, s).set(near.astype(np.float32))
        self.view(self.seen, s).set(seen.astype(np.int32))
        self.refresh(s)
        self.forget_candidates(s)


def crop_prepare_ranged(rt, partial, B, com, cube, fx, fy, dsz, records, M_out=None, stretch=False, name='crop_prepare_ranged', tracks=None):
    """dpp_crop_prepare_ranged: crop_prepare's records from frame_range's partials (no pass over the frame)."""
    tail = (dsz, int(bool(stretch)), records.ptr, _p(M_out))
    if tracks is None:
        fn, args, keep = rt.lib.dpp_crop_prepare_ranged, (partial.ptr, B, com.ptr, cube.ptr, float(fx), float(fy)) + tail, (partial,)
    elif tracks.table is None:
        fn, keep = rt.lib.dpp_crop_prepare_ranged_ix, (partial, tracks.src, tracks.gate)
        args = (partial.ptr, tracks.T, tracks.src.ptr, tracks.gate.ptr, com.ptr, cube.ptr, float(fx), float(fy)) + tail
    else:
        fn, keep = rt.lib.dpp_crop_prepare_ranged_src, (partial, tracks.src, tracks.gate, tracks.table.dev)
        args = (partial.ptr, tracks.T, tracks.src.ptr, tracks.gate.ptr, tracks.table.dev.ptr, com.ptr, cube.ptr) + tail
    return Launch(fn, args, keep + (com, cube, records, M_out), name)


def track_refine(rt, frames, records_in, B, H, W, com_in, cube, net_out, cam, crop_fx, crop_fy, dsz, com_out, com3d_out, records_out, status,
                 M_out=None, name='track_refine', tracks=None):
    """dpp_track_refine: the tracked centre from the refinement net's output, fused with the prepare of the final crop around it."""
    nets, tail = (com_in.ptr, cube.ptr, net_out.ptr), (dsz, com_out.ptr, com3d_out.ptr, records_out.ptr, _p(M_out), status.ptr)
    if tracks is None or tracks.table is None:
        fx, fy, ux, uy, flip = cam
        cams = (float(fx), float(fy), float(ux), float(uy), int(flip), float(crop_fx), float(crop_fy))
    if tracks is None:
        fn, args, keep = rt.lib.dpp_track_refine, (frames.ptr, records_in.ptr, B, H, W) + nets + cams + tail, (frames, records_in)
    elif tracks.table is None:
        fn, keep = rt.lib.dpp_track_refine_ix, (frames, records_in, tracks.src, tracks.gate)
        args = (frames.ptr, records_in.ptr, tracks.T, tracks.src.ptr, tracks.gate.ptr, H, W) + nets + cams + tail
    else:
        fn, keep = rt.lib.dpp_track_refine_src, (frames, records_in, tracks.src, tracks.gate, tracks.table.dev)
        args = (frames.ptr, records_in.ptr, tracks.T, tracks.src.ptr, tracks.gate.ptr, tracks.table.dev.ptr) + nets + tail
    return Launch(fn, args, keep + (com_in, cube, net_out, com_out, com3d_out, records_out, M_out, status), name)


POSE_HAND_RIGHT, POSE_INV_X, POSE_INV_Y = 1, 2, 4      # dpp_pose_finish flags


def pose_finish(rt, net_out, B, J, cube, com3d, cam, flags, pose3d, pose_img, name='pose_finish', tracks=None):
    """dpp_pose_finish: estimatePose's sign rules, pose * cube_z / 2 + com3D and joints3DToImg of the result.  With tracks the sign
    rules come per track from tflags[t] and `flags` is not read."""
    if tracks is None or tracks.table is None:
        fx, fy, ux, uy, flip = cam
        cams = (float(fx), float(fy), float(ux), float(uy), int(flip))
    if tracks is None:
        fn, args, keep = rt.lib.dpp_pose_finish, (net_out.ptr, B, J, cube.ptr, com3d.ptr) + cams + (int(flags), pose3d.ptr, pose_img.ptr), (net_out,)
    elif tracks.table is None:
        fn, keep = rt.lib.dpp_pose_finish_ix, (net_out, tracks.tflags)
        args = (net_out.ptr, tracks.T, J, tracks.tflags.ptr, cube.ptr, com3d.ptr) + cams + (pose3d.ptr, pose_img.ptr)
    else:
        fn, keep = rt.lib.dpp_pose_finish_src, (net_out, tracks.src, tracks.tflags, tracks.table.dev)
        args = (net_out.ptr, tracks.T, J, tracks.src.ptr, tracks.tflags.ptr, tracks.table.dev.ptr, cube.ptr, com3d.ptr, pose3d.ptr, pose_img.ptr)
    return Launch(fn, args, keep + (cube, com3d, pose3d, pose_img), name)


TRACK_OK, TRACK_LOST, TRACK_IDLE = 0, 1, 2           # DPP_TRACK_*: dpp_track_refine's status word


def track_index(src, C):
    """The host's check of a `src` array (the kernels trust it): int32, every entry a frame of [0, C)."""
    src = np.ascontiguousarray(src, np.int32).reshape(-1)
    if src.size < 1 or src.min() < 0 or src.max() >= int(C):
        raise ValueError("every track reads one of the %d frame sources: %r" % (C, src.tolist()))
    return src


class TrackSet(object):
    """What a tracking launch knows about its rows (include/dpp_hip.h, ABI v16 / v19): T tracks; `src`, `gate`, `tflags`, int32 device
    arrays with one entry per track (frame source, takes part in this tick, POSE_* flags; the caller has checked `src` with track_index
    before uploading it -- a launch reads the ones its C entry point takes, a caller of single launches may leave the others out); `table`,
    the SourceTable of sources with cameras and frame sizes of their own, or None: one camera and one size, given as launch arguments."""
    __slots__ = ('T', 'src', 'gate', 'tflags', 'table')

    def __init__(self, T, src=None, gate=None, tflags=None, table=None):
        arrays = [a for a in (src, gate, tflags) if a is not None]
        if T < 1 or not arrays or any(a.size != T for a in arrays) or (table is not None and src is None):
            raise ValueError("a TrackSet has T >= 1 tracks and int32 device arrays of T entries (with a table: src among them)")
        self.T, self.src, self.gate, self.tflags, self.table = int(T), src, gate, tflags, table


# ---- frame sources of unlike cameras and frame sizes (include/dpp_hip.h, ABI v19) -------------------------------------------------------
# One record per source; the ragged frame buffers hold source c's H x W elements from its offset on, every offset padded to 16 bytes.
SOURCE_RECORD = np.dtype([('fx', np.float64), ('fy', np.float64), ('ux', np.float64), ('uy', np.float64), ('crop_fx', np.float64),
                          ('crop_fy', np.float64), ('frame_off', np.int64), ('raw_off', np.int64), ('H', np.int32), ('W', np.int32),
                          ('flip_y', np.int32), ('pad', np.int32)])


class SourceTable(object):
    """The per-source table of the *_src launches: `host` (a SOURCE_RECORD array, validated here -- the kernels trust it), `dev` (its
    device copy), and the element counts of the ragged float32 frame buffer and of the raw sensor buffer that hold its frames."""

    def __init__(self, rt, cams, crop_f, sizes, raw_itemsize=None):
        """cams: C (fx, fy, ux, uy, flip_y); crop_f: C (crop_fx, crop_fy); sizes: C (H, W); raw_itemsize: bytes per element of the raw
        sensor buffer (None: there is none, its offsets repeat the frame buffer's)."""
        assert SOURCE_RECORD.itemsize == rt.lib.dpp_source_record_bytes(), (SOURCE_RECORD.itemsize, rt.lib.dpp_source_record_bytes())
        C = len(sizes)
        if C < 1 or len(cams) != C or len(crop_f) != C:
            raise ValueError("one camera, one (fx, fy) and one (H, W) per source: %d, %d, %d" % (len(cams), len(crop_f), C))
        tab = np.zeros(C, SOURCE_RECORD)
        pad_f, pad_r = 4, 16 // int(raw_itemsize or 4)                 # elements per 16 bytes
        off_f = off_r = 0
        for c in range(C):
            (fx, fy, ux, uy, flip), (cfx, cfy), (H, W) = cams[c], crop_f[c], sizes[c]
            if int(H) != H or int(W) != W or H < 1 or W < 1:
                raise ValueError("source %d: frame size %r x %r" % (c, H, W))
            vals = [float(v) for v in (fx, fy, ux, uy, cfx, cfy)]
            if not all(np.isfinite(vals)) or vals[0] == 0. or vals[1] == 0. or vals[4] == 0. or vals[5] == 0.:
                raise ValueError("source %d: a camera needs finite values and focal lengths other than zero: %r" % (c, vals))
            tab[c] = (vals[0], vals[1], vals[2], vals[3], abs(vals[4]), abs(vals[5]), off_f, off_r, int(H), int(W), int(bool(flip)), 0)
            off_f += -(-int(H) * int(W) // pad_f) * pad_f
            off_r += -(-int(H) * int(W) // pad_r) * pad_r
        self.host, self.C, self.frame_elems, self.raw_elems, self.raw_pad = tab, C, off_f, off_r, pad_r
        self.check()
        self.npx = float(sum(int(r['H']) * int(r['W']) for r in tab))     # the sources' real sizes: what the launches' meta sums over
        self.dev = rt.upload(tab.view(np.uint8))

    def check(self):
        """Offsets in range and 16-byte aligned, sizes positive, focal lengths not zero -- once, on the host."""
        t = self.host
        for c in range(self.C):
            px = int(t['H'][c]) * int(t['W'][c])
            ok = (t['H'][c] > 0 and t['W'][c] > 0 and t['frame_off'][c] >= 0 and t['raw_off'][c] >= 0 and
                  t['frame_off'][c] + px <= self.frame_elems and t['raw_off'][c] + px <= self.raw_elems and
                  t['frame_off'][c] % 4 == 0 and t['raw_off'][c] % self.raw_pad == 0 and
                  all(t[k][c] != 0. for k in ('fx', 'fy', 'crop_fx', 'crop_fy')))
            if not ok:
                raise ValueError("source record %d is not valid: %r" % (c, t[c]))

    def size(self, c):
        return int(self.host['H'][c]), int(self.host['W'][c])


# ---- tracks of one hand across calibrated cameras (include/dpp_hip.h, ABI v20; csrc/fuse.hip) ------------------------------------------
FUSE_USED, FUSE_OUTLIER, FUSE_DISAGREE, FUSE_PEER_OK, FUSE_HANDED = 1, 2, 4, 8, 16     # DPP_FUSE_*: dpp_pose_fuse's per-track word
FUSE_HANDOVER = 1                                                                      # ... and its launch flag
FUSE_MAX_MEMBERS = 16


class FuseRig(object):
    """What dpp_pose_fuse reads about the rig, validated here (the kernel trusts it) and uploaded ONCE: `extr` (float64 [C][12]: R
    row-major, then t in mm, per source: w = R p + t takes the source's camera frame to the world), `members` / `offsets` (int32: group
    g is the tracks members[offsets[g]:offsets[g + 1]] in list order) and, on the host, `groups` and `group_of` (track -> group or -1).

    anchor (a source, or None): entries of `extrinsics` may then be None -- those sources are `pending`, to be calibrated against the
    anchor (dpp_extrinsics_accumulate, hipdp/calib.py) and written later through set_extrinsics.  Their rows hold the identity until
    then.  The anchor's own entry must be given, and every pending source must share a group with the anchor source."""

    def __init__(self, rt, extrinsics, groups, src, C, anchor=None):
        src = np.asarray(src, np.int32).reshape(-1)
        T = src.size
        if extrinsics is None or len(extrinsics) != C:
            raise ValueError("one (R, t) per source: %s for %d sources" % ('none' if extrinsics is None else len(extrinsics), C))
        if anchor is not None and (int(anchor) != anchor or not 0 <= anchor < C or extrinsics[int(anchor)] is None):
            raise ValueError("the anchor is a source whose (R, t) is given: %r of %d sources" % (anchor, C))
        ext = np.zeros((C, 12), np.float64)
        self.pending = []
        for c, e in enumerate(extrinsics):
            if e is None:
                if anchor is None:
                    raise ValueError("source %d has no (R, t): every source needs one (or calibrate= names an anchor to find it from)" % c)
                self.pending.append(c)
                e = (np.eye(3), np.zeros(3))
            ext[c] = self._row(c, *e)
        groups = [[int(m) for m in g] for g in groups]
        group_of = np.full(T, -1, np.int32)
        if not groups:
            raise ValueError("groups needs at least one group")
        for g, ms in enumerate(groups):
            if not 1 <= len(ms) <= FUSE_MAX_MEMBERS:
                raise ValueError("group %d has %d members: 1 .. %d" % (g, len(ms), FUSE_MAX_MEMBERS))
            if any(not 0 <= m < T for m in ms):
                raise ValueError("group %d names a track outside 0 .. %d: %r" % (g, T - 1, ms))
            if any(group_of[m] >= 0 for m in ms) or len(set(ms)) != len(ms):
                raise ValueError("groups are disjoint: group %d repeats a track: %r" % (g, ms))
            if len(set(int(src[m]) for m in ms)) != len(ms):
                raise ValueError("the members of group %d read pairwise distinct sources: %r" % (g, [int(src[m]) for m in ms]))
            group_of[ms] = g
        self.anchor = None if anchor is None else int(anchor)
        for c in self.pending:
            if not any(set((self.anchor, c)) <= set(int(src[m]) for m in ms) for ms in groups):
                raise ValueError("source %d shares no group with the anchor source %d: it cannot be calibrated against it (chained "
                                 "calibration through a third camera is out of scope)" % (c, self.anchor))
        if len(self.pending) > CALIB_MAX_SOURCES:
            raise ValueError("%d sources to calibrate at once: at most %d" % (len(self.pending), CALIB_MAX_SOURCES))
        self.G, self.C, self.T, self.groups, self.group_of, self.extr_host = len(groups), int(C), T, groups, group_of, ext
        self.members_host = np.int32([m for ms in groups for m in ms])
        self.offsets_host = np.int32(np.concatenate([[0], np.cumsum([len(ms) for ms in groups])]))
        self.extr, self.members, self.offsets = rt.upload(ext), rt.upload(self.members_host), rt.upload(self.offsets_host)

    @staticmethod
    def _row(c, Rm, t):
        """Source c's row of `extr` from (R, t), or ValueError."""
        Rm, t = np.asarray(Rm, np.float64), np.asarray(t, np.float64).reshape(-1)
        if Rm.shape != (3, 3) or t.shape != (3,) or not np.isfinite(Rm).all() or not np.isfinite(t).all():
            raise ValueError("source %d: R is a finite 3 x 3 rotation, t a finite 3-vector (mm)" % c)
        if np.abs(Rm.T.dot(Rm) - np.eye(3)).max() > 1e-6 or not np.linalg.det(Rm) > 0.:
            raise ValueError("source %d: R is not a rotation (max |R^T R - I| <= 1e-6 and det R > 0): %r" % (c, Rm))
        return np.concatenate([Rm.ravel(), t])

    def set_extrinsics(self, c, Rm, t):
        """Write source c's (R, t), validated as the constructor validates: one upload of its 96 bytes.  A pending source stops being
        pending."""
        c = int(c)
        if not 0 <= c < self.C:
            raise IndexError("source %d of %d" % (c, self.C))
        row = self._row(c, Rm, t)
        self.extr_host[c] = row
        self.extr.view(12 * c, (12,)).set(row)
        if c in self.pending:
            self.pending.remove(c)


# ---- extrinsics from the tracked hand (include/dpp_hip.h, ABI v21; csrc/calib.hip) -------------------------------------------------------
CALIB_MAX_SOURCES, CALIB_SLOTS = 32, 20                                                # DPP_CALIB_*


def extrinsics_accumulate(rt, pose3d, status, src, T, J, rig, anchor, cal_src, max_shape_dev, acc, name='extrinsics_accumulate'):
    """dpp_extrinsics_accumulate: one workgroup per source of `cal_src` (host ints), summing its joint pairs with the anchor source's into
    acc [len(cal_src)][CALIB_SLOTS] float64.  max_shape_dev: None (no shape gate) or > 0 (mm)."""
    if max_shape_dev is not None and not (np.isfinite(max_shape_dev) and max_shape_dev > 0.):
        raise ValueError("max_shape_dev is None or a distance > 0 (mm): %r" % (max_shape_dev,))
    cal = [int(c) for c in cal_src]
    if not 1 <= len(cal) <= CALIB_MAX_SOURCES or int(anchor) in cal or any(not 0 <= c < rig.C for c in cal + [int(anchor)]):
        raise ValueError("cal_src names 1 .. %d sources of %d other than the anchor %r: %r" % (CALIB_MAX_SOURCES, rig.C, anchor, cal))
    if acc.size != len(cal) * CALIB_SLOTS or acc.dtype != np.float64:
        raise ValueError("acc is float64 [%d][%d]" % (len(cal), CALIB_SLOTS))
    host = (C.c_int * len(cal))(*cal)                                                  # read once per call of the entry point: kept alive
    return Launch(rt.lib.dpp_extrinsics_accumulate,
                  (pose3d.ptr, status.ptr, src.ptr, T, J, rig.extr.ptr, rig.C, rig.members.ptr, rig.offsets.ptr, rig.G, int(anchor),
                   host, len(cal), 0.0 if max_shape_dev is None else float(max_shape_dev), acc.ptr),
                  (pose3d, status, src, rig.extr, rig.members, rig.offsets, acc, host), name)


def pose_fuse(rt, pose3d, com3d, status, src, T, J, rig, table, H, W, cam, max_dev, handover, com, fused_pose, fused_com, spread, n_out,
              peer_com, fstat, name='pose_fuse', weight=None, fused_weight=None):
    """dpp_pose_fuse: one workgroup per group of `rig`.  table: an ops.SourceTable, or None with (H, W, cam) for every source; max_dev:
    None (no consistency test) or > 0 (mm).  weight [T][J] with fused_weight [G][J] (both or neither): dpp_pose_fuse_w, the joints
    averaged with joint_visibility's weights."""
    if max_dev is not None and not (np.isfinite(max_dev) and max_dev > 0.):
        raise ValueError("max_dev is None or a distance > 0 (mm): %r" % (max_dev,))
    if (weight is None) != (fused_weight is None):
        raise ValueError("weight [T][J] and fused_weight [G][J] go together")
    fx, fy, ux, uy, flip = (0., 0., 0., 0., 0) if table is not None else cam
    weighted = () if weight is None else (weight, fused_weight)
    return Launch(rt.lib.dpp_pose_fuse if weight is None else rt.lib.dpp_pose_fuse_w,
                  (pose3d.ptr, com3d.ptr, status.ptr, src.ptr, T, J, rig.extr.ptr, rig.C, rig.members.ptr, rig.offsets.ptr, rig.G,
                   None if table is None else table.dev.ptr, 0 if table is not None else int(H), 0 if table is not None else int(W), float(fx),
                   float(fy), float(ux), float(uy), int(flip), 0.0 if max_dev is None else float(max_dev), FUSE_HANDOVER if handover else 0,
                   com.ptr, fused_pose.ptr, fused_com.ptr, spread.ptr, n_out.ptr, peer_com.ptr, fstat.ptr) + tuple(b.ptr for b in weighted),
                  (pose3d, com3d, status, src, rig.extr, rig.members, rig.offsets, None if table is None else table.dev, com, fused_pose,
                   fused_com, spread, n_out, peer_com, fstat) + weighted, name)


# ---- which joints of a tracked pose the frame shows (include/dpp_hip.h, ABI v23; csrc/visibility.hip) ------------------------------------
VIS_VISIBLE, VIS_OCCLUDED, VIS_UNSUPPORTED, VIS_OFFFRAME = 1, 2, 4, 8                   # DPP_VIS_*: dpp_joint_visibility's class per joint
VIS_MAX_RADIUS = 8


def visibility_spec(visibility):
    """dict(radius=, margin=, min_support=, hidden_weight=0.0) checked on the host -> (radius, margin, min_support, hidden_weight).
    radius (pixels, 0 .. 8), margin (mm) and min_support (pixels of the window, 1 .. (2 radius + 1)^2) are required: none has been
    chosen for a dataset.  hidden_weight: what a joint that is not VISIBLE weighs in the fusion, in [0, 1]."""
    s = dict(hidden_weight=0.0)
    known = ('radius', 'margin', 'min_support', 'hidden_weight')
    if not isinstance(visibility, dict) or set(visibility) - set(known):
        raise ValueError("visibility takes radius, margin, min_support and hidden_weight, not %r" %
                         (sorted(set(visibility) - set(known)) if isinstance(visibility, dict) else visibility,))
    s.update(visibility)
    missing = [k for k in known if k not in s]
    if missing:
        raise ValueError("visibility needs %s: no tuned default exists" % ', '.join(missing))
    try:
        radius, support = int(s['radius']), int(s['min_support'])
        margin, hidden = float(s['margin']), float(s['hidden_weight'])
    except (TypeError, ValueError, OverflowError):
        raise ValueError("visibility takes numbers: %r" % (visibility,))
    if radius != s['radius'] or not 0 <= radius <= VIS_MAX_RADIUS:
        raise ValueError("radius is a number of pixels, 0 .. %d: %r" % (VIS_MAX_RADIUS, s['radius']))
    if support != s['min_support'] or not 1 <= support <= (2 * radius + 1) ** 2:
        raise ValueError("min_support is a number of the window's %d pixels, 1 or more: %r" % ((2 * radius + 1) ** 2, s['min_support']))
    if not (np.isfinite(margin) and margin > 0.):
        raise ValueError("margin (mm) is finite and > 0: %r" % (s['margin'],))
    if not 0. <= hidden <= 1.:
        raise ValueError("hidden_weight is a weight in [0, 1]: %r" % (s['hidden_weight'],))
    return radius, margin, support, hidden


def joint_visibility(rt, pose_img, status, src, T, J, frames, C, spec, vis, weight, vword, table=None, H=0, W=0, name='joint_visibility'):
    """dpp_joint_visibility: one workgroup per (track, joint).  spec: visibility_spec's tuple.  frames: the float32 frame buffer --
    [C][H][W] with H, W, or the ragged one of `table` (an ops.SourceTable); src: int32 [T], every track's source."""
    radius, margin, support, hidden = spec
    return Launch(rt.lib.dpp_joint_visibility,
                  (pose_img.ptr, status.ptr, src.ptr, T, J, frames.ptr, int(C), None if table is None else table.dev.ptr,
                   0 if table is not None else int(H), 0 if table is not None else int(W), radius, margin, support, hidden, vis.ptr, weight.ptr,
                   vword.ptr),
                  (pose_img, status, src, frames, None if table is None else table.dev, vis, weight, vword), name)


# ---- tracked and fused poses smoothed over the ticks (include/dpp_hip.h, ABI v22; csrc/smooth.hip) --------------------------------------
SMOOTH_OK, SMOOTH_INIT, SMOOTH_HELD, SMOOTH_EMPTY, SMOOTH_DROPPED = 1, 2, 4, 8, 16     # DPP_SMOOTH_*: dpp_pose_smooth's per-row word


def smooth_spec(smooth):
    """dict(rate=, mincutoff=, beta=, dcutoff=1.0, max_hold=0) checked on the host -> (rate, mincutoff, beta, dcutoff, max_hold).  rate
    (ticks per second), mincutoff (Hz) and beta (Hz per mm / s) are required: there is no tuned default.  dcutoff: the paper's 1 Hz."""
    s = dict(dcutoff=1.0, max_hold=0)
    known = ('rate', 'mincutoff', 'beta', 'dcutoff', 'max_hold')
    if not isinstance(smooth, dict) or set(smooth) - set(known):
        raise ValueError("smooth takes rate, mincutoff, beta, dcutoff and max_hold, not %r" %
                         (sorted(set(smooth) - set(known)) if isinstance(smooth, dict) else smooth,))
    s.update(smooth)
    missing = [k for k in known if k not in s]
    if missing:
        raise ValueError("smooth needs %s: no tuned default exists" % ', '.join(missing))
    try:
        vals = [float(s[k]) for k in known[:4]]
        hold = int(s['max_hold'])
    except (TypeError, ValueError):
        raise ValueError("smooth takes numbers: %r" % (smooth,))
    if any(not (np.isfinite(v) and v > 0.) for v in (vals[0], vals[1], vals[3])):
        raise ValueError("rate (ticks / s), mincutoff and dcutoff (Hz) are finite and > 0: %r" % (smooth,))
    if not (np.isfinite(vals[2]) and vals[2] >= 0.):
        raise ValueError("beta (Hz per mm / s) is finite and >= 0: %r" % (smooth,))
    if hold != s['max_hold'] or not 0 <= hold < 2 ** 31:
        raise ValueError("max_hold is a number of ticks >= 0: %r" % (s['max_hold'],))
    return tuple(vals) + (hold,)


class SmoothState(object):
    """dpp_pose_smooth's device state over R = T + G rows of J joints, allocated apart from anything the host downloads: `since` (int32
    [R], -1: the row is empty), `xh` and `dxh` (float64 [R][J][3]; unread while since < 0).  clear(r): one 4-byte upload.  timed: the
    state of dpp_pose_smooth_t, which adds `tlast` (float64 [R], the row's last sample time; unread while since < 0) as a buffer of its
    own -- without it the state allocates what it always did."""

    def __init__(self, rt, R, J, timed=False):
        self.R, self.J = int(R), int(J)
        self.since = rt.upload(np.full(self.R, -1, np.int32))
        self.xh, self.dxh = rt.alloc((self.R, self.J, 3), np.float64), rt.alloc((self.R, self.J, 3), np.float64)
        self.tlast = rt.alloc((self.R,), np.float64) if timed else None
        self._empty = np.full(1, -1, np.int32)

    def clear(self, r):
        self.since.view(int(r), (1,)).set(self._empty)


def pose_smooth(rt, pose3d, status, T, J, spec, state, pose_f, pose_img_f, sstat, cam=None, src=None, table=None, fused_pose=None, n=None,
                G=0, fused_pose_f=None, gstat=None, stamps=None, C=None, name=None):
    """dpp_pose_smooth: one workgroup per row of `state` -- T tracks, then G groups (G = 0: no group rows, the four group buffers go
    unread).  spec: smooth_spec's tuple.  table: an ops.SourceTable with `src`, or None with `cam` for every track.  stamps (float64
    [C + 1] on the device: one per source, then `now`) with C: dpp_pose_smooth_t, the same kernel over real elapsed time on a
    SmoothState(timed=True); spec's rate goes unread and src (None: every track is source 0) also names the track's stamp."""
    rate, mincutoff, beta, dcutoff, hold = spec
    if state.R < T + G or state.J != J:
        raise ValueError("the state has %d rows of %d joints, the launch %d of %d" % (state.R, state.J, T + G, J))
    if table is not None and src is None:
        raise ValueError("a source table needs src")
    fx, fy, ux, uy, flip = (0., 0., 0., 0., 0) if table is not None else cam
    grp = (fused_pose, n, fused_pose_f, gstat) if G else (None,) * 4
    if G and any(b is None for b in grp):
        raise ValueError("G = %d groups need fused_pose, n, fused_pose_f and gstat" % G)
    head = (pose3d.ptr, status.ptr, _p(src), T, J, _p(grp[0]), _p(grp[1]), int(G), None if table is None else table.dev.ptr, float(fx),
            float(fy), float(ux), float(uy), int(flip))
    tail = (state.xh.ptr, state.dxh.ptr, pose_f.ptr, pose_img_f.ptr, sstat.ptr, _p(grp[2]), _p(grp[3]))
    keep = (pose3d, status, src, None if table is None else table.dev, state, pose_f, pose_img_f, sstat) + grp
    if stamps is None:
        return Launch(rt.lib.dpp_pose_smooth, head + (rate, mincutoff, beta, dcutoff, hold, state.since.ptr) + tail, keep, name or 'pose_smooth')
    if state.tlast is None or C is None or stamps.size < int(C) + 1:
        raise ValueError("stamps need a timed state and C, the number of sources, with C + 1 stamps")
    return Launch(rt.lib.dpp_pose_smooth_t, head + (stamps.ptr, int(C), mincutoff, beta, dcutoff, hold, state.since.ptr, state.tlast.ptr) + tail,
                  keep + (stamps,), name or 'pose_smooth_t')


# ---- every track of a tick brought to one instant (include/dpp_hip.h, ABI v24; csrc/align.hip) ------------------------------------------
ALIGN_NONE, ALIGN_MOVED, ALIGN_ASIS, ALIGN_NOPREV, ALIGN_GAP, ALIGN_FAR = 0, 1, 2, 4, 8, 16        # DPP_ALIGN_*: dpp_pose_align's per-track word
SMOOTH_STALE = 32                                                                        # DPP_SMOOTH_STALE: dpp_pose_smooth_t's refusal bit


def timing_spec(timing):
    """dict(max_gap=, max_lead=) checked on the host -> (max_gap, max_lead), both in seconds: the longest step between two samples of a
    track over which a velocity is still formed (> 0), and the farthest a sample is moved to the tick's instant (>= 0).  Neither has a
    default: none has been chosen for a rig."""
    known = ('max_gap', 'max_lead')
    if not isinstance(timing, dict) or set(timing) - set(known):
        raise ValueError("timing takes max_gap and max_lead, not %r" % (sorted(set(timing) - set(known)) if isinstance(timing, dict) else timing,))
    missing = [k for k in known if k not in timing]
    if missing:
        raise ValueError("timing needs %s: no default has been chosen for a rig" % ', '.join(missing))
    try:
        gap, lead = float(timing['max_gap']), float(timing['max_lead'])
    except (TypeError, ValueError):
        raise ValueError("timing takes numbers: %r" % (timing,))
    if not (np.isfinite(gap) and gap > 0.):
        raise ValueError("max_gap (s) is finite and > 0: %r" % (timing['max_gap'],))
    if not (np.isfinite(lead) and lead >= 0.):
        raise ValueError("max_lead (s) is finite and >= 0: %r" % (timing['max_lead'],))
    return gap, lead


def tick_stamps(stamps, now, fresh, C):
    """The float64 [C + 1] array a timed tick uploads: one finite stamp (s) per source that delivers a frame (`fresh[c]` is not None; a
    source without one keeps 0., which nothing reads: its tracks are IDLE), then `now` -- by default the largest stamp of the fresh
    frames."""
    if stamps is None or len(stamps) != C:
        raise ValueError("a timed tick needs stamps: one per source (%d), None where the source has no frame" % C)
    out = np.zeros(C + 1, np.float64)
    for c in range(C):
        if fresh[c] is None:
            continue
        try:
            v = float(stamps[c])
        except (TypeError, ValueError):
            v = np.nan
        if not np.isfinite(v):
            raise ValueError("source %d delivers a frame without a finite stamp: %r" % (c, stamps[c]))
        out[c] = v
    live = [out[c] for c in range(C) if fresh[c] is not None]
    if now is None:
        now = max(live) if live else 0.
    if not np.isfinite(float(now)):
        raise ValueError("now is a finite time in seconds: %r" % (now,))
    out[C] = float(now)
    return out


class AlignState(object):
    """dpp_pose_align's device state over T tracks of J joints, never downloaded: `have` (int32 [T], 0: the row is empty), `pt` (float64
    [T], the previous stamp), `pp` / `pc` (float32 [T][J][3] / [T][3], the previous pose and centre; all three unused while have == 0).
    clear(t): one 4-byte upload."""

    def __init__(self, rt, T, J):
        self.T, self.J = int(T), int(J)
        self.have = rt.upload(np.zeros(self.T, np.int32))
        self.pt = rt.alloc((self.T,), np.float64)
        self.pp, self.pc = rt.alloc((self.T, self.J, 3), np.float32), rt.alloc((self.T, 3), np.float32)
        self._empty = np.zeros(1, np.int32)

    def clear(self, t):
        self.have.view(int(t), (1,)).set(self._empty)


def pose_align(rt, pose3d, com3d, status, src, T, J, stamps, C, spec, state, pose_t, pose_img_t, com3d_t, lead, astat, cam=None, table=None,
               name='pose_align'):
    """dpp_pose_align: one workgroup per track.  spec: timing_spec's tuple.  stamps: float64 [C + 1] on the device.  table: an
    ops.SourceTable with `src`, or None with `cam` for every track (src then still names the track's stamp; None: stamps[0])."""
    gap, lead_max = spec
    if state.T < T or state.J != J:
        raise ValueError("the state has %d rows of %d joints, the launch %d of %d" % (state.T, state.J, T, J))
    if table is not None and src is None:
        raise ValueError("a source table needs src")
    if stamps.size < int(C) + 1:
        raise ValueError("%d sources need %d stamps" % (C, int(C) + 1))
    fx, fy, ux, uy, flip = (0., 0., 0., 0., 0) if table is not None else cam
    return Launch(rt.lib.dpp_pose_align,
                  (pose3d.ptr, com3d.ptr, status.ptr, _p(src), T, J, stamps.ptr, int(C), None if table is None else table.dev.ptr, float(fx),
                   float(fy), float(ux), float(uy), int(flip), gap, lead_max, state.have.ptr, state.pt.ptr, state.pp.ptr, state.pc.ptr,
                   pose_t.ptr, pose_img_t.ptr, com3d_t.ptr, lead.ptr, astat.ptr),
                  (pose3d, com3d, status, src, stamps, None if table is None else table.dev, state, pose_t, pose_img_t, com3d_t, lead, astat), name)


def refine_com_iterative(rt, frames, partial, B, H, W, com_in, cube, fx, fy, num_iter, com_out, status, name='refine_com_iterative'):
    """dpp_refine_com_iterative: refineCoMIterative of B frames, all iterations in one launch."""
    return Launch(rt.lib.dpp_refine_com_iterative, (frames.ptr, partial.ptr, B, H, W, com_in.ptr, cube.ptr, float(fx), float(fy), int(num_iter),
                                                    com_out.ptr, status.ptr),
                  (frames, partial, com_in, cube, com_out, status), name)


def refine_com_iterative_ix(rt, frames, partial, R, src, H, W, com_in, cube, fx, fy, num_iter, com_out, status, name='refine_com_iterative'):
    """dpp_refine_com_iterative_ix: R rows, row r in frame src[r] with that frame's cube (src: an int32 device array the caller has
    checked with track_index, or None: row r reads frame r)."""
    return Launch(rt.lib.dpp_refine_com_iterative_ix, (frames.ptr, partial.ptr, R, _p(src), H, W, com_in.ptr, cube.ptr, float(fx), float(fy),
                                                       int(num_iter), com_out.ptr, status.ptr),
                  (frames, partial, src, com_in, cube, com_out, status), name)


DETECT_FOUND, DETECT_NO_SIZE = 1, 2          # DPP_DETECT_*: status bits of detect_seed / hand_size
DETECT_MAX_HANDS = 16                        # DPP_DETECT_MAX_HANDS
DETECT_REPORT = ('key', 'count', 'xmin', 'xmax', 'ymin', 'ymax')      # one slot of dpp_detect_seeds' report, int32 each
KEY_BACKGROUND = 255
# one record of dpp_label_components' statistics (include/dpp_hip.h), meaningful at roots
COMPONENT_STAT = np.dtype([('count', np.int32), ('ixmin', np.int32), ('xmax', np.int32), ('iymin', np.int32), ('ymax', np.int32),
                           ('pad', np.int32), ('sum_x', np.uint64), ('sum_y', np.uint64)])


class ComponentWorkspace(object):
    """What labelling B frames of H x W needs on the device, allocated once: keys, the union-find parents, labels, the per-root
    statistics and the selection words (cleared by slab_keys / mask_keys inside the plan); with candidates=True also the
    candidate list of detect_seeds (several hands of one frame)."""

    def __init__(self, rt, B, H, W, stats=True, candidates=False):
        lib = rt.lib
        nb = int(lib.dpp_label_workspace_bytes(B, H, W))
        if nb == 0 or int(lib.dpp_component_stats_bytes(1, 1, 1)) != COMPONENT_STAT.itemsize:
            raise DppError("component labelling cannot index %d frames of %d x %d" % (B, H, W))
        self.B, self.H, self.W = B, H, W
        self.keys = rt.alloc((B, H, W), np.uint8, zero=False)
        self.parent = rt.alloc(nb // 4, np.int32, zero=False)
        self.labels = rt.alloc((B, H, W), np.int32, zero=False)
        self.stats = rt.alloc(int(lib.dpp_component_stats_bytes(B, H, W)), np.uint8, zero=False) if stats else None
        self.state = rt.alloc(int(lib.dpp_detect_state_bytes(B)) // 8, np.int64)
        self.candidates = rt.alloc(int(lib.dpp_detect_candidates_bytes(B, H, W)) // 8, np.int64, zero=False) if candidates else None


def slab_keys(rt, frames, partial, ws, name='slab_keys'):
    """dpp_slab_keys: detect's 20 depth slabs as one uint8 key per pixel, from frame_range's partials."""
    B, H, W = ws.B, ws.H, ws.W
    return Launch(rt.lib.dpp_slab_keys, (frames.ptr, partial.ptr, B, H, W, ws.keys.ptr, ws.state.ptr), (frames, partial, ws), name,
                  dict(kernel='slab_keys', flops=4.0 * B * H * W, bytes=5.0 * B * H * W))


def mask_keys(rt, frames, com, cube, ws, name='mask_keys'):
    """dpp_mask_keys: the hand's depth range com_z -+ cube_z / 2 as a binary key."""
    B, H, W = ws.B, ws.H, ws.W
    return Launch(rt.lib.dpp_mask_keys, (frames.ptr, B, H, W, com.ptr, cube.ptr, ws.keys.ptr, ws.state.ptr), (frames, com, cube, ws), name,
                  dict(kernel='mask_keys', flops=4.0 * B * H * W, bytes=5.0 * B * H * W))


def label_components(rt, ws, stats=True, name='label_components'):
    """dpp_label_components on the workspace's keys: canonical 8-connected labels (+ per-root statistics)."""
    B, H, W = ws.B, ws.H, ws.W
    st = ws.stats if stats else None
    return Launch(rt.lib.dpp_label_components, (ws.keys.ptr, B, H, W, ws.parent.ptr, ws.labels.ptr, _p(st)), (ws,), name, kernels=4 if st else 3)


def detect_seed(rt, frames, partial, ws, com_out, status, name='detect_seed'):
    """dpp_detect_seed: the nearest component of more than 200 px and the centre of mass of its window."""
    B, H, W = ws.B, ws.H, ws.W
    return Launch(rt.lib.dpp_detect_seed, (frames.ptr, partial.ptr, ws.keys.ptr, ws.labels.ptr, ws.stats.ptr, B, H, W, ws.state.ptr, com_out.ptr,
                                           status.ptr),
                  (frames, partial, ws, com_out, status), name, kernels=2)


def detect_seeds(rt, frames, partial, ws, K, seed_out, status, report, max_extent=None, fx=1.0, fy=1.0, name='detect_seeds'):
    """dpp_detect_seeds: up to K seeds per frame (rows b * K + k) -- the candidates of more than 200 px in (key, root) order, minus
    those wider or higher than max_extent mm (None / 0: off), greedily selected under window suppression -- and the per-slot report."""
    B, H, W = ws.B, ws.H, ws.W
    if ws.candidates is None:
        raise ValueError("detect_seeds needs a ComponentWorkspace(candidates=True)")
    return Launch(rt.lib.dpp_detect_seeds, (frames.ptr, partial.ptr, ws.keys.ptr, ws.labels.ptr, ws.stats.ptr, B, H, W, ws.state.ptr,
                                            ws.candidates.ptr, int(K), float(max_extent or 0.0), float(fx), float(fy), seed_out.ptr, status.ptr,
                                            report.ptr),
                  (frames, partial, ws, seed_out, status, report), name, kernels=3)


def hand_size(rt, ws, com, cube_in, fx, fy, cube_out, status, tol=0.0, name='hand_size'):
    """dpp_hand_size: estimateHandsize from the bounding box of the largest labelled component."""
    B, H, W = ws.B, ws.H, ws.W
    return Launch(rt.lib.dpp_hand_size, (ws.keys.ptr, ws.labels.ptr, ws.stats.ptr, B, H, W, ws.state.ptr, com.ptr, cube_in.ptr, float(fx), float(fy),
                                         float(tol), cube_out.ptr, status.ptr),
                  (ws, com, cube_in, cube_out, status), name, kernels=2)


def copy2d(rt, src, lds, dst, ldd, rows, cols, relu=False, name='copy2d'):
    return Launch(rt.lib.dpp_copy2d, (src.ptr, lds, dst.ptr, ldd, rows, cols, int(bool(relu))), (src, dst), name)


def rowscale(rt, x, s, scol, factor, out, rows, cols, name='rowscale'):
    """out[r][c] = x[r][c] * (s[r][scol] * factor); s has s.shape[-1] columns."""
    return Launch(rt.lib.dpp_rowscale, (x.ptr, s.ptr, int(s.shape[-1]), int(scol), float(factor), out.ptr, int(rows), int(cols)), (x, s, out), name)


def crop_center(rt, src, B, H, W, dst, h, w, name='crop_center'):
    return Launch(rt.lib.dpp_crop_center, (src.ptr, B, H, W, dst.ptr, h, w), (src, dst), name)


def fill_zero(rt, buf, name='fill_zero'):
    return Launch(rt.lib.dpp_fill_zero, (buf.ptr, buf.nbytes), (buf,), name)


def bernoulli_mask(rt, mask, n, keep, seed, counter, counter_dev=None, name='bernoulli_mask'):
    return Launch(rt.lib.dpp_bernoulli_mask, (mask.ptr, n, float(keep), int(seed), int(counter), _p(counter_dev)), (mask, counter_dev), name)


def adam_tick(rt, state, name='adam_tick'):
    return Launch(rt.lib.dpp_adam_tick, (state.ptr,), (state,), name)


def counter_add(rt, counter, inc=1, name='counter_add'):
    return Launch(rt.lib.dpp_counter_add, (counter.ptr, int(inc)), (counter,), name)


class ReduceJobs(object):
    """Collects (partial, nz, n, out) reductions and emits ONE dpp_reduce_multi launch for all of them."""

    def __init__(self, rt):
        self.rt = rt
        self.jobs = []

    def add(self, partial, nz, n, out):
        self.jobs.append((partial, int(nz), int(n), out))

    def pending_bytes(self):
        return 4 * sum(nz * n for (_, nz, n, _) in self.jobs)

    def flush(self, name='reduce_multi'):
        """The launch for the jobs collected so far; the list starts over (several launches per pass, see engine._emit_backward)."""
        op = self.launch(name)
        self.jobs = []
        return op

    def launch(self, name='reduce_multi'):
        if not self.jobs:
            return None
        import struct
        rt = self.rt
        assert rt.lib.dpp_reduce_job_bytes() == 32
        raw, block0 = b'', 0
        cols = rt.lib.dpp_reduce_multi_block_cols()
        for (partial, nz, n, out) in self.jobs:
            raw += struct.pack('<QQiiii', partial.ptr, out.ptr, nz, n, block0, 0)
            block0 += -(-n // cols)
        table = rt.upload(np.frombuffer(raw, np.uint8).copy())
        flops = float(sum(nz * n for (_, nz, n, _) in self.jobs))
        return Launch(rt.lib.dpp_reduce_multi, (table.ptr, len(self.jobs), block0), (table, list(self.jobs)), name,
                      dict(kernel='reduce_multi', flops=flops, bytes=4.0 * flops))
