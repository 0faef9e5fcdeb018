"""Every access of the MFMA training kernels that leaves the problem: each operand of each launch here lies between two 64 KiB bands of
0x7FC0DEAD words inside one allocation (tests/guards.py), leading-dimension padding and the rows a strided row map skips hold the same
NaN, and after the launch (a) the valid region equals the float64 reference within the tolerance the family's own test uses, (b) no
sentinel remains in it while every band, padding column and unaddressed row of an output is bit-intact, (c) every input is bit-unchanged,
(d) -- which follows from (a) -- nothing read from outside the problem reached a result.  Runs on the SIMT emulator in the CPU tier and
through the C ABI of libdpp_hip.so on the MI355X (`-m gpu`), where the workgroups of a launch run concurrently.

Misaligned operands.  Every pointer of these entry points, what the host does with one that is one element off a 16-byte boundary
(8 bytes for a bf16-stored tensor), and where that is decided.  "refused" means an error status before anything is launched.

  dpp_gemm (gemm_prepare, csrc/gemm.hip: vecA / vecB / wide and the DPP_E_BADARG lines under them)
    A, with a mode-4 prologue also actA.x2 and actA.out    vecA = false: scalar operand loads (and stores of the copy); variants 2-4 refuse
    B                                                      vecB = false: scalar operand loads; variants 2-4 refuse (DPP_E_UNSUPPORTED)
    C, residual, bias, epi.bn_x,
    epi.bn_mean / bn_inv_std / bn_scale / bn_beta          wide = false: the one-float-per-store epilogue (gemm_epilogue)
    actA / actB mean, scale, beta (modes 2, 3), actA.aux   refused: DPP_E_BADARG
    partial, epi.stats, epi.bn_partial                     not looked at: stored one float at a time; tolerated (emulator-only cases)
  dpp_fc_gemm (csrc/fcgemm.hip)
    A, B                                                   fs_accepts declines the three-stage kernel, fc_gemm_kernel loads one float at a time
    C / partial, residual, bias                            refused: DPP_E_UNSUPPORTED
    actA / actB mean, scale, beta                          were looked at by fs_accepts only, but fc_gemm_kernel loads them 16 bytes at a time too:
                                                           now refused, DPP_E_BADARG
  dpp_conv3x3 / dpp_conv3x3_bf16 (conv3x3_launch, csrc/conv3x3.hip: a.wide)
    Y, residual, bias, epi.bn_x and the four bn vectors    a.wide = false: the narrow epilogue
    X, Wk, act mean / scale / beta                         were not looked at, loaded 16 bytes at a time: now refused, DPP_E_BADARG
  dpp_conv3x3_stream                                       X, Wk, act vectors: refused (DPP_E_UNSUPPORTED).  Y, bias, epi.*: one float per access,
                                                           tolerated (emulator-only cases)
  dpp_conv3x3_wgrad (+ _bf16)                              X, dY, act vectors were not looked at, loaded 8 / 16 bytes at a time: now refused,
                                                           DPP_E_BADARG.  partial: stored float by float, tolerated (emulator-only case)
  dpp_wgrad_stream (+ _bf16), dpp_wgrad3_stream,
  dpp_fc_wgrad_stream                                      dY, X, partial / dW: DPP_E_BADARG; the prologue vectors were not looked at, loaded 8 / 16
                                                           bytes at a time (load_vec): now refused, DPP_E_BADARG
  dpp_stem_wgrad (stem_wgrad_kernel itself, `vec`)         dY, argmax: element-by-element loads.  dpp_stem_fwd stores the mask byte by byte
  dpp_convpool_fwd / _wgrad / _dgrad                       nothing looked at, every global access one element wide: tolerated (emulator-only cases)
  dpp_bn_stats_partial, _bwd_reduce, _bwd_apply,
  _bwd_finalize_apply                                      the [M][C] tensors and the per-channel vectors they read (and finalize_apply's block sums
                                                           when nb % 4 == 0) were not looked at, accessed four channels at a time: now refused,
                                                           DPP_E_BADARG.  Partials, column sums, dbeta / dgamma: float by float, tolerated (emulator only)
  dpp_bn_finalize, dpp_bn_bwd_finalize                     one float per access throughout; run aligned here
  dpp_reduce_multi (reduce_multi_kernel itself, `vec`)     partial, out: the scalar path
  dpp_reduce_partials                                      one-float accesses only; run aligned here

Each case below runs the family's smallest problem with ONE pointer moved by one element, guarded like every other launch, and
asserts the outcome the code prescribes: the same values within the same tolerance, or DppError with every buffer bit-unchanged.  Which
path a launch took cannot be seen from outside (the walking conv3x3 apart, which reports it): it is read from the conditions named
above.  On the GPU tier a kernel runs with a misaligned pointer only where the dispatch (or, for the stem and dpp_reduce_multi, the
kernel) branches on that pointer; the tolerated pointers nothing looks at run misaligned on the emulator only."""
import numpy as np
import pytest

from hipdp import layout, ops
from hipdp.lib import Act, DppError, RowMap
from oracle import layers as L
from tests.backends import BACKENDS, get_runtime
from tests.guards import NAN, Guards, all_written, fetch, padded, untouched
from tests.test_gemm import _check as gemm_check

f32, f64 = np.float32, np.float64


def _vec(rng, n, kind='normal'):
    return (rng.uniform(0.5, 1.5, n) if kind == 'scale' else rng.normal(0, 0.3, n)).astype(f32)


def _bn_relu(a, coef, relu=True):
    mean, scale, beta = (c.astype(f64) for c in coef)
    v = (a.astype(f64) - mean) * scale + beta
    return np.maximum(v, 0) if relu else v


# ======================================================================================================================
# dpp_gemm, variant 0 (the LDS-tiled kernel)
# ======================================================================================================================
GEMM_SHAPES = [(200, 48, 40), (37, 30, 50), (130, 68, 100), (17, 20, 36), (5, 7, 3), (129, 132, 65)]
GEMM_LAYOUTS = [(1, 1), (1, 0), (0, 0)]
GEMM_TILES = [(0, 0, 0), (128, 64, 4), (64, 16, 4), (16, 64, 1)]


def _operand(g, op, kc, pad, off=0, name=None):
    """A [rows][K] (or B [N][K]) operand value matrix `op`, laid out K-contiguous (kc = 1) or transposed, with `pad` NaN padding columns:
    (the guarded view, the leading dimension)."""
    mem = op if kc else op.T
    ld = mem.shape[1] + pad
    return g.inp(padded(mem, ld), off=off, name=name), ld


def _gemm_plain(rt, M, N, K, a_kc, b_kc, pad, tile, seed=1, offs=(), splitk=1, with_bias=False, with_res=False):
    """One guarded launch of C = A_op . B_op^T (+ bias + aliased residual), checked against float64."""
    rng = np.random.RandomState(seed + M + 7 * N + 131 * K)
    A = rng.normal(size=(M, K)).astype(f32)
    B = rng.normal(size=(N, K)).astype(f32)
    g = Guards(rt)
    dA, lda = _operand(g, A, a_kc, pad, 'A' in offs, 'A')
    dB, ldb = _operand(g, B, b_kc, pad, 'B' in offs, 'B')
    ldc = N + pad
    ref = A.astype(f64) @ B.astype(f64).T
    bias = res = db = None
    if with_bias:
        bias = rng.normal(size=N).astype(f32)
        db = g.inp(bias, off='bias' in offs, name='bias')
        ref = ref + bias
    if with_res:
        res = rng.normal(size=(M, N)).astype(f32)
        ref = ref + res
    if splitk > 1:
        part = g.out((splitk, M * N), name='partial', off='partial' in offs)
        ops.gemm(rt, dA, dB, None, M, N, K, a_kc, b_kc, lda, ldb, splitk=splitk, partial=part, tile=tile)(rt.stream)
        rt.synchronize()
        p = fetch(part)
        assert all_written(p)
        got = p.astype(f64).sum(axis=0).reshape(M, N)
    else:
        dC = g.out((M, ldc), name='C', off='C' in offs, init=padded(res, ldc) if with_res else None)
        ops.gemm(rt, dA, dB, dC, M, N, K, a_kc, b_kc, lda, ldb, ldc, bias=db, residual=dC if with_res else None, tile=tile)(rt.stream)
        rt.synchronize()
        c = fetch(dC)
        assert all_written(c[:, :N]) and untouched(c[:, N:])
        got = c[:, :N]
    gemm_check(got, ref, K, 4)
    g.check()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('layout_', GEMM_LAYOUTS, ids=lambda v: 'a%db%d' % v)
@pytest.mark.parametrize('shape', GEMM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_gemm_tiles_layouts_and_padding(backend, shape, layout_):
    rt = get_runtime(backend)
    M, N, K = shape
    for pad in (0, 4):
        for tile in GEMM_TILES:
            _gemm_plain(rt, M, N, K, layout_[0], layout_[1], pad, tile)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('layout_', GEMM_LAYOUTS, ids=lambda v: 'a%db%d' % v)
def test_gemm_splitk_bias_and_aliased_residual(backend, layout_):
    rt = get_runtime(backend)
    for (M, N, K) in ((37, 30, 50), (129, 132, 65), (17, 20, 36)):
        for pad in (0, 4):
            _gemm_plain(rt, M, N, K, layout_[0], layout_[1], pad, (0, 0, 0), splitk=3)
            _gemm_plain(rt, M, N, K, layout_[0], layout_[1], pad, (64, 16, 4), with_bias=True, with_res=True)
            _gemm_plain(rt, M, N, K, layout_[0], layout_[1], pad, (16, 64, 1), with_bias=True)


@pytest.mark.parametrize('backend', BACKENDS)
def test_gemm_refuses_the_layout_it_does_not_have(backend):
    """a_kc = 0 with b_kc = 1: DPP_E_UNSUPPORTED before any launch."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(2)
    for (M, N, K) in GEMM_SHAPES:
        g = Guards(rt)
        dA, dB = g.inp(rng.normal(size=(K, M))), g.inp(rng.normal(size=(N, K)))
        dC = g.out((M, N))
        with pytest.raises(DppError, match='10002'):
            ops.gemm(rt, dA, dB, dC, M, N, K, 0, 1, M, K, N)(rt.stream)
        rt.synchronize()
        assert untouched(fetch(dC))
        g.check()


class _BN(object):
    pass


def _bn_object(g, rng, C, off=None):
    bn, v = _BN(), {}
    v['mean'], v['scale'], v['beta_buf'], v['inv_std'] = _vec(rng, C), _vec(rng, C, 'scale'), _vec(rng, C), _vec(rng, C, 'scale')
    for k, a in v.items():
        setattr(bn, k, g.inp(a, off=(off == k), name='bn.' + k))
    return bn, v


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('tile', [(64, 16, 4), (16, 64, 1), (128, 64, 4)], ids=lambda t: 'x'.join(map(str, t)))
def test_gemm_statistics_and_batchnorm_backward_epilogues(backend, tile):
    """300 rows x 48 columns: a ragged last row block in every tile; the per-block (mean, M2) and (sum G, sum G xhat) partials guarded."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(31)
    M, K, N, bm = 300, 32, 48, tile[0]
    nblk = -(-M // bm)
    x = (rng.normal(size=(M, K)) + 3.0).astype(f32)
    Wk = (rng.normal(size=(N, K)) * 0.2).astype(f32)
    res, bias = rng.normal(size=(M, N)).astype(f32), rng.normal(size=N).astype(f32)
    for pad in (0, 4):
        g = Guards(rt)
        xb, lda = _operand(g, x, 1, pad, name='X')
        wb, ldb = _operand(g, Wk, 1, pad, name='W')
        ldc = N + pad
        Y = g.out((M, ldc), name='Y')
        stats = g.out((2, N, nblk), name='stats')
        ops.gemm(rt, xb, wb, Y, M, N, K, 1, 1, lda, ldb, ldc, bias=g.inp(bias), residual=g.inp(padded(res, ldc), name='res'), tile=tile,
                 epi=ops.epilogue(stats=stats))(rt.stream)
        mean, istd, scale = (g.out((N,), name=n) for n in ('mean', 'inv_std', 'scale'))
        ops.bn_finalize(rt, stats, nblk, M, bm, N, g.inp(np.ones(N, f32)), 1e-4, mean, istd, scale)(rt.stream)
        rt.synchronize()
        y_ref = x.astype(f64) @ Wk.astype(f64).T + bias + res
        y = fetch(Y)
        assert all_written(y[:, :N]) and untouched(y[:, N:]) and all_written(fetch(stats))
        np.testing.assert_allclose(y[:, :N], y_ref, rtol=0, atol=3e-5 * np.abs(y_ref).max())
        np.testing.assert_allclose(fetch(mean), y_ref.mean(0), rtol=0, atol=3e-6 * np.abs(y_ref).max())
        np.testing.assert_allclose(fetch(istd), 1 / np.sqrt(y_ref.var(0) + f32(1e-4)), rtol=3e-5)
        g.check()
        _gemm_dgrad_bn_epilogue(rt, rng, x, Wk, (bm, 32 if tile[2] == 4 else 64, tile[2]), pad)


def _gemm_dgrad_bn_epilogue(rt, rng, x, Wk, tile, pad, off=None):
    """The data gradient of y = x . Wk^T with the BatchNorm-backward epilogue (G = dA * [bn(x) >= 0], per-block sums of G and G xhat);
    off: 'bn_x', or the name of one of the four BatchNorm vectors, to move by one element."""
    (M, K), N = x.shape, Wk.shape[0]
    nblk = -(-M // tile[0])
    g = Guards(rt)
    dy = rng.normal(size=(M, N)).astype(f32)
    bn, v = _bn_object(g, rng, K, off=off)
    bnx = g.inp(padded(x, K + pad), name='bn_x', off=int(off == 'bn_x'))
    dyb, ldy = _operand(g, dy, 1, pad, name='dY')
    wt, ldw = g.inp(padded(Wk, K + pad), name='W'), K + pad                     # B [k = N][n = K]
    G = g.out((M, K + pad), name='G')
    part = g.out((2, K, nblk), name='bn_partial', off=int(off == 'bn_partial'))
    ops.gemm(rt, dyb, wt, G, M, K, N, 1, 0, ldy, ldw, K + pad, tile=tile, epi=ops.epilogue(bn=bn, bn_x=bnx, bn_relu=True, bn_partial=part))(rt.stream)
    rt.synchronize()
    da_ref = dy.astype(f64) @ Wk.astype(f64)
    val = (x.astype(f64) - v['mean']) * v['scale'] + v['beta_buf']
    safe = np.abs(val) > 1e-4
    got = fetch(G)
    assert all_written(got[:, :K]) and untouched(got[:, K:]) and all_written(fetch(part))
    got = got[:, :K]
    np.testing.assert_allclose(got[safe], (da_ref * (val >= 0))[safe], rtol=0, atol=3e-5 * np.abs(da_ref).max())
    p = fetch(part).astype(f64).sum(axis=2)
    xhat = (x.astype(f64) - v['mean']) * v['inv_std']
    np.testing.assert_allclose(p[0], got.astype(f64).sum(0), rtol=0, atol=3e-5 * np.sqrt(M) * np.abs(got).max())
    np.testing.assert_allclose(p[1], (got.astype(f64) * xhat).sum(0), rtol=0, atol=3e-4 * np.sqrt(M) * np.abs(got).max())
    g.check()


def _strided_rows(Nb, Ho, Wo, Hi, Wi, s):
    n, q = np.divmod(np.arange(Nb * Ho * Wo), Ho * Wo)
    y, x = np.divmod(q, Wo)
    return n * Hi * Wi + (y * s) * Wi + x * s


@pytest.mark.parametrize('backend', BACKENDS)
def test_gemm_prologues_and_stride2_row_maps(backend):
    """The geometry of test_conv1x1_stride2_*: the rows the stride-2 map skips hold NaN (operand) or the sentinel (output), and so do
    three rows behind the map; the BatchNorm + ReLU coefficient vectors of the A and the B prologue are guarded."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(3)
    Nb, Hi, Wi, Ci, Co, s = 3, 8, 6, 32, 16, 2
    Ho, Wo = Hi // s, Wi // s
    M, rows = Nb * Ho * Wo, Nb * Hi * Wi
    at = _strided_rows(Nb, Ho, Wo, Hi, Wi, s)
    mp = RowMap.strided(s, Ho, Wo, Hi, Wi)
    for pad in (0, 4):
        # forward: A rows gathered, prologue on A, bias, residual
        g = Guards(rt)
        xv = rng.normal(size=(M, Ci)).astype(f32)
        X = np.full((rows + 3, Ci + pad), NAN, f32)
        X[at, :Ci] = xv
        Wk = rng.normal(size=(Co, Ci)).astype(f32)
        coef = [_vec(rng, Ci), _vec(rng, Ci, 'scale'), _vec(rng, Ci)]
        bias, res = rng.normal(size=Co).astype(f32), rng.normal(size=(M, Co)).astype(f32)
        cb = [g.inp(c, name='actA %d' % i) for i, c in enumerate(coef)]
        Y = g.out((M, Co + pad), name='Y')
        ops.gemm(rt, g.inp(X, name='X'), g.inp(padded(Wk, Ci + pad), name='W'), Y, M, Co, Ci, 1, 1, Ci + pad, Ci + pad, Co + pad, mapA=mp,
                 actA=ops.act(Act.BN_RELU, cb[0], cb[1], cb[2], Ci), bias=g.inp(bias), residual=g.inp(padded(res, Co + pad)))(rt.stream)
        rt.synchronize()
        y = fetch(Y)
        assert all_written(y[:, :Co]) and untouched(y[:, Co:])
        gemm_check(y[:, :Co], _bn_relu(xv, coef) @ Wk.astype(f64).T + bias + res, Ci, 8)
        g.check()
        # data gradient: C rows scattered, the second launch accumulates through the aliased residual
        g = Guards(rt)
        dY1, dY2 = rng.normal(size=(M, 16)).astype(f32), rng.normal(size=(M, 64)).astype(f32)
        W1, W2 = rng.normal(size=(16, Ci)).astype(f32), rng.normal(size=(64, Ci)).astype(f32)
        dH = g.out((rows + 3, Ci + pad), name='dH')
        ops.gemm(rt, g.inp(padded(dY2, 64 + pad)), g.inp(padded(W2, Ci + pad)), dH, M, Ci, 64, 1, 0, 64 + pad, Ci + pad, Ci + pad, mapC=mp)(rt.stream)
        ops.gemm(rt, g.inp(padded(dY1, 16 + pad)), g.inp(padded(W1, Ci + pad)), dH, M, Ci, 16, 1, 0, 16 + pad, Ci + pad, Ci + pad, mapC=mp,
                 residual=dH)(rt.stream)
        rt.synchronize()
        h = fetch(dH)
        skipped = np.setdiff1d(np.arange(rows + 3), at)
        assert all_written(h[at, :Ci]) and untouched(h[at, Ci:]) and untouched(h[skipped])
        gemm_check(h[at, :Ci], dY1.astype(f64) @ W1 + dY2.astype(f64) @ W2, 80, 8)
        g.check()
        # filter gradient: both operands [kred][mn], prologue on B, the stride-2 map on the reduction index, split-K 3
        for tile in ((0, 0, 0), (16, 64, 1), (64, 64, 4)):
            g = Guards(rt)
            dY = rng.normal(size=(M, Co)).astype(f32)
            cb = [g.inp(c, name='actB %d' % i) for i, c in enumerate(coef)]
            part = g.out((3, Co * Ci), name='partial')
            ops.gemm(rt, g.inp(padded(dY, Co + pad), name='dY'), g.inp(X, name='X'), None, Co, Ci, M, 0, 0, Co + pad, Ci + pad, mapB=mp,
                     actB=ops.act(Act.BN_RELU, cb[0], cb[1], cb[2], Ci), splitk=3, partial=part, tile=tile)(rt.stream)
            rt.synchronize()
            p = fetch(part)
            assert all_written(p)
            gemm_check(p.astype(f64).sum(0).reshape(Co, Ci), dY.astype(f64).T @ _bn_relu(xv, coef), M, 8)
            g.check()


GEMM_SMALL = (20, 24, 36)                  # whole quads in M, N and K, so every leading dimension is one too: with aligned pointers every 16-byte path is open


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('which', ['A', 'B', 'C', 'bias'])
@pytest.mark.parametrize('layout_', GEMM_LAYOUTS, ids=lambda v: 'a%db%d' % v)
def test_gemm_misaligned_operand_takes_the_scalar_path(backend, layout_, which):
    """One of A, B, C (with the residual that aliases it) and bias four bytes off a 16-byte boundary: gemm_prepare clears vecA / vecB / wide,
    the kernel loads that operand one float at a time or stores through the narrow epilogue, and the result is as good as the aligned one."""
    rt = get_runtime(backend)
    M, N, K = GEMM_SMALL
    for tile in ((0, 0, 0), (64, 16, 4)):
        _gemm_plain(rt, M, N, K, layout_[0], layout_[1], 4, tile, offs=(which,), with_bias=True, with_res=True)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('which', ['bn_x', 'mean', 'scale', 'beta_buf', 'inv_std'])
def test_gemm_misaligned_batchnorm_epilogue_operand_takes_the_narrow_epilogue(backend, which):
    rt = get_runtime(backend)
    rng = np.random.RandomState(37)
    M, K, N = 40, 32, 16
    x = (rng.normal(size=(M, K)) + 1.0).astype(f32)
    Wk = (rng.normal(size=(N, K)) * 0.2).astype(f32)
    _gemm_dgrad_bn_epilogue(rt, rng, x, Wk, (16, 64, 1), 4, off=which)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('side', ['A', 'B'])
@pytest.mark.parametrize('which', [0, 1, 2], ids=['mean', 'scale', 'beta'])
def test_gemm_refuses_a_misaligned_prologue_vector(backend, side, which):
    """The BatchNorm + ReLU coefficient vectors are read 16 bytes at a time: DPP_E_BADARG, nothing launched."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(5)
    M, N, K = GEMM_SMALL
    g = Guards(rt)
    dA, dB, dC = g.inp(rng.normal(size=(M, K)), name='A'), g.inp(rng.normal(size=(N, K)), name='B'), g.out((M, N), name='C')
    cb = [g.inp(_vec(rng, K), off=int(i == which)) for i in range(3)]
    a = ops.act(Act.BN_RELU, cb[0], cb[1], cb[2], K)
    with pytest.raises(DppError, match='10001'):
        ops.gemm(rt, dA, dB, dC, M, N, K, 1, 1, K, K, N, actA=a if side == 'A' else None, actB=a if side == 'B' else None)(rt.stream)
    rt.synchronize()
    assert untouched(fetch(dC))
    g.check()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('which', [None, 'G', 'x2', 'out', 'aux'])
def test_gemm_mode4_operand_alignment(backend, which):
    """The mode-4 operand of test_gemm_operand_through_batchnorm_backward (a_kc = 1), guarded.  gemm_prepare (csrc/gemm.hip) clears vecA
    when A (here G), actA.x2 or actA.out is four bytes off -- the operand, its BatchNorm input and the copy it leaves then go one float at
    a time, same tolerances -- and answers DPP_E_BADARG for a misaligned actA.aux, with nothing launched."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(77)
    Mp, Cc, Co = 75, 24, 100
    o = lambda name: int(which == name)                                            # noqa: E731
    Gm, Xm = rng.normal(size=(Mp, Cc)).astype(f32), (rng.normal(size=(Mp, Cc)) * 2 + 5).astype(f32)
    mean = Xm.mean(0).astype(f32)
    istd = (1 / np.sqrt(Xm.var(0) + 1e-4)).astype(f32)
    scale = (rng.uniform(0.5, 1.5, Cc) * istd).astype(f32)
    c1, c2 = rng.normal(size=Cc).astype(f32) * 0.1, rng.normal(size=Cc).astype(f32) * 0.1
    Wm = rng.normal(size=(Cc, Co)).astype(f32)
    dX = scale.astype(f64) * (Gm.astype(f64) - c1 - (Xm.astype(f64) - mean) * istd * c2)
    g = Guards(rt)
    bn = _BN()
    bn.mean, bn.inv_std, bn.scale = g.inp(mean, name='mean'), g.inp(istd, name='inv_std'), g.inp(scale, name='scale')
    q, p = g.inp(scale * c1, name='q'), g.inp(scale * istd * c2, name='aux', off=o('aux'))
    out, copy = g.out((Mp, Co), name='C'), g.out((Mp, Cc), name='actA.out', off=o('out'))
    launch = ops.gemm(rt, g.inp(Gm, name='G', off=o('G')), g.inp(Wm, name='W'), out, Mp, Co, Cc, 1, 0, Cc, Co, Co,
                      actA=ops.act_bn_bwd(bn, q, p, g.inp(Xm, name='x2', off=o('x2')), Cc, out=copy))
    if which == 'aux':
        with pytest.raises(DppError, match='10001'):
            launch(rt.stream)
        rt.synchronize()
        assert untouched(fetch(out)) and untouched(fetch(copy))
    else:
        launch(rt.stream)
        rt.synchronize()
        c, y = fetch(copy), fetch(out)
        assert all_written(c) and all_written(y)
        ref = dX @ Wm.astype(f64)
        np.testing.assert_allclose(c, dX, rtol=0, atol=2e-6 * np.abs(dX).max())
        np.testing.assert_allclose(y, ref, rtol=0, atol=2e-5 * np.abs(ref).max())
    g.check()


@pytest.mark.parametrize('backend', BACKENDS[:1])
@pytest.mark.parametrize('which', ['partial', 'bn_partial', 'stats'])
def test_gemm_tolerates_four_byte_aligned_partials_and_statistics(backend, which):
    """partial, epi.stats and epi.bn_partial are no part of gemm_prepare's alignment facts; the kernels store them one float at a time
    (include/dpp_hip.h says so).  Emulator only: on the GPU tier a misaligned pointer goes only where the dispatch branches on it."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(41)
    M, N, K = GEMM_SMALL
    if which == 'partial':
        for layout_ in GEMM_LAYOUTS:
            _gemm_plain(rt, M, N, K, layout_[0], layout_[1], 4, (0, 0, 0), offs=('partial',), splitk=3)
        return
    x, Wk = (rng.normal(size=(40, 32)) + 1.0).astype(f32), (rng.normal(size=(16, 32)) * 0.2).astype(f32)
    if which == 'bn_partial':
        _gemm_dgrad_bn_epilogue(rt, rng, x, Wk, (16, 64, 1), 4, off='bn_partial')
        _gemm_dgrad_bn_epilogue(rt, rng, x, Wk, (64, 32, 4), 0, off='bn_partial')
        return
    for tile in ((16, 64, 1), (64, 16, 4)):
        g = Guards(rt)
        Mx, Kx, Nx = 40, 32, 16
        nblk = -(-Mx // tile[0])
        Y, stats = g.out((Mx, Nx), name='Y'), g.out((2, Nx, nblk), name='stats', off=1)
        ops.gemm(rt, g.inp(x, name='X'), g.inp(Wk, name='W'), Y, Mx, Nx, Kx, 1, 1, Kx, Kx, Nx, tile=tile, epi=ops.epilogue(stats=stats))(rt.stream)
        mean, istd, scale = (g.out((Nx,), name=n) for n in ('mean', 'inv_std', 'scale'))
        ops.bn_finalize(rt, stats, nblk, Mx, tile[0], Nx, g.inp(np.ones(Nx, f32)), 1e-4, mean, istd, scale)(rt.stream)
        rt.synchronize()
        y_ref = x.astype(f64) @ Wk.astype(f64).T
        assert all_written(fetch(Y)) and all_written(fetch(stats))
        np.testing.assert_allclose(fetch(Y), y_ref, rtol=0, atol=3e-5 * np.abs(y_ref).max())
        np.testing.assert_allclose(fetch(mean), y_ref.mean(0), rtol=0, atol=3e-6 * np.abs(y_ref).max())
        np.testing.assert_allclose(fetch(istd), 1 / np.sqrt(y_ref.var(0) + f32(1e-4)), rtol=3e-5)
        g.check()


# ======================================================================================================================
# dpp_gemm, variants 1-4 (row stream, K-split, 16-column stream, expand)
# ======================================================================================================================
#                 variant, tile, M, N, K, rows per statistics block
VARIANT_CASES = [(1, (64, 16, 4), 180, 16, 32, 64),            # smallest of test_rowstream_variant_fwd_and_dgrad: 180 rows, a ragged third block
                 (1, (64, 16, 4), 180, 24, 40, 64),            # ... and its K, N off the tile grid
                 (1, (128, 32, 4), 130, 64, 128, 128),         # two rows in the last block
                 (2, (32, 32, 4), 96, 32, 128, 32),            # smallest of test_ksplit_variant_fwd_and_dgrad
                 (2, (32, 64, 4), 64, 64, 256, 32),
                 (3, (128, 16, 4), 384, 16, 64, 128),          # test_stream16_variant_against_the_tiled_kernel
                 (3, (64, 64, 4), 384, 64, 16, 64),
                 (4, (32, 64, 4), 96, 64, 16, 32),             # smallest of test_expand_variant_fwd_and_dgrad
                 (4, (64, 64, 4), 128, 128, 32, 64)]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('case', VARIANT_CASES, ids=lambda c: 'v%d-%dx%dx%d' % (c[0], c[2], c[3], c[4]))
def test_gemm_variants_forward_and_data_gradient(backend, case):
    """Forward (BatchNorm + ReLU prologue, bias, residual aliasing the output, fused statistics) and data gradient (B in [k][n] layout
    accumulating onto an earlier share; variants 0, 3 and 4 have the BatchNorm-backward epilogue) of the special-purpose kernels.
    Variants 2-4 take whole row blocks only: eight rows fewer is refused (DPP_E_UNSUPPORTED) with every buffer untouched."""
    rt = get_runtime(backend)
    variant, tile, M, N, K, rows = case
    rng = np.random.RandomState(8 + variant)
    X, Wk = rng.normal(size=(M, K)).astype(f32), (rng.normal(size=(N, K)) * 0.3).astype(f32)
    coef = [_vec(rng, K), _vec(rng, K, 'scale'), _vec(rng, K)]
    bias, res = rng.normal(size=N).astype(f32), rng.normal(size=(M, N)).astype(f32)
    nblk = -(-M // rows)
    for Mrun in ((M,) if variant == 1 else (M, M - 8)):
        g = Guards(rt)
        cb = [g.inp(c, name='act %d' % i) for i, c in enumerate(coef)]
        Y = g.out((M, N), name='Y', init=res)
        stats = g.out((2, N, nblk), name='stats')
        launch = ops.gemm(rt, g.inp(X, name='X'), g.inp(Wk, name='W'), Y, Mrun, N, K, 1, 1, K, K, N, actA=ops.act(Act.BN_RELU, cb[0], cb[1], cb[2], K),
                          bias=g.inp(bias, name='bias'), residual=Y, tile=tile, variant=variant, epi=ops.epilogue(stats=stats))
        if Mrun != M:
            assert ops.gemm_variant_rows(rt, launch) == 0
            with pytest.raises(DppError, match='10002'):
                launch(rt.stream)
            rt.synchronize()
            assert np.array_equal(fetch(Y).view(np.uint32), res.view(np.uint32)) and untouched(fetch(stats))
            g.check()
            continue
        launch(rt.stream)
        mean, istd, scale = (g.out((N,), name=n) for n in ('mean', 'inv_std', 'scale'))
        ops.bn_finalize(rt, stats, nblk, M, rows, N, g.inp(np.ones(N, f32)), 1e-4, mean, istd, scale)(rt.stream)
        rt.synchronize()
        ref = _bn_relu(X, coef) @ Wk.astype(f64).T + bias + res
        y = fetch(Y)
        assert all_written(y) and all_written(fetch(stats))
        gemm_check(y, ref, K, 8)
        np.testing.assert_allclose(fetch(mean), ref.mean(0), rtol=0, atol=3e-6 * np.abs(ref).max())
        np.testing.assert_allclose(fetch(istd), 1 / np.sqrt(ref.var(0) + f32(1e-4)), rtol=3e-5)
        g.check()
    # data gradient of a conv with K output and N input channels: dA[m][c] = share[m][c] + sum_o dY[m][o] W2[o][c]
    g = Guards(rt)
    W2, dY, share = (rng.normal(size=(K, N)) * 0.3).astype(f32), rng.normal(size=(M, K)).astype(f32), rng.normal(size=(M, N)).astype(f32)
    dH = g.out((M, N), name='dH', init=share)
    with_bn = variant in (3, 4)
    epi = None
    if with_bn:
        bn, bv = _bn_object(g, rng, N)
        bnx = rng.normal(size=(M, N)).astype(f32)
        part = g.out((2, N, nblk), name='bn_partial')
        epi = ops.epilogue(bn=bn, bn_x=g.inp(bnx, name='bn_x'), bn_relu=True, bn_partial=part)
    dtile = (tile[0], 16 if N < 32 else 32, 4) if variant == 1 else tile
    ops.gemm(rt, g.inp(dY, name='dY'), g.inp(W2, name='W2'), dH, M, N, K, 1, 0, K, N, N, residual=dH, tile=dtile, variant=variant, epi=epi)(rt.stream)
    rt.synchronize()
    want = share.astype(f64) + dY.astype(f64) @ W2.astype(f64)
    h = fetch(dH)
    assert all_written(h)
    if with_bn:
        val = (bnx.astype(f64) - bv['mean']) * bv['scale'] + bv['beta_buf']
        safe = np.abs(val) > 1e-4
        want = np.where(val >= 0, want, 0.0)
        p = fetch(part)
        assert all_written(p)
        xhat = (bnx.astype(f64) - bv['mean']) * bv['inv_std']
        gg = h.astype(f64)
        np.testing.assert_allclose(p.astype(f64).sum(axis=2)[0], gg.sum(0), rtol=0, atol=2e-5 * np.abs(gg).sum(0).max())
        np.testing.assert_allclose(p.astype(f64).sum(axis=2)[1], (gg * xhat).sum(0), rtol=0, atol=2e-5 * np.abs(gg * xhat).sum(0).max())
        gemm_check(np.where(safe, h, 0), np.where(safe, want, 0), K, 8)
    else:
        gemm_check(h, want, K, 8)
    g.check()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('which', ['A', 'B'])
@pytest.mark.parametrize('case', [VARIANT_CASES[3], VARIANT_CASES[5], VARIANT_CASES[7]], ids=lambda c: 'v%d' % c[0])
def test_gemm_variants_refuse_a_misaligned_operand(backend, case, which):
    """Variants 2-4 have no scalar operand loads: A or B four bytes off is DPP_E_UNSUPPORTED (dpp_gemm_variant_rows says 0), nothing launched."""
    rt = get_runtime(backend)
    variant, tile, M, N, K, rows = case
    rng = np.random.RandomState(3)
    g = Guards(rt)
    Y = g.out((M, N), name='Y')
    launch = ops.gemm(rt, g.inp(rng.normal(size=(M, K)), name='X', off=int(which == 'A')), g.inp(rng.normal(size=(N, K)), name='W', off=int(which == 'B')),
                      Y, M, N, K, 1, 1, K, K, N, tile=tile, variant=variant)
    assert ops.gemm_variant_rows(rt, launch) == 0
    with pytest.raises(DppError, match='10002'):
        launch(rt.stream)
    rt.synchronize()
    assert untouched(fetch(Y))
    g.check()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('cfg', [(64, 256, 96, 32), (32, 128, 128, 64), (16, 64, 256, 128)], ids=lambda c: 'x'.join(map(str, c)))
def test_expand_kernel_operand_through_batchnorm_backward(backend, cfg):
    """The mode-4 operand on variant 4 with the BatchNorm-backward epilogue of the block input: the operand it forms is left in actA.out,
    guarded like G, the BatchNorm input x2 and the per-channel constants."""
    rt = get_runtime(backend)
    K, N, M, rpw = cfg
    rng = np.random.RandomState(78)
    Gm, Xm = rng.normal(size=(M, K)).astype(f32), (rng.normal(size=(M, K)) * 2 + 5).astype(f32)
    mean = Xm.mean(0).astype(f32)
    istd = (1 / np.sqrt(Xm.var(0) + 1e-4)).astype(f32)
    scale = (rng.uniform(0.5, 1.5, K) * istd).astype(f32)
    c1, c2 = rng.normal(size=K).astype(f32) * 0.1, rng.normal(size=K).astype(f32) * 0.1
    dX = scale.astype(f64) * (Gm.astype(f64) - c1 - (Xm.astype(f64) - mean) * istd * c2)
    Wm, share, bnx = (rng.normal(size=(K, N)) * 0.3).astype(f32), rng.normal(size=(M, N)).astype(f32), rng.normal(size=(M, N)).astype(f32)
    g = Guards(rt)
    bn = _BN()
    bn.mean, bn.inv_std, bn.scale = g.inp(mean, name='mean'), g.inp(istd, name='inv_std'), g.inp(scale, name='scale')
    q, p = g.inp(scale * c1, name='q'), g.inp(scale * istd * c2, name='p')
    eb, ev = _bn_object(g, rng, N)
    copy, out = g.out((M, K), name='actA.out'), g.out((M, N), name='out', init=share)
    part = g.out((2, N, M // rpw), name='bn_partial')
    launch = ops.gemm(rt, g.inp(Gm, name='G'), g.inp(Wm, name='W'), out, M, N, K, 1, 0, K, N, N,
                      actA=ops.act_bn_bwd(bn, q, p, g.inp(Xm, name='x2'), K, out=copy), residual=out, tile=(rpw, 64, 4), variant=4,
                      epi=ops.epilogue(bn=eb, bn_x=g.inp(bnx, name='bn_x'), bn_relu=True, bn_partial=part))
    assert ops.gemm_variant_rows(rt, launch) == rpw
    launch(rt.stream)
    rt.synchronize()
    val = (bnx.astype(f64) - ev['mean']) * ev['scale'] + ev['beta_buf']
    safe = np.abs(val) > 1e-4                         # the mask is decided on the device's own float32 value
    ref = np.where(val >= 0, share.astype(f64) + dX @ Wm.astype(f64), 0.0)
    o, c, pp = fetch(out), fetch(copy), fetch(part)
    assert all_written(o) and all_written(c) and all_written(pp)
    np.testing.assert_allclose(c, dX, rtol=0, atol=2e-6 * np.abs(dX).max())
    np.testing.assert_allclose(o[safe], ref[safe], rtol=0, atol=2e-5 * np.abs(ref).max())
    np.testing.assert_allclose(pp.astype(f64).sum(axis=2)[0], o.astype(f64).sum(0), rtol=0, atol=2e-5 * np.abs(ref).sum(0).max())
    g.check()


# ======================================================================================================================
# dpp_fc_gemm (the weight-streaming kernels)
# ======================================================================================================================
FC_SHAPES = [(40, 72, 200, 1, 0, 'act+bias+res'), (200, 132, 96, 1, 32, 'relu'), (16, 8, 64, 2, 0, 'act'), (128, 192, 96, 1, 0, 'act+bias+res'),
             (256, 64, 256, 2, 0, 'relu')]
FC_LAYOUTS = {'fwd': (1, 0), 'dgrad': (1, 1), 'wgrad': (0, 0), 'tn': (0, 1)}


def _fc_case(rt, shape, layout_, precision, pad, offs=(), expect=None):
    """One guarded dpp_fc_gemm launch against float64 (bf16: on bf16-rounded operands, twice the tolerance); expect = a status string:
    the launch must be refused with it and leave every buffer as it was."""
    M, N, K, splitk, kchunk, feats = shape
    a_kc, b_kc = FC_LAYOUTS[layout_]
    rng = np.random.RandomState(17 + precision + M)
    A = rng.normal(0, 1, (M, K)).astype(f32)
    Bm = rng.normal(0, 1, (N, K)).astype(f32)
    cmod = K if a_kc else M
    g = Guards(rt)
    actA, Aact = None, A.astype(f64)
    if 'act' in feats and cmod % 4 == 0:
        coef = [_vec(rng, cmod), _vec(rng, cmod, 'scale'), _vec(rng, cmod)]
        cb = [g.inp(c, name='act %d' % i, off=int('act' in offs)) for i, c in enumerate(coef)]
        actA = ops.act(Act.BN_RELU, cb[0], cb[1], cb[2], cmod)
        c = coef if a_kc else [k[:, None] for k in coef]
        Aact = np.maximum(((A - c[0]) * c[1] + c[2]).astype(f32), 0).astype(f64)
    elif 'relu' in feats:
        actA = ops.act(Act.RELU, None, None, None, cmod)
        Aact = np.maximum(A, 0).astype(f64)
    Bq = Bm.astype(f64)
    if precision == 1:
        Aact, Bq = _bf16(Aact.astype(f32)), _bf16(Bm)
    want = Aact @ Bq.T
    dA, lda = _operand(g, A, a_kc, pad, int('A' in offs), 'A')
    dB, ldb = _operand(g, Bm, b_kc, pad, int('B' in offs), 'B')
    bias = rng.normal(0, 1, N).astype(f32) if 'bias' in feats and splitk == 1 else None
    res = rng.normal(0, 1, (M, N)).astype(f32) if 'res' in feats and splitk == 1 else None
    ldc = N + pad
    if splitk > 1:
        out = g.out((splitk, M * N), name='partial', off=int('C' in offs))
    else:
        out = g.out((M, ldc), name='C', off=int('C' in offs), init=padded(res, ldc) if res is not None else None)
    before = fetch(out).view(np.uint32).copy()
    launch = ops.fc_gemm(rt, dA, dB, out if splitk == 1 else None, M, N, K, a_kc, b_kc, lda, ldb, ldc, actA=actA,
                         bias=g.inp(bias, name='bias', off=int('bias' in offs)) if bias is not None else None,
                         residual=out if res is not None else None, splitk=splitk, partial=out if splitk > 1 else None, precision=precision, kchunk=kchunk)
    if expect is not None:
        with pytest.raises(DppError, match=expect):
            launch(rt.stream)
        rt.synchronize()
        assert np.array_equal(fetch(out).view(np.uint32), before)
        g.check()
        return
    launch(rt.stream)
    rt.synchronize()
    o = fetch(out)
    if splitk > 1:
        assert all_written(o)
        got = o.astype(f64).sum(axis=0).reshape(M, N)
    else:
        assert all_written(o[:, :N]) and untouched(o[:, N:])
        got = o[:, :N].astype(f64)
        want = want + (bias if bias is not None else 0) + (res if res is not None else 0)
    tol = 6e-7 * (np.sqrt(K) + 4) * max(1.0, float(np.abs(Aact).max()) * float(np.abs(Bq).max()))
    if precision == 1:
        tol *= 2        # v_mfma_f32_16x16x32_bf16 adds the 32 products of a k-step in its own order before the f32 accumulate
    assert np.abs(got - want).max() < tol, (layout_, precision, shape, np.abs(got - want).max(), tol)
    g.check()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('precision', [0, 1], ids=['f32', 'bf16'])
@pytest.mark.parametrize('layout_', list(FC_LAYOUTS))
def test_fc_gemm_layouts_precisions_and_padding(backend, layout_, precision):
    rt = get_runtime(backend)
    for shape in FC_SHAPES:
        for pad in (0, 4):
            _fc_case(rt, shape, layout_, precision, pad)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('layout_', list(FC_LAYOUTS))
@pytest.mark.parametrize('which', ['A', 'B'])
def test_fc_gemm_misaligned_operand_takes_the_scalar_loads(backend, layout_, which):
    """A or B four bytes off: fs_accepts declines the three-stage kernel (the 128-row shape would otherwise take it) and fc_gemm_kernel loads
    that operand one float at a time (vecA / vecB = false)."""
    rt = get_runtime(backend)
    for shape in (FC_SHAPES[2], FC_SHAPES[3]):
        for precision in (0, 1):
            _fc_case(rt, shape, layout_, precision, 4, offs=(which,))


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('which', ['C', 'bias'])
def test_fc_gemm_refuses_a_misaligned_output_or_bias(backend, which):
    """C (and the residual aliasing it), the split-K partial and bias only have 16-byte accesses: DPP_E_UNSUPPORTED, nothing launched."""
    rt = get_runtime(backend)
    for shape in (FC_SHAPES[0], FC_SHAPES[2]) if which == 'C' else (FC_SHAPES[0],):
        _fc_case(rt, shape, 'fwd', 0, 4, offs=(which,), expect='10002')


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('precision', [0, 1], ids=['f32', 'bf16'])
def test_fc_gemm_refuses_misaligned_prologue_vectors(backend, precision):
    """fs_accepts declines the three-stage kernel for them, and fc_gemm_kernel's prologue (dpp_act4) loads them 16 bytes at a time as well:
    dpp_fc_gemm answers DPP_E_BADARG like dpp_gemm, nothing launched -- on the ragged shape and on the 128-row one."""
    rt = get_runtime(backend)
    for shape in (FC_SHAPES[0], FC_SHAPES[3]):
        _fc_case(rt, shape, 'fwd', precision, 4, offs=('act',), expect='10001')


# ======================================================================================================================
# dpp_conv3x3 (+ _bf16, the tile-walking form) and dpp_conv3x3_stream
# ======================================================================================================================
C3_SHAPES = [(3, 8, 8, 16, 16, 64), (2, 6, 10, 16, 32, 128), (3, 5, 12, 64, 64, 64), (1, 7, 19, 32, 16, 64), (2, 8, 16, 32, 32, 0)]


def _bf16(a):
    """Round-to-nearest-even to bfloat16 (returned as float64): what the bf16 kernels do to an operand when they stage it."""
    u = np.ascontiguousarray(a, f32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(f32).astype(f64)


def _c3_inputs(cfg, seed=11):
    N, H, W, Ci, Co, bm = cfg
    rng = np.random.RandomState(seed)
    v = dict(x=rng.normal(size=(N, Ci, H, W)).astype(f32), Wr=(rng.normal(size=(Co, Ci, 3, 3)) * 0.2).astype(f32), b=rng.normal(size=Co).astype(f32),
             coef=[_vec(rng, Ci), _vec(rng, Ci, 'scale'), _vec(rng, Ci)], res=rng.normal(size=(N, Co, H, W)).astype(f32),
             dy=rng.normal(size=(N, Co, H, W)).astype(f32), bnx=(rng.normal(size=(N, H, W, Ci)) + 0.5).astype(f32))
    c = [k[None, :, None, None] for k in v['coef']]
    v['a32'] = np.maximum((v['x'] - c[0]) * c[1] + c[2], f32(0))             # the kernel's float32 prologue (bf16 rounds AFTER it)
    v['a'] = np.maximum((v['x'].astype(f64) - c[0]) * c[1] + c[2], 0)
    return v, rng


def _c3_forward_and_dgrad(rt, cfg, precision, off=None):
    """Forward (BatchNorm + ReLU prologue, bias, residual aliasing the output) and data gradient (mirrored weights, BatchNorm-backward
    epilogue) of one shape, every operand guarded.  off: the name of ONE operand to move by an element."""
    N, H, W, Ci, Co, bm = cfg
    v, rng = _c3_inputs(cfg)
    q = _bf16 if precision else (lambda a: np.asarray(a, f64))
    o = lambda name: int(off == name)                                            # noqa: E731
    g = Guards(rt)
    X = g.inp(layout.nchw_to_nhwc(v['x']), name='X', off=o('X'))
    Wk = g.inp(layout.conv_w_to_kernel(v['Wr']), name='Wk', off=o('Wk'))
    cb = [g.inp(c, name='act %d' % i, off=o('act')) for i, c in enumerate(v['coef'])]
    bias = g.inp(v['b'], name='bias', off=o('bias'))
    Y = g.out((N, H, W, Co), name='Y', off=o('Y'), init=layout.nchw_to_nhwc(v['res']))
    act = ops.act(Act.BN_RELU, cb[0], cb[1], cb[2], Ci)
    ops.conv3x3(rt, X, N, H, W, Ci, Wk, Co, Y, actX=act, bias=bias, residual=Y, bm=bm, precision=precision)(rt.stream)
    rt.synchronize()
    y_ref = L.conv2d_fwd(q(v['a32']) if precision else v['a'], q(v['Wr']), v['b'].astype(f64), (1, 1), 'half') + v['res']
    y = fetch(Y)
    assert all_written(y)
    np.testing.assert_allclose(layout.nhwc_to_nchw(y), y_ref, rtol=0, atol=3e-6 * np.sqrt(9 * Ci) * np.abs(y_ref).max())
    g.check()
    # data gradient = the same kernel on dY with the transposed / mirrored weights; G = dA * [bn(bn_x) >= 0], per-tile (sum G, sum G xhat)
    g = Guards(rt)
    Wk = g.inp(layout.conv_w_to_kernel(v['Wr']), name='Wk')
    Wd = g.out((Ci, 9, Co), name='Wd', off=o('Wd'))
    ops.conv3x3_wtrans(rt, Wk, Co, Ci, Wd)(rt.stream)
    rt.synchronize()
    assert all_written(fetch(Wd))
    bn, bv = _bn_object(g, rng, Ci, off='mean' if off == 'bn' else None)
    bm_eff = bm or 64                                   # (every shape here is far below the 512 workgroups that choose 128 rows)
    nblk = rt.lib.dpp_conv3x3_tiling(N, H, W, bm_eff, None, None, None)
    dYb = g.inp(layout.nchw_to_nhwc(v['dy']), name='dY', off=o('dY'))
    bnx = g.inp(v['bnx'], name='bn_x', off=o('bn_x'))
    G = g.out((N, H, W, Ci), name='G', off=o('G'))
    part = g.out((2, Ci, nblk), name='bn_partial')
    ops.conv3x3(rt, dYb, N, H, W, Co, Wd, Ci, G, bm=bm_eff, precision=precision,
                epi=ops.epilogue(bn=bn, bn_x=bnx, bn_relu=True, bn_partial=part))(rt.stream)
    rt.synchronize()
    da_ref = layout.nchw_to_nhwc(L.conv2d_bwd(np.zeros((N, Ci, H, W)), q(v['Wr']), q(v['dy']), (1, 1), 'half')[0])
    val = (v['bnx'].astype(f64) - bv['mean']) * bv['scale'] + bv['beta_buf']
    safe = np.abs(val) > 1e-4
    got = fetch(G)
    assert all_written(got) and all_written(fetch(part))
    np.testing.assert_allclose(got[safe], (da_ref * (val >= 0))[safe], rtol=0, atol=3e-6 * np.sqrt(9 * Co) * np.abs(da_ref).max())
    p = fetch(part).astype(f64).sum(axis=2)
    xhat = (v['bnx'].astype(f64) - bv['mean']) * bv['inv_std']
    M = N * H * W
    gg = got.astype(f64).reshape(M, Ci)
    np.testing.assert_allclose(p[0], gg.sum(0), rtol=0, atol=3e-5 * np.sqrt(M) * np.abs(got).max())
    np.testing.assert_allclose(p[1], (gg * xhat.reshape(M, Ci)).sum(0), rtol=0, atol=3e-4 * np.sqrt(M) * np.abs(got).max())
    g.check()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('precision', [0, 1], ids=['f32', 'bf16'])
@pytest.mark.parametrize('cfg', C3_SHAPES, ids=lambda c: 'x'.join(map(str, c)))
def test_conv3x3_forward_and_data_gradient(backend, cfg, precision):
    _c3_forward_and_dgrad(get_runtime(backend), cfg, precision)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('cfg', [(3, 8, 8, 16, 16, 64), (2, 8, 16, 32, 32, 128), (2, 16, 32, 16, 16, 128)], ids=lambda c: 'x'.join(map(str, c)))
def test_conv3x3_statistics_epilogue_one_tile_and_walking(backend, cfg, monkeypatch, capfd):
    """The statistics epilogue on maps of whole tiles (what dpp_bn_finalize can combine), on the one-tile kernel (DPP_C3_PERSIST = 0) and, for
    the two shapes conv3x3_launch lets walk (bm = 128, Ci = Co, 8 x 16 tiles that divide the map), with one and three workgroups walking
    the tiles; DPP_C3_PERSIST_VERBOSE makes the dispatch say when it takes conv3x3_p_kernel, which is asserted."""
    rt = get_runtime(backend)
    N, H, W, Ci, Co, bm = cfg
    v, rng = _c3_inputs(cfg, seed=41)
    M = N * H * W
    nblk = rt.lib.dpp_conv3x3_tiling(N, H, W, bm, None, None, None)
    y_ref = layout.nchw_to_nhwc(L.conv2d_fwd(v['a'], v['Wr'].astype(f64), v['b'].astype(f64), (1, 1), 'half')).reshape(M, Co)
    monkeypatch.setenv('DPP_C3_PERSIST_VERBOSE', '1')
    for mode in (('0', '1', '3') if bm == 128 else ('0',)):
        monkeypatch.setenv('DPP_C3_PERSIST', mode)
        capfd.readouterr()
        g = Guards(rt)
        cb = [g.inp(c, name='act %d' % i) for i, c in enumerate(v['coef'])]
        Y, stats = g.out((M, Co), name='Y'), g.out((2, Co, nblk), name='stats')
        ops.conv3x3(rt, g.inp(layout.nchw_to_nhwc(v['x']), name='X'), N, H, W, Ci, g.inp(layout.conv_w_to_kernel(v['Wr']), name='Wk'), Co, Y,
                    actX=ops.act(Act.BN_RELU, cb[0], cb[1], cb[2], Ci), bias=g.inp(v['b'], name='bias'), bm=bm, epi=ops.epilogue(stats=stats))(rt.stream)
        mean, istd, scale = (g.out((Co,), name=n) for n in ('mean', 'inv_std', 'scale'))
        ops.bn_finalize(rt, stats, nblk, M, bm, Co, g.inp(np.ones(Co, f32)), 1e-4, mean, istd, scale)(rt.stream)
        rt.synchronize()
        assert capfd.readouterr().err.count('conv3x3_p_kernel') == (0 if mode == '0' else 1)
        y = fetch(Y)
        assert all_written(y) and all_written(fetch(stats))
        np.testing.assert_allclose(y, y_ref, rtol=0, atol=3e-6 * np.sqrt(9 * Ci) * np.abs(y_ref).max())
        np.testing.assert_allclose(fetch(mean), y_ref.mean(0), rtol=0, atol=3e-6 * np.abs(y_ref).max())
        np.testing.assert_allclose(fetch(istd), 1 / np.sqrt(y_ref.var(0) + f32(1e-4)), rtol=3e-5)
        g.check()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('which', ['Y', 'bias', 'G', 'bn_x', 'bn'])
def test_conv3x3_misaligned_epilogue_operand_takes_the_narrow_epilogue(backend, which):
    """Y (with the residual that aliases it), bias, the data gradient's output, bn_x or a BatchNorm vector four bytes off: conv3x3_launch
    clears a.wide and the kernel stores one float at a time -- the only way into that epilogue, since Co % 16 == 0 always holds."""
    _c3_forward_and_dgrad(get_runtime(backend), C3_SHAPES[0], 0, off=which)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('precision', [0, 1], ids=['f32', 'bf16'])
@pytest.mark.parametrize('which', ['X', 'Wk', 'act'])
def test_conv3x3_refuses_a_misaligned_input_map_filter_or_prologue_vector(backend, which, precision):
    """X, Wk and the prologue vectors are only ever loaded 16 bytes at a time: DPP_E_BADARG, nothing launched."""
    rt = get_runtime(backend)
    N, H, W, Ci, Co, bm = C3_SHAPES[0]
    v, rng = _c3_inputs(C3_SHAPES[0])
    g = Guards(rt)
    X = g.inp(layout.nchw_to_nhwc(v['x']), name='X', off=int(which == 'X'))
    Wk = g.inp(layout.conv_w_to_kernel(v['Wr']), name='Wk', off=int(which == 'Wk'))
    cb = [g.inp(c, off=int(which == 'act' and i == 1)) for i, c in enumerate(v['coef'])]
    Y = g.out((N, H, W, Co), name='Y')
    with pytest.raises(DppError, match='10001'):
        ops.conv3x3(rt, X, N, H, W, Ci, Wk, Co, Y, actX=ops.act(Act.BN_RELU, cb[0], cb[1], cb[2], Ci), bm=bm, precision=precision)(rt.stream)
    rt.synchronize()
    assert untouched(fetch(Y))
    g.check()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('precision', [0, 1], ids=['f32', 'bf16'])
@pytest.mark.parametrize('cfg', [(3, 16, 32, 16), (3, 16, 16, 32), (2, 8, 16, 32), (7, 8, 8, 64)], ids=lambda c: 'x'.join(map(str, c)))
def test_conv3x3_walking_forward_and_data_gradient(backend, cfg, precision, monkeypatch, capfd):
    """conv3x3_p_kernel between bands: 128-row launches on maps of whole 8 x 16 tiles (16 and 32 channels) and on 8 x 8 maps of 64 channels
    (two images per tile, seven images: a ragged last tile), one and three workgroups walking the tiles -- forward with prologue, bias and
    the residual aliasing the output, data gradient with the bn_x epilogue, float32 and bf16 operands.  The dispatch reports the walk
    (DPP_C3_PERSIST_VERBOSE): both launches of each run must have taken it."""
    rt = get_runtime(backend)
    monkeypatch.setenv('DPP_C3_P_64', '2')            # (the 64-channel form in float32 as well: off by default)
    monkeypatch.setenv('DPP_C3_PERSIST_VERBOSE', '1')
    N, H, W, Cc = cfg
    for mode in ('1', '3'):
        monkeypatch.setenv('DPP_C3_PERSIST', mode)
        capfd.readouterr()
        _c3_forward_and_dgrad(rt, (N, H, W, Cc, Cc, 128), precision)
        assert capfd.readouterr().err.count('conv3x3_p_kernel') == 2


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('which', ['X', 'dY', 'act'])
def test_conv3x3_wgrad_refuses_misaligned_inputs(backend, which):
    """dpp_conv3x3_wgrad stages X, dY and the prologue vectors four channels at a time: one of them four bytes off is DPP_E_BADARG with
    nothing launched."""
    _c3_wgrad_alignment(get_runtime(backend), which)


@pytest.mark.parametrize('backend', BACKENDS[:1])
def test_conv3x3_wgrad_tolerates_four_byte_aligned_partials(backend):
    """The partials are stored float by float (include/dpp_hip.h): four bytes off they are as good as aligned.  Emulator only."""
    _c3_wgrad_alignment(get_runtime(backend), 'partial')


def _c3_wgrad_alignment(rt, which):
    N, H, W, Cc = 1, 8, 16, 16
    v, rng = _c3_inputs((N, H, W, Cc, Cc, 0), seed=19)
    o = lambda name: int(which == name)                                            # noqa: E731
    for bm in (64, 128):
        g = Guards(rt)
        cb = [g.inp(c, name='act %d' % i, off=int(which == 'act' and i == 2)) for i, c in enumerate(v['coef'])]
        nblk = rt.lib.dpp_conv3x3_wgrad_blocks(N, H, W, Cc, Cc, bm)
        part = g.out((nblk, Cc * 9 * Cc), name='partial', off=o('partial'))
        launch = ops.conv3x3_wgrad(rt, g.inp(layout.nchw_to_nhwc(v['x']), name='X', off=o('X')), N, H, W, Cc,
                                   g.inp(layout.nchw_to_nhwc(v['dy']), name='dY', off=o('dY')), Cc, part, actX=ops.act(Act.BN_RELU, cb[0], cb[1], cb[2], Cc), bm=bm)
        if which != 'partial':
            with pytest.raises(DppError, match='10001'):
                launch(rt.stream)
            rt.synchronize()
            assert untouched(fetch(part))
        else:
            launch(rt.stream)
            rt.synchronize()
            p = fetch(part)
            assert all_written(p)
            _, dW_ref, _ = L.conv2d_bwd(v['a'], np.zeros((Cc, Cc, 3, 3)), v['dy'].astype(f64), (1, 1), 'half')
            dW = layout.conv_w_from_kernel(p.astype(f64).sum(axis=0).reshape(Cc, 9, Cc), (Cc, Cc, 3, 3))
            np.testing.assert_allclose(dW, dW_ref, rtol=0, atol=3e-6 * np.sqrt(N * H * W) * np.abs(dW_ref).max())
        g.check()


C3S_SHAPES = [(2, 8, 16, 32), (2, 8, 16, 16), (1, 6, 32, 16), (4, 16, 16, 32)]          # the one stream-shaped map of C3_SHAPES, and three of the kernel's own test


def _c3s_launch(rt, g, v, cfg, off=None):
    N, H, W, Cc = cfg
    o = lambda name: int(off == name)                                            # noqa: E731
    cb = [g.inp(c, name='act %d' % i, off=o('act')) for i, c in enumerate(v['coef'])]
    Y, rows = g.out((N, H, W, Cc), name='Y', off=o('Y')), rt.lib.dpp_conv3x3_stream_rows(N, H, W, Cc)
    stats = g.out((2, Cc, max(1, N * H * W // max(rows, 1))), name='stats', off=o('stats'))
    L_ = ops.conv3x3_stream(rt, g.inp(layout.nchw_to_nhwc(v['x']), name='X', off=o('X')), N, H, W, Cc, g.inp(layout.conv_w_to_kernel(v['Wr']), name='Wk', off=o('Wk')),
                            Y, actX=ops.act(Act.BN_RELU, cb[0], cb[1], cb[2], Cc), bias=g.inp(v['b'], name='bias', off=o('bias')), epi=ops.epilogue(stats=stats))
    return L_, Y, stats, rows


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('cfg', C3S_SHAPES, ids=lambda c: 'x'.join(map(str, c)))
def test_conv3x3_stream_forward_and_data_gradient(backend, cfg):
    _c3s_case(get_runtime(backend), cfg)


@pytest.mark.parametrize('backend', BACKENDS[:1])
@pytest.mark.parametrize('which', ['Y', 'bias', 'stats'])
def test_conv3x3_stream_tolerates_four_byte_alignment_of_what_it_writes_and_of_bias(backend, which):
    """conv3x3_stream_kernel accesses Y, bias and the epilogue's buffers one float at a time (include/dpp_hip.h says so): emulator only."""
    _c3s_case(get_runtime(backend), C3S_SHAPES[0], off=which)


def _c3s_case(rt, cfg, off=None):
    N, H, W, Cc = cfg
    M = N * H * W
    v, rng = _c3_inputs((N, H, W, Cc, Cc, 0), seed=71)
    g = Guards(rt)
    launch, Y, stats, rows = _c3s_launch(rt, g, v, cfg, off=off)
    assert rows in (64, 128) and M % rows == 0
    launch(rt.stream)
    mean, istd, scale = (g.out((Cc,), name=n) for n in ('mean', 'inv_std', 'scale'))
    ops.bn_finalize(rt, stats, M // rows, M, rows, Cc, g.inp(np.ones(Cc, f32)), 1e-4, mean, istd, scale)(rt.stream)
    rt.synchronize()
    y_ref = layout.nchw_to_nhwc(L.conv2d_fwd(v['a'], v['Wr'].astype(f64), v['b'].astype(f64), (1, 1), 'half'))
    y = fetch(Y)
    assert all_written(y) and all_written(fetch(stats))
    np.testing.assert_allclose(y, y_ref, rtol=0, atol=3e-6 * np.sqrt(9 * Cc) * np.abs(y_ref).max())
    yv = y.astype(f64).reshape(M, Cc)
    np.testing.assert_allclose(fetch(mean), yv.mean(0), rtol=0, atol=1e-6 * np.abs(yv).max())
    np.testing.assert_allclose(fetch(istd), 1 / np.sqrt(yv.var(0) + f32(1e-4)), rtol=1e-5)
    g.check()
    # data gradient: the same kernel on dY with the mirrored weights, BatchNorm-backward epilogue
    g = Guards(rt)
    Wd = g.out((Cc, 9, Cc), name='Wd')
    ops.conv3x3_wtrans(rt, g.inp(layout.conv_w_to_kernel(v['Wr']), name='Wk'), Cc, Cc, Wd)(rt.stream)
    bn, bv = _bn_object(g, rng, Cc)
    G, part = g.out((M, Cc), name='G'), g.out((2, Cc, M // rows), name='bn_partial')
    ops.conv3x3_stream(rt, g.inp(layout.nchw_to_nhwc(v['dy']), name='dY'), N, H, W, Cc, Wd, G,
                       epi=ops.epilogue(bn=bn, bn_x=g.inp(v['bnx'], name='bn_x'), bn_relu=True, bn_partial=part))(rt.stream)
    rt.synchronize()
    da_ref = layout.nchw_to_nhwc(L.conv2d_bwd(np.zeros((N, Cc, H, W)), v['Wr'].astype(f64), v['dy'].astype(f64), (1, 1), 'half')[0]).reshape(M, Cc)
    bx = v['bnx'].astype(f64).reshape(M, Cc)
    val = (bx - bv['mean']) * bv['scale'] + bv['beta_buf']
    safe = np.abs(val) > 1e-4
    got = fetch(G)
    assert all_written(got) and all_written(fetch(part)) and all_written(fetch(Wd))
    np.testing.assert_allclose(got[safe], (da_ref * (val >= 0))[safe], rtol=0, atol=3e-6 * np.sqrt(9 * Cc) * np.abs(da_ref).max())
    p = fetch(part).astype(f64).sum(axis=2)
    np.testing.assert_allclose(p[0], got.astype(f64).sum(0), rtol=0, atol=3e-6 * np.sqrt(M) * np.abs(got).max())
    np.testing.assert_allclose(p[1], (got.astype(f64) * (bx - bv['mean']) * bv['inv_std']).sum(0), rtol=0, atol=3e-5 * np.sqrt(M) * np.abs(got).max())
    g.check()


@pytest.mark.parametrize('backend', BACKENDS)
def test_conv3x3_stream_refuses_other_maps_and_misaligned_inputs(backend):
    """The four maps of C3_SHAPES the stream kernel does not take (W % 16, 64 channels, Ci != Co), and X, Wk or a prologue vector four bytes
    off: DPP_E_UNSUPPORTED, nothing launched."""
    rt = get_runtime(backend)
    cases = [((N, H, W, Ci), None) for (N, H, W, Ci, Co, bm) in C3_SHAPES[:4]] + [(C3S_SHAPES[0], w) for w in ('X', 'Wk', 'act')]
    for cfg, off in cases:
        N, H, W, Cc = cfg
        v, rng = _c3_inputs((N, H, W, Cc, Cc, 0), seed=71)
        g = Guards(rt)
        launch, Y, stats, rows = _c3s_launch(rt, g, v, cfg, off=off)
        assert (rows == 0) == (off is None)
        with pytest.raises(DppError, match='10002'):
            launch(rt.stream)
        rt.synchronize()
        assert untouched(fetch(Y)) and untouched(fetch(stats))
        g.check()


# ======================================================================================================================
# filter gradients: dpp_conv3x3_wgrad (+ _bf16), dpp_wgrad3_stream, dpp_wgrad_stream (+ _bf16), dpp_fc_wgrad_stream
# ======================================================================================================================
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('cfg', [(1, 8, 16, 16), (2, 9, 13, 32), (2, 7, 19, 64)], ids=lambda c: 'x'.join(map(str, c)))
def test_conv3x3_filter_gradients(backend, cfg):
    """The LDS-tiled kernels (float32 with and without the prologue, bf16 operands; 64 and 128 rows) and the row stream (8 and 20 rows per
    wave), partials guarded.  The row stream takes whole quads of pixels: on the 13- and 19-wide maps dpp_wgrad3_stream_slices says 0, which
    is asserted, and the kernel runs on the next wider map instead.  A case is skipped only where dpp_conv3x3_wgrad_bf16_ok declines."""
    rt = get_runtime(backend)
    N, H, W0, Cc = cfg
    cases = skipped = 0
    for kind, arg, use_act in (('tiled', 64, True), ('tiled', 128, True), ('tiled', 64, False), ('tiled', 128, False), ('bf16', 64, False), ('bf16', 128, False),
                               ('stream', 8, True), ('stream', 20, True)):
        # (bf16: a float32 prologue here may round to the other bf16 neighbour than the device's FMA -- plain operands there)
        cases += 1
        W = W0
        if kind == 'stream' and W0 % 4:
            assert rt.lib.dpp_wgrad3_stream_slices(Cc, Cc, N, H, W0, arg) == 0
            W = W0 + 4 - W0 % 4                           # the row stream takes whole quads of pixels only: the next wider map
        v, rng = _c3_inputs((N, H, W, Cc, Cc, 0), seed=19)
        px = N * H * W
        if kind == 'stream':
            nblk = rt.lib.dpp_wgrad3_stream_slices(Cc, Cc, N, H, W, arg)
            assert nblk > 0
        else:
            nblk = rt.lib.dpp_conv3x3_wgrad_blocks(N, H, W, Cc, Cc, arg)
        if kind == 'bf16' and not rt.lib.dpp_conv3x3_wgrad_bf16_ok(N, H, W, Cc, Cc):
            skipped += 1
            continue
        g = Guards(rt)
        cb = [g.inp(c, name='act %d' % i) for i, c in enumerate(v['coef'])]
        act = ops.act(Act.BN_RELU, cb[0], cb[1], cb[2], Cc) if use_act else None
        X, dY = g.inp(layout.nchw_to_nhwc(v['x']), name='X'), g.inp(layout.nchw_to_nhwc(v['dy']), name='dY')
        part = g.out((nblk, Cc * 9 * Cc), name='partial')
        if kind == 'stream':
            ops.wgrad3_stream(rt, dY, Cc, X, Cc, N, H, W, arg, part, actX=act)(rt.stream)
        else:
            ops.conv3x3_wgrad(rt, X, N, H, W, Cc, dY, Cc, part, actX=act, bm=arg, precision=int(kind == 'bf16'))(rt.stream)
        rt.synchronize()
        p = fetch(part)
        assert all_written(p)
        q = _bf16 if kind == 'bf16' else (lambda a: np.asarray(a, f64))
        _, dW_ref, _ = L.conv2d_bwd(v['a'] if use_act else q(v['x']), np.zeros((Cc, Cc, 3, 3)), q(v['dy']), (1, 1), 'half')
        dW = layout.conv_w_from_kernel(p.astype(f64).sum(axis=0).reshape(Cc, 9, Cc), (Cc, Cc, 3, 3))
        np.testing.assert_allclose(dW, dW_ref, rtol=0, atol=3e-6 * np.sqrt(px) * np.abs(dW_ref).max())
        g.check()
    assert skipped * 4 <= cases, (skipped, cases)


@pytest.mark.parametrize('backend', BACKENDS)
def test_wgrad_stream_ragged_and_strided(backend):
    """150 rows (a ragged last slice) and the stride-2 row map of a 5 x 7 map, whose skipped rows hold NaN; float32 and bf16 operands (the latter:
    dpp_wgrad_stream_bf16_ok declines 256 x 128, two of the twelve cases of this test)."""
    rt = get_runtime(backend)
    tally = [0, 0]
    for shape in ((16, 64), (64, 16), (256, 128)):
        _wgrad_stream_shape(rt, shape, tally)
    assert tally == [12, 2]


def _wgrad_stream_shape(rt, shape, tally):
    Co, Ci = shape
    rng = np.random.RandomState(Co * 1000 + Ci)
    coef = [_vec(rng, Ci), _vec(rng, Ci, 'scale'), _vec(rng, Ci)]
    for strided in (False, True):
        if strided:
            Nb, Ho, Wo, s = 3, 5, 7, 2
            Hi, Wi = Ho * s, Wo * s
            M, rows = Nb * Ho * Wo, Nb * Hi * Wi + 3
            mp, at = RowMap.strided(s, Ho, Wo, Hi, Wi), _strided_rows(Nb, Ho, Wo, Hi, Wi, s)
        else:
            M = rows = 150
            mp, at = None, np.arange(M)
        dY = rng.normal(size=(M, Co)).astype(f32)
        xv = rng.normal(size=(M, Ci)).astype(f32)
        X = np.full((rows, Ci), NAN, f32)
        X[at] = xv
        nsl = rt.lib.dpp_wgrad_stream_slices(Co, Ci, M, 32)
        assert nsl >= 1
        for precision in (0, 1):
            tally[0] += 1
            if precision and not rt.lib.dpp_wgrad_stream_bf16_ok(Co, Ci):
                tally[1] += 1
                continue
            for mode in ((0, 1) if precision else (0, 3)):        # (bf16: no float32 arithmetic in front of the rounding)
                g = Guards(rt)
                cb = [g.inp(c, name='act %d' % i) for i, c in enumerate(coef)]
                part = g.out((nsl, Co, Ci), name='partial')
                ops.wgrad_stream(rt, g.inp(dY, name='dY'), Co, g.inp(X, name='X'), Ci, M, 32, part, mapX=mp,
                                 actX=ops.act(mode, cb[0], cb[1], cb[2], cmod=Ci) if mode else None, precision=precision)(rt.stream)
                rt.synchronize()
                p = fetch(part)
                assert all_written(p)
                Xa = _bn_relu(xv, coef) if mode == 3 else (np.maximum(xv, 0).astype(f64) if mode == 1 else xv.astype(f64))
                if precision:
                    ref = _bf16(dY).T @ _bf16(Xa)
                    np.testing.assert_allclose(p.astype(f64).sum(axis=0), ref, rtol=0, atol=3e-6 * np.sqrt(M) * np.abs(ref).max())
                else:
                    gemm_check(p.astype(f64).sum(axis=0), dY.astype(f64).T @ Xa, M, 4)
                g.check()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('which', ['dY', 'X', 'partial', 'mean', 'scale', 'beta'])
def test_row_stream_filter_gradients_refuse_misaligned_pointers(backend, which):
    """dpp_wgrad_stream, dpp_wgrad3_stream and dpp_fc_wgrad_stream have 8- and 16-byte accesses only, to the prologue's per-channel vectors
    as well (load_vec, csrc/wgrad.hip): DPP_E_BADARG, nothing launched."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(9)
    o = lambda name: int(which == name)                                            # noqa: E731
    for kind in ('1x1', '3x3', 'fc'):
        g = Guards(rt)
        cm = {'1x1': 64, '3x3': 16, 'fc': 32}[kind]
        cb = [g.inp(_vec(rng, cm, 'scale' if n == 'scale' else 'normal'), name=n, off=o(n)) for n in ('mean', 'scale', 'beta')]
        act = ops.act(Act.BN_RELU, cb[0], cb[1], cb[2], cm)
        if kind == '1x1':
            Co, Ci, M = 16, 64, 150
            part = g.out((rt.lib.dpp_wgrad_stream_slices(Co, Ci, M, 32), Co, Ci), name='partial', off=o('partial'))
            launch = ops.wgrad_stream(rt, g.inp(rng.normal(size=(M, Co)), off=o('dY')), Co, g.inp(rng.normal(size=(M, Ci)), off=o('X')), Ci, M, 32, part, actX=act)
        elif kind == '3x3':
            N, H, W, Cc = 1, 8, 16, 16
            part = g.out((rt.lib.dpp_wgrad3_stream_slices(Cc, Cc, N, H, W, 8), Cc * 9 * Cc), name='partial', off=o('partial'))
            launch = ops.wgrad3_stream(rt, g.inp(rng.normal(size=(N, H, W, Cc)), off=o('dY')), Cc, g.inp(rng.normal(size=(N, H, W, Cc)), off=o('X')), Cc,
                                       N, H, W, 8, part, actX=act)
        else:
            Nb, K, N = 1, 128, 128
            part = g.out((K, N), name='dW', off=o('partial'))
            launch = ops.fc_wgrad_stream(rt, g.inp(rng.normal(size=(Nb, K)), off=o('X')), g.inp(rng.normal(size=(Nb, N)), off=o('dY')), part, Nb, K, N, actX=act)
        with pytest.raises(DppError, match='10001'):
            launch(rt.stream)
        rt.synchronize()
        assert untouched(fetch(part))
        g.check()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('cfg', [(6, 128, 256), (1, 128, 128), (37, 128, 128)], ids=lambda c: 'x'.join(map(str, c)))
def test_fc_wgrad_stream(backend, cfg):
    rt = get_runtime(backend)
    Nb, K, N = cfg
    rng = np.random.RandomState(77)
    X, dY = rng.normal(size=(Nb, K)).astype(f32), rng.normal(size=(Nb, N)).astype(f32)
    cmod = 32
    coef = [_vec(rng, cmod), _vec(rng, cmod, 'scale'), _vec(rng, cmod)]
    ch = np.arange(K) % cmod
    for with_act in (True, False):
        g = Guards(rt)
        cb = [g.inp(c, name='act %d' % i) for i, c in enumerate(coef)]
        dW = g.out((K, N), name='dW')
        ops.fc_wgrad_stream(rt, g.inp(X, name='X'), g.inp(dY, name='dY'), dW, Nb, K, N,
                            actX=ops.act(Act.BN_RELU, cb[0], cb[1], cb[2], cmod) if with_act else None)(rt.stream)
        rt.synchronize()
        A = _bn_relu(X, [c[ch] for c in coef]) if with_act else X.astype(f64)
        ref = A.T @ dY.astype(f64)
        w = fetch(dW)
        assert all_written(w)
        np.testing.assert_allclose(w, ref, rtol=0, atol=3e-6 * np.sqrt(Nb) * np.abs(ref).max())
        g.check()


# ======================================================================================================================
# the stem (dpp_stem_fwd / dpp_stem_wgrad) and the generic ConvPoolLayer kernels
# ======================================================================================================================
def _stem_case(rt, cfg, off=None):
    N, H, W, Co = cfg
    rng = np.random.RandomState(12)
    o = lambda name: int(off == name)                                            # noqa: E731
    x = rng.uniform(-1, 1, size=(N, 1, H, W))
    x[:, :, :, W // 2:] = 1.0                        # constant far-plane background: whole pooling windows tie
    Wr = rng.normal(size=(Co, 1, 5, 5)) * 0.3
    b = rng.normal(size=Co)
    y_ref, cache = L.convpool_fwd(x, Wr, b, (1, 1), 'half', (2, 2), False)
    g = Guards(rt)
    X, Wk, bias = g.inp(x[:, 0], name='X'), g.inp(layout.conv_w_to_kernel(Wr).reshape(Co, 25), name='Wk'), g.inp(b, name='bias')
    Y = g.out((N, H // 2, W // 2, Co), name='Y')
    arg = g.out((N, H // 2, W // 2, Co), np.uint8, name='argmax', off=o('argmax'))
    full = H % 16 == 0 and W % 16 == 0                 # the fused BatchNorm statistics need full 16x16 conv tiles
    nblk_s = N * (H // 16) * (W // 16)
    stats = g.out((2, Co, nblk_s), name='stats') if full else None
    ops.stem_fwd(rt, X, N, H, W, Wk, bias, Co, Y, arg, stats)(rt.stream)
    rt.synchronize()
    y, bits_ = fetch(Y), fetch(arg)
    assert all_written(y) and bits_.max() < 16              # (a tie mask of four bits: no byte of the sentinel is one)
    np.testing.assert_allclose(layout.nhwc_to_nchw(y), y_ref, rtol=0, atol=3e-6 * 5 * np.abs(y_ref).max())
    if full:
        M = N * (H // 2) * (W // 2)
        mean, istd, scale = (g.out((Co,), name=n) for n in ('mean', 'inv_std', 'scale'))
        ops.bn_finalize(rt, stats, nblk_s, M, 64, Co, g.inp(np.ones(Co, f32)), 1e-4, mean, istd, scale)(rt.stream)
        rt.synchronize()
        yv = y.astype(f64).reshape(M, Co)
        assert all_written(fetch(stats))
        np.testing.assert_allclose(fetch(mean), yv.mean(0), rtol=0, atol=1e-6 * np.abs(yv).max())
        np.testing.assert_allclose(fetch(istd), 1.0 / np.sqrt(yv.var(0) + 1e-4), rtol=1e-5)
    # the tie mask agrees with the oracle wherever the oracle's window is either clearly decided or exactly tied
    cshape, ties_ref, _ = cache
    c = L.conv2d_fwd(x, Wr, None, (1, 1), 'half')
    cv = c.reshape(N, Co, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, Co, H // 2, W // 2, 4)
    gap = cv.max(axis=4, keepdims=True) - cv
    clear = ((gap == 0) | (gap > 1e-4)).all(axis=4)
    got = ((layout.nhwc_to_nchw(bits_)[..., None] >> np.arange(4)) & 1).astype(bool)
    assert clear.mean() > 0.9 and (got[clear] == ties_ref[clear]).all()
    g.check()
    # filter gradient with the device's own tie mask
    g2 = Guards(rt)
    dy = rng.normal(size=y_ref.shape)
    tpb = 2
    nblk = rt.lib.dpp_stem_wgrad_blocks(N, H, W, tpb)
    part = g2.out((nblk, Co * 25), name='partial')
    ops.stem_wgrad(rt, g2.inp(x[:, 0], name='X'), N, H, W, g2.inp(layout.nchw_to_nhwc(dy), name='dY', off=o('dY')), arg, Co, part, tpb)(rt.stream)
    rt.synchronize()
    p = fetch(part)
    assert all_written(p)
    _, dW_ref, _ = L.convpool_bwd(x, Wr, dy, (cshape, got, y_ref), (1, 1), 'half', (2, 2), False, need_dx=False)
    dW = layout.conv_w_from_kernel(p.astype(f64).sum(axis=0).reshape(Co, 25, 1), (Co, 1, 5, 5))
    np.testing.assert_allclose(dW, dW_ref, rtol=0, atol=3e-6 * np.sqrt(N * H * W / 4) * np.abs(dW_ref).max())
    g2.check()
    g.check()                                        # (the tie mask is an input of the second launch)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('cfg', [(1, 36, 20, 16), (1, 32, 16, 30), (2, 16, 16, 24)], ids=lambda c: 'x'.join(map(str, c)))
def test_stem_forward_and_filter_gradient(backend, cfg):
    _stem_case(get_runtime(backend), cfg)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('which', ['dY', 'argmax'])
def test_stem_filter_gradient_misaligned_takes_the_scalar_loads(backend, which):
    """stem_wgrad_kernel reads four channels of dY (16 bytes) and of the tie mask (4 bytes) at once only when both pointers allow it
    (`vec`, csrc/stem.hip): dY one float off, or the mask one byte off, and it loads them element by element."""
    _stem_case(get_runtime(backend), (2, 16, 16, 24), off=which)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('cfg', [(3, 31, 31, 8, 8, 5, 'valid', 2), (2, 20, 18, 3, 12, 3, 'half', 3), (2, 30, 22, 12, 8, 5, 'half', 2)],
                         ids=lambda c: 'x'.join(map(str, c)))
def test_convpool_forward_and_gradients(backend, cfg):
    _convpool_case(get_runtime(backend), cfg)


def _convpool_case(rt, cfg, off=None):
    N, H, W, Ci, Co, k, border, pool = cfg
    o = lambda name: int(off == name)                                            # noqa: E731
    pad = k // 2 if border == 'half' else 0
    rng = np.random.RandomState(31)
    pre = rng.uniform(-1, 1, size=(N, Ci, H, W))
    pre[:, :, :, W // 2:] = 0.75                       # constant region: conv output ties inside whole pooling windows
    x = np.maximum(pre, 0)                             # the previous layer's ReLU is this layer's operand prologue
    Wr = rng.normal(size=(Co, Ci, k, k)) * 0.3
    b = rng.normal(size=Co)
    y_ref, cache = L.convpool_fwd(x, Wr, b, (1, 1), border, (pool, pool), False)
    cshape, ties_ref, _ = cache
    Hp, Wp = y_ref.shape[2:]
    g = Guards(rt)
    X, Wk = g.inp(layout.nchw_to_nhwc(pre), name='X', off=o('X')), g.inp(layout.conv_w_to_kernel(Wr), name='Wk', off=o('Wk'))
    act = ops.act(mode=1)
    Y, ties = g.out((N, Hp, Wp, Co), name='Y', off=o('Y')), g.out((N, Hp, Wp, Co), np.uint16, name='ties', off=o('ties'))
    ops.convpool_fwd(rt, X, N, H, W, Ci, Wk, k, k, pad, Co, pool, g.inp(b, name='bias', off=o('bias')), Y, ties, actX=act)(rt.stream)
    rt.synchronize()
    y, tb = fetch(Y), fetch(ties)
    assert all_written(y) and tb.max() < (1 << (pool * pool))          # (no half of the sentinel is a tie mask of at most nine bits)
    np.testing.assert_allclose(layout.nhwc_to_nchw(y), y_ref, rtol=0, atol=3e-6 * np.sqrt(k * k * Ci) * np.abs(y_ref).max())
    c = L.conv2d_fwd(x, Wr, None, (1, 1), border)
    cv = c[:, :, :Hp * pool, :Wp * pool].reshape(N, Co, Hp, pool, Wp, pool).transpose(0, 1, 2, 4, 3, 5).reshape(N, Co, Hp, Wp, pool * pool)
    gap = cv.max(axis=4, keepdims=True) - cv
    clear = ((gap == 0) | (gap > 1e-4)).all(axis=4)
    got = ((layout.nhwc_to_nchw(tb)[..., None] >> np.arange(pool * pool)) & 1).astype(bool)
    assert clear.mean() > 0.9 and (got[clear] == ties_ref[clear]).all()
    dy = rng.normal(size=y_ref.shape)
    dyb = g.inp(layout.nchw_to_nhwc(dy), name='dY', off=o('dY'))
    nblk = rt.lib.dpp_convpool_wgrad_blocks(N, Hp, Wp)
    nW = Co * k * k * Ci
    part, dX = g.out((nblk, nW), name='partial', off=o('partial')), g.out((N, H, W, Ci), name='dX', off=o('dX'))
    ops.convpool_wgrad(rt, X, N, H, W, Ci, dyb, ties, k, k, pad, Co, pool, part, actX=act)(rt.stream)
    ops.convpool_dgrad(rt, dyb, ties, N, H, W, Ci, Wk, k, k, pad, Co, pool, dX)(rt.stream)
    rt.synchronize()
    dx_ref, dW_ref, _ = L.convpool_bwd(x, Wr, dy, (cshape, got, y_ref), (1, 1), border, (pool, pool), False)
    p, dx = fetch(part), fetch(dX)
    assert all_written(p) and all_written(dx) and np.array_equal(fetch(ties), tb)
    dW = layout.conv_w_from_kernel(p.astype(f64).sum(axis=0).reshape(Co, k * k, Ci), (Co, Ci, k, k))
    np.testing.assert_allclose(dW, dW_ref, rtol=0, atol=3e-6 * np.sqrt(N * Hp * Wp) * np.abs(dW_ref).max())
    np.testing.assert_allclose(layout.nhwc_to_nchw(dx), dx_ref, rtol=0, atol=3e-6 * np.sqrt(k * k * Co) * np.abs(dx_ref).max())
    g.check()


# ======================================================================================================================
# BatchNorm reductions and the partial-sum reductions
# ======================================================================================================================
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('cfg', [(333, 64, 64), (130, 256, 32)], ids=lambda c: 'x'.join(map(str, c)))
def test_batchnorm_statistics_and_backward(backend, cfg):
    rt = get_runtime(backend)
    M, Cc, rpb = cfg
    rng = np.random.RandomState(13)
    x = (rng.normal(size=(M, Cc)) * rng.uniform(0.05, 2.0, Cc) + rng.normal(size=Cc) * 20.0).astype(f32)
    gamma, beta = rng.uniform(0.5, 1.5, Cc).astype(f32), (rng.normal(size=Cc) * 0.3).astype(f32)
    rm, ris = rng.normal(size=Cc).astype(f32), rng.uniform(0.5, 2, Cc).astype(f32)
    x4 = x.astype(f64).T.reshape(1, Cc, M, 1)
    y_ref, mean_ref, istd_ref = L.bn_fwd_train(x4, gamma.astype(f64), beta.astype(f64))
    nb = -(-M // rpb)
    g = Guards(rt)
    X, gb, bb = g.inp(x, name='X'), g.inp(gamma, name='gamma'), g.inp(beta, name='beta')
    rmb, risb = g.out((Cc,), name='run_mean', init=rm), g.out((Cc,), name='run_inv_std', init=ris)
    part = g.out((2, Cc, nb), name='partial')
    mean, istd, scale = (g.out((Cc,), name=n) for n in ('mean', 'inv_std', 'scale'))
    ops.bn_stats_partial(rt, X, M, Cc, rpb, part)(rt.stream)
    ops.bn_finalize(rt, part, nb, M, rpb, Cc, gb, 1e-4, mean, istd, scale, rmb, risb, 0.1)(rt.stream)
    rt.synchronize()
    assert all_written(fetch(part))
    np.testing.assert_allclose(fetch(mean), mean_ref, rtol=2e-7, atol=1e-7)          # f32 rounding of an f64 result
    np.testing.assert_allclose(fetch(istd), istd_ref, rtol=2e-6)
    np.testing.assert_allclose(fetch(scale), gamma * istd_ref, rtol=2e-6)
    rm2, ris2 = L.bn_running_update(rm, ris, mean_ref.astype(f32), istd_ref.astype(f32))
    np.testing.assert_allclose(fetch(rmb), rm2, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(fetch(risb), ris2, rtol=2e-6)
    g.check()
    # backward with the ReLU mask: reduce, finalize, apply (+ the gradient added to it, + the column sums of dX)
    dA, add = rng.normal(size=(M, Cc)).astype(f32), rng.normal(size=(M, Cc)).astype(f32)
    G, part2 = g.out((M, Cc), name='G'), g.out((2, Cc, nb), name='partial2')
    dbeta, dgamma, c1, c2 = (g.out((Cc,), name=n) for n in ('dbeta', 'dgamma', 'c1', 'c2'))
    dX, csp = g.out((M, Cc), name='dX'), g.out((nb, Cc), name='colsum')
    ops.bn_bwd_reduce(rt, g.inp(dA, name='dA'), X, M, Cc, mean, istd, scale, bb, 1, G, rpb, part2)(rt.stream)
    ops.bn_bwd_finalize(rt, part2, nb, M, Cc, dbeta, dgamma, c1, c2)(rt.stream)
    ops.bn_bwd_apply(rt, G, X, M, Cc, mean, istd, scale, c1, c2, dX, add=g.inp(add, name='add'), rpb=rpb, colsum=csp)(rt.stream)
    rt.synchronize()
    gd, dx = fetch(G), fetch(dX)
    assert all_written(gd) and all_written(dx) and all_written(fetch(part2)) and all_written(fetch(csp))
    np.testing.assert_allclose(fetch(csp).astype(f64).sum(0), dx.astype(f64).sum(0), rtol=0, atol=3e-6 * np.sqrt(M) * np.abs(dx).max())
    val = y_ref[0, :, :, 0].T                         # bn output (M, C)
    safe = np.abs(val) > 1e-4                         # the mask is decided on the device's own f32 bn value
    assert (gd[safe] == (dA.astype(f64) * (val >= 0))[safe].astype(f32)).all()
    dx_ref, dgamma_ref, dbeta_ref = L.bn_bwd_train(x4, gamma.astype(f64), mean_ref, istd_ref, gd.astype(f64).T.reshape(1, Cc, M, 1))
    np.testing.assert_allclose(fetch(dbeta), dbeta_ref, rtol=0, atol=2e-6 * np.sqrt(M) * np.abs(gd).max())
    np.testing.assert_allclose(fetch(dgamma), dgamma_ref, rtol=0, atol=2e-5 * np.sqrt(M) * np.abs(gd).max())
    np.testing.assert_allclose(dx, dx_ref[0, :, :, 0].T + add, rtol=0, atol=2e-5 * np.abs(dx_ref).max())
    g.check()


@pytest.mark.parametrize('backend', BACKENDS)
def test_batchnorm_backward_finalize_apply_in_one_launch(backend):
    """(96, 256, 3, 32) of test_bn_bwd_finalize_apply_equals_the_two_launches, guarded: equal bits from the one launch and the two."""
    rt = get_runtime(backend)
    M, Cc, nb, rpb = 96, 256, 3, 32
    rng = np.random.RandomState(83)
    assert rt.lib.dpp_bn_bwd_finalize_apply_ok(M, Cc, nb)
    g = Guards(rt)
    G, X, add = (g.inp(rng.normal(size=(M, Cc)), name=n) for n in ('G', 'X', 'add'))
    mean, istd, scale = (g.inp(rng.uniform(0.5, 1.5, Cc), name=n) for n in ('mean', 'inv_std', 'scale'))
    part = g.inp(rng.normal(size=(2, Cc, nb)) * 10, name='partial')
    dX1, dX2 = g.out((M, Cc), name='dX1'), g.out((M, Cc), name='dX2')
    db1, dg1, db2, dg2, c1, c2 = (g.out((Cc,), name=n) for n in ('db1', 'dg1', 'db2', 'dg2', 'c1', 'c2'))
    nb1 = -(-M // rpb)
    cs1, cs2 = g.out((nb1, Cc), name='cs1'), g.out((nb1, Cc), name='cs2')
    ops.bn_bwd_finalize(rt, part, nb, M, Cc, db1, dg1, c1, c2)(rt.stream)
    ops.bn_bwd_apply(rt, G, X, M, Cc, mean, istd, scale, c1, c2, dX1, add=add, rpb=rpb, colsum=cs1)(rt.stream)
    ops.bn_bwd_finalize_apply(rt, G, X, M, Cc, mean, istd, scale, part, nb, dX2, db2, dg2, add=add, rpb=rpb, colsum=cs2)(rt.stream)
    rt.synchronize()
    for a, b_ in ((db1, db2), (dg1, dg2), (dX1, dX2)):
        assert all_written(fetch(b_))
        np.testing.assert_array_equal(fetch(a), fetch(b_))
    s1, s2 = fetch(cs1).astype(f64).sum(0), fetch(cs2).astype(f64).sum(0)
    assert all_written(fetch(cs2))
    np.testing.assert_allclose(s2, s1, rtol=0, atol=1e-5 * np.abs(fetch(dX1)).sum(0).max())
    np.testing.assert_allclose(s2, fetch(dX2).astype(f64).sum(0), rtol=0, atol=1e-5 * np.abs(fetch(dX1)).sum(0).max())
    g.check()


def _bn_launches(rt, g, rng, off):
    """The four BatchNorm launches with tensor accesses, at (96, 32), four blocks of 24 rows, with the operand named `off` ('launch:operand')
    one element off: {launch: (Launch, its outputs)}."""
    M, Cc, rpb, nb = 96, 32, 24, 4
    o = lambda name: int(off == name)                                            # noqa: E731
    t = lambda name: g.inp(rng.normal(size=(M, Cc)), name=name, off=o(name))      # noqa: E731
    c = lambda name: g.inp(_vec(rng, Cc, 'scale'), name=name, off=o(name))        # noqa: E731
    out = {}
    part = g.out((2, Cc, nb), name='stats:partial', off=o('stats:partial'))
    out['stats'] = (ops.bn_stats_partial(rt, t('stats:X'), M, Cc, rpb, part), [part])
    G, p2 = g.out((M, Cc), name='reduce:G', off=o('reduce:G')), g.out((2, Cc, nb), name='reduce:partial', off=o('reduce:partial'))
    out['reduce'] = (ops.bn_bwd_reduce(rt, t('reduce:dA'), t('reduce:X'), M, Cc, c('reduce:mean'), c('reduce:inv_std'), c('reduce:scale'), c('reduce:beta'),
                                       1, G, rpb, p2), [G, p2])
    dX, cs = g.out((M, Cc), name='apply:dX', off=o('apply:dX')), g.out((nb, Cc), name='apply:colsum', off=o('apply:colsum'))
    out['apply'] = (ops.bn_bwd_apply(rt, t('apply:G'), t('apply:X'), M, Cc, c('apply:mean'), c('apply:inv_std'), c('apply:scale'), c('apply:c1'), c('apply:c2'),
                                     dX, add=t('apply:add'), rpb=rpb, colsum=cs), [dX, cs])
    dX2, cs2 = g.out((M, Cc), name='fa:dX', off=o('fa:dX')), g.out((nb, Cc), name='fa:colsum', off=o('fa:colsum'))
    db, dg = g.out((Cc,), name='fa:dbeta', off=o('fa:dbeta')), g.out((Cc,), name='fa:dgamma', off=o('fa:dgamma'))
    pin = g.inp(rng.normal(size=(2, Cc, nb)), name='fa:partial', off=o('fa:partial'))
    out['fa'] = (ops.bn_bwd_finalize_apply(rt, t('fa:G'), t('fa:X'), M, Cc, c('fa:mean'), c('fa:inv_std'), c('fa:scale'), pin, nb, dX2, db, dg,
                                           add=t('fa:add'), rpb=rpb, colsum=cs2), [dX2, cs2, db, dg])
    return out


BN_REFUSED = ['stats:X', 'reduce:dA', 'reduce:X', 'reduce:G', 'reduce:mean', 'reduce:inv_std', 'reduce:scale', 'reduce:beta',
              'apply:G', 'apply:X', 'apply:add', 'apply:dX', 'apply:mean', 'apply:inv_std', 'apply:scale', 'apply:c1', 'apply:c2',
              'fa:G', 'fa:X', 'fa:add', 'fa:dX', 'fa:mean', 'fa:inv_std', 'fa:scale', 'fa:partial']
BN_TOLERATED = ['stats:partial', 'reduce:partial', 'apply:colsum', 'fa:colsum', 'fa:dbeta', 'fa:dgamma']


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('which', BN_REFUSED)
def test_batchnorm_kernels_refuse_misaligned_tensors_and_vectors(backend, which):
    """The BatchNorm kernels read and write their [M][C] tensors and read their per-channel vectors four channels at a time (and
    bwd_finalize_apply its block sums, four blocks here): none of the entry points looked at those pointers.  Now DPP_E_BADARG, nothing launched."""
    rt = get_runtime(backend)
    g = Guards(rt)
    launch, outs = _bn_launches(rt, g, np.random.RandomState(3), which)[which.split(':')[0]]
    with pytest.raises(DppError, match='10001'):
        launch(rt.stream)
    rt.synchronize()
    assert all(untouched(fetch(b)) for b in outs)
    g.check()


@pytest.mark.parametrize('backend', BACKENDS[:1])
@pytest.mark.parametrize('which', BN_TOLERATED)
def test_batchnorm_kernels_tolerate_four_byte_aligned_partials_and_sums(backend, which):
    """What the BatchNorm kernels store float by float (include/dpp_hip.h): one element off, the same bits as aligned.  Emulator only."""
    rt = get_runtime(backend)
    got = []
    for off in (None, which):
        g = Guards(rt)
        launch, outs = _bn_launches(rt, g, np.random.RandomState(3), off)[which.split(':')[0]]
        launch(rt.stream)
        rt.synchronize()
        got.append([fetch(b) for b in outs])
        assert all(all_written(a) for a in got[-1])
        g.check()
    for a, b in zip(*got):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('backend', BACKENDS[:1])
@pytest.mark.parametrize('which', ['X', 'Wk', 'bias', 'Y', 'ties', 'dY', 'partial', 'dX'])
def test_convpool_kernels_tolerate_element_alignment(backend, which):
    """The ConvPoolLayer kernels access global memory one element at a time (include/dpp_hip.h): any operand one element off.  Emulator only."""
    _convpool_case(get_runtime(backend), (2, 20, 18, 3, 12, 3, 'half', 3), off=which)


@pytest.mark.parametrize('backend', BACKENDS)
def test_reduce_partials_and_reduce_multi_ragged_jobs(backend):
    """The ragged jobs of test_reduce_multi_ragged_jobs: every job's slices and its output guarded on their own (outputs of n % 4 != 0 jobs
    start four bytes off a 16-byte boundary, as they do inside that test's one flat buffer), by the batched and by the single launch."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(5)
    cases = [(1, 16), (5, 30), (37, 100), (20, 1028), (129, 63), (256, 64), (3, 1), (70, 260)]
    g = Guards(rt)
    jobs, outs = ops.ReduceJobs(rt), []
    for nz, n in cases:
        P = rng.normal(size=(nz, n)).astype(f32)
        pb = g.inp(P, name='partial %dx%d' % (nz, n))
        # (one float off for dpp_reduce_multi, whose kernel branches on its job's pointers; dpp_reduce_partials looks at no alignment: aligned)
        o1, o2 = g.out((n,), name='multi %dx%d' % (nz, n), off=int(n % 4 != 0)), g.out((n,), name='single %dx%d' % (nz, n))
        jobs.add(pb, nz, n, o1)
        ops.reduce_partials(rt, pb, nz, n, o2)(rt.stream)
        outs.append((o1, o2, P.astype(f64).sum(0)))
    jobs.launch()(rt.stream)
    rt.synchronize()
    for o1, o2, ref in outs:
        for o in (o1, o2):
            got = fetch(o)
            assert all_written(got)
            np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)
    g.check()
