"""The walking form of dpp_gemm's LDS-tiled kernel (gemm_walk_kernel, csrc/gemm_kernels.h): a launch of more row tiles than the device holds
at once runs on as many workgroups as are resident, each staging its B panel once and taking row tiles b, b + gx, ...

1. Walk equals one workgroup per tile BIT FOR BIT (C and every partial buffer), DPP_GEMM_WALK=2 (two workgroups per column tile) against
   DPP_GEMM_WALK=0, at the smallest shapes that can go wrong: 6 row tiles of 64 with a ragged last one (the two workgroups walk three tiles
   each, one of them ends on the ragged tile), 4 whole tiles, 128-row tiles with a ragged fourth; one and two column tiles; K as one chunk of
   32, two of 32 and two of 64; plain / stride-2 row map / prologue + bias + residual + statistics / data-gradient epilogue accumulating
   into C / bf16-stored A and C.
2. The same results against the float64 product formed the way tests/gemm_cases.py forms it, at that file's bar
   (6e-7 (sqrt(K) + 4) x operand scale); the bf16-stored output adds the rounding on its store, at most 2^-8 |value|.
3. The plan of the benchmarked net: what dpp_gemm_walk_grid says about every variant-0 descriptor (needs no GPU)."""
import ctypes as C
import functools

import numpy as np
import pytest

from hipdp import engine, ops
from hipdp.lib import Act, RowMap
from tests import gemm_cases
from tests.backends import BACKENDS, get_runtime

# (bm, M): 6 tiles of 64 the last one ragged, 4 whole tiles of 64, 4 tiles of 128 the last one ragged
ROWS = [(64, 5 * 64 + 24), (64, 4 * 64), (128, 3 * 128 + 8)]
COLS = [32, 64]                 # at bn = 32: one and two column tiles
DEPTHS = [32, 64, 128]          # one chunk of 32, two chunks of 32, two chunks of 64
MODES = ['plain', 'stride2', 'fwd_fused', 'dgrad_fused', 'bf16_stored']
BN = 32


def _bf16_bits(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _widen(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


class _BN(object):
    pass


def _walk_grid(rt, launch):
    gx, gy = C.c_int(-1), C.c_int(-1)
    w = rt.lib.dpp_gemm_walk_grid(C.byref(launch.keep[0]), C.byref(gx), C.byref(gy))
    return int(w), gx.value, gy.value


@functools.lru_cache(maxsize=None)
def _case(backend, bm, M, N, K, mode):
    """Runs one problem twice (walking with two workgroups per column tile, one workgroup per tile) on identical inputs.
    Returns (results of the walk, results of the one-tile grid, float64 reference dict, what the query said for both)."""
    import os
    rt = get_runtime(backend)
    rng = np.random.RandomState(1000 * bm + 10 * M + N + K + len(mode))
    ntiles = -(-M // bm)
    b_kc = mode != 'dgrad_fused'
    mapA = RowMap.strided(2, 4, 4, 8, 8) if mode == 'stride2' else RowMap.identity()
    mapC = RowMap.strided(2, 4, 4, 8, 8) if mode == 'dgrad_fused' else RowMap.identity()
    rowsA, rowsC = gemm_cases._maprows(mapA, M), gemm_cases._maprows(mapC, M)
    nA, nC = int(rowsA.max()) + 1, int(rowsC.max()) + 1
    A = rng.normal(0, 1, (nA, K)).astype(np.float32)
    Bm = (rng.normal(0, 1, (N, K) if b_kc else (K, N)) * 0.3).astype(np.float32)
    if mode == 'bf16_stored':
        A = _widen(_bf16_bits(A))
    act = None
    if mode == 'fwd_fused':
        act = dict(mode=Act.BN_RELU, cmod=K, mean=rng.normal(0, 0.3, K).astype(np.float32), scale=rng.uniform(0.5, 1.5, K).astype(np.float32),
                   beta=rng.normal(0, 0.3, K).astype(np.float32))
    bias = rng.normal(0, 1, N).astype(np.float32) if mode == 'fwd_fused' else None
    res = (rng.normal(0, 1, (nC, N)) + np.linspace(-3, 3, N)).astype(np.float32) if mode in ('fwd_fused', 'dgrad_fused') else None
    bnx = rng.normal(0, 1, (nC, N)).astype(np.float32) if mode == 'dgrad_fused' else None
    bnv = [rng.normal(0, 0.3, N), rng.uniform(0.5, 1.5, N), rng.normal(0, 0.3, N), rng.uniform(0.5, 1.5, N)] if mode == 'dgrad_fused' else None
    bnv = [v.astype(np.float32) for v in bnv] if bnv else None

    # ---- float64 reference (tests/gemm_cases.py: prologue in float64 on the float32 difference, product in float64) ----
    Aop = gemm_cases._apply_act(A, act)[rowsA]
    Bop = Bm.astype(np.float64).T if b_kc else Bm.astype(np.float64)
    want = Aop @ Bop
    if bias is not None:
        want = want + bias
    if res is not None:
        want = want + res[rowsC]
    ref = dict(scale=max(1.0, float(np.abs(Aop).max()) * float(np.abs(Bop).max())))
    if mode == 'dgrad_fused':
        bm_, bs_, bb_, bi_ = bnv
        x = bnx[rowsC].astype(np.float64)
        want = np.where((x - bm_) * bs_ + bb_ >= 0, want, 0.0)
        ref['bn_sums'] = (want.sum(0), (want * ((x - bm_) * bi_)).sum(0))
    ref['C'] = want

    def run(walk):
        os.environ['DPP_GEMM_WALK'] = walk
        try:
            dA = rt.upload(_bf16_bits(A)) if mode == 'bf16_stored' else rt.upload(A)
            dB = rt.upload(Bm)
            if mode == 'bf16_stored':
                Cb = rt.upload(np.full((nC, N), 0x7FC0, np.uint16))                # (NaN: rows the kernel must write)
            else:
                Cb = rt.upload(res) if res is not None else rt.upload(np.full((nC, N), np.nan, np.float32))
            a = ops.act(act['mode'], rt.upload(act['mean']), rt.upload(act['scale']), rt.upload(act['beta']), K) if act else None
            stats = rt.upload(np.full((2, N, ntiles), np.nan, np.float32)) if mode == 'fwd_fused' else None
            part = rt.upload(np.full((2, N, ntiles), np.nan, np.float32)) if mode == 'dgrad_fused' else None
            epi = None
            if stats is not None:
                epi = ops.epilogue(stats=stats)
            if part is not None:
                bnl = _BN()
                bnl.mean, bnl.scale, bnl.beta_buf, bnl.inv_std = (rt.upload(v) for v in bnv)
                epi = ops.epilogue(bn=bnl, bn_x=rt.upload(bnx), bn_relu=True, bn_partial=part)
            L = ops.gemm(rt, dA, dB, Cb, M, N, K, 1, int(b_kc), K, K if b_kc else N, N, mapA=mapA, mapC=mapC, actA=a,
                         bias=rt.upload(bias) if bias is not None else None, residual=Cb if res is not None else None, tile=(bm, BN, 4), epi=epi,
                         name='walk_%s' % mode)
            said = _walk_grid(rt, L)
            L(rt.stream)
            rt.synchronize()
            return dict(C=Cb.get().copy(), stats=stats.get().copy() if stats is not None else None,
                        part=part.get().copy() if part is not None else None), said
        finally:
            del os.environ['DPP_GEMM_WALK']

    walked, said_walk = run('2')
    single, said_single = run('0')
    return walked, single, ref, rowsC, said_walk, said_single


def _cases():
    return [pytest.param(bm, M, N, K, mode, id='bm%d-M%d-N%d-K%d-%s' % (bm, M, N, K, mode))
            for (bm, M) in ROWS for N in COLS for K in DEPTHS for mode in MODES]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('bm,M,N,K,mode', _cases())
def test_walk_is_bit_identical_to_one_workgroup_per_tile(backend, bm, M, N, K, mode):
    walked, single, _, _, said_walk, said_single = _case(backend, bm, M, N, K, mode)
    assert said_walk == (1, 2, N // BN)             # two workgroups per column tile walk the 4 - 6 row tiles
    assert said_single == (0, 0, 0)
    for key in ('C', 'stats', 'part'):
        if walked[key] is None:
            assert single[key] is None
            continue
        assert np.array_equal(walked[key].view(np.uint8), single[key].view(np.uint8)), key      # (bytes: NaN fill of untouched rows compares equal)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('bm,M,N,K,mode', _cases())
def test_walk_against_float64(backend, bm, M, N, K, mode):
    walked, _, ref, rowsC, _, _ = _case(backend, bm, M, N, K, mode)
    want = ref['C']
    # tests/gemm_cases.py: f32 accumulation of K products of O(1) operands, error ~ eps * sqrt(K) * |operand scale|^2, a few times that allowed
    tol = 6e-7 * (np.sqrt(K) + 4) * ref['scale']
    if mode == 'bf16_stored':
        got = _widen(walked['C'])[rowsC].astype(np.float64)
        err = np.abs(got - want) - 2.0 ** -8 * np.abs(want)          # + the unit roundoff of bfloat16 (8 significant bits) on the store
    else:
        got = walked['C'][rowsC].astype(np.float64)
        err = np.abs(got - want)
    print('%s bm %d M %d N %d K %d: max err %.3g, tol %.3g' % (mode, bm, M, N, K, float(err.max()), tol))
    assert float(err.max()) < tol
    ntiles = -(-M // bm)
    if walked['stats'] is not None:                                   # per row TILE (mean, M2), the ragged tile over its valid rows
        st = walked['stats'].reshape(2, N, ntiles)
        for t in range(ntiles):
            blk = got[t * bm:min(M, (t + 1) * bm)]
            mean = blk.mean(axis=0)
            m2 = ((blk - mean) ** 2).sum(axis=0)
            np.testing.assert_allclose(st[0, :, t], mean, rtol=0, atol=1e-5 * max(1.0, np.abs(got).max()))
            np.testing.assert_allclose(st[1, :, t], m2, rtol=5e-5, atol=1e-4 * max(1.0, m2.max()))
    if walked['part'] is not None:                                    # per row tile (sum G, sum G xhat), summed over the tiles
        p = walked['part'].reshape(2, N, ntiles).astype(np.float64).sum(axis=2)
        for i in (0, 1):
            np.testing.assert_allclose(p[i], ref['bn_sums'][i], rtol=0, atol=2e-5 * max(1.0, np.abs(want).sum(0).max()))


def _v0_descriptors(eng):
    out = []
    for plan in (eng.fwd, eng.bwd):
        for op, _ in plan.ops:
            if getattr(op, 'fn', None) is eng.rt.lib.dpp_gemm and op.keep[0].variant == 0:
                out.append(op)
    return out


def test_plan_of_the_benchmarked_net(monkeypatch):
    """bs128 128 x 128 train engine on the emulator runtime.  Which launches walk must follow from the descriptor: split-K and LAZY
    (two-tensor operand) launches never do; an eligible launch -- splitk 1, K-contiguous A with a mode 0-3 prologue, plain B, K <= 128 --
    of more row tiles than the cap does, on a grid within the cap and with one column of workgroups per column tile.  The cap: with
    DPP_GEMM_WALK unset what the device holds at once, never more than 8 workgroups of four waves on each of 256 CUs; with
    DPP_GEMM_WALK=N at most N workgroups per column tile.
    The walk changes the grid alone: the query leaves the descriptor (kernel variant, tile) as it was, a batch of 8 of the same net asks for
    the same kernel variant layer by layer, and the bs128 descriptors shrunk to the rows of a batch of 8 -- same tile -- fit at once and do
    not walk.  (The engine's own tile choice follows the row count -- 64 x 16 at batch 8 where batch 128 takes 128 x 16 or 64 x 64 --, as
    it did before the walk existed.)"""
    from net.resnet import ResNet, ResNetParams
    rt = get_runtime('emu')

    def build(batch):
        net = ResNet(np.random.RandomState(23455), cfgParams=ResNetParams(type=0, nChan=1, wIn=128, hIn=128, batchSize=batch, numJoints=1, nDims=30))
        return engine.CompiledNet(net, train=True, runtime=rt, loss=dict(kind='embedding'))

    big = _v0_descriptors(build(128))
    assert len(big) >= 40

    def eligible(d):
        return d.splitk == 1 and d.a_kc == 1 and d.actA.mode in (0, 1, 2, 3) and d.actB.mode == 0 and d.K <= 128 and d.wm == 4

    n_walk = 0
    for cap_env in (None, '256'):
        if cap_env is None:
            monkeypatch.delenv('DPP_GEMM_WALK', raising=False)
        else:
            monkeypatch.setenv('DPP_GEMM_WALK', cap_env)
        for op in big:
            d = op.keep[0]
            before = (d.variant, d.bm, d.bn, d.wm, d.M, d.N, d.K, d.splitk)
            w, gx, gy = _walk_grid(rt, op)
            assert (d.variant, d.bm, d.bn, d.wm, d.M, d.N, d.K, d.splitk) == before
            ntiles, ncol = -(-d.M // d.bm), -(-d.N // d.bn)
            if d.splitk > 1 or d.actA.mode == 4 or not eligible(d):
                assert (w, gx, gy) == (0, 0, 0), op.name
                continue
            if w:
                n_walk += 1
                assert gy == ncol and 0 < gx < ntiles, (op.name, gx, gy)
                assert gx * gy <= 256 * 8 and (cap_env is None or gx <= int(cap_env)), (op.name, gx, gy)
            else:
                assert (gx, gy) == (0, 0)
                # not walking is only right when the tiles fit: under the explicit cap, or (unset) within what any device could hold
                assert ntiles <= int(cap_env) if cap_env is not None else ntiles * ncol <= 256 * 8, (op.name, ntiles, ncol)
    assert n_walk >= 6                        # the stride-2 entries, the projection shortcuts and their data gradients are among them
    monkeypatch.delenv('DPP_GEMM_WALK', raising=False)
    small = {op.name: op.keep[0] for op in _v0_descriptors(build(8))}
    for op in big:
        d = op.keep[0]
        if op.name in small:
            assert small[op.name].variant == d.variant, op.name
        m0 = d.M
        try:
            d.M = m0 // 16                    # the rows of a batch of 8, the tile of batch 128
            assert _walk_grid(rt, op) == (0, 0, 0), op.name
        finally:
            d.M = m0
