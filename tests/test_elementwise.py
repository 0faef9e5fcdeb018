"""The train-step tail kernels of csrc/elementwise.hip, and the two job-table launches of csrc/bn.hip and csrc/conv3x3.hip, called
directly through hipdp.ops and held to the references of tests/elementwise_ref.py at the sizes where each kernel takes another path:
a second trip of a strided loop, a tail, a misaligned pointer, the grid cap, a segment or job that ends on a block boundary.
Runs on the SIMT emulator in the CPU tier and through the C ABI of libdpp_hip.so on the MI355X (`-m gpu`); on the emulator the
workgroups of a launch run one after another, so the ticket of dpp_adam_ticked is only contended on the GPU tier."""
import numpy as np
import pytest

from hipdp import ops
from hipdp.lib import DppError
from oracle import layers as L
from tests import elementwise_ref as R
from tests.backends import BACKENDS, get_runtime

f32, f64 = np.float32, np.float64
GRID_CAP = 4096 * 256                     # elements of one trip of a grid-stride loop at the cap of 4096 workgroups
SENTINEL = np.uint32(0x7FC0DEAD)          # a NaN: a canary that also poisons whatever reads it


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_bits_equal(got, want):
    np.testing.assert_array_equal(bits(got), bits(want))


def canaried(rt, n, tail=8):
    """A buffer of n floats with `tail` sentinel words behind it: (the whole buffer, the view a kernel gets)."""
    whole = rt.upload(np.full(n + tail, SENTINEL, np.uint32).view(f32))
    return whole, whole.view(0, (n,))


def canary_ok(whole, n):
    return (bits(whole.get())[n:] == SENTINEL).all()


def offset_view(rt, arr, off=1):
    """arr uploaded `off` floats into an allocation: a pointer that is not 16-byte aligned."""
    arr = np.asarray(arr, f32).ravel()
    v = rt.alloc(arr.size + off, zero=False).view(off, (arr.size,))
    v.set(arr)
    return v


# ======================================================================================================================
# 1. fused split-K reduction + cost
# ======================================================================================================================
RPL_CASES = [(4, 30, 8),        # one trip, vector path
             (3, 30, 8),        # n & 3 = 2: scalar path
             (140, 30, 5),      # n4 = 1050: a second trip with 26 quads
             (137, 30, 3),      # scalar path, two trips
             (8, 4, 1),         # single slice
             (8, 4, 16), (8, 4, 17), (16, 30, 19),     # both sides of the 16-slice register window
             (64, 1, 2),        # nbias = 1
             (2048, 32, 2)]     # n = 65536, the largest admitted


def _rpl_inputs(rows, d, nz, seed=3):
    rng = np.random.RandomState(seed + rows * 131 + d * 7 + nz)
    n = rows * d
    partial = rng.normal(size=(nz, n)).astype(f32)
    partial[partial == 0] = 1.0                      # never -0.0 (nor +0.0): "0 + slice 0" and "slice 0" are then the same bits
    return partial, rng.normal(size=d).astype(f32), rng.normal(size=n).astype(f32)


def _rpl_run(rt, partial, bias, y, rows, d, with_dout, yb=None, doutb=None):
    nz, n = partial.shape
    pb, bb = rt.upload(partial), (rt.upload(bias) if bias is not None else None)
    yb = rt.upload(y) if yb is None else yb
    out, cost = rt.alloc(n, zero=False), rt.alloc(1, zero=False)
    if with_dout and doutb is None:
        doutb = rt.alloc(n, zero=False)
    ops.reduce_partials_loss(rt, pb, nz, rows, d, out, bb, yb, rows, cost, doutb if with_dout else None)(rt.stream)
    rt.synchronize()
    return out.get(), float(cost.get()[0]), (doutb.get() if with_dout else None)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('case', RPL_CASES)
def test_reduce_partials_loss(backend, case):
    rt = get_runtime(backend)
    rows, d, nz = case
    n = rows * d
    partial, bias, y = _rpl_inputs(rows, d, nz)
    for use_bias in (True, False):
        b = bias if use_bias else None
        want = R.reduce_partials_f32(partial, b)
        # the two launches this one replaced
        pb, o2, c2 = rt.upload(partial), rt.alloc(n, zero=False), rt.alloc(1, zero=False)
        ops.reduce_partials(rt, pb, nz, n, o2, bias=rt.upload(b) if use_bias else None, nbias=d)(rt.stream)
        ops.loss_sse(rt, o2, rt.upload(y), rows, d, rows, c2)(rt.stream)
        rt.synchronize()
        for with_dout in (True, False):
            out, cost, dout = _rpl_run(rt, partial, b, y, rows, d, with_dout)
            assert_bits_equal(out, want)
            if with_dout:
                assert_bits_equal(dout, R.dout_f32(want, y, rows))
            # the float32 difference, the float32 1 / denom and the final rounding to float32: three round-offs of 6e-8
            np.testing.assert_allclose(cost, R.cost_f64(out, y, rows), rtol=1e-6)
            np.testing.assert_allclose(cost, float(c2.get()[0]), rtol=1e-6)


@pytest.mark.parametrize('backend', BACKENDS)
def test_reduce_partials_loss_misaligned_pointers_take_the_scalar_path(backend):
    rt = get_runtime(backend)
    rows, d, nz = 4, 30, 8
    partial, bias, y = _rpl_inputs(rows, d, nz)
    out0, cost0, dout0 = _rpl_run(rt, partial, bias, y, rows, d, True)
    out1, cost1, dout1 = _rpl_run(rt, partial, bias, y, rows, d, True, yb=offset_view(rt, y))
    out2, cost2, dout2 = _rpl_run(rt, partial, bias, y, rows, d, True, doutb=rt.alloc(rows * d + 1, zero=False).view(1, (rows * d,)))
    for out, dout, cost in ((out1, dout1, cost1), (out2, dout2, cost2)):
        assert_bits_equal(out, out0)
        assert_bits_equal(dout, dout0)
        np.testing.assert_allclose(cost, cost0, rtol=1e-6)


@pytest.mark.parametrize('backend', BACKENDS)
def test_reduce_partials_loss_refuses_more_than_65536_outputs(backend):
    rt = get_runtime(backend)
    n = 65537
    pb, yb = rt.upload(np.ones(n, f32)), rt.upload(np.ones(n, f32))
    out, cost = rt.upload(np.full(n, 7.0, f32)), rt.upload(np.full(1, 7.0, f32))
    with pytest.raises(DppError):
        ops.reduce_partials_loss(rt, pb, 1, n, 1, out, None, yb, n, cost)(rt.stream)
    rt.synchronize()
    assert (out.get() == 7.0).all() and cost.get()[0] == 7.0          # nothing was launched


# ======================================================================================================================
# 2. ADAM with the in-launch step count
# ======================================================================================================================
ADAM_BIG = 4 * GRID_CAP + 4 * 256 * 3 + 2        # a second grid-stride trip that only three workgroups take, and a tail of two
# The big size under the emulator (six launches of 4096 workgroups): 4.8 s and 7.2 s in two runs; the slowest case of
# tests/test_kernels.py, test_conv3x3_filter_gradient_on_transposed_images[cfg5], 7.3 s on the same machine.  It stays in both tiers.
ADAM_SIZES = [1, 2, 3, 4, 7, 1003, 2049, ADAM_BIG]
HYPER = [1e-3, 1.0, 0.9, 0.999, 1e-8, 1 - 1e-8, 0, 0]


def _ticket(hyper):
    return int(hyper.get().view(np.uint32)[7])


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('n', ADAM_SIZES)
def test_adam_ticked(backend, n):
    rt = get_runtime(backend)
    rng = np.random.RandomState(100 + n % 1000)
    w = rng.normal(size=n).astype(f32)
    grads = [(rng.normal(size=n) * 10 ** rng.uniform(-6, 0, n)).astype(f32) for _ in range(3)]
    gb = [rt.upload(g) for g in grads]
    lr = f32(1e-3)
    # step by step, a host read after every launch
    wb, m, v, hyper = rt.upload(w), rt.alloc(n), rt.alloc(n), rt.upload(np.array(HYPER, f32))
    for step in range(3):
        # The bars below are round-off bounds of ONE step, so the oracle takes every step from the state the device holds (m of two
        # runs that differ by an ulp after step 1 stay an ulp apart, and 0.9 ulp of m_prev is more than 2e-7 |g| for a small g).
        # What the steps accumulate to is held by test_adam_ticked_update_from_zero_weights.
        P, Mo, Vo = [wb.get()], [m.get()], [v.get()]
        ops.adam(rt, wb, gb[step], m, v, n, hyper, tick=True)(rt.stream)
        rt.synchronize()
        assert hyper.get()[1] == step + 2
        assert _ticket(hyper) == 0
        m_prev = Mo[0].copy()
        assert L.adam_step(P, [grads[step]], Mo, Vo, step + 1.0, lr) == step + 2.0
        np.testing.assert_allclose(wb.get(), P[0], rtol=2e-6, atol=1e-9)
        # b1*m + (1-b1)*g may cancel: the round-off bound is relative to the terms, not to the result
        assert (np.abs(m.get() - Mo[0]) <= 2e-7 * (np.abs(m_prev) + np.abs(grads[step])) + 1e-30).all()
        np.testing.assert_allclose(v.get(), Vo[0], rtol=2e-6, atol=1e-20)
    # the same three launches back to back: every launch reads the step count the one before it left
    wb2, m2, v2, hyper2 = rt.upload(w), rt.alloc(n), rt.alloc(n), rt.upload(np.array(HYPER, f32))
    launches = [ops.adam(rt, wb2, gb[step], m2, v2, n, hyper2, tick=True) for step in range(3)]
    rt.synchronize()
    for launch in launches:
        launch(rt.stream)
    rt.synchronize()
    assert hyper2.get()[1] == 4.0 and _ticket(hyper2) == 0
    assert_bits_equal(wb2.get(), wb.get())
    assert_bits_equal(m2.get(), m.get())
    assert_bits_equal(v2.get(), v.get())


# Maximum error of the device powf in ulp: 1, from the table of single-precision functions of the HIP math API reference ("powf:
# maximum ULP error 1"; the same table lists sqrtf and the division as correctly rounded, which hipcc's default
# -fhip-fp32-correctly-rounded-divide-sqrt makes them).
POWF_ULP = 1.0


@pytest.mark.parametrize('backend', BACKENDS)
def test_adam_ticked_update_from_zero_weights(backend):
    """From w = 0 the parameters ARE the accumulated updates, so a bar on w binds on the update (about 1e-3 here) and not on
    |w| ~ 1.  Gradients of one sign per element: m and v are sums of positive terms, and the bound of R.adam_update_relerr holds:
      |w_T - sum_t u_t| <= sum_t du_t |u_t|  +  (T - 1) U |w_T|      (w_1 = -u_1 exactly; every later subtraction rounds once,
                                                                      relative to a |w_t| that only grows)
    times 1.01 for the second-order terms the first-order du_t leaves out (du_t <= 1.3e-4: they are below 1e-4 of it).
    du_1 = 6.0e-5 (the power of beta2 at t = 1, amplified by 999 and halved by the square root), du_2 = 3.1e-5, du_3 = 2.1e-5."""
    rt = get_runtime(backend)
    n, T = 1003, 3
    rng = np.random.RandomState(7)
    grads = [((np.abs(rng.normal(size=n)) + 0.1) * 10 ** rng.uniform(-3, 0, n)).astype(f32) for _ in range(T)]
    wb, m, v, hyper = rt.alloc(n), rt.alloc(n), rt.alloc(n), rt.upload(np.array(HYPER, f32))
    for g in grads:
        ops.adam(rt, wb, rt.upload(g), m, v, n, hyper, tick=True)(rt.stream)
    rt.synchronize()
    assert hyper.get()[1] == T + 1.0 and _ticket(hyper) == 0
    u = R.adam_updates_f64(grads, HYPER[0])
    w_ref = -np.sum(u, axis=0)
    bound = 1.01 * (sum(R.adam_update_relerr(t + 1, POWF_ULP) * np.abs(u[t]) for t in range(T)) + (T - 1) * R.U * np.abs(w_ref))
    err = np.abs(wb.get().astype(f64) - w_ref)
    print("adam from zero: max err / bound = %.3g, bound / |w| in [%.3g, %.3g]" % ((err / bound).max(), (bound / np.abs(w_ref)).min(),
                                                                                  (bound / np.abs(w_ref)).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize('backend', BACKENDS)
def test_rmsprop_ticked(backend):
    rt = get_runtime(backend)
    rng = np.random.RandomState(15)
    n = 1003
    w = rng.normal(size=n).astype(f32)
    wb, m, msg = rt.upload(w), rt.alloc(n), rt.alloc(n)
    hyper = rt.upload(np.array([1e-2, 1.0, 0, 0.9, 1.0 / 100., 0, 1, 0], f32))
    ref_w, ref_ms = w.copy(), np.zeros(n, f32)
    for step in range(3):
        g = (rng.normal(size=n) * 10 ** rng.uniform(-4, 0, n)).astype(f32)
        ops.adam(rt, wb, rt.upload(g), m, msg, n, hyper, tick=True)(rt.stream)
        rt.synchronize()
        assert hyper.get()[1] == step + 2 and _ticket(hyper) == 0
        ref_w, ref_ms = R.rmsprop_step_f32(ref_w, ref_ms, g, 1e-2, 0.9, 1.0 / 100.)
        np.testing.assert_allclose(msg.get(), ref_ms, rtol=2e-6, atol=1e-20)
        np.testing.assert_allclose(wb.get(), ref_w, rtol=2e-6, atol=1e-7)
    assert (m.get() == 0).all()                      # the rule does not use m


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('which', range(4))
def test_adam_refuses_a_misaligned_pointer(backend, which):
    rt = get_runtime(backend)
    n = 8
    bufs = [rt.upload(np.full(n + 1, 3.0, f32)) for _ in range(4)]
    args = [b.view(1, (n,)) if i == which else b.view(0, (n,)) for i, b in enumerate(bufs)]
    hyper = rt.upload(np.array(HYPER, f32))
    for tick in (True, False):
        with pytest.raises(DppError):
            ops.adam(rt, args[0], args[1], args[2], args[3], n, hyper, tick=tick)(rt.stream)
    rt.synchronize()
    assert all((b.get() == 3.0).all() for b in bufs) and hyper.get()[1] == 1.0 and _ticket(hyper) == 0


# ======================================================================================================================
# 3. the weight-decay regulariser
# ======================================================================================================================
SEG_LENS = [1, 3, 255, 256, 257, 1023, 1024, 1025, 1024 * 256 + 1]       # the last: per = 257 > 256, the inner loop strides


def _segments(lens):
    """Odd offsets (so none is a multiple of 4) with a gap of at least three floats in front of every segment."""
    offs, off = [], 3
    for ln in lens:
        offs.append(off)
        off += ln + 3
        off += 1 - (off & 1)
    return offs, off + 3


def _sumsq_bar(out0, alpha, ssq):
    """out = fl(out0 + fl(alpha * S)) with S summed in float64: the product rounds once relative to alpha * S, the sum once relative
    to |out0 + alpha * S| <= |out0| + alpha * S.  Two roundings of one float32 ulp (2^-23 = 1.2e-7) of that larger term."""
    return 2.4e-7 * (abs(out0) + float(alpha) * ssq)


def _flat(rng, lens, fill_nan=True):
    offs, total = _segments(lens)
    x = np.full(total, np.nan if fill_nan else 0.0, f32)
    inside = np.zeros(total, bool)
    for o, ln in zip(offs, lens):
        x[o:o + ln] = rng.normal(size=ln)
        inside[o:o + ln] = True
    return x, offs, inside


def _table_with_an_empty_entry(rt, base, offs, lens, empty_at):
    """ops.segment_table over the views, with one zero-length entry (pointing into a gap) written into it by hand."""
    seg, nseg = ops.segment_table(rt, base, [base.view(o, (ln,)) for o, ln in zip(offs, lens)])
    assert nseg == len(lens)
    t = seg.get().reshape(-1, 2)
    np.testing.assert_array_equal(t, np.stack([offs, lens], 1))
    k = len(lens) // 2
    t = np.concatenate([t[:k], [[empty_at, 0]], t[k:]])
    return rt.upload(t.astype(np.int64).ravel()), nseg + 1


@pytest.mark.parametrize('backend', BACKENDS)
def test_sumsq_multi_reads_its_segments_and_nothing_else(backend):
    rt = get_runtime(backend)
    rng = np.random.RandomState(21)
    x, offs, inside = _flat(rng, SEG_LENS)                     # NaN in every gap: one read outside a segment poisons the sum
    base = rt.upload(x)
    seg, nseg = _table_with_an_empty_entry(rt, base, offs, SEG_LENS, offs[4] - 2)
    alpha = f32(1e-3)
    ssq = float((x[inside].astype(f64) ** 2).sum())
    for out0, accumulate in ((np.nan, 0), (12.5, 1), (-3e3, 1)):
        out = rt.upload(np.array([out0], f32))
        ops.sumsq_multi(rt, base, seg, nseg, alpha, out, accumulate)(rt.stream)
        rt.synchronize()
        start = out0 if accumulate else 0.0
        want = start + float(alpha) * ssq
        got = float(out.get()[0])
        print("sumsq_multi: out0 %r got %.9g want %.9g bar %.3g" % (out0, got, want, _sumsq_bar(start, alpha, ssq)))
        assert abs(got - want) <= _sumsq_bar(start, alpha, ssq)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('n', [1, 255, 257, 70001])
def test_sumsq_and_sumsq_multi_over_one_segment(backend, n):
    rt = get_runtime(backend)
    rng = np.random.RandomState(n)
    x, offs, inside = _flat(rng, [n])
    base = rt.upload(x)
    view = base.view(offs[0], (n,))
    seg, nseg = ops.segment_table(rt, base, [view])
    alpha = f32(0.37)
    ssq = float((x[inside].astype(f64) ** 2).sum())
    for out0, accumulate in ((np.nan, 0), (-2.25, 1)):
        o1, o2 = rt.upload(np.array([out0], f32)), rt.upload(np.array([out0], f32))
        ops.sumsq(rt, view, n, alpha, o1, accumulate)(rt.stream)
        ops.sumsq_multi(rt, base, seg, nseg, alpha, o2, accumulate)(rt.stream)
        rt.synchronize()
        start = out0 if accumulate else 0.0
        bar = _sumsq_bar(start, alpha, ssq)
        want = start + float(alpha) * ssq
        assert abs(float(o1.get()[0]) - want) <= bar
        assert abs(float(o2.get()[0]) - want) <= bar
        assert abs(float(o1.get()[0]) - float(o2.get()[0])) <= bar


def _axpy_check(got, y, x, alpha):
    """|got - (y + alpha x)| <= 2e-7 (|y| + |alpha x|) against float64: the form the ADAM test uses for m (the multiply-add may be
    contracted, and the sum may cancel)."""
    ax = f64(f32(alpha)) * x.astype(f64)
    assert (np.abs(got.astype(f64) - (y.astype(f64) + ax)) <= 2e-7 * (np.abs(y) + np.abs(ax))).all()


@pytest.mark.parametrize('backend', BACKENDS)
def test_axpy_multi_writes_its_segments_and_nothing_else(backend):
    rt = get_runtime(backend)
    rng = np.random.RandomState(22)
    x, offs, inside = _flat(rng, SEG_LENS)
    y = np.full(x.size, SENTINEL, np.uint32).view(f32).copy()
    y[inside] = rng.normal(size=int(inside.sum()))
    xb, yb = rt.upload(x), rt.upload(y)
    seg, nseg = _table_with_an_empty_entry(rt, yb, offs, SEG_LENS, offs[4] - 2)
    alpha = f32(2 * 1e-3)
    ops.axpy_multi(rt, yb, xb, seg, nseg, alpha)(rt.stream)
    rt.synchronize()
    got = yb.get()
    assert (bits(got)[~inside] == SENTINEL).all()
    _axpy_check(got[inside], y[inside], x[inside], alpha)
    # a launch that did nothing would pass the bound wherever alpha x is below the round-off of y: it must have moved the rest
    assert (got[inside] != y[inside]).mean() > 0.9


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('n', [1, 257, GRID_CAP + 259])
def test_axpy(backend, n):
    rt = get_runtime(backend)
    rng = np.random.RandomState(n % 1000)
    x, y = rng.normal(size=n).astype(f32), rng.normal(size=n).astype(f32)
    ywhole, yb = canaried(rt, n)
    yb.set(y)
    alpha = f32(-0.3)
    ops.axpy(rt, yb, rt.upload(x), alpha, n)(rt.stream)
    rt.synchronize()
    got = yb.get()
    _axpy_check(got, y, x, alpha)
    assert (got != y).mean() > 0.9 or n == 1 and got[0] != y[0]
    assert canary_ok(ywhole, n)


# ======================================================================================================================
# 4. the other cost and monitor kernels
# ======================================================================================================================
def _bcast_check(rt, o, y):
    n = o.size
    c_ref, d_ref, e_mean, e_max = R.loss_bcast_f64(o, y)
    ob, yb = rt.upload(o), rt.upload(y)
    for with_dout in (True, False):
        for with_err in (True, False):
            cost, dout, err = rt.alloc(1, zero=False), rt.alloc(n, zero=False), rt.alloc(2, zero=False)
            ops.loss_sse_bcast(rt, ob, yb, n, cost, dout if with_dout else None, err if with_err else None)(rt.stream)
            rt.synchronize()
            got = float(cost.get()[0])
            print("loss_sse_bcast n=%d: cost %.9g, pairwise float64 %.9g, relative %.3g" % (n, got, c_ref, abs(got - c_ref) / c_ref))
            np.testing.assert_allclose(got, c_ref, rtol=1e-6)
            if with_dout:
                np.testing.assert_allclose(dout.get(), d_ref, rtol=1e-6, atol=1e-9 * np.abs(d_ref).max())
            if with_err:
                np.testing.assert_allclose(err.get(), [e_mean, e_max], rtol=1e-6)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, 1000])
def test_loss_sse_bcast(backend, n):
    rng = np.random.RandomState(n)
    _bcast_check(get_runtime(backend), rng.normal(size=n).astype(f32), rng.normal(size=n).astype(f32))


@pytest.mark.parametrize('backend', BACKENDS)
def test_loss_sse_bcast_far_from_zero(backend):
    """o, y = 1000 +- 1e-3 at B = 128.  The expanded form (B sum o^2 - 2 sum o sum y + B sum y^2) / B^2 on the raw values cancels
    eleven digits of its float64 sums: restated in NumPy float64 in the kernel's order of summation it is off by 9.0e-6 of the
    pairwise cost at such inputs (1e-16 at offset 0, 7e-9 at 100 +- 0.01), and the kernel itself, before it subtracted y[0] from
    both, by 1.3e-4 on the draw below (cost 1.794077e-06 against 1.793842e-06)."""
    rng = np.random.RandomState(128)
    B = 128
    o = (1000.0 + 1e-3 * rng.normal(size=B)).astype(f32)
    y = (1000.0 + 1e-3 * rng.normal(size=B)).astype(f32)
    _bcast_check(get_runtime(backend), o, y)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('shape', [(1, 30), (257, 3), (600, 1)])
def test_error_l2(backend, shape):
    rt = get_runtime(backend)
    rng = np.random.RandomState(shape[0])
    out, y = rng.normal(size=shape).astype(f32), rng.normal(size=shape).astype(f32)
    err = rt.alloc(2, zero=False)
    ops.error_l2(rt, rt.upload(out), rt.upload(y), shape[0], shape[1], err)(rt.stream)
    rt.synchronize()
    np.testing.assert_allclose(err.get(), R.error_l2_f64(out, y), rtol=1e-6)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('shape', [(1, 1), (257, 3)])
def test_loss_sse(backend, shape):
    rt = get_runtime(backend)
    rng = np.random.RandomState(shape[0])
    rows, d = shape
    out, y = rng.normal(size=shape).astype(f32), rng.normal(size=shape).astype(f32)
    for with_dout in (True, False):
        cost, dout = rt.alloc(1, zero=False), rt.alloc(rows * d, zero=False)
        ops.loss_sse(rt, rt.upload(out), rt.upload(y), rows, d, rows, cost, dout if with_dout else None)(rt.stream)
        rt.synchronize()
        np.testing.assert_allclose(cost.get()[0], R.cost_f64(out, y, rows), rtol=1e-6)
        if with_dout:
            assert_bits_equal(dout.get(), R.dout_f32(out, y, rows))
            np.testing.assert_allclose(dout.get(), 2.0 / rows * (out.astype(f64) - y).ravel(), rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('cfg', [(5, 300, 8), (77, 257, 16), (300, 513, 1), (33, 1, 7), (9, 256, 128)])
def test_colsum_partial_and_reduce(backend, cfg):
    rt = get_runtime(backend)
    M, Cc, rpb = cfg
    X = np.random.RandomState(M).normal(size=(M, Cc)).astype(f32)
    nb = -(-M // rpb)
    pwhole, part = canaried(rt, nb * Cc)
    swhole, s = canaried(rt, Cc)
    ops.colsum_partial(rt, rt.upload(X), M, Cc, rpb, part)(rt.stream)
    ops.reduce_partials(rt, part, nb, Cc, s)(rt.stream)
    rt.synchronize()
    np.testing.assert_allclose(s.get(), X.astype(f64).sum(0), rtol=0, atol=2e-6 * np.sqrt(M) * 4)
    assert canary_ok(pwhole, nb * Cc) and canary_ok(swhole, Cc)


# ======================================================================================================================
# 5. helpers: bit for bit
# ======================================================================================================================
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('cfg', [(5, 42, 3, 2), (1, 1, 1, 0), (300, 3, 3, 2), (4099, 257, 3, 1)])     # the last: above the grid cap
def test_rowscale(backend, cfg):
    rt = get_runtime(backend)
    rows, cols, sld, scol = cfg
    rng = np.random.RandomState(rows)
    x = rng.normal(size=(rows, cols)).astype(f32)
    s = rng.uniform(100, 400, size=(rows, sld)).astype(f32)
    factor = f32(1.0 / 3.0)
    whole, out = canaried(rt, rows * cols)
    ops.rowscale(rt, rt.upload(x), rt.upload(s), scol, factor, out, rows, cols)(rt.stream)
    rt.synchronize()
    assert_bits_equal(out.get(), R.rowscale_f32(x, s, scol, factor).ravel())
    assert canary_ok(whole, rows * cols)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('cfg', [(3, 5, 7, 2, 3), (2, 8, 8, 8, 8), (1, 9, 6, 1, 1), (2, 128, 128, 64, 64)])
def test_crop_center(backend, cfg):
    rt = get_runtime(backend)
    B, H, W, h, w = cfg
    src = np.random.RandomState(H).normal(size=(B, H, W)).astype(f32)
    whole, dst = canaried(rt, B * h * w)
    ops.crop_center(rt, rt.upload(src), B, H, W, dst, h, w)(rt.stream)
    rt.synchronize()
    assert_bits_equal(dst.get(), R.crop_center(src, h, w).ravel())
    assert canary_ok(whole, B * h * w)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('hw', [(6, 5), (5, 8), (6, 8)])
def test_crop_center_refuses_a_window_larger_than_the_image(backend, hw):
    rt = get_runtime(backend)
    B, H, W = 2, 5, 7
    dst = rt.upload(np.full(B * 8 * 8, 7.0, f32))
    with pytest.raises(DppError):
        ops.crop_center(rt, rt.upload(np.ones((B, H, W), f32)), B, H, W, dst, hw[0], hw[1])(rt.stream)
    rt.synchronize()
    assert (dst.get() == 7.0).all()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('cfg', [(7, 5, 9, 11), (1, 1, 2, 3), (300, 7, 8, 10), (3, 4, 4, 6)])
def test_copy2d(backend, cfg):
    rt = get_runtime(backend)
    rows, cols, lds, ldd = cfg
    rng = np.random.RandomState(rows)
    src = rng.normal(size=(rows, lds)).astype(f32)
    src[rng.uniform(size=src.shape) < 0.2] = -0.0
    src[:, cols:] = np.nan                               # source columns beyond `cols` are not read
    for relu in (False, True):
        dst0 = np.full((rows, ldd), SENTINEL, np.uint32)
        db = rt.upload(dst0.view(f32))
        ops.copy2d(rt, rt.upload(src), lds, db, ldd, rows, cols, relu=relu)(rt.stream)
        rt.synchronize()
        got = db.get().reshape(rows, ldd)
        assert (bits(got)[:, cols:] == SENTINEL).all()   # destination columns beyond `cols` are untouched
        if relu:
            np.testing.assert_array_equal(got[:, :cols], np.maximum(src[:, :cols], 0))
            assert not np.signbit(got[:, :cols][src[:, :cols] < 0]).any()
        else:
            assert_bits_equal(got[:, :cols], src[:, :cols])       # -0.0 stays -0.0


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('n', [1, GRID_CAP + 259])
def test_scale_and_relu_bwd(backend, n):
    rt = get_runtime(backend)
    rng = np.random.RandomState(n % 1000)
    pre = rng.normal(size=n).astype(f32)
    pre[::5] = 0.0
    pre[1::5] = -0.0
    if n == 1:
        pre[0] = -1.5
    dy = rng.normal(size=n).astype(f32)
    mask = (rng.uniform(size=n) < 0.7).astype(f32)
    a = f32(0.7)
    pb, dyb, mb = rt.upload(pre), rt.upload(dy), rt.upload(mask)
    outs = [canaried(rt, n) for _ in range(5)]
    o = [v for (_, v) in outs]
    ops.scale(rt, pb, o[0], n, a=a)(rt.stream)
    ops.scale(rt, pb, o[1], n, a=a, relu=True)(rt.stream)
    ops.scale(rt, pb, o[2], n, relu=True, mask=mb)(rt.stream)
    ops.relu_bwd(rt, dyb, pb, o[3], n, a=a)(rt.stream)
    ops.relu_bwd(rt, dyb, pb, o[4], n, mask=mb)(rt.stream)
    rt.synchronize()
    assert_bits_equal(o[0].get(), a * pre)
    np.testing.assert_array_equal(o[1].get(), a * np.maximum(pre, 0))
    np.testing.assert_array_equal(o[2].get(), mask * np.maximum(pre, 0))
    # [pre >= 0]: the gradient passes at +0.0 and at -0.0
    np.testing.assert_array_equal(o[3].get(), np.where(pre >= 0, dy * a, f32(0)))
    np.testing.assert_array_equal(o[4].get(), np.where(pre >= 0, dy * mask, f32(0)))
    assert all(canary_ok(whole, n) for (whole, _) in outs)


@pytest.mark.parametrize('backend', BACKENDS)
def test_relu_bwd_passes_the_gradient_at_both_zeros(backend):
    rt = get_runtime(backend)
    pre = np.array([0.0, -0.0, 1e-45, -1e-45, 2.0, -2.0], f32)
    dy = np.arange(1, 7).astype(f32)
    g = rt.alloc(6, zero=False)
    ops.relu_bwd(rt, rt.upload(dy), rt.upload(pre), g, 6)(rt.stream)
    rt.synchronize()
    np.testing.assert_array_equal(g.get(), [1, 2, 3, 0, 5, 0])


# ======================================================================================================================
# 6. job-table launches: a workgroup finds its job from the block offsets
# ======================================================================================================================
BN_JOBS = [1, 30, 255, 256, 257, 512, 64]


def _bn_job_data(Cs):
    rng = np.random.RandomState(31)
    return [tuple(rng.normal(size=Cc).astype(f32) for _ in range(3)) for Cc in Cs]


def _bn_single(rt, data):
    """ops.bn_eval_coeffs per job: [(mean, inv_std, scale)] as arrays."""
    res = []
    for (gamma, rm, ris) in data:
        Cc = gamma.size
        o = [rt.alloc(Cc, zero=False) for _ in range(3)]
        ops.bn_eval_coeffs(rt, rt.upload(gamma), rt.upload(rm), rt.upload(ris), Cc, *o)(rt.stream)
        rt.synchronize()
        res.append(tuple(b.get() for b in o))
    return res


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('order', ['listed', 'reversed', 'each alone'])
def test_bn_eval_coeffs_multi(backend, order):
    rt = get_runtime(backend)
    data = _bn_job_data(BN_JOBS)
    single = _bn_single(rt, data)
    for (gamma, rm, ris), (mean, inv_std, scale) in zip(data, single):
        assert_bits_equal(mean, rm)
        assert_bits_equal(inv_std, ris)
        assert_bits_equal(scale, gamma * ris)
    idx = list(range(len(BN_JOBS)))
    groups = {'listed': [idx], 'reversed': [idx[::-1]], 'each alone': [[i] for i in idx]}[order]
    for group in groups:
        jobs, outs = [], []
        for i in group:
            gamma, rm, ris = data[i]
            o = [canaried(rt, gamma.size) for _ in range(3)]
            outs.append(o)
            jobs.append((rt.upload(gamma), rt.upload(rm), rt.upload(ris), gamma.size) + tuple(v for (_, v) in o))
        ops.bn_eval_coeffs_multi(rt, jobs)(rt.stream)
        rt.synchronize()
        for i, o in zip(group, outs):
            for k in range(3):
                assert_bits_equal(o[k][1].get(), single[i][k])
                assert canary_ok(o[k][0], BN_JOBS[i])


WT_JOBS = [(16, 16), (1, 1), (32, 16), (3, 5), (64, 64)]        # 16 x 9 x 16 = 2304 = 9 x 256: ends exactly on a block boundary


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('order', ['listed', 'reversed', 'each alone'])
def test_conv3x3_wtrans_multi(backend, order):
    rt = get_runtime(backend)
    rng = np.random.RandomState(32)
    data = [rng.normal(size=(Co, 9, Ci)).astype(f32) for (Co, Ci) in WT_JOBS]
    single = []
    for Wk in data:
        Co, _, Ci = Wk.shape
        wd = rt.alloc(Wk.size, zero=False)
        ops.conv3x3_wtrans(rt, rt.upload(Wk), Co, Ci, wd)(rt.stream)
        rt.synchronize()
        single.append(wd.get())
        assert_bits_equal(single[-1], R.wtrans(Wk).ravel())
    idx = list(range(len(WT_JOBS)))
    groups = {'listed': [idx], 'reversed': [idx[::-1]], 'each alone': [[i] for i in idx]}[order]
    for group in groups:
        outs = [canaried(rt, data[i].size) for i in group]
        jobs = [(rt.upload(data[i]), WT_JOBS[i][0], WT_JOBS[i][1], o[1]) for i, o in zip(group, outs)]
        ops.conv3x3_wtrans_multi(rt, jobs)(rt.stream)
        rt.synchronize()
        for i, o in zip(group, outs):
            assert_bits_equal(o[1].get(), single[i])
            assert canary_ok(o[0], data[i].size)
