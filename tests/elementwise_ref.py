"""NumPy references for the train-step tail kernels of csrc/elementwise.hip (fused split-K reduction + cost, ADAM, the weight-decay
regulariser, the scalar-target cost, the monitors, the copy / scale helpers), used by tests/test_elementwise.py.

Two rules.  Whatever the C ABI takes as `float` (alpha, factor, 1 / denom) is rounded to float32 before it is used; sums are float64.
Where a kernel's arithmetic has one rounding order and no multiply-add a compiler may contract, the reference is a float32 restatement
of that order and the test compares bit for bit."""
import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24          # unit round-off of float32 (round to nearest): |fl(x) - x| <= U |x|


# ---- fused reduction + cost ------------------------------------------------------------------------------------------
def reduce_partials_f32(partial, bias=None):
    """out[i] = ((0 + p[0][i]) + p[1][i]) + ... + p[nz-1][i], then + bias[i % nbias]: float32, rounded after every addition.
    partial [nz][n] float32, bias [nbias] float32 or None."""
    partial = np.asarray(partial, f32)
    s = np.zeros(partial.shape[1], f32)
    for z in range(partial.shape[0]):
        s = (s + partial[z]).astype(f32)
    if bias is not None:
        bias = np.asarray(bias, f32)
        s = (s + bias[np.arange(s.size) % bias.size]).astype(f32)
    return s


def dout_f32(out, y, denom):
    """(2 * (1 / denom)) * (out - y), every operation in float32 (a product of a constant and a difference: nothing to contract)."""
    k = f32(f32(2.0) * (f32(1.0) / f32(denom)))
    return (k * (np.asarray(out, f32).ravel() - np.asarray(y, f32).ravel()).astype(f32)).astype(f32)


def cost_f64(out, y, denom):
    d = np.asarray(out, f64).ravel() - np.asarray(y, f64).ravel()
    return float((d * d).sum() / denom)


# ---- scalar-target cost: the (B, B) matrix o_i - y_j ----------------------------------------------------------------
def loss_bcast_f64(o, y):
    """cost, dout [B], mean |o_i - y_j|, max |o_i - y_j| of the pairwise matrix, float64."""
    o, y = np.asarray(o, f64).ravel(), np.asarray(y, f64).ravel()
    P = o[:, None] - y[None, :]
    return float((P * P).mean()), 2.0 / o.size * (o - y.mean()), float(np.abs(P).mean()), float(np.abs(P).max())


def error_l2_f64(out, y):
    """mean and max over the rows of sqrt(sum_d (out - y)^2)."""
    e = np.sqrt(((np.asarray(out, f64) - np.asarray(y, f64)) ** 2).sum(1))
    return float(e.mean()), float(e.max())


# ---- ADAM -----------------------------------------------------------------------------------------------------------
def rmsprop_step_f32(w, ms, g, lr, decay, eps):
    """The float32 restatement test_loss_colsum_adam_elementwise uses for the RMSProp branch; returns (w, ms)."""
    lr, decay, eps = f32(lr), f32(decay), f32(eps)
    ms = (decay * ms + f32(f32(1) - decay) * (g * g)).astype(f32)
    return (w + (-lr * g) / np.maximum(np.sqrt(ms), eps)).astype(f32), ms


def adam_updates_f64(grads, lr, beta1=0.9, beta2=0.999, epsilon=1e-8):
    """The ADAM updates u_t = lr * (m_t / (1 - beta1^t)) / (sqrt(v_t / (1 - beta2^t)) + eps), t = 1, 2, ... from m = v = 0, exact
    recurrences in float64 on the float32-rounded constants (gamma = float32(1 - 1e-8) = 1: beta1 does not decay)."""
    lr, b1, b2, eps = (f64(f32(z)) for z in (lr, beta1, beta2, epsilon))
    m = np.zeros(grads[0].shape, f64)
    v = np.zeros(grads[0].shape, f64)
    out = []
    for t, g in enumerate(grads, 1):
        g = np.asarray(g, f64)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * (g * g)
        out.append(lr * (m / (1.0 - b1 ** t)) / (np.sqrt(v / (1.0 - b2 ** t)) + eps))
    return out


def adam_update_relerr(t, powf_ulp, beta1=0.9, beta2=0.999):
    """First-order bound, in units of 1, on the relative error of the float32 update u_t of a kernel that evaluates the expression of
    adam_updates_f64 operation by operation (division and square root correctly rounded, a multiply-add contracted or not), for
    gradients of ONE sign per element, so that m and v are sums of positive terms and nothing cancels:
      m_t = fl(b1 m + fl((1-b1) g))           dm_t <= dm_{t-1} + 2U          -> 2 t U       (1 - b1 is exact: Sterbenz)
      v_t = fl(fl(b2 v) + fl((1-b2) fl(g g))) dv_t <= max(dv_{t-1} + U, 2U) + U -> (t + 2) U
      c_k = fl(1 - powf(beta_k, t))           dc_k <= beta_k^t / (1 - beta_k^t) * powf_ulp * 2U + U
            (an ulp is at most 2U relative; the subtraction turns the ABSOLUTE error of the power into a relative error of 1 - power,
             which is what amplifies it: by 999 for beta2 = 0.999 at t = 1, by 499 at t = 2)
      u_t = fl(fl(lr fl(m / c1)) / fl(fl(sqrt(fl(v / c2))) + eps))
            du_t <= (dm + dc1 + U) + U + ((dv + dc2 + U) / 2 + U) + U + U."""
    b1, b2 = f64(f32(beta1)), f64(f32(beta2))
    dm, dv = 2.0 * t * U, (t + 2.0) * U
    dc1 = b1 ** t / (1.0 - b1 ** t) * powf_ulp * 2.0 * U + U
    dc2 = b2 ** t / (1.0 - b2 ** t) * powf_ulp * 2.0 * U + U
    return (dm + dc1 + U) + U + ((dv + dc2 + U) / 2.0 + U) + U + U


# ---- helpers --------------------------------------------------------------------------------------------------------
def rowscale_f32(x, s, scol, factor):
    """x * (s[:, scol] * factor): the product s * factor is formed (and rounded) first."""
    k = (np.asarray(s, f32)[:, scol] * f32(factor)).astype(f32)
    return (np.asarray(x, f32) * k[:, None]).astype(f32)


def crop_center(src, h, w):
    H, W = src.shape[1:]
    y0, x0 = int(H / 2. - h / 2.), int(W / 2. - w / 2.)
    return src[:, y0:y0 + h, x0:x0 + w]


def wtrans(Wk):
    """Wd[c][8 - t][o] = Wk[o][t][c] for Wk [Co][9][Ci]."""
    return np.ascontiguousarray(Wk[:, ::-1, :].transpose(2, 1, 0))
