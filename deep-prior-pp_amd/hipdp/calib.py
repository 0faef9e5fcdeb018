"""
The host half of calibrating a camera's extrinsics from the tracked hand (ABI v21; this project's own, see include/dpp_hip.h).

While a MultiTracker calibrates, dpp_extrinsics_accumulate (csrc/calib.hip) adds every tick's joint pairs -- p in the camera's own frame,
q the same joint as the anchor camera sees it, taken to the world frame -- to one row of running sums per camera.  solve_rigid turns such a
row into the (R, t) with w = R p + t that fits the pairs best in the least-squares sense (Kabsch / Umeyama without scale).  It runs once
per calibration on a 3 x 3 matrix: NumPy float64 on the host is the right tool, there is no device solver.
"""
import numpy as np

SLOTS = 20          # DPP_CALIB_SLOTS: n, sum p [3], sum q [3], S [3][3] (S[d][e] = sum p_d q_e), sum |p|^2, sum |q|^2, pairs, refused


def solve_rigid(acc_row, min_cond=0.):
    """One accumulator row -> dict(R, t, n, pairs, refused, rms, cond, ok).

    S_c = S - sum p sum q^T / n; U, s, Vt = svd(S_c); d = sign(det(Vt^T U^T)); R = Vt^T diag(1, 1, d) U^T; t = q_mean - R p_mean.
    rms (mm): the root of the mean squared residual |R p + t - q|^2, from the sums alone:
        rms^2 = (sum |p - p_mean|^2 + sum |q - q_mean|^2 - 2 (s1 + s2 + d s3)) / n, clamped at 0.
    cond = s2 / s1: joints on one line leave the rotation about that line open (s2 = 0, up to the rounding of S_c: cond is then 0).
    ok is False for n < 3, s2 == 0 or cond < min_cond; R, t are then the identity and zero, or the (unreliable) fit where one exists.
    No threshold is built in: the project has measured none."""
    a = np.asarray(acc_row, np.float64).reshape(-1)
    if a.size != SLOTS:
        raise ValueError("an accumulator row has %d entries, not %d" % (SLOTS, a.size))
    n = a[0]
    out = dict(R=np.eye(3), t=np.zeros(3), n=int(n), pairs=int(a[18]), refused=int(a[19]), rms=float('nan'), cond=0., ok=False)
    if not (np.isfinite(a).all() and n >= 1.):
        return out
    sp, sq, S = a[1:4], a[4:7], a[7:16].reshape(3, 3)
    pm, qm = sp / n, sq / n
    Sc = S - np.outer(sp, sq) / n
    U, s, Vt = np.linalg.svd(Sc)
    d = 1. if np.linalg.det(Vt.T.dot(U.T)) >= 0. else -1.
    Rm = Vt.T.dot(np.diag([1., 1., d])).dot(U.T)
    var_p, var_q = a[16] - sp.dot(sp) / n, a[17] - sq.dot(sq) / n
    rms2 = max(0., (var_p + var_q - 2. * (s[0] + s[1] + d * s[2])) / n)
    # "s2 == 0" as far as float64 can tell: S_c is a difference of sums of the size of S, each entry good to a few ulp of THAT size, so
    # a singular value below that noise is a zero (exactly collinear joints come out at 1e-16 of |S|, not at 0.0)
    noise = 32. * np.finfo(np.float64).eps * max(np.abs(S).max(), np.abs(np.outer(sp, sq)).max() / n)
    cond = float(s[1] / s[0]) if s[1] > noise else 0.
    out.update(R=Rm, t=qm - Rm.dot(pm), rms=float(np.sqrt(rms2)), cond=cond, ok=bool(n >= 3. and cond > 0. and cond >= min_cond))
    return out
