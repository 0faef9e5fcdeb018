"""The restatement of dpp_pose_smooth (csrc/smooth.hip, ABI v22) in NumPy float64, written from the statement of its semantics in
include/dpp_hip.h: the One-Euro filter (Casiez, Roussel, Vogel, CHI 2012) over T track rows and G group rows, the orders of evaluation
given there, every output rounded to float32 once.  The semantics are this project's own (the reference draws what the net returns);
the kernel is pinned to this file bit for bit by tests/test_smooth.py."""
import numpy as np

from tests.fuse_ref import to_img

TRACK_OK = 0
OK, INIT, HELD, EMPTY, DROPPED = 1, 2, 4, 8, 16
f64, f32 = np.float64, np.float32
TWO_PI = f64(6.283185307179586)


def alpha(fc, Te):
    r = (TWO_PI * f64(fc)) * f64(Te)
    return r / (r + f64(1.0))


class State(object):
    """since [R] int32 (-1: empty), xh / dxh [R][J][3] float64 -- what the device holds, updated in place by smooth()."""

    def __init__(self, R, J, fill=0.0):
        self.since = np.full(R, -1, np.int32)
        self.xh, self.dxh = np.full((R, J, 3), fill, f64), np.full((R, J, 3), fill, f64)

    def copy(self):
        s = State(*self.xh.shape[:2])
        s.since, s.xh, s.dxh = self.since.copy(), self.xh.copy(), self.dxh.copy()
        return s


def row(x, valid, r, st, rate, mincutoff, beta, dcutoff, max_hold):
    """One row of one tick: updates st's row r in place, returns (word, the row's filtered output as float32 [J][3])."""
    x = np.asarray(x, f32)
    J = x.shape[0]
    since = int(st.since[r])
    zero = np.zeros((J, 3), f32)
    if valid and since < 0:
        st.xh[r], st.dxh[r], st.since[r] = x.astype(f64), 0.0, 0
        return INIT, st.xh[r].astype(f32)
    if valid:
        Te = f64(since + 1) / f64(rate)
        ad = alpha(dcutoff, Te)
        for j in range(J):
            for d in range(3):
                dv = (f64(x[j, d]) - st.xh[r, j, d]) / Te
                st.dxh[r, j, d] = ad * dv + (f64(1.0) - ad) * st.dxh[r, j, d]
            v = st.dxh[r, j]
            speed = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            a = alpha(f64(mincutoff) + f64(beta) * speed, Te)
            for d in range(3):
                st.xh[r, j, d] = a * f64(x[j, d]) + (f64(1.0) - a) * st.xh[r, j, d]
        st.since[r] = 0
        return OK, st.xh[r].astype(f32)
    if since < 0:
        return EMPTY, zero
    if since + 1 > max_hold:
        st.since[r] = -1
        return EMPTY | DROPPED, zero
    st.since[r] = since + 1
    return HELD, st.xh[r].astype(f32)


def smooth(pose3d, status, src, cams, fused_pose, n, st, rate, mincutoff, beta, dcutoff=1.0, max_hold=0):
    """All outputs of one launch; `st` (a State of T + G rows) is updated in place.  cams: per source (fx, fy, ux, uy, flip_y); src:
    per track its source (None: cams[0] for every track); fused_pose / n: None or the G group samples and their member counts."""
    pose3d = np.asarray(pose3d, f32)
    T, J = pose3d.shape[:2]
    G = 0 if fused_pose is None else len(fused_pose)
    par = (rate, mincutoff, beta, dcutoff, max_hold)
    out = dict(pose_f=np.zeros((T, J, 3), f32), pose_img_f=np.zeros((T, J, 3), f32), sstat=np.zeros(T, np.int32),
               fused_pose_f=np.zeros((G, J, 3), f32), gstat=np.zeros(G, np.int32))
    for t in range(T):
        w, o = row(pose3d[t], status[t] == TRACK_OK, t, st, *par)
        out['sstat'][t], out['pose_f'][t] = w, o
        if not w & EMPTY:
            cam = cams[0 if src is None else src[t]]
            out['pose_img_f'][t] = [to_img(cam, o[j]) for j in range(J)]
    for g in range(G):
        w, o = row(fused_pose[g], n[g] >= 1, T + g, st, *par)
        out['gstat'][g], out['fused_pose_f'][g] = w, o
    return out
