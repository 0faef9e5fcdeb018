"""The restatement of dpp_pose_align (csrc/align.hip) and dpp_pose_smooth_t (csrc/smooth.hip), both ABI v24, in NumPy float64, written
from the statement of their semantics in include/dpp_hip.h: every track of a tick moved from its source's stamp to the tick's instant
along the velocity between its previous sample and this one, and the One-Euro filter of tests/smooth_ref.py over real elapsed time.  The
orders of evaluation are the ones given there; every output is rounded to float32 once.  The semantics are this project's own (the
reference has one camera); the kernels are pinned to this file bit for bit by tests/test_timing.py."""
import numpy as np

from tests import smooth_ref as S
from tests.fuse_ref import to_img

TRACK_OK = 0
NONE, MOVED, ASIS, NOPREV, GAP, FAR = 0, 1, 2, 4, 8, 16
STALE = 32
f64, f32 = np.float64, np.float32


class AlignState(object):
    """have [T] int32 (0: empty), pt [T] float64, pp [T][J][3] / pc [T][3] float32 -- what the device holds, updated in place."""

    def __init__(self, T, J, fill=0.0):
        self.have = np.zeros(T, np.int32)
        self.pt = np.full(T, fill, f64)
        self.pp, self.pc = np.full((T, J, 3), fill, f32), np.full((T, 3), fill, f32)

    def copy(self):
        s = AlignState(*self.pp.shape[:2])
        s.have, s.pt, s.pp, s.pc = self.have.copy(), self.pt.copy(), self.pp.copy(), self.pc.copy()
        return s


def moved(x, xp, dt, lead):
    """One coordinate: v = (x - xp) / dt, y = x + v * lead, each operation rounded to float64, the result to float32."""
    v = (f64(x) - f64(xp)) / dt
    return f32(f64(x) + v * lead)


def align(pose3d, com3d, status, src, cams, stamps, st, max_gap, max_lead):
    """All outputs of one launch; `st` is updated in place.  cams: per source (fx, fy, ux, uy, flip_y); src: per track its source (None:
    source 0 for every track); stamps: C + 1 float64, the last one `now`."""
    pose3d, com3d, stamps = np.asarray(pose3d, f32), np.asarray(com3d, f32), np.asarray(stamps, f64)
    T, J = pose3d.shape[:2]
    now = stamps[-1]
    out = dict(pose_t=np.zeros((T, J, 3), f32), pose_img_t=np.zeros((T, J, 3), f32), com3d_t=np.zeros((T, 3), f32), lead=np.zeros(T, f32),
               astat=np.zeros(T, np.int32))
    with np.errstate(all='ignore'):
        for t in range(T):
            if status[t] != TRACK_OK:
                continue                                                 # NONE: zeros, the state untouched
            c = 0 if src is None else int(src[t])
            ts = stamps[c]
            dt, lead = ts - st.pt[t], now - ts
            if not st.have[t]:
                word = ASIS | NOPREV
            elif not (dt > 0.0 and dt <= f64(max_gap)):
                word = ASIS | GAP
            elif not (np.abs(lead) <= f64(max_lead)):
                word = ASIS | FAR
            else:
                word = MOVED
            if word == MOVED:
                for j in range(J):
                    for d in range(3):
                        out['pose_t'][t, j, d] = moved(pose3d[t, j, d], st.pp[t, j, d], dt, lead)
                for d in range(3):
                    out['com3d_t'][t, d] = moved(com3d[t, d], st.pc[t, d], dt, lead)
            else:
                out['pose_t'][t], out['com3d_t'][t] = pose3d[t], com3d[t]
            out['pose_img_t'][t] = [to_img(cams[c], out['pose_t'][t, j]) for j in range(J)]
            out['lead'][t], out['astat'][t] = f32(lead), word
            st.have[t], st.pt[t], st.pp[t], st.pc[t] = 1, ts, pose3d[t], com3d[t]
    return out


class SmoothState(S.State):
    """smooth_ref's state and tlast [R] float64, the row's last sample time."""

    def __init__(self, R, J, fill=0.0):
        S.State.__init__(self, R, J, fill)
        self.tlast = np.full(R, fill, f64)

    def copy(self):
        s = SmoothState(*self.xh.shape[:2])
        s.since, s.xh, s.dxh, s.tlast = self.since.copy(), self.xh.copy(), self.dxh.copy(), self.tlast.copy()
        return s


def row_t(x, valid, r, st, s, mincutoff, beta, dcutoff, max_hold):
    """One row of one tick at sample time s: smooth_ref.row with Te = s - tlast.  smooth_ref.row forms its Te from since and rate (a
    rate of 1 / Te would round once more), so the OK branch is restated here with the same expressions; every other branch forms no Te
    and is smooth_ref.row's."""
    x = np.asarray(x, f32)
    J = x.shape[0]
    since = int(st.since[r])
    if valid and since >= 0:
        Te = f64(s) - st.tlast[r]
        if not Te > 0.0:                                                 # refused: the not-valid path, and the bit
            w, o = S.row(x, False, r, st, 1.0, mincutoff, beta, dcutoff, max_hold)
            return w | STALE, o
        ad = S.alpha(dcutoff, Te)
        for j in range(J):
            for d in range(3):
                dv = (f64(x[j, d]) - st.xh[r, j, d]) / Te
                st.dxh[r, j, d] = ad * dv + (f64(1.0) - ad) * st.dxh[r, j, d]
            v = st.dxh[r, j]
            speed = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            a = S.alpha(f64(mincutoff) + f64(beta) * speed, Te)
            for d in range(3):
                st.xh[r, j, d] = a * f64(x[j, d]) + (f64(1.0) - a) * st.xh[r, j, d]
        st.since[r], st.tlast[r] = 0, s
        return S.OK, st.xh[r].astype(f32)
    w, o = S.row(x, valid, r, st, 1.0, mincutoff, beta, dcutoff, max_hold)       # INIT, or not valid: no Te is formed
    if w == S.INIT:
        st.tlast[r] = s
    return w, o


def smooth_t(pose3d, status, src, cams, fused_pose, n, st, stamps, mincutoff, beta, dcutoff=1.0, max_hold=0, rate=None):
    """All outputs of one dpp_pose_smooth_t launch; `st` (a SmoothState of T + G rows) is updated in place.  Arguments as
    smooth_ref.smooth; stamps: C + 1 float64, the last one `now`.  `rate` is accepted and unread, as the trackers' spec carries it."""
    pose3d, stamps = np.asarray(pose3d, f32), np.asarray(stamps, f64)
    T, J = pose3d.shape[:2]
    G = 0 if fused_pose is None else len(fused_pose)
    par = (mincutoff, beta, dcutoff, max_hold)
    out = dict(pose_f=np.zeros((T, J, 3), f32), pose_img_f=np.zeros((T, J, 3), f32), sstat=np.zeros(T, np.int32),
               fused_pose_f=np.zeros((G, J, 3), f32), gstat=np.zeros(G, np.int32))
    for t in range(T):
        c = 0 if src is None else int(src[t])
        w, o = row_t(pose3d[t], status[t] == TRACK_OK, t, st, stamps[c], *par)
        out['sstat'][t], out['pose_f'][t] = w, o
        if not w & S.EMPTY:
            out['pose_img_f'][t] = [to_img(cams[c], o[j]) for j in range(J)]
    for g in range(G):
        w, o = row_t(fused_pose[g], n[g] >= 1, T + g, st, stamps[-1], *par)
        out['gstat'][g], out['fused_pose_f'][g] = w, o
    return out
