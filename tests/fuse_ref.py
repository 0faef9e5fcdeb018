"""The restatement of dpp_pose_fuse (csrc/fuse.hip, ABI v20) in NumPy float64, written from the statement of its semantics in
include/dpp_hip.h: the orders of evaluation given there, every output rounded to float32 once.  The semantics are this project's own
(the reference has one camera); the kernel is pinned to this file bit for bit by tests/test_fuse.py."""
import numpy as np

OK, LOST, IDLE = 0, 1, 2
USED, OUTLIER, DISAGREE, PEER_OK, HANDED = 1, 2, 4, 8, 16
f64, f32 = np.float64, np.float32


def to_world(e, p):
    """w = R p + t; e = 12 float64 (R row-major, t); row i is ((R_i0 x + R_i1 y) + R_i2 z) + t_i."""
    x, y, z = f64(p[0]), f64(p[1]), f64(p[2])
    return np.array([((e[3 * i] * x + e[3 * i + 1] * y) + e[3 * i + 2] * z) + e[9 + i] for i in range(3)], f64)


def to_camera(e, w):
    """p = R^T (w - t): d = w - t, row i is (R_0i d0 + R_1i d1) + R_2i d2."""
    d = [f64(w[i]) - e[9 + i] for i in range(3)]
    return np.array([(e[i] * d[0] + e[3 + i] * d[1]) + e[6 + i] * d[2] for i in range(3)], f64)


def dist(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def to_img(cam, p):
    """importer.joint3DToImg of a float32 sample: the two quotients are float32 divisions, the rest float64, stored as float32."""
    fx, fy, ux, uy, flip = cam
    p = np.asarray(p, f32)
    if p[2] == 0.:
        return np.array([ux, uy, 0.], f32)
    q0, q1 = f64(p[0] / p[2]), f64(p[1] / p[2])
    return np.array([q0 * fx + ux, (uy - q1 * fy) if flip else (q1 * fy + uy), f64(p[2])], f32)


def ill_defined(c):
    return not np.all(np.isfinite(c)) or abs(f64(c[2])) <= 1e-8


def mean_of(ws):
    """The sum in list order from 0.0, divided by the count."""
    s = np.zeros(3, f64)
    for w in ws:
        s = s + w
    return s / f64(len(ws))


def median(vals):
    v = sorted(f64(x) for x in vals)
    n = len(v)
    return v[n // 2] if n & 1 else (v[n // 2 - 1] + v[n // 2]) / f64(2.)


def fuse(pose3d, com3d, status, src, extr, groups, cams, sizes, max_dev, handover, com):
    """All outputs of one launch.  cams: per source (fx, fy, ux, uy, flip_y); sizes: per source (H, W); extr [C][12] float64; com: the
    centres before the launch.  Tracks in no group: com untouched, peer_com and fstat as allocated (zero)."""
    pose3d, com3d = np.asarray(pose3d, f32), np.asarray(com3d, f32)
    T, J = pose3d.shape[:2]
    G = len(groups)
    out = dict(com=np.array(com, f32), fused_pose=np.zeros((G, J, 3), f32), fused_com=np.zeros((G, 3), f32), spread=np.zeros((G, J), f32),
               n=np.zeros(G, np.int32), peer_com=np.zeros((T, 3), f32), fstat=np.zeros(T, np.int32))
    for g, ms in enumerate(groups):
        contrib = [m for m in ms if status[m] == OK]
        W = dict((m, to_world(extr[src[m]], com3d[m])) for m in contrib)
        bits = dict((m, 0) for m in ms)
        inl = list(contrib)
        if max_dev is not None and len(contrib) >= 3:
            med = np.array([median([W[m][d] for m in contrib]) for d in range(3)], f64)
            for m in contrib:
                if dist(W[m], med) > max_dev:
                    bits[m] |= OUTLIER
            inl = [m for m in contrib if not bits[m] & OUTLIER]
        elif max_dev is not None and len(contrib) == 2:
            if dist(W[contrib[0]], W[contrib[1]]) > max_dev:
                bits[contrib[0]] |= DISAGREE
                bits[contrib[1]] |= DISAGREE
        n = len(inl)
        out['n'][g] = n
        if n:
            out['fused_com'][g] = mean_of([W[m] for m in inl])
            for j in range(J):
                wj = [to_world(extr[src[m]], pose3d[m, j]) for m in inl]
                mean = mean_of(wj)
                out['fused_pose'][g, j] = mean
                out['spread'][g, j] = max([f64(0.)] + [dist(w, mean) for w in wj])
        for m in ms:
            others = [W[q] for q in inl if q != m]
            pc, ok = np.zeros(3, f32), False
            if others:
                c = src[m]
                p = to_camera(extr[c], mean_of(others)).astype(f32)
                pc = to_img(cams[c], p)
                H, Wd = sizes[c]
                ok = bool(pc[2] > 0. and not ill_defined(pc) and 0. <= pc[0] < Wd and 0. <= pc[1] < H)
            out['peer_com'][m] = pc
            f = bits[m] | (USED if m in inl else 0) | (PEER_OK if ok else 0)
            if handover and ok and (status[m] == LOST or f & OUTLIER):
                out['com'][m] = pc
                f |= HANDED
            out['fstat'][m] = f
    return out
