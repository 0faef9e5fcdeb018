"""The restatement of dpp_extrinsics_accumulate (csrc/calib.hip, ABI v21) in NumPy float64, written from the statement of its semantics
in include/dpp_hip.h: the lanes' joint strides, the orders of the additions and the xor butterfly given there.  The semantics are this
project's own (the reference has one camera); the kernel is pinned to this file bit for bit by tests/test_calib.py."""
import numpy as np

from tests.fuse_ref import dist, to_world

OK = 0
WAVE, SLOTS = 64, 20
f64 = np.float64


def butterfly(v, op=np.add):
    """v [64, ...]: off = 32 .. 1: v[l] = op(v[l], v[l ^ off]) for all lanes at once; every lane ends with the same bits."""
    v = np.array(v, f64)
    lanes = np.arange(WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        v = op(v, v[lanes ^ off])
    assert (v == v[0]).all() or np.isnan(v).any()
    return v[0]


def pair_of(ms, src, anchor, c):
    a = [m for m in ms if src[m] == anchor]
    m = [m for m in ms if src[m] == c]
    return (a[0] if a else None), (m[0] if m else None)


def shape_deviations(p, q):
    """dev_j of the shape gate for one pair: p, q [J][3] float64 (q in the world frame)."""
    J = len(p)
    sp, sq = np.zeros((WAVE, 3), f64), np.zeros((WAVE, 3), f64)
    for j in range(J):
        sp[j % WAVE] = sp[j % WAVE] + p[j]
        sq[j % WAVE] = sq[j % WAVE] + q[j]
    pc, qc = butterfly(sp) / f64(J), butterfly(sq) / f64(J)
    return np.array([abs(dist(p[j], pc) - dist(q[j], qc)) for j in range(J)], f64)


def shape_worst(dev):
    worst = np.zeros(WAVE, f64)
    for j, d in enumerate(dev):
        worst[j % WAVE] = np.fmax(worst[j % WAVE], d)
    return butterfly(worst, np.fmax)


def accumulate(acc, pose3d, status, src, extr, groups, anchor, cal_src, max_shape_dev=None):
    """One launch: returns the new accumulator [n_cal][20]; `acc` is not changed."""
    acc = np.array(acc, f64).reshape(len(cal_src), SLOTS)
    pose3d = np.asarray(pose3d, np.float32)
    J = pose3d.shape[1]
    for k, c in enumerate(cal_src):
        v = np.zeros((WAVE, 18), f64)
        pairs, refused = f64(0.), f64(0.)
        for ms in groups:
            a, m = pair_of(ms, src, anchor, c)
            if a is None or m is None or status[a] != OK or status[m] != OK:
                continue
            p = pose3d[m].astype(f64)
            q = np.array([to_world(extr[anchor], pose3d[a, j]) for j in range(J)], f64)
            if max_shape_dev is not None:
                if not shape_worst(shape_deviations(p, q)) <= max_shape_dev:
                    refused = refused + f64(1.)
                    continue
            pairs = pairs + f64(1.)
            for j in range(J):
                l = v[j % WAVE]
                l[0] = l[0] + f64(1.)
                for d in range(3):
                    l[1 + d] = l[1 + d] + p[j, d]
                for d in range(3):
                    l[4 + d] = l[4 + d] + q[j, d]
                for d in range(3):
                    for e in range(3):
                        l[7 + 3 * d + e] = l[7 + 3 * d + e] + p[j, d] * q[j, e]
                l[16] = l[16] + ((p[j, 0] * p[j, 0] + p[j, 1] * p[j, 1]) + p[j, 2] * p[j, 2])
                l[17] = l[17] + ((q[j, 0] * q[j, 0] + q[j, 1] * q[j, 1]) + q[j, 2] * q[j, 2])
        acc[k, :18] = acc[k, :18] + butterfly(v)
        acc[k, 18] = acc[k, 18] + pairs
        acc[k, 19] = acc[k, 19] + refused
    return acc
