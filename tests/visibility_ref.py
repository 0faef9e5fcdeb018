"""The restatement of dpp_joint_visibility (csrc/visibility.hip) and of dpp_pose_fuse_w (csrc/fuse.hip), both ABI v23, in NumPy float64,
written from the statement of their semantics in include/dpp_hip.h: the comparisons and the orders of evaluation given there, every
float output rounded to float32 once.  The semantics are this project's own (the reference has nothing comparable); the kernels are
pinned to this file bit for bit by tests/test_visibility.py.  fuse_w extends tests/fuse_ref.py, whose helpers it imports: everything
but the fused joints, their spread and the fused weight is that file's fuse()."""
import math

import numpy as np

from tests import fuse_ref as F

TRACK_OK = 0
VISIBLE, OCCLUDED, UNSUPPORTED, OFFFRAME = 1, 2, 4, 8
f64, f32 = np.float64, np.float32


def joint(frame, u, v, z, radius, margin, min_support, hidden_weight):
    """One joint of an OK track against its source's frame [H][W]: (vis, weight, class)."""
    H, W = frame.shape
    if not (np.isfinite(u) and np.isfinite(v) and np.isfinite(z)) or not f64(z) > 0.:
        return f32(0.), f32(0.), OFFFRAME
    px, py = math.floor(f64(u) + f64(0.5)), math.floor(f64(v) + f64(0.5))       # Python ints of any size: compared before any use
    if not (0 <= px < W and 0 <= py < H):
        return f32(0.), f32(0.), OFFFRAME
    n_in = n_on = n_front = 0
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            x, y = px + dx, py + dy
            if not (0 <= x < W and 0 <= y < H):
                continue
            n_in += 1
            d = f64(frame[y, x])
            if d == 0.:
                continue
            e = d - f64(z)
            if e < -f64(margin):
                n_front += 1
            elif e > f64(margin):
                pass
            else:
                n_on += 1
    vis = f32(f64(n_on) / f64(n_in))
    if n_on >= min_support:
        return vis, f32(1.), VISIBLE
    return vis, f32(f64(hidden_weight)), OCCLUDED if n_front >= min_support else UNSUPPORTED


def visibility(pose_img, status, src, frames, radius, margin, min_support, hidden_weight=0.0):
    """All outputs of one launch.  frames: per source a float32 [H][W] array; src: per track its source."""
    pose_img = np.asarray(pose_img, f32)
    T, J = pose_img.shape[:2]
    out = dict(vis=np.zeros((T, J), f32), weight=np.zeros((T, J), f32), vword=np.zeros((T, J), np.int32))
    for t in range(T):
        if status[t] != TRACK_OK:
            continue
        fr = np.asarray(frames[src[t]], f32)
        for j in range(J):
            u, v, z = pose_img[t, j]
            out['vis'][t, j], out['weight'][t, j], out['vword'][t, j] = joint(fr, u, v, z, radius, margin, min_support, hidden_weight)
    return out


def fuse_w(pose3d, com3d, status, src, extr, groups, cams, sizes, max_dev, handover, com, weight):
    """dpp_pose_fuse_w: F.fuse's outputs with fused_pose and spread replaced by the weighted ones, and fused_weight [G][J].  The inliers
    of a group are the members with USED in F.fuse's fstat, in list order."""
    pose3d, weight = np.asarray(pose3d, f32), np.asarray(weight, f32)
    out = F.fuse(pose3d, com3d, status, src, extr, groups, cams, sizes, max_dev, handover, com)
    T, J = pose3d.shape[:2]
    out['fused_weight'] = np.zeros((len(groups), J), f32)
    for g, ms in enumerate(groups):
        inl = [m for m in ms if out['fstat'][m] & F.USED]
        assert len(inl) == out['n'][g]
        for j in range(J if inl else 0):
            wj = [F.to_world(extr[src[m]], pose3d[m, j]) for m in inl]
            sw, s = f64(0.), np.zeros(3, f64)
            for m, w in zip(inl, wj):
                sw = sw + f64(weight[m, j])
                s = s + f64(weight[m, j]) * w
            if sw > 0.:
                mean = s / sw
                out['fused_pose'][g, j] = mean
                out['spread'][g, j] = max([f64(0.)] + [F.dist(w, mean) for m, w in zip(inl, wj) if weight[m, j] > 0.])
                out['fused_weight'][g, j] = max(weight[m, j] for m in inl)
    return out
