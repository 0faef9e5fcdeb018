"""NumPy restatement of finding SEVERAL hands of one frame (csrc/components.hip: comp_candidates, detect_select, detect_seeds;
hipdp/detect.py with hands=K), built on tests/detect_ref.py and tests/track_ref.py.  Per frame:

  1. candidates: the components of slab_keys with count > 200, ordered by (key, root);
  2. extent filter (optional): a candidate with (xmax - xmin + 1) * hi / fx > max_extent or the same in y is removed, hi = the far
     bound of its slab, float64 in that order;
  3. greedy selection: in order, a candidate whose centroid lies in the seed window [xs, xe) x [ys, ye) of an ACCEPTED candidate is
     suppressed (and suppresses nothing), any other is accepted, until K are;
  4. seeds: per accepted candidate what detect (handdetector.py:589-607) computes for its one winner;
  5. centres: refineCoMIterative(5) of every seed with the frame's cube; a zero seed stops at once with status 1.
"""
import numpy as np

from oracle import augment as A
from tests import detect_ref as D
from tests import track_ref

REPORT = ('key', 'count', 'xmin', 'xmax', 'ymin', 'ymax')


def _window(c, n):
    return int(max(c - 100, 0)), int(min(c + 100, n - 1))            # handdetector.py:595-598


def seed_ref(frame, dpt, b, key, cx, cy, mn, mx):
    """detect's seed (:595-607) from the component of slab `key` with centroid (cx, cy): float32 [3]."""
    H, W = frame.shape
    (xstart, xend), (ystart, yend) = _window(cx, W), _window(cy, H)
    cropped = dpt[ystart:yend, xstart:xend].copy()
    cd = cropped.astype(np.float64)
    cropped[(cd < b[key]) | (cd > b[key + 1])] = 0.
    com = A.calculate_com(cropped, mn, mx)
    if np.allclose(com, 0.) and cropped.size:
        com[2] = cropped[cropped.shape[0] // 2, cropped.shape[1] // 2]
    com[0] += xstart
    com[1] += ystart
    return com.astype(np.float32)


def find_hands_ref(frame, cube, fx, fy, K, max_extent=None):
    """One frame: dict(seed (K, 3) f32, com (K, 3) f32, found (K,) bool, refine_status (K,) int, report: name -> (K,) int, stats)."""
    frame = np.asarray(frame, np.float32)
    H, W = frame.shape
    fx, fy = abs(float(fx)), abs(float(fy))
    mn, mx = D.depth_range(frame)
    keys = D.slab_keys_ref(frame)
    st = D.stats_ref(keys, D.labels_ref(keys))
    b = D.slab_bounds(mn, mx)
    cand = [i for i in np.lexsort((st['root'], st['key'])) if st['count'][i] > D.MIN_AREA]
    if max_extent:
        kept = []
        for i in cand:
            hi = b[st['key'][i] + 1]
            ex = np.float64(st['xmax'][i] - st['xmin'][i] + 1) * hi / np.float64(fx)
            ey = np.float64(st['ymax'][i] - st['ymin'][i] + 1) * hi / np.float64(fy)
            if not (ex > max_extent or ey > max_extent):
                kept.append(i)
        cand = kept
    accepted, windows = [], []
    for i in cand:
        if len(accepted) == K:
            break
        n = np.float64(st['count'][i])
        cx, cy = int(np.rint(np.float64(st['sum_x'][i]) / n)), int(np.rint(np.float64(st['sum_y'][i]) / n))
        if any(xs <= cx < xe and ys <= cy < ye for xs, xe, ys, ye in windows):
            continue
        accepted.append((i, cx, cy))
        windows.append(_window(cx, W) + _window(cy, H))
    dpt = frame.copy()
    dpt[(dpt > mx) | (dpt < mn)] = 0.
    out = dict(seed=np.zeros((K, 3), np.float32), com=np.zeros((K, 3), np.float32), found=np.zeros(K, bool),
               refine_status=np.ones(K, np.int32), report=dict((n, np.zeros(K, np.int32)) for n in REPORT), stats=st)
    cube = tuple(float(c) for c in np.float32(cube))
    for k, (i, cx, cy) in enumerate(accepted):
        seed = seed_ref(frame, dpt, b, int(st['key'][i]), cx, cy, mn, mx)
        fin, status = track_ref.refine_com_iterative(dpt, seed.astype(np.float64), 5, cube, fx, fy, mn, mx)
        out['seed'][k], out['com'][k], out['found'][k], out['refine_status'][k] = seed, fin.astype(np.float32), True, status
        for n in REPORT:
            out['report'][n][k] = st[n][i]
    return out
