"""NumPy restatement of whole-frame hand detection by connected components (csrc/components.hip, hipdp/detect.py): what
HandDetector.detect and estimateHandsize (/root/reference/src/util/handdetector.py:569-632, :911-937) take from cv2.findContours,
defined order-free.  Pure NumPy; scipy.ndimage.label is a cross-check where it imports (labels_crosscheck), never a dependency.
float64 wherever the kernels' definition says float64; the refinement step is tests/track_ref.refine_com_iterative."""
import numpy as np

from oracle import augment as A
from tests import track_ref

BG = 255
STEPS = 20                 # handdetector.py:576
MIN_AREA = 200             # :587, in pixels here
FOUND, NO_SIZE = 1, 2


def labels_ref(keys):
    """labels[y, x] = smallest linear index y * W + x of the pixel's 8-connected component of equal key, -1 for key 255: the minimum
    is propagated over equal-key 8-neighbours until nothing changes."""
    keys = np.asarray(keys, np.uint8)
    H, W = keys.shape
    big = np.int64(H) * W
    lab = np.where(keys != BG, np.arange(H * W, dtype=np.int64).reshape(H, W), big)
    kp = np.pad(keys.astype(np.int16), 1, constant_values=-1)
    same = [(dy, dx, kp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == keys) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
    fg = keys != BG
    while True:
        lp = np.pad(lab, 1, constant_values=big)
        new = lab
        for dy, dx, eq in same:
            new = np.where(eq & fg, np.minimum(new, lp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]), new)
        # pointer jumping: a pixel also takes its label's label (same component), which shortens long chains
        flat = new.reshape(-1)
        jump = np.where(flat < big, flat[np.minimum(flat, big - 1)], big).reshape(H, W)
        new = np.minimum(new, jump)
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(fg, lab, -1).astype(np.int32)


def labels_crosscheck(keys, labels):
    """Where scipy imports: the partition of scipy.ndimage.label (8-connectivity, per key) is the partition of `labels`."""
    try:
        from scipy import ndimage
    except ImportError:
        return False
    keys = np.asarray(keys)
    for k in np.unique(keys[keys != BG]):
        lab, n = ndimage.label(keys == k, structure=np.ones((3, 3), int))
        for c in range(1, n + 1):
            m = lab == c
            assert np.unique(labels[m]).size == 1 and labels[m][0] == np.flatnonzero(m.reshape(-1))[0]
    return True


def stats_ref(keys, labels):
    """Per component, ordered by root: root, key, count, xmin, xmax, ymin, ymax, sum_x, sum_y (exact integers)."""
    H, W = labels.shape
    flat = labels.reshape(-1)
    roots = np.flatnonzero(flat == np.arange(H * W))
    yy, xx = np.divmod(np.arange(H * W, dtype=np.int64), W)
    out = dict((n, []) for n in ('root', 'key', 'count', 'xmin', 'xmax', 'ymin', 'ymax', 'sum_x', 'sum_y'))
    for r in roots:
        m = flat == r
        x, y = xx[m], yy[m]
        for n, v in (('root', r), ('key', np.asarray(keys).reshape(-1)[r]), ('count', m.sum()), ('xmin', x.min()), ('xmax', x.max()),
                     ('ymin', y.min()), ('ymax', y.max()), ('sum_x', x.sum()), ('sum_y', y.sum())):
            out[n].append(int(v))
    return dict((n, np.asarray(v, np.int64)) for n, v in out.items())


def depth_range(frame):
    """The detector's range as float32 (handdetector.py:57-58)."""
    frame = np.asarray(frame, np.float32)
    return np.float32(max(np.float32(10), frame.min())), np.float32(min(np.float32(1500), frame.max()))


def slab_bounds(min_depth, max_depth):
    """The 21 bounds b_i = minDepth + i * (maxDepth - minDepth) / 20 in float64 from the float32 range (:577-581)."""
    mn, mx = np.float64(np.float32(min_depth)), np.float64(np.float32(max_depth))
    return np.array([mn + i * (mx - mn) / 20. for i in range(STEPS + 1)], np.float64)


def slab_keys_ref(frame):
    """key = the smallest i with b_i <= d <= b_{i+1} (compared, never divided); 255 for d == 0, d < minDepth, d > maxDepth."""
    frame = np.asarray(frame, np.float32)
    mn, mx = depth_range(frame)
    b = slab_bounds(mn, mx)
    d = frame.astype(np.float64)
    keys = np.full(frame.shape, BG, np.uint8)
    ok = (frame != 0) & (frame >= mn) & (frame <= mx)
    for i in range(STEPS - 1, -1, -1):
        keys[ok & (b[i] <= d) & (d <= b[i + 1])] = i
    return keys


def find_hand_ref(frame, cube, fx, fy):
    """detect (handdetector.py:576-610) on components: (seed float32 [3], final centre float32 [3], found, winning key, stats)."""
    frame = np.asarray(frame, np.float32)
    H, W = frame.shape
    mn, mx = depth_range(frame)
    keys = slab_keys_ref(frame)
    st = stats_ref(keys, labels_ref(keys))
    big = st['count'] > MIN_AREA
    if not big.any():
        return np.zeros(3, np.float32), np.zeros(3, np.float32), False, None, st           # :632
    key = st['key'][big].min()
    i = np.flatnonzero(big & (st['key'] == key))[0]                                          # raster-first: smallest root
    n = np.float64(st['count'][i])
    cx, cy = int(np.rint(np.float64(st['sum_x'][i]) / n)), int(np.rint(np.float64(st['sum_y'][i]) / n))      # :591-592
    xstart, xend = int(max(cx - 100, 0)), int(min(cx + 100, W - 1))                          # :595-598
    ystart, yend = int(max(cy - 100, 0)), int(min(cy + 100, H - 1))
    b = slab_bounds(mn, mx)
    dpt = frame.copy()                                                                       # the constructor's zeroing, :60-61
    dpt[(dpt > mx) | (dpt < mn)] = 0.
    cropped = dpt[ystart:yend, xstart:xend].copy()
    cd = cropped.astype(np.float64)
    cropped[(cd < b[key]) | (cd > b[key + 1])] = 0.                                          # :601-602, float64 bounds
    com = A.calculate_com(cropped, mn, mx)                                                   # :603, float64 sums
    if np.allclose(com, 0.) and cropped.size:
        com[2] = cropped[cropped.shape[0] // 2, cropped.shape[1] // 2]                       # :604-605
    com[0] += xstart
    com[1] += ystart
    seed = com.astype(np.float32)
    fin, _ = track_ref.refine_com_iterative(dpt, seed.astype(np.float64), 5, tuple(float(c) for c in np.float32(cube)), fx, fy, mn, mx)   # :610
    return seed, fin.astype(np.float32), True, int(key), st


def handsize_ref(frame, com, cube, fx, fy, tol=0.):
    """detect's part_ref (:616-624) + estimateHandsize (:920-935) on components, raw frame, float32 centre: (cube float32 [3], status)."""
    frame = np.asarray(frame, np.float32)
    com = np.asarray(com, np.float32).astype(np.float64)
    cube = np.asarray(cube, np.float32)
    zlo, zhi = com[2] - np.float64(cube[2]) / 2., com[2] + np.float64(cube[2]) / 2.
    d = frame.astype(np.float64)
    keys = np.where((frame != 0) & (zlo <= d) & (d <= zhi), 0, BG).astype(np.uint8)
    st = stats_ref(keys, labels_ref(keys))
    if st['count'].size == 0:
        return cube.copy(), FOUND | NO_SIZE
    i = np.flatnonzero(st['count'] == st['count'].max())[0]                                   # largest; ties: smallest root
    w, h = int(st['xmax'][i] - st['xmin'][i] + 1), int(st['ymax'][i] - st['ymin'][i] + 1)   # cv2.boundingRect of the outer contour
    xstart = (com[0] - w / 2.) * com[2] / fx                                                 # :928-935
    xend = (com[0] + w / 2.) * com[2] / fx
    ystart = (com[1] - h / 2.) * com[2] / fy
    yend = (com[1] + h / 2.) * com[2] / fy
    szx = xend - xstart
    szy = yend - ystart
    sz = (szx + szy) / 2.
    return np.array((sz + tol, sz + tol, sz + tol), np.float64).astype(np.float32), FOUND
