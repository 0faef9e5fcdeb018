"""NumPy restatement of the learned-background semantics (csrc/background.hip, hipdp.ops.BackgroundModel; ABI v25).  The reference
has no counterpart: this file IS the definition the kernels and the host's cut map are pinned to, bit for bit.

  model      near  float32, the smallest non-zero depth seen while learning (0: none seen)
             seen  int32, the number of learning frames in which the pixel had a depth
  learning   for every pixel with f != 0:  near = (near == 0 or f < near) ? f : near;  seen += 1
  cut map    near - (margin + rel * near), every operation rounded to float32, where seen >= min_seen, near != 0 and the result is
             > 0; +inf elsewhere (no background known: every depth is foreground)
  applying   out = (f != 0 and f < cut) ? f : 0 -- strict: a depth exactly at cut is background

Written element by element where that is affordable and with explicit float32 temporaries otherwise, apart from the product's code."""
import numpy as np

FR_BANDS, THREADS = 64, 256             # frame_range's grid: the partials' layout
IDENT = (np.float32(3.4e38), np.float32(-3.4e38))
INF = np.float32(np.inf)


def learn(near, seen, frame):
    """One learning frame; returns new (near, seen)."""
    near, seen, f = np.array(near, np.float32), np.array(seen, np.int32), np.asarray(frame, np.float32)
    has = f != 0
    take = has & ((near == 0) | (f < near))
    near[take] = f[take]
    seen[has] += 1
    return near, seen


def cut_map(near, seen, margin, rel=0.0, min_seen=1):
    near = np.asarray(near, np.float32)
    prod = (np.float32(rel) * near).astype(np.float32)               # float32(rel * near)
    band = (np.float32(margin) + prod).astype(np.float32)            # float32(margin + .)
    cut = (near - band).astype(np.float32)                           # float32(near - .)
    out = np.full(near.shape, INF, np.float32)
    known = (np.asarray(seen) >= min_seen) & (near != 0) & (cut > 0)
    out[known] = cut[known]
    return out


def apply(frames, cut):
    f = np.asarray(frames, np.float32)
    out = np.zeros(f.shape, np.float32)
    keep = (f != 0) & (f < cut)
    out[keep] = f[keep]
    return out


def band_of(npx, vector):
    """The band (workgroup) that owns each of a frame's npx elements under frame_range's partition: thread t of FR_BANDS * THREADS
    takes the 16-byte groups (vector) or the single elements t, t + nt, ..."""
    i = np.arange(npx)
    unit = i // 4 if vector else i
    return (unit % (FR_BANDS * THREADS)) // THREADS


def partials(out, vector=None):
    """(B, FR_BANDS, 2): every band's (min, max) of the masked frames `out` (B, H, W); a band without elements has the identities.
    vector None: what a [B][H][W] buffer at a 16-byte aligned address gives -- 16-byte groups iff H * W is a multiple of 4."""
    B = out.shape[0]
    npx = out[0].size
    band = band_of(npx, npx % 4 == 0 if vector is None else vector)
    p = np.empty((B, FR_BANDS, 2), np.float32)
    p[:, :, 0], p[:, :, 1] = IDENT
    for b in range(B):
        flat = out[b].ravel()
        for k in np.unique(band):
            v = flat[band == k]
            p[b, k] = (v.min(), v.max())
    return p


def case(rng, B, H, W):
    """(frames, near, seen, cut spec) for the kernel tests: a model with regions never seen (+inf cut), seen too rarely, and known; frames
    with about 30 % zeros and depths exactly at, one ulp below and one ulp above their cut, the rest spread around it."""
    margin, rel, min_seen = 20., 0.01, 2
    near = rng.uniform(400., 1500., (B, H, W)).astype(np.float32)
    seen = rng.randint(2, 9, (B, H, W)).astype(np.int32)
    u = rng.uniform(size=(B, H, W))
    near[u < 0.1] = 0.
    seen[u < 0.1] = 0
    seen[(u >= 0.1) & (u < 0.2)] = 1                                  # below min_seen
    near[(u >= 0.2) & (u < 0.23)] = 10.                               # cut = 10 - 20.1 <= 0
    cut = cut_map(near, seen, margin, rel, min_seen)
    ref = np.where(np.isfinite(cut), cut, np.float32(900.)).astype(np.float32)
    f = (ref + rng.uniform(-300., 300., (B, H, W))).astype(np.float32)
    f = np.maximum(f, np.float32(1.))
    w = rng.uniform(size=(B, H, W))
    fin = np.isfinite(cut)
    at, below, above = fin & (w < 0.1), fin & (w >= 0.1) & (w < 0.2), fin & (w >= 0.2) & (w < 0.3)
    f[at] = cut[at]
    f[below] = np.nextafter(cut[below], np.float32(0.))
    f[above] = np.nextafter(cut[above], INF)
    f[rng.uniform(size=(B, H, W)) < 0.3] = 0.
    return f, near, seen, (margin, rel, min_seen)
