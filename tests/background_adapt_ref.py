"""NumPy restatement of the background model kept current while tracking (csrc/background.hip: frame_background_adapt_kernel;
hipdp.ops.BackgroundModel with adapt=; additive to ABI v25).  The reference has no counterpart: this file IS the definition the kernel
is pinned to, bit for bit.  tests/background_ref.py (cut_map / apply / partials) is imported and left as it is.

  state      beside near / seen / cut, per source and pixel, in their layout:
             cand  float32, a depth that may become the new background (0: none)
             run   int32, the number of consecutive adapting ticks that supported it
  options    persist (ticks, an int >= max(2, min_seen)), guard (pixels, an int >= 0), every (ticks, an int >= 1; the host's)
  band(x)    float32(margin + float32(rel * x)): the roundings of cut_map, step by step

One tick of one source with frame f (float32, behind the ingest, before the cut):
  1 cut        out = (f != 0 and f < cut) ? f : 0, with the cut AS IT STOOD BEFORE THIS TICK: exactly background_ref.apply
  2 take == 0  the source does not adapt in this tick: nothing else happens
  3 protected  a pixel inside a window (xstart, ystart, cw, ch) of a track on this source, dilated by guard on every side --
               x in [xstart - guard, xstart + cw + guard), y likewise; cw <= 0 or ch <= 0 protects nothing:
               cand = 0, run = 0; near, seen and cut untouched
  4 holes      f == 0: nothing changes
  5 confirm    near != 0 and float32(near - band(near)) <= f <= float32(near + band(near)):
               near = f where f < near; seen += 1 (saturating at 2^31 - 1); cand = 0, run = 0
  6 candidate  anything else (nearer than the model, behind it, or the model unknown):
               cand != 0 and float32(cand - band(cand)) <= f <= float32(cand + band(cand)):  cand = f where f < cand, run += 1
               otherwise:  cand = f, run = 1
               run >= persist:  near = cand, seen = run, cand = 0, run = 0 -- the model is replaced (a new object is absorbed, a
               removed one recedes)
  7 cut map    where a pixel confirmed or was replaced, cut = cut_map(near, seen) of that pixel.  With cut == cut_map(near, seen)
               before the tick, cut == cut_map(near, seen) after it, everywhere.  The new cut applies from the next tick on.

A source that sits a tick out has its stale, already masked frame cut again, now possibly by a newer cut: apply(apply(f, cut0), cut1).
The host never lets such a source adapt (take = 0 without a fresh frame), so a masked frame is never learned from; Source.tick models
exactly that when handed frame=None."""
import numpy as np

from tests import background_ref as G

INT_MAX = np.int32(2 ** 31 - 1)


def band(x, margin, rel):
    x = np.asarray(x, np.float32)
    prod = (np.float32(rel) * x).astype(np.float32)
    return (np.float32(margin) + prod).astype(np.float32)


def in_band(f, ref, margin, rel):
    """ref != 0 and float32(ref - band(ref)) <= f <= float32(ref + band(ref))"""
    ref = np.asarray(ref, np.float32)
    b = band(ref, margin, rel)
    return (ref != 0) & (f >= (ref - b).astype(np.float32)) & (f <= (ref + b).astype(np.float32))


def protected(shape, windows, guard):
    """The (H, W) mask of the windows [(xstart, ystart, cw, ch), ...] dilated by guard, clipped to the frame."""
    H, W = shape
    m = np.zeros((H, W), bool)
    for xs, ys, cw, ch in windows:
        if cw <= 0 or ch <= 0:
            continue
        x0, x1, y0, y1 = max(xs - guard, 0), min(xs + cw + guard, W), max(ys - guard, 0), min(ys + ch + guard, H)
        if x0 < x1 and y0 < y1:
            m[y0:y1, x0:x1] = True
    return m


def tick(f, near, seen, cand, run, cut, take, windows, spec, persist, guard):
    """One tick of one source: (H, W) arrays in, (out, near, seen, cand, run, cut) out, new arrays.  spec = (margin, rel, min_seen);
    windows: the (xstart, ystart, cw, ch) of the tracks that read this source, as the previous tick left them."""
    margin, rel, min_seen = spec
    f = np.asarray(f, np.float32)
    near, cand, cut = np.array(near, np.float32), np.array(cand, np.float32), np.array(cut, np.float32)
    seen, run = np.array(seen, np.int32), np.array(run, np.int32)
    out = G.apply(f, cut)                                                            # 1
    if not take:                                                                     # 2
        return out, near, seen, cand, run, cut
    prot = protected(f.shape, windows, guard)                                        # 3
    cand[prot], run[prot] = 0, 0
    live = ~prot & (f != 0)                                                          # 4
    confirm = live & in_band(f, near, margin, rel)                                   # 5
    lower = confirm & (f < near)
    near[lower] = f[lower]
    up = confirm & (seen < INT_MAX)
    seen[up] += 1
    cand[confirm], run[confirm] = 0, 0
    other = live & ~confirm                                                          # 6
    cont = other & in_band(f, cand, margin, rel)
    lower = cont & (f < cand)
    cand[lower] = f[lower]
    run[cont] += 1
    start = other & ~cont
    cand[start], run[start] = f[start], 1
    replace = other & (run >= persist)
    near[replace], seen[replace] = cand[replace], run[replace]
    cand[replace], run[replace] = 0, 0
    changed = confirm | replace                                                      # 7
    cut[changed] = G.cut_map(near, seen, margin, rel, min_seen)[changed]
    return out, near, seen, cand, run, cut


def launch(frames, cut, near, seen, cand, run, take, windows, src, spec, persist, guard):
    """One dpp_frame_background_adapt launch over per-source lists (or (B, H, W) arrays): windows [T] of (xstart, ystart, cw, ch),
    src [T] (None: track t reads frame t).  Returns the six per-source lists (out, cut, near, seen, cand, run)."""
    B = len(frames)
    res = []
    for b in range(B):
        mine = [w for t, w in enumerate(windows) if (t if src is None else src[t]) == b]
        o, n, s, c, r, k = tick(frames[b], near[b], seen[b], cand[b], run[b], cut[b], take[b], mine, spec, persist, guard)
        res.append((o, k, n, s, c, r))
    return [list(x) for x in zip(*res)]


class Source(object):
    """The model of one source over ticks, as the tracker drives it: tick(frame or None, take, windows) -> the masked frame."""

    def __init__(self, shape, spec, persist, guard, near=None, seen=None):
        self.spec, self.persist, self.guard = spec, persist, guard
        self.near = np.zeros(shape, np.float32) if near is None else np.array(near, np.float32)
        self.seen = np.zeros(shape, np.int32) if seen is None else np.array(seen, np.int32)
        self.cand, self.run = np.zeros(shape, np.float32), np.zeros(shape, np.int32)
        self.cut = G.cut_map(self.near, self.seen, *spec)
        self.frame = None                                                            # what the source's frame buffer holds

    def tick(self, frame, take, windows):
        if frame is None:                                                            # the stale, masked frame, cut again; never learned from
            frame, take = self.frame, 0
        self.frame, self.near, self.seen, self.cand, self.run, self.cut = tick(
            frame, self.near, self.seen, self.cand, self.run, self.cut, take, windows, self.spec, self.persist, self.guard)
        return self.frame


def case(rng, B, H, W, persist=3):
    """State and frames for the kernel tests: background_ref.case's model and frames (holes, depths around the cut), random cand / run,
    and frames moved exactly onto, one ulp inside and one ulp outside both edges of the band of near and of cand.
    Returns (frames, near, seen, cand, run, cut, spec)."""
    f, near, seen, spec = G.case(rng, B, H, W)
    margin, rel, min_seen = spec
    f32 = np.float32
    cand = rng.uniform(300., 1600., (B, H, W)).astype(f32)
    run = rng.randint(1, persist, (B, H, W)).astype(np.int32)
    none = rng.uniform(size=(B, H, W)) < 0.4
    cand[none], run[none] = 0., 0
    w = rng.uniform(size=(B, H, W))
    holes = f == 0
    for k, (ref, side) in enumerate([(near, -1), (near, 1), (cand, -1), (cand, 1)]):
        b = band(ref, margin, rel)
        edge = (ref + f32(side) * b).astype(f32)
        for j, v in enumerate([edge, np.nextafter(edge, f32(0.)), np.nextafter(edge, f32(np.inf))]):
            m = (ref != 0) & ~holes & (w >= (3 * k + j) * 0.05) & (w < (3 * k + j + 1) * 0.05) & (v > 0)
            f[m] = v[m]
    near_on = (near != 0) & ~holes & (w >= 0.6) & (w < 0.65)                          # and some right on the model / the candidate
    f[near_on] = near[near_on]
    cand_on = (cand != 0) & ~holes & (w >= 0.65) & (w < 0.7)
    f[cand_on] = cand[cand_on]
    return f, near, seen, cand, run, G.cut_map(near, seen, *spec), spec
