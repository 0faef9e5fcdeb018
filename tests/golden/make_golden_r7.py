#!/usr/bin/env python3
"""
Round-7 additions to the golden fixtures (run in the build container only; make_golden.py has the rules: the reference is IMPORTED
here, the fixtures hold inputs and the reference's OUTPUTS, never its source).

  resize.npz   the reference's own HandDetector.bilinearResize (/root/reference/src/util/handdetector.py:132-202) and
               HandDetector.getInverseCrop (:298-334) with resizeMethod = RESIZE_BILINEAR, executed here on seeded inputs:
                 bl_*   bilinearResize cases: 0-4 undefined taps in every corner position, the all-weights-zero case, up- and
                        down-scaling, non-square sizes, a non-zero ND value;
                 inv_*  getInverseCrop cases: windows inside the frame, leaving it on every side, z-threshold on / off, a non-zero
                        background, and the three early returns (window left / above, right / below, zero width or height).

NumPy 1 arithmetic.  The reference ran on NumPy 1, where `float32 scalar * Python float` is a float64; on NumPy 2 (this container)
the same expression is a float32.  Every source handed to bilinearResize is therefore widened to float64 first -- for the direct
calls here, and inside getInverseCrop through an instance attribute that wraps the reference's static method the same way.  The
output array of bilinearResize is float32 in either case (one rounding on store).

getNDValue stand-in.  getInverseCrop asks self.getNDValue(), which calls `stats.mode(...)[0][0]`; on SciPy 1.15 `mode` returns
scalars and that indexing fails.  The instance's getNDValue is replaced by a function returning a FIXED value (`inv_nd` in the
fixture); the value is what the reference would return for a frame whose most frequent out-of-range depth it is.  Everything else
that runs is the reference's code.

applyCrop3D and cropArea3D are NOT run from the reference: their Python-2 integer divisions change meaning
under the lib2to3 import.  The tests compose them from the pieces pinned here and in crop.npz.
"""
import os
import sys

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True


def _taps_cases(rng):
    """Sources with undefined depth (nd) sprinkled so that every 2x2 tap pattern occurs, plus hand-built corner cases."""
    cases = []
    for (sh, sw), (dw, dh), nd, p in (((12, 10), (23, 17), 0., 0.35), ((12, 10), (5, 7), 0., 0.35), ((9, 16), (16, 9), 32001., 0.3),
                                       ((20, 20), (7, 31), 0., 0.5), ((6, 5), (11, 12), 0., 0.25), ((33, 17), (13, 13), 0., 0.15)):
        src = rng.uniform(300., 900., (sh, sw)).astype(numpy.float32)
        src[rng.uniform(size=(sh, sw)) < p] = nd
        cases.append((src, (dw, dh), nd))
    # the all-weights-zero case: the sample point (0, 0) lies on the source grid (x_diff = y_diff = 0) and its top two taps are
    # undefined -- numND = 2, both remaining weights are 0 -> ND
    src = rng.uniform(300., 900., (5, 5)).astype(numpy.float32)
    src[0, 0] = src[0, 1] = 0.
    cases.append((src, (8, 8), 0.))
    # every one of the 16 ND patterns of a single 2x2 cell, on an off-grid sample point
    for m in range(16):
        src = rng.uniform(300., 900., (2, 2)).astype(numpy.float32)
        for k in range(4):
            if m >> k & 1:
                src[k // 2, k % 2] = 0.
        cases.append((src, (3, 3), 0.))
    return cases


def _inverse_cases(rng):
    H, W = 40, 52
    out = []
    for (ch, cw), (xs, xe, ys, ye), thresh, bg in (
            ((16, 16), (10, 30, 8, 28), True, 0.),        # inside, upscaled
            ((16, 16), (-6, 14, -5, 15), True, 0.),       # leaves the frame left / top
            ((16, 16), (40, 60, 30, 50), True, 0.),       # leaves it right / bottom
            ((12, 20), (5, 15, 3, 9), False, 0.),         # downscaled, non-square, no threshold
            ((16, 16), (4, 44, 2, 38), True, 700.),       # non-zero background (thresholded too)
            ((16, 16), (-30, -5, 3, 20), True, 0.),       # early return: entirely left
            ((16, 16), (3, 20, -30, -2), True, 0.),       # early return: entirely above
            ((16, 16), (60, 80, 3, 20), True, 0.),        # early return: entirely right
            ((16, 16), (3, 20, 45, 70), True, 0.),        # early return: entirely below
            ((16, 16), (10, 10, 3, 20), True, 700.),      # early return: zero width
            ((16, 16), (3, 20, 7, 7), True, 0.)):         # early return: zero height
        crop = rng.uniform(450., 750., (ch, cw)).astype(numpy.float32)
        crop[rng.uniform(size=(ch, cw)) < 0.2] = 0.
        crop[rng.uniform(size=(ch, cw)) < 0.05] = 380.       # nearer than the cube
        crop[rng.uniform(size=(ch, cw)) < 0.05] = 900.       # farther than the cube
        out.append((crop, (H, W), (xs, xe, ys, ye, 475., 725.), thresh, bg))
    return out


def make_resize():
    import make_golden as G                                    # placeholder modules, numpy.cast shim, REF on sys.path
    hd_mod = sys.modules.get('util.handdetector') or G.load_py2_module('util.handdetector', 'util/handdetector.py')
    HD = hd_mod.HandDetector
    rng = numpy.random.RandomState(707)
    d = {}
    cases = _taps_cases(rng)
    d['bl_n'] = numpy.array(len(cases))
    for i, (src, dsize, nd) in enumerate(cases):
        d['bl_src_%d' % i], d['bl_dsize_%d' % i], d['bl_nd_%d' % i] = src, numpy.array(dsize), numpy.float32(nd)
        d['bl_out_%d' % i] = HD.bilinearResize(src.astype(numpy.float64), dsize, nd)
    # the reference refuses a source narrower than 2 pixels
    try:
        HD.bilinearResize(numpy.ones((4, 1)), (3, 3), 0.)
        raise AssertionError("no Shape mismatch")
    except UserWarning:
        pass
    inv_nd = 0.
    hd = HD(rng.uniform(400., 800., (40, 52)).astype(numpy.float32), 241.42, 241.42)
    hd.resizeMethod = HD.RESIZE_BILINEAR
    hd.getNDValue = lambda: inv_nd                              # stand-in, see the header
    hd.bilinearResize = lambda src, dsize, nd: HD.bilinearResize(numpy.asarray(src, numpy.float64), dsize, nd)
    inv = _inverse_cases(rng)
    d['inv_n'], d['inv_nd'] = numpy.array(len(inv)), numpy.float32(inv_nd)
    for i, (crop, sz, b, thresh, bg) in enumerate(inv):
        d['inv_crop_%d' % i], d['inv_sz_%d' % i], d['inv_bounds_%d' % i] = crop, numpy.array(sz), numpy.array(b, numpy.float64)
        d['inv_thresh_%d' % i], d['inv_bg_%d' % i] = numpy.array(thresh), numpy.float32(bg)
        d['inv_out_%d' % i] = hd.getInverseCrop(crop, sz, int(b[0]), int(b[1]), int(b[2]), int(b[3]), b[4], b[5], thresh_z=thresh, background=bg)
    numpy.savez_compressed(os.path.join(HERE, 'resize.npz'), **d)
    return d


if __name__ == '__main__':
    out = make_resize()
    print('resize.npz:', len(out), 'arrays,', os.path.getsize(os.path.join(HERE, 'resize.npz')), 'bytes')
