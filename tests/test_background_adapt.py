"""The background model kept current while tracking (csrc/background.hip: dpp_frame_background_adapt, additive to ABI v25; HandTracker /
MultiTracker / the pipelines with background=dict(..., adapt=dict(persist=, guard=, every=1))) against the NumPy restatement of
tests/background_adapt_ref.py, which is the definition: the reference has no counterpart.  Everything is comparisons, selects, integer
increments and three rounded float32 operations: every comparison here is np.array_equal.  The device tests run on the SIMT emulator
and, with -m gpu, on the card."""
import functools
import os
import re

import numpy as np
import pytest

from hipdp import lib, ops
from hipdp import runtime as R
from oracle import augment as A
from tests import background_adapt_ref as AD
from tests import background_ref as G
from tests.backends import BACKENDS, get_runtime
from tests.test_multitrack_sources import _pads, _ragged, _table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = 10001
SENTINEL = np.float32(-7.25)
INF = np.float32(np.inf)
f32, i32 = np.float32, np.int32
PERSIST = 3
# 16-byte groups that straddle rows (W = 10), an unaligned second frame (odd H * W: single elements), aligned groups, one column
SHAPES = [(2, 6, 10), (3, 37, 53), (3, 16, 64), (2, 5, 1)]
SRC_SIZES = [(37, 53), (5, 1), (64, 64)]
REC = np.dtype([(k, 'i4') for k in ('xstart', 'ystart', 'cw', 'ch', 'szw', 'szh', 'xs', 'ys')] + [('ifx', 'f8'), ('ify', 'f8')] +
               [(k, 'f4') for k in ('min_depth', 'max_depth', 'zstart', 'zend', 'far_v', 'norm_off', 'norm_div')], align=True)
NAMES = ('frames', 'cut', 'near', 'seen', 'cand', 'run')


def _sid(s):
    return 'x'.join(map(str, s))


def _spec(spec, persist=PERSIST, guard=0, **kw):
    return dict(margin=spec[0], rel=spec[1], min_seen=spec[2], adapt=dict(persist=persist, guard=guard, **kw))


# ---- 1: the restatement ------------------------------------------------------------------------------------------------------------
def _one(f, near, seen, cand=0., run=0, take=1, windows=(), persist=PERSIST, guard=0, spec=(20., 0.01, 2)):
    a = lambda v, t: np.array([[v]], t)
    cut = G.cut_map(a(near, f32), a(seen, i32), *spec)
    out = AD.tick(a(f, f32), a(near, f32), a(seen, i32), a(cand, f32), a(run, i32), cut, take, list(windows), spec, persist, guard)
    return tuple(x[0, 0] for x in out)


def test_restatement_hand_values():
    # band(1000) = 20 + 10 = 30: [970, 1030] confirms; the cut is 970
    out, near, seen, cand, run, cut = _one(990., 1000., 5, cand=600., run=2)
    assert (out, near, seen, cand, run) == (0., 990., 6, 0., 0) and cut == f32(f32(990.) - f32(f32(20.) + f32(f32(0.01) * f32(990.))))
    assert _one(1030., 1000., 5)[1:5] == (1000., 6, 0., 0) and _one(970., 1000., 5)[1:5] == (970., 6, 0., 0)       # both edges are inside
    assert _one(1020., 1000., 2 ** 31 - 1)[2] == 2 ** 31 - 1                                                      # seen saturates
    # a candidate starts (nearer, behind, or no model at all) ...
    assert _one(600., 1000., 5) == (600., 1000., 5, 600., 1, f32(970.))
    assert _one(1400., 1000., 5)[1:5] == (1000., 5, 1400., 1) and _one(600., 0., 0)[1:5] == (0., 0, 600., 1)
    # ... continues inside band(cand) = 26 and keeps the nearest depth ...
    assert _one(610., 1000., 5, cand=600., run=1)[1:5] == (1000., 5, 600., 2)
    assert _one(590., 1000., 5, cand=600., run=1)[1:5] == (1000., 5, 590., 2)
    # ... and replaces the model at persist; the new cut holds from the next tick on (600 itself is kept in this one)
    out, near, seen, cand, run, cut = _one(598., 1000., 5, cand=600., run=2)
    assert (out, near, seen, cand, run) == (598., 598., 3, 0., 0) and cut == G.cut_map(f32([598.]), i32([3]), 20., 0.01, 2)[0]
    assert _one(598., 1000., 5, cand=600., run=2, persist=4)[1:5] == (1000., 5, 598., 3)
    # a flicker starts over; a hole changes nothing; take == 0 changes nothing but the frame
    assert _one(800., 1000., 5, cand=600., run=2)[1:5] == (1000., 5, 800., 1)
    assert _one(0., 1000., 5, cand=600., run=2) == (0., 1000., 5, 600., 2, f32(970.))
    assert _one(990., 1000., 5, cand=600., run=2, take=0) == (0., 1000., 5, 600., 2, f32(970.))
    # protected: the candidate is dropped, the model is left alone -- also where the depth would have confirmed, also in a hole
    for f in (600., 990., 0.):
        assert _one(f, 1000., 5, cand=600., run=2, windows=[(0, 0, 1, 1)])[1:] == (1000., 5, 0., 0, f32(970.))
    assert _one(600., 1000., 5, cand=600., run=1, windows=[(1, 0, 1, 1)])[3:5] == (600., 2)                         # beside the window
    assert _one(600., 1000., 5, cand=600., run=1, windows=[(1, 0, 1, 1)], guard=1)[3:5] == (0., 0)                  # ... inside its guard
    assert _one(600., 1000., 5, cand=600., run=1, windows=[(0, 0, 0, 1)], guard=1)[3:5] == (600., 2)                # an empty window
    # recede: the object the model was learned with is gone, the wall behind it takes over after persist ticks
    near, seen, cand, run = f32(600.), i32(4), f32(0.), i32(0)
    for k in range(PERSIST):
        out, near, seen, cand, run, cut = _one(1400. + k, near, seen, cand, run)
        assert out == 0.                                                             # (behind the old cut: background all the while)
    assert (near, seen, cand, run) == (1400., 3, 0., 0) and cut == G.cut_map(f32([1400.]), i32([3]), 20., 0.01, 2)[0]
    # the kernel cases hold pixels where a contracted multiply-add, or float64 rounded once, gives another cut: bit-for-bit means no FMA
    f, near, seen, cand, run, cut, (margin, rel, min_seen) = _case((3, 37, 53))[:7]
    n64 = near.astype(np.float64)
    fma_band = (np.float64(f32(margin)) + np.float64(f32(rel)) * n64).astype(f32)
    known = np.isfinite(cut)
    assert ((near - fma_band).astype(f32) != cut)[known].any()
    assert ((n64 - (np.float64(f32(margin)) + np.float64(f32(rel)) * n64)).astype(f32) != cut)[known].any()
    assert np.array_equal(ops.background_cut(near, seen, (margin, rel, min_seen)), cut)
    # ... and depths on, one ulp inside and one ulp outside every band edge
    live = (f != 0)
    for ref in (near, cand):
        b = AD.band(ref, margin, rel)
        for edge in ((ref - b).astype(f32), (ref + b).astype(f32)):
            m = live & (ref != 0)
            assert (f[m] == edge[m]).sum() > 20 and (f[m] == np.nextafter(edge[m], INF)).sum() > 20
            assert (f[m] == np.nextafter(edge[m], f32(0.))).sum() > 20


# ---- 2, 3: one launch, bit for bit ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(shape):
    out = AD.case(np.random.RandomState(7 + sum(shape)), *shape, persist=PERSIST)
    for a in out[:6]:
        a.setflags(write=False)
    return out


def _windows(B, H, W):
    """(windows, src): partly outside the frame, two overlapping on source 0, one of source 1 that would cover all of source 0 (it
    must not protect there), an empty one, one pixel in a corner of the last source."""
    win = [(-2, -1, W // 2 + 2, H // 2 + 1), (W // 4, H // 4, W // 2 + 1, H // 2 + 1), (-5, -5, W + 10, 2 + 5), (0, 0, 0, H), (W - 1, H - 1, 4, 4)]
    return win, [0, 0, 1, 0, B - 1]


VARIANTS = {
    # name: (guard, take of source b, how the tracks are handed over)
    'ix-mixed': (0, lambda b, B: int(b != B - 1), 'ix'),
    'ix-guard3': (3, lambda b, B: 1, 'ix'),
    'null-src': (3, lambda b, B: int(b != 0), 'null'),
    'no-tracks': (0, lambda b, B: 1, 'T0'),
    'no-records': (3, lambda b, B: 1, 'norec'),
    'take-none': (3, lambda b, B: 0, 'ix'),
}


def _records(windows):
    rec = np.zeros(len(windows), REC)
    for t, (xs, ys, cw, ch) in enumerate(windows):
        rec[t]['xstart'], rec[t]['ystart'], rec[t]['cw'], rec[t]['ch'] = xs, ys, cw, ch
    return rec


def _model(rt, shape, spec, guard, state, persist=PERSIST, table=None):
    """A BackgroundModel holding `state` = (cut, near, seen, cand, run), (B, H, W) arrays or with a table ragged host buffers."""
    B, H, W = shape if table is None else (table.C, None, None)
    bg = ops.BackgroundModel(rt, _spec(spec, persist, guard), B, H, W, table=table)
    for buf, a in zip((bg.cut, bg.near, bg.seen, bg.cand, bg.run), state):
        buf.set(np.ascontiguousarray(a).reshape(-1))
    return bg


def _launch(rt, shape, frames, state, spec, guard, take, windows, src, how='ix', persist=PERSIST):
    """One dpp_frame_background_adapt on (B, H, W) arrays -> dict of the six buffers and the partials, as (B, H, W) / (B, bands, 2)."""
    B, H, W = shape
    assert REC.itemsize == rt.lib.dpp_crop_record_bytes()
    bg = _model(rt, shape, spec, guard, state, persist)
    fr, tk = rt.upload(frames), rt.upload(np.asarray(take, i32))
    rec = rt.upload(_records(windows).view(np.uint8)) if windows else rt.alloc(REC.itemsize, np.uint8)
    sr = rt.upload(np.asarray(src, i32)) if windows and how == 'ix' else None
    part = ops.frame_range_workspace(rt, B)
    part.set(np.full(part.size, SENTINEL, f32))
    T = 0 if how == 'T0' else len(windows)
    ops.frame_background_adapt(rt, fr, bg, tk, B, H, W, None if how == 'norec' else rec, T, sr, part)(rt.stream)
    rt.synchronize()
    got = dict(frames=fr.get())
    got.update((k, getattr(bg, k).get().reshape(shape)) for k in NAMES[1:])
    got['partial'] = part.get().reshape(B, -1, 2)
    return got


def _want(shape, frames, state, spec, guard, take, windows, src, persist=PERSIST):
    cut, near, seen, cand, run = state
    res = AD.launch(frames, cut, near, seen, cand, run, take, windows, src, spec, persist, guard)
    want = dict((k, np.stack(v)) for k, v in zip(NAMES, res))
    want['partial'] = G.partials(want['frames'])
    return want


def _variant(shape, name):
    B, H, W = shape
    f, near, seen, cand, run, cut, spec = _case(shape)
    guard, take_of, how = VARIANTS[name]
    take = [take_of(b, B) for b in range(B)]
    win, src = _windows(B, H, W)
    if how == 'null':                                           # track t reads frame t; the tracks beyond B read nothing
        eff_win, eff_src = win, list(range(len(win)))
    elif how in ('T0', 'norec'):
        eff_win, eff_src = [], []
    else:
        eff_win, eff_src = win, src
    return f, (cut, near, seen, cand, run), spec, guard, take, win, src, how, eff_win, eff_src


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', sorted(VARIANTS))
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_adapt_launch_bit_for_bit(backend, shape, name):
    """2 and 3: all six buffers and the partials against the restatement; frame and partials against dpp_frame_background with the
    pre-tick cut; where take == 0 every model bit as it was."""
    rt = get_runtime(backend)
    B, H, W = shape
    f, state, spec, guard, take, win, src, how, eff_win, eff_src = _variant(shape, name)
    got = _launch(rt, shape, f, state, spec, guard, take, win, src, how)
    want = _want(shape, f, state, spec, guard, take, eff_win, eff_src)
    for k in NAMES + ('partial',):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, shape, name)
    assert not (got['partial'] == SENTINEL).any()
    assert np.array_equal(got['cut'][np.array(take) == 1], G.cut_map(got['near'], got['seen'], *spec)[np.array(take) == 1])      # the invariant
    # the existing launch with the pre-tick cut
    fr, cu = rt.upload(f), rt.upload(state[0])
    part = ops.frame_range_workspace(rt, B)
    ops.frame_background(rt, fr, cu, B, H, W, part)(rt.stream)
    rt.synchronize()
    assert np.array_equal(got['frames'], fr.get()) and np.array_equal(got['partial'], part.get().reshape(B, -1, 2))
    for b in range(B):
        if not take[b]:
            for k, a in zip(NAMES[1:], state):
                assert got[k][b].tobytes() == a[b].tobytes(), (k, b)
    if name == 'ix-guard3' and H > 10:                          # the case does what it is there for (at 6 x 10 guard 3 covers the frame)
        cut, near, seen, cand, run = state
        prot = AD.protected((H, W), [w for w, s in zip(win, src) if s == 0], guard)
        assert prot.any() and not prot.all() and (cand[0][prot] != 0).any() and not got['cand'][0][prot].any()
        assert np.array_equal(got['near'][0][prot], near[0][prot])
        other = AD.protected((H, W), [win[2]], guard)                                  # source 1's window protects nothing of source 0
        assert (got['near'][0][other & ~prot] != near[0][other & ~prot]).any()
        assert (got['seen'] > seen).any() and ((got['run'] == 0) & (run == PERSIST - 1) & (got['seen'] == PERSIST)).any()    # confirmed; replaced


@pytest.mark.parametrize('backend', BACKENDS)
def test_more_windows_on_a_source_than_the_workgroup_keeps(backend):
    """T is any number: 70 one-pixel windows on source 0 (and one of source 1 between them) protect exactly their pixels."""
    rt = get_runtime(backend)
    shape = (2, 12, 10)
    f, near, seen, cand, run, cut, spec = _case(shape)
    win = [(t % 10, t // 10, 1, 1) for t in range(70)]
    src = [0] * 70
    win[5], src[5] = (0, 8, 10, 4), 1
    state = (cut, near, seen, cand, run)
    got = _launch(rt, shape, f, state, spec, 0, [1, 1], win, src)
    want = _want(shape, f, state, spec, 0, [1, 1], win, src)
    for k in NAMES + ('partial',):
        assert np.array_equal(got[k], want[k]), k
    assert not got['cand'][0].ravel()[:70][np.arange(70) != 5].any() and got['cand'][0].ravel()[70:].any() and not got['cand'][1, 8:].any()


@pytest.mark.parametrize('backend', BACKENDS)
def test_adapt_unaligned_model_keeps_the_partition(backend):
    """H * W a multiple of 4, frame and cut map aligned, the model one element off a 16-byte boundary: the 16-byte groups of the cut
    (its partials) with the model read by elements, and not a byte outside the arrays."""
    rt = get_runtime(backend)
    shape = (1, 6, 10)
    f, near, seen, cand, run, cut, spec = _case((2, 6, 10))
    f, near, seen, cand, run, cut = (a[:1] for a in (f, near, seen, cand, run, cut))
    n = f.size
    bg = ops.BackgroundModel(rt, _spec(spec, PERSIST, 1), 1, 6, 10)
    bufs = {}
    for k, a, off in (('near', near, 1), ('seen', seen, 2), ('cand', cand, 3), ('run', run, 1)):
        bufs[k] = rt.upload(np.full(n + 8, 77, a.dtype))
        view = bufs[k].view(off, (n,), a.dtype)
        view.set(a.reshape(-1))
        setattr(bg, k, view)
    bg.cut.set(cut.reshape(-1))
    fr, tk = rt.upload(f), rt.upload(np.ones(1, i32))
    win = [(2, 1, 3, 3)]
    rec = rt.upload(_records(win).view(np.uint8))
    part = ops.frame_range_workspace(rt, 1)
    ops.frame_background_adapt(rt, fr, bg, tk, 1, 6, 10, rec, 1, None, part)(rt.stream)
    rt.synchronize()
    want = _want(shape, f, (cut, near, seen, cand, run), spec, 1, [1], win, [0])
    assert np.array_equal(fr.get(), want['frames']) and np.array_equal(bg.cut.get().reshape(shape), want['cut'])
    assert np.array_equal(part.get().reshape(1, -1, 2), G.partials(want['frames'], vector=True))
    for k, off in (('near', 1), ('seen', 2), ('cand', 3), ('run', 1)):
        host = bufs[k].get()
        assert np.array_equal(host[off:off + n].reshape(shape), want[k]), k
        assert np.all(host[:off] == 77) and np.all(host[off + n:] == 77), k


# ---- 4: the invariant over a scripted sequence -----------------------------------------------------------------------------------------
def _script():
    """8 ticks of a 6 x 10 frame in front of a wall at 1400 mm: (frames, near, seen, windows per tick).  Columns 0-1: an object (500 mm)
    appears in tick 1 and stays; columns 3-4: an object (700 mm) that was learned is gone; pixel (5, 6) flickers between the wall and
    900 mm; columns 7-9, rows 0-2: a hand (600 mm) rests under a window all the time."""
    rng = np.random.RandomState(3)
    near, seen = np.full((6, 10), 1400., f32), np.full((6, 10), 3, i32)
    near[:, 3:5] = 700.
    near[0, 5], seen[0, 5] = 0., 0                                                   # never seen while learning
    frames = (np.full((8, 6, 10), 1400., f32) + rng.randint(-3, 4, (8, 6, 10)).astype(f32)).astype(f32)
    frames[1:, :, 0:2] = 500. + rng.randint(-2, 3, (7, 6, 2)).astype(f32)
    frames[::2, 5, 6] = 900.
    frames[:, 0:3, 7:10] = 600.
    frames[3, 2, 2] = 0.                                                            # a hole
    windows = [[(8, 0, 2, 2)]] * 8                                                   # with guard 1: columns 7 .. 9, rows 0 .. 2
    return frames, near, seen, windows


@pytest.mark.parametrize('backend', BACKENDS)
def test_invariant_over_a_scripted_sequence(backend):
    rt = get_runtime(backend)
    frames, near, seen, windows = _script()
    spec, shape = (20., 0.01, 2), (1, 6, 10)
    ref = AD.Source((6, 10), spec, PERSIST, 1, near, seen)
    bg = _model(rt, shape, spec, 1, (ref.cut, near, seen, ref.cand, ref.run))
    tk = rt.upload(np.ones(1, i32))
    part = ops.frame_range_workspace(rt, 1)
    for i in range(8):
        fr, rec = rt.upload(frames[i][None]), rt.upload(_records(windows[i]).view(np.uint8))
        ops.frame_background_adapt(rt, fr, bg, tk, 1, 6, 10, rec, 1, None, part)(rt.stream)
        rt.synchronize()
        want = ref.tick(frames[i], 1, windows[i])
        assert np.array_equal(fr.get()[0], want), i
        for k in NAMES[1:]:
            assert np.array_equal(getattr(bg, k).get().reshape(6, 10), getattr(ref, k)), (k, i)
        assert np.array_equal(bg.cut.get().reshape(6, 10), G.cut_map(bg.near.get().reshape(6, 10), bg.seen.get().reshape(6, 10), *spec)), i
        assert np.array_equal(part.get().reshape(1, -1, 2), G.partials(want[None])), i
        if i == PERSIST - 1:
            assert (want[:, 0:2] != 0).all()                                         # the new object is still foreground ...
        if i == PERSIST + 1:
            assert not want[:, 0:2].any()                                            # ... and background from persist ticks on
    assert np.all(ref.near[:, 0:2] <= 502.) and np.all(ref.seen[:, 0:2] >= PERSIST)  # absorbed
    assert np.all(ref.near[3:, 3:5] >= 1397.)                                        # receded to the wall
    assert 1397. <= ref.near[5, 6] <= 1400. and ref.seen[5, 6] == 3 + 4              # the flicker never got to persist
    assert np.all(ref.near[0:3, 7:10] >= 1397.) and not ref.cand[0:3, 7:10].any() and np.all(ref.seen[0:3, 7:10] == 3)    # the hand: never learned
    assert ref.near[0, 5] != 0 and ref.seen[0, 5] >= PERSIST                         # an unknown pixel is learned


# ---- 5: the ragged layout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_adapt_src_equals_the_plain_launch_on_each_source_alone(backend):
    rt = get_runtime(backend)
    tab = _table(rt, [A.Camera.icvl()] * 3, SRC_SIZES)
    cases = [_case((1,) + s) for s in SRC_SIZES]
    spec, guard = cases[0][6], 2
    win = [(-1, -1, 20, 9), (10, 5, 30, 30), (0, 0, 1, 2), (30, 30, 40, 40), (3, 3, 0, 0)]
    src = [0, 0, 1, 2, 2]
    take = [1, 1, 1]
    # per source: frames, cut, near, seen, cand, run
    per = [[c[0][0], c[5][0], c[1][0], c[2][0], c[3][0], c[4][0]] for c in cases]
    bufs, hosts = zip(*[_ragged(rt, tab, [p[k] for p in per], per[0][k].dtype) if per[0][k].dtype == f32 else
                        _ragged_int(rt, tab, [p[k] for p in per]) for k in range(6)])
    bg = ops.BackgroundModel(rt, _spec(spec, PERSIST, guard), 3, table=tab)
    bg.cut, bg.near, bg.seen, bg.cand, bg.run = bufs[1:]
    tk, rec, sr = rt.upload(np.asarray(take, i32)), rt.upload(_records(win).view(np.uint8)), rt.upload(np.asarray(src, i32))
    part = ops.frame_range_workspace(rt, 3)
    ops.frame_background_adapt(rt, bufs[0], bg, tk, None, None, None, rec, len(win), sr, part, table=tab)(rt.stream)
    rt.synchronize()
    got, p = [b.get() for b in bufs], part.get().reshape(3, -1, 2)
    for c, (H, W) in enumerate(SRC_SIZES):
        mine = [w for w, s in zip(win, src) if s == c]
        state = tuple(per[c][k][None] for k in (1, 2, 3, 4, 5))
        one = _launch(rt, (1, H, W), per[c][0][None], state, spec, guard, [1], mine, [0] * len(mine))
        want = _want((1, H, W), per[c][0][None], state, spec, guard, [1], mine, [0] * len(mine))
        off = int(tab.host['frame_off'][c])
        for k, name in enumerate(NAMES):
            assert np.array_equal(got[k][off:off + H * W].reshape(H, W), one[name][0]) and np.array_equal(one[name], want[name]), (c, name)
        assert np.array_equal(p[c], one['partial'][0]), c
    for k in range(6):
        assert _pads(tab, got[k]).tobytes() == _pads(tab, hosts[k]).tobytes(), NAMES[k]   # the padding words kept their bits


def _ragged_int(rt, tab, arrays):
    host = np.full(tab.frame_elems, -99, i32)
    for c, a in enumerate(arrays):
        off = int(tab.host['frame_off'][c])
        host[off:off + a.size] = a.ravel()
    return rt.upload(host), host


# ---- 6: refused calls ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_adapt_refused_calls(backend):
    rt = get_runtime(backend)
    B, H, W = shape = (2, 6, 10)
    n = B * H * W
    big = rt.upload(np.full(7 * n, SENTINEL, f32))                                    # six arrays side by side, and one spare
    p = [big.ptr + 4 * n * k for k in range(7)]
    take, rec, src = rt.upload(np.ones(B, i32)), rt.upload(_records([(0, 0, 5, 5)] * 2).view(np.uint8)), rt.upload(np.zeros(2, i32))
    part = ops.frame_range_workspace(rt, B)
    part.set(np.full(part.size, SENTINEL, f32))
    good = dict(bufs=p[:6], take=take.ptr, shape=(B, H, W), rec=rec.ptr, T=2, src=src.ptr, opts=(20., 0.01, 2, 3, 1))

    def call(**kw):
        a = dict(good, **kw)
        return rt.lib.dpp_frame_background_adapt(*(tuple(a['bufs']) + (a['take'],) + tuple(a['shape']) + (a['rec'], a['T'], a['src']) +
                                                   tuple(a['opts']) + (part.ptr, rt.stream)))
    bad = [dict(bufs=p[:k] + [None] + p[k + 1:6]) for k in range(6)]
    bad += [dict(bufs=p[:j] + [p[k]] + p[j + 1:6]) for k in range(6) for j in range(6) if j != k]      # one buffer handed twice
    bad += [dict(bufs=p[:5] + [p[4] + 4 * (n - 1)]), dict(bufs=[p[1] + 4] + p[1:6])]                   # overlapping by one element
    bad += [dict(take=None), dict(T=-1), dict(shape=(0, H, W)), dict(shape=(65536, H, W)), dict(shape=(B, 0, W)), dict(shape=(B, H, -1)),
            dict(shape=(1, 65536, 65536))]
    bad += [dict(opts=o) for o in [(20., 0.01, 2, 1, 1), (20., 0.01, 1, 1, 0), (20., 0.01, 2, 0, 1), (20., 0.01, 4, 3, 1), (20., 0.01, 0, 3, 1),
                                   (20., 0.01, 2, 3, -1), (np.nan, 0.01, 2, 3, 1), (np.inf, 0.01, 2, 3, 1), (20., np.nan, 2, 3, 1),
                                   (20., -np.inf, 2, 3, 1)]]
    for kw in bad:
        assert call(**kw) == BADARG, kw
    tab = _table(rt, [A.Camera.icvl()] * 2, [(6, 10), (5, 1)])

    def call_src(**kw):
        a = dict(good, **kw)
        return rt.lib.dpp_frame_background_adapt_src(*(tuple(a['bufs']) + (a['take'], a.get('tab', tab.dev.ptr), a.get('C', 2), a['rec'], a['T'],
                                                                            a['src']) + tuple(a['opts']) + (part.ptr, rt.stream)))
    bad = [dict(bufs=p[:k] + [None] + p[k + 1:6]) for k in range(6)] + [dict(bufs=p[:5] + [p[2]]), dict(bufs=[p[1]] + p[1:6])]
    bad += [dict(take=None), dict(tab=None), dict(C=0), dict(C=65536), dict(T=-1), dict(opts=(20., 0.01, 2, 1, 1)), dict(opts=(20., 0.01, 2, 3, -1)),
            dict(opts=(np.nan, 0.01, 2, 3, 1)), dict(opts=(20., np.inf, 2, 3, 1))]
    for kw in bad:
        assert call_src(**kw) == BADARG, kw
    rt.synchronize()
    assert np.all(big.get() == SENTINEL) and np.all(part.get() == SENTINEL)                # nothing was written
    big.set(np.ones(7 * n, f32))                                                          # (as int32 a count of 1065353216: still legal)
    assert call(rec=None) == 0 and call(T=0, src=None) == 0 and call(bufs=p[1:7]) == 0    # no records, no tracks; adjacent is not overlapping
    rt.synchronize()
    bg = ops.BackgroundModel(rt, _spec((20., 0.01, 2), 3, 1), B, H, W)
    m = ops.frame_background_adapt(rt, rt.upload(np.zeros(shape, f32)), bg, take, B, H, W, rec, 2, src, part).meta
    assert m['kernel'] == 'frame_background_adapt' and m['bytes'] == 12 * 4 * n and m['flops'] > 0


# ---- 8: the options --------------------------------------------------------------------------------------------------------------------
def test_adapt_options_are_validated():
    base = dict(margin=20., rel=0.01, min_seen=2)
    assert ops.background_spec(dict(base, adapt=dict(persist=3, guard=0))) == (20., 0.01, 2)
    assert ops.background_adapt_spec(dict(base, adapt=dict(persist=3, guard=0))) == (3, 0, 1)
    assert ops.background_adapt_spec(dict(base, adapt=dict(persist=2, guard=5, every=4))) == (2, 5, 4)
    assert ops.background_adapt_spec(base) is None and ops.background_adapt_spec(dict(base, adapt=None)) is None
    assert ops.background_adapt_spec((20., 0.01, 2)) is None                             # what a tracker hands its detectors
    for bad in (dict(), dict(persist=3), dict(guard=1), dict(persist=1, guard=0), dict(persist=3, guard=-1), dict(persist=3, guard=0, every=0),
                dict(persist=2.5, guard=0), dict(persist=3, guard=0.5), dict(persist=3, guard=0, every=1.5), dict(persist='x', guard=0),
                dict(persist=3, guard=0, blur=1), dict(persist=True, guard=0), dict(persist=2 ** 31, guard=0), (3, 0), 3):
        for fn in (ops.background_spec, ops.background_adapt_spec):
            with pytest.raises(ValueError):
                fn(dict(base, adapt=bad))
    with pytest.raises(ValueError):
        ops.background_spec(dict(base, min_seen=4, adapt=dict(persist=3, guard=0)))       # persist >= max(2, min_seen)
    assert ops.background_adapt_spec(dict(base, min_seen=4, adapt=dict(persist=4, guard=0))) == (4, 0, 1)
    with pytest.raises(ValueError):
        ops.background_spec(dict(adapt=dict(persist=3, guard=0)))                         # margin still has no default
    for bad in (3, 'far', None, [20., 0.01, 2], dict(base, blur=1)):                      # no dict of the known keys: ValueError, both
        for fn in (ops.background_spec, ops.background_adapt_spec):
            with pytest.raises(ValueError):
                fn(bad)
    with pytest.raises(ValueError):
        ops.BackgroundModel(None, 3, 1, 4, 4)


@pytest.mark.parametrize('backend', BACKENDS)
def test_model_holder_zeroes_the_candidates(backend):
    rt = get_runtime(backend)
    tab = _table(rt, [A.Camera.icvl()] * 3, SRC_SIZES)
    plain = ops.BackgroundModel(rt, dict(margin=20.), 3, table=tab)
    assert plain.adapt is None and plain.cand is None and plain.run is None
    plain.clear()                                                                        # nothing to forget
    bg = ops.BackgroundModel(rt, dict(margin=20., rel=0.01, min_seen=2, adapt=dict(persist=3, guard=1, every=2)), 3, table=tab)
    assert bg.adapt == (3, 1, 2) and bg.spec == (20., 0.01, 2) and not bg.cand.get().any() and not bg.run.get().any()
    assert bg.cand.dtype == f32 and bg.run.dtype == i32 and bg.cand.size == bg.near.size == bg.run.size
    bg.cand.set(np.full(bg.cand.size, 5., f32))
    bg.run.set(np.full(bg.run.size, 2, i32))
    bg.clear(1)
    near = np.full(SRC_SIZES[2], 900., f32)
    bg.set(2, near, np.full(SRC_SIZES[2], 3, i32))
    for c, zeroed in enumerate((False, True, True)):
        assert bg.view(bg.cand, c).get().any() != zeroed and bg.view(bg.run, c).get().any() != zeroed, c
    assert np.all(_pads(tab, bg.cand.get()) == 5.) and np.all(_pads(tab, bg.run.get()) == 2)
    assert np.array_equal(bg.get(2)['cut'], G.cut_map(near, np.full(SRC_SIZES[2], 3, i32), 20., 0.01, 2))
    assert set(bg.get(2)) == {'near', 'seen', 'cut'}


# ---- 9: the ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_new_symbols_and_the_abi_version(backend):
    rt = get_runtime(backend)
    with open(os.path.join(ROOT, 'include', 'dpp_hip.h')) as fh:
        header = fh.read()
    assert re.search(r'#define DPP_ABI_VERSION (\d+)', header).group(1) == '25'
    assert lib.ABI_VERSION == 25 and rt.lib.dpp_abi_version() == 25
    for name in ('dpp_frame_background_adapt', 'dpp_frame_background_adapt_src'):
        assert re.search(r'\bint %s\(' % name, header) and hasattr(rt.lib, name) and name in lib.SIGNATURES
    assert rt.lib.dpp_crop_record_bytes() == REC.itemsize == 80


# ---- 7: the trackers -------------------------------------------------------------------------------------------------------------------
from tests.test_background import KINDS, NLEARN, SENSOR, SPEC, _Rig, _same_ticks          # noqa: E402  (the small blob set-ups)

ADAPT = dict(persist=2, guard=2)                       # SPEC: margin 50 mm, rel 0.01, min_seen 2 -- band(1400) = 64 mm, band(300) = 53 mm


def _bg(**adapt):
    return dict(SPEC, adapt=dict(ADAPT, **adapt))


def _wall(seed, n, H, W):
    """n frames of the empty scene: drifting_sequence's wall (noise, holes, pixels beyond maxDepth), in whole millimetres."""
    rng = np.random.RandomState(seed)
    f = np.full((n, H, W), 1400., f32) + rng.normal(0, 3., (n, H, W)).astype(f32)
    f[rng.uniform(size=f.shape) < 0.05] = 0.
    f[rng.uniform(size=f.shape) < 0.01] = 2500.
    return np.rint(f).astype(f32)


@functools.lru_cache(maxsize=None)
def _raw(kind):
    """Per source (frames in whole millimetres, centres) of tests.test_background's set-ups, WITHOUT its slab."""
    from tests.test_multitrack import _setup as homo
    from tests.test_multitrack_sources import _setup as hetero
    seqs = hetero('small')[6] if kind == 'hetero' else homo('small')[7][:1 if kind == 'hand' else None]
    return [(np.rint(f).astype(f32), c) for f, c in seqs]


def _box(H, W):
    """The late clutter: a rectangle of 1280 px at 300 mm along the right edge, outside the window of the blob (which ends near
    x = 122 at 120 x 160) and its guard."""
    return slice(H // 6, H * 5 // 6), slice(W - 20, W - 4), f32(300.)


def _paste(frame, H, W):
    f = np.array(frame, f32)
    r, c, d = _box(H, W)
    f[r, c] = d
    return f


def _in_box(com, H, W):
    """The centre sits on the rectangle: at its depth (the blob is at 600 mm, the stick at 350) and on its side of the frame.  (The
    refined centre is a mean over a cube that also holds part of the stick: it need not lie inside the rectangle's outline.)"""
    return com[2] < 340. and com[0] > W * 0.7


def _window(res, cube, fx, fy):
    """The crop window track_refine left for a result of the tracker: comToBounds of the float32 centre, empty unless the track is OK."""
    if res['status'] != 0:
        return (0, 0, 0, 0)
    xs, xe, ys, ye = A.com_to_bounds(res['com'].astype(np.float64), cube, fx, fy)[:4]
    return (xs, ys, xe - xs, ye - ys)


def _model_state(tr, c=0):
    bg = tr.bg
    return dict((k, bg.view(getattr(bg, k), c).get()[0]) for k in NAMES[1:])


def _learn_wall(rig, tr, seed=90):
    for i in range(NLEARN):
        frames = [_wall(seed + c, NLEARN, *rig.sizes[c])[i] for c in range(rig.C)]
        tr.learn_background(frames[0] if rig.kind == 'hand' else frames)


def _ref_sources(rig, tr, persist, guard):
    """The restatement's model per source, learned as _learn_wall learns."""
    out = []
    for c in range(rig.C):
        near, seen = np.zeros(rig.sizes[c], f32), np.zeros(rig.sizes[c], i32)
        for f in _wall(90 + c, NLEARN, *rig.sizes[c]):
            near, seen = G.learn(near, seen, f)
        out.append(AD.Source(rig.sizes[c], tr.background, persist, guard, near, seen))
    return out


@pytest.mark.parametrize('backend', BACKENDS)
def test_late_clutter_is_absorbed_and_acquire_finds_the_hand_again(backend):
    """(a) a rectangle of 1280 px at 300 mm appears after learning: it takes acquire, with the option too, until it has stood for
    `persist` adapting ticks; from then on acquire lands on the blob."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    rig = _Rig(rt, backend, 'hand')
    H, W = rig.sizes[0]
    frames, coms = _raw('hand')[0]
    F = [_paste(f, H, W) for f in frames]
    r_, c_, d = _box(H, W)
    plain, tr = rig.build(background=SPEC), rig.build(background=_bg())
    _learn_wall(rig, plain)
    _learn_wall(rig, tr)
    for t in (plain, tr):
        got = t.acquire(F[0])
        assert got['found'] and _in_box(got['com'], H, W)                                    # the nearest object of more than 200 px
    tr.reset(coms[0])
    assert tr.process(F[1])['status'] == 0                                                   # the tick after reset: nothing adapts
    m = _model_state(tr)
    assert not m['run'].any() and not m['cand'].any() and m['seen'].max() == NLEARN
    assert tr.process(F[2])['status'] == 0                                                   # the first adapting tick: a candidate
    m = _model_state(tr)
    assert np.all(m['cand'][r_, c_] == d) and np.all(m['run'][r_, c_] == 1) and np.all(m['near'][r_, c_] > 1300.)
    assert tr.frames[0].get()[0][r_, c_].all()                                               # ... and still foreground
    assert tr.process(F[3])['status'] == 0                                                   # the second: persist = 2, absorbed
    m = _model_state(tr)
    assert np.all(m['near'][r_, c_] == d) and np.all(m['seen'][r_, c_] == 2) and not m['run'][r_, c_].any()
    assert np.array_equal(m['cut'], G.cut_map(m['near'], m['seen'], *tr.background))
    assert tr.frames[0].get()[0][r_, c_].all()                                               # the new cut holds from the next tick on
    got = tr.acquire(F[4])
    assert got['found'] and not _in_box(got['com'], H, W) and got['com'][2] > 340.
    assert np.hypot(got['com'][0] - coms[4][0], got['com'][1] - coms[4][1]) < 40.            # the blob
    assert not tr.frames[0].get()[0][r_, c_].any()
    still = plain.acquire(F[4])
    assert still['found'] and _in_box(still['com'], H, W)                                    # without adapt: for ever
    assert np.array_equal(tr.background_model()['near'], m['near']) and set(tr.background_model()) == {'near', 'seen', 'cut'}


@pytest.mark.parametrize('backend', BACKENDS)
def test_resting_hand_is_not_learned_and_the_model_is_the_restatements(backend):
    """(b) a tracked blob that rests for 3 x persist adapting ticks stays OK and the model under its window keeps its bits; (c) the
    whole model, every tick, is the restatement's driven with the windows tests/track_ref.py's comToBounds gives for the tracker's
    centres."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    rig = _Rig(rt, backend, 'hand')
    H, W = rig.sizes[0]
    frames, coms = _raw('hand')[0]
    tr = rig.build(background=_bg())
    _learn_wall(rig, tr)
    (ref,) = _ref_sources(rig, tr, ADAPT['persist'], ADAPT['guard'])
    first = _model_state(tr)
    for k in ('near', 'seen', 'cut'):
        assert np.array_equal(first[k], getattr(ref, k)), k
    tr.reset(coms[1])
    win, under = (0, 0, 0, 0), np.ones((H, W), bool)
    for i in range(1 + 3 * ADAPT['persist']):
        res = tr.process(frames[1])
        assert res['status'] == 0, i
        want = ref.tick(frames[1], int(i > 0), [win])                                        # tick 0 follows reset
        assert np.array_equal(tr.frames[0].get()[0], want), i
        m = _model_state(tr)
        for k in NAMES[1:]:
            assert np.array_equal(m[k], getattr(ref, k)), (k, i)
        win = _window(res, rig.cube, tr.fx, tr.fy)
        under &= AD.protected((H, W), [win], ADAPT['guard'])
    blob = (frames[1] > 400.) & (frames[1] < 800.)
    assert blob.sum() > 1000 and under[blob].all() and not under.all()                       # the window covered the hand all the time
    for k in ('near', 'seen', 'cut'):
        assert m[k][under].tobytes() == first[k][under].tobytes(), k
    assert not m['cand'][under].any() and (m['seen'][~under] > first['seen'][~under]).mean() > 0.8


@pytest.mark.parametrize('backend', BACKENDS)
def test_every_third_tick_adapts_and_never_the_tick_after_reset(backend):
    """(d) every = 3: of ticks 0 .. 6 only 0, 3 and 6 are adapting ticks -- and (e) tick 0 follows reset, so the model changes in
    ticks 3 and 6 alone; after another reset, tick 9 does not adapt either."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    rig = _Rig(rt, backend, 'hand')
    frames, coms = _raw('hand')[0]
    tr = rig.build(background=_bg(every=3))
    _learn_wall(rig, tr)
    tr.reset(coms[1])
    changed, last = [], _model_state(tr)
    for i in range(7):
        assert tr.process(frames[1 + i % 2])['status'] == 0
        m = _model_state(tr)
        if any(m[k].tobytes() != last[k].tobytes() for k in m):
            changed.append(i)
        last = m
    assert changed == [3, 6] and tr.adapt.tick == 7 and tr.adapt.hosts[0].tolist() == [1]
    tr.process_sequence([frames[1], frames[2]])                                              # ticks 7, 8: counted alike, not adapting
    m = _model_state(tr)
    assert all(m[k].tobytes() == last[k].tobytes() for k in m) and tr.adapt.tick == 9


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('kind', ['multi', 'hetero'])
def test_sources_adapt_alone_and_sequences_equal_the_loop(backend, kind):
    """MultiTracker, homogeneous and on the per-source table: (c) the model is the restatement's, (e) no adaptation for a source
    without a frame, nor for the source of a track that was reset, (f) process_sequence gives the bits of the process() loop, results
    and model."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    rig = _Rig(rt, backend, kind)
    raw = _raw(kind)
    a, b = rig.build(background=_bg()), rig.build(background=_bg())                          # the process() loop and the sequence
    ticks = [[raw[c][0][i] for c in range(rig.C)] for i in (1, 2, 3)]
    ticks[1][1] = None                                                                       # source 1 sits tick 1 out
    refs = _ref_sources(rig, a, ADAPT['persist'], ADAPT['guard'])
    for tr in (b, a):
        _learn_wall(rig, tr)
        for t, (c, _) in enumerate(rig.tracks):
            tr.reset(t, raw[c][1][0])
        out = rig.process(tr, [raw[c][0][0] for c in range(rig.C)])                          # tick 0: every source behind a reset
    for c, ref in enumerate(refs):
        ref.tick(raw[c][0][0], 0, [])
        for k in NAMES[1:]:
            assert np.array_equal(_model_state(b, c)[k], getattr(ref, k)), (c, k)
    loop = []
    for i, frames in enumerate(ticks):                                                       # (`out`: a's tick 0)
        wins = [_window(out[t], rig.cube, a.fxs[c], a.fys[c]) for t, (c, _) in enumerate(rig.tracks)]
        out = rig.process(a, frames)
        loop.append(out)
        for c, ref in enumerate(refs):
            mine = [w for w, (s, _) in zip(wins, rig.tracks) if s == c]
            before = dict((k, np.array(getattr(ref, k))) for k in NAMES[1:])
            ref.tick(frames[c], 1, mine)
            m = _model_state(a, c)
            for k in NAMES[1:]:
                assert np.array_equal(m[k], getattr(ref, k)), (i, c, k)
            if frames[c] is None:
                assert all(m[k].tobytes() == before[k].tobytes() for k in NAMES[1:]), (i, c)
            else:
                assert (m['seen'] != before['seen']).any(), (i, c)
    assert all(r['status'] == 0 for r in loop[-1])
    seq = rig.sequence(b, ticks)
    _same_ticks(loop, seq, 'sequence')
    for c in range(rig.C):
        ma, mb = _model_state(a, c), _model_state(b, c)
        assert all(ma[k].tobytes() == mb[k].tobytes() for k in NAMES[1:]), c
    assert a.adapt.tick == b.adapt.tick == 4
    # a reset between ticks: the track's source sits one tick out, the others adapt
    before = [_model_state(a, c) for c in range(rig.C)]
    last, out_ = len(rig.tracks) - 1, rig.C - 1
    assert rig.tracks[last][0] == out_                                                      # the last track reads the last source, alone
    a.reset(last, loop[-1][last]['com'])
    rig.process(a, ticks[0])
    after = [_model_state(a, c) for c in range(rig.C)]
    assert all(after[out_][k].tobytes() == before[out_][k].tobytes() for k in NAMES[1:])
    assert all((after[c]['seen'] != before[c]['seen']).any() for c in range(out_))
    assert a.adapt.hosts[0].tolist() == [1] * out_ + [0]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('kind', KINDS)
def test_adapt_plan_structure(backend, kind):
    """(g) frame_background_adapt in frame_background's place, the launch count unchanged, with and without a sensor; (h) without
    adapt: the plan and the allocation of before."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    rig = _Rig(rt, backend, kind)
    hetero = kind == 'hetero'
    for kw in (dict(), dict(sensor=SENSOR)):
        old, tr = rig.build(background=SPEC, **kw), rig.build(background=_bg(every=2), **kw)
        assert old.adapt is None and old.bg.cand is None and old.bg.run is None and old.bg.adapt is None           # (h)
        names = [l.name for l in old.plan(0).launches()]
        assert 'frame_background' in names and 'frame_background_adapt' not in names
        assert old.plan(0).launches()[names.index('frame_background')].fn is (rt.lib.dpp_frame_background_src if hetero else rt.lib.dpp_frame_background)
        assert tr.bg.adapt == (2, 2, 2) and tr.background == old.background == (50., 0.01, 2)
        for slot in (0, 1):
            la = tr.plan(slot).launches()
            at = names.index('frame_background')
            assert [l.name for l in la] == names[:at] + ['frame_background_adapt'] + names[at + 1:] and len(la) == len(names)
            l = la[at]
            assert l.fn is (rt.lib.dpp_frame_background_adapt_src if hetero else rt.lib.dpp_frame_background_adapt)
            bg = tr.bg
            frames = (tr.frames[slot] if kind == 'hand' else (tr._inputs2 if slot and not kw else tr.frames))
            assert l.args[:7] == (frames.ptr, bg.cut.ptr, bg.near.ptr, bg.seen.ptr, bg.cand.ptr, bg.run.ptr, tr.adapt.bufs[slot].ptr)
            T = 1 if kind == 'hand' else tr.T
            assert l.args[-9:-6] == (tr.rec.ptr, T, None if kind == 'hand' else tr.src.ptr)
            assert l.args[-6:-1] == (50., 0.01, 2, 2, 2) and l.args[-1] == tr.partial.ptr
        assert tr.adapt.bufs[0].ptr != tr.adapt.bufs[1].ptr                                  # one take array per input set
        det = tr.detector() if kind == 'hand' else tr.detector(0)                            # the detectors do not adapt
        assert 'frame_background' in [l.name for l in det.plan(False).launches()]
        assert 'frame_background_adapt' not in [l.name for l in det.plan(False).launches()]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('kind', KINDS)
def test_without_adapt_the_results_are_those_of_before(backend, kind):
    """(h) results: one tick of a tracker with background=SPEC (no adapt) has, key for key and bit for bit, the results of a tracker
    without the option that is fed the frames tests/background_ref.py masks with its own cut map of the learned model -- what the
    option gave before adaptation existed.  And a tracker WITH adapt gives the same bits in a tick in which it does not adapt (the one
    after reset), with its model untouched: the adapting launch cuts as frame_background does."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    rig = _Rig(rt, backend, kind)
    raw = _raw(kind)
    plain, old, new = rig.build(), rig.build(background=SPEC), rig.build(background=_bg())
    _learn_wall(rig, old)
    _learn_wall(rig, new)
    refs = _ref_sources(rig, old, ADAPT['persist'], ADAPT['guard'])
    for tr in (plain, old, new):
        if kind == 'hand':
            tr.reset(raw[0][1][0])
        else:
            for t, (c, _) in enumerate(rig.tracks):
                tr.reset(t, raw[c][1][0])
    frames = [raw[c][0][1] for c in range(rig.C)]
    masked = [G.apply(f, G.cut_map(ref.near, ref.seen, *old.background)) for f, ref in zip(frames, refs)]
    assert all((m != f).mean() > 0.5 and m.any() for m, f in zip(masked, frames))           # the wall goes, the hand stays
    want, got, too = rig.process(plain, masked), rig.process(old, frames), rig.process(new, frames)
    assert all(r['status'] == 0 for r in want)
    for other in (got, too):
        assert all(set(p) == set(q) for p, q in zip(want, other))                           # no key more, none less
        _same_ticks([want], [other], 'adapt absent')
    for c, ref in enumerate(refs):
        for tr in (old, new):
            m = rig.model(tr, c)
            assert np.array_equal(m['near'], ref.near) and np.array_equal(m['seen'], ref.seen) and np.array_equal(m['cut'], ref.cut), c
        assert not _model_state(new, c)['cand'].any() and not _model_state(new, c)['run'].any()


# ---- 8: the pipelines and the examples -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_pipelines_pass_the_option(backend):
    from tests.test_detect import _ListDevice
    from util.realtimehandposepipeline import MultiStreamPipeline, RealtimeHandposePipeline
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    rig = _Rig(rt, backend, 'hand')
    H, W = rig.sizes[0]
    config = {'fx': 241.42, 'fy': 241.42, 'cube': (250, 250, 250)}
    rtp = RealtimeHandposePipeline(rig.pnet, dict(config), rig.dis[0], comrefNet=rig.snet, background=_bg(every=3))
    rtp.initNets()
    t = rtp.tracker(H, W)
    assert t.bg.adapt == (2, 2, 3) and t.adapt.every == 3 and t.plan(0).launches()[0].name == 'frame_background_adapt'
    with pytest.raises(ValueError):
        bad = RealtimeHandposePipeline(rig.pnet, dict(config), rig.dis[0], comrefNet=rig.snet, background=dict(SPEC, adapt=dict(persist=1, guard=0)))
        bad.initNets()
        bad.tracker(H, W)
    mrig = _Rig(rt, backend, 'multi')
    Lh, Rh = MultiStreamPipeline.HAND_LEFT, MultiStreamPipeline.HAND_RIGHT
    hands = [(c, Rh if right else Lh) for c, right in mrig.tracks]
    msp = MultiStreamPipeline(mrig.pnet, dict(config), mrig.dis[0], [_ListDevice([]) for _ in range(mrig.C)], hands, mrig.snet,
                              init_com=[mrig.src[c]['coms'][0] for c, _ in mrig.tracks], background=_bg())
    mt = msp.tracker(H, W)
    assert mt.bg.adapt == (2, 2, 1) and mt.adapt.C == mrig.C and mt.plan(0).launches()[0].name == 'frame_background_adapt'


@pytest.mark.parametrize('backend', BACKENDS)
def test_examples_run_with_the_new_flags(backend, tmp_path):
    import importlib.util
    from tests import track_ref as T
    from tests.test_background import _files
    R.set_default_runtime(get_runtime(backend))
    cam, cube, H, W = A.Camera.icvl(), (250., 250., 250.), 120, 160
    frames, coms = T.drifting_sequence(np.random.RandomState(36), 5, cam, H, W, cube)
    base, _, _ = _files(tmp_path, 'test_seq_1', frames, coms, cam)
    net = 'resnet' if backend == 'hip' else 'poseregnet'               # (the 128x128 ResNet is too slow for the SIMT emulator)
    spec = importlib.util.spec_from_file_location('adapt_realtime_background', os.path.join(ROOT, 'examples', 'realtime_background.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    assert ex.parse_clutter('1:2:3:4:300') == (1, 2, 3, 4, 300.) and ex.parse_clutter('1:2:3:4:300:7', with_start=True) == ((1, 2, 3, 4, 300.), 7)
    assert ex.parse_clutter('1:2:3:4:300', with_start=True) == ((1, 2, 3, 4, 300.), None)
    common = ['--dataset', 'icvl', '--data', base, '--net', net, '--cache', str(tmp_path / 'cache')]
    r_, c_, d = _box(H, W)
    late = '%d:%d:%d:%d:%g:1' % (c_.start, r_.start, c_.stop, r_.stop, d)
    flags = common + ['--background', '50', '0.01', '--learn', '2', '--clutter', late]
    poses, err, fig = ex.main(flags + ['--adapt', '2', '2'])
    assert poses.shape == (5, 16, 3) and np.isfinite(poses).all() and np.isfinite(err)
    assert len(fig['landed']) == 5 and fig['landed'][0] is not None and not ex.on_clutter(fig['landed'][0], (c_.start, r_.start, c_.stop, r_.stop, d))
    assert ex.on_clutter(fig['landed'][1], (c_.start, r_.start, c_.stop, r_.stop, d))       # it appears in tick 1 and takes the detector ...
    assert fig['hand_again'] == 1 + 2                                   # ... until it has stood for persist = 2 adapting ticks (1 and 2)
    _, _, fig0 = ex.main(flags)
    assert fig0['hand_again'] is None and ex.on_clutter(fig0['landed'][4], (c_.start, r_.start, c_.stop, r_.stop, d))      # without --adapt: never
    for bad in (['--adapt', '2', '2'], flags + ['--adapt-every', '2'], flags + ['--adapt', '1', '0'], common + ['--background', '50', '0.01',
                '--clutter', '5:5:9:9:300:-1']):
        with pytest.raises((SystemExit, ValueError)):
            ex.main(common + bad if bad[0] == '--adapt' and len(bad) == 3 else bad)
    spec = importlib.util.spec_from_file_location('adapt_realtime_multi', os.path.join(ROOT, 'examples', 'realtime_multi.py'))
    multi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(multi)
    made, Msp = [], multi.MultiStreamPipeline

    class Recorded(Msp):
        def __init__(self, *a, **k):
            made.append(self)
            super(Recorded, self).__init__(*a, **k)
    multi.MultiStreamPipeline = Recorded
    try:
        mposes, _ = multi.main(flags + ['--seqs', 'test_seq_1', 'test_seq_1', '--max-frames', '4', '--adapt', '2', '2', '--adapt-every', '1'])
    finally:
        multi.MultiStreamPipeline = Msp
    assert [q.shape for q in mposes] == [(4, 16, 3)] * 3 and all(np.isfinite(q).all() for q in mposes)
    assert made[-1]._tracker.bg.adapt == (2, 2, 1) and all(k > 0.9 for k in made[-1].background_absorbed), made[-1].background_absorbed
