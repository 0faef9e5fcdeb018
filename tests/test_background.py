"""A learned static background removed on the device (csrc/background.hip, ABI v25; HandTracker / MultiTracker / FrameDetector /
the pipelines with background=...) against the NumPy restatement of tests/background_ref.py, which is the definition: the reference
has no counterpart.  Learning and applying are selections and the cut map is computed by the host in float32: every comparison here
is np.array_equal.  The device tests run on the SIMT emulator and, with -m gpu, on the card."""
import functools
import importlib.util
import os
import re

import numpy as np
import pytest

from data.importers import ICVLImporter
from hipdp import lib, ops
from hipdp import runtime as R
from oracle import augment as A
from tests import background_ref as G
from tests import ingest_ref as I
from tests import track_ref as T
from tests.backends import BACKENDS, get_runtime
from tests.test_multitrack import _nets, _same
from tests.test_multitrack_sources import _pads, _ragged, _table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = 10001
SENTINEL = np.float32(-7.25)
INF = np.float32(np.inf)
# H below / not a multiple of / equal to FR_BANDS = 64, H * W not a multiple of 4 (the scalar path), an unaligned second frame (odd H * W),
# more elements than one sweep of the grid (129 x 641 scalar: 5 per thread)
SHAPES = [(1, 1, 1), (2, 1, 7), (2, 5, 1), (3, 3, 5), (2, 37, 53), (1, 65, 66), (3, 63, 64), (1, 64, 64), (1, 129, 641)]
SRC_SIZES = [(37, 53), (5, 1), (64, 64)]


def _sid(s):
    return 'x'.join(map(str, s))


@functools.lru_cache(maxsize=None)
def _case(shape):
    f, near, seen, spec = G.case(np.random.RandomState(sum(shape)), *shape)
    cut = G.cut_map(near, seen, *spec)
    out = G.apply(f, cut)
    for a in (f, near, seen, cut, out):
        a.setflags(write=False)
    return f, near, seen, spec, cut, out


# ---- 1: the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_hand_values():
    one, f32 = np.ones((1, 1), np.int32), np.float32
    cut = G.cut_map(f32([[1000.]]), one, 20., 0.01)
    assert cut.dtype == np.float32 and cut[0, 0] == f32(970.)
    assert G.cut_map(f32([[1000.]]), one, 20., 0.01, min_seen=2)[0, 0] == INF           # seen < min_seen
    assert G.cut_map(f32([[0.]]), one * 5, 20.)[0, 0] == INF                            # nothing seen
    assert G.cut_map(f32([[20.]]), one, 20.)[0, 0] == INF and G.cut_map(f32([[5.]]), one, 20.)[0, 0] == INF     # cut <= 0
    assert G.cut_map(f32([[20.5]]), one, 20.)[0, 0] == f32(0.5)
    # every operation rounds to float32: not the float64 expression rounded once
    near = f32([[1234.5677]])
    want = f32(near[0, 0] - f32(f32(7.3) + f32(f32(0.013) * near[0, 0])))
    assert G.cut_map(near, one, 7.3, 0.013)[0, 0] == want
    assert np.array_equal(ops.background_cut(near, one, (7.3, 0.013, 1)), G.cut_map(near, one, 7.3, 0.013))
    c = f32(970.)
    below, above = np.nextafter(c, f32(0.)), np.nextafter(c, INF)
    got = G.apply(f32([[c, below, above, 0., 100.]]), f32([[c] * 5]))
    assert np.array_equal(got, f32([[0., below, 0., 0., 100.]]))                         # strict: a depth at its cut is background
    f, near, seen, spec, cut, out = _case((2, 37, 53))
    assert np.array_equal(G.apply(out, cut), out)                                       # idempotent
    assert np.array_equal(G.apply(f, np.full(f.shape, INF, np.float32)), f)             # an all-+inf cut is the identity
    assert 0.25 < (f == 0).mean() < 0.35 and np.isinf(cut).mean() > 0.15 and np.isfinite(cut).mean() > 0.5
    fin = np.isfinite(cut) & (f != 0)
    assert (f[fin] == cut[fin]).sum() > 50 and (f[fin] == np.nextafter(cut[fin], INF)).sum() > 50
    assert (f[fin] == np.nextafter(cut[fin], f32(0.))).sum() > 50
    assert np.array_equal(ops.background_cut(near, seen, spec), cut)
    # learning
    n, s = G.learn(f32([[0., 500., 500., 0.]]), np.int32([[0, 1, 1, 0]]), f32([[0., 400., 600., 700.]]))
    assert np.array_equal(n, f32([[0., 400., 500., 700.]])) and np.array_equal(s, np.int32([[0, 2, 2, 1]]))
    # the partition: 16-byte groups iff H * W is a multiple of 4; a band without elements has the identities
    p = G.partials(f32(np.arange(1, 9)).reshape(1, 2, 4))
    assert np.array_equal(p[0, 0], f32([1., 8.])) and np.all(p[0, 1:, 0] == G.IDENT[0]) and np.all(p[0, 1:, 1] == G.IDENT[1])
    assert G.band_of(4 * 256 + 4, True).tolist() == [0] * 1024 + [1] * 4 and G.band_of(257, False).tolist() == [0] * 256 + [1]


# ---- 2: the kernels, bit for bit ---------------------------------------------------------------------------------------------------
def _apply(rt, frames, cut, with_partial=True):
    B, H, W = frames.shape
    fr, cu = rt.upload(frames), rt.upload(cut)
    part = ops.frame_range_workspace(rt, B) if with_partial else None
    if with_partial:
        part.set(np.full(part.size, SENTINEL, np.float32))
    ops.frame_background(rt, fr, cu, B, H, W, part)(rt.stream)
    rt.synchronize()
    return fr, cu, (part.get().reshape(B, -1, 2) if with_partial else None)


def _check_apply(rt, shape):
    f, near, seen, spec, cut, out = _case(shape)
    fr, cu, p = _apply(rt, f, cut)
    assert np.array_equal(fr.get(), out), shape
    assert np.array_equal(cu.get(), cut)
    assert p.shape[1] == G.FR_BANDS and not (p == SENTINEL).any()                       # every band's pair was written
    want = G.partials(out)
    assert np.array_equal(p, want), shape
    npx = shape[1] * shape[2]
    units = npx // 4 if npx % 4 == 0 else npx
    empty = np.arange(G.FR_BANDS) * G.THREADS >= units                                  # frame_range's identities in the empty bands
    assert np.all(p[:, empty, 0] == np.float32(3.4e38)) and np.all(p[:, empty, 1] == np.float32(-3.4e38))
    assert np.array_equal(p[:, :, 0].min(1), out.reshape(shape[0], -1).min(1)) and np.array_equal(p[:, :, 1].max(1), out.reshape(shape[0], -1).max(1))
    return fr, cu, out


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_frame_background_bit_for_bit(backend, shape):
    rt = get_runtime(backend)
    fr, cu, out = _check_apply(rt, shape)
    B, H, W = shape
    part = ops.frame_range_workspace(rt, B)
    ops.frame_background(rt, fr, cu, B, H, W, part)(rt.stream)                           # again, on the masked frame: the same bits
    rt.synchronize()
    assert np.array_equal(fr.get(), out) and np.array_equal(part.get().reshape(B, -1, 2), G.partials(out))
    # an all-+inf cut map: the frame as it was, frame_range's overall range
    f = _case(shape)[0]
    fr2, _, p2 = _apply(rt, f, np.full(shape, INF, np.float32))
    assert np.array_equal(fr2.get(), f) and np.array_equal(p2, G.partials(f))
    rp = ops.frame_range_workspace(rt, B)
    ops.frame_range(rt, fr2, B, H, W, rp)(rt.stream)
    rt.synchronize()
    rp = rp.get().reshape(B, -1, 2)
    assert np.array_equal(rp[:, :, 0].min(1), p2[:, :, 0].min(1)) and np.array_equal(rp[:, :, 1].max(1), p2[:, :, 1].max(1))


@pytest.mark.parametrize('backend', BACKENDS)
def test_frame_background_working_size(backend):
    _check_apply(get_runtime(backend), (1, 480, 640))


@pytest.mark.parametrize('backend', BACKENDS)
def test_frame_background_unaligned_buffers_take_the_scalar_path(backend):
    """H * W a multiple of 4 but the frame (or the cut map) one element off a 16-byte boundary: single elements, their partition, and
    not a byte outside the frame."""
    rt = get_runtime(backend)
    shape = (1, 64, 64)
    f, _, _, _, cut, out = _case(shape)
    n = f.size
    for off_f, off_c in ((1, 0), (0, 1), (3, 2)):
        fb, cb = rt.upload(np.full(n + 8, SENTINEL, np.float32)), rt.upload(np.full(n + 8, SENTINEL, np.float32))
        fr, cu = fb.view(off_f, shape), cb.view(off_c, shape)
        fr.set(f)
        cu.set(cut)
        part = ops.frame_range_workspace(rt, 1)
        ops.frame_background(rt, fr, cu, 1, 64, 64, part)(rt.stream)
        rt.synchronize()
        host = fb.get()
        assert np.array_equal(host[off_f:off_f + n].reshape(shape), out)
        assert np.all(host[:off_f] == SENTINEL) and np.all(host[off_f + n:] == SENTINEL)
        assert np.array_equal(part.get().reshape(1, -1, 2), G.partials(out, vector=False))


@pytest.mark.parametrize('backend', BACKENDS)
def test_frame_background_null_partial_and_refused_calls(backend):
    rt = get_runtime(backend)
    shape = (2, 37, 53)
    B, H, W = shape
    f, near, seen, spec, cut, out = _case(shape)
    fr, _, _ = _apply(rt, f, cut, with_partial=False)
    assert np.array_equal(fr.get(), out)
    fr = rt.upload(np.full(shape, SENTINEL, np.float32))
    cu = rt.upload(np.full(shape, np.float32(-100.), np.float32))                      # would zero everything it reached
    part = ops.frame_range_workspace(rt, B)
    part.set(np.full(part.size, SENTINEL, np.float32))
    fn = rt.lib.dpp_frame_background
    bad = [(None, cu.ptr, B, H, W), (fr.ptr, None, B, H, W), (fr.ptr, cu.ptr, 0, H, W), (fr.ptr, cu.ptr, 65536, H, W), (fr.ptr, cu.ptr, B, 0, W),
           (fr.ptr, cu.ptr, B, H, -1), (fr.ptr, cu.ptr, 1, 65536, 65536),                                   # H * W overflows
           (fr.ptr, fr.ptr, B, H, W), (fr.ptr, fr.ptr + 4 * (H * W - 1), 1, H, W), (fr.ptr + 4 * H * W, fr.ptr + 4, 1, H, W)]   # cut overlaps frames
    for args in bad:
        assert fn(*args, part.ptr, rt.stream) == BADARG, args
    tab = _table(rt, [A.Camera.icvl()] * 3, SRC_SIZES)
    fs = rt.lib.dpp_frame_background_src
    for args in [(None, cu.ptr, tab.dev.ptr, 3), (fr.ptr, None, tab.dev.ptr, 3), (fr.ptr, cu.ptr, None, 3), (fr.ptr, cu.ptr, tab.dev.ptr, 0),
                 (fr.ptr, cu.ptr, tab.dev.ptr, 65536), (fr.ptr, fr.ptr, tab.dev.ptr, 3)]:
        assert fs(*args, part.ptr, rt.stream) == BADARG, args
    model_n, model_s, take = rt.upload(np.full(shape, SENTINEL, np.float32)), rt.upload(np.full(shape, 7, np.int32)), rt.upload(np.ones(B, np.int32))
    fl = rt.lib.dpp_background_learn
    for args in [(None, take.ptr, B, H, W, model_n.ptr, model_s.ptr), (cu.ptr, None, B, H, W, model_n.ptr, model_s.ptr),
                 (cu.ptr, take.ptr, B, H, W, None, model_s.ptr), (cu.ptr, take.ptr, B, H, W, model_n.ptr, None),
                 (cu.ptr, take.ptr, 0, H, W, model_n.ptr, model_s.ptr), (cu.ptr, take.ptr, 65536, H, W, model_n.ptr, model_s.ptr),
                 (cu.ptr, take.ptr, B, 0, W, model_n.ptr, model_s.ptr), (cu.ptr, take.ptr, B, H, 0, model_n.ptr, model_s.ptr),
                 (cu.ptr, take.ptr, 1, 65536, 65536, model_n.ptr, model_s.ptr),
                 (model_n.ptr, take.ptr, B, H, W, model_n.ptr, model_s.ptr), (model_n.ptr + 4 * H * W, take.ptr, 1, H, W, model_n.ptr + 4, model_s.ptr),
                 (model_s.ptr, take.ptr, B, H, W, model_n.ptr, model_s.ptr)]:
        assert fl(*args, rt.stream) == BADARG, args
    fls = rt.lib.dpp_background_learn_src
    for args in [(None, take.ptr, tab.dev.ptr, 3, model_n.ptr, model_s.ptr), (cu.ptr, None, tab.dev.ptr, 3, model_n.ptr, model_s.ptr),
                 (cu.ptr, take.ptr, None, 3, model_n.ptr, model_s.ptr), (cu.ptr, take.ptr, tab.dev.ptr, 3, None, model_s.ptr),
                 (cu.ptr, take.ptr, tab.dev.ptr, 3, model_n.ptr, None), (cu.ptr, take.ptr, tab.dev.ptr, 0, model_n.ptr, model_s.ptr),
                 (cu.ptr, take.ptr, tab.dev.ptr, 65536, model_n.ptr, model_s.ptr), (model_n.ptr, take.ptr, tab.dev.ptr, 3, model_n.ptr, model_s.ptr)]:
        assert fls(*args, rt.stream) == BADARG, args
    rt.synchronize()
    assert np.all(fr.get() == SENTINEL) and np.all(part.get() == SENTINEL)                 # nothing was written
    assert np.all(model_n.get() == SENTINEL) and np.all(model_s.get() == 7)
    assert fn(fr.ptr + 4 * H * W, fr.ptr, 1, H, W, part.ptr, rt.stream) == 0               # adjacent is not overlapping
    rt.synchronize()
    m = ops.frame_background(rt, fr, cu, B, H, W, part).meta
    assert m['kernel'] == 'frame_background' and m['bytes'] == 3 * 4 * B * H * W and m['flops'] > 0
    assert ops.frame_background(rt, fr, cu, None, None, None, None, table=tab).meta['bytes'] == 3 * 4 * sum(h * w for h, w in SRC_SIZES)
    assert ops.background_learn(rt, cu, take, B, H, W, model_n, model_s).meta['kernel'] == 'background_learn'


@functools.lru_cache(maxsize=None)
def _src_case():
    cases = [_case((1,) + s) for s in SRC_SIZES]
    return [c[0][0] for c in cases], [c[4][0] for c in cases], [c[5][0] for c in cases]


@pytest.mark.parametrize('backend', BACKENDS)
def test_frame_background_src_equals_the_plain_launch_on_each_source_alone(backend):
    rt = get_runtime(backend)
    frames, cuts, outs = _src_case()
    tab = _table(rt, [A.Camera.icvl()] * 3, SRC_SIZES)
    assert tab.host['frame_off'].tolist() == [0, 1964, 1972]                          # 37 * 53 = 1961, 5 * 1 = 5: both padded
    fr, fhost = _ragged(rt, tab, frames, np.float32)
    cu, chost = _ragged(rt, tab, cuts, np.float32)
    part = ops.frame_range_workspace(rt, 3)
    part.set(np.full(part.size, SENTINEL, np.float32))
    for rep in range(2):                                                                 # the second launch: a stale, masked frame masked again
        ops.frame_background(rt, fr, cu, None, None, None, part, table=tab)(rt.stream)
        rt.synchronize()
        got, p = fr.get(), part.get().reshape(3, -1, 2)
        for c, (H, W) in enumerate(SRC_SIZES):
            one, _, p1 = _apply(rt, frames[c][None], cuts[c][None])
            off = int(tab.host['frame_off'][c])
            assert np.array_equal(got[off:off + H * W].reshape(H, W), one.get()[0]) and np.array_equal(one.get()[0], outs[c]), (rep, c)
            assert np.array_equal(p[c], p1[0]), (rep, c)
        assert _pads(tab, got).tobytes() == _pads(tab, fhost).tobytes()                  # the padding words kept their (NaN) bits
        assert cu.get().tobytes() == chost.tobytes()
    fr2, _ = _ragged(rt, tab, frames, np.float32)
    ops.frame_background(rt, fr2, cu, None, None, None, None, table=tab)(rt.stream)       # partial=None
    rt.synchronize()
    assert fr2.get().tobytes() == got.tobytes()


def _learning_frames(rng, n, shape):
    f = rng.uniform(300., 1500., (n,) + shape).astype(np.float32)
    f[rng.uniform(size=f.shape) < 0.3] = 0.
    f[:, :, 0, 0] = 0.                                                                   # a pixel never seen
    f[1:, :, -1, -1] = f[0, :, -1, -1]                                                   # the same depth again: near keeps, seen counts
    return f


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('shape', [(3, 37, 53), (3, 16, 64), (2, 5, 1)], ids=_sid)
def test_background_learn_over_frames_with_holes(backend, shape):
    rt = get_runtime(backend)
    B, H, W = shape
    seq = _learning_frames(np.random.RandomState(5 + H), 5, shape)
    take = np.ones(B, np.int32)
    take[1] = 0                                                                          # source 1 sits out
    n0 = np.zeros(shape, np.float32)
    s0 = np.zeros(shape, np.int32)
    n0[1], s0[1] = 777., 3                                                               # ... and keeps what it had
    near, seen, tk = rt.upload(n0), rt.upload(s0), rt.upload(take)
    want_n, want_s = n0.copy(), s0.copy()
    for i in range(5):
        fr = rt.upload(seq[i])
        ops.background_learn(rt, fr, tk, B, H, W, near, seen)(rt.stream)
        rt.synchronize()
        assert np.array_equal(fr.get(), seq[i])                                          # the frame is read only
        for b in np.flatnonzero(take):
            want_n[b], want_s[b] = G.learn(want_n[b], want_s[b], seq[i][b])
    assert np.array_equal(near.get(), want_n) and np.array_equal(seen.get(), want_s)
    assert want_s.max() == 5 and (want_s[0] == 0).any() and np.all(want_n[1] == 777.) and want_n[0, 0, 0] == 0.
    lowest = np.where(seq[:, take == 1] == 0, INF, seq[:, take == 1]).min(0)              # the restatement itself, said another way
    assert want_s[0, -1, -1] in (0, 5) and np.array_equal(want_n[take == 1], np.where(np.isinf(lowest), np.float32(0.), lowest))
    assert np.array_equal(want_s[take == 1], (seq[:, take == 1] != 0).sum(0))


@pytest.mark.parametrize('backend', BACKENDS)
def test_background_learn_src_and_the_model_holder(backend):
    """dpp_background_learn_src on the ragged layout against the restatement per source; BackgroundModel: refresh / get / set / clear."""
    rt = get_runtime(backend)
    tab = _table(rt, [A.Camera.icvl()] * 3, SRC_SIZES)
    rng = np.random.RandomState(9)
    seqs = [_learning_frames(rng, 5, (1,) + s)[:, 0] for s in SRC_SIZES]
    spec = dict(margin=20., rel=0.01, min_seen=2)
    bg = ops.BackgroundModel(rt, spec, 3, table=tab)
    assert bg.spec == (20., 0.01, 2) and np.all(np.isinf(bg.cut.get())) and not bg.near.get().any() and not bg.seen.get().any()
    want = [(np.zeros(s, np.float32), np.zeros(s, np.int32)) for s in SRC_SIZES]
    for i in range(5):
        fr, fhost = _ragged(rt, tab, [s[i] for s in seqs], np.float32)
        take = [1, int(i % 2 == 0), 1]
        bg.set_take(take)
        ops.background_learn(rt, fr, bg.take, None, None, None, bg.near, bg.seen, table=tab)(rt.stream)
        rt.synchronize()
        assert fr.get().tobytes() == fhost.tobytes()
        for c in range(3):
            if take[c]:
                want[c] = G.learn(want[c][0], want[c][1], seqs[c][i])
    assert not _pads(tab, bg.near.get()).any() and not _pads(tab, bg.seen.get()).any()    # the padding words: untouched
    bg.refresh()
    for c in range(3):
        m = bg.get(c)
        assert np.array_equal(m['near'], want[c][0]) and np.array_equal(m['seen'], want[c][1]), c
        assert m['cut'].dtype == np.float32 and np.array_equal(m['cut'], G.cut_map(want[c][0], want[c][1], 20., 0.01, 2)), c
    assert want[1][1].max() == 3 and np.isinf(bg.get(0)['cut']).any() and np.isfinite(bg.get(0)['cut']).any()
    assert np.all(np.isinf(_pads(tab, bg.cut.get())))
    other = ops.BackgroundModel(rt, spec, 3, table=tab)                                   # learn once, reload
    other.set(2, **{k: v for k, v in bg.get(2).items() if k != 'cut'})
    assert np.array_equal(other.get(2)['cut'], bg.get(2)['cut']) and np.all(np.isinf(other.get(0)['cut']))
    bg.clear(0)
    assert np.all(np.isinf(bg.get(0)['cut'])) and not bg.get(0)['near'].any() and not bg.get(0)['seen'].any()
    assert np.isfinite(bg.get(2)['cut']).any()
    with pytest.raises(ValueError):
        other.set(1, np.zeros((5, 2), np.float32), np.zeros((5, 2), np.int32))
    with pytest.raises(ValueError):
        other.set(1, np.full((5, 1), np.nan, np.float32), np.zeros((5, 1), np.int32))
    with pytest.raises(IndexError):
        other.get(3)


# ---- 3: the plans ------------------------------------------------------------------------------------------------------------------
SPEC = dict(margin=50., rel=0.01, min_seen=2)
SENSOR = dict(dtype='uint16', median=True, mirror=False)
NLEARN = 3


def _slab(H, W):
    """The static object: rows, columns and depth of a rectangle of far more than 200 px, nearer than the blob (600 mm) and the stick
    (350 mm) of tests.track_ref.drifting_sequence and to the right of both.  (The stick lies in the 250 mm cube around it: the slab is
    large enough to keep the refined centre.)"""
    return slice(H // 8, H * 7 // 8), slice(W * 3 // 4, W * 3 // 4 + W // 5), np.float32(300.)


def _empty_scene(rng, n, H, W):
    """n frames of the scene without a hand: drifting_sequence's wall (noise, holes, pixels beyond maxDepth) and the slab."""
    f = (np.full((n, H, W), 1400., np.float32) + rng.normal(0, 3., (n, H, W)).astype(np.float32)).astype(np.float32)
    f[rng.uniform(size=f.shape) < 0.05] = 0.
    f[rng.uniform(size=f.shape) < 0.01] = 2500.
    r, c, d = _slab(H, W)
    f[:, r, c] = d
    return f


def _clutter(frames):
    f = np.array(frames, np.float32)
    r, c, d = _slab(*f.shape[-2:])
    f[..., r, c] = d
    return f


def _model_ref(learn, sensor):
    """(near, seen, cut) of the restatement after the learning frames (through ingest_ref with a sensor)."""
    seen_frames = I.ingest(np.rint(learn).astype(np.uint16), median=True, mirror=False)[0] if sensor else learn
    near, seen = np.zeros(learn.shape[1:], np.float32), np.zeros(learn.shape[1:], np.int32)
    for f in seen_frames:
        near, seen = G.learn(near, seen, f)
    return near, seen, G.cut_map(near, seen, SPEC['margin'], SPEC['rel'], SPEC['min_seen'])


@functools.lru_cache(maxsize=None)
def _scenes(kind):
    """Per source of the set-up: the cluttered frames F, the learning frames, and per sensor (False, True) the restatement's model and
    masked frames.  hand: one 120 x 160 ICVL source; multi: tests.test_multitrack's small set-up; hetero: tests.test_multitrack_sources'."""
    from tests.test_multitrack import _setup as homo
    from tests.test_multitrack_sources import _setup as hetero
    if kind == 'hetero':
        dis, cams, sizes, cube, n, tracks, seqs = hetero('small')
    else:
        di, cam, cube, H, W, n, tracks, seqs = homo('small')
        if kind == 'hand':
            tracks, seqs = [(0, False)], seqs[:1]
        dis, sizes = [di] * len(seqs), [(H, W)] * len(seqs)
    out = []
    for c, (frames, coms) in enumerate(seqs):
        F = np.rint(_clutter(frames))                                  # whole millimetres: the uint16 sensor route loses nothing
        learn = np.rint(_empty_scene(np.random.RandomState(70 + c), NLEARN, *sizes[c]))
        per = {}
        for sensor in (False, True):
            near, seen, cut = _model_ref(learn, sensor)
            seenF = I.ingest(F.astype(np.uint16), median=True, mirror=False)[0] if sensor else F
            per[sensor] = dict(near=near, seen=seen, cut=cut, frames=seenF, masked=G.apply(seenF, cut))
        out.append(dict(F=F, learn=learn, coms=coms, per=per))
    return dis, sizes, cube, n, tracks, out


def _feed(frames, sensor):
    return [None if f is None else (f.astype(np.uint16) if sensor else f) for f in frames]


class _Rig(object):
    """One interface over HandTracker and MultiTracker for the plan tests: build(background=, sensor=), start, tick, learn."""

    def __init__(self, rt, backend, kind):
        self.rt, self.backend, self.kind = rt, backend, kind
        self.dis, self.sizes, self.cube, self.n, self.tracks, self.src = _scenes(kind)
        (self.snet, _, _), (self.pnet, _, _) = _nets(rt, backend, len(self.tracks))
        self.C = len(self.src)

    def build(self, **kw):
        from hipdp.multitrack import MultiTracker
        from hipdp.tracker import HandTracker
        if self.kind == 'hand':
            return HandTracker(self.rt, self.dis[0], self.pnet, self.snet, self.sizes[0][0], self.sizes[0][1], self.cube, **kw)
        if self.kind == 'multi':
            return MultiTracker(self.rt, self.dis[0], self.pnet, self.snet, self.sizes[0][0], self.sizes[0][1], self.cube, self.tracks, **kw)
        return MultiTracker(self.rt, self.dis, self.pnet, self.snet, [s[0] for s in self.sizes], [s[1] for s in self.sizes], self.cube,
                            self.tracks, **kw)

    def start(self, tr):
        if self.kind == 'hand':
            tr.reset(self.src[0]['coms'][0])
        else:
            for t, (c, _) in enumerate(self.tracks):
                tr.reset(t, self.src[c]['coms'][0])

    def ticks(self, which, sensor=False, idle=True, last=2):
        """Ticks 1 .. last of per-source frames (the nets of the CPU tier take a second per tick); `which`: 'F' or a key of the
        restatement's per-sensor dict.  With several sources, source 1 sits tick 2 out: its stale, masked frame is masked again."""
        out = []
        for i in range(1, last + 1):
            fr = [(s['F'] if which == 'F' else s['per'][sensor][which])[i] for s in self.src]
            if idle and self.C > 1 and i == 2:
                fr[1] = None
            out.append(fr)
        return out

    def process(self, tr, frames):
        if self.kind == 'hand':
            return [tr.process(frames[0], return_crop=True)]
        return tr.process(frames, return_crop=True)

    def sequence(self, tr, ticks):
        if self.kind == 'hand':
            return [[r] for r in tr.process_sequence([t[0] for t in ticks], return_crops=True)]
        return tr.process_sequence(ticks, return_crops=True)

    def learn(self, tr, sensor):
        for i in range(NLEARN):
            fr = _feed([s['learn'][i] for s in self.src], sensor)
            if self.C > 1 and i == 0:                                  # one source at a time is allowed too
                tr.learn_background([fr[0]] + [None] * (self.C - 1))
                tr.learn_background([None] + fr[1:])
            elif self.kind == 'hand':
                tr.learn_background(fr[0])
            else:
                tr.learn_background(fr)

    def model(self, tr, c):
        return tr.background_model() if self.kind == 'hand' else tr.background_model(c)

    def set_model(self, tr, c, m):
        if self.kind == 'hand':
            tr.set_background_model(m)
        else:
            tr.set_background_model(c, m)


def _same_ticks(a, b, where):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert [r['status'] for r in x] == [r['status'] for r in y], (where, i)
        for t, (p, q) in enumerate(zip(x, y)):
            if p['status'] == 0:
                _same(p, q, (where, i, t))


KINDS = ['hand', 'multi', 'hetero']


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('sensor', [False, True], ids=['f32', 'sensor'])
@pytest.mark.parametrize('kind', KINDS)
def test_unlearned_model_is_the_tracker_without_the_option(backend, kind, sensor):
    """(a): every key of every tick, bit for bit."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    rig = _Rig(rt, backend, kind)
    kw = dict(sensor=SENSOR) if sensor else {}
    a, b = rig.build(**kw), rig.build(background=SPEC, **kw)
    rig.start(a)
    rig.start(b)
    ticks = [_feed(t, sensor) for t in rig.ticks('F')]
    ra, rb = [rig.process(a, t) for t in ticks], [rig.process(b, t) for t in ticks]
    assert all(r['status'] in (0, 2) for tick in ra for r in tick) and any(r['status'] == 0 for r in ra[-1])
    assert all(set(p) == set(q) for x, y in zip(ra, rb) for p, q in zip(x, y))          # no key more, none less
    _same_ticks(ra, rb, 'unlearned')
    m = rig.model(b, 0)
    assert np.all(np.isinf(m['cut'])) and not m['near'].any() and not m['seen'].any()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('sensor', [False, True], ids=['f32', 'sensor'])
@pytest.mark.parametrize('kind', KINDS)
def test_learned_model_equals_the_plain_tracker_on_the_masked_frames(backend, kind, sensor):
    """(b) process(F) against a tracker without the option (and without a sensor) fed the restatement's masked frames; (c)
    process_sequence against the process() loop; (f) the model's round trip into a new tracker, and clear_background."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    rig = _Rig(rt, backend, kind)
    kw = dict(sensor=SENSOR) if sensor else {}
    a, b = rig.build(), rig.build(background=SPEC, **kw)
    rig.learn(b, sensor)
    for c in range(rig.C):                                                               # the model is the restatement's
        m, ref = rig.model(b, c), rig.src[c]['per'][sensor]
        assert np.array_equal(m['near'], ref['near']) and np.array_equal(m['seen'], ref['seen']) and np.array_equal(m['cut'], ref['cut']), c
        assert m['seen'].max() == NLEARN and np.isfinite(m['cut']).mean() > 0.9
        assert (ref['masked'] != ref['frames']).mean() > 0.5 and ref['masked'].any()     # the wall and the slab go, the hand stays
        r_, c_, _ = _slab(*rig.sizes[c])
        r_, c_ = slice(r_.start + 1, r_.stop - 1), slice(c_.start + 1, c_.stop - 1)          # (the median moves the slab's outline)
        assert not ref['masked'][:, r_, c_].any() and (ref['frames'][:, r_, c_] == 300.).all()
    rig.start(a)
    rig.start(b)
    want = [rig.process(a, t) for t in rig.ticks('masked', sensor)]
    ticks = [_feed(t, sensor) for t in rig.ticks('F')]
    got = [rig.process(b, t) for t in ticks]
    assert all(r['status'] in (0, 2) for tick in want for r in tick) and any(r['status'] == 0 for r in want[-1])
    _same_ticks(want, got, 'learned')
    rig.start(b)                                                                         # (c) both input sets against the one cut map
    _same_ticks(want, rig.sequence(b, ticks), 'sequence')
    c2 = rig.build(background=SPEC, **kw)                                                # (f) learn once, reload
    for c in range(rig.C):
        rig.set_model(c2, c, rig.model(b, c))
        assert np.array_equal(rig.model(c2, c)['cut'], rig.src[c]['per'][sensor]['cut'])
    rig.start(c2)
    _same_ticks(want[:1], [rig.process(c2, ticks[0])], 'reloaded')
    c2.clear_background()
    plain = rig.build(**kw)
    rig.start(plain)
    rig.start(c2)
    _same_ticks([rig.process(plain, ticks[0])], [rig.process(c2, ticks[0])], 'cleared')
    assert np.all(np.isinf(rig.model(c2, 0)['cut']))


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('kind', KINDS)
def test_background_plan_structure(backend, kind):
    """(d)"""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    rig = _Rig(rt, backend, kind)
    lib_ = rt.lib
    hetero = kind == 'hetero'
    plan = (lambda tr, slot: tr.plan(slot))
    old = rig.build()
    names = [l.name for l in plan(old, 0).launches()]
    assert names[0] == 'frame_range' and plan(old, 0).launches()[0].fn is (lib_.dpp_frame_range_src if hetero else lib_.dpp_frame_range)
    assert 'frame_background' not in names and old.bg is None and old.background is None
    tr = rig.build(background=SPEC)
    for slot in (0, 1):
        la = plan(tr, slot).launches()
        assert [l.name for l in la] == ['frame_background'] + names[1:]
        assert la[0].fn is (lib_.dpp_frame_background_src if hetero else lib_.dpp_frame_background)
        frames = (tr.frames[slot] if kind == 'hand' else (tr.frames if slot == 0 else tr._inputs2))
        assert la[0].args[0] == frames.ptr and la[0].args[1] == tr.bg.cut.ptr and la[0].args[-1] == tr.partial.ptr
    sens_old = rig.build(sensor=SENSOR)
    snames = [l.name for l in plan(sens_old, 0).launches()]
    assert snames == ['frame_ingest'] + names[1:] and plan(sens_old, 0).launches()[0].args[6 if hetero else 7] == sens_old.partial.ptr
    sens = rig.build(background=SPEC, sensor=SENSOR)
    for slot in (0, 1):
        la = plan(sens, slot).launches()
        assert [l.name for l in la] == ['frame_ingest', 'frame_background'] + names[1:] and len(la) == len(names) + 1
        assert la[0].args[6 if hetero else 7] is None and la[1].args[-1] == sens.partial.ptr          # ingest writes no partials
        assert la[1].args[0] == (sens.frames[slot] if kind == 'hand' else sens.frames).ptr and la[1].args[1] == sens.bg.cut.ptr
    det = tr.detector() if kind == 'hand' else tr.detector(0)
    dn = [l.name for l in det.plan(False).launches()]
    don = [l.name for l in (old.detector() if kind == 'hand' else old.detector(0)).plan(False).launches()]
    assert don[0] == 'frame_range' and dn == ['frame_background'] + don[1:]
    assert [l.name for l in det.stage(False, with_range=False)] == don[1:]
    sd = sens.detector() if kind == 'hand' else sens.detector(0)
    sn = [l.name for l in sd.plan(False).launches()]
    assert sn == ['frame_ingest', 'frame_background'] + don[1:] and [l.name for l in sd.stage(False)] == sn
    assert sd.plan(False).launches()[0].args[7] is None
    cut0 = sens.bg.view(sens.bg.cut, 0)
    assert sd.plan(False).launches()[1].args[1] == cut0.ptr                              # a view of the tracker's own cut map


def _inside(com, H, W):
    r, c, _ = _slab(H, W)
    return r.start <= com[1] < r.stop and c.start <= com[0] < c.stop


@pytest.mark.parametrize('backend', BACKENDS)
def test_acquire_sees_the_masked_frame(backend):
    """(e) the detector: a static slab of more than 200 px nearer than the hand takes acquire / acquire_source; with the learned model they
    return what the plain tracker returns on the restatement's masked frame."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    rig = _Rig(rt, backend, 'hand')
    H, W = rig.sizes[0]
    s = rig.src[0]
    F, ref = s['F'][0], s['per'][False]
    r_, c_, d = _slab(H, W)
    blob = (F > 400.) & (F < 800.)
    assert (F[r_, c_] == d).all() and F[r_, c_].size > 200 and d < F[blob].min() and blob.sum() > 1000     # larger than 200 px, nearer ...
    cols = np.flatnonzero(blob.any(0))
    assert cols.max() + 8 < c_.start and not blob[r_, c_].any()                          # ... and apart from the blob
    a, b = rig.build(), rig.build(background=SPEC)
    got = a.acquire(F)
    assert got['found'] and _inside(got['com'], H, W) and got['com'][2] < 340.  # without the option: the slab
    rig.learn(b, False)
    want = a.acquire(ref['masked'][0])
    for hs in (False, True):
        want, got = a.acquire(ref['masked'][0], do_hand_size=hs), b.acquire(F, do_hand_size=hs)
        assert want['found'] and got['found'] and not b.lost and not _inside(got['com'], H, W)
        assert got['com'].tobytes() == want['com'].tobytes() and got['cube'].tobytes() == want['cube'].tobytes(), hs
    assert np.hypot(got['com'][0] - s['coms'][0][0], got['com'][1] - s['coms'][0][1]) < 40. and got['com'][2] > 340.
    assert np.array_equal(b.frames[0].get()[0], ref['masked'][0])                        # what hand_size() and visibility look at
    assert np.array_equal(a.hand_size(), b.hand_size())
    assert b.process(F)['status'] == 0
    # two hands on one source
    rig2 = _Rig(rt, backend, 'multi')
    s0 = rig2.src[0]
    F2 = np.array(s0['F'][0])
    F2[H - 40:H - 10, 2:28] = 500.                                                       # a second hand, below and left of the blob
    ma, mb = rig2.build(), rig2.build(background=SPEC)
    first = ma.acquire_source(0, F2)
    assert first[0]['found'] and _inside(first[0]['com'], H, W)                          # without the option the slab is the first hand
    rig2.learn(mb, False)
    ma2 = rig2.build()
    want, got = ma2.acquire_source(0, G.apply(F2, s0['per'][False]['cut'])), mb.acquire_source(0, F2)
    assert [o['found'] for o in got] == [o['found'] for o in want] and got[0]['found']      # (at 120 x 160 one hand may lie in the other's seed window)
    for w, g in zip(want, got):
        assert g['com'].tobytes() == w['com'].tobytes() and not _inside(g['com'], H, W)
    w1, g1 = ma2.acquire(2, rig2.src[1]['per'][False]['masked'][0]), mb.acquire(2, rig2.src[1]['F'][0])
    assert g1['found'] and g1['com'].tobytes() == w1['com'].tobytes()


@pytest.mark.parametrize('backend', BACKENDS)
def test_background_options_and_frames_are_validated(backend):
    """(g)"""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    assert ops.background_spec(dict(margin=20)) == (20., 0., 1) and ops.background_spec((1., 0.5, 3)) == (1., 0.5, 3)
    assert ops.background_spec(dict(margin=0, rel=0.25, min_seen=4)) == (0., 0.25, 4)
    for bad in (dict(), dict(rel=0.1), dict(margin=-1.), dict(margin=np.nan), dict(margin=np.inf), dict(margin=5., rel=1.), dict(margin=5., rel=-0.1),
                dict(margin=5., min_seen=0), dict(margin=5., min_seen=1.5), dict(margin=5., blur=3), dict(margin='x'), 20.):
        with pytest.raises(ValueError):
            ops.background_spec(bad)
    rig = _Rig(rt, backend, 'hand')
    H, W = rig.sizes[0]
    with pytest.raises(ValueError):
        rig.build(background=dict(margin=5., every=2))
    tr = rig.build(background=SPEC)
    with pytest.raises(ValueError):
        tr.learn_background(np.zeros((H, W + 1), np.float32))
    with pytest.raises(ValueError):
        tr.set_background_model(dict(near=np.zeros((H, W + 1), np.float32), seen=np.zeros((H, W + 1), np.int32)))
    for fn in (lambda t: t.learn_background(np.zeros((H, W), np.float32)), lambda t: t.background_model(), lambda t: t.clear_background()):
        with pytest.raises(RuntimeError):
            fn(rig.build())
    sens = rig.build(background=SPEC, sensor=SENSOR)
    with pytest.raises(ValueError):
        sens.learn_background(np.zeros((H, W), np.float32))                              # not the sensor's dtype
    m = _Rig(rt, backend, 'hetero')
    mt = m.build(background=SPEC)
    with pytest.raises(ValueError):
        mt.learn_background([np.zeros(m.sizes[0], np.float32)])                          # one frame for three sources
    with pytest.raises(ValueError):
        mt.learn_background([np.zeros(m.sizes[0], np.float32)] * 3)                      # source 1 delivers another size
    with pytest.raises(IndexError):
        mt.background_model(3)
    with pytest.raises(RuntimeError):
        m.build().learn_background([None] * 3)
    assert len(mt.background_model()) == 3 and mt.background_model(1)['cut'].shape == m.sizes[1]
    from hipdp.detect import FrameDetector
    with pytest.raises(ValueError):
        FrameDetector(rt, H, W, 241.42, 241.42, 1, cut=tr.bg.cut)                        # a cut map without its options
    det = FrameDetector(rt, H, W, 241.42, 241.42, 2, background=SPEC)                    # a detector of its own owns a model
    assert det.bg is not None and det.cut is det.bg.cut and np.all(np.isinf(det.cut.get()))
    assert [l.name for l in det.plan(False).launches()][0] == 'frame_background'


# ---- 4: the pipelines and the example ----------------------------------------------------------------------------------------------
FX = FY = 241.42


def _files(tmp_path, name, frames, coms, cam):
    from tests.test_realtime import _write_icvl_sequence
    base = str(tmp_path / 'ICVL')
    frames, _ = _write_icvl_sequence(base, name, frames, coms, cam)
    return base, [os.path.join(base, 'Depth', '201403121135', '%s_%04d.png' % (name, i)) for i in range(len(frames))], frames


@pytest.mark.parametrize('backend', BACKENDS)
def test_pipeline_learns_the_background_and_follows_the_blob(backend, tmp_path):
    from tests.test_detect import _ListDevice
    from util.cameradevice import FileDevice
    from util.realtimehandposepipeline import RealtimeHandposePipeline
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    rig = _Rig(rt, backend, 'hand')
    H, W = rig.sizes[0]
    s = rig.src[0]
    ref = s['per'][False]
    base, files, empty = _files(tmp_path, 'empty', s['learn'], s['coms'][:NLEARN], A.Camera.icvl())
    assert np.array_equal(empty, s['learn'])
    di = ICVLImporter(base, useCache=False)
    config = {'fx': FX, 'fy': FY, 'cube': (250, 250, 250)}
    rtp = RealtimeHandposePipeline(rig.pnet, dict(config), di, comrefNet=rig.snet, seed_detect=True, background=SPEC)
    model = rtp.learnBackground(FileDevice(files, di), frames=NLEARN)
    assert np.array_equal(model['near'], ref['near']) and np.array_equal(model['seen'], ref['seen']) and np.array_equal(model['cut'], ref['cut'])
    poses = rtp.processVideo(_ListDevice(list(s['F'][:3])))
    plain = RealtimeHandposePipeline(rig.pnet, dict(config), di, comrefNet=rig.snet, seed_detect=True)
    want = plain.processVideo(_ListDevice(list(ref['masked'][:3])))
    assert poses.shape == (3, 14, 3) and np.array_equal(poses, want)                 # every frame followed, the plain pipeline's bits
    assert np.hypot(rtp.lastcom[0] - s['coms'][2][0], rtp.lastcom[1] - s['coms'][2][1]) < 40. and rtp.lastcom[2] > 340.     # the blob
    lost = RealtimeHandposePipeline(rig.pnet, dict(config), di, comrefNet=rig.snet, seed_detect=True)
    lost.initNets()
    lost.processFrame(s['F'][0])
    assert lost._tracker.com.get()[0][2] < 340. or np.allclose(lost.lastcom, 0)           # without the option: seeded on the slab
    with pytest.raises(RuntimeError, match="ran out of frames"):
        rtp.learnBackground(FileDevice(files, di), frames=NLEARN + 1)
    with pytest.raises(RuntimeError):
        plain.learnBackground(FileDevice(files, di), frames=1)


@pytest.mark.parametrize('backend', BACKENDS)
def test_multi_stream_pipeline_learns_the_background(backend):
    from tests.test_detect import _ListDevice
    from util.realtimehandposepipeline import MultiStreamPipeline
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    rig = _Rig(rt, backend, 'multi')
    config = {'fx': FX, 'fy': FY, 'cube': (250, 250, 250)}
    Lh, Rh = MultiStreamPipeline.HAND_LEFT, MultiStreamPipeline.HAND_RIGHT
    hands = [(c, Rh if right else Lh) for c, right in rig.tracks]
    init = [rig.src[c]['coms'][0] for c, _ in rig.tracks]

    def pipe(which, sensor=False, **kw):
        devs = [_ListDevice(list((s[which] if which in s else s['per'][sensor][which])[1:3])) for s in rig.src]
        return MultiStreamPipeline(rig.pnet, dict(config), rig.dis[0], devs, hands, rig.snet, init_com=init, **kw)
    msp = pipe('F', background=SPEC)
    learn_devs = msp.devices
    msp.devices = [_ListDevice(list(s['learn'])) for s in rig.src]
    models = msp.learnBackground(NLEARN)
    for c, m in enumerate(models):
        assert np.array_equal(m['cut'], rig.src[c]['per'][False]['cut']), c
    with pytest.raises(RuntimeError, match="ran out of frames"):
        msp.learnBackground(NLEARN + 1)
    msp.devices = learn_devs
    got, want = msp.processVideos(), pipe('masked').processVideos()
    assert len(got) == len(want) == len(hands)
    for g, w in zip(got, want):
        assert g.shape == (2, 14, 3) and np.array_equal(g, w)
    with pytest.raises(RuntimeError):
        pipe('F').learnBackground(1)


@pytest.mark.parametrize('backend', BACKENDS)
def test_realtime_background_example(backend, tmp_path):
    R.set_default_runtime(get_runtime(backend))
    cam, cube, H, W = A.Camera.icvl(), (250., 250., 250.), 120, 160
    frames, coms = T.drifting_sequence(np.random.RandomState(36), 3, cam, H, W, cube)
    base, _, _ = _files(tmp_path, 'test_seq_1', frames, coms, cam)
    net = 'resnet' if backend == 'hip' else 'poseregnet'               # (the 128x128 ResNet is too slow for the SIMT emulator)
    mods = {}
    for name in ('test_realtimepipeline', 'realtime_background'):
        spec = importlib.util.spec_from_file_location('background_' + name, os.path.join(ROOT, 'examples', name + '.py'))
        mods[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    common = ['--dataset', 'icvl', '--data', base, '--net', net, '--cache', str(tmp_path / 'cache')]
    main = mods['realtime_background'].main
    plain, err0 = mods['test_realtimepipeline'].main(common)
    same, err1 = main(common)
    assert np.array_equal(same, plain) and err1 == err0               # without the flags: the plain example's output
    r_, c_, d = _slab(H, W)
    clutter = '%d:%d:%d:%d:%g' % (c_.start, r_.start, c_.stop, r_.stop, d)
    poses, err, fig = main(common + ['--background', '50', '0.01', '--learn', '2', '--clutter', clutter])
    assert poses.shape == (3, 16, 3) and np.isfinite(poses).all() and np.isfinite(err)
    assert fig['without']['found'] and _inside(fig['without']['com'], H, W)             # the slab takes the detector ...
    assert fig['with_model']['found'] and not _inside(fig['with_model']['com'], H, W) and fig['with_model']['com'][2] > 340.     # ... until it is learned
    assert 0.7 < fig['known'] < 1.                                    # (where the hand was taken out nothing was seen)
    assert mods['realtime_background'].base.FileDevice is mods['realtime_background'].FileDevice      # the example's names are put back
    with pytest.raises(SystemExit):
        main(common + ['--clutter', clutter])
    with pytest.raises(SystemExit):
        main(common + ['--background', '50', '0.01', '--clutter', '5:5:3:9:300'])
    # the same options on examples/realtime_multi.py: two cameras (here: the one sequence twice), the third track found by detection
    spec = importlib.util.spec_from_file_location('background_realtime_multi', os.path.join(ROOT, 'examples', 'realtime_multi.py'))
    multi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(multi)
    seqs = ['--seqs', 'test_seq_1', 'test_seq_1', '--seed', 'detect', '--max-frames', '2']
    made, Msp = [], multi.MultiStreamPipeline

    class Recorded(Msp):                                               # the example's pipeline, kept for a look at its tracker
        def __init__(self, *a, **k):
            made.append(self)
            super(Recorded, self).__init__(*a, **k)
    multi.MultiStreamPipeline = Recorded
    try:
        mposes, _ = multi.main(common + seqs + ['--background', '50', '0.01', '--learn', '2', '--clutter', clutter])
    finally:
        multi.MultiStreamPipeline = Msp
    assert [q.shape for q in mposes] == [(2, 16, 3)] * 3 and all(np.isfinite(q).all() for q in mposes)
    com = made[-1]._tracker.com_host[2]                                # the detector started camera 1's track on the hand, not on the slab
    assert not _inside(com, H, W) and com[2] > 340. and np.hypot(com[0] - coms[1][0], com[1] - coms[1][1]) < 40.
    assert made[-1].background_known[1] > 0.7
    with pytest.raises(SystemExit):
        multi.main(common + seqs + ['--clutter', clutter])
    with pytest.raises(SystemExit):
        multi.main(common + seqs + ['--background', '50', '0.01', '--fuse'])


# ---- 5: the ABI --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_abi_version_is_25(backend):
    rt = get_runtime(backend)
    with open(os.path.join(ROOT, 'include', 'dpp_hip.h')) as fh:
        header = fh.read()
    assert re.search(r'#define DPP_ABI_VERSION (\d+)', header).group(1) == '25'
    assert lib.ABI_VERSION == 25 and rt.lib.dpp_abi_version() == 25
    for name in ('dpp_frame_background', 'dpp_frame_background_src', 'dpp_background_learn', 'dpp_background_learn_src'):
        assert name in header and hasattr(rt.lib, name)
