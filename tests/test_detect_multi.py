"""Several hands of one frame in one detector plan (csrc/components.hip: comp_candidates, detect_select, detect_seeds; crop.hip:
refine_com_iterative_ix; hipdp/detect.py hands=K; util.handdetector.find_hands(max_hands=); MultiTracker.acquire_source;
MultiStreamPipeline) against the NumPy restatement of tests/detect_multi_ref.py.  Everything compared is an integer, a float64 of
exact sums or a float32 store of one: every comparison is np.array_equal.  Frames are 120 x 160 unless a scene needs more room (the
seed window is +-100 px); the ICVL camera."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from data.importers import ICVLImporter
from hipdp import ops
from hipdp import runtime as R
from tests import detect_multi_ref as M
from tests import detect_ref as D
from tests.backends import BACKENDS, get_runtime

FX = FY = 241.42
CUBE = (250., 250., 250.)
BADARG = 10001


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def _wall(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    f = (1400. + ((xx * 7 + yy * 3) % 11)).astype(np.float32)
    f[::9, ::7] = 0.                                 # holes: the frame's minimum is 0, the detector's 10
    f[4::31, 5::29] = 2000.                          # beyond maxDepth: the detector's maximum is 1500, no pixel has it
    return f


def _put(f, y0, x0, h, w, d):
    yy, xx = np.mgrid[0:h, 0:w]
    f[y0:y0 + h, x0:x0 + w] = (d + ((xx + 2 * yy) % 5)).astype(np.float32)


def _specks(f, H, W, d=303.):
    for y0, x0 in ((2, W // 2), (H // 2, 3), (H - 12, W // 3)):
        _put(f, y0, x0, 9, 8, d)                     # 72 px each, 8-disconnected from one another


# With the wall's range (10, 1500) a slab is 74.5 mm deep: 503.. lies in slab 6, 580.. in 7, 660.. in 8, the wall in 18.
def _scene(kind):
    """(frame, max_extent).  Block centroids: a block of odd width w at x0 has cx = x0 + (w - 1) / 2 exactly."""
    H, W, ext = 120, 160, None
    if kind in ('open_y', 'open_y_inside', 'hand_wall_extent', 'many'):
        H, W = 240, 320
    f = _wall(H, W)
    if kind == 'same_slab':                          # 1: centroids 130 px apart in x, the right one first in raster order
        _put(f, 50, 5, 24, 21, 503.)
        _put(f, 40, 135, 24, 21, 503.)
    elif kind == 'by_key':                           # 2: the nearer block comes later in raster order
        _put(f, 20, 5, 24, 21, 660.)
        _put(f, 70, 135, 24, 21, 503.)
    elif kind == 'two_slabs_one_hand':               # 3: one hand over two adjacent slabs, touching
        _put(f, 50, 60, 24, 20, 503.)
        _put(f, 50, 80, 30, 20, 580.)
    elif kind == 'not_transitive':                   # 4: A; C in A's window (suppressed); D near C, outside A's window: A and D
        _put(f, 40, 0, 24, 21, 503.)                 # A: cx 10, window x [0, 110)
        _put(f, 40, 90, 24, 21, 580.)                # C: cx 100
        _put(f, 40, 140, 24, 20, 660.)               # D: cx 149.5 -> 150
    elif kind in ('open_x', 'open_x_inside'):        # 5: the window [xs, xe) is open at cx_A + 100
        _put(f, 40, 0, 24, 21, 503.)                 # A: cx 10, xe = 110
        _put(f, 40, 100 if kind == 'open_x' else 99, 24, 21, 580.)       # cx 110: accepted; cx 109: suppressed
    elif kind in ('open_y', 'open_y_inside'):        # ... and at cy_A + 100, with room for it at 240 x 320
        _put(f, 0, 40, 21, 24, 503.)                 # A: cy 10, ye = 110
        _put(f, 100 if kind == 'open_y' else 99, 40, 21, 24, 580.)
    elif kind == 'three':                            # 6: three that do not suppress one another: C lies below both windows in y
        _put(f, 0, 0, 21, 21, 503.)                  # A: (10, 10), window [0, 110) x [0, 110)
        _put(f, 0, 139, 21, 21, 580.)                # B: (149, 10), window [49, 159) x [0, 110)
        _put(f, 110, 60, 10, 41, 660.)               # C: (80, 114.5 -> 114)
    elif kind == 'wall':                             # 7: the wall alone ...
        pass
    elif kind == 'wall_extent':                      # ... is no hand under an extent of 500 mm
        ext = 500.
    elif kind == 'hand_wall_extent':                 # ... and does not become the second hand of a frame that holds one
        _put(f, 100, 150, 24, 21, 503.)
        ext = 500.
    elif kind == 'empty':                            # 8
        f[:] = 0.
    elif kind == 'specks':
        f[:] = 0.
        f[4::31, 5::29] = 2000.
        _specks(f, H, W)
    elif kind == 'many':                             # 9: 320 candidates of 210 px in one slab, zero gaps, a list longer than a workgroup
        f[:] = 0.
        for y0 in range(0, H, 15):
            for x0 in range(0, W, 16):
                _put(f, y0, x0, 14, 15, 503.)
        f[14::15, 15::16] = 2000.                    # gap crossings beyond maxDepth: the range is (10, 1500) as with the wall
    else:
        raise KeyError(kind)
    return f, ext


SCENES = ['same_slab', 'by_key', 'two_slabs_one_hand', 'not_transitive', 'open_x', 'open_x_inside', 'open_y', 'open_y_inside', 'three',
          'wall', 'wall_extent', 'hand_wall_extent', 'empty', 'specks']


def _check_scene_conditions(f, st, small=100, big=400):
    """On the reference alone: what keeps the documented deviations of the labelling out of the comparison."""
    mn, mx = D.depth_range(f)
    inr = f[(f != 0) & (f >= mn) & (f <= mx)]
    assert not np.isin(inr.astype(np.float64), D.slab_bounds(mn, mx)).any()              # no depth on a slab boundary
    assert ((st['count'] >= big) | (st['count'] <= small)).all()                            # nothing near the area threshold


@functools.lru_cache(maxsize=None)
def _ref(kind, K, cube=CUBE):
    f, ext = _scene(kind)
    r = M.find_hands_ref(f, cube, FX, FY, K, ext)
    f.setflags(write=False)
    return f, ext, r


def _detect(rt, frames, cubes, K, ext):
    """FrameDetector(hands=K).run through the per-shape cache of util.handdetector: (coms, cubes, found, seeds, status, report)."""
    from util.handdetector import _detector
    frames = np.ascontiguousarray(frames, np.float32)
    B, H, W = frames.shape
    det = _detector(rt, H, W, FX, FY, B, K, ext)
    return det, _k_axis(det, det.run(frames, np.float32(cubes).reshape(B, 3)))


def _k_axis(det, out):
    """hands=1 without an extent IS today's detector, with today's result: give it the K axis; it has no report."""
    if det.multi:
        return out
    coms, cubes, found, seeds, status = out
    return coms[:, None], cubes[:, None], found[:, None], seeds[:, None], status[:, None], None


def _equal(got, b, r, what):
    coms, cubes, found, seeds, status, report = got
    assert np.array_equal(found[b], r['found']), (what, found[b], r['found'])
    assert np.array_equal(seeds[b], r['seed']), (what, seeds[b], r['seed'])
    assert np.array_equal(coms[b], r['com']), (what, coms[b], r['com'])
    assert np.array_equal(status[b], r['found'].astype(np.int32))
    if report is None:
        return
    assert np.array_equal(report['refine_status'][b], r['refine_status']), what
    for n in M.REPORT:
        assert np.array_equal(report[n][b], r['report'][n]), (what, n, report[n][b], r['report'][n])


# ---- 1 - 8: the scenes against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('kind', SCENES)
def test_scene_equals_the_restatement(backend, kind, K):
    rt = get_runtime(backend)
    f, ext, r = _ref(kind, K)
    _check_scene_conditions(f, r['stats'])
    det, got = _detect(rt, f[None], [CUBE], K, ext)
    coms, cubes, found, seeds, status, report = got
    assert coms.shape == seeds.shape == cubes.shape == (1, K, 3) and found.shape == (1, K) and coms.dtype == np.float32
    _equal(got, 0, r, kind)
    assert np.array_equal(cubes[0], np.tile(np.float32(CUBE), (K, 1)))
    # what the scene is for, on the restatement (the comparison above carries it over to the kernels)
    want = {'same_slab': [1, 1, 0], 'by_key': [1, 1, 0], 'two_slabs_one_hand': [1, 0, 0], 'not_transitive': [1, 1, 0], 'open_x': [1, 1, 0],
            'open_x_inside': [1, 0, 0], 'open_y': [1, 1, 1], 'open_y_inside': [1, 0, 1], 'three': [1, 1, 1], 'wall': [1, 0, 0],
            'wall_extent': [0, 0, 0], 'hand_wall_extent': [1, 0, 0], 'empty': [0, 0, 0], 'specks': [0, 0, 0]}[kind]
    if kind == 'open_y_inside':                      # at 240 x 320 the wall's centroid lies outside A's window: it is the second
        want = [1, 1, 0]
    assert list(r['found']) == [bool(w) for w in want[:K]], (kind, r['found'])
    rep = r['report']
    for k in range(K):
        if not r['found'][k]:                        # empty slots: all zero, the refinement stopped at once
            assert not r['seed'][k].any() and not r['com'][k].any() and r['refine_status'][k] == 1
            assert not any(rep[n][k] for n in M.REPORT)
    if K >= 2:
        if kind == 'same_slab':                      # one slab: raster order, the right block's rows come first
            assert rep['key'][0] == rep['key'][1] == 6 and rep['xmin'][0] == 135 and rep['xmin'][1] == 5
        if kind == 'by_key':                         # the nearer slab first, though it is later in raster order
            assert list(rep['key'][:2]) == [6, 8] and rep['ymin'][0] == 70 and rep['ymin'][1] == 20
        if kind == 'not_transitive':                 # A and D: C (slab 7) was suppressed and suppressed nothing
            assert list(rep['key'][:2]) == [6, 8] and rep['xmin'][1] == 140
        if kind == 'open_x':
            assert list(rep['key'][:2]) == [6, 7] and rep['xmin'][1] == 100
        if kind == 'open_y':
            assert list(rep['key'][:2]) == [6, 7] and rep['ymin'][1] == 100
        if kind == 'three':
            assert list(rep['key'][:2]) == [6, 7]
    if K == 3 and kind == 'three':
        assert rep['key'][2] == 8 and rep['ymin'][2] == 110
    if kind in ('wall', 'hand_wall_extent'):
        assert rep['key'][0] == (18 if kind == 'wall' else 6)
    # the class API and the batched one give the same answer
    from util.handdetector import HandDetector, find_hands
    c2, s2, f2, e2 = find_hands(f[None], [CUBE], FX, FY, runtime=rt, return_seed=True, max_hands=K, max_extent=ext)
    if K == 1:
        assert c2.shape == (1, 3) and f2.shape == (1,)
        assert np.array_equal(c2[0], coms[0][0]) and np.array_equal(e2[0], seeds[0][0]) and f2[0] == found[0][0]
    else:
        assert np.array_equal(c2, coms) and np.array_equal(e2, seeds) and np.array_equal(f2, found) and np.array_equal(s2, cubes)
        if kind == 'same_slab':
            R.set_default_runtime(rt)
            d = f.copy()
            d[d > 1500] = 0.                         # the constructor's zeroing leaves the detector's range as it is
            cc, size = HandDetector(f.copy(), FX, FY).detectComponents(size=CUBE, doHandSize=False, max_hands=K)
            assert cc.shape == (K, 3) and cc.dtype == np.float64 and size == CUBE
            assert np.array_equal(np.float32(cc), M.find_hands_ref(d, CUBE, FX, FY, K)['com'])


# ---- 9: a candidate list longer than the selecting workgroup ------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_more_candidates_than_the_workgroup_has_threads(backend):
    rt = get_runtime(backend)
    f, ext, r = _ref('many', 4)
    _check_scene_conditions(f, r['stats'], big=210)                                          # 15 x 14 = 210 px: exact counts, above 200
    assert (r['stats']['count'] > D.MIN_AREA).sum() == 320 > 256
    assert list(r['found']) == [True] * 4
    det, first = _detect(rt, f[None], [CUBE], 4, ext)
    _equal(first, 0, r, 'many')
    det.plan(False).run(rt)                          # the same plan object again: the counter is cleared inside the plan
    rt.synchronize()
    second = _k_axis(det, det.result())
    _equal(second, 0, r, 'many, second run')
    for a, b in zip(first[:5], second[:5]):
        assert np.array_equal(a, b)


# ---- 10: several frames, different cubes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_three_frames_of_different_scenes_and_cubes_in_one_run(backend):
    rt = get_runtime(backend)
    kinds, cubes = ['three', 'empty', 'by_key'], [(250., 250., 250.), (200., 200., 200.), (300., 280., 260.)]
    refs = [_ref(k, 3, c) for k, c in zip(kinds, cubes)]
    _, got = _detect(rt, np.stack([r[0] for r in refs]), cubes, 3, None)
    for b, (f, _, r) in enumerate(refs):
        _equal(got, b, r, kinds[b])
    assert np.array_equal(got[1], np.repeat(np.float32(cubes)[:, None], 3, axis=1))
    # the cube matters: the same frame refined with another cube ends elsewhere
    assert not np.array_equal(refs[2][2]['com'], _ref('by_key', 3)[2]['com'])


# ---- K = 1 is today's detector ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_one_hand_equals_today(backend):
    from hipdp.detect import FrameDetector
    from util.handdetector import find_hands
    rt = get_runtime(backend)
    for kind in SCENES + ['many']:
        f, ext, _ = _ref(kind, 1)
        if ext is not None:
            continue
        a = find_hands(f[None], [CUBE], FX, FY, runtime=rt, return_seed=True)
        b = find_hands(f[None], [CUBE], FX, FY, runtime=rt, return_seed=True, max_hands=1)
        for x, y in zip(a, b):
            assert x.shape == y.shape and np.array_equal(x, y), kind
        # ... and the several-hands launches at K = 1 give the same bits (an extent no component reaches switches them on)
        c = find_hands(f[None], [CUBE], FX, FY, runtime=rt, return_seed=True, max_hands=1, max_extent=1e9)
        for x, y in zip(a, c):
            assert x.shape == y.shape and np.array_equal(x, y), kind
    # one hand under an extent filter may still be measured: the hand-size stage behind the several-hands launches
    f = _ref('by_key', 1)[0]
    a = find_hands(f[None], [CUBE], FX, FY, runtime=rt, do_hand_size=True)
    c = find_hands(f[None], [CUBE], FX, FY, runtime=rt, do_hand_size=True, max_extent=1e9)
    assert a[2][0] and not np.array_equal(a[1][0], np.float32(CUBE))
    for x, y in zip(a, c):
        assert x.shape == y.shape and np.array_equal(x, y)
    det = FrameDetector(rt, 120, 160, FX, FY, 1, hands=1)
    stage = det.stage()
    assert [op.name for op in stage] == ['frame_range', 'slab_keys', 'label_components', 'detect_seed', 'detect_refine']
    assert sum(op.kernels for op in stage) == 9 and not det.multi and det.ws.candidates is None
    assert det.res.size == 8 and det.com.size == 3
    multi = FrameDetector(rt, 120, 160, FX, FY, 1, hands=5)
    stage = multi.stage()
    assert [op.name for op in stage] == ['frame_range', 'slab_keys', 'label_components', 'detect_seeds', 'detect_refine']
    assert sum(op.kernels for op in stage) == 10                                             # at most two more than nine, for any K
    with pytest.raises(ValueError):
        multi.stage(do_hand_size=True)
    with pytest.raises(ValueError):
        find_hands(np.zeros((1, 8, 8), np.float32), [CUBE], FX, FY, runtime=rt, do_hand_size=True, max_hands=2)
    with pytest.raises(ValueError):
        FrameDetector(rt, 120, 160, FX, FY, 1, hands=17)
    with pytest.raises(ValueError):
        FrameDetector(rt, 120, 160, FX, FY, 1, hands=0)


# ---- refine_com_iterative_ix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_refine_com_iterative_ix_equals_the_plain_launch_on_gathered_frames(backend):
    rt = get_runtime(backend)
    H, W = 37, 45
    rng = np.random.RandomState(7)
    frames = np.stack([_wall(H, W), _wall(H, W)[::-1].copy()])
    _put(frames[0], 5, 8, 12, 14, 503.)
    _put(frames[1], 18, 22, 14, 12, 640.)
    cubes = np.float32([(250., 250., 250.), (180., 200., 220.)])
    src = np.int32([1, 0, 1, 1])
    coms = np.float32([(28., 25., 645.), (15., 11., 505.), (30., 20., 1400.), (0., 0., 0.)])
    coms[:3, :2] += rng.uniform(-2, 2, (3, 2)).astype(np.float32)

    def run(fr, cu, co, ix):
        n, C = len(co), len(fr)
        fb, cb, ib = rt.upload(np.ascontiguousarray(fr)), rt.upload(np.ascontiguousarray(cu)), rt.upload(np.ascontiguousarray(co))
        partial = ops.frame_range_workspace(rt, C)
        out, status = rt.alloc((n, 3), zero=False), rt.alloc((n,), np.int32, zero=False)
        ops.frame_range(rt, fb, C, H, W, partial)(rt.stream)
        if isinstance(ix, str):
            ops.refine_com_iterative(rt, fb, partial, n, H, W, ib, cb, FX, FY, 5, out, status)(rt.stream)
        else:
            sb = None if ix is None else rt.upload(ops.track_index(ix, C))
            ops.refine_com_iterative_ix(rt, fb, partial, n, sb, H, W, ib, cb, FX, FY, 5, out, status)(rt.stream)
        rt.synchronize()
        return out.get(), status.get()
    got, gst = run(frames, cubes, coms, src)
    want, wst = run(frames[src], cubes[src], coms, 'plain')
    assert got.tobytes() == want.tobytes() and np.array_equal(gst, wst) and list(wst) == [0, 0, 0, 1]
    assert not np.array_equal(got[0], got[2])                                                # rows of one frame, different centres
    null, nst = run(frames, cubes, coms[:2], None)                                           # a NULL src is the plain entry point
    plain, pst = run(frames, cubes, coms[:2], 'plain')
    assert null.tobytes() == plain.tobytes() and np.array_equal(nst, pst)


# ---- bad arguments -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_bad_arguments_are_refused_before_any_launch(backend):
    rt = get_runtime(backend)
    lib = rt.lib
    H, W = 16, 24
    ws = ops.ComponentWorkspace(rt, 1, H, W, candidates=True)
    fr, partial = rt.alloc((1, H, W)), ops.frame_range_workspace(rt, 1)
    seed, status, report = rt.alloc((16, 3)), rt.alloc((16,), np.int32), rt.alloc((16, 6), np.int32)
    seed.set(np.full((16, 3), 7., np.float32))

    def call(K=2, ext=0.0, fx=FX, fy=FY, null=None):
        p = dict(frames=fr.ptr, partial=partial.ptr, keys=ws.keys.ptr, labels=ws.labels.ptr, stats=ws.stats.ptr, state=ws.state.ptr,
                 cand=ws.candidates.ptr, seed=seed.ptr, status=status.ptr, report=report.ptr)
        if null:
            p[null] = None
        return lib.dpp_detect_seeds(p['frames'], p['partial'], p['keys'], p['labels'], p['stats'], 1, H, W, p['state'], p['cand'], K, ext, fx, fy,
                                    p['seed'], p['status'], p['report'], None)
    for K in (0, 17, -1):
        assert call(K=K) == BADARG
    for ext in (-1.0, float('nan'), float('inf'), -float('inf')):
        assert call(ext=ext) == BADARG
    assert call(ext=100., fx=0.0) == BADARG
    for name in ('frames', 'partial', 'keys', 'labels', 'stats', 'state', 'cand', 'seed', 'status', 'report'):
        assert call(null=name) == BADARG, name
    assert lib.dpp_detect_seeds(fr.ptr, partial.ptr, ws.keys.ptr, ws.labels.ptr, ws.stats.ptr, 1, 1 << 16, 1 << 16, ws.state.ptr,
                                ws.candidates.ptr, 2, 0.0, FX, FY, seed.ptr, status.ptr, report.ptr, None) == BADARG
    assert np.array_equal(seed.get(), np.full((16, 3), 7., np.float32))                      # nothing ran
    assert lib.dpp_detect_candidates_bytes(1, 1 << 16, 1 << 16) == 0
    assert lib.dpp_detect_candidates_bytes(2, 480, 640) == 2 * (2 * (480 * 640 // 201) + 16) * 8 and 480 * 640 // 201 == 1528
    assert lib.dpp_detect_candidates_bytes(1, 10, 20) == 16 * 8                              # fewer than 201 px: no candidate can exist
    assert lib.dpp_refine_com_iterative_ix(None, None, 1, None, 4, 4, None, None, 1., 1., 5, None, None, None) == BADARG
    assert lib.dpp_refine_com_iterative_ix(fr.ptr, partial.ptr, 0, None, H, W, seed.ptr, seed.ptr, 1., 1., 5, seed.ptr, status.ptr, None) == BADARG
    with pytest.raises(ValueError):
        ops.detect_seeds(rt, fr, partial, ops.ComponentWorkspace(rt, 1, H, W), 2, seed, status, report)


# ---- MultiTracker.acquire_source -------------------------------------------------------------------------------------------------
def _two_hands(H=120, W=160, left_z=503., right_z=580., right=True):
    """The left hand nearer than the right one: slot order (nearest first) is left, right; ascending x is the same -- unless the
    depths are swapped.  With MT_CUBE the refinement windows (+-24 px at 503 mm) do not reach over the left or the top frame edge,
    where refineCoMIterative's max(xstart, 0) would move the centre."""
    f = _wall(H, W)
    _put(f, 40, 26, 30, 24, left_z)                  # centroids 38 and 140: outside each other's window either way round
    if right:
        _put(f, 50, 128, 30, 24, right_z)
    return f


MT_CUBE = (100., 100., 100.)


def _mt(backend, tracks=((0, False), (0, True))):
    from hipdp.multitrack import MultiTracker
    from tests.test_multitrack import _nets
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, len(tracks))
    di = ICVLImporter('../data/ICVL/')
    return rt, di, snet, pnet, MultiTracker(rt, di, pnet, snet, 120, 160, MT_CUBE, list(tracks), fx=FX, fy=FY)


KEYS = ('pose', 'pose_img', 'com', 'com3D', 'M', 'crop')


@pytest.mark.parametrize('backend', BACKENDS)
def test_acquire_source_starts_both_tracks_of_a_source(backend):
    from hipdp.multitrack import MultiTracker
    rt, di, snet, pnet, mt = _mt(backend)
    f = _two_hands()
    ref = M.find_hands_ref(f, MT_CUBE, FX, FY, 2)
    assert list(ref['found']) == [True, True] and ref['com'][0][0] < 60 and ref['com'][1][0] > 120
    acq = mt.acquire_source(0, f)
    assert [a['found'] for a in acq] == [True, True] and not mt.lost.any()
    for k in range(2):
        assert np.array_equal(acq[k]['com'], ref['com'][k]) and np.array_equal(acq[k]['cube'], np.float32(MT_CUBE))
    got = mt.process([f], return_crop=True)
    other = MultiTracker(rt, di, pnet, snet, 120, 160, MT_CUBE, [(0, False), (0, True)], fx=FX, fy=FY)
    for t in range(2):
        other.reset(t, acq[t]['com'])
    want = other.process([f], return_crop=True)
    for t in range(2):
        assert got[t]['status'] == want[t]['status'] == 0
        for k in KEYS:
            assert np.array_equal(got[t][k], want[t][k]), (t, k)
    assert not np.array_equal(got[0]['com'], got[1]['com'])
    with pytest.raises(ValueError):
        mt.acquire_source(0, f, order='y')
    with pytest.raises(IndexError):
        mt.acquire_source(1, f)


@pytest.mark.parametrize('backend', BACKENDS)
def test_acquire_source_gives_a_lost_track_the_other_hand(backend):
    rt, di, snet, pnet, mt = _mt(backend)
    f = _two_hands()
    ref = M.find_hands_ref(f, MT_CUBE, FX, FY, 2)
    # track 0 follows the RIGHT hand (slot 1); track 1 is lost: it must get the left one (slot 0), track 0 keeps its centre's bits
    mt.reset(0, ref['com'][1])
    before = mt.com.get().copy()
    acq = mt.acquire_source(0, f)
    assert [a['found'] for a in acq] == [True, True] and not mt.lost.any()
    after = mt.com.get()
    assert after[0].tobytes() == before[0].tobytes() and np.array_equal(acq[0]['com'], ref['com'][1])
    assert np.array_equal(acq[1]['com'], ref['com'][0]) and np.array_equal(after[1], ref['com'][0])
    # one hand in view and two tracks: the second stays lost (the wall is farther than max_extent allows a hand to be wide)
    rt, di, snet, pnet, mt = _mt(backend)
    one = _two_hands(right=False)
    acq = mt.acquire_source(0, one, max_extent=500.)
    assert [a['found'] for a in acq] == [True, False] and list(mt.lost) == [False, True] and not acq[1]['com'].any()
    assert np.array_equal(acq[0]['com'], M.find_hands_ref(one, MT_CUBE, FX, FY, 2, 500.)['com'][0])
    res = mt.process([one])
    assert [r['status'] for r in res] == [0, 1]
    # the hand comes back: the lost track takes it, the followed one is left alone
    acq = mt.acquire_source(0, f, max_extent=500.)
    assert [a['found'] for a in acq] == [True, True] and not mt.lost.any()
    assert np.array_equal(acq[1]['com'], M.find_hands_ref(f, MT_CUBE, FX, FY, 2, 500.)['com'][1])


@pytest.mark.parametrize('backend', BACKENDS)
def test_acquire_source_order(backend):
    """The right hand nearer than the left one: 'near' hands slot 0 (the right hand) to track 0, 'x' the leftmost."""
    f = _two_hands(left_z=580., right_z=503.)
    ref = M.find_hands_ref(f, MT_CUBE, FX, FY, 2)
    assert list(ref['found']) == [True, True] and ref['com'][0][0] > 120 and ref['com'][1][0] < 60
    rt, di, snet, pnet, mt = _mt(backend)
    near = mt.acquire_source(0, f)
    assert np.array_equal(near[0]['com'], ref['com'][0]) and np.array_equal(near[1]['com'], ref['com'][1])
    mt.lost[:] = True
    byx = mt.acquire_source(0, f, order='x')
    assert np.array_equal(byx[0]['com'], ref['com'][1]) and np.array_equal(byx[1]['com'], ref['com'][0])
    assert np.array_equal(mt.com.get(), np.stack([ref['com'][1], ref['com'][0]]))


# ---- MultiStreamPipeline(seed_detect=True) -----------------------------------------------------------------------------------------
class _ListDevice(object):
    """A depth source over frames in memory with FileDevice's interface."""

    def __init__(self, frames):
        self.frames, self.i = frames, 0

    def start(self):
        self.i = 0

    def stop(self):
        pass

    def getDepth(self):
        if self.i >= len(self.frames):
            raise IndexError(self.i)
        self.i += 1
        return True, self.frames[self.i - 1].copy()


@pytest.mark.parametrize('backend', BACKENDS)
def test_pipeline_starts_two_hands_of_one_device_without_init_com(backend):
    from hipdp.multitrack import MultiTracker
    from tests.test_multitrack import _nets
    from util.realtimehandposepipeline import MultiStreamPipeline
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 2)
    di = ICVLImporter('../data/ICVL/')
    config = {'fx': FX, 'fy': FY, 'cube': MT_CUBE}
    L, Rr = MultiStreamPipeline.HAND_LEFT, MultiStreamPipeline.HAND_RIGHT
    f = _two_hands()
    msp = MultiStreamPipeline(pnet, dict(config), di, [_ListDevice([f, f])], [(0, L), (0, Rr)], snet, seed_detect=True, max_extent=500.)
    poses = msp.processVideos()
    assert [p.shape for p in poses] == [(2, 14, 3)] * 2 and all(np.isfinite(p).all() for p in poses)
    ref = M.find_hands_ref(f, MT_CUBE, FX, FY, 2, 500.)
    mt = MultiTracker(rt, di, pnet, snet, 120, 160, MT_CUBE, [(0, False), (0, True)], fx=FX, fy=FY)
    for t in range(2):
        mt.reset(t, ref['com'][t])
    want = mt.process([f])
    for t in range(2):                               # two different hands, the ones the restatement finds
        assert np.array_equal(poses[t][0], want[t]['pose']), t
    assert not np.array_equal(want[0]['com'], want[1]['com'])
    # one track per device: the poses of the per-track acquire path
    (snet2, _, _), (pnet2, _, _) = _nets(rt, backend, 2)
    g = _two_hands(left_z=580., right_z=503.)
    msp = MultiStreamPipeline(pnet2, dict(config), di, [_ListDevice([f]), _ListDevice([g])], [(0, L), (1, L)], snet2, seed_detect=True)
    poses = msp.processVideos()
    mt = MultiTracker(rt, di, pnet2, snet2, 120, 160, MT_CUBE, [(0, False), (1, False)], fx=FX, fy=FY)
    assert mt.acquire(0, f)['found'] and mt.acquire(1, g)['found']
    want = mt.process([f, g])
    for t in range(2):
        assert poses[t].shape == (1, 14, 3) and np.array_equal(poses[t][0], want[t]['pose']), t


@pytest.mark.parametrize('backend', BACKENDS)
def test_realtime_multi_example_detects_every_track(backend, tmp_path):
    from tests.test_multitrack import ROOT, _two_icvl_sequences
    R.set_default_runtime(get_runtime(backend))
    base, _, _, _, _ = _two_icvl_sequences(tmp_path, 2)
    spec = importlib.util.spec_from_file_location('realtime_multi_driver', os.path.join(ROOT, 'examples', 'realtime_multi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = 'resnet' if backend == 'hip' else 'poseregnet'               # (the 128x128 ResNet is too slow for the SIMT emulator)
    common = ['--dataset', 'icvl', '--data', base, '--net', net, '--cache', str(tmp_path / 'cache')]
    poses, _ = mod.main(common + ['--seed', 'detect-all', '--max-extent', '500'])
    # one hand per sequence: the first track of camera 0 and the track of camera 1 are found, the second hand of camera 0 is not there
    assert [p.shape for p in poses] == [(2, 16, 3), (0, 16, 3), (2, 16, 3)] and all(np.isfinite(p).all() for p in poses)
    ref, _ = mod.main(common + ['--seed', 'detect'])
    assert np.array_equal(poses[2], ref[2])


# ---- working size ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_working_size_480x640():
    rt = get_runtime('hip')
    H, W, fx, fy = 480, 640, 588., 587.
    a = _wall(H, W)
    _put(a, 200, 100, 60, 50, 503.)                  # two hands in different slabs, far apart, and the wall
    _put(a, 220, 480, 60, 50, 660.)
    b = _wall(H, W)
    _put(b, 40, 300, 60, 50, 580.)                   # one hand over two slabs (the farther part is suppressed), a second hand, the wall
    _put(b, 100, 300, 40, 50, 503.)
    _put(b, 350, 40, 60, 50, 880.)
    rng = np.random.RandomState(5)
    b[rng.uniform(size=(H, W)) < 0.02] = 0.          # ragged holes: many small runs
    cubes = [(250., 250., 250.), (300., 300., 300.)]
    _, got = _detect_at(rt, np.stack([a, b]), cubes, 3, 700., fx, fy)
    for i, f in enumerate((a, b)):
        r = M.find_hands_ref(f, cubes[i], fx, fy, 3, 700.)
        mn, mx = D.depth_range(f)
        inr = f[(f != 0) & (f >= mn) & (f <= mx)]
        assert not np.isin(inr.astype(np.float64), D.slab_bounds(mn, mx)).any()
        assert ((r['stats']['count'] >= 400) | (r['stats']['count'] <= 100)).all()
        assert list(r['found']) == [True, True, False]                                       # the wall is 3400 mm wide
        _equal(got, i, r, i)


def _detect_at(rt, frames, cubes, K, ext, fx, fy):
    from util.handdetector import _detector
    B, H, W = frames.shape
    det = _detector(rt, H, W, fx, fy, B, K, ext)
    return det, _k_axis(det, det.run(frames, np.float32(cubes).reshape(B, 3)))
