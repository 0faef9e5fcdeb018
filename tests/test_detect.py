"""Whole-frame hand detection by connected components (csrc/components.hip, hipdp/detect.py, util.handdetector.find_hands /
label_components, HandTracker.acquire, RealtimeHandposePipeline(seed_detect=True) / calibrateHandsize) against the NumPy restatement
of tests/detect_ref.py: integer results and float32 centres / cubes bit for bit.  Every test runs on the SIMT emulator and, with
-m gpu, on the card; shapes are the smallest that can still break the kernels (tile 32 x 32, wave runs of 64 pixels)."""
import functools

import numpy as np
import pytest

from data.importers import ICVLImporter
from hipdp import ops
from hipdp import runtime as R
from oracle import augment as A
from tests import detect_ref as D
from tests import track_ref as T
from tests.backends import BACKENDS, get_runtime

BG = D.BG
FX = FY = 241.42


# ---- 1 / 2: labels and statistics ------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (1, 5, 7), (1, 64, 64), (1, 33, 130), (3, 40, 72)]
PATTERNS = ['background', 'one_key', 'checkerboard', 'spiral', 'comb', 'two_keys_diagonal', 'noise']


def _spiral(H, W):
    """A one-pixel-wide spiral from the top-left corner inwards, one background pixel between its turns."""
    k = np.full((H, W), BG, np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    k[0, 0] = 2
    while True:
        moved = False
        while True:
            ny, nx = y + dy, x + dx
            if not (0 <= ny < H and 0 <= nx < W) or k[ny, nx] != BG:
                break
            if 0 <= ny + dy < H and 0 <= nx + dx < W and k[ny + dy, nx + dx] != BG:         # the previous turn is two steps ahead
                break
            y, x = ny, nx
            k[y, x] = 2
            moved = True
        if not moved:
            break
        dy, dx = dx, -dy
    return k


def _pattern(name, H, W, seed):
    yy, xx = np.mgrid[0:H, 0:W]
    k = np.full((H, W), BG, np.uint8)
    if name == 'one_key':
        k[:] = 7
    elif name == 'checkerboard':                     # ONE component under 8-connectivity, H * W / 2 under 4
        k[(yy + xx) % 2 == 0] = 3
    elif name == 'spiral':
        k = _spiral(H, W)
    elif name == 'comb':                             # teeth joined only in the last row: the equivalence is found late, across tiles
        k[:, ::2] = 5
        k[H - 1, :] = 5
    elif name == 'two_keys_diagonal':                # equal keys touch only diagonally, between the other key's pixels
        k[:] = ((yy + xx) % 2).astype(np.uint8)
    elif name == 'noise':
        rng = np.random.RandomState(seed)
        k = np.where(rng.uniform(size=(H, W)) < 0.5, rng.randint(0, 3, (H, W)), BG).astype(np.uint8)
    return k


@functools.lru_cache(maxsize=None)
def _keys_and_ref(shape, name):
    B, H, W = shape
    frames = [_pattern(name, H, W, 11 + b) for b in range(B)]
    if B > 1:                                        # three different frames in one call
        frames[1] = np.ascontiguousarray(frames[1][:, ::-1])
        frames[2] = np.ascontiguousarray(frames[2][::-1])
    keys = np.stack(frames)
    labels = np.stack([D.labels_ref(k) for k in keys])
    stats = [D.stats_ref(k, lab) for k, lab in zip(keys, labels)]
    for a in (keys, labels):
        a.setflags(write=False)
    return keys, labels, stats


def test_restatement_agrees_with_scipy_where_it_imports():
    checked = [D.labels_crosscheck(_keys_and_ref((1, 33, 130), name)[0][0], _keys_and_ref((1, 33, 130), name)[1][0]) for name in PATTERNS]
    assert all(checked) or not any(checked)          # scipy imports, or it does not
    lab = D.labels_ref(_pattern('checkerboard', 6, 6, 0))
    assert set(np.unique(lab)) == {-1, 0}
    lab = D.labels_ref(_pattern('two_keys_diagonal', 4, 4, 0))
    assert set(np.unique(lab)) == {0, 1}


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', PATTERNS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_labels_equal_the_restatement(backend, shape, name):
    from util.handdetector import label_components
    rt = get_runtime(backend)
    keys, ref, _ = _keys_and_ref(shape, name)
    got = label_components(keys, runtime=rt)
    assert got.dtype == np.int32 and got.shape == keys.shape
    assert np.array_equal(got, ref)
    assert np.array_equal(label_components(keys, runtime=rt), got)          # scheduling cannot show: the label is canonical


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', PATTERNS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_statistics_equal_the_restatement(backend, shape, name):
    from util.handdetector import label_components
    rt = get_runtime(backend)
    keys, ref, sref = _keys_and_ref(shape, name)
    labels, st = label_components(keys, runtime=rt, return_stats=True)
    assert np.array_equal(labels, ref)
    for b in range(shape[0]):
        m = st['frame'] == b
        for f in ('root', 'key', 'count', 'xmin', 'xmax', 'ymin', 'ymax', 'sum_x', 'sum_y'):
            assert np.array_equal(st[f][m].astype(np.int64), sref[b][f]), (b, f)
    if name in ('one_key', 'spiral', 'comb') and shape[1] > 1:               # a component touching all four image edges
        _, H, W = shape
        i = int(np.argmax(st['count'][st['frame'] == 0]))
        assert (st['xmin'][i], st['xmax'][i], st['ymin'][i], st['ymax'][i]) == (0, W - 1, 0, H - 1)


@pytest.mark.parametrize('backend', BACKENDS)
def test_bad_arguments_are_refused_before_any_launch(backend):
    rt = get_runtime(backend)
    lib = rt.lib
    assert lib.dpp_label_components(None, 1, 4, 4, None, None, None, None) == 10001
    assert lib.dpp_slab_keys(None, None, 1, 4, 4, None, None, None) == 10001
    assert lib.dpp_mask_keys(None, 1, 4, 4, None, None, None, None, None) == 10001
    assert lib.dpp_detect_seed(None, None, None, None, None, 1, 4, 4, None, None, None, None) == 10001
    assert lib.dpp_hand_size(None, None, None, 1, 4, 4, None, None, None, 1., 1., 0., None, None, None) == 10001
    assert lib.dpp_label_workspace_bytes(1, 65536, 65536) == 0 and lib.dpp_label_workspace_bytes(2, 3, 5) == 2 * 3 * 5 * 4
    assert lib.dpp_component_stats_bytes(1, 1, 1) == ops.COMPONENT_STAT.itemsize == 40
    k = rt.alloc((1, 4, 4), np.uint8)
    assert lib.dpp_label_components(k.ptr, 0, 4, 4, k.ptr, k.ptr, None, None) == 10001
    assert lib.dpp_label_components(k.ptr, 1, 1 << 16, 1 << 16, k.ptr, k.ptr, None, None) == 10001
    assert lib.dpp_label_components(k.ptr, 1, 65535 * 32 + 1, 1, k.ptr, k.ptr, None, None) == 10001      # more rows of tiles than a grid has
    assert lib.dpp_label_workspace_bytes(1, 65535 * 32 + 1, 1) == 0 and lib.dpp_label_workspace_bytes(1, 65535 * 32, 1) == 65535 * 32 * 4


# ---- 3: find_hands ---------------------------------------------------------------------------------------------------------
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


def _scene(kind, H, W):
    f = _wall(H, W)
    if kind == 'a':                                  # far wall, hand nearest but for specks of fewer than 200 px
        _put(f, H // 2 - 12, W // 2 + 20, 24, 20, 503.)
        _specks(f, H, W)
    elif kind == 'b':                                # a big object in a farther slab, the hand in a nearer one
        _put(f, H // 4, W // 8, 50, 60, 880.)
        _put(f, H // 2, W // 2 + 10, 24, 20, 503.)
    elif kind == 'c':                                # specks only: NONE
        f[:] = 0.
        f[4::31, 5::29] = 2000.
        _specks(f, H, W)
    elif kind == 'd':
        f[:] = 0.
    elif kind == 'e':                                # the +-100 window clamps at the top-left corner
        _put(f, 3, 5, 24, 20, 503.)
    elif kind == 'f':                                # ... and at the bottom-right
        _put(f, H - 26, W - 23, 24, 20, 503.)
        _specks(f, H, W)
    return f


@functools.lru_cache(maxsize=None)
def _scene_ref(kind, H, W, cube):
    f = _scene(kind, H, W)
    seed, fin, found, key, st = D.find_hand_ref(f, cube, FX, FY)
    f.setflags(write=False)
    return f, seed, fin, found, key, st


def _check_scene_conditions(f, found, key, st):
    """What keeps the three documented deviations out of the comparison."""
    mn, mx = D.depth_range(f)
    inr = f[(f != 0) & (f >= mn) & (f <= mx)]
    assert not np.isin(inr.astype(np.float64), D.slab_bounds(mn, mx)).any()              # no depth on a slab boundary
    if found:
        big = (st['key'] == key) & (st['count'] > D.MIN_AREA)
        assert big.sum() == 1 and st['count'][big][0] >= 400                                # one winner, far from the area threshold
        assert not ((st['key'] < key) & (st['count'] > D.MIN_AREA // 2)).any()              # nearer things are clearly specks


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('kinds', ['abc', 'def'])
@pytest.mark.parametrize('size', [(120, 160), (240, 320)], ids=['120x160', '240x320'])
def test_find_hands_equals_the_restatement(backend, size, kinds):
    from util.handdetector import find_hands, refine_com_iterative
    rt = get_runtime(backend)
    H, W = size
    cube = (250., 250., 250.)
    refs = [_scene_ref(k, H, W, cube) for k in kinds]
    for f, _, _, found, key, st in refs:
        _check_scene_conditions(f, found, key, st)
    frames = np.stack([r[0] for r in refs])
    cubes = np.tile(np.float32(cube), (3, 1))
    coms, sizes, found, seeds = find_hands(frames, cubes, FX, FY, runtime=rt, return_seed=True)
    assert coms.dtype == np.float32 and coms.shape == (3, 3) and found.dtype == bool
    assert list(found) == [r[3] for r in refs] == [k not in 'cd' for k in kinds]
    for i, (f, seed, fin, ok, _, _) in enumerate(refs):
        assert np.array_equal(seeds[i], seed), (kinds[i], seeds[i], seed)
        assert np.array_equal(coms[i], fin), (kinds[i], coms[i], fin)
        if not ok:
            assert not coms[i].any() and not seeds[i].any()                                 # NONE: (0, 0, 0), handdetector.py:632
    assert np.array_equal(sizes, cubes)                                                     # the cube is handed back
    ok = np.flatnonzero(found)
    same = refine_com_iterative(frames[ok], seeds[ok], cubes[ok], FX, FY, 5, runtime=rt)    # it IS the tracker's kernel
    assert np.array_equal(coms[ok], same)
    if kinds == 'abc':                                                                      # the hand's cube, not the specks' or the big object's
        for i in (0, 1):
            assert abs(coms[i][2] - 505.) < 125.


# ---- 4: hand size ----------------------------------------------------------------------------------------------------------
def _size_scene(case, H=96, W=120):
    f = _wall(H, W)
    com = np.float32([60.25, 40.5, 505.])
    if case == 'two':                                # two components in the depth range, the larger more than twice the smaller
        _put(f, 20, 40, 41, 37, 503.)
        _put(f, 70, 10, 15, 20, 520.)
    elif case == 'hole':                             # the box is the outer one
        _put(f, 15, 30, 50, 61, 503.)
        f[30:45, 50:70] = 1400.
    elif case == 'empty':
        pass
    return f, com


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('case', ['two', 'hole', 'empty'])
def test_hand_size_equals_the_restatement(backend, case):
    from hipdp.detect import FrameDetector
    from util.handdetector import HandDetector
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    f, com = _size_scene(case)
    H, W = f.shape
    cube = np.float32([250., 250., 250.])
    ref, rstat = D.handsize_ref(f, com, cube, FX, FY)
    det = FrameDetector(rt, H, W, FX, FY, 1)
    det.frames.set(f[None])
    det.com.set(com[None])
    det.cube.set(cube[None])
    got, status = det.hand_size()
    assert got.dtype == np.float32 and np.array_equal(got[0], ref), (got, ref)
    assert status[0] == rstat
    if case == 'empty':
        assert np.array_equal(got[0], cube) and status[0] & ops.DETECT_NO_SIZE
    else:
        assert not status[0] & ops.DETECT_NO_SIZE and got[0][0] == got[0][1] == got[0][2] and got[0][0] != cube[0]
    if case == 'two':
        st = D.stats_ref(*(lambda k: (k, D.labels_ref(k)))(np.where((f >= 380) & (f <= 630), 0, BG).astype(np.uint8)))
        cnt = np.sort(st['count'])
        assert cnt.size == 2 and cnt[1] >= 2 * cnt[0]
    # the class API: same number, with a tolerance added in float64 before the cast
    hd = HandDetector(f.copy(), FX, FY)
    assert hd.estimateHandsizeComponents(com, tuple(cube)) == tuple(float(c) for c in ref)
    ref5, _ = D.handsize_ref(f, com, cube, FX, FY, tol=5.)
    assert hd.estimateHandsizeComponents(com, tuple(cube), tol=5.) == tuple(float(c) for c in (ref5 if case != 'empty' else cube))


@pytest.mark.parametrize('backend', BACKENDS)
def test_detect_components_class_api(backend):
    from util.handdetector import HandDetector
    R.set_default_runtime(get_runtime(backend))
    cube = (250., 250., 250.)
    f = _scene('a', 120, 160)
    d = f.copy()
    d[d > 1500] = 0.                                 # the constructor's zeroing: the class works on (and takes its range from) self.dpt
    _, fin, found, _, _ = D.find_hand_ref(d, cube, FX, FY)
    assert found
    com, size = HandDetector(f.copy(), FX, FY).detectComponents(size=cube, doHandSize=False)
    assert size == cube and com.dtype == np.float64 and np.array_equal(np.float32(com), fin)
    com, size = HandDetector(f.copy(), FX, FY).detectComponents(size=cube)
    ref, _ = D.handsize_ref(d, fin, cube, FX, FY)
    assert np.array_equal(np.float32(com), fin) and size == tuple(float(c) for c in ref)
    none, size = HandDetector(_scene('c', 120, 160), FX, FY).detectComponents(size=cube)
    assert not np.any(none) and size == cube
    for m in (HandDetector.detectComponents, HandDetector.estimateHandsizeComponents):
        for word in ('pixel count', 'raster-first', 'nearer slab'):
            assert word in m.__doc__


# ---- 5: tracker and pipeline -------------------------------------------------------------------------------------------------
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


def _setup(backend, zero_refine=False, n=5, seed=41, cube=(250., 250., 250.)):
    from tests.test_realtime import _track_nets
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend, zero_refine=zero_refine)
    di, cam = ICVLImporter('../data/ICVL/'), A.Camera.icvl()
    frames, _ = T.drifting_sequence(np.random.RandomState(seed), n, cam, 240, 320, cube)
    return rt, di, snet, pnet, frames


@pytest.mark.parametrize('backend', BACKENDS)
def test_acquire_then_process_equals_reset_then_process(backend):
    from hipdp.tracker import HandTracker
    from util.handdetector import find_hands
    cube = (250., 250., 250.)
    rt, di, snet, pnet, frames = _setup(backend, n=2)
    coms, _, found = find_hands(frames[:1], np.float32([cube]), FX, FY, runtime=rt)
    assert found[0]
    a = HandTracker(rt, di, pnet, snet, 240, 320, cube, fx=FX, fy=FY)
    with pytest.raises(RuntimeError):
        a.process(frames[0])                                                                # never started
    acq = a.acquire(frames[0])
    assert acq['found'] and not a.lost and np.array_equal(acq['com'], coms[0]) and np.array_equal(acq['cube'], np.float32(cube))
    ra = a.process(frames[0], return_crop=True)
    b = HandTracker(rt, di, pnet, snet, 240, 320, cube, fx=FX, fy=FY)
    b.reset(coms[0])
    rb = b.process(frames[0], return_crop=True)
    for k in ('pose', 'pose_img', 'com', 'com3D', 'M', 'crop'):
        assert np.array_equal(ra[k], rb[k]), k
    assert ra['status'] == rb['status'] == 0
    # with the hand size: the same centre, and the cube of the restatement around it; the tracker's own cube stays
    acq = a.acquire(frames[1], do_hand_size=True)
    c1, s1, _ = find_hands(frames[1:2], np.float32([cube]), FX, FY, do_hand_size=True, runtime=rt)
    assert np.array_equal(acq['com'], c1[0]) and np.array_equal(acq['cube'], s1[0])
    assert np.array_equal(s1[0], D.handsize_ref(frames[1], c1[0], cube, FX, FY)[0])
    assert np.array_equal(a.cube.get().reshape(3), np.float32(cube))
    # hand_size() sees the frame of the last process() / acquire() only
    assert np.array_equal(a.hand_size(), s1[0])
    a.process_sequence(list(frames))
    with pytest.raises(RuntimeError):
        a.hand_size()
    # nothing to find: the track is lost again
    acq = a.acquire(np.zeros((240, 320), np.float32))
    assert not acq['found'] and a.lost and not acq['com'].any()
    with pytest.raises(RuntimeError):
        a.process(frames[1])


@pytest.mark.parametrize('backend', BACKENDS)
def test_pipeline_seed_detect(backend):
    from hipdp.tracker import HandTracker
    from util.handdetector import find_hands
    from util.realtimehandposepipeline import RealtimeHandposePipeline
    cube = (250, 250, 250)
    rt, di, snet, pnet, frames = _setup(backend, n=2)
    config = {'fx': FX, 'fy': FY, 'cube': cube}
    rtp = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, seed_detect=True, seed_com=True)
    assert rtp.tracking.value is True and rtp.seed_detect is True
    poses = rtp.processVideo(_ListDevice(frames))
    assert poses.shape == (2, 14, 3) and np.isfinite(poses).all()
    # its first centre is find_hands's (not seed_com's): the first pose is that of a tracker reset to it
    coms, _, found = find_hands(frames[:1], np.float32([cube]), FX, FY, runtime=rt)
    assert found[0]
    tr = HandTracker(rt, di, pnet, snet, 240, 320, cube, fx=FX, fy=FY)
    tr.reset(coms[0])
    assert np.array_equal(tr.process(frames[0])['pose'], poses[0])
    # detect() + estimatePose() called separately seed themselves the same way
    rtp2 = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, seed_detect=True)
    rtp2.initNets()
    crop, M, com3D = rtp2.detect(frames[0].copy())
    assert np.array_equal(rtp2.estimatePose(crop, com3D) * cube[2] / 2. + com3D, poses[0])
    # without seed_detect a seedless pipeline still needs HandDetector.detect
    rtp3 = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet)
    rtp3.initNets()
    with pytest.raises(NotImplementedError):
        rtp3.detect(frames[0].copy())
    with pytest.raises(NotImplementedError):
        rtp3.processVideo(_ListDevice(frames))


@pytest.mark.parametrize('backend', BACKENDS)
def test_pipeline_finds_the_hand_again_after_a_lost_frame(backend):
    """The refinement net of the existing LOST test, which always answers (0, 0, -2): with a 300 mm cube a flat blob at 600 mm is
    acquired at 600, tracked to 300 and lost at exactly 0 in the next frame -- which seed_detect skips, finding the hand again."""
    from util.realtimehandposepipeline import RealtimeHandposePipeline
    cube = (300, 300, 300)
    rt, di, snet, pnet, _ = _setup(backend, zero_refine=True, n=1, cube=(300., 300., 300.))
    f = np.full((240, 320), 1400., np.float32)
    f[100:140, 150:190] = 600.
    frames = [f, f, np.zeros_like(f), f]                                                    # the hand is lost, the view empty, the hand back
    config = {'fx': FX, 'fy': FY, 'cube': cube}
    rtp = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, seed_detect=True)
    poses = rtp.processVideo(_ListDevice(frames))
    assert len(rtp.frame_times) == 4                                                        # every frame was looked at
    assert poses.shape == (2, 14, 3) and np.isfinite(poses).all()                           # frames 0 and 3; 1 was LOST, 2 had no hand
    assert np.array_equal(poses[0], poses[1])
    assert rtp.lastcom[2] == 300.
    # without seed_detect the same sequence stops at the lost frame
    rtp = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=(169.5, 119.5, 600.))
    assert rtp.processVideo(_ListDevice(frames)).shape == (1, 14, 3)


@pytest.mark.parametrize('backend', BACKENDS)
def test_pipeline_skips_frames_without_a_hand(backend):
    """An empty view before the hand enters, and a hand that leaves it: under seed_detect such frames are answered like lost ones and
    skipped, never HandDetector.detect's NotImplementedError; the fused plan and the per-call API agree."""
    from util.realtimehandposepipeline import RealtimeHandposePipeline
    cube = (250, 250, 250)
    rt, di, snet, pnet, frames = _setup(backend, n=2)
    empty = np.zeros((240, 320), np.float32)
    specks = _scene('c', 240, 320)
    seq = [empty, specks, frames[0], frames[1]]
    config = {'fx': FX, 'fy': FY, 'cube': cube}
    rtp = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, seed_detect=True)
    poses = rtp.processVideo(_ListDevice(seq))
    assert len(rtp.frame_times) == 4 and poses.shape == (2, 14, 3) and np.isfinite(poses).all()
    rtp.initNets()
    rtp.lastcom = (0, 0, 0)
    res = rtp.processFrame(empty)
    assert res['status'] == 1 and not res['pose'].any() and np.array_equal(res['M'], np.eye(3)) and np.allclose(rtp.lastcom, 0)
    # the track that follows a hand-less frame is the one a fresh pipeline finds
    fresh = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, seed_detect=True)
    assert np.array_equal(fresh.processVideo(_ListDevice(seq[2:3])), poses[:1])
    # detect() called separately: the zero crop of a lost frame, then the hand
    rtp2 = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, seed_detect=True)
    rtp2.initNets()
    crop, M, com3D = rtp2.detect(empty.copy())
    assert not crop.any() and np.array_equal(M, np.eye(3)) and not com3D.any()
    crop, M, com3D = rtp2.detect(frames[0].copy())
    assert np.array_equal(rtp2.estimatePose(crop, com3D) * cube[2] / 2. + com3D, poses[0])


@pytest.mark.parametrize('backend', BACKENDS)
def test_calibrate_handsize(backend):
    from hipdp.tracker import HandTracker
    from util.realtimehandposepipeline import RealtimeHandposePipeline
    cube = (250, 250, 250)
    rt, di, snet, pnet, frames = _setup(backend, n=5, seed=43)
    rtp = RealtimeHandposePipeline(pnet, {'fx': FX, 'fy': FY, 'cube': cube}, di, comrefNet=snet, seed_detect=True)
    rtp.numinitframes = 5
    assert rtp.state.value == rtp.STATE_IDLE
    got = rtp.calibrateHandsize(_ListDevice(frames))
    # frame 0: the size around the acquired centre; then around the tracked one
    tr = HandTracker(rt, di, pnet, snet, 240, 320, cube, fx=FX, fy=FY)
    acq = tr.acquire(frames[0], do_hand_size=True)
    assert acq['found']
    sizes = [acq['cube']]
    for f in frames[1:]:
        r = tr.process(f)
        assert r['status'] == 0
        sizes.append(D.handsize_ref(f, r['com'], cube, FX, FY)[0])
    want = tuple(int(c) for c in np.median(np.asarray(sizes, np.float64), axis=0).astype('int'))
    assert got == want == rtp.sync['config']['cube'] and want != cube
    assert rtp.state.value == rtp.STATE_RUN and rtp.handsizes == []
    with pytest.raises(NotImplementedError):
        rtp.processKey(ord('i'))                                                            # the cv2 calibration stays not built


@pytest.mark.parametrize('backend', BACKENDS)
def test_realtime_detect_example(backend, tmp_path):
    """examples/realtime_detect.py: no annotation seeds the track, the hand is found on the device; --calibrate measures it first."""
    import importlib.util
    import os
    from tests.test_realtime import ROOT, _write_icvl_sequence
    R.set_default_runtime(get_runtime(backend))
    cam, cube = A.Camera.icvl(), (250., 250., 250.)
    frames, coms = T.drifting_sequence(np.random.RandomState(36), 2, cam, 240, 320, cube)
    base = str(tmp_path / 'ICVL')
    _write_icvl_sequence(base, 'test_seq_1', frames, coms, cam)
    spec = importlib.util.spec_from_file_location('realtime_detect_driver', os.path.join(ROOT, 'examples', 'realtime_detect.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = 'resnet' if backend == 'hip' else 'poseregnet'               # (the 128x128 ResNet is too slow for the SIMT emulator)
    poses, size = mod.main(['--dataset', 'icvl', '--data', base, '--net', net, '--calibrate', '1', '--cache', str(tmp_path / 'cache')])
    assert poses.shape == (2, 16, 3) and np.isfinite(poses).all()
    assert len(size) == 3 and size[0] == size[1] == size[2] and size != (250, 250, 250)


# ---- 6: working size -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_working_size_480x640():
    from util.handdetector import find_hands, label_components
    rt = get_runtime('hip')
    cube = (250., 250., 250.)
    frames = np.stack([_scene('b', 480, 640), _scene('f', 480, 640)])
    rng = np.random.RandomState(5)
    frames[1][rng.uniform(size=(480, 640)) < 0.02] = 0.                                      # ragged holes: many small runs
    keys = np.stack([D.slab_keys_ref(f) for f in frames])
    labels, st = label_components(keys, runtime=rt, return_stats=True)
    for b in range(2):
        ref = D.labels_ref(keys[b])
        assert np.array_equal(labels[b], ref)
        sref = D.stats_ref(keys[b], ref)
        m = st['frame'] == b
        for f in ('root', 'key', 'count', 'xmin', 'xmax', 'ymin', 'ymax', 'sum_x', 'sum_y'):
            assert np.array_equal(st[f][m].astype(np.int64), sref[f]), (b, f)
    coms, sizes, found, seeds = find_hands(frames, np.tile(np.float32(cube), (2, 1)), 588., 587., do_hand_size=True, runtime=rt, return_seed=True)
    for b in range(2):
        seed, fin, ok, key, s = D.find_hand_ref(frames[b], cube, 588., 587.)
        _check_scene_conditions(frames[b], ok, key, s)
        assert ok and found[b] and np.array_equal(seeds[b], seed) and np.array_equal(coms[b], fin)
        assert np.array_equal(sizes[b], D.handsize_ref(frames[b], fin, cube, 588., 587.)[0])
