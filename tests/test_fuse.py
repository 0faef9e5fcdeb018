"""Tracks of one hand fused across calibrated cameras (csrc/fuse.hip: dpp_pose_fuse, ABI v20; hipdp/multitrack.py `groups=`).  The
semantics are this project's own -- the reference has one camera -- so the launch is pinned bit for bit to the NumPy restatement of
tests/fuse_ref.py, checked for plain geometric sense independently of it, and then the tracker on top: the fused results, the
hand-over of a lost track on the device and from the host, process_sequence against a process() loop, the plan's structure, validation,
the pipeline class and the example.  Every test runs on the emulator (CPU tier) and through libdpp_hip.so (-m gpu); the GPU tier adds
one working-size case (T = 8 over C = 4, 480 x 640 beside 240 x 320)."""
import ctypes
import functools
import os

import numpy as np
import pytest

from data.importers import DepthImporter, ICVLImporter, MSRA15Importer, NYUImporter
from hipdp import lib, ops
from hipdp import runtime as R
from hipdp.augmenter import camera_tuple
from tests import fuse_ref as F
from tests.backends import BACKENDS, get_runtime

OK, LOST, IDLE = 0, 1, 2
USED, OUTLIER, DISAGREE, PEER_OK, HANDED = ops.FUSE_USED, ops.FUSE_OUTLIER, ops.FUSE_DISAGREE, ops.FUSE_PEER_OK, ops.FUSE_HANDED
OLD_KEYS = ('pose', 'pose_img', 'com', 'com3D', 'M', 'status')
OUTPUTS = ('com', 'fused_pose', 'fused_com', 'spread', 'n', 'peer_com', 'fstat')


def _rotation(rng):
    """A random rotation: the Q of a seeded QR, its determinant fixed to +1."""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def _importers():
    half = DepthImporter(241.42 / 2, 241.42 / 2, 80., 60.)
    return [ICVLImporter('../data/ICVL/'), MSRA15Importer('../data/MSRA15/'), half, NYUImporter('../data/NYU/')]


# ---- 1: the launch alone against the restatement -----------------------------------------------------------------------------------
def _case(form, src, groups, J, seed=5):
    """Cameras that all look at the world's origin from 500 .. 700 mm through random rotations (t = -R (dx, dy, -z): a few hundred mm),
    one hand per group within 60 mm of the origin, every member seeing it with a few mm of its own error.  form 'table': ICVL, MSRA15
    (flip_y), ICVL of half the intrinsics at half the size, NYU; 'scalar': four ICVL cameras."""
    rng = np.random.RandomState(seed)
    C, T = 4, len(src)
    cams = [camera_tuple(di) for di in _importers()] if form == 'table' else [camera_tuple(ICVLImporter('../data/ICVL/'))] * C
    sizes = [(240, 320), (240, 320), (120, 160), (480, 640)] if form == 'table' else [(240, 320)] * C
    extr = np.zeros((C, 12))
    for c in range(C):
        Rm = _rotation(rng)
        extr[c, :9], extr[c, 9:] = Rm.ravel(), -Rm.dot([rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(500, 700)])
    group_of = np.full(T, -1)
    for g, ms in enumerate(groups):
        group_of[ms] = g
    hands = rng.uniform(-60, 60, (len(groups) + 1, 3))                   # the last one: what the ungrouped tracks look at
    skel = rng.normal(0, 40, (len(groups) + 1, J, 3))
    com3d, pose3d = np.zeros((T, 3), np.float32), np.zeros((T, J, 3), np.float32)
    for t in range(T):
        Rm, tv = extr[src[t], :9].reshape(3, 3), extr[src[t], 9:]
        w = hands[group_of[t]] + rng.normal(0, 3, 3)
        com3d[t] = Rm.T.dot(w - tv)
        pose3d[t] = (w + skel[group_of[t]] + rng.normal(0, 2, (J, 3)) - tv).dot(Rm)
    com = rng.uniform(5, 100, (T, 3)).astype(np.float32)                 # the centres before the launch: any bits, all different
    return dict(cams=cams, sizes=sizes, extr=extr, src=np.int32(src), groups=groups, J=J, com3d=com3d, pose3d=pose3d, com=com,
                status=np.zeros(T, np.int32), form=form)


SRC7, GROUPS7 = [0, 2, 1, 0, 2, 3, 1], [[3], [1, 6], [0, 2, 5]]          # T = 7 over C = 4: groups of 1, 2 and 3, track 4 in none


def _launch(rt, d, max_dev=None, handover=True, groups=None):
    groups = d['groups'] if groups is None else groups
    T, J, G = len(d['src']), d['J'], len(groups)
    rig = ops.FuseRig(rt, [(e[:9].reshape(3, 3), e[9:]) for e in d['extr']], groups, d['src'], 4)
    table = None
    if d['form'] == 'table':
        table = ops.SourceTable(rt, d['cams'], [(abs(c[0]), abs(c[1])) for c in d['cams']], d['sizes'])
    (H, W), cam = d['sizes'][0], d['cams'][0]
    p3, c3, st, sr, co = rt.upload(d['pose3d']), rt.upload(d['com3d']), rt.upload(d['status']), rt.upload(d['src']), rt.upload(d['com'])
    fp, fc, sp = rt.alloc((G, J, 3), zero=False), rt.alloc((G, 3), zero=False), rt.alloc((G, J), zero=False)
    n, pc, fs = rt.alloc((G,), np.int32, zero=False), rt.alloc((T, 3)), rt.alloc((T,), np.int32)
    ops.pose_fuse(rt, p3, c3, st, sr, T, J, rig, table, H, W, cam, max_dev, handover, co, fp, fc, sp, n, pc, fs)(rt.stream)
    rt.synchronize()
    got = dict(com=co.get(), fused_pose=fp.get(), fused_com=fc.get(), spread=sp.get(), n=n.get(), peer_com=pc.get(), fstat=fs.get())
    want = F.fuse(d['pose3d'], d['com3d'], d['status'], d['src'], d['extr'], groups, d['cams'], d['sizes'], max_dev, handover, d['com'])
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert np.array_equal(p3.get(), d['pose3d']) and np.array_equal(c3.get(), d['com3d']) and np.array_equal(st.get(), d['status'])
    return got


def _world(d, t):
    return F.to_world(d['extr'][d['src'][t]], d['com3d'][t])


def _move(d, t, w):
    """Track t's centre (and pose) as its camera would see the world point w."""
    e = d['extr'][d['src'][t]]
    old = d['com3d'][t].copy()
    d['com3d'][t] = F.to_camera(e, w)
    d['pose3d'][t] += d['com3d'][t] - old


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('form', ['table', 'scalar'])
def test_pose_fuse_equals_the_restatement_bit_for_bit(backend, form):
    rt = get_runtime(backend)
    base = _case(form, SRC7, GROUPS7, 5)

    def fresh():
        return dict((k, v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items())
    alone = dict(com=base['com'][4].tobytes())

    def ungrouped_untouched(got):
        assert got['com'][4].tobytes() == alone['com'] and got['fstat'][4] == 0 and not got['peer_com'][4].any()
    # all members OK and consistent: all used, n = the group's size; a group of one has no peer
    got = _launch(rt, base, max_dev=50.)
    assert got['n'].tolist() == [1, 2, 3] and got['com'].tobytes() == base['com'].tobytes()
    assert got['fstat'].tolist() == [USED | PEER_OK, USED | PEER_OK, USED | PEER_OK, USED, 0, USED | PEER_OK, USED | PEER_OK]
    assert not got['peer_com'][3].any() and got['spread'].max() < 20. and np.abs(got['fused_com']).max() < 70.
    ungrouped_untouched(got)
    # one member LOST with peers: handed, its centre is its peers'; one member IDLE: never rewritten
    d = fresh()
    d['status'][2], d['status'][6] = LOST, IDLE
    got = _launch(rt, d, max_dev=50.)
    assert got['n'].tolist() == [1, 1, 2]
    assert got['fstat'][2] == PEER_OK | HANDED and got['com'][2].tobytes() == got['peer_com'][2].tobytes() != d['com'][2].tobytes()
    assert got['fstat'][6] == PEER_OK and got['com'][6].tobytes() == d['com'][6].tobytes()
    assert got['fstat'][1] == USED and got['fstat'][0] == got['fstat'][5] == USED | PEER_OK
    assert np.array_equal(np.delete(got['com'], 2, 0), np.delete(d['com'], 2, 0))
    ungrouped_untouched(got)
    # handover=False: no centre changes anywhere
    got = _launch(rt, d, max_dev=50., handover=False)
    assert got['com'].tobytes() == d['com'].tobytes() and not (got['fstat'] & HANDED).any() and got['fstat'][2] == PEER_OK
    # a whole group not OK: n == 0, zeros, nothing handed
    d = fresh()
    d['status'][[0, 2, 5]] = [LOST, LOST, IDLE]
    got = _launch(rt, d, max_dev=50.)
    assert got['n'].tolist() == [1, 2, 0] and not got['fused_pose'][2].any() and not got['fused_com'][2].any() and not got['spread'][2].any()
    assert got['fstat'][[0, 2, 5]].tolist() == [0, 0, 0] and got['com'].tobytes() == d['com'].tobytes() and not got['peer_com'][[0, 2, 5]].any()
    # n = 3, one centre moved 200 mm, max_dev = 50: an outlier, handed; the other two fuse as a group of two
    d = fresh()
    _move(d, 2, _world(d, 2) + [200., 0., 0.])
    got = _launch(rt, d, max_dev=50.)
    assert got['n'].tolist() == [1, 2, 2] and got['fstat'][2] == OUTLIER | PEER_OK | HANDED
    assert got['fstat'][0] == got['fstat'][5] == USED | PEER_OK and got['com'][2].tobytes() == got['peer_com'][2].tobytes()
    two = _launch(rt, d, max_dev=50., groups=[[3], [1, 6], [0, 5]])
    for k in ('fused_pose', 'fused_com', 'spread', 'n'):
        assert got[k][2].tobytes() == two[k][2].tobytes(), k
    assert got['peer_com'][[0, 5]].tobytes() == two['peer_com'][[0, 5]].tobytes()
    # ... max_dev=None: no OUTLIER / DISAGREE bits, the moved one goes into the mean
    got = _launch(rt, d)
    assert got['n'].tolist() == [1, 2, 3] and not (got['fstat'] & (OUTLIER | DISAGREE | HANDED)).any() and got['com'].tobytes() == d['com'].tobytes()
    assert got['spread'][2].min() > 100.
    # n = 2 moved apart: DISAGREE on both, both contribute
    d = fresh()
    _move(d, 6, _world(d, 6) + [0., 80., 0.])
    got = _launch(rt, d, max_dev=50.)
    assert got['n'].tolist() == [1, 2, 3] and got['fstat'][1] == got['fstat'][6] == USED | DISAGREE | PEER_OK
    assert got['com'].tobytes() == d['com'].tobytes()
    assert not (_launch(rt, d, max_dev=200.)['fstat'] & DISAGREE).any()
    # a peer centre that projects outside the member's frame, and one behind its camera: no PEER_OK, no hand-over
    for p_in_cam1 in ([3000., 0., 500.], [0., 0., -300.], [10., -3000., 600.]):
        d = fresh()
        d['status'][1] = LOST
        _move(d, 6, F.to_world(d['extr'][d['src'][1]], p_in_cam1))
        got = _launch(rt, d)
        assert got['fstat'][1] == 0 and got['com'].tobytes() == d['com'].tobytes() and got['fstat'][6] == USED
        z = got['peer_com'][1][2]
        assert (z <= 0.) == (p_in_cam1[2] < 0.) and np.isfinite(got['peer_com'][1]).all()


@pytest.mark.parametrize('backend', BACKENDS)
def test_pose_fuse_even_median_and_many_groups(backend):
    rt = get_runtime(backend)
    # four contributors: the median is the mean of the two middle values; one and then two of them pushed away
    d = _case('table', [0, 2, 1, 0, 2, 3, 1], [[0, 1, 2, 5]], 5, seed=6)
    got = _launch(rt, d, max_dev=40.)
    assert got['n'].tolist() == [4] and got['fstat'][[0, 1, 2, 5]].tolist() == [USED | PEER_OK] * 4
    _move(d, 1, _world(d, 1) + [0., 0., 150.])
    got = _launch(rt, d, max_dev=40.)
    assert got['n'].tolist() == [3] and got['fstat'][1] == OUTLIER | PEER_OK | HANDED
    _move(d, 5, _world(d, 5) + [0., -150., 0.])
    d['status'][2] = LOST
    _launch(rt, d, max_dev=40.)                                          # three left: the odd median
    # G x J = 13 x 21 = 273 joints, more than one workgroup's threads; J = 21 does not divide a wave
    T = 26
    d = _case('scalar', [t % 4 for t in range(T)], [[2 * g, 2 * g + 1] for g in range(13)], 21, seed=7)
    d['status'][[3, 8, 9, 20]] = [LOST, LOST, IDLE, IDLE]
    got = _launch(rt, d, max_dev=30.)
    assert got['n'].tolist() == [2, 1, 2, 2, 0, 2, 2, 2, 2, 2, 1, 2, 2] and got['fstat'][3] == PEER_OK | HANDED and got['fstat'][8] == 0
    assert np.abs(got['fused_pose'][12]).max() > 1. and got['fused_pose'].shape == (13, 21, 3)


# ---- 2: geometry, independently of the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_pose_fuse_returns_the_world_skeleton(backend):
    """Three cameras (ICVL, MSRA15, NYU) see ONE world skeleton exactly: pose3d[m] = R_m^T (w - t_m) in float64, stored as float32.
    Bound: every coordinate here is below 1024 mm, so storing one as float32 moves it by at most half an ulp of [512, 1024), 2^-15 =
    3.1e-5 mm.  A member's joint is off by at most sqrt(3) * 2^-15 = 5.3e-5 mm in norm, and so are its world joint (a rotation) and the
    mean; the fused coordinate adds its own float32 rounding (2^-15): 8.4e-5.  A member's world joint is at most 2 * 5.3e-5 = 1.1e-4 from
    the mean (spread).  A peer centre in the member's camera frame is off by 5.3e-5 + 2^-15 per coordinate, with z >= 500 mm and
    fx <= 588.03 that is at most 1.0e-4 px, plus the float32 quotient (2^-24 * 588 = 3.5e-5) and the float32 pixel (ulp of [256, 512) / 2
    = 1.5e-5), against the importer's projection of the member's own float32 centre (off by 2^-15 again): 1.8e-4.  float64 rounding is
    nine orders below all of this.  So: 4 ulp of [512, 1024) = 2^-12 = 2.44e-4 for all three."""
    rt = get_runtime(backend)
    bound = 2. ** -12
    rng = np.random.RandomState(21)
    dis = [ICVLImporter('../data/ICVL/'), MSRA15Importer('../data/MSRA15/'), NYUImporter('../data/NYU/')]
    sizes, J = [(240, 320), (240, 320), (480, 640)], 14
    hand = rng.uniform(-40, 40, 3)
    skel = hand + rng.normal(0, 35, (J, 3))
    extr = np.zeros((3, 12))
    pose3d, com3d = np.zeros((3, J, 3), np.float32), np.zeros((3, 3), np.float32)
    for c in range(3):
        Rm = _rotation(rng)
        tv = -Rm.dot([rng.uniform(-20, 20), rng.uniform(-20, 20), rng.uniform(550, 700)])
        extr[c, :9], extr[c, 9:] = Rm.ravel(), tv
        pose3d[c], com3d[c] = (skel - tv).dot(Rm), Rm.T.dot(hand - tv)
    assert np.abs(pose3d).max() < 1024. and np.abs(skel).max() < 1024. and com3d[:, 2].min() > 500.
    rig = ops.FuseRig(rt, [(e[:9].reshape(3, 3), e[9:]) for e in extr], [[0, 1, 2]], [0, 1, 2], 3)
    table = ops.SourceTable(rt, [camera_tuple(di) for di in dis], [(di.fx, di.fy) for di in dis], sizes)
    co = rt.upload(np.zeros((3, 3), np.float32))
    fp, fc, sp, n = rt.alloc((1, J, 3), zero=False), rt.alloc((1, 3), zero=False), rt.alloc((1, J), zero=False), rt.alloc((1,), np.int32)
    pc, fs = rt.alloc((3, 3)), rt.alloc((3,), np.int32)
    ops.pose_fuse(rt, rt.upload(pose3d), rt.upload(com3d), rt.upload(np.zeros(3, np.int32)), rt.upload(np.int32([0, 1, 2])), 3, J, rig, table,
                  None, None, None, 1., True, co, fp, fc, sp, n, pc, fs)(rt.stream)
    rt.synchronize()
    assert n.get().tolist() == [3] and fs.get().tolist() == [USED | PEER_OK] * 3 and not co.get().any()
    assert np.abs(fp.get()[0].astype(np.float64) - skel).max() <= bound
    assert np.abs(fc.get()[0].astype(np.float64) - hand).max() <= bound
    assert 0. <= sp.get().min() and sp.get().max() <= bound
    for c in range(3):
        own = dis[c].joint3DToImg(com3d[c])
        assert 0 <= own[0] < sizes[c][1] and 0 <= own[1] < sizes[c][0]
        assert np.abs(pc.get()[c].astype(np.float64) - own).max() <= bound, c


# ---- 4: validation -------------------------------------------------------------------------------------------------------------------
def test_pose_fuse_entry_point_refuses_bad_arguments_without_a_gpu():
    """Argument validation happens before any launch: callable on the product library without a GPU."""
    import __graft_entry__
    if not os.path.exists(lib.DEFAULT_LIB):
        __graft_entry__.build()
    so = lib.load()
    assert so.dpp_abi_version() == lib.ABI_VERSION >= 20
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    E = 10001

    def call(**kw):
        a = dict(pose3d=p, com3d=p, status=p, src=p, T=2, J=5, extr=p, C=2, members=p, offsets=p, G=1, sources=None, H=8, W=8, fx=1., fy=1.,
                 ux=0., uy=0., flip=0, max_dev=0., flags=1, com=p, fused_pose=p, fused_com=p, spread=p, n=p, peer_com=p, fstat=p)
        a.update(kw)
        return so.dpp_pose_fuse(*(list(a.values()) + [None]))
    for k in ('pose3d', 'com3d', 'status', 'src', 'extr', 'members', 'offsets', 'com', 'fused_pose', 'fused_com', 'spread', 'n', 'peer_com', 'fstat'):
        assert call(**{k: None}) == E, k
    for k in ('T', 'J', 'C', 'G'):
        assert call(**{k: 0}) == E and call(**{k: -1}) == E, k
    assert call(G=3) == E                                                # more groups than tracks
    assert call(max_dev=-1.) == E and call(max_dev=float('nan')) == E and call(max_dev=float('inf')) == E
    assert call(flags=2) == E
    assert call(H=0) == E and call(W=0) == E and call(fx=0.) == E and call(fy=0.) == E


@pytest.mark.parametrize('backend', BACKENDS)
def test_rig_and_groups_are_validated_on_the_host(backend):
    from hipdp.multitrack import MultiTracker
    from tests.test_multitrack import _nets
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di = ICVLImporter('../data/ICVL/')
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 3)
    tracks = [(0, False), (1, False), (1, True)]
    eye = (np.eye(3), np.zeros(3))

    def make(extrinsics=(eye, eye), **kw):
        return MultiTracker(rt, di, pnet, snet, 37, 45, (250., 250., 250.), tracks, extrinsics=None if extrinsics is None else list(extrinsics), **kw)
    assert make(groups=[[0, 1]]).rig.G == 1 and make(groups=[[0, 2], [1]], max_dev=10.).rig.offsets_host.tolist() == [0, 2, 3]
    skew = np.eye(3)
    skew[0, 1] = 1e-3
    for bad in (dict(extrinsics=((skew, np.zeros(3)), eye), groups=[[0, 1]]),                   # not orthonormal
                dict(extrinsics=((np.diag([1., 1., -1.]), np.zeros(3)), eye), groups=[[0, 1]]), # a reflection
                dict(extrinsics=((np.eye(3), [0., np.nan, 0.]), eye), groups=[[0, 1]]),
                dict(extrinsics=(eye,), groups=[[0, 1]]),                                        # one (R, t) for two sources
                dict(groups=[[0, 1], [1]]),                                                      # overlapping groups
                dict(groups=[[1, 2]]),                                                           # two members on one source
                dict(groups=[[0, 3]]), dict(groups=[[-1, 1]]),                                   # an index out of range
                dict(groups=[[0, 1], []]), dict(groups=[]),
                dict(extrinsics=None, groups=[[0, 1]]),                                          # groups without extrinsics
                dict(groups=[[0, 1]], max_dev=0.), dict(groups=[[0, 1]], max_dev=-5.), dict(max_dev=0.)):
        with pytest.raises(ValueError):
            make(**bad)
    with pytest.raises(ValueError):                                      # a group of 17 (on 17 sources, so that only its size is wrong)
        ops.FuseRig(rt, [eye] * 17, [list(range(17))], np.arange(17), 17)
    assert ops.FuseRig(rt, [eye] * 16, [list(range(16))], np.arange(16), 16).G == 1
    with pytest.raises(ValueError):
        ops.pose_fuse(rt, None, None, None, None, 2, 5, None, None, 8, 8, camera_tuple(di), -1., True, None, None, None, None, None, None, None)


# ---- 3 / 6: the tracker -----------------------------------------------------------------------------------------------------------------
SETUPS = [pytest.param('emu', 'small', id='emu'), pytest.param('hip', 'small', marks=pytest.mark.gpu, id='hip'),
          pytest.param('hip', 'large', marks=pytest.mark.gpu, id='hip-480x640+240x320')]


@functools.lru_cache(maxsize=None)
def _rig(size):
    """(importers, sizes, cube, tracks, groups, extrinsics, ticks, starts, drop).  small: T = 3 over C = 3, frames of the kind
    tests.test_multitrack_sources._launch_case builds (37 x 45 ICVL, 48 x 64 MSRA15, 37 x 45 ICVL of half the intrinsics), one group of
    all three, 4 ticks.  large: T = 8 over C = 4 of that module's large set-up (480 x 640 NYU beside 240 x 320 ICVL, two tracks per
    source), two groups of four, 6 ticks.

    HOW A TRACK IS LOST HERE.  An all-zero frame alone loses no track: track_refine's new centre is net_out * cube_z / 2 + com3D, which
    does not read the frame, and LOST means that centre's depth is 0.  So these tests lose a track the way the existing lost-track tests
    do, with the refinement net that always answers (0, 0, -2): every tick moves a centre by one cube towards its camera along the
    camera's z axis.  The tracks of source 1 start at (drop + 1) cubes and reach depth 0 exactly in tick `drop` -- the tick in which
    source 1 also delivers its all-zero frame -- while the others start far away and go on.  The extrinsics put the other sources'
    centres OF TICK `drop` on one world point, which source 1's camera sees at `target`, inside its frame: that is where the hand-over
    puts source 1's tracks.  starts: the centres the tracks start from."""
    rng = np.random.RandomState(31)
    if size == 'small':
        dis = [ICVLImporter('../data/ICVL/'), MSRA15Importer('../data/MSRA15/'), DepthImporter(241.42 / 2, 241.42 / 2, 80., 60.)]
        sizes, cube, tracks, groups, drop, n = [(37, 45), (48, 64), (37, 45)], (250., 250., 250.), [(0, False), (1, False), (2, False)], [[0, 1, 2]], 1, 4
        ticks = []
        for i in range(n):
            fr = []
            for c, (H, W) in enumerate(sizes):
                f = (1400. + rng.normal(0, 3., (H, W))).astype(np.float32)
                f[8:30, 5 + 4 * c:28 + 4 * c] = rng.uniform(450., 650., (22, 23))
                f[rng.uniform(size=f.shape) < 0.05] = 0.
                f[rng.uniform(size=f.shape) < 0.02] = 2500.
                fr.append(f)
            ticks.append(fr)
        far = [np.float32([30., 25., 10000.])] * 3
        target = np.float32([30., 20., 900.])
    else:
        from tests.test_multitrack_sources import _setup
        dis, _, sizes, cube, _, tracks, seqs = _setup('large')
        groups, drop = [[0, 1, 2, 4], [3, 5, 6, 7]], 2
        ticks = [[np.array(f[i]) for f, _ in seqs] for i in (1, 2, 3, 4, 3, 2)]
        far = [np.float32([300., 230., 3000.]), np.float32([150., 110., 3000.])] * 2
        target = np.float32([170., 100., 1500.])
    lose = np.float32([target[0], target[1], (drop + 1) * cube[2]])
    world = np.float64([40., -25., 60.])
    extr, start_of = [], []
    for c, di in enumerate(dis):
        Rm = _rotation(rng)
        if c == 1:
            p = di.jointImgTo3D(target).astype(np.float64)
        else:
            p = di.jointImgTo3D(far[c]).astype(np.float64) - [0., 0., (drop + 1) * cube[2]]
        extr.append((Rm, world - Rm.dot(p)))
        start_of.append(lose if c == 1 else far[c])
    starts = [start_of[c] for c, _ in tracks]
    for fr in ticks:
        for f in fr:
            f.setflags(write=False)
    return dis, sizes, cube, tracks, groups, extr, ticks, starts, drop


def _tracker(rt, backend, size, grouped=True, **kw):
    from hipdp.multitrack import MultiTracker
    from tests.test_multitrack import _nets
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig(size)
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, len(tracks), zero_refine=True)
    if grouped:
        kw = dict(dict(extrinsics=extr, groups=groups), **kw)
    return MultiTracker(rt, dis, pnet, snet, [s[0] for s in sizes], [s[1] for s in sizes], cube, tracks, **kw)


def _dropped(size):
    """The ticks with source 1's frame all zero in tick `drop`."""
    ticks, drop = _rig(size)[6], _rig(size)[8]
    return [[np.zeros_like(f) if (i == drop and c == 1) else f for c, f in enumerate(fr)] for i, fr in enumerate(ticks)]


def _fused_matches_the_restatement(mt, res, fused):
    dis, sizes, cube, tracks, groups, extr = _rig('small')[:6] if mt.T == 3 else _rig('large')[:6]
    want = F.fuse(np.stack([r['pose'] for r in res]), np.stack([r['com3D'] for r in res]), [r['status'] for r in res], mt.src_host,
                  mt.rig.extr_host, groups, mt.cams, mt.sizes, mt.max_dev, mt.handover, np.stack([r['com'] for r in res]))
    for g, f in enumerate(fused):
        assert f['n'] == want['n'][g] and f['pose'].tobytes() == want['fused_pose'][g].tobytes(), g
        assert f['com'].tobytes() == want['fused_com'][g].tobytes() and f['spread'].tobytes() == want['spread'][g].tobytes(), g
    for t, r in enumerate(res):
        assert r['peer_com'].tobytes() == want['peer_com'][t].tobytes(), t
        f = want['fstat'][t]
        assert (r['outlier'], r['disagree'], r['handed']) == (bool(f & OUTLIER), bool(f & DISAGREE), bool(f & HANDED)), t
        assert r['group'] == mt.rig.group_of[t]
    return want


def _same_old_keys(a, b, where, keys=OLD_KEYS + ('crop',)):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (where, k)


@pytest.mark.parametrize('backend,size', SETUPS)
def test_grouped_tracker_fuses_and_hands_over(backend, size):
    """(a) with every track OK the grouped tracker's pre-existing keys have the bits of the ungrouped tracker's, and `fused` is the
    restatement applied to the downloaded per-track results; (b) source 1 delivers an all-zero frame in tick `drop`: its tracks are LOST
    and handed, not marked lost, and OK in the next tick with the bits of a fresh tracker reset to the centres of that tick and run on
    the next tick's frames; no detector was built."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig(size)
    Tn = len(tracks)
    on1 = [t for t, (c, _) in enumerate(tracks) if c == 1]
    mt, plain = _tracker(rt, backend, size), _tracker(rt, backend, size, grouped=False)
    for t in range(Tn):
        mt.reset(t, starts[t])
        plain.reset(t, starts[t])
    frames = _dropped(size)
    for i in range(drop):                                                                                   # (a)
        res, ref = mt.process(frames[i], return_crop=True), plain.process(frames[i], return_crop=True)
        assert [r['status'] for r in res] == [OK] * Tn
        for t in range(Tn):
            _same_old_keys(res[t], ref[t], (i, t))
            assert set(res[t]) == set(ref[t]) | {'group', 'outlier', 'disagree', 'handed', 'peer_com'}
        assert len(mt.fused) == len(groups) and [f['n'] for f in mt.fused] == [len(g) for g in groups] and plain.fused == []
        want = _fused_matches_the_restatement(mt, res, mt.fused)
        assert not any(r['handed'] for r in res)
    res = mt.process(frames[drop], return_crop=True)                                                        # (b)
    assert [r['status'] for r in res] == [LOST if t in on1 else OK for t in range(Tn)]
    _fused_matches_the_restatement(mt, res, mt.fused)
    for t in on1:
        assert res[t]['handed'] and res[t]['com'].tobytes() == res[t]['peer_com'].tobytes() and res[t]['com'][2] > 0.
    assert not mt.lost.any() and [f['n'] for f in mt.fused] == [len(g) - sum(t in on1 for t in g) for g in groups]
    fresh = _tracker(rt, backend, size, grouped=False)
    for t in range(Tn):
        fresh.reset(t, res[t]['com'])
    nxt, ref = mt.process(frames[drop + 1], return_crop=True), fresh.process(frames[drop + 1], return_crop=True)
    assert [r['status'] for r in nxt] == [OK] * Tn and mt.gate_host.tolist() == [1] * Tn
    for t in range(Tn):
        _same_old_keys(nxt[t], ref[t], ('after the hand-over', t))
    assert mt._detectors == {} and [f['n'] for f in mt.fused] == [len(g) for g in groups]


@pytest.mark.parametrize('backend,size', SETUPS)
def test_grouped_process_sequence_equals_a_process_loop(backend, size):
    """(d) the ticks of (b): the hand-over on the device needs no host knowledge, so the sequence is the loop key for key."""
    from tests.test_multitrack_sources import _compare_sequence
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig(size)
    Tn = len(tracks)
    frames = _dropped(size)
    a, b = _tracker(rt, backend, size), _tracker(rt, backend, size)
    for mt in (a, b):
        for t in range(Tn):
            mt.reset(t, starts[t])
    loop, loop_fused = [], []
    for fr in frames:
        loop.append(b.process(fr, return_crop=True))
        loop_fused.append(b.fused)
    seq = a.process_sequence(iter(frames), return_crops=True)
    lost_ticks = sum(c == 1 for c, _ in tracks)
    assert [[r['status'] for r in tick] for tick in loop] == [[LOST if (i == drop and c == 1) else OK for c, _ in tracks] for i in range(len(frames))]
    assert _compare_sequence(seq, loop, a, b) == len(frames) * Tn - lost_ticks
    for i, (ts, tl) in enumerate(zip(seq, loop)):
        for t in range(Tn):
            for k in ('group', 'outlier', 'disagree', 'handed'):
                assert ts[t][k] == tl[t][k], (i, t, k)
            assert ts[t]['peer_com'].tobytes() == tl[t]['peer_com'].tobytes(), (i, t)
        for fa, fb in zip(a.fused_ticks[i], loop_fused[i]):
            assert fa['n'] == fb['n'] and all(fa[k].tobytes() == fb[k].tobytes() for k in ('pose', 'com', 'spread')), i
    assert not a.lost.any() and len(a.fused_ticks) == len(frames)


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_track_lost_without_peers_is_reset_when_they_return(backend):
    """(c) source 1 delivers an all-zero frame while the other sources idle: track 1 is lost and nobody can hand it over, so it is
    gated.  In the next tick its peers are OK: process() resets it from peer_com, and it is OK the tick after, with the bits of a fresh
    tracker reset to that centre."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig('small')
    mt = _tracker(rt, backend, 'small')
    for t in range(3):
        mt.reset(t, starts[t])
    assert [r['status'] for r in mt.process(ticks[0])] == [OK] * 3
    res = mt.process([None, np.zeros_like(ticks[1][1]), None])
    assert [r['status'] for r in res] == [IDLE, LOST, IDLE] and not res[1]['handed'] and mt.lost.tolist() == [False, True, False]
    assert mt.fused[0]['n'] == 0 and not res[1]['peer_com'].any()
    res = mt.process(ticks[2])
    assert [r['status'] for r in res] == [OK, LOST, OK] and mt.gate_host.tolist() == [1, 0, 1] and not res[1]['handed']
    assert mt.fused[0]['n'] == 2 and mt.lost.tolist() == [False] * 3                      # reset from the host: one small upload
    assert mt.com_host[1].tobytes() == res[1]['peer_com'].tobytes() == mt.com.get()[1].tobytes() and res[1]['peer_com'][2] > 0.
    fresh = _tracker(rt, backend, 'small', grouped=False)
    for t in range(3):
        fresh.reset(t, mt.com_host[t])
    nxt, ref = mt.process(ticks[3], return_crop=True), fresh.process(ticks[3], return_crop=True)
    assert [r['status'] for r in nxt] == [OK] * 3 and mt.fused[0]['n'] == 3
    for t in range(3):
        _same_old_keys(nxt[t], ref[t], t)
    assert mt._detectors == {}
    # handover=False reports and touches nothing: the track stays lost
    off = _tracker(rt, backend, 'small', handover=False)
    for t in range(3):
        off.reset(t, starts[t])
    off.process(ticks[0])
    res = off.process(_dropped('small')[1])
    assert res[1]['status'] == LOST and not res[1]['handed'] and off.lost.tolist() == [False, True, False] and res[1]['peer_com'][2] > 0.
    assert off.process(ticks[2])[1]['status'] == LOST and off.lost[1]


@pytest.mark.parametrize('backend', BACKENDS)
def test_grouped_plan_structure(backend, monkeypatch):
    """(e) one launch more than the ungrouped plan whatever T, C and G are, the last one of the main lane; the rig is uploaded once;
    still one download per tick.  (f) groups=None is the tracker of before: result block, launches, keys."""
    from hipdp.multitrack import MultiTracker
    from tests.test_multitrack import _nets
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di = ICVLImporter('../data/ICVL/')
    half = DepthImporter(241.42 / 2, 241.42 / 2, 80., 60.)
    eye = (np.eye(3), np.zeros(3))
    for Tn, C, groups in ((2, 2, [[0, 1]]), (3, 3, [[2, 0, 1]]), (6, 4, [[0, 1, 2, 3], [4, 5]])):
        tracks = [(t % C, False) for t in range(Tn)]
        (snet, _, _), (pnet, _, _) = _nets(rt, backend, Tn)
        dis = di if C == 2 else [di, half] * (C // 2) + [di] * (C % 2)                   # C = 2: the homogeneous path, launch scalars
        Hs, Ws = (37, 45) if C == 2 else ([37, 48] * (C // 2) + [37] * (C % 2), [45, 64] * (C // 2) + [45] * (C % 2))
        plain = MultiTracker(rt, dis, pnet, snet, Hs, Ws, (250., 250., 250.), tracks)
        mt = MultiTracker(rt, dis, pnet, snet, Hs, Ws, (250., 250., 250.), tracks, extrinsics=[eye] * C, groups=groups, max_dev=40.)
        assert mt.hetero == (C != 2)
        lp, lg = plain.plan().launches(), mt.plan().launches()
        assert len(lg) == len(lp) + 1 and [l.name for l in lg[:-1]] == [l.name for l in lp] and [l.fn for l in lg[:-1]] == [l.fn for l in lp]
        last, side = mt.plan().ops[-1]
        assert last is lg[-1] and last.fn is rt.lib.dpp_pose_fuse and not side and last.name == 'pose_fuse'
        assert last.args[10] == len(groups) and (last.args[11] is None) == (C == 2) and last.args[19] == 40. and last.args[20] == ops.FUSE_HANDOVER
        assert len(mt.plan(1).launches()) == len(lg)
        # (f) the tracker of before: the result block's size, the launches, the keys
        J3 = mt.J * 3
        assert plain.rig is None and plain.res.size == 2 * Tn * J3 + 16 * Tn + 8 and 'pose_fuse' not in [l.name for l in lp]
        assert sorted(plain._off) == sorted(['pose', 'pose_img', 'com', 'com3D', 'M', 'status', 'det'])
        assert all(mt._off[k] == plain._off[k] for k in plain._off) and mt._off['fused_pose'] == plain.res.size
        assert mt.res.size == plain.res.size + len(groups) * (J3 + 3 + mt.J + 1) + 4 * Tn
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig('small')
    plain = _tracker(rt, backend, 'small', grouped=False)
    plain.reset(0, starts[0])
    assert [sorted(r) for r in plain.process(ticks[0])] == [sorted(OLD_KEYS)] * 3 and plain.fused == []
    calls = dict(h2d=[], run=0, d2h=[])
    real_in, real_out, real_run = rt.copy_in, rt.download, ops.Plan.run
    monkeypatch.setattr(rt, 'copy_in', lambda buf, arr: (calls['h2d'].append(buf.ptr), real_in(buf, arr))[1], raising=False)
    monkeypatch.setattr(rt, 'download', lambda buf: (calls['d2h'].append(buf.ptr), real_out(buf))[1], raising=False)
    monkeypatch.setattr(ops.Plan, 'run', lambda self, r: (calls.__setitem__('run', calls['run'] + 1), real_run(self, r))[1])
    mt = _tracker(rt, backend, 'small')
    rig = [mt.rig.extr.ptr, mt.rig.members.ptr, mt.rig.offsets.ptr]
    assert [p for p in calls['h2d'] if p in rig] == rig                                  # uploaded once, when the tracker was built
    for t in range(3):
        mt.reset(t, starts[t])
    f = [mt.frames.ptr + 4 * int(o) for o in mt.table.host['frame_off']]
    for i, h2d in ((0, f + [mt.gate.ptr]), (1, f), (2, f)):
        calls.update(h2d=[], run=0, d2h=[])
        mt.process(_dropped('small')[i])
        assert calls['h2d'] == h2d and calls['run'] == 1 and calls['d2h'] == [mt.res.ptr], (i, calls)
    monkeypatch.undo()


# ---- 5: the class API and the example on top ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_multi_stream_pipeline_returns_the_fused_pose(backend, tmp_path):
    """Two FileDevices play ONE sequence, both with the recorded camera and the identity as extrinsics: the two tracks are one track
    twice, so the fused pose is each track's own pose (the mean of two equal float64 values, rounded back) and the spread is 0."""
    from tests.test_multitrack import _nets, _two_icvl_sequences
    from util.cameradevice import FileDevice
    from util.realtimehandposepipeline import MultiStreamPipeline
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    n = 3
    base, di, cube, seqs, _ = _two_icvl_sequences(tmp_path, n)
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 2, J=16)
    eye = (np.eye(3), np.zeros(3))
    config = {'fx': 241.42, 'fy': 241.42, 'cube': cube, 'extrinsics': [eye, eye]}
    L = MultiStreamPipeline.HAND_LEFT
    init = [seqs[0][1][0]] * 2

    def pipeline(**kw):
        return MultiStreamPipeline(pnet, dict(config), di, [FileDevice(seqs[0][2], di), FileDevice(seqs[0][2], di)], [(0, L), (1, L)], snet,
                                   init_com=init, **kw)
    msp = pipeline(groups=[[0, 1]], max_dev=5.)
    poses = msp.processVideos()
    assert [p.shape for p in poses] == [(n, 16, 3)] * 2 and np.array_equal(poses[0], poses[1])
    assert len(msp.fused_poses) == 1 and np.array_equal(msp.fused_poses[0], poses[0])
    assert msp.fused[0]['n'] == 2 and not msp.fused[0]['spread'].any() and msp._tracker.rig.G == 1
    plain = pipeline()
    assert all(np.array_equal(a, b[:1]) for a, b in zip(plain.processVideos(max_frames=1), poses)) and plain.fused_poses == [] and plain.fused == []
    over = pipeline(groups=[[0, 1]], max_dev=5.)
    assert all(np.array_equal(a, b) for a, b in zip(over.processVideos(overlapped=True), poses))
    assert np.array_equal(over.fused_poses[0], msp.fused_poses[0])
    with pytest.raises(ValueError):
        MultiStreamPipeline(pnet, {'fx': 241.42, 'fy': 241.42, 'cube': cube}, di, [FileDevice(seqs[0][2], di)] * 2, [(0, L), (1, L)], snet,
                            init_com=init, groups=[[0, 1]]).processVideos()


@pytest.mark.parametrize('backend', BACKENDS)
def test_realtime_multi_example_fuses_and_brings_a_covered_camera_back(backend, tmp_path):
    """examples/realtime_multi.py --fuse --drop-second: camera 1 (half resolution, upside down) is covered in ticks 1 and 2 of 5.  An
    all-zero frame alone loses no track (see _rig), so the example marks the covered camera's track lost; it is handed camera 0's centre
    in every covered tick and is followed again in tick 3, the first one with frames -- no detector, no tick lost to finding it again."""
    import importlib.util
    from tests.test_multitrack import ROOT, _two_icvl_sequences
    R.set_default_runtime(get_runtime(backend))
    base, _, _, _, _ = _two_icvl_sequences(tmp_path, 5)
    spec = importlib.util.spec_from_file_location('realtime_multi_driver', os.path.join(ROOT, 'examples', 'realtime_multi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = 'resnet' if backend == 'hip' else 'poseregnet'               # (the 128x128 ResNet is too slow for the SIMT emulator)
    common = ['--dataset', 'icvl', '--data', base, '--net', net, '--cache', str(tmp_path / 'cache'), '--fuse']
    out = mod.main(common + ['--max-frames', '2'])
    assert out['status'] == [[OK, OK]] * 2 and out['fused'].shape == (2, 16, 3) and np.isfinite(out['fused']).all()
    assert np.isfinite(out['spread']) and out['spread'] >= 0. and all(np.isfinite(d) for d in out['dist']) and out['back'] is None
    assert max(out['dist']) <= out['spread'] + 1e-3                    # the mean of two lies between them
    out = mod.main(common + ['--drop-second', '1:3'])
    assert out['dropped'] == [1, 2] and out['back'] == 3
    assert out['status'] == [[OK, OK], [OK, LOST], [OK, LOST], [OK, OK], [OK, OK]] and out['fused'].shape == (5, 16, 3)
