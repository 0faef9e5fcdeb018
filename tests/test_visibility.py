"""Joint visibility from the frame and the fusion weighted by it (csrc/visibility.hip: dpp_joint_visibility; csrc/fuse.hip:
dpp_pose_fuse_w; ABI v23; `visibility=` of hipdp/tracker.py and hipdp/multitrack.py).  The semantics are this project's own, so the
launches are pinned bit for bit to the NumPy restatement of tests/visibility_ref.py, the classifier is checked on a scene whose answer
is plain independently of it, and then the trackers on top: the new keys against the restatement fed with the downloaded results and
frames, the old keys against a tracker without the option, the plan's structure, lost / handed tracks, process_sequence against a
process() loop, a calibrating tracker, validation, the pipeline classes and the example.  Every test runs on the emulator (CPU tier)
and through libdpp_hip.so (-m gpu); the GPU tier adds one working-size case (T = 8 over C = 4, 480 x 640 beside 240 x 320, two groups of
four)."""
import ctypes
import os

import numpy as np
import pytest

from data.importers import DepthImporter, ICVLImporter, MSRA15Importer
from hipdp import lib, ops
from hipdp import runtime as R
from hipdp.augmenter import camera_tuple
from tests import fuse_ref as F
from tests import visibility_ref as V
from tests.backends import BACKENDS, get_runtime

OK, LOST, IDLE = 0, 1, 2
VISIBLE, OCCLUDED, UNSUPPORTED, OFFFRAME = ops.VIS_VISIBLE, ops.VIS_OCCLUDED, ops.VIS_UNSUPPORTED, ops.VIS_OFFFRAME
nan, inf = np.nan, np.inf
f32 = np.float32


def test_the_constants_are_the_headers():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dpp_hip.h')).read()
    for name, v in (('VISIBLE', VISIBLE), ('OCCLUDED', OCCLUDED), ('UNSUPPORTED', UNSUPPORTED), ('OFFFRAME', OFFFRAME)):
        assert '#define DPP_VIS_%s %d\n' % (name, v) in hdr and getattr(V, name) == v
    assert '#define DPP_VIS_MAX_RADIUS %d\n' % ops.VIS_MAX_RADIUS in hdr
    assert lib.ABI_VERSION >= 23 and '#define DPP_ABI_VERSION %d\n' % lib.ABI_VERSION in hdr


# ---- 1: the launch alone against the restatement -----------------------------------------------------------------------------------
MARGIN = 12.5                                                            # with frames and depths on a 0.25 mm grid d - z is exact


def _frames(rng, sizes):
    """Per source: a far wall, a hand-sized patch, something nearer over a part of it, 12 % holes -- all on a 0.25 mm grid."""
    out = []
    for H, W in sizes:
        f = 1400. + rng.normal(0., 6., (H, W))
        hand = f[H // 4:3 * H // 4, W // 4:3 * W // 4]
        hand[:] = 500. + rng.normal(0., 6., hand.shape)
        f[H // 4:H // 2, W // 2:3 * W // 4] = 300.
        f[rng.uniform(size=(H, W)) < 0.12] = 0.
        out.append((np.round(f * 4.) / 4.).astype(f32))
    return out


def _special(frame, rng):
    """The joints the restatement must be right about, for one frame: (u, v, z) float32 triples."""
    H, W = frame.shape
    up, down = lambda x: np.nextafter(f32(x), f32(inf)), lambda x: np.nextafter(f32(x), f32(-inf))

    def at(x, y, dz=0.):                                                 # a joint on pixel (x, y) at that pixel's depth (500 in a hole) + dz
        d = frame[y, x] if frame[y, x] != 0. else 500.
        return (x, y, d + dz)
    cx, cy = W // 2, H // 2
    s = [at(0, 0), at(W - 1, 0), at(0, H - 1), at(W - 1, H - 1), at(cx, 0), at(0, cy), at(W - 1, cy), at(cx, H - 1)]      # clipped windows
    s += [at(1, 0), at(0, 1), at(W - 2, H - 1), at(W - 1, H - 2)]
    s += [(3.5, 2.5, 500.), (-0.5, 4., 1400.), (up(-0.5), 4., 1400.), (down(-0.5), 4., 1400.), (4., -0.5, 1400.), (4., down(-0.5), 1400.)]
    s += [(W - 0.5, 4., 1400.), (down(W - 0.5), 4., 1400.), (4., H - 0.5, 1400.), (4., down(H - 0.5), 1400.), (-0.25, -0.25, 1400.)]
    s += [(cx, cy, 0.), (cx, cy, -500.), (cx, cy, -0.), (cx, cy, down(0.)), (cx, cy, up(0.))]
    for bad in (nan, inf, -inf):
        s += [(bad, cy, 500.), (cx, bad, 500.), (cx, cy, bad)]
    s += [(3e38, cy, 500.), (cx, -3e38, 500.), (2. ** 31, cy, 500.), (cx, 2. ** 40, 500.), (cx, cy, 3e38)]
    ys, xs = np.nonzero(frame)
    for k in rng.choice(len(ys), 6, replace=False):                      # d - z exactly +-margin (ON), and one float32 step beyond
        x, y, d = xs[k], ys[k], frame[ys[k], xs[k]]
        s += [(x, y, d + MARGIN), (x, y, d - MARGIN), (x, y, up(d + MARGIN)), (x, y, down(d - MARGIN))]
    ys, xs = np.nonzero(frame == 0.)
    for k in rng.choice(len(ys), 3, replace=False):                      # a hole under the joint and in its window
        s += [at(xs[k], ys[k]), (min(xs[k] + 1, W - 1), ys[k], 500.)]
    return [tuple(f32(c) for c in j) for j in s]


def _poses(rng, T, J, src, frames):
    """[T][J][3]: the special joints of the track's frame, each track starting at another one so that a small J still covers them over
    the tracks, then seeded joints around and on the frame at the depth under them plus one of a few offsets."""
    pose = np.zeros((T, J, 3), f32)
    for t in range(T):
        fr = frames[src[t]]
        H, W = fr.shape
        sp = _special(fr, rng)
        k0 = (t * 17) % len(sp)
        sp = sp[k0:] + sp[:k0]
        for j in range(J):
            if j < len(sp) and (J > 1 or t == 0):
                pose[t, j] = sp[j]
                continue
            u, v = rng.uniform(-3., W + 3.), rng.uniform(-3., H + 3.)
            x, y = int(np.clip(np.floor(u + .5), 0, W - 1)), int(np.clip(np.floor(v + .5), 0, H - 1))
            d = fr[y, x] if fr[y, x] != 0. else 500.
            pose[t, j] = (u, v, d + rng.choice([0., 0., 5., -5., 30., -30., 200., -200., 1000.]))
    if T == 1 and J == 1:
        pose[0, 0] = (frames[src[0]].shape[1] - 1, 0., frames[src[0]][0, -1] or 500.)      # a corner: n_in = 1, 4, 16
    return pose


def _launch(rt, form, pose, status, src, frames, spec):
    """One launch into NaN / -7 filled outputs with a pad row behind; returns what the device wrote (all T + 1 rows)."""
    T, J = pose.shape[:2]
    sizes = [f.shape for f in frames]
    if form == 'table':
        half = DepthImporter(241.42 / 2, 241.42 / 2, 80., 60.)
        cams = [camera_tuple(di) for di in (ICVLImporter('../data/ICVL/'), MSRA15Importer('../data/MSRA15/'), half)]
        assert cams[1][4] and not cams[0][4] and len(set(cams)) == 3            # unlike cameras, one of them flip_y
        table = ops.SourceTable(rt, cams, [(abs(c[0]), abs(c[1])) for c in cams], sizes)
        buf = rt.upload(np.full(table.frame_elems, 777., f32))
        for c, f in enumerate(frames):
            buf.view(int(table.host['frame_off'][c]), f.shape).set(f)
        kw = dict(table=table)
    else:
        assert len(set(sizes)) == 1
        buf, kw = rt.upload(np.stack(frames)), dict(H=sizes[0][0], W=sizes[0][1])
    p, st, sr = rt.upload(pose), rt.upload(np.int32(status)), rt.upload(np.int32(src))
    vis, wgt, word = rt.upload(np.full((T + 1, J), nan, f32)), rt.upload(np.full((T + 1, J), nan, f32)), rt.upload(np.full((T + 1, J), -7, np.int32))
    before = buf.get().copy()
    ops.joint_visibility(rt, p, st, sr, T, J, buf, len(frames), ops.visibility_spec(spec), vis, wgt, word, **kw)(rt.stream)
    rt.synchronize()
    assert p.get().tobytes() == pose.tobytes() and np.array_equal(st.get(), np.int32(status)) and buf.get().tobytes() == before.tobytes()
    return dict(vis=vis.get(), weight=wgt.get(), vword=word.get())


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('form', ['table', 'scalar'])
@pytest.mark.parametrize('radius', [0, 1, 3])
@pytest.mark.parametrize('T,J', [(5, 5), (5, 70), (1, 1)])
def test_joint_visibility_equals_the_restatement_bit_for_bit(backend, form, radius, T, J):
    """Every output array against the restatement, pad rows included.  J = 70 goes past one joint per lane of a wave-per-track kernel;
    radius 3 has windows of 49 pixels, clipped to 16 in a corner; the table's sources are ragged (24 x 32, 24 x 32, 12 x 16)."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(100 * radius + J)
    sizes = [(24, 32), (24, 32), (12, 16)] if form == 'table' else [(24, 32)] * 3
    frames = _frames(rng, sizes)
    src = [2, 0, 1, 0, 1][:T]
    status = [OK, LOST, OK, IDLE, OK][:T]
    pose = _poses(rng, T, J, src, frames)
    spec = dict(radius=radius, margin=MARGIN, min_support={0: 1, 1: 3, 3: 10}[radius], hidden_weight=0.3)
    got = _launch(rt, form, pose, status, src, frames, spec)
    want = V.visibility(pose, status, src, frames, **spec)
    for k, fill in (('vis', nan), ('weight', nan), ('vword', -7)):
        full = np.full((T + 1, J), fill, want[k].dtype)
        full[:T] = want[k]
        assert got[k].dtype == full.dtype and got[k].tobytes() == full.tobytes(), k
    for t in range(T):
        if status[t] != OK:                                              # written, and as zeros
            assert not want['vis'][t].any() and not want['weight'][t].any() and not want['vword'][t].any()
    live = want['vword'][[t for t in range(T) if status[t] == OK]]
    assert np.isin(live, (VISIBLE, OCCLUDED, UNSUPPORTED, OFFFRAME)).all()
    assert (want['weight'][want['vword'] == VISIBLE] == 1.).all() and (want['weight'][want['vword'] == OFFFRAME] == 0.).all()
    hidden = want['weight'][(want['vword'] == OCCLUDED) | (want['vword'] == UNSUPPORTED)]
    assert (hidden == f32(0.3)).all()
    if (T, J) == (5, 70):
        assert {VISIBLE, OCCLUDED, UNSUPPORTED, OFFFRAME} <= set(live.ravel().tolist())


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('radius', [1, 3])
def test_joint_visibility_on_every_border_pixel(backend, radius):
    """One joint on EVERY border pixel of a 24 x 32 frame (108 of them, the corners included; J goes past one wave), at the depth under
    it: every clipped window there is -- n_in = (r + 1)^2 in a corner up to (r + 1)(2 r + 1) along an edge -- against the restatement."""
    rt = get_runtime(backend)
    frame = _frames(np.random.RandomState(7 + radius), [(24, 32)])[0]
    H, W = frame.shape
    border = [(x, y) for y in range(H) for x in range(W) if x in (0, W - 1) or y in (0, H - 1)]
    assert len(border) == 2 * (H + W) - 4 == 108
    pose = np.float32([[(x, y, frame[y, x] or 500.) for x, y in border]])
    spec = dict(radius=radius, margin=MARGIN, min_support=radius + 1, hidden_weight=0.5)
    got, want = _launch(rt, 'scalar', pose, [OK], [0], [frame], spec), V.visibility(pose, [OK], [0], [frame], **spec)
    for k in ('vis', 'weight', 'vword'):
        assert got[k][:1].tobytes() == want[k].tobytes(), k
    assert OFFFRAME not in want['vword'] and VISIBLE in want['vword']
    # the share of ON pixels is a multiple of 1 / n_in: in the corners n_in is (r + 1)^2
    corners = [border.index(c) for c in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1))]
    assert all(abs(want['vis'][0, j] * (radius + 1) ** 2 - round(want['vis'][0, j] * (radius + 1) ** 2)) < 1e-4 for j in corners)


# ---- 2: what the classifier must say about a plain scene, independently of the restatement ---------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('radius,support', [(0, 1), (1, 5), (2, 25)])
def test_visibility_of_a_plain_scene(backend, radius, support):
    """A wall at 1400 mm, a 12 x 12 hand patch at 500, a 6 x 12 occluder at 300 over its right half, a hole of zeros.  Joints at z = 500
    whose windows lie entirely in one region: on the free half VISIBLE with vis == 1; under the occluder OCCLUDED; over the wall and
    over the hole UNSUPPORTED; off the frame OFFFRAME -- and the weights 1 / hidden_weight / 0 accordingly."""
    rt = get_runtime(backend)
    frame = np.full((40, 48), 1400., f32)
    frame[10:22, 10:22] = 500.
    frame[10:22, 16:22] = 300.
    frame[28:35, 28:35] = 0.
    joints = [(12., 12., 500.), (12.4, 18.6, 500.), (19., 13., 500.), (18.6, 18.5, 500.), (40., 5., 500.), (5., 30., 500.), (31., 31., 500.),
              (-5., 12., 500.), (12., 40., 500.), (60., 12., 500.), (12., 12., 0.)]
    expect = [VISIBLE, VISIBLE, OCCLUDED, OCCLUDED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, OFFFRAME, OFFFRAME, OFFFRAME, OFFFRAME]
    pose = np.float32(joints)[None]
    spec = dict(radius=radius, margin=20., min_support=support, hidden_weight=0.25)
    got = _launch(rt, 'scalar', pose, [OK], [0], [frame], spec)
    assert got['vword'][0].tolist() == expect
    assert got['vis'][0].tolist() == [1., 1.] + [0.] * 9
    assert got['weight'][0].tolist() == [1., 1.] + [0.25] * 5 + [0.] * 4
    # a joint on the edge between the free and the covered half sees both: the class follows min_support
    edge = _launch(rt, 'scalar', np.float32([[(15.5, 15., 500.)]]), [OK], [0], [frame], dict(spec, radius=1, min_support=4))
    assert edge['vword'][0, 0] == OCCLUDED and edge['vis'][0, 0] == f32(3. / 9.)         # px = 16: columns 15 (free), 16, 17 (covered)
    edge = _launch(rt, 'scalar', np.float32([[(15.5, 15., 500.)]]), [OK], [0], [frame], dict(spec, radius=1, min_support=3))
    assert edge['vword'][0, 0] == VISIBLE and edge['weight'][0, 0] == 1.


# ---- 3: dpp_pose_fuse_w against the extended restatement ---------------------------------------------------------------------------------
from tests.test_fuse import OLD_KEYS, SETUPS, _case, _dropped, _move, _rig, _tracker, _world  # noqa: E402  (the fusion tests' rigs, not edited)

FUSE_OUT = ('com', 'fused_pose', 'fused_com', 'spread', 'n', 'peer_com', 'fstat')
SRC8, GROUPS8 = [0, 1, 2, 3, 0, 1, 3, 2], [[0, 1, 2, 3], [4, 5], [6]]    # T = 8 over C = 4: groups of 4, 2 and 1, track 7 in none


def _fuse(rt, d, weight, max_dev=None, handover=True):
    """dpp_pose_fuse (weight None) or dpp_pose_fuse_w into NaN-filled group outputs; fused_weight has a pad row behind."""
    groups = d['groups']
    T, J, G = len(d['src']), d['J'], len(groups)
    rig = ops.FuseRig(rt, [(e[:9].reshape(3, 3), e[9:]) for e in d['extr']], groups, d['src'], 4)
    table = None
    if d['form'] == 'table':
        table = ops.SourceTable(rt, d['cams'], [(abs(c[0]), abs(c[1])) for c in d['cams']], d['sizes'])
    (H, W), cam = d['sizes'][0], d['cams'][0]
    p3, c3, st, sr, co = rt.upload(d['pose3d']), rt.upload(d['com3d']), rt.upload(d['status']), rt.upload(d['src']), rt.upload(d['com'])
    fp, fc, sp = rt.upload(np.full((G, J, 3), nan, f32)), rt.upload(np.full((G, 3), nan, f32)), rt.upload(np.full((G, J), nan, f32))
    n, pc, fs = rt.upload(np.full(G, -7, np.int32)), rt.alloc((T, 3)), rt.alloc((T,), np.int32)
    kw = {}
    if weight is not None:
        wd, fw = rt.upload(np.asarray(weight, f32)), rt.upload(np.full((G + 1, J), nan, f32))
        kw = dict(weight=wd, fused_weight=fw)
    launch = ops.pose_fuse(rt, p3, c3, st, sr, T, J, rig, table, H, W, cam, max_dev, handover, co, fp, fc, sp, n, pc, fs, **kw)
    assert launch.fn is (rt.lib.dpp_pose_fuse if weight is None else rt.lib.dpp_pose_fuse_w)
    launch(rt.stream)
    rt.synchronize()
    got = dict(com=co.get(), fused_pose=fp.get(), fused_com=fc.get(), spread=sp.get(), n=n.get(), peer_com=pc.get(), fstat=fs.get())
    if weight is not None:
        got['fused_weight'] = fw.get()
        assert got['fused_weight'][G:].tobytes() == np.full((1, J), nan, f32).tobytes() and wd.get().tobytes() == np.asarray(weight, f32).tobytes()
        got['fused_weight'] = got['fused_weight'][:G]
    assert np.array_equal(p3.get(), d['pose3d']) and np.array_equal(c3.get(), d['com3d']) and np.array_equal(st.get(), d['status'])
    return got


def _weights(rng, T, J):
    """float32 weights in [0, 1] with a third of exact zeros, a few exact ones, and one joint that nobody sees."""
    w = rng.uniform(0., 1., (T, J)).astype(f32)
    w[rng.uniform(size=(T, J)) < 0.33] = 0.
    w[rng.uniform(size=(T, J)) < 0.1] = 1.
    w[:, min(2, J - 1)] = 0.
    return w


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('form', ['table', 'scalar'])
@pytest.mark.parametrize('J', [7, 70])
def test_pose_fuse_w_equals_the_restatement_bit_for_bit(backend, form, J):
    """Groups of 4, 2 and 1 members, max_dev off and on (track 2 moved 300 mm away: an OUTLIER, whose weights must not count; track 1
    LOST), random weights with exact zeros and a joint that no member sees.  Every output of the launch, fused_weight included."""
    rt = get_runtime(backend)
    d = _case(form, SRC8, GROUPS8, J, seed=9 + J)
    w = _weights(np.random.RandomState(J), 8, J)
    for max_dev, handover in ((None, True), (60., True), (60., False)):
        dd = dict(d, pose3d=d['pose3d'].copy(), com3d=d['com3d'].copy(), status=d['status'].copy())
        if max_dev is not None:
            _move(dd, 2, _world(dd, 2) + [300., 0., 0.])
            dd['status'][1] = LOST
        got = _fuse(rt, dd, w, max_dev, handover)
        want = V.fuse_w(dd['pose3d'], dd['com3d'], dd['status'], dd['src'], dd['extr'], GROUPS8, dd['cams'], dd['sizes'], max_dev, handover,
                        dd['com'], w)
        for k in FUSE_OUT + ('fused_weight',):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, max_dev)
        plain = F.fuse(dd['pose3d'], dd['com3d'], dd['status'], dd['src'], dd['extr'], GROUPS8, dd['cams'], dd['sizes'], max_dev, handover, dd['com'])
        for k in ('com', 'fused_com', 'n', 'peer_com', 'fstat'):         # what does not read the weights
            assert want[k].tobytes() == plain[k].tobytes(), k
        j0 = min(2, J - 1)                                               # nobody sees it: the plain mean, weight 0
        assert want['fused_pose'][:, j0].tobytes() == plain['fused_pose'][:, j0].tobytes() and not want['fused_weight'][:, j0].any()
        assert want['spread'][:, j0].tobytes() == plain['spread'][:, j0].tobytes()
        assert not np.array_equal(want['fused_pose'][0], plain['fused_pose'][0])
        if max_dev is not None:
            assert want['fstat'][2] & F.OUTLIER and want['n'].tolist() == [2, 2, 1]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('form', ['table', 'scalar'])
def test_weights_all_one_and_all_zero_give_pose_fuse_bytes(backend, form):
    """1.0 * x is exact and sw == n; with sw == 0 the launch falls back to the unweighted mean: both are dpp_pose_fuse in every output,
    with an outlier, a lost member and a group without inliers among the cases."""
    rt = get_runtime(backend)
    d = _case(form, SRC8, GROUPS8, 21, seed=3)
    _move(d, 2, _world(d, 2) + [300., 0., 0.])
    d['status'][4] = LOST
    d['status'][6] = IDLE                                                # group 2: n == 0
    for max_dev in (None, 60.):
        plain = _fuse(rt, d, None, max_dev)
        assert plain['n'].tolist() == ([4, 1, 0] if max_dev is None else [3, 1, 0])
        for value in (1., 0.):
            got = _fuse(rt, d, np.full((8, 21), value, f32), max_dev)
            for k in FUSE_OUT:
                assert got[k].tobytes() == plain[k].tobytes(), (k, value, max_dev)
            assert (got['fused_weight'][:2] == value).all() and not got['fused_weight'][2].any()


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_joint_that_one_camera_does_not_see_is_the_other_cameras(backend):
    """Two cameras on one hand; camera 1's joint 3 is off by 40 mm and weighs 0: the fused joint is camera 0's world joint to the bit
    (1.0 * W + 0.0 * W' = W, sw = 1) and the spread, taken over the members that took part, is 0.  Unweighted the joint moves by about 20 mm."""
    rt = get_runtime(backend)
    d = _case('table', [0, 1], [[0, 1]], 6, seed=21)
    d['pose3d'][1, 3] += np.float32([40., 0., 0.])
    w = np.ones((2, 6), f32)
    w[1, 3] = 0.
    got, plain = _fuse(rt, d, w), _fuse(rt, d, None)
    mine = F.to_world(d['extr'][0], d['pose3d'][0, 3]).astype(f32)
    assert got['fused_pose'][0, 3].tobytes() == mine.tobytes() and got['spread'][0, 3] == 0. and got['fused_weight'][0].tolist() == [1.] * 6
    # unweighted the joint lands half of 40 mm +- the two cameras' own error (a few mm, _case) away
    assert np.linalg.norm(plain['fused_pose'][0, 3].astype(np.float64) - mine) > 10. and plain['spread'][0, 3] > 10.
    others = [0, 1, 2, 4, 5]
    assert got['fused_pose'][0, others].tobytes() == plain['fused_pose'][0, others].tobytes()
    assert got['spread'][0, others].tobytes() == plain['spread'][0, others].tobytes()


# ---- 4: refusals ----------------------------------------------------------------------------------------------------------------------------
def _product_library():
    import __graft_entry__
    if not os.path.exists(lib.DEFAULT_LIB):
        __graft_entry__.build()
    so = lib.load()
    assert so.dpp_abi_version() == lib.ABI_VERSION >= 23
    return so


def test_joint_visibility_entry_point_refuses_bad_arguments_without_a_gpu():
    """Argument validation happens before any launch: callable on the product library without a GPU."""
    so = _product_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    E = 10001

    def call(**kw):
        a = dict(pose_img=p, status=p, src=p, T=2, J=5, frames=p, C=2, sources=None, H=8, W=8, radius=1, margin=20., min_support=3,
                 hidden_weight=0., vis=p, weight=p, vword=p)
        a.update(kw)
        return so.dpp_joint_visibility(*(list(a.values()) + [None]))
    for k in ('pose_img', 'status', 'src', 'frames', 'vis', 'weight', 'vword'):
        assert call(**{k: None}) == E, k
    for k in ('T', 'J', 'C'):
        assert call(**{k: 0}) == E and call(**{k: -1}) == E, k
    assert call(radius=-1) == E and call(radius=9, min_support=1) == E
    assert call(min_support=0) == E and call(min_support=-1) == E and call(min_support=10) == E and call(radius=0, min_support=2) == E
    assert call(radius=8, min_support=290) == E
    assert all(call(margin=v) == E for v in (0., -1., inf, -inf, nan))
    assert all(call(hidden_weight=v) == E for v in (-1e-9, 1. + 1e-9, inf, -inf, nan))
    assert call(H=0) == E and call(W=0) == E and call(H=-1) == E


def test_pose_fuse_w_entry_point_refuses_bad_arguments_without_a_gpu():
    so = _product_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    E = 10001

    def call(**kw):
        a = dict(pose3d=p, com3d=p, status=p, src=p, T=2, J=5, extr=p, C=2, members=p, offsets=p, G=1, sources=None, H=8, W=8, fx=1., fy=1.,
                 ux=0., uy=0., flip=0, max_dev=0., flags=1, com=p, fused_pose=p, fused_com=p, spread=p, n=p, peer_com=p, fstat=p, weight=p,
                 fused_weight=p)
        a.update(kw)
        return so.dpp_pose_fuse_w(*(list(a.values()) + [None]))
    for k in ('pose3d', 'com3d', 'status', 'src', 'extr', 'members', 'offsets', 'com', 'fused_pose', 'fused_com', 'spread', 'n', 'peer_com', 'fstat',
              'weight', 'fused_weight'):
        assert call(**{k: None}) == E, k
    for k in ('T', 'J', 'C', 'G'):
        assert call(**{k: 0}) == E and call(**{k: -1}) == E, k
    assert call(G=3) == E
    assert call(max_dev=-1.) == E and call(max_dev=nan) == E and call(max_dev=inf) == E
    assert call(flags=2) == E
    assert call(H=0) == E and call(W=0) == E and call(fx=0.) == E and call(fy=0.) == E


@pytest.mark.parametrize('backend', BACKENDS)
def test_visibility_is_validated_on_the_host(backend):
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    good = dict(radius=1, margin=20., min_support=3)
    assert ops.visibility_spec(good) == (1, 20., 3, 0.) and ops.visibility_spec(dict(good, radius=8, min_support=289, hidden_weight=1)) == (8, 20., 289, 1.)
    assert ops.visibility_spec(dict(good, radius=0, min_support=1, hidden_weight=0.5)) == (0, 20., 1, 0.5)
    bad = [dict(good, window=1), dict(margin=20., min_support=3), dict(radius=1, min_support=3), dict(radius=1, margin=20.), 1, [1, 20., 3]]
    bad += [dict(good, radius=v) for v in (-1, 9, 1.5, None, nan)] + [dict(good, margin=v) for v in (0., -1., inf, nan, None)]
    bad += [dict(good, min_support=v) for v in (0, -1, 10, 2.5, None)] + [dict(good, hidden_weight=v) for v in (-0.1, 1.1, inf, nan, None)]
    for b in bad:
        with pytest.raises(ValueError):
            ops.visibility_spec(b)
    for b in (dict(good, window=1), dict(good, margin=0.), dict(radius=1)):
        with pytest.raises(ValueError):
            _tracker(rt, backend, 'small', grouped=False, visibility=b)
    with pytest.raises(ValueError):                                      # weight without fused_weight
        ops.pose_fuse(rt, None, None, None, None, 2, 5, None, None, 8, 8, (1., 1., 0., 0., 0), None, True, None, None, None, None, None, None, None,
                      weight=rt.alloc((2, 5)))


# ---- 5: MultiTracker ---------------------------------------------------------------------------------------------------------------------------
NEW_KEYS = ('vis', 'vis_class')


def _spec(size):
    """The margin for the fusion tests' rigs, from what those rigs hold.  Their tracks on sources other than 1 start `far` away (10000
    mm small, 3000 mm large) over their frame's hand patch (450 .. 650 mm), and the zero-refinement net moves every centre one cube
    (250 / 300 mm) towards the camera per tick, the joints staying within half a cube of it.  margin = far - 2 cubes - 550 is the
    distance from the middle of the patch's depths to the centres of tick 1: in tick 0 the patch is more than `margin` in FRONT of every
    such joint (OCCLUDED), in tick 1 about half of its pixels are, and from tick 2 on the patch is ON the joints (VISIBLE).  (Source 1's
    tracks start one to three cubes from the camera, within `margin` of anything in their frame.)  So both occur among the OK tracks,
    which the test asserts."""
    far, cube = (10000., 250.) if size == 'small' else (3000., 300.)
    return dict(radius=1, margin=far - 2. * cube - 550., min_support=5, hidden_weight=0.25)


def _start(mt, starts):
    for t, c in enumerate(starts):
        mt.reset(t, c)


def _restated(mt, res, fused, where, slot=0):
    """The new keys against the restatement fed with what the tracker DOWNLOADED: the block's pose_img and (device) status, and the
    float32 frames the plan read; the fused outputs against fuse_w fed with the downloaded weight.  Returns the block."""
    blk = mt.block.split(mt.res.get())
    buf = mt.frames if slot == 0 or mt.sensor is not None else mt._inputs2
    frames = [mt._slice(buf, c).get()[0] for c in range(mt.C)]
    want = V.visibility(blk['pose_img'], blk['status'], mt.src_host, frames, *mt.visibility)
    assert blk['vis'].tobytes() == want['vis'].tobytes() and blk['vis_class'].tobytes() == want['vword'].tobytes(), where
    assert blk['vis_weight'].tobytes() == want['weight'].tobytes(), where
    for t, r in enumerate(res):
        assert r['vis'].tobytes() == want['vis'][t].tobytes() and r['vis_class'].tobytes() == want['vword'][t].tobytes(), (where, t)
        assert r['vis'].dtype == f32 and r['vis_class'].dtype == np.int32 and r['vis'].shape == r['vis_class'].shape == (mt.J,)
        if blk['status'][t] != OK:
            assert not r['vis'].any() and not r['vis_class'].any()
    if fused:
        fw = V.fuse_w(blk['pose'], blk['com3D'], blk['status'], mt.src_host, mt.rig.extr_host, mt.rig.groups, mt.cams, mt.sizes, mt.max_dev,
                      mt.handover, blk['com'], blk['vis_weight'])
        for g, f in enumerate(fused):
            assert f['n'] == fw['n'][g] and f['pose'].tobytes() == fw['fused_pose'][g].tobytes(), (where, g)
            assert f['spread'].tobytes() == fw['spread'][g].tobytes() and f['weight'].tobytes() == fw['fused_weight'][g].tobytes(), (where, g)
            assert f['com'].tobytes() == fw['fused_com'][g].tobytes(), (where, g)
    return blk


@pytest.mark.parametrize('backend,size', SETUPS)
def test_visibility_tracker_keeps_every_old_key_and_adds_the_restatement(backend, size):
    """A grouped tracker with and without `visibility` (the working-size GPU case: T = 8 over C = 4, two groups of four): every
    pre-existing per-track key and the crop are bit-identical; of `fused`, n and com are, and pose / spread are wherever all inliers
    weigh 1; the new keys and the weighted fusion are the restatements fed with the downloaded block and frames.  Source 1's tracks lose
    the hand in tick `drop` (rows of zeros) and are handed their peers' centre on the device: OK and classified again in the next tick."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig(size)
    Tn = len(tracks)
    on1 = [t for t, (c, _) in enumerate(tracks) if c == 1]
    mt, plain = _tracker(rt, backend, size, visibility=_spec(size)), _tracker(rt, backend, size)
    _start(mt, starts)
    _start(plain, starts)
    frames = _dropped(size)
    seen, differs = set(), False
    for i in range(drop + 2):
        res, old = mt.process(frames[i], return_crop=True), plain.process(frames[i], return_crop=True)
        for t in range(Tn):
            assert set(res[t]) == set(old[t]) | set(NEW_KEYS), (i, t)
            for k in old[t]:
                assert np.array_equal(res[t][k], old[t][k]), (i, t, k)
        blk = _restated(mt, res, mt.fused, i)
        for g, (fa, fb) in enumerate(zip(mt.fused, plain.fused)):
            assert set(fa) == set(fb) | {'weight'} and fa['n'] == fb['n'] and np.array_equal(fa['com'], fb['com']), (i, g)
            inl = [m for m in groups[g] if blk['fstat'][m] & ops.FUSE_USED]
            same = np.all([blk['vis_weight'][m] == 1. for m in inl], axis=0) if inl else np.ones(mt.J, bool)
            assert fa['pose'][same].tobytes() == fb['pose'][same].tobytes() and fa['spread'][same].tobytes() == fb['spread'][same].tobytes(), (i, g)
            differs = differs or not np.array_equal(fa['pose'], fb['pose'])
        for t in range(Tn):
            if res[t]['status'] == OK:
                seen |= set(res[t]['vis_class'].tolist())
        if i == drop:
            assert all(res[t]['status'] == LOST and res[t]['handed'] and not res[t]['vis_class'].any() for t in on1)
        if i == drop + 1:
            assert all(res[t]['status'] == OK and res[t]['vis_class'].all() for t in on1)
    assert VISIBLE in seen and seen - {VISIBLE}, seen                    # the margin of _spec: both occur among the OK tracks
    assert differs                                                       # and the weights moved a fused joint


@pytest.mark.parametrize('backend', BACKENDS)
def test_visibility_plan_structure(backend):
    """Exactly one more launch whatever T, C and G are: dpp_joint_visibility right behind pose_finish, on the main lane, reading the
    slot's float32 frames; with groups the fusion launch is dpp_pose_fuse_w on the block's weights; pose_smooth stays last.  The new
    fields FOLLOW every existing field, smooth's included.  visibility=None: the block and the launches of before."""
    from hipdp.multitrack import MultiTracker
    from tests.test_multitrack import _nets
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di = ICVLImporter('../data/ICVL/')
    half = DepthImporter(241.42 / 2, 241.42 / 2, 80., 60.)
    eye = (np.eye(3), np.zeros(3))
    smooth = dict(rate=30., mincutoff=1., beta=0.007)
    vis = dict(radius=2, margin=30., min_support=4, hidden_weight=0.5)
    for Tn, C, groups, sm in ((2, 2, None, None), (2, 2, [[0, 1]], None), (3, 3, [[2, 0, 1]], smooth), (6, 4, [[0, 1, 2, 3], [4, 5]], smooth),
                              (2, 2, None, smooth)):
        tracks = [(t % C, False) for t in range(Tn)]
        (snet, _, _), (pnet, _, _) = _nets(rt, backend, Tn)
        dis = di if C == 2 else [di, half] * (C // 2) + [di] * (C % 2)
        Hs, Ws = (37, 45) if C == 2 else ([37, 48] * (C // 2) + [37] * (C % 2), [45, 64] * (C // 2) + [45] * (C % 2))
        kw = dict(smooth=sm)
        if groups is not None:
            kw.update(extrinsics=[eye] * C, groups=groups, max_dev=40.)
        plain = MultiTracker(rt, dis, pnet, snet, Hs, Ws, (250., 250., 250.), tracks, **kw)
        none = MultiTracker(rt, dis, pnet, snet, Hs, Ws, (250., 250., 250.), tracks, visibility=None, **kw)
        mt = MultiTracker(rt, dis, pnet, snet, Hs, Ws, (250., 250., 250.), tracks, visibility=vis, **kw)
        G, J = len(groups or []), mt.J
        for slot in (0, 1):
            lp, lv = plain.plan(slot).launches(), mt.plan(slot).launches()
            names = [l.name for l in lp]
            at = names.index('pose_finish') + 1
            assert len(lv) == len(lp) + 1 and lv[at].name == 'joint_visibility' and lv[at].fn is rt.lib.dpp_joint_visibility
            rest = lv[:at] + lv[at + 1:]
            assert [l.name for l in rest] == [n.replace('pose_fuse', 'pose_fuse_w') for n in names]
            assert all(a.fn is b.fn for a, b in zip(rest, lp) if b.name != 'pose_fuse')
            assert [side for op, side in mt.plan(slot).ops if op is lv[at]] == [False]
            a = lv[at].args
            frames = mt.frames if slot == 0 else mt._inputs2
            assert a[:3] == (mt.pose_img.ptr, mt.status.ptr, mt.src.ptr) and a[3:5] == (Tn, J) and a[5] == frames.ptr and a[6] == C
            assert (a[7] is None) == (C == 2) and a[8:10] == ((37, 45) if C == 2 else (0, 0)) and a[10:14] == (2, 30., 4, 0.5)
            assert a[14:] == tuple(mt.block.view(k).ptr for k in ('vis', 'vis_weight', 'vis_class'))
            if G:
                fuse, old = [l for l in lv if l.name == 'pose_fuse_w'][0], [l for l in lp if l.name == 'pose_fuse'][0]
                assert fuse.fn is rt.lib.dpp_pose_fuse_w and old.fn is rt.lib.dpp_pose_fuse and len(old.args) == 28 and len(fuse.args) == 30
                assert all(fuse.args[k] == old.args[k] for k in (4, 5, 7, 10, 12, 13, 14, 15, 16, 17, 18, 19, 20))
                assert fuse.args[21:24] == (mt.com.ptr, mt.fused_pose.ptr, mt.fused_com.ptr) and fuse.args[24] == mt.spread.ptr
                assert fuse.args[28:] == (mt.block.view('vis_weight').ptr, mt.block.view('fused_weight').ptr)
            if sm is not None:
                assert lv[-1].name == 'pose_smooth' and lv[-1].fn is rt.lib.dpp_pose_smooth and lv[-1].args[14:19] == lp[-1].args[14:19]
            assert [l.name for l in none.plan(slot).launches()] == names and [l.fn for l in none.plan(slot).launches()] == [l.fn for l in lp]
        assert plain.res.size == none.res.size and plain._off == none._off and none.visibility is None
        assert all(mt._off[k] == plain._off[k] for k in plain._off) and mt._off['vis'] == plain.res.size
        assert mt._off['vis_weight'] == mt._off['vis'] + Tn * J and mt._off['vis_class'] == mt._off['vis'] + 2 * Tn * J
        assert mt.res.size == plain.res.size + 3 * Tn * J + G * J and ('fused_weight' in mt._off) == bool(G)
        assert mt.visibility == (2, 30., 4, 0.5)


@pytest.mark.parametrize('backend,size', SETUPS)
def test_visibility_process_sequence_equals_a_process_loop(backend, size):
    """Both slots append the launch on their OWN frames: for every track-tick that is OK or IDLE the new keys have the loop's bits, and
    `fused_ticks` carries the weighted fusion of every tick.  Source 1 loses its tracks in tick `drop`, source 0 idles in tick 3."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig(size)
    Tn = len(tracks)
    frames = [list(fr) for fr in _dropped(size)]
    frames[3][0] = None
    a, b = _tracker(rt, backend, size, visibility=_spec(size)), _tracker(rt, backend, size, visibility=_spec(size))
    _start(a, starts)
    _start(b, starts)
    loop, loop_fused = [], []
    for i, fr in enumerate(frames):
        loop.append(b.process(fr))
        loop_fused.append(b.fused)
        _restated(b, loop[-1], b.fused, i)
    seq = a.process_sequence(iter(frames))
    live = 0
    for i, (ts, tl) in enumerate(zip(seq, loop)):
        for t in range(Tn):
            assert ts[t]['status'] == tl[t]['status'], (i, t)
            if ts[t]['status'] != LOST:
                live += 1
                assert all(ts[t][k].tobytes() == tl[t][k].tobytes() for k in NEW_KEYS), (i, t)
        for fa, fb in zip(a.fused_ticks[i], loop_fused[i]):
            assert all(np.array_equal(fa[k], fb[k]) for k in ('pose', 'spread', 'weight', 'n', 'com')), i
    idle = [t for t in range(Tn) if loop[3][t]['status'] == IDLE]
    assert idle == [t for t, (c, _) in enumerate(tracks) if c == 0] and all(not loop[3][t]['vis_class'].any() for t in idle)
    assert live == len(frames) * Tn - len([t for t, (c, _) in enumerate(tracks) if c == 1])


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_calibrating_tracker_classifies_and_fuses_nothing(backend):
    """While a source's extrinsics are pending the visibility launch still runs, in front of extrinsics_accumulate, and nothing is
    fused: fused_weight reads as zeros.  After finish_calibration() the rebuilt plan ends in dpp_pose_fuse_w."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig('small')
    withheld = [extr[0]] + [None] * (len(extr) - 1)
    mt = _tracker(rt, backend, 'small', extrinsics=withheld, calibrate=dict(anchor=0), visibility=_spec('small'))
    _start(mt, starts)
    names = [l.name for l in mt.plan().launches()]
    assert mt.calibrating and names[-3:] == ['pose_finish', 'joint_visibility', 'extrinsics_accumulate']
    for i in range(drop + 1):
        res = mt.process(ticks[i])
        assert mt.fused == [] and set(NEW_KEYS) <= set(res[0])
        blk = _restated(mt, res, None, i)
        assert not blk['fused_weight'].any()
    report = mt.finish_calibration()
    assert all(r['ok'] for r in report.values()) and not mt.calibrating
    assert [l.name for l in mt.plan().launches()][-3:] == ['pose_finish', 'joint_visibility', 'pose_fuse_w']
    centres = mt.com_host.copy()
    centres[1] = starts[1]
    _start(mt, centres)
    res = mt.process(ticks[0])
    assert [r['status'] for r in res] == [OK] * 3 and [f['n'] for f in mt.fused] == [3]
    _restated(mt, res, mt.fused, 'first fused tick')


# ---- 6: HandTracker, the pipelines and the example ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_hand_tracker_classifies_its_joints(backend):
    """The same launch at T = 1 with the scalar frame size, right behind pose_finish in every plan: process() and process_sequence
    against the restatement fed with the downloaded pose_img and the frame; the old keys those of a tracker without the option."""
    from hipdp.tracker import HandTracker
    from oracle import augment as A
    from tests import track_ref as T
    from tests.test_realtime import _track_nets
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend)
    di, cam, cube, H, W, n = ICVLImporter('../data/ICVL/'), A.Camera.icvl(), (250., 250., 250.), 120, 160, 4
    frames, coms = T.drifting_sequence(np.random.RandomState(32), n, cam, H, W, cube)
    spec = dict(radius=2, margin=40., min_support=6, hidden_weight=0.5)
    tr, plain = HandTracker(rt, di, pnet, snet, H, W, cube, visibility=spec), HandTracker(rt, di, pnet, snet, H, W, cube)
    for slot in (0, 1):
        lv, lp = tr.plan(slot).launches(), plain.plan(slot).launches()
        assert len(lv) == len(lp) + 1 and lv[-1].fn is rt.lib.dpp_joint_visibility and [l.name for l in lv[:-1]] == [l.name for l in lp]
        assert lv[-1].args[3:11] == (1, tr.J, tr.frames[slot].ptr, 1, None, H, W, 2) and lv[-2].name == 'pose_finish'
    assert tr.res.size == plain.res.size + 3 * tr.J
    tr.reset(coms[0])
    plain.reset(coms[0])
    loop = []
    for i, f in enumerate(frames):
        r, old = tr.process(f, return_crop=True), plain.process(f, return_crop=True)
        assert set(r) == set(old) | set(NEW_KEYS) and all(np.array_equal(r[k], old[k]) for k in old), i
        want = V.visibility(r['pose_img'][None], [r['status']], [0], [tr.frames[0].get()[0]], **spec)
        assert r['vis'].tobytes() == want['vis'][0].tobytes() and r['vis_class'].tobytes() == want['vword'][0].tobytes(), i
        assert np.array_equal(tr.frames[0].get()[0], f)
        loop.append(r)
    tr.reset(coms[0])
    seq = tr.process_sequence(frames)
    for i in range(n):
        assert all(np.array_equal(seq[i][k], loop[i][k]) for k in loop[i] if k != 'crop'), i
    both = HandTracker(rt, di, pnet, snet, H, W, cube, visibility=spec, smooth=dict(rate=30., mincutoff=1., beta=0.007))
    assert [l.name for l in both.plan().launches()][-3:] == ['pose_finish', 'joint_visibility', 'pose_smooth']
    assert both.block.offsets['vis'] > both.block.offsets['sstat']
    with pytest.raises(ValueError):
        HandTracker(rt, di, pnet, snet, H, W, cube, visibility=dict(radius=1))


@pytest.mark.parametrize('backend', BACKENDS)
def test_both_pipelines_pass_visibility_through(backend, tmp_path):
    from tests.test_multitrack import _nets, _two_icvl_sequences
    from tests.test_realtime import _track_nets
    from util.cameradevice import FileDevice
    from util.realtimehandposepipeline import MultiStreamPipeline, RealtimeHandposePipeline
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    n = 3
    base, di, cube, seqs, _ = _two_icvl_sequences(tmp_path, n)
    config = {'fx': 241.42, 'fy': 241.42, 'cube': cube}
    spec = dict(radius=1, margin=40., min_support=4, hidden_weight=0.5)
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend, J=16)
    rtp = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=seqs[0][1][0], visibility=spec)
    raw = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=seqs[0][1][0])
    assert np.array_equal(rtp.processVideo(FileDevice(seqs[0][2], di)), raw.processVideo(FileDevice(seqs[0][2], di)))
    assert rtp._tracker.visibility == ops.visibility_spec(spec) and raw._tracker.visibility is None
    assert rtp.vis_classes.shape == (n, 16) and rtp.vis_classes.dtype == np.int32 and rtp.vis_classes.all() and raw.vis_classes is None
    res = rtp.processFrame(seqs[0][0][0])
    want = V.visibility(res['pose_img'][None], [res['status']], [0], [rtp._tracker.frames[0].get()[0]], **spec)
    assert res['vis'].tobytes() == want['vis'][0].tobytes() and res['vis_class'].tobytes() == want['vword'][0].tobytes()
    assert 'vis' not in raw.processFrame(seqs[0][0][0]) and set(rtp._no_hand_result()) == set(res)
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 2, J=16)
    eye = (np.eye(3), np.zeros(3))
    L = MultiStreamPipeline.HAND_LEFT

    def pipeline(**kw):
        return MultiStreamPipeline(pnet, dict(config, extrinsics=[eye, eye]), di, [FileDevice(seqs[0][2], di), FileDevice(seqs[0][2], di)],
                                   [(0, L), (1, L)], snet, init_com=[seqs[0][1][0]] * 2, groups=[[0, 1]], **kw)
    msp, plain = pipeline(visibility=spec), pipeline()
    poses, old = msp.processVideos(), plain.processVideos()
    # one track twice: equal joints with equal weights -- the weighted mean of two equal values is that value, as the plain mean is
    assert all(np.array_equal(a, b) for a, b in zip(poses, old)) and np.array_equal(msp.fused_poses[0], plain.fused_poses[0])
    assert plain.vis_classes is None and 'weight' not in plain.fused[0] and msp.fused[0]['weight'].shape == (16,)
    assert [c.shape for c in msp.vis_classes] == [(n, 16)] * 2 and np.array_equal(msp.vis_classes[0], msp.vis_classes[1])
    assert np.isin(msp.vis_classes[0], (VISIBLE, OCCLUDED, UNSUPPORTED, OFFFRAME)).all()
    mt = msp._tracker
    assert mt.visibility == ops.visibility_spec(spec) and 'pose_fuse_w' in [l.name for l in mt.plan().launches()]
    over = pipeline(visibility=spec)
    over.processVideos(overlapped=True)
    assert all(np.array_equal(a, b) for a, b in zip(over.vis_classes, msp.vis_classes))


@pytest.mark.parametrize('backend', BACKENDS)
def test_the_example_prints_the_class_shares_and_the_occluded_figures(backend, tmp_path, capsys):
    """examples/realtime_multi.py --visibility prints the share of joints per class per track; with --fuse --occlude-second it prints
    how far the fused joints are from the unoccluded run's, weighted and unweighted -- sanity figures: they are printed and finite,
    nothing is asked of their size.  Without the new options the example prints what it printed."""
    import importlib.util
    from tests.test_multitrack import ROOT, _two_icvl_sequences
    R.set_default_runtime(get_runtime(backend))
    base, _, _, _, _ = _two_icvl_sequences(tmp_path, 3)
    spec = importlib.util.spec_from_file_location('realtime_multi_visibility_driver', os.path.join(ROOT, 'examples', 'realtime_multi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = 'resnet' if backend == 'hip' else 'poseregnet'               # (the 128x128 ResNet is too slow for the SIMT emulator)
    common = ['--dataset', 'icvl', '--data', base, '--net', net, '--cache', str(tmp_path / 'cache'), '--max-frames', '2']
    flag = ['--visibility', '1', '40', '4']
    names = ['visible', 'occluded', 'unsupported', 'off-frame']
    capsys.readouterr()
    poses, errs = mod.main(common)
    plain_out = capsys.readouterr().out
    poses_v, errs_v, shares = mod.main(common + flag)
    out = capsys.readouterr().out
    assert all(np.array_equal(a, b) for a, b in zip(poses, poses_v)) and errs == errs_v and 'visibility' not in plain_out
    assert len(shares) == 3 and all(sorted(s) == sorted(names) and abs(sum(s.values()) - 1.) < 1e-6 for s in shares)
    assert out.count(', visibility: visible ') == 3
    fused = mod.main(common + ['--fuse'])
    plain_out = capsys.readouterr().out
    occ = mod.main(common + ['--fuse'] + flag + ['--hidden-weight', '0.25', '--occlude-second', '60:30:100:90:200'])
    out = capsys.readouterr().out
    assert 'visibility' not in fused and 'occluded' not in fused and 'visibility' not in plain_out
    assert len(occ['visibility']) == 2 and sorted(occ['occluded']) == ['unweighted', 'weighted']
    assert all(np.isfinite(v) and v >= 0. for v in occ['occluded'].values())
    assert out.count('camera 1 occluded (sanity figures): fused joints ') == 1 and out.count(', visibility: visible ') == 2
    assert out.count('ticks, both cameras followed') == 1               # the two runs it compares with print nothing
    with pytest.raises(SystemExit):
        mod.main(common + ['--fuse', '--occlude-second', '60:30:100:90:200'])
    # one hand.  examples/test_realtimepipeline.py is a test_*.py file and stays as it is: its option lives in a wrapper without a
    # main of its own, as examples/realtime_smooth.py
    def driver(name):
        spec = importlib.util.spec_from_file_location(name + '_visibility_driver', os.path.join(ROOT, 'examples', name + '.py'))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    one, wrapped = driver('test_realtimepipeline'), driver('realtime_visibility')
    common = common[:-2]
    capsys.readouterr()
    poses, err = one.main(common)
    plain_out = [line for line in capsys.readouterr().out.splitlines() if ' ms per ' not in line]
    again = wrapped.main(common)
    assert len(again) == 2 and np.array_equal(again[0], poses) and again[1] == err
    assert [line for line in capsys.readouterr().out.splitlines() if ' ms per ' not in line] == plain_out
    poses_v, err_v, shares, classes = wrapped.main(common + flag)
    out = [line for line in capsys.readouterr().out.splitlines() if ' ms per ' not in line]
    assert np.array_equal(poses, poses_v) and err_v == err and classes.shape == poses.shape[:2] and sorted(shares) == sorted(names)
    assert abs(sum(shares.values()) - 1.) < 1e-6 and out[:-1] == plain_out and out[-1].startswith('visibility: visible ')
