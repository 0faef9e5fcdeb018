"""Tracked and fused poses smoothed on the device (csrc/smooth.hip: dpp_pose_smooth, ABI v22; `smooth=` of hipdp/tracker.py and
hipdp/multitrack.py).  The semantics are this project's own -- the reference draws what the net returns -- so the launch is pinned bit for
bit to the NumPy restatement of tests/smooth_ref.py, checked for what a One-Euro filter must do independently of it, and then the
trackers on top: the new keys against the restatement fed with the downloaded results, the plan's structure, lost / handed / idle
tracks, process_sequence against a process() loop, a calibrating tracker, validation, the pipeline classes and the examples.  Every test
runs on the emulator (CPU tier) and through libdpp_hip.so (-m gpu); the GPU tier adds one working-size case (T = 8 over C = 4, 480 x 640
beside 240 x 320, two groups of four)."""
import ctypes
import os

import numpy as np
import pytest

from data.importers import DepthImporter, ICVLImporter, MSRA15Importer
from hipdp import lib, ops
from hipdp import runtime as R
from hipdp.augmenter import camera_tuple
from tests import smooth_ref as S
from tests.backends import BACKENDS, get_runtime

OK, LOST, IDLE = 0, 1, 2
S_OK, S_INIT, S_HELD, S_EMPTY, S_DROPPED = ops.SMOOTH_OK, ops.SMOOTH_INIT, ops.SMOOTH_HELD, ops.SMOOTH_EMPTY, ops.SMOOTH_DROPPED
OUTPUTS = ('pose_f', 'pose_img_f', 'sstat', 'fused_pose_f', 'gstat')
PAPER = dict(rate=30., mincutoff=1., beta=0.007, dcutoff=1.)             # what the properties of section 2 were checked with
SMOOTH = dict(rate=30., mincutoff=1., beta=0.007, max_hold=2)            # what the tracker tests filter with
nan = np.nan


def test_the_constants_are_the_headers():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dpp_hip.h')).read()
    for name, v in (('OK', S_OK), ('INIT', S_INIT), ('HELD', S_HELD), ('EMPTY', S_EMPTY), ('DROPPED', S_DROPPED)):
        assert '#define DPP_SMOOTH_%s %d\n' % (name, v) in hdr and getattr(S, name) == v
    assert lib.ABI_VERSION >= 22 and '#define DPP_ABI_VERSION %d\n' % lib.ABI_VERSION in hdr


# ---- 1: the launch alone against the restatement -----------------------------------------------------------------------------------
class _Rows(object):
    """One state of T + G rows on the device and its restatement, both with a pad row behind; every buffer the launch may write starts
    as NaN (`since`: -1, the pad 12345), so a region it leaves alone keeps NaN bits and an EMPTY row must have been written as zeros."""

    def __init__(self, rt, T, J, G, form, par):
        self.rt, self.T, self.J, self.G, self.par = rt, T, J, G, par
        half = DepthImporter(241.42 / 2, 241.42 / 2, 80., 60.)
        if form == 'table':
            cams = [camera_tuple(di) for di in (ICVLImporter('../data/ICVL/'), MSRA15Importer('../data/MSRA15/'), half)]
            self.src_host = np.int32([2, 0, 1, 0, 1][:T])
            self.table = ops.SourceTable(rt, cams, [(abs(c[0]), abs(c[1])) for c in cams], [(240, 320), (240, 320), (120, 160)])
            self.src, self.cams = rt.upload(self.src_host), cams
        else:
            self.cams = [camera_tuple(MSRA15Importer('../data/MSRA15/'))]                     # flip_y
            assert self.cams[0][4]
            self.src_host = self.table = self.src = None
        Rn = T + G
        self.state = ops.SmoothState(rt, Rn + 1, J)
        self.ref = S.State(Rn + 1, J, fill=nan)
        self.ref.since[Rn] = 12345
        self.state.since.set(self.ref.since)
        self.state.xh.set(self.ref.xh)
        self.state.dxh.set(self.ref.dxh)
        f32, i32 = np.float32, np.int32
        self.want = dict(pose_f=np.full((T + 1, J, 3), nan, f32), pose_img_f=np.full((T + 1, J, 3), nan, f32), sstat=np.full(T + 1, -7, i32),
                         fused_pose_f=np.full((G + 1, J, 3), nan, f32), gstat=np.full(G + 1, -7, i32))
        self.out = dict((k, rt.upload(v)) for k, v in self.want.items())

    def tick(self, pose, status, fused=None, n=None):
        rt, T, J, G, o = self.rt, self.T, self.J, self.G, self.out
        p, st = rt.upload(pose), rt.upload(np.int32(status))
        grp = {}
        if G:
            fp, nn = rt.upload(fused), rt.upload(np.int32(n))
            grp = dict(fused_pose=fp, n=nn, G=G, fused_pose_f=o['fused_pose_f'], gstat=o['gstat'])
        ops.pose_smooth(rt, p, st, T, J, ops.smooth_spec(self.par), self.state, o['pose_f'], o['pose_img_f'], o['sstat'], cam=self.cams[0],
                        src=self.src, table=self.table, **grp)(rt.stream)
        rt.synchronize()
        res = S.smooth(pose, status, self.src_host, self.cams, fused if G else None, n, self.ref, **self.par)
        for k in OUTPUTS:
            rows = G if k in ('fused_pose_f', 'gstat') else T
            self.want[k][:rows] = res[k]
            got = o[k].get()
            assert got.dtype == self.want[k].dtype and got.tobytes() == self.want[k].tobytes(), k
        for k in ('since', 'xh', 'dxh'):
            assert getattr(self.state, k).get().tobytes() == getattr(self.ref, k).tobytes(), k
        assert np.array_equal(p.get(), pose) and np.array_equal(st.get(), np.int32(status))   # the inputs: read only
        return res


def _walk(rng, ticks, rows, J):
    """Seeded float32 poses with hundreds of mm of range (z in front of the camera) that jump by up to 50 mm per tick and coordinate."""
    x = rng.uniform(-300., 300., (rows, J, 3)) + [0., 0., 700.]
    out = []
    for _ in range(ticks):
        out.append(x.astype(np.float32))
        x = x + rng.uniform(-50., 50., x.shape)
    return out


# ten ticks: T = 5 tracks, G = 2 groups, max_hold = 2
STATUS = [[OK, OK, IDLE, OK, IDLE, IDLE, OK, OK, OK, OK],                # INIT, OK at 1, HELD, OK at 2, HELD, HELD, OK at 3, OK ...
          [OK, OK, LOST, LOST, LOST, LOST, OK, OK, LOST, OK],            # INIT, OK, HELD, HELD, DROPPED, EMPTY, INIT, OK, HELD, OK at 2
          [LOST, IDLE, LOST, IDLE, LOST, IDLE, LOST, IDLE, LOST, IDLE],  # never valid: EMPTY throughout
          [OK] * 10,
          [LOST, OK, OK, IDLE, OK, OK, LOST, LOST, OK, OK]]              # EMPTY, INIT, OK, HELD, OK at 2, OK, HELD, HELD, OK at 3, OK
N_IN = [[2, 2, 0, 1, 1, 0, 0, 0, 0, 3],                                  # INIT, OK, HELD, OK at 2, OK, HELD, HELD, DROPPED, EMPTY, INIT
        [0, 0, 3, 3, 0, 0, 0, 0, 3, 0]]                                  # EMPTY, EMPTY, INIT, OK, HELD, HELD, DROPPED, EMPTY, INIT, HELD
WORDS = [[S_INIT, S_OK, S_HELD, S_OK, S_HELD, S_HELD, S_OK, S_OK, S_OK, S_OK],
         [S_INIT, S_OK, S_HELD, S_HELD, S_EMPTY | S_DROPPED, S_EMPTY, S_INIT, S_OK, S_HELD, S_OK],
         [S_EMPTY] * 10,
         [S_INIT] + [S_OK] * 9,
         [S_EMPTY, S_INIT, S_OK, S_HELD, S_OK, S_OK, S_HELD, S_HELD, S_OK, S_OK]]
GWORDS = [[S_INIT, S_OK, S_HELD, S_OK, S_OK, S_HELD, S_HELD, S_EMPTY | S_DROPPED, S_EMPTY, S_INIT],
          [S_EMPTY, S_EMPTY, S_INIT, S_OK, S_HELD, S_HELD, S_EMPTY | S_DROPPED, S_EMPTY, S_INIT, S_HELD]]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('form', ['table', 'scalar'])
@pytest.mark.parametrize('T,J,G', [(5, 5, 2), (5, 70, 2), (1, 1, 0)])
def test_pose_smooth_equals_the_restatement_bit_for_bit(backend, form, T, J, G):
    """Ten launches into ONE state, every output array and all three state arrays compared after each.  J = 70 reaches the second joint
    of a lane; T = 1, J = 1, G = 0 has no group pointers."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(11 + J)
    par = dict(PAPER, max_hold=2)
    rows = _Rows(rt, T, J, G, form, par)
    poses, fused = _walk(rng, 10, T, J), _walk(rng, 10, max(G, 1), J)
    moved = 0.
    for i in range(10):
        before = rows.ref.copy()
        res = rows.tick(poses[i], [STATUS[t][i] for t in range(T)], fused[i][:G], [N_IN[g][i] for g in range(G)])
        assert res['sstat'].tolist() == [WORDS[t][i] for t in range(T)], i
        assert res['gstat'].tolist() == [GWORDS[g][i] for g in range(G)], i
        for r, w in enumerate(res['sstat'].tolist() + res['gstat'].tolist()):
            if w == S_OK:                                                # beta * speed moves the cut-off by more than mincutoff
                moved = max(moved, par['beta'] * np.sqrt((rows.ref.dxh[r] ** 2).sum(1)).max())
                assert rows.ref.since[r] == 0 and before.since[r] >= 0
            if w & S_EMPTY:
                out = res['pose_f'][r] if r < T else res['fused_pose_f'][r - T]
                assert not out.any() and (r >= T or not res['pose_img_f'][r].any()) and rows.ref.since[r] == -1
            if w == S_HELD:                                              # the state's values: untouched
                assert rows.ref.xh[r].tobytes() == before.xh[r].tobytes() and rows.ref.since[r] == before.since[r] + 1
            if w == S_INIT:
                assert np.array_equal(res['pose_f'][r] if r < T else res['fused_pose_f'][r - T], (poses[i] if r < T else fused[i])[r if r < T else r - T])
    assert moved > par['mincutoff']
    if T == 5:                                                           # the gaps the script promises: OK at since + 1 = 2 and 3
        assert np.isnan(rows.ref.xh[2]).all() and np.isnan(rows.ref.dxh[2]).all()               # the row that was never valid


# ---- 2: what a One-Euro filter must do, independently of the restatement -------------------------------------------------------------
def _run(rt, xs, valid, par, J=21):
    """T = 1, G = 0 through the scalar camera: the float32 outputs, the words and the float64 state after every tick."""
    cam = camera_tuple(ICVLImporter('../data/ICVL/'))
    st = ops.SmoothState(rt, 1, J)
    pf, pi, ss = rt.alloc((1, J, 3)), rt.alloc((1, J, 3)), rt.alloc((1,), np.int32)
    spec = ops.smooth_spec(par)
    out, words, xh = [], [], []
    for i, (x, v) in enumerate(zip(xs, valid)):
        p, s = rt.upload(np.float32(x).reshape(1, J, 3)), rt.upload(np.int32([OK if v else (LOST, IDLE)[i & 1]]))
        ops.pose_smooth(rt, p, s, 1, J, spec, st, pf, pi, ss, cam=cam)(rt.stream)
        rt.synchronize()
        out.append(pf.get()[0])
        words.append(int(ss.get()[0]))
        xh.append(st.xh.get()[0])
    return np.stack(out), words, np.stack(xh)


def _alpha(fc, Te):
    r = 2. * np.pi * fc * Te
    return r / (r + 1.)


A0 = _alpha(1., 1. / 30.)                                                # the smallest weight a new sample gets with PAPER: 0.1732
U = 2. ** -53                                                            # float64 unit round-off


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_constant_pose_comes_back_exactly(backend):
    """(a) xh = a x + (1 - a) xh with xh = x (1 + e): the two products, 1 - a and the sum each round once, 3 U relative to |x| at most
    (a < 1), and the old error comes back scaled by 1 - a <= 1 - A0.  So |e| <= 3 U / A0 = 17.4 U in every tick: xh stays within 9
    float64 ulp of the float32 sample -- 2^29 times closer than half a float32 ulp, so the float32 output IS the sample."""
    rt = get_runtime(backend)
    x = np.random.RandomState(3).uniform(-400., 900., (21, 3)).astype(np.float32)
    out, words, xh = _run(rt, [x] * 30, [True] * 30, PAPER)
    assert words == [S_INIT] + [S_OK] * 29
    for i in range(30):
        assert np.array_equal(out[i], x), i
        assert (np.abs(xh[i] - x.astype(np.float64)) <= 3. * U / A0 * np.abs(x.astype(np.float64))).all(), i


@pytest.mark.parametrize('backend', BACKENDS)
def test_the_filtered_pose_stays_inside_its_samples(backend):
    """(b) a convex combination cannot leave the hull of what went in.  In float64 it can by the round-off of (a): at most 17.4 U
    relative beyond the largest (smallest) valid sample since INIT.  The samples are float32 and rounding to float32 is monotone, so the
    float32 output lies inside [min, max] of them EXACTLY, in OK and in HELD ticks alike.  A seeded noisy ramp, 300 ticks, one in five
    invalid, max_hold = 3; the seed is one whose runs of invalid ticks are no longer than 3."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(4)
    n, J = 300, 21
    valid = rng.uniform(size=n) >= 0.2
    valid[0] = True
    runs = ''.join('v' if v else '.' for v in valid)
    assert '....' not in runs and '...' in runs
    t = np.arange(n)[:, None, None] / 30.
    xs = (rng.uniform(-200., 200., (1, J, 3)) + rng.uniform(-150., 150., (1, J, 3)) * t + rng.normal(0., 4., (n, J, 3))).astype(np.float32)
    out, words, _ = _run(rt, xs, valid, dict(PAPER, max_hold=3))
    assert words[0] == S_INIT and set(words[1:]) == {S_OK, S_HELD} and words.count(S_HELD) == int((~valid).sum()) > 40
    lo = hi = xs[0]
    for i in range(n):
        if valid[i]:
            lo, hi = np.minimum(lo, xs[i]), np.maximum(hi, xs[i])
        assert (out[i] >= lo).all() and (out[i] <= hi).all(), i
        if not valid[i]:
            assert np.array_equal(out[i], out[i - 1]), i


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_step_is_followed_as_a_first_order_low_pass_follows_it(backend):
    """(c) beta = 0: the cut-off is mincutoff whatever the speed, a = alpha(mincutoff, 1 / rate) in every tick, and a 0 -> 100 mm step
    gives 100 (1 - (1 - a)^n) after n ticks.  float64 round-off is 1e-14 mm; the float32 output rounds by at most half an ulp of
    [64, 128), 3.8e-6 mm.  Bound: one float32 ulp at 100 mm, 2^-17 = 7.6e-6 mm."""
    rt = get_runtime(backend)
    n = 60
    xs = [np.zeros((21, 3), np.float32)] + [np.full((21, 3), 100., np.float32)] * n
    out, words, _ = _run(rt, xs, [True] * (n + 1), dict(PAPER, beta=0.))
    assert not out[0].any()
    want = 100. * (1. - (1. - A0) ** np.arange(1, n + 1))
    worst = np.abs(out[1:].astype(np.float64) - want[:, None, None]).max()
    print('step: worst deviation %.3g mm' % worst)
    assert worst <= 2. ** -17


@pytest.mark.parametrize('backend', BACKENDS)
def test_the_lag_on_a_ramp_and_what_beta_buys(backend):
    """(d) a ramp of v = 200 mm/s: with beta = 0 the lag settles at v Te (1 - a) / a = v / (2 pi mincutoff) = 31.83 mm (the transient
    decays as (1 - a)^n: 1e-10 of it is left after 120 ticks).  Bound: one float32 ulp of the last sample (2^-14 mm in [512, 1024)).
    With beta = 0.007 the cut-off rises with the speed and the lag is strictly smaller."""
    rt = get_runtime(backend)
    n, v = 120, 200.
    xs = [np.full((21, 3), v * i / 30., np.float32) for i in range(n)]
    last = np.float64(xs[-1])
    assert 512. <= last.max() < 1024.
    out0, _, _ = _run(rt, xs, [True] * n, dict(PAPER, beta=0.))
    lag0 = last - out0[-1].astype(np.float64)
    print('ramp: lag %.6f mm with beta = 0, off by %.3g' % (lag0.max(), np.abs(lag0 - v / (2. * np.pi)).max()))
    assert np.abs(lag0 - v / (2. * np.pi * 1.)).max() <= 2. ** -14
    out1, _, _ = _run(rt, xs, [True] * n, PAPER)
    lag1 = last - out1[-1].astype(np.float64)
    print('ramp: lag %.6f mm with beta = 0.007' % lag1.max())
    assert (lag1 > 0.).all() and (lag1 < lag0).all()


@pytest.mark.parametrize('backend', BACKENDS)
def test_every_finite_parameter_that_the_host_accepts_is_launched(backend):
    """'Not finite' means just that: a rate between 1.7e308 and the largest float64, which ops.smooth_spec accepts, is launched.  (Te
    is then denormal and a constant pose still comes back as it went in: x - xh is exactly 0.)"""
    rt = get_runtime(backend)
    x = np.random.RandomState(5).uniform(-400., 900., (21, 3)).astype(np.float32)
    for rate in (1.75e308, float(np.finfo(np.float64).max)):
        out, words, _ = _run(rt, [x] * 3, [True] * 3, dict(PAPER, rate=rate))
        assert words == [S_INIT, S_OK, S_OK] and all(np.array_equal(o, x) for o in out)


# ---- 3: the entry point's refusals ------------------------------------------------------------------------------------------------------
def test_pose_smooth_entry_point_refuses_bad_arguments_without_a_gpu():
    """Argument validation happens before any launch: callable on the product library without a GPU."""
    import __graft_entry__
    if not os.path.exists(lib.DEFAULT_LIB):
        __graft_entry__.build()
    so = lib.load()
    assert so.dpp_abi_version() == lib.ABI_VERSION >= 22
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    E = 10001
    inf, qnan = float('inf'), float('nan')

    def call(**kw):
        a = dict(pose3d=p, status=p, src=p, T=2, J=5, fused_pose=p, n=p, G=1, sources=None, fx=1., fy=1., ux=0., uy=0., flip=0, rate=30.,
                 mincutoff=1., beta=0., dcutoff=1., max_hold=0, since=p, xh=p, dxh=p, pose_f=p, pose_img_f=p, sstat=p, fused_pose_f=p, gstat=p)
        a.update(kw)
        return so.dpp_pose_smooth(*(list(a.values()) + [None]))
    for k in ('pose3d', 'status', 'since', 'xh', 'dxh', 'pose_f', 'pose_img_f', 'sstat', 'fused_pose', 'n', 'fused_pose_f', 'gstat'):
        assert call(**{k: None}) == E, k
    assert call(sources=p, src=None) == E                                # a table needs src
    assert call(T=0) == E and call(T=-1) == E and call(J=0) == E and call(J=-1) == E and call(G=-1) == E and call(max_hold=-1) == E
    for k in ('rate', 'mincutoff', 'dcutoff'):
        assert all(call(**{k: v}) == E for v in (0., -1., inf, -inf, qnan)), k
    assert all(call(beta=v) == E for v in (-1e-9, inf, -inf, qnan))
    assert call(fx=0.) == E and call(fy=0.) == E


# ---- 4: MultiTracker ------------------------------------------------------------------------------------------------------------------------
from tests.test_fuse import OLD_KEYS, SETUPS, _dropped, _rig, _tracker  # noqa: E402  (the rigs of the fusion tests, not edited)

NEW_KEYS = ('pose_f', 'pose_img_f', 'smooth')
HANDED = ops.FUSE_HANDED


def _start(mt, starts):
    for t, c in enumerate(starts):
        mt.reset(t, c)


class _Restated(object):
    """The restatement fed with what a tracker downloads: per tick the poses and statuses (a track's sample is valid iff its reported
    status is OK: a gated track is IDLE on the device and IDLE or LOST on the host) and, where it fuses, the fused poses and n."""

    def __init__(self, mt, par):
        self.mt, self.par = mt, dict(dict(dcutoff=1., max_hold=0), **par)
        G = 0 if mt.rig is None else mt.rig.G
        self.state = S.State(mt.T + G, mt.J)

    def check(self, res, fused, where):
        mt = self.mt
        fp, n = (np.stack([f['pose'] for f in fused]), [f['n'] for f in fused]) if fused else (None, None)
        want = S.smooth(np.stack([r['pose'] for r in res]), [r['status'] for r in res], mt.src_host, mt.cams, fp, n, self.state, **self.par)
        for t, r in enumerate(res):
            assert r['smooth'] == want['sstat'][t], (where, t, r['smooth'], want['sstat'][t])
            assert r['pose_f'].tobytes() == want['pose_f'][t].tobytes() and r['pose_img_f'].tobytes() == want['pose_img_f'][t].tobytes(), (where, t)
        for g, f in enumerate(fused or []):
            assert f['smooth'] == want['gstat'][g] and f['pose_f'].tobytes() == want['fused_pose_f'][g].tobytes(), (where, g)
        return want

    def since(self):
        return self.state.since


@pytest.mark.parametrize('backend,size', SETUPS)
def test_smoothing_tracker_keeps_every_old_key_and_adds_the_restatement(backend, size):
    """A grouped tracker with and without `smooth` over 6 ticks (the working-size GPU case: T = 8 over C = 4, two groups of four, 3
    ticks): every pre-existing key, the crop and `fused` are bit-identical; the new keys are the restatement fed with the downloaded
    pose / status and fused pose / n.  Source 1's tracks lose the hand in tick `drop` and are handed their peers' centre ON THE DEVICE:
    HANDED together with HELD -- the state was not cleared -- and OK, not INIT, in the tick after, filtered with Te = 2 / rate."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig(size)
    Tn = len(tracks)
    on1 = [t for t, (c, _) in enumerate(tracks) if c == 1]
    mt, plain = _tracker(rt, backend, size, smooth=SMOOTH), _tracker(rt, backend, size)
    _start(mt, starts)
    _start(plain, starts)
    ref = _Restated(mt, SMOOTH)
    n = 6 if size == 'small' else 3
    for i in range(n):
        fr = ticks[i % len(ticks)]
        res, old = mt.process(fr, return_crop=True), plain.process(fr, return_crop=True)
        for t in range(Tn):
            assert set(res[t]) == set(old[t]) | set(NEW_KEYS), (i, t)
            for k in old[t]:
                assert np.array_equal(res[t][k], old[t][k]), (i, t, k)
        for fa, fb in zip(mt.fused, plain.fused):
            assert set(fa) == set(fb) | {'pose_f', 'smooth'} and all(np.array_equal(fa[k], fb[k]) for k in fb), i
        want = ref.check(res, mt.fused, i)
        if i == 0:
            assert want['sstat'].tolist() == [S_INIT] * Tn and want['gstat'].tolist() == [S_INIT] * len(groups)
            assert all(np.array_equal(r['pose_f'], r['pose']) and np.array_equal(r['pose_img_f'], r['pose_img']) for r in res)
        if i == drop:
            assert all(res[t]['status'] == LOST and res[t]['handed'] and res[t]['smooth'] == S_HELD for t in on1)
            assert all(np.array_equal(res[t]['pose_f'], before[t]) for t in on1)
        if i == drop + 1:
            assert all(res[t]['status'] == OK and res[t]['smooth'] == S_OK for t in on1)
        before = [r['pose_f'] for r in res]
    rt.synchronize()
    assert np.array_equal(mt.sstate.since.get(), ref.since())
    assert not mt.lost.any() or size == 'small'


@pytest.mark.parametrize('backend', BACKENDS)
def test_smoothing_plan_structure(backend, monkeypatch):
    """Exactly one more launch than the tracker without `smooth`, whatever T, C and G are: the last one, on the main lane,
    dpp_pose_smooth; the new fields FOLLOW every existing field; the state is no part of the block; still one download per tick and no
    upload of the filter's; a reset is one 4-byte upload more.  smooth=None: the block and the launches of before."""
    from hipdp.multitrack import MultiTracker
    from tests.test_multitrack import _nets
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di = ICVLImporter('../data/ICVL/')
    half = DepthImporter(241.42 / 2, 241.42 / 2, 80., 60.)
    eye = (np.eye(3), np.zeros(3))
    for Tn, C, groups in ((2, 2, None), (2, 2, [[0, 1]]), (3, 3, [[2, 0, 1]]), (6, 4, [[0, 1, 2, 3], [4, 5]])):
        tracks = [(t % C, False) for t in range(Tn)]
        (snet, _, _), (pnet, _, _) = _nets(rt, backend, Tn)
        dis = di if C == 2 else [di, half] * (C // 2) + [di] * (C % 2)
        Hs, Ws = (37, 45) if C == 2 else ([37, 48] * (C // 2) + [37] * (C % 2), [45, 64] * (C // 2) + [45] * (C % 2))
        kw = {} if groups is None else dict(extrinsics=[eye] * C, groups=groups, max_dev=40.)
        plain = MultiTracker(rt, dis, pnet, snet, Hs, Ws, (250., 250., 250.), tracks, **kw)
        none = MultiTracker(rt, dis, pnet, snet, Hs, Ws, (250., 250., 250.), tracks, smooth=None, **kw)
        mt = MultiTracker(rt, dis, pnet, snet, Hs, Ws, (250., 250., 250.), tracks, smooth=dict(SMOOTH, dcutoff=2.), **kw)
        G, J3 = len(groups or []), mt.J * 3
        for slot in (0, 1):
            lp, ls = plain.plan(slot).launches(), mt.plan(slot).launches()
            assert len(ls) == len(lp) + 1 and [l.name for l in ls[:-1]] == [l.name for l in lp] and [l.fn for l in ls[:-1]] == [l.fn for l in lp]
            last, side = mt.plan(slot).ops[-1]
            assert last is ls[-1] and last.fn is rt.lib.dpp_pose_smooth and not side and last.name == 'pose_smooth'
            assert last.args[3:5] == (Tn, mt.J) and last.args[7] == G and (last.args[8] is None) == (C == 2)
            assert last.args[14:19] == (30., 1., 0.007, 2., 2) and last.args[19] == mt.sstate.since.ptr
            assert [l.name for l in none.plan(slot).launches()] == [l.name for l in lp]
        assert plain.res.size == none.res.size and sorted(plain._off) == sorted(none._off) and none.sstate is None and plain.sstate is None
        if groups is None:
            assert plain.res.size == 2 * Tn * J3 + 16 * Tn + 8
        assert all(mt._off[k] == plain._off[k] for k in plain._off) and mt._off['pose_f'] == plain.res.size
        assert mt.res.size == plain.res.size + Tn * (2 * J3 + 1) + G * (J3 + 1)
        assert ('fused_pose_f' in mt._off) == ('gstat' in mt._off) == bool(G)
        st = mt.sstate
        assert st.since.get().tolist() == [-1] * (Tn + G) and st.xh.shape == st.dxh.shape == (Tn + G, mt.J, 3) and st.xh.dtype == np.float64
        for b in (st.since, st.xh, st.dxh):
            assert not mt.res.ptr <= b.ptr < mt.res.ptr + 4 * mt.res.size
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig('small')
    calls = dict(h2d=[], run=0, d2h=[])
    real_in, real_out, real_run = rt.copy_in, rt.download, ops.Plan.run
    monkeypatch.setattr(rt, 'copy_in', lambda buf, arr: (calls['h2d'].append((buf.ptr, buf.size * buf.dtype.itemsize)), real_in(buf, arr))[1], raising=False)
    monkeypatch.setattr(rt, 'download', lambda buf: (calls['d2h'].append(buf.ptr), real_out(buf))[1], raising=False)
    monkeypatch.setattr(ops.Plan, 'run', lambda self, r: (calls.__setitem__('run', calls['run'] + 1), real_run(self, r))[1])
    mt = _tracker(rt, backend, 'small', smooth=SMOOTH)
    calls.update(h2d=[])
    mt.reset(1, starts[1])
    assert calls['h2d'] == [(mt.com.ptr + 12, 12), (mt.sstate.since.ptr + 4, 4)]
    _start(mt, starts)
    f = [(mt.frames.ptr + 4 * int(o), 4 * h * w) for o, (h, w) in zip(mt.table.host['frame_off'], sizes)]
    for i, h2d in ((0, f + [(mt.gate.ptr, 12)]), (1, f), (2, f)):
        calls.update(h2d=[], run=0, d2h=[])
        mt.process(ticks[i])
        assert calls['h2d'] == h2d and calls['run'] == 1 and calls['d2h'] == [mt.res.ptr], (i, calls)
    calls.update(h2d=[])
    mt.set_hand(2, False)                                                # no flip: tflags only
    assert calls['h2d'] == [(mt.tflags.ptr, 12)]
    calls.update(h2d=[])
    mt.set_hand(2, True)
    assert calls['h2d'] == [(mt.sstate.since.ptr + 8, 4), (mt.tflags.ptr, 12)]
    monkeypatch.undo()


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_lost_track_is_held_then_dropped_and_a_reset_starts_it_again(backend):
    """The refinement net that answers (0, 0, -2): track 1 starts two cubes from its camera and reaches depth 0 in tick 1.  Ungrouped, so
    nobody hands it over: LOST in tick 1 (HELD: max_hold = 1), gated -- IDLE on the device -- from tick 2 on (DROPPED, then EMPTY), and
    after reset(1, com) INIT again with pose_f == pose.  A second tracker is reset right after the HELD tick: INIT there, not OK."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig('small')
    par = dict(SMOOTH, max_hold=1)
    far = starts[0]
    for reset_at in (4, 2):
        mt = _tracker(rt, backend, 'small', grouped=False, smooth=par)
        _start(mt, starts)
        ref = _Restated(mt, par)
        words, status = [], []
        for i in range(6):
            if i == reset_at:
                mt.reset(1, far)
                ref.state.since[1] = -1                                  # what the 4-byte upload does
            res = mt.process(ticks[i % 4])
            ref.check(res, None, (reset_at, i))
            words.append(res[1]['smooth'])
            status.append(res[1]['status'])
            if i == reset_at:
                assert np.array_equal(res[1]['pose_f'], res[1]['pose']) and np.array_equal(res[1]['pose_img_f'], res[1]['pose_img'])
            if res[1]['smooth'] & S_EMPTY:
                assert not res[1]['pose_f'].any() and not res[1]['pose_img_f'].any()
            assert [res[t]['smooth'] for t in (0, 2)] == [S_INIT if i == 0 else S_OK] * 2
        if reset_at == 4:
            assert status == [OK, LOST, LOST, LOST, OK, OK] and words == [S_INIT, S_HELD, S_EMPTY | S_DROPPED, S_EMPTY, S_INIT, S_OK]
        else:
            assert status == [OK, LOST, OK, OK, OK, OK] and words == [S_INIT, S_HELD, S_INIT, S_OK, S_OK, S_OK]
        assert np.array_equal(mt.sstate.since.get(), ref.since())


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_source_that_idles_every_second_tick_filters_at_half_the_rate(backend):
    """Source 2 delivers a frame in the even ticks only: its track is IDLE in between (HELD: the last filtered pose again) and its
    valid samples are filtered with Te = 2 / rate -- the bits of a filter at rate / 2 that is fed the even ticks alone."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig('small')
    par = dict(SMOOTH, max_hold=1)
    mt = _tracker(rt, backend, 'small', grouped=False, smooth=par)
    _start(mt, [starts[0]] * 3)
    ref, slow = _Restated(mt, par), S.State(1, mt.J)
    for i in range(6):
        fr = list(ticks[i % 4])
        if i & 1:
            fr[2] = None
        res = mt.process(fr)
        ref.check(res, None, i)
        assert [r['status'] for r in res] == [OK, OK, IDLE if i & 1 else OK]
        if i & 1:
            assert res[2]['smooth'] == S_HELD and np.array_equal(res[2]['pose_f'], last)
        else:
            want = S.smooth(res[2]['pose'][None], [OK], None, [mt.cams[2]], None, None, slow, **dict(par, rate=15.))
            assert res[2]['smooth'] == want['sstat'][0] == (S_OK if i else S_INIT)
            assert res[2]['pose_f'].tobytes() == want['pose_f'][0].tobytes() and res[2]['pose_img_f'].tobytes() == want['pose_img_f'][0].tobytes()
        last = res[2]['pose_f']


@pytest.mark.parametrize('backend,size', SETUPS)
def test_smoothing_process_sequence_equals_a_process_loop(backend, size):
    """Both slots append the same launch on the ONE state and the ticks are stream-ordered: for every track-tick that is OK or IDLE the
    new keys have the loop's bits, `fused_ticks` carries the filtered fused pose of every tick, and the device's `since` is afterwards
    what the loop left.  The ticks: source 1 loses its tracks in tick `drop` (handed over on the device), source 0 idles in tick 3."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig(size)
    Tn = len(tracks)
    frames = [list(fr) for fr in _dropped(size)]
    frames[3][0] = None
    a, b = _tracker(rt, backend, size, smooth=SMOOTH), _tracker(rt, backend, size, smooth=SMOOTH)
    _start(a, starts)
    _start(b, starts)
    loop, loop_fused = [], []
    for fr in frames:
        loop.append(b.process(fr))
        loop_fused.append(b.fused)
    seq = a.process_sequence(iter(frames))
    live = 0
    for i, (ts, tl) in enumerate(zip(seq, loop)):
        for t in range(Tn):
            assert ts[t]['status'] == tl[t]['status'], (i, t)
            if ts[t]['status'] != LOST:
                live += 1
                assert ts[t]['smooth'] == tl[t]['smooth'] and all(ts[t][k].tobytes() == tl[t][k].tobytes() for k in ('pose_f', 'pose_img_f')), (i, t)
        for fa, fb in zip(a.fused_ticks[i], loop_fused[i]):
            assert fa['smooth'] == fb['smooth'] and fa['pose_f'].tobytes() == fb['pose_f'].tobytes(), i
    idle = [[r['status'] for r in tick].count(IDLE) for tick in loop]
    assert idle[3] == sum(c == 0 for c, _ in tracks) and sum(idle) == idle[3] and live == len(frames) * Tn - sum(c == 1 for c, _ in tracks)
    assert {r['smooth'] for r in loop[3] if r['status'] == IDLE} == {S_HELD}
    rt.synchronize()
    assert np.array_equal(a.sstate.since.get(), b.sstate.since.get())
    for k in ('xh', 'dxh'):
        assert getattr(a.sstate, k).get().tobytes() == getattr(b.sstate, k).get().tobytes(), k


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_calibrating_tracker_filters_its_tracks_and_then_its_groups(backend):
    """While a source's extrinsics are pending nothing is fused: the launch runs with G = 0 behind extrinsics_accumulate and
    fused_pose_f / gstat read as zeros.  After finish_calibration() the rebuilt plan passes the groups, whose rows start EMPTY: INIT in
    the first fused tick."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig('small')
    withheld = [extr[0]] + [None] * (len(extr) - 1)
    mt = _tracker(rt, backend, 'small', extrinsics=withheld, calibrate=dict(anchor=0), smooth=SMOOTH)
    _start(mt, starts)
    ref = _Restated(mt, SMOOTH)
    names = [l.name for l in mt.plan().launches()]
    assert mt.calibrating and names[-2:] == ['extrinsics_accumulate', 'pose_smooth'] and mt.plan().launches()[-1].args[7] == 0
    assert mt.plan().launches()[-1].args[5] is None and mt.plan().launches()[-1].args[25] is None
    for i in range(drop + 1):
        res = mt.process(ticks[i])
        assert mt.fused == [] and set(NEW_KEYS) <= set(res[0])
        S.smooth(np.stack([r['pose'] for r in res]), [r['status'] for r in res], mt.src_host, mt.cams, None, None, ref.state, **ref.par)
        blk = mt.block.split(mt.res.get())
        assert not blk['fused_pose_f'].any() and not blk['gstat'].any() and blk['sstat'].tolist() == [r['smooth'] for r in res]
    assert mt.sstate.since.get()[mt.T:].tolist() == [-1] * len(groups)
    report = mt.finish_calibration()
    assert all(r['ok'] for r in report.values()) and not mt.calibrating
    last = mt.plan().launches()[-1]
    assert [l.name for l in mt.plan().launches()][-2:] == ['pose_fuse', 'pose_smooth'] and last.args[7] == len(groups) and last.args[5] == mt.fused_pose.ptr
    centres = mt.com_host.copy()
    centres[1] = starts[1]                                               # the lost one starts again: its row is cleared
    _start(mt, centres)
    ref.state.since[:mt.T] = -1
    res = mt.process(ticks[0])
    assert [r['status'] for r in res] == [OK] * 3 and [f['n'] for f in mt.fused] == [3]
    ref.check(res, mt.fused, 'first fused tick')
    assert [f['smooth'] for f in mt.fused] == [S_INIT] and np.array_equal(mt.fused[0]['pose_f'], mt.fused[0]['pose'])
    res = mt.process(ticks[1])
    ref.check(res, mt.fused, 'second fused tick')
    assert mt.fused[0]['smooth'] == S_OK


@pytest.mark.parametrize('backend', BACKENDS)
def test_smooth_is_validated_on_the_host(backend):
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    good = dict(rate=30., mincutoff=1., beta=0.)
    assert ops.smooth_spec(good) == (30., 1., 0., 1., 0) and ops.smooth_spec(dict(good, dcutoff=2, max_hold=3)) == (30., 1., 0., 2., 3)
    inf = float('inf')
    bad = [dict(good, cutoff=1.), dict(mincutoff=1., beta=0.), dict(rate=30., beta=0.), dict(rate=30., mincutoff=1.), 30., [30., 1., 0.]]
    bad += [dict(good, rate=v) for v in (0., -30., inf, nan, None)] + [dict(good, mincutoff=v) for v in (0., -1., inf, nan)]
    bad += [dict(good, dcutoff=v) for v in (0., -1., inf, nan)] + [dict(good, beta=v) for v in (-1e-9, inf, nan)]
    bad += [dict(good, max_hold=v) for v in (-1, 1.5, 2 ** 31)]
    for b in bad:
        with pytest.raises(ValueError):
            ops.smooth_spec(b)
    for b in (dict(good, cutoff=1.), dict(good, rate=0.), dict(rate=30.)):
        with pytest.raises(ValueError):
            _tracker(rt, backend, 'small', grouped=False, smooth=b)
    st = ops.SmoothState(rt, 3, 4)
    with pytest.raises(ValueError):                                      # a state of other dimensions than the launch
        ops.pose_smooth(rt, st.xh, st.since, 4, 4, ops.smooth_spec(good), st, st.xh, st.xh, st.since, cam=(1., 1., 0., 0., 0))
    with pytest.raises(ValueError):                                      # groups without their buffers
        ops.pose_smooth(rt, st.xh, st.since, 2, 4, ops.smooth_spec(good), st, st.xh, st.xh, st.since, cam=(1., 1., 0., 0., 0), G=1)


# ---- 5: HandTracker -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_hand_tracker_smooths_its_pose(backend):
    """The same launch at T = 1, G = 0 with the scalar camera, last in every plan keyed by `flags`: 6 frames through process() and
    through process_sequence against the restatement, the old keys those of a tracker without `smooth`; a set_hand flip clears the
    state, a set_hand that changes nothing does not."""
    from hipdp.tracker import HandTracker
    from oracle import augment as A
    from tests import track_ref as T
    from tests.test_realtime import _track_nets
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend)
    di, cam, cube, H, W, n = ICVLImporter('../data/ICVL/'), A.Camera.icvl(), (250., 250., 250.), 120, 160, 6
    frames, coms = T.drifting_sequence(np.random.RandomState(32), n, cam, H, W, cube)
    tr, plain = HandTracker(rt, di, pnet, snet, H, W, cube, smooth=SMOOTH), HandTracker(rt, di, pnet, snet, H, W, cube)
    assert len(tr.plan().launches()) == len(plain.plan().launches()) + 1 and tr.plan().ops[-1][0].fn is rt.lib.dpp_pose_smooth
    assert tr.plan().ops[-1][0].args[3:5] == (1, tr.J) and tr.plan().ops[-1][0].args[7:9] == (0, None) and not tr.plan().ops[-1][1]
    assert tr.res.size == plain.res.size + 2 * tr.J * 3 + 1 and len(tr.plan(1).launches()) == len(tr.plan(0).launches())
    cams = [camera_tuple(di)]

    def against(results, state, where):
        for i, r in enumerate(results):
            want = S.smooth(r['pose'][None], [r['status']], None, cams, None, None, state, **dict(SMOOTH, dcutoff=1.))
            assert r['smooth'] == want['sstat'][0] and r['pose_f'].tobytes() == want['pose_f'][0].tobytes(), (where, i)
            assert r['pose_img_f'].tobytes() == want['pose_img_f'][0].tobytes(), (where, i)
    tr.reset(coms[0])
    plain.reset(coms[0])
    loop = [tr.process(f, return_crop=True) for f in frames]
    old = [plain.process(f, return_crop=True) for f in frames]
    for i in range(n):
        assert set(loop[i]) == set(old[i]) | set(NEW_KEYS) and all(np.array_equal(loop[i][k], old[i][k]) for k in old[i]), i
    assert [r['smooth'] for r in loop] == [S_INIT] + [S_OK] * (n - 1)
    against(loop, S.State(1, tr.J), 'process')
    tr.reset(coms[0])                                                    # clears the row: the sequence starts as the loop did
    seq = tr.process_sequence(frames)
    for i in range(n):
        assert all(np.array_equal(seq[i][k], loop[i][k]) for k in loop[i] if k != 'crop'), i
    # the other hand: another plan, the same state, cleared by the flip alone
    state = S.State(1, tr.J)
    tr.reset(coms[0])
    out = [tr.process(frames[0]), tr.process(frames[1])]
    tr.set_hand(True)
    state_flip = S.State(1, tr.J)
    flipped = [tr.process(frames[2])]
    tr.set_hand(True)
    flipped.append(tr.process(frames[3]))
    assert [r['smooth'] for r in out + flipped] == [S_INIT, S_OK, S_INIT, S_OK] and tr.plan().ops[-1][0].fn is rt.lib.dpp_pose_smooth
    against(out, state, 'left')
    against(flipped, state_flip, 'right')
    with pytest.raises(ValueError):
        HandTracker(rt, di, pnet, snet, H, W, cube, smooth=dict(rate=30.))


# ---- 6: the pipelines and the examples --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_both_pipelines_pass_smooth_through(backend, tmp_path):
    from tests.test_multitrack import _nets, _two_icvl_sequences
    from tests.test_realtime import _track_nets
    from util.cameradevice import FileDevice
    from util.realtimehandposepipeline import MultiStreamPipeline, RealtimeHandposePipeline, smoothing_figures
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    n = 3
    base, di, cube, seqs, _ = _two_icvl_sequences(tmp_path, n)
    config = {'fx': 241.42, 'fy': 241.42, 'cube': cube}
    cams = [camera_tuple(di)]
    par = dict(SMOOTH, dcutoff=1.)
    # one hand
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend, J=16)
    rtp = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=seqs[0][1][0], smooth=SMOOTH)
    raw = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=seqs[0][1][0])
    poses = rtp.processVideo(FileDevice(seqs[0][2], di))
    assert np.array_equal(poses, raw.processVideo(FileDevice(seqs[0][2], di))) and raw.poses_f is None and raw._tracker.sstate is None
    assert rtp._tracker.smooth == ops.smooth_spec(SMOOTH) and rtp.poses_f.shape == poses.shape == (n, 16, 3)
    state = S.State(1, 16)
    for i in range(n):
        want = S.smooth(poses[i][None], [OK], None, cams, None, None, state, **par)
        assert rtp.poses_f[i].tobytes() == want['pose_f'][0].tobytes(), i
    res = rtp.processFrame(seqs[0][0][0])
    assert set(NEW_KEYS) <= set(res) and res['smooth'] == S_OK and 'pose_f' not in raw.processFrame(seqs[0][0][0])
    fig = smoothing_figures(poses, rtp.poses_f)
    assert sorted(fig) == ['distance', 'filtered_step', 'raw_step'] and all(np.isfinite(v) and v >= 0. for v in fig.values())
    # two cameras on one sequence, fused
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 2, J=16)
    eye = (np.eye(3), np.zeros(3))
    L = MultiStreamPipeline.HAND_LEFT

    def pipeline(**kw):
        return MultiStreamPipeline(pnet, dict(config, extrinsics=[eye, eye]), di, [FileDevice(seqs[0][2], di), FileDevice(seqs[0][2], di)],
                                   [(0, L), (1, L)], snet, init_com=[seqs[0][1][0]] * 2, groups=[[0, 1]], **kw)
    msp, plain = pipeline(smooth=SMOOTH), pipeline()
    poses, old = msp.processVideos(), plain.processVideos()
    assert all(np.array_equal(a, b) for a, b in zip(poses, old)) and np.array_equal(msp.fused_poses[0], plain.fused_poses[0])
    assert plain.poses_f is None and plain.fused_poses_f is None and 'pose_f' not in plain.fused[0]
    assert [p.shape for p in msp.poses_f] == [(n, 16, 3)] * 2 and [p.shape for p in msp.fused_poses_f] == [(n, 16, 3)]
    state = S.State(3, 16)
    for i in range(n):
        want = S.smooth(np.stack([poses[0][i], poses[1][i]]), [OK, OK], [0, 1], cams * 2, msp.fused_poses[0][i][None], [2], state, **par)
        assert all(msp.poses_f[t][i].tobytes() == want['pose_f'][t].tobytes() for t in (0, 1)), i
        assert msp.fused_poses_f[0][i].tobytes() == want['fused_pose_f'][0].tobytes(), i
    assert msp.fused[0]['smooth'] == S_OK
    over = pipeline(smooth=SMOOTH)
    over.processVideos(overlapped=True)
    assert all(np.array_equal(a, b) for a, b in zip(over.poses_f, msp.poses_f)) and np.array_equal(over.fused_poses_f[0], msp.fused_poses_f[0])


def _driver(name):
    import importlib.util
    from tests.test_multitrack import ROOT
    spec = importlib.util.spec_from_file_location(name + '_smooth_driver', os.path.join(ROOT, 'examples', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _untimed(text):
    """An example's output without its timing line."""
    return [line for line in text.splitlines() if ' ms per ' not in line]


@pytest.mark.parametrize('backend', BACKENDS)
def test_both_examples_print_the_sanity_figures_with_smooth_and_nothing_new_without(backend, tmp_path, capsys):
    from tests.test_multitrack import _two_icvl_sequences
    R.set_default_runtime(get_runtime(backend))
    base, _, _, _, _ = _two_icvl_sequences(tmp_path, 4)
    net = 'resnet' if backend == 'hip' else 'poseregnet'               # (the 128x128 ResNet is too slow for the SIMT emulator)
    common = ['--dataset', 'icvl', '--data', base, '--net', net, '--cache', str(tmp_path / 'cache')]
    flag = ['--smooth', '30', '1.0', '0.007', '--hold', '2']

    def figures_ok(fig):
        return sorted(fig) == ['distance', 'filtered_step', 'raw_step'] and all(np.isfinite(v) and v >= 0. for v in fig.values())
    # one hand.  examples/test_realtimepipeline.py is a test_*.py file and stays as it is: its --smooth lives in examples/realtime_smooth.py,
    # which has no main of its own (as examples/realtime_sensor.py): it hands everything else to that example's main().
    one, smoothed = _driver('test_realtimepipeline'), _driver('realtime_smooth')
    capsys.readouterr()
    poses, err = one.main(common)
    plain_out = capsys.readouterr().out
    again = smoothed.main(common)                                        # without the flag: that example, output and all
    again_out = capsys.readouterr().out
    assert len(again) == 2 and np.array_equal(again[0], poses) and again[1] == err and _untimed(again_out) == _untimed(plain_out)
    assert 'smoothing' not in plain_out and any('Mean error' in line for line in _untimed(plain_out))
    poses_s, err_s, fig, poses_f = smoothed.main(common + flag)
    out = capsys.readouterr().out
    assert np.array_equal(poses, poses_s) and err_s == err and poses_f.shape == poses.shape == (4, 16, 3) and figures_ok(fig)
    assert np.array_equal(poses_f[0], poses[0]) and not np.array_equal(poses_f[1:], poses[1:])      # INIT, then filtered
    assert _untimed(out)[:-1] == _untimed(plain_out) and out.count('smoothing') == 1
    assert 'smoothing (sanity figures): mean frame-to-frame displacement' in _untimed(out)[-1] and 'mean raw-to-filtered distance' in out
    # that example's other options still apply to the filtered run
    right = smoothed.main(common + flag + ['--seed', 'com', '--hand', 'right', '--max-frames', '2'])
    capsys.readouterr()
    assert right[0].shape == right[3].shape == (2, 16, 3) and np.array_equal(right[3][0], right[0][0]) and figures_ok(right[2])
    multi = _driver('realtime_multi')
    capsys.readouterr()
    poses, errs = multi.main(common + ['--max-frames', '3'])
    plain_out = capsys.readouterr().out
    poses_s, errs_s, figs = multi.main(common + ['--max-frames', '3'] + flag)
    out = capsys.readouterr().out
    assert all(np.array_equal(a, b) for a, b in zip(poses, poses_s)) and errs == errs_s and len(figs) == 3 and all(figures_ok(f) for f in figs)
    assert 'smoothing' not in plain_out and _untimed(out)[:-3] == _untimed(plain_out) and out.count('smoothing (sanity figures)') == 3
    fused = multi.main(common + ['--fuse', '--max-frames', '3'])
    plain_out = capsys.readouterr().out
    fused_s = multi.main(common + ['--fuse', '--max-frames', '3'] + flag)
    out = capsys.readouterr().out
    assert 'smooth' not in fused and 'smoothing' not in plain_out and figures_ok(fused_s['smooth']) and np.array_equal(fused['fused'], fused_s['fused'])
    assert _untimed(out)[:-1] == _untimed(plain_out) and 'fused pose, smoothing (sanity figures)' in out
