"""Timestamps per source and time-aligned fusion (csrc/align.hip: dpp_pose_align; csrc/smooth.hip: dpp_pose_smooth_t; ABI v24; `timing=`
of hipdp/multitrack.py and hipdp/tracker.py).  The semantics are this project's own -- the reference has one camera -- so both launches
are pinned bit for bit to the NumPy restatement of tests/align_ref.py, the alignment is checked on inputs on which every operation is
exact, independently of the restatement, and then the trackers on top: old keys kept, new keys restated, the plan's structure and
counters, lost / handed / reset tracks, process_sequence against a process() loop, a calibrating tracker, validation, HandTracker, the
pipeline classes and the example.  Every test runs on the emulator (CPU tier) and through libdpp_hip.so (-m gpu)."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

from data.importers import DepthImporter, ICVLImporter, MSRA15Importer
from hipdp import lib, ops
from hipdp import runtime as R
from hipdp.augmenter import camera_tuple
from tests import align_ref as A
from tests import smooth_ref as S
from tests.backends import BACKENDS, get_runtime
from tests.test_smooth import GWORDS, N_IN, PAPER, STATUS, WORDS, _Rows, _walk

OK, LOST, IDLE = 0, 1, 2
NONE, MOVED, ASIS = ops.ALIGN_NONE, ops.ALIGN_MOVED, ops.ALIGN_ASIS
NOPREV, GAP, FAR = ASIS | ops.ALIGN_NOPREV, ASIS | ops.ALIGN_GAP, ASIS | ops.ALIGN_FAR
S_OK, S_INIT, S_HELD, S_EMPTY, S_DROPPED, S_STALE = (ops.SMOOTH_OK, ops.SMOOTH_INIT, ops.SMOOTH_HELD, ops.SMOOTH_EMPTY, ops.SMOOTH_DROPPED,
                                                     ops.SMOOTH_STALE)
ALIGN_OUT = ('pose_t', 'pose_img_t', 'com3d_t', 'lead', 'astat')
SMOOTH_OUT = ('pose_f', 'pose_img_f', 'sstat', 'fused_pose_f', 'gstat')
nan = np.nan
P = 1. / 32.                                                             # the scripts' tick: a power of two, so every stamp is exact


def test_the_constants_are_the_headers():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dpp_hip.h')).read()
    for name in ('NONE', 'MOVED', 'ASIS', 'NOPREV', 'GAP', 'FAR'):
        v = getattr(ops, 'ALIGN_' + name)
        assert '#define DPP_ALIGN_%s %d\n' % (name, v) in hdr and getattr(A, name) == v
    assert '#define DPP_SMOOTH_STALE %d\n' % ops.SMOOTH_STALE in hdr and A.STALE == ops.SMOOTH_STALE
    words = [ops.ALIGN_MOVED, ops.ALIGN_ASIS, ops.ALIGN_NOPREV, ops.ALIGN_GAP, ops.ALIGN_FAR]
    assert ops.ALIGN_NONE == 0 and all(w & (w - 1) == 0 for w in words) and len(set(words)) == 5
    assert ops.SMOOTH_STALE not in (S_OK, S_INIT, S_HELD, S_EMPTY, S_DROPPED) and ops.SMOOTH_STALE & (ops.SMOOTH_STALE - 1) == 0
    assert lib.ABI_VERSION >= 24 and '#define DPP_ABI_VERSION %d\n' % lib.ABI_VERSION in hdr


# ---- 1: the launch alone against the restatement -----------------------------------------------------------------------------------
class _Tracks(object):
    """One align state of T rows on the device and its restatement, both with a pad row behind; every buffer the launch may write starts
    as NaN (`have`: 0, the pad 12345; astat -7), so a region it leaves alone keeps NaN bits and a NONE row must have been written as zeros.
    table: three cameras through the ABI v19 table; scalar: ONE camera as launch scalars, the tracks still naming three sources' stamps
    (T = 1: src is NULL and the track reads stamps[0])."""

    def __init__(self, rt, T, J, form, spec):
        self.rt, self.T, self.J, self.spec = rt, T, J, spec
        half = DepthImporter(241.42 / 2, 241.42 / 2, 80., 60.)
        self.src_host = np.int32([2, 0, 1, 0, 1][:T])
        self.C = 3
        if form == 'table':
            self.cams = [camera_tuple(di) for di in (ICVLImporter('../data/ICVL/'), MSRA15Importer('../data/MSRA15/'), half)]
            self.table = ops.SourceTable(rt, self.cams, [(abs(c[0]), abs(c[1])) for c in self.cams], [(240, 320), (240, 320), (120, 160)])
        else:
            self.cams = [camera_tuple(MSRA15Importer('../data/MSRA15/'))] * 3                 # flip_y
            assert self.cams[0][4]
            self.table = None
            if T == 1:
                self.src_host = None
        self.src = None if self.src_host is None else rt.upload(self.src_host)
        self.state = ops.AlignState(rt, T + 1, J)
        self.ref = A.AlignState(T + 1, J, fill=nan)
        self.ref.have[T] = 12345
        for k in ('have', 'pt', 'pp', 'pc'):
            getattr(self.state, k).set(getattr(self.ref, k))
        f32, i32 = np.float32, np.int32
        self.want = dict(pose_t=np.full((T + 1, J, 3), nan, f32), pose_img_t=np.full((T + 1, J, 3), nan, f32), com3d_t=np.full((T + 1, 3), nan, f32),
                         lead=np.full(T + 1, nan, f32), astat=np.full(T + 1, -7, i32))
        self.out = dict((k, rt.upload(v)) for k, v in self.want.items())

    def clear(self, t):
        self.state.clear(t)
        self.ref.have[t] = 0

    def tick(self, pose, com, status, stamps):
        rt, T, J, o = self.rt, self.T, self.J, self.out
        stamps = np.float64(stamps)
        p, c3, st, sm = rt.upload(pose), rt.upload(com), rt.upload(np.int32(status)), rt.upload(stamps)
        ops.pose_align(rt, p, c3, st, self.src, T, J, sm, self.C, ops.timing_spec(self.spec), self.state, o['pose_t'], o['pose_img_t'],
                       o['com3d_t'], o['lead'], o['astat'], cam=self.cams[0], table=self.table)(rt.stream)
        rt.synchronize()
        res = A.align(pose, com, status, self.src_host, self.cams, stamps, self.ref, **self.spec)
        for k in ALIGN_OUT:
            self.want[k][:T] = res[k]
            got = o[k].get()
            assert got.dtype == self.want[k].dtype and got.tobytes() == self.want[k].tobytes(), k
        for k in ('have', 'pt', 'pp', 'pc'):
            assert getattr(self.state, k).get().tobytes() == getattr(self.ref, k).tobytes(), k
        assert np.array_equal(p.get(), pose) and np.array_equal(c3.get(), com) and np.array_equal(st.get(), np.int32(status))   # read only
        assert np.array_equal(sm.get(), stamps) and (self.src is None or np.array_equal(self.src.get(), self.src_host))
        return res


# ten launches: tracks on sources (2, 0, 1, 0, 1); max_gap = 2.5 P, max_lead = 0.4 P.  Source 0 is stamped i P, source 1 a quarter tick
# and source 2 half a tick earlier (FAR), and `now` is source 0's stamp, except:
ALIGN_SPEC = dict(max_gap=2.5 * P, max_lead=0.4 * P)


def _script_stamps(i):
    s = [i * P, i * P - P / 4, i * P - P / 2, i * P]
    if i in (3, 4):
        s[2] = i * P - P / 8                                             # source 2 within max_lead
    if i == 5:
        s[1] = 4 * P - P / 4                                             # source 1 repeats its stamp: dt == 0
    if i == 7:
        s[3] = i * P - P / 8                                             # `now` before source 0's stamp: a negative lead, within max_lead
    if i == 9:
        s[3] = i * P - P / 2                                             # ... and beyond it; source 2 has lead 0
    return s


ALIGN_STATUS = [[OK] * 10,
                [OK, OK, LOST, LOST, LOST, OK, OK, IDLE, OK, OK],        # dt = 4 P > max_gap in launch 5, 2 P in launch 8
                [OK] * 10,
                [LOST, IDLE, OK, OK, OK, OK, OK, OK, OK, OK],            # cleared by the host before launch 5
                [IDLE, LOST] * 5]                                        # never OK: its state keeps its NaN
ALIGN_WORDS = [[NOPREV, FAR, FAR, MOVED, MOVED, FAR, FAR, MOVED, FAR, MOVED],
               [NOPREV, MOVED, NONE, NONE, NONE, GAP, MOVED, NONE, MOVED, FAR],
               [NOPREV, MOVED, MOVED, MOVED, MOVED, GAP, MOVED, MOVED, MOVED, MOVED],
               [NONE, NONE, NOPREV, MOVED, MOVED, NOPREV, MOVED, MOVED, MOVED, FAR],
               [NONE] * 10]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('form', ['table', 'scalar'])
@pytest.mark.parametrize('T,J', [(5, 5), (5, 70), (1, 1)])
def test_pose_align_equals_the_restatement_bit_for_bit(backend, form, T, J):
    """Ten launches into ONE state, every output array and all four state arrays compared after each.  J = 70 reaches the second joint of
    a lane.  The script reaches every word: MOVED (with a positive, a zero and a negative lead), ASIS with NOPREV, GAP (dt == 0 and
    dt > max_gap) and FAR (either sign), NONE for LOST and for IDLE, and a row the host clears in mid-run."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(17 + J)
    rows = _Tracks(rt, T, J, form, ALIGN_SPEC)
    poses, coms = _walk(rng, 10, T, J), [c[:, 0] for c in _walk(rng, 10, T, 1)]
    seen, leads = set(), set()
    for i in range(10):
        if i == 5 and T == 5:
            rows.clear(3)
        before = rows.ref.copy()
        status = [ALIGN_STATUS[t][i] for t in range(T)]
        res = rows.tick(poses[i], coms[i], status, _script_stamps(i))
        if T == 5:
            assert res['astat'].tolist() == [ALIGN_WORDS[t][i] for t in range(T)], i
        for t, w in enumerate(res['astat'].tolist()):
            seen.add((w, status[t]) if w == NONE else w)
            if w == NONE:
                assert not res['pose_t'][t].any() and not res['pose_img_t'][t].any() and not res['com3d_t'][t].any() and res['lead'][t] == 0
                for k in ('have', 'pt', 'pp', 'pc'):                       # the state: untouched
                    assert getattr(rows.ref, k)[t].tobytes() == getattr(before, k)[t].tobytes()
                continue
            if w & ASIS:                                                 # the inputs' bits
                assert res['pose_t'][t].tobytes() == poses[i][t].tobytes() and res['com3d_t'][t].tobytes() == coms[i][t].tobytes()
            else:
                leads.add(float(np.sign(res['lead'][t])))
                if res['lead'][t] != 0:
                    assert not np.array_equal(res['pose_t'][t], poses[i][t])
            assert rows.ref.have[t] == 1 and rows.ref.pp[t].tobytes() == poses[i][t].tobytes() and rows.ref.pc[t].tobytes() == coms[i][t].tobytes()
    if T == 5:
        assert seen == {MOVED, NOPREV, GAP, FAR, (NONE, LOST), (NONE, IDLE)} and leads == {-1., 0., 1.}
        assert np.isnan(rows.ref.pp[4]).all() and np.isnan(rows.ref.pt[4]) and rows.ref.have[4] == 0           # the row that was never OK
    else:
        assert {MOVED, NOPREV} <= seen


# ---- 2: what an alignment must do, independently of the restatement ---------------------------------------------------------------------
STEP = 1. / 64.                                                          # the trajectories' time step (s)


def _trajectory(seed, rows, J):
    """x0 [rows][J][3] and s [rows][J][3], multiples of 1/64 mm: |x0| < 512 (z in 256 .. 512, in front of the camera), |s| < 4, so every
    x0 + k s with k <= 8 is a multiple of 1/64 below 1024 mm -- 16 significant bits, exact in float32."""
    rng = np.random.RandomState(seed)
    x0 = rng.randint(-2 ** 15 + 1, 2 ** 15, (rows, J, 3)) / 64.
    x0[..., 2] = rng.randint(2 ** 14, 2 ** 15, (rows, J)) / 64.
    s = rng.randint(-255, 256, (rows, J, 3)) / 64.
    s[s == 0] = 1. / 64.
    return x0, s


def _at(x0, s, k):
    x = x0 + k * s
    assert np.abs(x).max() < 1024. and np.array_equal(x.astype(np.float32).astype(np.float64), x) and np.array_equal(x * 64., np.round(x * 64.))
    return x.astype(np.float32)


def _exact(x0, s, k_prev, k, k_now):
    """The claim of exactness, checked in rational arithmetic: with float32 samples at steps k_prev and k, v = (x - xp) / dt and
    y = x + v * lead are formed without any rounding in float64, and y is the trajectory's point at k_now, a float32 number."""
    dt, lead = (k - k_prev) * STEP, (k_now - k) * STEP
    for a, b in zip(x0.ravel(), s.ravel()):
        x, xp = Fraction(float(np.float32(a + k * b))), Fraction(float(np.float32(a + k_prev * b)))
        diff = np.float64(float(x)) - np.float64(float(xp))
        v = diff / np.float64(dt)
        y = np.float64(float(x)) + v * np.float64(lead)
        assert Fraction(float(diff)) == x - xp and Fraction(float(v)) == (x - xp) / Fraction(dt) and Fraction(float(y)) == x + (x - xp) / Fraction(dt) * Fraction(lead)
        assert Fraction(float(np.float32(y))) == Fraction(float(a)) + k_now * Fraction(float(b))
    return True


class _Plain(object):
    """T tracks on T sources through the scalar camera, fresh buffers: launch after launch into one state."""

    def __init__(self, rt, T, J, spec=None):
        self.rt, self.T, self.J = rt, T, J
        self.cam = camera_tuple(ICVLImporter('../data/ICVL/'))
        self.spec = ops.timing_spec(spec or dict(max_gap=1., max_lead=1.))
        self.state = ops.AlignState(rt, T, J)
        self.src = rt.upload(np.arange(T, dtype=np.int32))
        self.status = rt.upload(np.zeros(T, np.int32))
        self.out = [rt.alloc((T, J, 3)), rt.alloc((T, J, 3)), rt.alloc((T, 3)), rt.alloc((T,)), rt.alloc((T,), np.int32)]

    def tick(self, pose, com, stamps):
        rt = self.rt
        ops.pose_align(rt, rt.upload(pose), rt.upload(com), self.status, self.src, self.T, self.J, rt.upload(np.float64(stamps)), self.T, self.spec,
                       self.state, *self.out, cam=self.cam)(rt.stream)
        rt.synchronize()
        return dict(zip(ALIGN_OUT, [b.get() for b in self.out]))


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_track_on_a_straight_line_is_moved_to_the_lines_point_at_now(backend):
    """(a) a track sampled at the even steps with `now` one step later returns EXACTLY the trajectory's point at `now`, joints and centre:
    the velocity between two samples of a straight line is the line's."""
    rt = get_runtime(backend)
    J = 21
    x0, s = _trajectory(41, 1, J + 1)
    assert _exact(x0, s, 0, 2, 3) and _exact(x0, s, 2, 4, 5) and _exact(x0, s, 4, 6, 7)
    tr = _Plain(rt, 1, J)
    for k in (0, 2, 4, 6):
        x = _at(x0, s, k)
        res = tr.tick(x[:, :J], x[:, J], [k * STEP, (k + 1) * STEP])
        want = _at(x0, s, k + 1)
        assert res['lead'][0] == np.float32(STEP)
        if k == 0:
            assert res['astat'][0] == NOPREV and np.array_equal(res['pose_t'], x[:, :J]) and np.array_equal(res['com3d_t'], x[:, J])
        else:
            assert res['astat'][0] == MOVED and np.array_equal(res['pose_t'], want[:, :J]) and np.array_equal(res['com3d_t'], want[:, J]), k
            img = np.float32([S.to_img(tr.cam, p) for p in want[0, :J]])
            assert res['pose_img_t'][0].tobytes() == img.tobytes(), k


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_track_stamped_now_comes_back_as_it_went_in(backend):
    """(b) lead == 0: the input's bits with the word MOVED, whatever the velocity (seeded float32 poses that jump by tens of mm)."""
    rt = get_runtime(backend)
    J = 21
    rng = np.random.RandomState(43)
    poses, coms = _walk(rng, 4, 1, J), [c[:, 0] for c in _walk(rng, 4, 1, 1)]
    tr = _Plain(rt, 1, J)
    for i in range(4):
        res = tr.tick(poses[i], coms[i], [i * P, i * P])
        assert res['astat'][0] == (MOVED if i else NOPREV) and res['lead'][0] == 0
        assert res['pose_t'].tobytes() == poses[i].tobytes() and res['com3d_t'].tobytes() == coms[i].tobytes(), i


@pytest.mark.parametrize('backend', BACKENDS)
def test_two_cameras_one_lagging_fuse_to_the_synchronous_pose_once_aligned(backend):
    """(c) two members of one group through identity extrinsics see one trajectory; the second is one step late.  ops.pose_fuse on the
    ALIGNED arrays gives exactly the fused pose of two synchronous samples (the trajectory's point at `now`); on the unaligned arrays it is
    off by exactly s / 2 in every coordinate."""
    rt = get_runtime(backend)
    J = 14
    x0, s = _trajectory(47, 1, J + 1)
    x0, s = np.repeat(x0, 2, 0), np.repeat(s, 2, 0)
    assert _exact(x0[:1], s[:1], 1, 3, 4) and _exact(x0[:1], s[:1], 2, 4, 4)
    tr = _Plain(rt, 2, J)
    eye = (np.eye(3), np.zeros(3))
    rig = ops.FuseRig(rt, [eye, eye], [[0, 1]], [0, 1], 2)
    co = rt.upload(np.zeros((2, 3), np.float32))
    fp, fc, sp, n = rt.alloc((1, J, 3), zero=False), rt.alloc((1, 3), zero=False), rt.alloc((1, J), zero=False), rt.alloc((1,), np.int32)
    pc, fs = rt.alloc((2, 3)), rt.alloc((2,), np.int32)

    def fused(pose, com):
        ops.pose_fuse(rt, pose, com, tr.status, tr.src, 2, J, rig, None, 240, 320, tr.cam, None, False, co, fp, fc, sp, n, pc, fs)(rt.stream)
        rt.synchronize()
        assert n.get().tolist() == [2]
        return fp.get()[0].astype(np.float64), fc.get()[0].astype(np.float64)
    for k in (2, 4, 6):
        x = np.concatenate([_at(x0[:1], s[:1], k), _at(x0[1:], s[1:], k - 1)])
        res = tr.tick(x[:, :J], x[:, J], [k * STEP, (k - 1) * STEP, k * STEP])
        if k == 2:
            continue
        assert res['astat'].tolist() == [MOVED, MOVED] and res['lead'].tolist() == [0., STEP]
        sync = _at(x0[:1], s[:1], k)[0].astype(np.float64)
        pose, com = fused(tr.out[0], tr.out[2])
        assert np.array_equal(pose, sync[:J]) and np.array_equal(com, sync[J]), k
        pose, com = fused(rt.upload(x[:, :J]), rt.upload(x[:, J]))
        assert np.array_equal(sync[:J] - pose, s[0, :J] / 2.) and np.array_equal(sync[J] - com, s[0, J] / 2.), k


# ---- 3: dpp_pose_smooth_t -----------------------------------------------------------------------------------------------------------------
class _TimedRows(_Rows):
    """tests.test_smooth._Rows on a timed state: tlast starts as NaN as well, and tick() launches dpp_pose_smooth_t."""

    def __init__(self, rt, T, J, G, form, par):
        _Rows.__init__(self, rt, T, J, G, form, par)
        Rn = T + G
        self.state = ops.SmoothState(rt, Rn + 1, J, timed=True)
        self.ref = A.SmoothState(Rn + 1, J, fill=nan)
        self.ref.since[Rn] = 12345
        for k in ('since', 'xh', 'dxh', 'tlast'):
            getattr(self.state, k).set(getattr(self.ref, k))
        self.C = 1 if self.src_host is None else 3

    def tick(self, pose, status, stamps, fused=None, n=None):
        rt, T, J, G, o = self.rt, self.T, self.J, self.G, self.out
        stamps = np.float64(stamps)
        assert len(stamps) == self.C + 1
        p, st, sm = rt.upload(pose), rt.upload(np.int32(status)), rt.upload(stamps)
        grp = {}
        if G:
            fp, nn = rt.upload(fused), rt.upload(np.int32(n))
            grp = dict(fused_pose=fp, n=nn, G=G, fused_pose_f=o['fused_pose_f'], gstat=o['gstat'])
        op = ops.pose_smooth(rt, p, st, T, J, ops.smooth_spec(dict(self.par, rate=1.)), self.state, o['pose_f'], o['pose_img_f'], o['sstat'],
                             cam=self.cams[0], src=self.src, table=self.table, stamps=sm, C=self.C, **grp)
        assert op.fn is rt.lib.dpp_pose_smooth_t and op.name == 'pose_smooth_t'
        op(rt.stream)
        rt.synchronize()
        par = dict((k, v) for k, v in self.par.items() if k != 'rate')
        res = A.smooth_t(pose, status, self.src_host, self.cams, fused if G else None, n, self.ref, stamps, **par)
        for k in SMOOTH_OUT:
            rows = G if k in ('fused_pose_f', 'gstat') else T
            self.want[k][:rows] = res[k]
            got = o[k].get()
            assert got.dtype == self.want[k].dtype and got.tobytes() == self.want[k].tobytes(), k
        for k in ('since', 'xh', 'dxh', 'tlast'):
            assert getattr(self.state, k).get().tobytes() == getattr(self.ref, k).tobytes(), k
        assert np.array_equal(p.get(), pose) and np.array_equal(st.get(), np.int32(status)) and np.array_equal(sm.get(), stamps)
        return res


def _jitter_stamps(rng, i, C):
    """Per source a stamp near i / 30 s that grows from tick to tick (jitter below a third of the period), then `now`, the largest."""
    s = [(i + rng.uniform(-0.3, 0.3)) / 30. for _ in range(C)]
    return s + [max(s)]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('form', ['table', 'scalar'])
@pytest.mark.parametrize('T,J,G', [(5, 5, 2), (5, 70, 2), (1, 1, 0)])
def test_pose_smooth_t_equals_the_restatement_bit_for_bit(backend, form, T, J, G):
    """test_smooth's ten-tick script with jittered stamps per source: ten launches into ONE state, every output array and all FOUR state
    arrays compared after each.  The words are the tick-counting launch's (no stamp repeats), the elapsed times are not."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(23 + J)
    rows = _TimedRows(rt, T, J, G, form, dict(PAPER, max_hold=2))
    poses, fused = _walk(rng, 10, T, J), _walk(rng, 10, max(G, 1), J)
    for i in range(10):
        before = rows.ref.copy()
        stamps = _jitter_stamps(rng, i, rows.C)
        res = rows.tick(poses[i], [STATUS[t][i] for t in range(T)], stamps, fused[i][:G], [N_IN[g][i] for g in range(G)])
        assert res['sstat'].tolist() == [WORDS[t][i] for t in range(T)], i
        assert res['gstat'].tolist() == [GWORDS[g][i] for g in range(G)], i
        for r, w in enumerate(res['sstat'].tolist() + res['gstat'].tolist()):
            s = stamps[-1] if r >= T else stamps[0 if rows.src_host is None else rows.src_host[r]]
            if w in (S_OK, S_INIT):
                assert rows.ref.tlast[r] == s
            else:
                assert rows.ref.tlast[r].tobytes() == before.tlast[r].tobytes()
    if T == 5:
        assert np.isnan(rows.ref.tlast[2])                               # the row that was never valid


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('form', ['table', 'scalar'])
@pytest.mark.parametrize('T,J,G', [(5, 5, 2), (5, 70, 2), (1, 1, 0)])
def test_ticks_that_are_a_clock_give_the_tick_counting_launchs_bytes(backend, form, T, J, G):
    """rate = 32 and every stamp k / 32: Te = k2 / 32 - k1 / 32 is exactly (since + 1) / 32, so dpp_pose_smooth_t gives dpp_pose_smooth's
    bytes in every output and in since / xh / dxh over the ten-tick script."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(29 + J)
    par = dict(PAPER, rate=32., max_hold=2)
    timed, counted = _TimedRows(rt, T, J, G, form, par), _Rows(rt, T, J, G, form, par)
    poses, fused = _walk(rng, 10, T, J), _walk(rng, 10, max(G, 1), J)
    for i in range(10):
        args = (poses[i], [STATUS[t][i] for t in range(T)])
        grp = (fused[i][:G], [N_IN[g][i] for g in range(G)])
        a = timed.tick(*(args + ([i / 32.] * (timed.C + 1),) + grp))
        b = counted.tick(*(args + grp))
        for k in SMOOTH_OUT:
            assert timed.out[k].get().tobytes() == counted.out[k].get().tobytes() and a[k].tobytes() == b[k].tobytes(), (i, k)
        for k in ('since', 'xh', 'dxh'):
            assert getattr(timed.state, k).get().tobytes() == getattr(counted.state, k).get().tobytes(), (i, k)


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_repeated_stamp_is_stale_and_held(backend):
    """A valid sample whose stamp is not later than the row's last one is refused: STALE together with HELD (then with DROPPED: max_hold
    keeps counting ticks), the state's values and tlast untouched; a later stamp is filtered against the untouched state."""
    rt = get_runtime(backend)
    J = 5
    rng = np.random.RandomState(31)
    rows = _TimedRows(rt, 1, J, 0, 'scalar', dict(PAPER, max_hold=1))
    poses = _walk(rng, 7, 1, J)
    script = [(0., S_INIT), (P, S_OK), (P, S_HELD | S_STALE), (2 * P, S_OK), (P, S_HELD | S_STALE), (2 * P, S_EMPTY | S_DROPPED | S_STALE),
              (2 * P, S_INIT)]
    for i, (s, word) in enumerate(script):
        before = rows.ref.copy()
        res = rows.tick(poses[i], [OK], [s, s])
        assert res['sstat'].tolist() == [word], i
        if word & S_STALE:
            for k in ('xh', 'dxh', 'tlast'):
                assert getattr(rows.ref, k)[0].tobytes() == getattr(before, k)[0].tobytes(), (i, k)
        if word == S_HELD | S_STALE:
            assert res['pose_f'][0].tobytes() == before.xh[0].astype(np.float32).tobytes() and rows.ref.since[0] == before.since[0] + 1
        if word & S_EMPTY:
            assert not res['pose_f'].any() and not res['pose_img_f'].any() and rows.ref.since[0] == -1


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_source_that_delivers_every_second_tick_filters_over_its_own_time(backend):
    """Two tracks on two sources: source 1 delivers in the even ticks only (IDLE in between: HELD), with its true stamps.  Its filtered
    poses have the bits of a filter that is fed those samples alone, tick after tick -- the elapsed time comes from the stamps, not from
    counted ticks."""
    rt = get_runtime(backend)
    J = 21
    rng = np.random.RandomState(37)
    par = dict(PAPER, max_hold=1)
    cams = [camera_tuple(ICVLImporter('../data/ICVL/'))] * 2
    poses = _walk(rng, 8, 2, J)
    src = rt.upload(np.int32([0, 1]))
    state, alone = ops.SmoothState(rt, 2, J, timed=True), ops.SmoothState(rt, 1, J, timed=True)
    pf, pi, ss = rt.alloc((2, J, 3)), rt.alloc((2, J, 3)), rt.alloc((2,), np.int32)
    af, ai, as_ = rt.alloc((1, J, 3)), rt.alloc((1, J, 3)), rt.alloc((1,), np.int32)
    spec = ops.smooth_spec(dict(par, rate=1.))
    ok1 = rt.upload(np.int32([OK]))
    last = None
    for i in range(8):
        even = not i & 1
        stamps = [i / 30., (i + 0.25) / 30. if even else 0., (i + 0.25) / 30.]
        ops.pose_smooth(rt, rt.upload(poses[i]), rt.upload(np.int32([OK, OK if even else IDLE])), 2, J, spec, state, pf, pi, ss, cam=cams[0],
                        src=src, stamps=rt.upload(np.float64(stamps)), C=2)(rt.stream)
        rt.synchronize()
        if even:
            ops.pose_smooth(rt, rt.upload(poses[i][1:]), ok1, 1, J, spec, alone, af, ai, as_, cam=cams[0],
                            stamps=rt.upload(np.float64([stamps[1], stamps[1]])), C=1)(rt.stream)
            rt.synchronize()
            assert ss.get().tolist() == [S_OK if i else S_INIT] * 2 and as_.get().tolist() == [S_OK if i else S_INIT]
            assert pf.get()[1].tobytes() == af.get()[0].tobytes() and pi.get()[1].tobytes() == ai.get()[0].tobytes(), i
        else:
            assert ss.get().tolist() == [S_OK, S_HELD] and pf.get()[1].tobytes() == last.tobytes()
        last = pf.get()[1]
    for k in ('xh', 'dxh'):
        assert getattr(state, k).get()[1].tobytes() == getattr(alone, k).get()[0].tobytes()
    assert state.tlast.get()[1] == alone.tlast.get()[0] == (6 + 0.25) / 30.


# ---- 4: the entry points' refusals ------------------------------------------------------------------------------------------------------
def _product_library():
    import __graft_entry__
    if not os.path.exists(lib.DEFAULT_LIB):
        __graft_entry__.build()
    so = lib.load()
    assert so.dpp_abi_version() == lib.ABI_VERSION >= 24
    return so


def test_pose_align_entry_point_refuses_bad_arguments_without_a_gpu():
    """Argument validation happens before any launch: callable on the product library without a GPU."""
    so = _product_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    E = 10001
    inf, qnan = float('inf'), float('nan')

    def call(**kw):
        a = dict(pose3d=p, com3d=p, status=p, src=p, T=2, J=5, stamps=p, C=2, sources=None, fx=1., fy=1., ux=0., uy=0., flip=0, max_gap=0.1,
                 max_lead=0.02, have=p, pt=p, pp=p, pc=p, pose_t=p, pose_img_t=p, com3d_t=p, lead=p, astat=p)
        a.update(kw)
        return so.dpp_pose_align(*(list(a.values()) + [None]))
    for k in ('pose3d', 'com3d', 'status', 'stamps', 'have', 'pt', 'pp', 'pc', 'pose_t', 'pose_img_t', 'com3d_t', 'lead', 'astat'):
        assert call(**{k: None}) == E, k
    assert call(sources=p, src=None) == E                                # a table needs src
    assert all(call(**{k: v}) == E for k in ('T', 'J', 'C') for v in (0, -1))
    assert all(call(max_gap=v) == E for v in (0., -0.1, inf, -inf, qnan))
    assert all(call(max_lead=v) == E for v in (-1e-9, inf, -inf, qnan))
    assert call(fx=0.) == E and call(fy=0.) == E


def test_pose_smooth_t_entry_point_refuses_bad_arguments_without_a_gpu():
    so = _product_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    E = 10001
    inf, qnan = float('inf'), float('nan')

    def call(**kw):
        a = dict(pose3d=p, status=p, src=p, T=2, J=5, fused_pose=p, n=p, G=1, sources=None, fx=1., fy=1., ux=0., uy=0., flip=0, stamps=p, C=2,
                 mincutoff=1., beta=0., dcutoff=1., max_hold=0, since=p, tlast=p, xh=p, dxh=p, pose_f=p, pose_img_f=p, sstat=p, fused_pose_f=p,
                 gstat=p)
        a.update(kw)
        return so.dpp_pose_smooth_t(*(list(a.values()) + [None]))
    for k in ('pose3d', 'status', 'stamps', 'since', 'tlast', 'xh', 'dxh', 'pose_f', 'pose_img_f', 'sstat', 'fused_pose', 'n', 'fused_pose_f',
              'gstat'):
        assert call(**{k: None}) == E, k
    assert call(sources=p, src=None) == E                                # a table needs src
    assert all(call(**{k: v}) == E for k in ('T', 'J', 'C') for v in (0, -1)) and call(G=-1) == E and call(max_hold=-1) == E
    for k in ('mincutoff', 'dcutoff'):
        assert all(call(**{k: v}) == E for v in (0., -1., inf, -inf, qnan)), k
    assert all(call(beta=v) == E for v in (-1e-9, inf, -inf, qnan))
    assert call(fx=0.) == E and call(fy=0.) == E


# ---- 5: MultiTracker ------------------------------------------------------------------------------------------------------------------------
from tests import calib_ref as K  # noqa: E402
from tests.test_fuse import OLD_KEYS, SETUPS, _dropped, _fused_matches_the_restatement, _rig, _tracker  # noqa: E402  (the fusion tests' rigs, not edited)
from tests.test_smooth import SMOOTH, _start  # noqa: E402

TIMING = dict(max_gap=0.1, max_lead=0.02)
TIMING_SPEC = (0.1, 0.02)
VIS = dict(radius=2, margin=30., min_support=3)                        # any legal spec: the plan's structure is what is looked at
NEW_KEYS = ('pose_t', 'pose_img_t', 'com3D_t', 'lead', 'align')
LAG = 0.004                                                              # source c is stamped c * 4 ms before source 0


def _lagging(i, C):
    """Tick i at 30 Hz: source c's frame was taken c * LAG before source 0's; `now` (left to its default) is source 0's stamp."""
    return [i / 30. - c * LAG for c in range(C)]


def _when(mt, stamps, fresh, now=None):
    return ops.tick_stamps(stamps, now, fresh, mt.C)


class _Aligned(object):
    """The restatements fed with what a timed tracker downloads: per tick the poses, centres and statuses (a track's sample is valid iff
    its reported status is OK) and the tick's stamps; with `smooth`, dpp_pose_smooth_t's as well."""

    def __init__(self, mt, smooth=None):
        self.mt = mt
        self.state = A.AlignState(mt.T, mt.J)
        G = 0 if mt.rig is None else mt.rig.G
        self.par = None if smooth is None else dict((k, v) for k, v in dict(dict(dcutoff=1., max_hold=0), **smooth).items() if k != 'rate')
        self.sstate = A.SmoothState(mt.T + G, mt.J)

    def check(self, res, when, where, fused=None):
        mt = self.mt
        want = A.align(np.stack([r['pose'] for r in res]), np.stack([r['com3D'] for r in res]), [r['status'] for r in res], mt.src_host,
                       mt.cams, when, self.state, *mt.timing)
        for t, r in enumerate(res):
            assert r['align'] == want['astat'][t], (where, t, r['align'], want['astat'][t])
            assert r['lead'].tobytes() == want['lead'][t].tobytes() and r['com3D_t'].tobytes() == want['com3d_t'][t].tobytes(), (where, t)
            assert r['pose_t'].tobytes() == want['pose_t'][t].tobytes() and r['pose_img_t'].tobytes() == want['pose_img_t'][t].tobytes(), (where, t)
        if self.par is not None:
            fp, n = (np.stack([f['pose'] for f in fused]), [f['n'] for f in fused]) if fused else (None, None)
            sm = A.smooth_t(np.stack([r['pose'] for r in res]), [r['status'] for r in res], mt.src_host, mt.cams, fp, n, self.sstate, when,
                            **self.par)
            for t, r in enumerate(res):
                assert r['smooth'] == sm['sstat'][t] and r['pose_f'].tobytes() == sm['pose_f'][t].tobytes(), (where, t)
                assert r['pose_img_f'].tobytes() == sm['pose_img_f'][t].tobytes(), (where, t)
            for g, f in enumerate(fused or []):
                assert f['smooth'] == sm['gstat'][g] and f['pose_f'].tobytes() == sm['fused_pose_f'][g].tobytes(), (where, g)
        return want

    def device_state_matches(self):
        mt = self.mt
        mt.rt.synchronize()
        have = mt.astate.have.get()
        assert have.tolist() == self.state.have.tolist()
        for k in ('pt', 'pp', 'pc'):
            got = getattr(mt.astate, k).get()
            assert got[have != 0].tobytes() == getattr(self.state, k)[have != 0].tobytes(), k


def _at_now(res):
    """The per-track results as the launches that combine tracks see them: the aligned pose and centre in place of the unaligned."""
    return [dict(r, pose=r['pose_t'], com3D=r['com3D_t']) for r in res]


@pytest.mark.parametrize('backend,size', SETUPS)
def test_timed_tracker_keeps_every_old_key_and_adds_the_restatement(backend, size):
    """A grouped, smoothing tracker with and without `timing` over 4 ticks (the working-size GPU case: 3) of lagging sources.  The new
    keys are dpp_pose_align's restatement fed with the downloaded pose / com3D / status; `fused`, peer_com and the fusion's flags are
    tests.fuse_ref fed with pose_t / com3D_t -- they refer to `now`; pose_f and the fused pose_f are dpp_pose_smooth_t's restatement.
    What tracking alone produces does not read the alignment: every pre-existing per-track key and the crop are bit-identical to the
    tracker without `timing` for every track that was never handed its peers' centre (that centre is one at `now`), and for all
    tracks before the first hand-over.  A third tracker whose stamps all equal `now` has the bytes of the tracker without timing in every
    key and in `fused`."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig(size)
    Tn, C = len(tracks), len(sizes)
    on1 = [t for t, (c, _) in enumerate(tracks) if c == 1]
    mt, plain, same = (_tracker(rt, backend, size, smooth=SMOOTH, timing=TIMING), _tracker(rt, backend, size, smooth=SMOOTH),
                       _tracker(rt, backend, size, timing=TIMING))
    unsmoothed = _tracker(rt, backend, size)
    for m in (mt, plain, same, unsmoothed):
        _start(m, starts)
    ref = _Aligned(mt, SMOOTH)
    moved = 0.
    for i in range(4 if size == 'small' else 3):
        fr = ticks[i % len(ticks)]
        stamps = _lagging(i, C)
        res, old = mt.process(fr, return_crop=True, stamps=stamps), plain.process(fr, return_crop=True)
        assert mt.now == stamps[0]
        for t in range(Tn):
            assert set(res[t]) == set(old[t]) | set(NEW_KEYS), (i, t)
            if i < drop or t not in on1:
                for k in OLD_KEYS + ('crop',):
                    assert np.array_equal(res[t][k], old[t][k]), (i, t, k)
        want = ref.check(res, _when(mt, stamps, fr), i, mt.fused)
        _fused_matches_the_restatement(mt, _at_now(res), mt.fused)
        if i == 0:
            assert want['astat'].tolist() == [NOPREV] * Tn
        elif i != drop and i != drop + 1:
            assert want['astat'].tolist() == [MOVED] * Tn
            moved = max(moved, max(np.abs(res[t]['pose_t'] - res[t]['pose']).max() for t in range(Tn) if tracks[t][0] != 0))
        if i == drop:                                                    # LOST and handed on the device: NONE, and its row is kept
            assert all(res[t]['status'] == LOST and res[t]['handed'] and res[t]['align'] == NONE and not res[t]['pose_t'].any() for t in on1)
        if i == drop + 1:                                                # dt = two ticks <= max_gap: moved from the sample before the loss
            assert all(res[t]['status'] == OK and res[t]['align'] == MOVED for t in on1)
        # all stamps equal `now`
        a, b = same.process(fr, return_crop=True, stamps=[i / 30.] * C, now=i / 30.), unsmoothed.process(fr, return_crop=True)
        for t in range(Tn):
            assert all(np.array_equal(a[t][k], b[t][k]) for k in b[t]), (i, t)
            assert a[t]['lead'] == 0 and (a[t]['status'] != OK or a[t]['pose_t'].tobytes() == a[t]['pose'].tobytes())
        for fa, fb in zip(same.fused, unsmoothed.fused):
            assert set(fa) == set(fb) and fa['n'] == fb['n'] and all(fa[k].tobytes() == fb[k].tobytes() for k in ('pose', 'com', 'spread')), i
    assert moved > 1.                                                    # the lag is worth millimetres here
    ref.device_state_matches()


@pytest.mark.parametrize('backend', BACKENDS)
def test_timed_plan_structure_and_counters(backend, monkeypatch):
    """Exactly one more launch than the plan without `timing`, whatever T, C and G are and whichever options are on: pose_align, on the
    main lane, behind pose_finish (behind joint_visibility where the plan has it) and before the launches that combine tracks, which
    receive pose_t / com3D_t in place of pose / com3D; with `smooth` the last launch is dpp_pose_smooth_t on the unaligned pose.  The new
    fields FOLLOW every existing field; the states are no part of the block.  Per tick: the frames and the stamps (and `gate` when it
    changes) go up, one plan runs, one block comes down; a reset is one 4-byte upload more.  timing=None: the block and launches of
    before."""
    from hipdp.multitrack import MultiTracker
    from tests.test_multitrack import _nets
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di = ICVLImporter('../data/ICVL/')
    half = DepthImporter(241.42 / 2, 241.42 / 2, 80., 60.)
    eye = (np.eye(3), np.zeros(3))
    cases = ((2, 2, None, {}), (2, 2, [[0, 1]], dict(smooth=SMOOTH)), (3, 3, [[2, 0, 1]], dict(visibility=VIS)),
             (6, 4, [[0, 1, 2, 3], [4, 5]], dict(smooth=SMOOTH, visibility=VIS)), (2, 2, [[0, 1]], dict(calibrate=dict(anchor=0))))
    for Tn, C, groups, opt in cases:
        tracks = [(t % C, False) for t in range(Tn)]
        (snet, _, _), (pnet, _, _) = _nets(rt, backend, Tn)
        dis = di if C == 2 else [di, half] * (C // 2) + [di] * (C % 2)
        Hs, Ws = (37, 45) if C == 2 else ([37, 48] * (C // 2) + [37] * (C % 2), [45, 64] * (C // 2) + [45] * (C % 2))
        kw = dict(opt) if groups is None else dict(opt, extrinsics=[eye] * C, groups=groups, max_dev=40.)
        if 'calibrate' in opt:
            kw['extrinsics'] = [eye, None]
        plain = MultiTracker(rt, dis, pnet, snet, Hs, Ws, (250., 250., 250.), tracks, **kw)
        none = MultiTracker(rt, dis, pnet, snet, Hs, Ws, (250., 250., 250.), tracks, timing=None, **kw)
        mt = MultiTracker(rt, dis, pnet, snet, Hs, Ws, (250., 250., 250.), tracks, timing=TIMING, **kw)
        J3 = mt.J * 3
        for slot in (0, 1):
            lp, lt = plain.plan(slot).launches(), mt.plan(slot).launches()
            names = [l.name for l in lt]
            at = names.index('pose_align')
            assert len(lt) == len(lp) + 1 and names.count('pose_align') == 1
            rest = lt[:at] + lt[at + 1:]
            assert [l.name.replace('pose_smooth_t', 'pose_smooth') for l in rest] == [l.name for l in lp]
            assert names[at - 1] == ('joint_visibility' if 'visibility' in opt else 'pose_finish')
            assert names[at + 1:] == [n for n in names if n in ('pose_fuse', 'pose_fuse_w', 'extrinsics_accumulate', 'pose_smooth_t')]
            op = lt[at]
            assert (op, False) in [tuple(o) for o in mt.plan(slot).ops] and op.fn is rt.lib.dpp_pose_align
            stamps = mt._stamps2 if slot else mt.stamps
            pose_t, com_t = mt.block.view('pose_t').ptr, mt.block.view('com3D_t').ptr
            assert op.args[:2] == (mt.pose3d.ptr, mt.com3d.ptr) and op.args[4:8] == (Tn, mt.J, stamps.ptr, C) and (op.args[8] is None) == (C == 2)
            assert op.args[14:16] == TIMING_SPEC and op.args[16] == mt.astate.have.ptr and op.args[20] == pose_t and op.args[22] == com_t
            by = dict((l.name, l) for l in lt)
            was = dict((l.name, l) for l in lp)
            for name in ('pose_fuse', 'pose_fuse_w'):
                if name in by:                                           # the pointer swap, and nothing else
                    assert by[name].args[:2] == (pose_t, com_t) and was[name].args[:2] == (plain.pose3d.ptr, plain.com3d.ptr)
                    assert by[name].fn is was[name].fn and len(by[name].args) == len(was[name].args)
            if 'calibrate' in opt:
                assert by['extrinsics_accumulate'].args[0] == pose_t and was['extrinsics_accumulate'].args[0] == plain.pose3d.ptr
            if 'smooth' in opt:
                last = lt[-1]
                assert last.fn is rt.lib.dpp_pose_smooth_t and last.args[0] == mt.pose3d.ptr and last.args[14:16] == (stamps.ptr, C)
                assert last.args[16:20] == (1., 0.007, 1., 2) and last.args[20:22] == (mt.sstate.since.ptr, mt.sstate.tlast.ptr)
                assert lp[-1].fn is rt.lib.dpp_pose_smooth and plain.sstate.tlast is None
            assert [l.name for l in none.plan(slot).launches()] == [l.name for l in lp]
            assert [l.fn for l in none.plan(slot).launches()] == [l.fn for l in lp]
        assert plain.res.size == none.res.size and plain._off == none._off and none.astate is None and none.stamps is None
        assert all(mt._off[k] == plain._off[k] for k in plain._off) and mt._off['pose_t'] == plain.res.size
        assert mt.res.size == plain.res.size + Tn * (2 * J3 + 3 + 2)
        assert [k for k in sorted(mt._off, key=mt._off.get) if k not in plain._off] == ['pose_t', 'pose_img_t', 'com3D_t', 'lead', 'astat']
        st = mt.astate
        assert st.have.get().tolist() == [0] * Tn and st.pp.shape == (Tn, mt.J, 3) and st.pt.dtype == np.float64 and mt.stamps.shape == (C + 1,)
        for b in (st.have, st.pt, st.pp, st.pc, mt.stamps):
            assert not mt.res.ptr <= b.ptr < mt.res.ptr + 4 * mt.res.size
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig('small')
    calls = dict(h2d=[], run=0, d2h=[])
    real_in, real_out, real_run = rt.copy_in, rt.download, ops.Plan.run
    monkeypatch.setattr(rt, 'copy_in', lambda buf, arr: (calls['h2d'].append((buf.ptr, buf.size * buf.dtype.itemsize)), real_in(buf, arr))[1], raising=False)
    monkeypatch.setattr(rt, 'download', lambda buf: (calls['d2h'].append(buf.ptr), real_out(buf))[1], raising=False)
    monkeypatch.setattr(ops.Plan, 'run', lambda self, r: (calls.__setitem__('run', calls['run'] + 1), real_run(self, r))[1])
    mt = _tracker(rt, backend, 'small', smooth=SMOOTH, timing=TIMING)
    calls.update(h2d=[])
    mt.reset(1, starts[1])
    assert calls['h2d'] == [(mt.com.ptr + 12, 12), (mt.sstate.since.ptr + 4, 4), (mt.astate.have.ptr + 4, 4)]
    _start(mt, starts)
    f = [(mt.frames.ptr + 4 * int(o), 4 * h * w) for o, (h, w) in zip(mt.table.host['frame_off'], sizes)]
    when = [(mt.stamps.ptr, 8 * 4)]
    for i, h2d in ((0, f + when + [(mt.gate.ptr, 12)]), (1, f + when), (2, f + when)):
        calls.update(h2d=[], run=0, d2h=[])
        mt.process(ticks[i], stamps=_lagging(i, 3))
        assert calls['h2d'] == h2d and calls['run'] == 1 and calls['d2h'] == [mt.res.ptr], (i, calls)
    calls.update(h2d=[])
    mt.set_hand(2, False)                                                # no flip: tflags only
    assert calls['h2d'] == [(mt.tflags.ptr, 12)]
    calls.update(h2d=[])
    mt.set_hand(2, True)
    assert calls['h2d'] == [(mt.sstate.since.ptr + 8, 4), (mt.astate.have.ptr + 8, 4), (mt.tflags.ptr, 12)]
    monkeypatch.undo()


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_handed_track_keeps_its_row_and_a_reset_clears_it(backend):
    """Source 1's track loses the hand in tick `drop` and is handed its peers' centre ON THE DEVICE: NONE in that tick, and MOVED -- not
    NOPREV -- in the tick after, from the sample before the loss.  The same tracker reset from the host right before a tick is NOPREV
    there: the 4-byte upload cleared its row, and only its row."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig('small')
    mt = _tracker(rt, backend, 'small', timing=TIMING)
    _start(mt, starts)
    ref = _Aligned(mt)
    words = []
    for i in range(5):
        if i == 4:
            mt.reset(1, mt.com_host[1])
            ref.state.have[1] = 0                                        # what the 4-byte upload does
        stamps = _lagging(i, 3)
        res = mt.process(ticks[i % 4], stamps=stamps)
        ref.check(res, _when(mt, stamps, ticks[i % 4]), i)
        words.append([r['align'] for r in res])
    assert [w[1] for w in words] == [NOPREV, NONE, MOVED, MOVED, NOPREV] and drop == 1
    assert [w[0] for w in words] == [w[2] for w in words] == [NOPREV] + [MOVED] * 4
    ref.device_state_matches()


@pytest.mark.parametrize('backend,size', SETUPS)
def test_timed_process_sequence_equals_a_process_loop(backend, size):
    """Both slots append the same launches on the ONE align state and the ONE smooth state, each slot with its own stamps buffer, and the
    ticks are stream-ordered: for every track-tick that is OK or IDLE every key has the loop's bits, `fused_ticks` is the loop's `fused`,
    and the device's align and smooth state are afterwards what the loop left.  The ticks: source 1 loses its tracks in tick `drop`
    (handed over on the device), source 0 idles in tick 3; every second tick names `now` explicitly, behind the latest stamp."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig(size)
    Tn, C = len(tracks), len(sizes)
    frames = [list(fr) for fr in _dropped(size)]
    frames[3][0] = None
    timed = []
    for i, fr in enumerate(frames):
        stamps = [None if f is None else s for f, s in zip(fr, _lagging(i, C))]
        timed.append((fr, stamps, i / 30. + 0.002) if i & 1 else (fr, stamps))
    a, b = _tracker(rt, backend, size, smooth=SMOOTH, timing=TIMING), _tracker(rt, backend, size, smooth=SMOOTH, timing=TIMING)
    _start(a, starts)
    _start(b, starts)
    loop, loop_fused, nows = [], [], []
    for tick in timed:
        loop.append(b.process(tick[0], stamps=tick[1], now=tick[2] if len(tick) == 3 else None))
        loop_fused.append(b.fused)
        nows.append(b.now)
    assert nows[1] == 1 / 30. + 0.002 and nows[2] == 2 / 30. and nows[3] == 3 / 30. + 0.002
    seq = a.process_sequence(iter(timed))
    assert a.now == b.now
    live = 0
    for i, (ts, tl) in enumerate(zip(seq, loop)):
        for t in range(Tn):
            assert ts[t]['status'] == tl[t]['status'] and set(ts[t]) == set(tl[t]), (i, t)
            if ts[t]['status'] != LOST:
                live += 1
                assert all(np.asarray(ts[t][k]).tobytes() == np.asarray(tl[t][k]).tobytes() for k in tl[t]), (i, t)
        for fa, fb in zip(a.fused_ticks[i], loop_fused[i]):
            assert fa['n'] == fb['n'] and fa['smooth'] == fb['smooth'], i
            assert all(fa[k].tobytes() == fb[k].tobytes() for k in ('pose', 'com', 'spread', 'pose_f')), i
    idle = [[r['status'] for r in tick].count(IDLE) for tick in loop]
    assert idle[3] == sum(c == 0 for c, _ in tracks) and sum(idle) == idle[3] and live == len(frames) * Tn - sum(c == 1 for c, _ in tracks)
    assert {r['align'] for r in loop[3] if r['status'] == IDLE} == {NONE} and any(r['align'] == MOVED for tick in loop for r in tick)
    rt.synchronize()
    for st in ('astate', 'sstate'):
        for k in (('have', 'pt', 'pp', 'pc') if st == 'astate' else ('since', 'tlast', 'xh', 'dxh')):
            assert getattr(getattr(a, st), k).get().tobytes() == getattr(getattr(b, st), k).get().tobytes(), (st, k)
    with pytest.raises(ValueError):
        a.process_sequence([frames[0]])                                  # a timed sequence's ticks carry their stamps


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_calibrating_timed_tracker_sums_the_aligned_poses(backend):
    """While a source's extrinsics are pending the tick ends in pose_align, extrinsics_accumulate: the sums are tests.calib_ref fed with
    pose_t, tick after tick -- the pairs refer to one instant."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig('small')
    withheld = [extr[0]] + [None] * (len(extr) - 1)
    mt = _tracker(rt, backend, 'small', extrinsics=withheld, calibrate=dict(anchor=0), timing=TIMING)
    _start(mt, starts)
    assert mt.calibrating and [l.name for l in mt.plan().launches()][-2:] == ['pose_align', 'extrinsics_accumulate']
    ref = _Aligned(mt)
    acc = np.zeros((len(mt.cal_src), ops.CALIB_SLOTS))
    unaligned = acc.copy()
    for i in range(drop + 1):
        stamps = _lagging(i, 3)
        res = mt.process(ticks[i], stamps=stamps)
        ref.check(res, _when(mt, stamps, ticks[i]), i)
        status = [r['status'] for r in res]
        acc = K.accumulate(acc, np.stack([r['pose_t'] for r in res]), status, mt.src_host, mt.rig.extr_host, groups, mt.anchor, mt.cal_src)
        unaligned = K.accumulate(unaligned, np.stack([r['pose'] for r in res]), status, mt.src_host, mt.rig.extr_host, groups, mt.anchor, mt.cal_src)
        rt.synchronize()
        assert mt.acc.get().tobytes() == acc.tobytes(), i
    assert acc.any() and acc.tobytes() != unaligned.tobytes()


@pytest.mark.parametrize('backend', BACKENDS)
def test_timing_is_validated_on_the_host(backend):
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig('small')
    assert ops.timing_spec(dict(max_gap=0.1, max_lead=0)) == (0.1, 0.) and ops.timing_spec(TIMING) == TIMING_SPEC
    inf = float('inf')
    bad = [dict(TIMING, gap=1.), dict(max_gap=0.1), dict(max_lead=0.02), {}, 0.1, [0.1, 0.02], True]
    bad += [dict(TIMING, max_gap=v) for v in (0., -0.1, inf, nan, None, 'x')] + [dict(TIMING, max_lead=v) for v in (-1e-9, inf, nan, None)]
    for b in bad:
        with pytest.raises(ValueError):
            ops.timing_spec(b)
    for b in (dict(TIMING, gap=1.), dict(max_gap=0.1), dict(TIMING, max_gap=0.)):
        with pytest.raises(ValueError):
            _tracker(rt, backend, 'small', grouped=False, timing=b)
    mt, plain = _tracker(rt, backend, 'small', timing=TIMING), _tracker(rt, backend, 'small')
    _start(mt, starts)
    _start(plain, starts)
    for stamps in (None, [0., 0.], [0., None, 0.], [0., nan, 0.], [0., inf, 0.], [0., 'x', 0.]):
        with pytest.raises(ValueError):
            mt.process(ticks[0], stamps=stamps)                          # a source that delivers a frame needs its stamp
    with pytest.raises(ValueError):
        mt.process(ticks[0], stamps=[0., 0., 0.], now=nan)
    with pytest.raises(ValueError):
        plain.process(ticks[0], stamps=[0., 0., 0.])                     # stamps without timing
    with pytest.raises(ValueError):
        plain.process(ticks[0], now=0.)
    assert mt.runs == 0 and plain.runs == 0
    res = mt.process([ticks[0][0], None, ticks[0][2]], stamps=[0.25, None, 0.125])       # an idle source needs none; now: the largest
    assert mt.now == 0.25 and [r['status'] for r in res] == [OK, IDLE, OK] and [r['align'] for r in res] == [NOPREV, NONE, NOPREV]
    assert res[2]['lead'] == np.float32(0.125)
    st = ops.AlignState(rt, 3, 4)
    with pytest.raises(ValueError):                                      # a state of other dimensions than the launch
        ops.pose_align(rt, st.pp, st.pc, st.have, st.have, 4, 4, st.pt, 2, TIMING_SPEC, st, st.pp, st.pp, st.pc, st.pc, st.have, cam=(1., 1., 0., 0., 0))
    with pytest.raises(ValueError):                                      # fewer stamps than sources
        ops.pose_align(rt, st.pp, st.pc, st.have, st.have, 3, 4, st.pt, 3, TIMING_SPEC, st, st.pp, st.pp, st.pc, st.pc, st.have, cam=(1., 1., 0., 0., 0))
    with pytest.raises(ValueError):                                      # stamps on a state without tlast
        sm = ops.SmoothState(rt, 3, 4)
        ops.pose_smooth(rt, st.pp, st.have, 3, 4, ops.smooth_spec(SMOOTH), sm, st.pp, st.pp, st.have, cam=(1., 1., 0., 0., 0), stamps=st.pt, C=2)


# ---- 6: HandTracker -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_hand_tracker_filters_over_its_frames_stamps(backend):
    """dpp_pose_smooth_t at T = 1, G = 0, C = 1 with src NULL, last in every plan; one camera has nothing to align, so the plan is as
    long as the one without timing.  6 frames with uneven stamps through process() and through process_sequence against the restatement,
    the old keys those of a tracker without `smooth`; a repeated stamp is STALE and HELD; timing without smooth raises."""
    from hipdp.tracker import HandTracker
    from oracle import augment as AU
    from tests import track_ref as TR
    from tests.test_realtime import _track_nets
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend)
    di, cam, cube, H, W, n = ICVLImporter('../data/ICVL/'), AU.Camera.icvl(), (250., 250., 250.), 120, 160, 6
    frames, coms = TR.drifting_sequence(np.random.RandomState(32), n, cam, H, W, cube)
    smooth = dict(SMOOTH, max_hold=2)
    tr, counted, plain = (HandTracker(rt, di, pnet, snet, H, W, cube, smooth=smooth, timing=True), HandTracker(rt, di, pnet, snet, H, W, cube, smooth=smooth),
                          HandTracker(rt, di, pnet, snet, H, W, cube))
    assert [l.name for l in tr.plan().launches()][:-1] == [l.name for l in counted.plan().launches()][:-1]
    last = tr.plan().ops[-1][0]
    assert last.fn is rt.lib.dpp_pose_smooth_t and 'pose_align' not in [l.name for l in tr.plan().launches()] and not tr.plan().ops[-1][1]
    assert last.args[2] is None and last.args[3:5] == (1, tr.J) and last.args[7:9] == (0, None) and last.args[14:16] == (tr.stamps[0].ptr, 1)
    assert tr.plan(1).ops[-1][0].args[14] == tr.stamps[1].ptr and tr.res.size == counted.res.size and counted.stamps is None
    cams = [camera_tuple(di)]
    stamps = [0., 0.031, 0.07, 0.1, 0.1, 0.14]                           # frame 4 repeats frame 3's stamp
    par = dict((k, v) for k, v in dict(smooth, dcutoff=1.).items() if k != 'rate')

    def against(results, where):
        state = A.SmoothState(1, tr.J)
        for i, r in enumerate(results):
            want = A.smooth_t(r['pose'][None], [r['status']], None, cams, None, None, state, [stamps[i], stamps[i]], **par)
            assert r['smooth'] == want['sstat'][0] and r['pose_f'].tobytes() == want['pose_f'][0].tobytes(), (where, i)
            assert r['pose_img_f'].tobytes() == want['pose_img_f'][0].tobytes(), (where, i)
    tr.reset(coms[0])
    plain.reset(coms[0])
    loop = [tr.process(f, return_crop=True, stamp=s) for f, s in zip(frames, stamps)]
    old = [plain.process(f, return_crop=True) for f in frames]
    for i in range(n):
        assert set(loop[i]) == set(old[i]) | {'pose_f', 'pose_img_f', 'smooth'} and all(np.array_equal(loop[i][k], old[i][k]) for k in old[i]), i
    assert [r['smooth'] for r in loop] == [S_INIT, S_OK, S_OK, S_OK, S_HELD | S_STALE, S_OK]
    assert loop[4]['pose_f'].tobytes() == loop[3]['pose_f'].tobytes()
    against(loop, 'process')
    tr.reset(coms[0])                                                    # clears the row: the sequence starts as the loop did
    seq = tr.process_sequence(list(zip(frames, stamps)))
    for i in range(n):
        assert all(np.array_equal(seq[i][k], loop[i][k]) for k in loop[i] if k != 'crop'), i
    for call in (lambda: tr.process(frames[0]), lambda: tr.process(frames[0], stamp=nan), lambda: tr.process_sequence(frames[:1]),
                 lambda: plain.process(frames[0], stamp=0.), lambda: HandTracker(rt, di, pnet, snet, H, W, cube, timing=True)):
        with pytest.raises(ValueError):
            call()


# ---- 7: the pipelines and the example --------------------------------------------------------------------------------------------------------
def test_file_devices_report_the_stamp_of_the_frame_last_delivered(tmp_path):
    from tests.test_multitrack import _two_icvl_sequences
    from util.cameradevice import CameraDevice, FileDevice, FilteredDevice
    base, di, cube, seqs, _ = _two_icvl_sequences(tmp_path, 3)
    files = seqs[0][2]
    dev = FileDevice(files, di, stamps=[0.5, 0.75, 1.5])
    assert dev.getTimestamp() is None                                    # nothing delivered yet
    seen = []
    for _ in files:
        dev.getDepth()
        seen.append(dev.getTimestamp())
    assert seen == [0.5, 0.75, 1.5] and FileDevice(files, di).getTimestamp() is None and CameraDevice().getTimestamp() is None
    through = FilteredDevice(FileDevice(files, di, stamps=(1, 2, 3)), runtime=object())     # passes it through: nothing is filtered here
    through.device.getDepth()
    assert through.getTimestamp() == 1.
    for bad in ([0., 1.], [0., 1., nan], [0., 1., float('inf')]):
        with pytest.raises(ValueError):
            FileDevice(files, di, stamps=bad)


@pytest.mark.parametrize('backend', BACKENDS)
def test_both_pipelines_pass_timing_through(backend, tmp_path):
    from tests.test_multitrack import _nets, _two_icvl_sequences
    from tests.test_realtime import _track_nets
    from util.cameradevice import FileDevice
    from util.realtimehandposepipeline import MultiStreamPipeline, RealtimeHandposePipeline
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    n = 3
    base, di, cube, seqs, _ = _two_icvl_sequences(tmp_path, n)
    config = {'fx': 241.42, 'fy': 241.42, 'cube': cube}
    cams = [camera_tuple(di)]
    par = dict((k, v) for k, v in dict(SMOOTH, dcutoff=1.).items() if k != 'rate')
    stamps = [0.01, 0.05, 0.08]
    # one hand
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend, J=16)
    rtp = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=seqs[0][1][0], smooth=SMOOTH, timing=True)
    raw = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=seqs[0][1][0])
    poses = rtp.processVideo(FileDevice(seqs[0][2], di, stamps=stamps))
    assert np.array_equal(poses, raw.processVideo(FileDevice(seqs[0][2], di))) and rtp._tracker.timing and not raw._tracker.timing
    state = A.SmoothState(1, 16)
    for i in range(n):
        want = A.smooth_t(poses[i][None], [OK], None, cams, None, None, state, [stamps[i]] * 2, **par)
        assert rtp.poses_f[i].tobytes() == want['pose_f'][0].tobytes(), i
    assert rtp.processFrame(seqs[0][0][0], stamp=0.2)['smooth'] == S_OK
    with pytest.raises(ValueError):
        rtp.processFrame(seqs[0][0][0])                                  # a timed pipeline's frame without its stamp
    with pytest.raises(ValueError):
        RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=seqs[0][1][0], smooth=SMOOTH,
                                 timing=True).processVideo(FileDevice(seqs[0][2], di))       # a device without stamps
    with pytest.raises(ValueError):
        RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, timing=True)
    # two cameras on one sequence, fused; camera 1's frames are stamped 5 ms earlier
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 2, J=16)
    eye = (np.eye(3), np.zeros(3))
    L = MultiStreamPipeline.HAND_LEFT
    s0, s1 = [i / 30. for i in range(n)], [i / 30. - 0.005 for i in range(n)]

    def pipeline(stamped=True, **kw):
        devs = [FileDevice(seqs[0][2], di, stamps=s0 if stamped else None), FileDevice(seqs[0][2], di, stamps=s1 if stamped else None)]
        return MultiStreamPipeline(pnet, dict(config, extrinsics=[eye, eye]), di, devs, [(0, L), (1, L)], snet, init_com=[seqs[0][1][0]] * 2,
                                   groups=[[0, 1]], **kw)
    msp, plain = pipeline(timing=TIMING), pipeline()
    poses, old = msp.processVideos(), plain.processVideos()
    assert all(np.array_equal(a, b) for a, b in zip(poses, old)) and plain.poses_t is None and plain._tracker.timing is None
    assert [p.shape for p in msp.poses_t] == [(n, 16, 3)] * 2 and msp._tracker.now == s0[-1] and msp._tracker.timing == TIMING_SPEC
    state = A.AlignState(2, 16)
    mt = msp._tracker
    for i in range(n):
        # com3D is not recorded by processVideos: the centre's alignment is covered by the tracker tests; the joints are restated here
        want = A.align(np.stack([poses[0][i], poses[1][i]]), np.zeros((2, 3), np.float32), [OK, OK], [0, 1], mt.cams, [s0[i], s1[i], s0[i]],
                       state, *TIMING_SPEC)
        assert all(msp.poses_t[t][i].tobytes() == want['pose_t'][t].tobytes() for t in (0, 1)), i
        assert want['astat'].tolist() == ([MOVED] * 2 if i else [NOPREV] * 2)
    assert np.array_equal(msp.poses_t[0], poses[0]) and not np.array_equal(msp.poses_t[1][1:], poses[1][1:])      # lead 0; 5 ms
    over = pipeline(timing=TIMING)
    over.processVideos(overlapped=True)
    assert all(np.array_equal(a, b) for a, b in zip(over.poses_t, msp.poses_t)) and np.array_equal(over.fused_poses[0], msp.fused_poses[0])
    with pytest.raises(ValueError):
        pipeline(stamped=False, timing=TIMING).processVideos()           # a device without stamps


@pytest.mark.parametrize('backend', BACKENDS)
def test_the_example_prints_the_two_figures_with_stamps_and_nothing_new_without(backend, tmp_path, capsys):
    from tests.test_multitrack import _two_icvl_sequences
    from tests.test_smooth import _driver, _untimed
    R.set_default_runtime(get_runtime(backend))
    base, _, _, _, _ = _two_icvl_sequences(tmp_path, 4)
    net = 'resnet' if backend == 'hip' else 'poseregnet'               # (the 128x128 ResNet is too slow for the SIMT emulator)
    common = ['--dataset', 'icvl', '--data', base, '--net', net, '--cache', str(tmp_path / 'cache'), '--fuse', '--max-frames', '4']
    multi = _driver('realtime_multi')
    capsys.readouterr()
    fused = multi.main(common)
    plain_out = capsys.readouterr().out
    assert 'lagging' not in fused and 'lagging' not in plain_out and 'timing' not in plain_out
    timed = multi.main(common + ['--stamps', '30', '--lag-second', '1'])
    out = capsys.readouterr().out
    fig = timed['lagging']
    assert sorted(fig) == ['timed', 'untimed'] and all(np.isfinite(v) and v >= 0. for v in fig.values())
    assert out.count('camera 1 lagging by 1 frames (sanity figures)') == 1 and 'with timing' in _untimed(out)[-1]
    assert len(_untimed(out)) == len(_untimed(plain_out)) + 1
    sync = multi.main(common + ['--stamps', '30'])                       # no lag: every lead is 0, the fused pose is the plain run's
    capsys.readouterr()
    assert np.array_equal(sync['fused'], fused['fused']) and sync['lagging'] == dict(timed=0., untimed=0.)
    for bad in (['--lag-second', '1'], ['--stamps', '0']):
        with pytest.raises(SystemExit):
            multi.main(common + bad)
