"""Extrinsics of a camera from the tracked hand (csrc/calib.hip: dpp_extrinsics_accumulate, ABI v21; hipdp/calib.py: solve_rigid;
hipdp/multitrack.py `calibrate=`).  The semantics are this project's own -- the reference has one camera -- so the launch is pinned bit
for bit to the NumPy restatement of tests/calib_ref.py, checked for plain geometric sense independently of it, the host solve is checked
against a Kabsch on centred float64 pairs, and then the tracker on top: the calibrating plan, the sums it leaves, the finish, the plan
after it against a tracker constructed with the solved extrinsics, process_sequence, validation, the pipeline class and the example.
Every device test runs on the emulator (CPU tier) and through libdpp_hip.so (-m gpu)."""
import ctypes
import os

import numpy as np
import pytest

from data.importers import ICVLImporter
from hipdp import lib, ops
from hipdp import runtime as R
from hipdp.calib import solve_rigid
from tests import calib_ref as K
from tests import fuse_ref as F
from tests.backends import BACKENDS, get_runtime
from tests.test_fuse import GROUPS7, OLD_KEYS, SETUPS, SRC7, _case, _dropped, _rig, _rotation, _tracker

OK, LOST, IDLE = 0, 1, 2
GROUPS7B = [[3, 6], [0, 2, 5], [1]]            # the second rig: source 1 is fed by two groups (tracks 6 and 2), source 2 by none


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _angle(Ra, Rb):
    """The angle (rad) of the rotation that takes Ra to Rb, from the skew part: accurate near 0, where arccos of the trace is not."""
    D = Ra.T.dot(Rb)
    return float(np.arcsin(min(1., np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2.)))


# ---- 1: the launch alone against the restatement -----------------------------------------------------------------------------------
class _Launcher(object):
    """One accumulator on the device and its restatement on the host, fed by the same launches."""

    def __init__(self, rt, d, groups, anchor, cal):
        self.rt, self.groups, self.anchor, self.cal = rt, groups, anchor, cal
        self.rig = ops.FuseRig(rt, [(e[:9].reshape(3, 3), e[9:]) for e in d['extr']], groups, d['src'], 4)
        self.acc = rt.alloc((len(cal), ops.CALIB_SLOTS), np.float64)
        self.want = np.zeros((len(cal), ops.CALIB_SLOTS))

    def __call__(self, d, max_shape_dev=None):
        rt, T, J = self.rt, len(d['src']), d['J']
        p3, st, sr = rt.upload(d['pose3d']), rt.upload(d['status']), rt.upload(d['src'])
        ops.extrinsics_accumulate(rt, p3, st, sr, T, J, self.rig, self.anchor, self.cal, max_shape_dev, self.acc)(rt.stream)
        rt.synchronize()
        self.want = K.accumulate(self.want, d['pose3d'], d['status'], d['src'], d['extr'], self.groups, self.anchor, self.cal, max_shape_dev)
        got = self.acc.get()
        assert _bits(got, self.want), np.argwhere(got != self.want)
        assert np.array_equal(p3.get(), d['pose3d']) and np.array_equal(st.get(), d['status'])
        assert _bits(self.rig.extr.get(), d['extr'])
        return got


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('J', [5, 70])
def test_accumulator_equals_the_restatement_bit_for_bit(backend, J):
    """T = 7 over C = 4, anchor 0, calibrating 1, 2 and 3.  J = 5: fewer joints than lanes; J = 70: a lane's stride beyond one wave."""
    rt = get_runtime(backend)
    cases = [_case('scalar', SRC7, GROUPS7, J, seed=s) for s in (5, 6, 7)]
    for d in cases[1:]:                                                          # one rig: the other seeds give other poses only
        d['extr'] = cases[0]['extr']
    run =_Launcher(rt, cases[0], GROUPS7, 0, [1, 2, 3])
    # all OK: group 2 = tracks (0, 2, 5) on sources (0, 1, 3) pairs source 1 and source 3 with the anchor; source 2 meets it nowhere
    got = run(cases[0])
    assert got[:, 0].tolist() == [J, 0, J] and got[:, 18].tolist() == [1, 0, 1] and not got[:, 19].any() and not got[1].any()
    # the anchor's member LOST: the whole group sits the launch out
    d = dict(cases[1], status=np.int32([LOST, 0, 0, 0, 0, 0, 0]))
    assert _bits(run(d), got)
    # one member LOST (track 2, source 1): source 3 goes on alone
    d = dict(cases[1], status=np.int32([0, 0, LOST, 0, 0, 0, 0]))
    got = run(d)
    assert got[:, 0].tolist() == [J, 0, 2 * J] and got[:, 18].tolist() == [1, 0, 2]
    # a third launch with other poses, an IDLE member this time (track 5, source 3)
    d = dict(cases[2], status=np.int32([0, 0, 0, 0, 0, IDLE, 0]))
    got = run(d)
    assert got[:, 0].tolist() == [2 * J, 0, 2 * J] and got[:, 18].tolist() == [2, 0, 2] and not got[1].any()
    # the second rig: two groups feed source 1, in ascending group order
    run = _Launcher(rt, cases[0], GROUPS7B, 0, [3, 1])
    got = run(cases[0])
    assert got[:, 0].tolist() == [J, 2 * J] and got[:, 18].tolist() == [1, 2]
    got = run(dict(cases[1], status=np.int32([0, 0, 0, LOST, 0, 0, 0])))       # group 0's anchor member lost: only group 1 adds
    assert got[:, 0].tolist() == [2 * J, 3 * J] and got[:, 18].tolist() == [2, 3]


# ---- 2: the shape gate -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('J', [5, 70])
def test_shape_gate_at_its_bound(backend, J):
    """One pair (tracks 0 and 2 of GROUPS7, calibrating source 1 alone).  Joint 1 of the member is moved 30 mm along the ray from the
    member's centroid: its distance from the centroid no longer matches the anchor's view, and its deviation is the pair's largest.  With
    max_shape_dev = that deviation the pair goes in, with the next float64 towards 0 it is refused."""
    rt = get_runtime(backend)
    d = _case('scalar', SRC7, GROUPS7, J, seed=9)
    p = d['pose3d'][2].astype(np.float64)
    ray = p[1] - p.mean(0)
    d['pose3d'][2, 1] = (p[1] + 30. * ray / np.linalg.norm(ray)).astype(np.float32)
    q = np.array([F.to_world(d['extr'][0], x) for x in d['pose3d'][0]])
    dev = K.shape_deviations(d['pose3d'][2].astype(np.float64), q)
    bound = K.shape_worst(dev)
    # the precondition: the pair's other deviations are far from the bound, so neither case hangs on the last bit of a square root
    assert bound == dev[1] and bound - np.sort(dev)[-2] >= 1e-6 and bound > 20.
    below = np.nextafter(bound, 0.)
    assert below < bound and bound - below < 1e-6
    run = _Launcher(rt, d, GROUPS7, 0, [1])
    got = run(d, max_shape_dev=bound)
    assert got[0, 0] == J and got[0, 18] == 1 and got[0, 19] == 0
    got2 = run(d, max_shape_dev=below)
    assert got2[0, 19] == 1 and _bits(got2[0, :19], got[0, :19])
    off = _Launcher(rt, d, GROUPS7, 0, [1])
    assert _bits(off(d)[0], got[0])                                               # None: no gate, the sums of the accepted case


# ---- 3: geometric sense, independently of the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_one_launch_recovers_the_extrinsics(backend):
    """Four cameras as in tests.test_fuse._case (random rotations, looking at the origin from 500 .. 700 mm) see ONE world skeleton
    (sigma = 40 mm per axis) exactly; the coordinates are rounded to float32 once.  Half a float32 ulp at 512 .. 1024 mm is 3.1e-5 mm:
    over a 40 mm lever that is 7.6e-7 rad, and at 700 mm from the camera 5.6e-4 mm.  The bounds are 13 x and 18 x those."""
    rt = get_runtime(backend)
    rng = np.random.RandomState(41)
    C, J = 4, 21
    extr = np.zeros((C, 12))
    skel = rng.uniform(-60, 60, 3) + rng.normal(0, 40, (J, 3))
    pose3d = np.zeros((C, J, 3), np.float32)
    for c in range(C):
        Rm = _rotation(rng)
        extr[c, :9], extr[c, 9:] = Rm.ravel(), -Rm.dot([rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(500, 700)])
        pose3d[c] = (skel - extr[c, 9:]).dot(Rm)
    src = np.int32([0, 1, 2, 3])
    # the rig knows the anchor's (R, t) only: the other rows hold the identity
    rig = ops.FuseRig(rt, [(extr[0, :9].reshape(3, 3), extr[0, 9:]), None, None, None], [[0, 1, 2, 3]], src, C, anchor=0)
    assert rig.pending == [1, 2, 3]
    acc = rt.alloc((3, ops.CALIB_SLOTS), np.float64)
    ops.extrinsics_accumulate(rt, rt.upload(pose3d), rt.upload(np.zeros(C, np.int32)), rt.upload(src), C, J, rig, 0, [1, 2, 3], None, acc)(rt.stream)
    rt.synchronize()
    for k, row in enumerate(acc.get()):
        r = solve_rigid(row)
        assert r['cond'] >= 0.1, r['cond']                                        # the bounds' precondition
        assert r['ok'] and r['n'] == J and r['pairs'] == 1 and r['refused'] == 0
        Rt, tt = extr[k + 1, :9].reshape(3, 3), extr[k + 1, 9:]
        print("source %d: %.3g rad, %.3g mm, rms %.3g mm, cond %.3f" % (k + 1, _angle(r['R'], Rt), np.linalg.norm(r['t'] - tt), r['rms'], r['cond']))
        assert _angle(r['R'], Rt) <= 1e-5 and np.linalg.norm(r['t'] - tt) <= 1e-2
        assert r['rms'] <= 1e-3                                                    # sqrt(3) half ulps of two views: 1.1e-4 mm


# ---- 4: the host solve ---------------------------------------------------------------------------------------------------------------------
def _row(p, q, pairs=1, refused=0):
    """The accumulator row of the pairs (p, q), summed plainly."""
    return np.concatenate([[len(p)], p.sum(0), q.sum(0), p.T.dot(q).ravel(), [(p * p).sum(), (q * q).sum(), pairs, refused]])


def _kabsch(p, q):
    pc, qc = p - p.mean(0), q - q.mean(0)
    U, s, Vt = np.linalg.svd(pc.T.dot(qc))
    d = np.sign(np.linalg.det(Vt.T.dot(U.T)))
    Rm = Vt.T.dot(np.diag([1., 1., d])).dot(U.T)
    return Rm, q.mean(0) - Rm.dot(p.mean(0)), s


def test_solve_rigid_against_a_kabsch_on_centred_pairs():
    """numpy.linalg.svd on the centred float64 pairs of noisy data (sigma = 2 mm).  Forming S_c from raw sums loses about (600 / 40)^2 =
    2e2 in relative accuracy: 1e-16 * 2e2 = 2e-14 in S_c, and with cond >= 0.1 the rotation moves by less than 1e-12.  R to 1e-9 and t
    (|p| about 600 mm) to 1e-6 mm leave three orders of margin."""
    rng = np.random.RandomState(43)
    n = 63
    Rm = _rotation(rng)
    tv = rng.uniform(-300, 300, 3)
    p = np.float64([0., 0., 600.]) + rng.normal(0, 40, (n, 3))
    q = p.dot(Rm.T) + tv + rng.normal(0, 2, (n, 3))
    r = solve_rigid(_row(p, q, pairs=3, refused=2))
    Rk, tk, s = _kabsch(p, q)
    assert r['ok'] and r['n'] == n and r['pairs'] == 3 and r['refused'] == 2 and r['cond'] >= 0.1
    assert np.abs(r['R'] - Rk).max() <= 1e-9 and np.abs(r['t'] - tk).max() <= 1e-6
    assert abs(r['cond'] - s[1] / s[0]) <= 1e-9
    res = p.dot(Rk.T) + tk - q
    assert abs(r['rms'] - np.sqrt((res ** 2).sum() / n)) <= 1e-6 and 2. < r['rms'] < 5.   # three axes of sigma 2: about 3.4 mm
    assert np.abs(r['R'].T.dot(r['R']) - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(r['R']) - 1.) <= 1e-12
    # min_cond above the data's cond: not ok, the fit is reported all the same
    assert solve_rigid(_row(p, q), min_cond=r['cond'] + 1e-6)['ok'] is False and solve_rigid(_row(p, q), min_cond=r['cond'] - 1e-6)['ok'] is True
    # a mirrored cloud: the best orthogonal map is a reflection, the best ROTATION is returned
    qm = (p * [1., 1., -1.]).dot(Rm.T) + tv + rng.normal(0, 2, (n, 3))
    r = solve_rigid(_row(p, qm))
    Rk, tk, _ = _kabsch(p, qm)
    assert abs(np.linalg.det(r['R']) - 1.) <= 1e-12 and np.abs(r['R'] - Rk).max() <= 1e-9 and r['rms'] > 10.
    # joints on one line: the rotation about the line is open
    line = np.float64([0., 0., 600.]) + np.outer(rng.uniform(-80, 80, n), [0.6, -0.48, 0.64])
    r = solve_rigid(_row(line, line.dot(Rm.T) + tv))
    assert r['ok'] is False and r['cond'] == 0. and r['n'] == n
    # fewer than three pairs, and none at all
    assert solve_rigid(_row(p[:2], q[:2]))['ok'] is False and solve_rigid(_row(p[:3], q[:3]))['n'] == 3
    r = solve_rigid(np.zeros(20))
    assert r['ok'] is False and r['n'] == 0 and np.array_equal(r['R'], np.eye(3)) and not r['t'].any()
    with pytest.raises(ValueError):
        solve_rigid(np.zeros(18))


# ---- 5: the tracker ------------------------------------------------------------------------------------------------------------------------
def _withheld(size):
    extr = _rig(size)[5]
    return [extr[0]] + [None] * (len(extr) - 1)


def _calibrating(rt, backend, size, **cal):
    return _tracker(rt, backend, size, extrinsics=_withheld(size), calibrate=dict(dict(anchor=0), **cal))


def _start(mt, starts):
    for t, c in enumerate(starts):
        mt.reset(t, c)


def _fingerprint(rt, mt):
    from tests.track_plan_fingerprint import _regions, reduce_launches
    plans = [mt.plan(0).launches(), mt.plan(1).launches()]
    return [reduce_launches(rt, p, _regions(mt)) for p in plans]


@pytest.mark.parametrize('backend,size', SETUPS)
def test_tracker_calibrates_and_then_fuses(backend, size):
    """The extrinsics of every source but 0 are withheld.  (a) while calibrating every pre-existing key has the ungrouped tracker's
    bits, nothing is fused, the plan ends in extrinsics_accumulate; (b) the sums are the restatement fed with the per-tick downloaded
    poses and statuses, the tick in which source 1 loses its tracks included; (c) finish_calibration returns solve_rigid of them; (d)
    after it the plan is that of a tracker constructed with the solved extrinsics, and so is the next tick; (f) a finish that is not ok
    changes nothing."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, sizes, cube, tracks, groups, extr, ticks, starts, drop = _rig(size)
    Tn, C = len(tracks), len(dis)
    on1 = [t for t, (c, _) in enumerate(tracks) if c == 1]
    mt, plain = _calibrating(rt, backend, size), _tracker(rt, backend, size, grouped=False)
    strict = _calibrating(rt, backend, size, min_cond=2.)                       # cond = s2 / s1 <= 1: never ok
    assert mt.calibrating and mt.cal_src == list(range(1, C)) and mt.rig.pending == mt.cal_src and mt.acc.shape == (C - 1, 20)
    assert _bits(mt.rig.extr.get()[1:], np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (C - 1, 1)))
    for m in (mt, plain, strict):
        _start(m, starts)
    lp, lc = plain.plan().launches(), mt.plan().launches()                      # (a) the plan
    assert len(lc) == len(lp) + 1 and [l.fn for l in lc[:-1]] == [l.fn for l in lp] and len(mt.plan(1).launches()) == len(lc)
    last, side = mt.plan().ops[-1]
    assert last is lc[-1] and last.fn is rt.lib.dpp_extrinsics_accumulate and not side and last.name == 'extrinsics_accumulate'
    assert rt.lib.dpp_pose_fuse not in [l.fn for l in lc] and mt.res.size == _tracker(rt, backend, size).res.size
    want = np.zeros((C - 1, 20))
    srcs = [c for c, _ in tracks]
    frames = _dropped(size)                                                      # source 1 delivers an all-zero frame in tick `drop`
    for i in range(drop + 1):
        res, ref = mt.process(frames[i], return_crop=True), plain.process(frames[i], return_crop=True)
        strict.process(frames[i])
        assert [r['status'] for r in res] == [LOST if (i == drop and t in on1) else OK for t in range(Tn)]
        for t in range(Tn):
            for k in OLD_KEYS + ('crop',):
                assert np.array_equal(res[t][k], ref[t][k]), (i, t, k)
            assert set(res[t]) == set(ref[t]) | {'group'} and res[t]['group'] == mt.rig.group_of[t]
        assert mt.fused == [] and mt.calibrating
        want = K.accumulate(want, np.stack([r['pose'] for r in res]), [r['status'] for r in res], srcs, mt.rig.extr_host, groups, 0,
                            mt.cal_src, None)
    rt.synchronize()
    got = mt.acc.get()                                                           # (b)
    assert _bits(got, want)
    per_source = [sum(1 for g in groups if {0, c} <= set(srcs[t] for t in g)) for c in mt.cal_src]
    assert got[:, 18].tolist() == [n * (drop if c == 1 else drop + 1) for n, c in zip(per_source, mt.cal_src)]
    assert mt.lost.tolist() == [t in on1 for t in range(Tn)] and mt._detectors == {}
    report = mt.calibration_report()                                             # (c)
    assert sorted(report) == mt.cal_src and mt.calibrating
    for k, c in enumerate(mt.cal_src):
        mine = solve_rigid(want[k])
        assert set(report[c]) == set(mine) == {'R', 't', 'n', 'pairs', 'refused', 'rms', 'cond', 'ok'}
        assert all(_bits(np.float64(report[c][key]), np.float64(mine[key])) for key in mine), (c, report[c], mine)
        assert report[c]['ok'] and report[c]['n'] == mt.J * report[c]['pairs']
    # (f) not ok: the report, and nothing else
    before, plan_before = strict.rig.extr.get(), strict.plan()
    rep = strict.finish_calibration()
    assert not any(r['ok'] for r in rep.values()) and all(_bits(rep[c]['R'], report[c]['R']) for c in rep)
    assert strict.calibrating and strict.plan() is plan_before and _bits(strict.rig.extr.get(), before) and strict.rig.pending == strict.cal_src
    assert _bits(strict.acc.get(), want)
    strict.reset_calibration()
    assert not strict.acc.get().any() and strict.calibrating
    # (d) ok: the tracker constructed with the solved extrinsics
    done = mt.finish_calibration()
    assert not mt.calibrating and mt.rig.pending == [] and all(_bits(done[c]['R'], report[c]['R']) and _bits(done[c]['t'], report[c]['t']) for c in done)
    solved = [extr[0]] + [(done[c]['R'], done[c]['t']) for c in range(1, C)]
    fresh = _tracker(rt, backend, size, extrinsics=solved)
    assert _bits(mt.rig.extr.get(), fresh.rig.extr.get()) and _bits(mt.rig.extr_host, fresh.rig.extr_host)
    assert _fingerprint(rt, mt) == _fingerprint(rt, fresh)
    assert mt.plan().launches()[-1].fn is rt.lib.dpp_pose_fuse
    centres = mt.com_host.copy()
    centres[on1] = starts[on1[0]]                                                # the lost ones start again
    _start(mt, centres)
    _start(fresh, centres)
    nxt, ref = mt.process(ticks[0], return_crop=True), fresh.process(ticks[0], return_crop=True)
    assert [r['status'] for r in nxt] == [OK] * Tn and len(mt.fused) == len(groups)
    for t in range(Tn):
        assert set(nxt[t]) == set(ref[t]) and 'peer_com' in nxt[t]
        for k in nxt[t]:
            assert np.array_equal(nxt[t][k], ref[t][k]), (t, k)
    for fa, fb, g in zip(mt.fused, fresh.fused, groups):
        assert fa['n'] == fb['n'] == len(g) and all(_bits(fa[k], fb[k]) for k in ('pose', 'com', 'spread'))
    with pytest.raises(RuntimeError):
        mt.calibration_report()


@pytest.mark.parametrize('backend,size', SETUPS)
def test_process_sequence_while_calibrating_leaves_the_loops_sums(backend, size):
    """(e) the plan needs no host decision, so the overlapped sequence adds what the process() loop adds."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    tracks, starts, drop = _rig(size)[3], _rig(size)[7], _rig(size)[8]
    frames = _dropped(size)                    # all ticks: source 1's tracks are lost in tick `drop` (the sequence learns it a tick late:
    n = len(frames)                            # they run ungated once more and are LOST there too, so no pair of theirs goes in either way)
    a, b = _calibrating(rt, backend, size), _calibrating(rt, backend, size)
    for mt in (a, b):
        _start(mt, starts)
    loop = [b.process(fr) for fr in frames]
    seq = a.process_sequence(iter(frames))
    want = [[(LOST if i >= drop else OK) if c == 1 else OK for c, _ in tracks] for i in range(n)]
    assert [[r['status'] for r in tick] for tick in seq] == want == [[r['status'] for r in tick] for tick in loop]
    rt.synchronize()
    got = a.acc.get()
    assert _bits(got, b.acc.get()) and a.fused_ticks == [[]] * n and a.calibrating and a.lost.tolist() == b.lost.tolist()
    assert all(got[k, 18] > 0 and got[k, 18] % (drop if c == 1 else n) == 0 for k, c in enumerate(a.cal_src))


# ---- 6: validation ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_calibration_is_validated_on_the_host(backend):
    from hipdp.multitrack import MultiTracker
    from tests.test_multitrack import _nets
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di = ICVLImporter('../data/ICVL/')
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 3)
    tracks = [(0, False), (1, False), (2, False)]
    eye = (np.eye(3), np.zeros(3))

    def make(**kw):
        return MultiTracker(rt, di, pnet, snet, 37, 45, (250., 250., 250.), tracks, **kw)
    ok = make(extrinsics=[eye, None, None], groups=[[0, 1, 2]], calibrate=dict(anchor=0))
    assert ok.calibrating and ok.cal_src == [1, 2] and ok.max_shape_dev is None and ok.min_cond == 0.
    assert make(extrinsics=[None, eye, None], groups=[[2, 1, 0]], calibrate=dict(anchor=1, max_shape_dev=8.)).cal_src == [0, 2]
    full = make(extrinsics=[eye, eye, eye], groups=[[0, 1, 2]], calibrate=dict(anchor=0))     # nothing withheld: the grouped tracker
    assert not full.calibrating and full.acc is None and full.plan().launches()[-1].fn is rt.lib.dpp_pose_fuse
    for bad in (dict(extrinsics=[eye, None, eye], groups=[[0, 1, 2]]),                               # None without calibrate
                dict(extrinsics=[None, eye, eye], groups=[[0, 1, 2]], calibrate=dict(anchor=0)),     # the anchor itself is withheld
                dict(extrinsics=[eye, eye, None], groups=[[0, 1, 2]], calibrate=dict(anchor=3)),
                dict(extrinsics=[eye, eye, None], groups=[[0, 1], [2]], calibrate=dict(anchor=0)),   # source 2 never meets the anchor
                dict(extrinsics=[eye, eye, None], calibrate=dict(anchor=0)),                         # no groups
                dict(extrinsics=[eye, eye, None], groups=[[0, 1, 2]], calibrate=dict(anchor=0, max_shape_dev=0.)),
                dict(extrinsics=[eye, eye, None], groups=[[0, 1, 2]], calibrate=dict(anchor=0, min_cond=-1.)),
                dict(extrinsics=[eye, eye, None], groups=[[0, 1, 2]], calibrate=dict(anchor=0, weights=1))):
        with pytest.raises(ValueError):
            make(**bad)
    with pytest.raises(ValueError, match='chained'):
        make(extrinsics=[eye, eye, None], groups=[[0, 1], [2]], calibrate=dict(anchor=0))
    with pytest.raises(ValueError, match='chained'):                     # source 2 meets the anchor only through source 1
        ops.FuseRig(rt, [eye, None, None], [[0, 1], [2, 3]], [0, 1, 1, 2], 3, anchor=0)
    assert ops.FuseRig(rt, [eye, None, None], [[0, 1], [2, 3]], [0, 1, 0, 2], 3, anchor=0).pending == [1, 2]
    skew = np.eye(3)
    skew[0, 1] = 1e-3
    before = ok.rig.extr.get()
    for Rm, t in ((skew, np.zeros(3)), (np.diag([1., 1., -1.]), np.zeros(3)), (np.eye(3), [0., np.nan, 0.]), (np.eye(2), np.zeros(3))):
        with pytest.raises(ValueError):
            ok.rig.set_extrinsics(1, Rm, t)
    with pytest.raises(IndexError):
        ok.rig.set_extrinsics(3, np.eye(3), np.zeros(3))
    assert _bits(ok.rig.extr.get(), before) and ok.rig.pending == [1, 2]
    Rz = np.diag([-1., -1., 1.])
    ok.rig.set_extrinsics(1, Rz, [1., 2., 3.])
    assert ok.rig.pending == [2] and ok.rig.extr.get()[1].tolist() == Rz.ravel().tolist() + [1., 2., 3.] and _bits(ok.rig.extr.get()[[0, 2]], before[[0, 2]])
    rig = ops.FuseRig(rt, [eye, None], [[0, 1]], [0, 1], 2, anchor=0)
    acc = rt.alloc((1, 20), np.float64)
    for bad in (dict(cal_src=[0]), dict(cal_src=[2]), dict(cal_src=[]), dict(cal_src=[1], anchor=2), dict(cal_src=[1], max_shape_dev=0.)):
        kw = dict(dict(anchor=0, max_shape_dev=None), **bad)
        with pytest.raises(ValueError):
            ops.extrinsics_accumulate(rt, acc, acc, acc, 2, 5, rig, kw['anchor'], kw['cal_src'], kw['max_shape_dev'], acc)


def test_accumulate_entry_point_refuses_bad_arguments_without_a_gpu():
    """Argument validation happens before any launch: callable on the product library without a GPU."""
    import __graft_entry__
    if not os.path.exists(lib.DEFAULT_LIB):
        __graft_entry__.build()
    so = lib.load()
    assert so.dpp_abi_version() == lib.ABI_VERSION >= 21
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    E = 10001

    def call(cal=(1,), **kw):
        a = dict(pose3d=p, status=p, src=p, T=2, J=5, extr=p, C=3, members=p, offsets=p, G=1, anchor=0,
                 cal_src=None if cal is None else (ctypes.c_int * max(1, len(cal)))(*cal), n_cal=0 if cal is None else len(cal), max_shape_dev=0., acc=p)
        a.update(kw)
        return so.dpp_extrinsics_accumulate(*(list(a.values()) + [None]))
    for k in ('pose3d', 'status', 'src', 'extr', 'members', 'offsets', 'acc'):
        assert call(**{k: None}) == E, k
    assert call(cal=None, n_cal=1) == E
    for k in ('T', 'J', 'C', 'G'):
        assert call(**{k: 0}) == E and call(**{k: -1}) == E, k
    assert call(G=3) == E                                                # more groups than tracks
    assert call(anchor=-1) == E and call(anchor=3) == E
    assert call(cal=(0,)) == E and call(cal=(1, 0)) == E                 # the anchor among the sources to calibrate
    assert call(cal=(3,)) == E and call(cal=(-1,)) == E and call(cal=(1, 2, 7)) == E
    assert call(cal=(), n_cal=0) == E and call(cal=(1,) * 33) == E and call(n_cal=-1) == E
    assert call(max_shape_dev=-1.) == E and call(max_shape_dev=float('nan')) == E and call(max_shape_dev=float('inf')) == E


# ---- 7: the class API and the example on top ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_multi_stream_pipeline_calibrates_and_then_fuses(backend, tmp_path):
    """Two FileDevices play ONE sequence through the recorded camera, the second device's extrinsics withheld: the two tracks are one
    track twice, so p = q in every pair, the fit is the identity up to rounding, and the fused pose afterwards is each track's own."""
    from tests.test_multitrack import _nets, _two_icvl_sequences
    from util.cameradevice import FileDevice
    from util.realtimehandposepipeline import MultiStreamPipeline
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    n = 3
    base, di, cube, seqs, _ = _two_icvl_sequences(tmp_path, n)
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 2, J=16)
    eye = (np.eye(3), np.zeros(3))
    L = MultiStreamPipeline.HAND_LEFT
    init = [seqs[0][1][0]] * 2

    def pipeline(extrinsics, **kw):
        config = {'fx': 241.42, 'fy': 241.42, 'cube': cube, 'extrinsics': extrinsics}
        return MultiStreamPipeline(pnet, config, di, [FileDevice(seqs[0][2], di), FileDevice(seqs[0][2], di)], [(0, L), (1, L)], snet,
                                   init_com=init, groups=[[0, 1]], **kw)
    with pytest.raises(ValueError):
        pipeline([eye, None]).processVideos(max_frames=1)                # None needs calibrate=
    msp = pipeline([eye, None], calibrate=dict(anchor=0))
    report = msp.calibrateExtrinsics(2)
    assert sorted(report) == [1] and report[1]['ok'] and report[1]['n'] == 2 * 16 and report[1]['pairs'] == 2 and report[1]['refused'] == 0
    assert np.abs(report[1]['R'] - np.eye(3)).max() <= 1e-9 and np.abs(report[1]['t']).max() <= 1e-6 and report[1]['rms'] <= 1e-6
    assert not msp._tracker.calibrating and msp.fused == [] and msp.config['extrinsics'][1][0] is not None
    res = msp.processFrames(msp._read())                                 # the third frame: fused
    assert [r['status'] for r in res] == [OK, OK] and msp.fused[0]['n'] == 2 and np.array_equal(res[0]['pose'], res[1]['pose'])
    assert np.abs(msp.fused[0]['pose'] - res[0]['pose']).max() <= 1e-3 and msp.fused[0]['spread'].max() <= 1e-3
    with pytest.raises(RuntimeError):
        msp.calibrateExtrinsics(1)                                       # nothing left to calibrate


@pytest.mark.parametrize('backend', BACKENDS)
def test_realtime_multi_example_calibrates_its_second_camera(backend, tmp_path, capsys):
    """examples/realtime_multi.py --fuse --calibrate-extrinsics 3: camera 1's rotation is withheld, three ticks calibrate, one report line
    per calibrated camera is printed, and the run goes on fusing.  The nets are untrained: the figures themselves mean nothing."""
    import importlib.util
    from tests.test_multitrack import ROOT, _two_icvl_sequences
    R.set_default_runtime(get_runtime(backend))
    base, _, _, _, _ = _two_icvl_sequences(tmp_path, 5)
    spec = importlib.util.spec_from_file_location('realtime_multi_driver', os.path.join(ROOT, 'examples', 'realtime_multi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = 'resnet' if backend == 'hip' else 'poseregnet'               # (the 128x128 ResNet is too slow for the SIMT emulator)
    out = mod.main(['--dataset', 'icvl', '--data', base, '--net', net, '--cache', str(tmp_path / 'cache'), '--fuse', '--calibrate-extrinsics', '3'])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('camera 1 after 3 ticks')]
    assert len(lines) == 1 and 'rms' in lines[0] and 'cond' in lines[0]
    cal = out['calibration']
    assert len(cal) == 1 and cal[0]['source'] == 1 and cal[0]['ok'] and cal[0]['n'] == 3 * 16 and cal[0]['pairs'] == 3
    assert all(np.isfinite(cal[0][k]) for k in ('rms', 'cond', 'angle', 'shift'))
    assert out['status'] == [[OK, OK]] * 5 and out['fused'].shape == (2, 16, 3) and np.isfinite(out['fused']).all()
