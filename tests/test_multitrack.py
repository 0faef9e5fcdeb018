"""Several hands and cameras as one device plan (hipdp/multitrack.py; the *_ix entry points of csrc/crop.hip, ABI v16): T tracks over
C frame sources.  The indexed launches against their plain siblings on gathered inputs; MultiTracker against HandTracker (T = C = 1),
against the restatement of tests/track_ref.py (teacher-forced), against itself (a track does not depend on the others, on its row or
on an idle tick), its plan's structure, a sensor, and the pipeline class and example on top.  Every test runs on the emulator (CPU
tier) and through libdpp_hip.so (-m gpu); the GPU tier adds one full-size case (480 x 640, T = 8, C = 4)."""
import functools
import os

import numpy as np
import pytest

from data.importers import ICVLImporter, NYUImporter
from hipdp import ops
from hipdp import runtime as R
from oracle import augment as A
from tests import track_ref as T
from tests.backends import BACKENDS, get_runtime
from tests.test_realtime import REC_BYTES, _oracle_forward, _rec_fields, _records, _sequence, _track_nets, _write_icvl_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('pose', 'pose_img', 'com', 'com3D', 'M', 'status', 'crop')
OK, LOST, IDLE = 0, 1, 2
# (backend, set-up): the small set-up everywhere, the full-size one on the GPU only
SETUPS = [pytest.param('emu', 'small', id='emu'), pytest.param('hip', 'small', marks=pytest.mark.gpu, id='hip'),
          pytest.param('hip', 'large', marks=pytest.mark.gpu, id='hip-480x640')]


def _same(a, b, where, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (where, k)


def _i32(rt, v):
    return rt.upload(np.asarray(v, np.int32))


# ---- 1 / 2: the indexed launches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('camname', ['icvl', 'nyu'])
def test_indexed_launches_equal_their_siblings_on_gathered_frames(backend, camname):
    """Two 37 x 45 frames, three tracks reading frames (1, 0, 1): every *_ix launch on (frames, src) gives the bytes of its sibling on
    frames[src]; then with track 1 gated."""
    rt = get_runtime(backend)
    cam = dict(icvl=A.Camera.icvl(), nyu=A.Camera.nyu())[camname]
    camt = (cam.fx, cam.fy, cam.ux, cam.uy, int(cam.flip_y))
    fx, fy = abs(cam.fx), abs(cam.fy)
    H, W, C, Tn = 37, 45, 2, 3                                         # 37 x 45: not a multiple of 4 pixels, the scalar range path
    rng = np.random.RandomState(11)
    frames = (1400. + rng.normal(0, 3., (C, H, W))).astype(np.float32)    # a far wall, a hand-sized patch of 450 .. 650 mm on it,
    frames[0, 8:30, 5:28] = rng.uniform(450., 650., (22, 23))             # holes, pixels beyond maxDepth and nearer than minDepth
    frames[1, 4:25, 15:40] = rng.uniform(450., 650., (21, 25))
    frames[rng.uniform(size=frames.shape) < 0.05] = 0.
    frames[rng.uniform(size=frames.shape) < 0.02] = 2500.
    frames[1][rng.uniform(size=(H, W)) < 0.02] = 3.
    src = np.int32([1, 0, 1])
    tflags = np.int32([0, 1, 5])
    coms = np.float32([[27., 14., 550.], [16., 19., 540.], [30.5, 11.25, 565.]])
    cubes = np.float32([[250, 250, 250], [300, 300, 300], [233, 241, 287]])
    net_out = np.random.RandomState(12).normal(0, 0.08, (Tn, 3)).astype(np.float32)
    rs, ds = 24, 19
    nrec = int(rt.lib.dpp_crop_record_bytes())
    with pytest.raises(ValueError):
        ops.track_index([0, 2], C)
    with pytest.raises(ValueError):
        ops.track_index([-1, 0], C)
    assert ops.track_index(src, C).dtype == np.int32

    def run(ix, gate):
        """The tracking launches in the plan's order; ix: through the indexed entry points on the C frames, else the plain ones on
        the gathered frames."""
        fr = rt.upload(frames if ix else frames[src])
        nB = C if ix else Tn
        partial = ops.frame_range_workspace(rt, nB)
        ops.frame_range(rt, fr, nB, H, W, partial)(rt.stream)
        co, cu, no = rt.upload(coms), rt.upload(cubes), rt.upload(net_out)
        s, g, tf = _i32(rt, src), _i32(rt, gate), _i32(rt, tflags)
        rec = rt.alloc(Tn * nrec, np.uint8)
        in0, crop = rt.alloc((Tn, rs, rs), zero=False), rt.alloc((Tn, ds, ds), zero=False)
        c3, M, st = rt.alloc((Tn, 3), zero=False), rt.alloc((Tn, 9), zero=False), rt.alloc((Tn,), np.int32)
        out = {}
        if ix:
            ops.crop_prepare_ranged(rt, partial, Tn, co, cu, fx, fy, rs, rec, None, stretch=True, tracks=ops.TrackSet(Tn, s, g))(rt.stream)
            rt.synchronize()
            out['rec0'] = _records(rt, rec, Tn)
            ops.crop_warp(rt, fr, rec, Tn, H, W, rs, in0, normalize=True, nd_value=0.0, tracks=ops.TrackSet(Tn, s))(rt.stream)
            ops.track_refine(rt, fr, rec, Tn, H, W, co, cu, no, camt, fx, fy, ds, co, c3, rec, st, M_out=M, tracks=ops.TrackSet(Tn, s, g))(rt.stream)
            ops.crop_warp_ex(rt, fr, rec, Tn, H, W, ds, crop, flags=ops.CROP_NORMALIZE, nd_value=0.0, tracks=ops.TrackSet(Tn, s, tflags=tf))(rt.stream)
            rt.synchronize()
            out['crop'] = crop.get()
        else:
            ops.crop_prepare_ranged(rt, partial, Tn, co, cu, fx, fy, rs, rec, None, stretch=True)(rt.stream)
            rt.synchronize()
            out['rec0'] = _records(rt, rec, Tn)
            ops.crop_warp(rt, fr, rec, Tn, H, W, rs, in0, normalize=True, nd_value=0.0)(rt.stream)
            ops.track_refine(rt, fr, rec, Tn, H, W, co, cu, no, camt, fx, fy, ds, co, c3, rec, st, M_out=M)(rt.stream)
            flip = rt.alloc((Tn, ds, ds), zero=False)
            ops.crop_warp_ex(rt, fr, rec, Tn, H, W, ds, crop, flags=ops.CROP_NORMALIZE, nd_value=0.0)(rt.stream)
            ops.crop_warp_ex(rt, fr, rec, Tn, H, W, ds, flip, flags=ops.CROP_NORMALIZE | ops.CROP_FLIP_X, nd_value=0.0)(rt.stream)
            rt.synchronize()
            plain, flipped = crop.get(), flip.get()
            out['crop'] = np.stack([flipped[t] if tflags[t] & ops.POSE_HAND_RIGHT else plain[t] for t in range(Tn)])
        out.update(in0=in0.get(), com=co.get(), com3D=c3.get(), M=M.get(), status=st.get(), rec1=_records(rt, rec, Tn))
        return out

    want, got = run(False, [1, 1, 1]), run(True, [1, 1, 1])
    assert want['rec0'].shape == (Tn, REC_BYTES) and want['status'].tolist() == [0, 0, 0]
    assert _rec_fields(want['rec1'])['cw'].min() > 0 and not np.array_equal(want['crop'][1], want['crop'][1][:, ::-1])
    assert not np.array_equal(want['com'], coms)
    for k in want:
        assert want[k].tobytes() == got[k].tobytes(), k
    gated = run(True, [1, 0, 1])
    for k in want:
        assert want[k][[0, 2]].tobytes() == gated[k][[0, 2]].tobytes(), k
    for k in ('rec0', 'rec1'):
        r = _rec_fields(gated[k])
        for f in ('cw', 'ch', 'szw', 'szh', 'xstart', 'ystart', 'xs', 'ys'):
            assert r[f][1] == 0, (k, f)
        assert r['min_depth'][1] == _rec_fields(want[k])['min_depth'][1] and r['norm_div'][1] == 1.
    assert gated['com'][1].tobytes() == coms[1].tobytes()                # the centre's bytes: untouched
    assert gated['status'].tolist() == [0, IDLE, 0] and IDLE == ops.TRACK_IDLE == 2
    assert np.array_equal(gated['M'][1], np.eye(3, dtype=np.float32).ravel()) and not gated['com3D'][1].any()
    assert not gated['crop'][1].any() and not gated['in0'][1].any()
    # a gated track whose centre is ill-defined is idle, not lost, and keeps even a NaN's bits
    fr = rt.upload(frames)
    partial = ops.frame_range_workspace(rt, C)
    ops.frame_range(rt, fr, C, H, W, partial)(rt.stream)
    bad = coms.copy()
    bad[1] = (np.nan, 3., 0.)
    co, cu, no = rt.upload(bad), rt.upload(cubes), rt.upload(net_out)
    s, g = _i32(rt, src), _i32(rt, [1, 0, 1])
    rec, c3, st = rt.alloc(Tn * nrec, np.uint8), rt.alloc((Tn, 3), zero=False), rt.alloc((Tn,), np.int32)
    ops.crop_prepare_ranged(rt, partial, Tn, co, cu, fx, fy, rs, rec, None, stretch=True, tracks=ops.TrackSet(Tn, s, g))(rt.stream)
    ops.track_refine(rt, fr, rec, Tn, H, W, co, cu, no, camt, fx, fy, ds, co, c3, rec, st, tracks=ops.TrackSet(Tn, s, g))(rt.stream)
    rt.synchronize()
    assert st.get().tolist() == [0, IDLE, 0] and co.get()[1].tobytes() == bad[1].tobytes()
    # the entry points refuse missing index arrays and the per-track flag as a launch flag
    assert rt.lib.dpp_crop_warp_ex_ix(fr.ptr, rec.ptr, Tn, s.ptr, g.ptr, H, W, ds, ops.CROP_FLIP_X, 0., 0., 0., c3.ptr, None) != 0
    assert rt.lib.dpp_crop_warp_ix(fr.ptr, rec.ptr, Tn, None, H, W, ds, 1, 0., c3.ptr, None) != 0
    assert rt.lib.dpp_crop_prepare_ranged_ix(partial.ptr, Tn, s.ptr, None, co.ptr, cu.ptr, fx, fy, rs, 1, rec.ptr, None, None) != 0


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('camname', ['icvl', 'nyu'])
def test_pose_finish_ix_carries_all_flag_values_in_one_launch(backend, camname):
    rt = get_runtime(backend)
    cam = dict(icvl=A.Camera.icvl(), nyu=A.Camera.nyu())[camname]
    camt = (cam.fx, cam.fy, cam.ux, cam.uy, int(cam.flip_y))
    Tn, J = 8, 14
    rng = np.random.RandomState(8)
    net_out = rng.normal(0, 0.4, (Tn, J, 3)).astype(np.float32)
    cubes = (np.float32([250, 250, 250]) + rng.uniform(0, 60, (Tn, 3))).astype(np.float32)
    com3d = (np.float32([10., -40., 500.]) + rng.normal(0, 50, (Tn, 3))).astype(np.float32)
    no, cu, c3 = rt.upload(net_out), rt.upload(cubes), rt.upload(com3d)
    p3, pi = rt.alloc((Tn, J, 3), zero=False), rt.alloc((Tn, J, 3), zero=False)
    q3, qi = rt.alloc((Tn, J, 3), zero=False), rt.alloc((Tn, J, 3), zero=False)
    for perm in (np.arange(8), np.int32([5, 2, 7, 0, 3, 6, 1, 4])):
        ops.pose_finish(rt, no, Tn, J, cu, c3, camt, None, p3, pi, tracks=ops.TrackSet(Tn, tflags=_i32(rt, perm)))(rt.stream)
        rt.synchronize()
        got3, goti = p3.get(), pi.get()
        for t in range(Tn):
            ops.pose_finish(rt, no, Tn, J, cu, c3, camt, int(perm[t]), q3, qi)(rt.stream)
            rt.synchronize()
            assert got3[t].tobytes() == q3.get()[t].tobytes() and goti[t].tobytes() == qi.get()[t].tobytes(), (perm, t)
            hand, invX, invY = perm[t] & 1, bool(perm[t] & 2), bool(perm[t] & 4)
            assert np.array_equal(got3[t], T.denormalize(T.pose_signs(net_out[t], hand, invX, invY), cubes[t, 2], com3d[t]))
    assert rt.lib.dpp_pose_finish_ix(no.ptr, Tn, J, None, cu.ptr, c3.ptr, 1., 1., 0., 0., 0, p3.ptr, pi.ptr, None) != 0


# ---- the tracker --------------------------------------------------------------------------------------------------------------------
_nets_cache = {}


def _nets(rt, backend, Tn, zero_refine=False, J=14):
    """ScaleNet and a pose net at batch Tn with the weights of tests.test_realtime._track_nets (the seeds are the same): a small
    PoseRegNet on the emulator, the 128 x 128 ResNet on the GPU.  Built once per (backend, Tn, zero_refine, J)."""
    key = (backend, Tn, zero_refine, J)
    if key not in _nets_cache:
        if Tn == 1:
            _nets_cache[key] = _track_nets(rt, backend, J=J, zero_refine=zero_refine)
        else:
            from tests.test_engine import make_net
            from tests.test_poseregnet import make as make_poseregnet
            from tests.test_scalenet import make as make_scalenet
            snet, sonet, sP = make_scalenet(rt, Tn)
            if zero_refine:
                Wl, b = snet.layers[-1].params
                Wl.set_value(np.zeros_like(Wl.get_value()))
                b.set_value(np.float32([0., 0., -2.]))
            pnet, ponet, pP = make_net(rt, 1, Tn, 128, J, 3, calib_batch=1) if backend == 'hip' else make_poseregnet(rt, 0, Tn, 128, J, 3)
            snet.setDeterministic()
            pnet.setDeterministic()
            _nets_cache[key] = ((snet, sonet, sP), (pnet, ponet, pP))
    return _nets_cache[key]


@functools.lru_cache(maxsize=None)
def _setup(size):
    """(importer, camera, cube, H, W, ticks, tracks, sequences): `small` is T = 3 over C = 2 -- tracks 0 and 1 the left- and right-hand
    views of source 0, track 2 on source 1 -- at 120 x 160, 4 ticks + the starting frame; `large` is T = 8 over C = 4 (src not
    monotone, hands mixed) at 480 x 640 with the NYU camera, 8 ticks."""
    if size == 'small':
        di, cam, cube, H, W, n = ICVLImporter('../data/ICVL/'), A.Camera.icvl(), (250., 250., 250.), 120, 160, 5
        tracks = [(0, False), (0, True), (1, False)]
    else:
        di, cam, cube, H, W, n = NYUImporter('../data/NYU/'), A.Camera.nyu(), (300., 300., 300.), 480, 640, 9
        tracks = [(2, False), (0, True), (1, False), (0, False), (3, True), (3, False), (1, True), (2, True)]
    C = max(s for s, _ in tracks) + 1
    seqs = [T.drifting_sequence(np.random.RandomState(41 + c), n, cam, H, W, cube) for c in range(C)]
    for f, c in seqs:
        f.setflags(write=False)
        c.setflags(write=False)
    return di, cam, cube, H, W, n, tracks, seqs


def _tick(seqs, i):
    return [f[i] for f, _ in seqs]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('hand', [T.HAND_LEFT, T.HAND_RIGHT], ids=['left', 'right'])
def test_one_track_one_source_is_the_hand_tracker(backend, hand):
    """T = C = 1 on the same batch-one nets: every key of every frame has HandTracker's bits."""
    from hipdp.multitrack import MultiTracker
    from hipdp.tracker import HandTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 1)
    di, cam, cube, H, W, n = _sequence('emu')[0]
    frames, coms = T.drifting_sequence(np.random.RandomState(32), n, cam, H, W, cube)
    right = hand == T.HAND_RIGHT
    tr = HandTracker(rt, di, pnet, snet, H, W, cube, hand_right=right, invX=True)
    tr.reset(coms[0])
    want = [tr.process(f, return_crop=True) for f in frames]
    mt = MultiTracker(rt, di, pnet, snet, H, W, cube, [(0, right)], invX=True)
    mt.reset(0, coms[0])
    for i, f in enumerate(frames):
        got = mt.process([f], return_crop=True)
        assert len(got) == 1 and got[0]['status'] == OK
        _same(got[0], want[i], i)
    assert mt.runs == n and len(mt.plan().launches()) == len(tr.plan(0).launches())
    with pytest.raises(ValueError, match="batch of 3"):
        MultiTracker(rt, di, pnet, snet, H, W, cube, [(0, False), (0, True), (1, False)])
    with pytest.raises(ValueError):
        MultiTracker(rt, di, pnet, snet, H, W, cube, [(0, False)], sources=2)            # a source nobody reads
    with pytest.raises(ValueError):
        mt.process([frames[0], frames[1]])
    with pytest.raises(ValueError):
        mt.reset(0, (10., 10., 0.))


@pytest.mark.parametrize('backend,size', SETUPS)
def test_tracks_match_restatement_teacher_forced(backend, size):
    """test_tracker_stages_match_restatement_teacher_forced for every track of one plan, with its assertions and bars: the net inputs
    and the final crop exact, the centre to 2e-4, the pose within 1e-3 mm of the float64 oracle net, pose_img exact."""
    from hipdp.multitrack import MultiTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di, cam, cube, H, W, n, tracks, seqs = _setup(size)
    Tn = len(tracks)
    (snet, sonet, sP), (pnet, ponet, pP) = _nets(rt, backend, Tn)
    sfwd, pfwd = _oracle_forward(sonet, sP), _oracle_forward(ponet, pP)
    fx, fy = abs(cam.fx), abs(cam.fy)
    mt = MultiTracker(rt, di, pnet, snet, H, W, cube, tracks)
    pre = {}
    for i in range(1, n):
        for t, (c, _) in enumerate(tracks):
            mt.reset(t, seqs[c][1][i - 1])                            # teacher: the previous frame's true centre
        res = mt.process(_tick(seqs, i), return_crop=True)
        x_ins = [b.buf.get() for b in mt.ceng.x_ins]
        oracle_pose = size == 'small' or i in (1, n - 1)              # (the float64 ResNet takes a second per crop)
        for t, (c, right) in enumerate(tracks):
            r, com0 = res[t], seqs[c][1][i - 1]
            assert r['status'] == OK
            if (c, i) not in pre:                                     # the restatement of a source's tick, shared by its tracks
                d, lo, hi = A.detector_preprocess(seqs[c][0][i])
                pre[(c, i)] = (d,) + T.track(d, com0, cube, cam, fx, fy, sfwd)[:2]
            d, c_ref, rz = pre[(c, i)]
            ins = T.refine_inputs(rz, cube, com0)
            for x, a in zip(x_ins, ins):                              # what the refinement net sees in row t: exact
                assert np.array_equal(x.reshape((Tn,) + a.shape[1:])[t], a[0]), (i, t)
            np.testing.assert_allclose(r['com'], c_ref, rtol=0, atol=2e-4)
            crop, M, com3D, _ = T.detect_tail(d, r['com'], cube, cam, fx, fy, (128, 128))
            hand = T.HAND_RIGHT if right else T.HAND_LEFT
            want = T.pose_input(crop, hand)[0, 0]
            assert np.array_equal(r['crop'], want), (i, t)            # the final crop around the device's own centre: exact
            np.testing.assert_allclose(r['M'], M, rtol=1e-6, atol=1e-4)
            assert np.array_equal(r['com3D'], com3D)
            if oracle_pose:
                o = pfwd(want[None, None])[0].reshape(-1, 3).copy()
                if right:
                    o[:, 0] *= -1.
                pose64 = o * cube[2] / 2. + com3D.astype(np.float64)
                assert np.abs(r['pose'] - pose64).max() < 1e-3
            assert np.array_equal(r['pose_img'], cam.joints3DToImg(r['pose']))
        if size == 'small':                                           # the two views of source 0: one centre, mirrored crops
            assert np.array_equal(res[0]['com'], res[1]['com']) and np.array_equal(res[0]['crop'], res[1]['crop'][:, ::-1])


def _free_run(mt, tracks, seqs, n, started, order=None):
    """reset the tracks of `started` to their sources' first centres and run ticks 1 .. n - 1; results[tick][track]."""
    order = list(range(len(tracks))) if order is None else order
    for row, t in enumerate(order):
        if t in started:
            mt.reset(row, seqs[tracks[t][0]][1][0])
    return [mt.process(_tick(seqs, i), return_crop=True) for i in range(1, n)]


@pytest.mark.parametrize('backend,size', SETUPS)
def test_a_track_does_not_depend_on_the_other_tracks(backend, size):
    """Free-running: track t's results with all tracks running, with only t un-gated, and with the tracks in another order."""
    from hipdp.multitrack import MultiTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di, cam, cube, H, W, n, tracks, seqs = _setup(size)
    Tn = len(tracks)
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, Tn)
    full = _free_run(MultiTracker(rt, di, pnet, snet, H, W, cube, tracks), tracks, seqs, n, set(range(Tn)))
    assert all(r['status'] == OK for tick in full for r in tick)
    assert not np.array_equal(full[0][0]['com'], full[-1][0]['com'])
    for t in (range(Tn) if size == 'small' else (1, 6)):
        alone = _free_run(MultiTracker(rt, di, pnet, snet, H, W, cube, tracks), tracks, seqs, n, {t})
        for i in range(n - 1):
            _same(alone[i][t], full[i][t], ('alone', t, i))
            assert all(alone[i][u]['status'] == LOST for u in range(Tn) if u != t)          # never started: refused
    order = [2, 0, 1] if Tn == 3 else [5, 2, 7, 0, 3, 6, 1, 4]
    perm = _free_run(MultiTracker(rt, di, pnet, snet, H, W, cube, [tracks[t] for t in order]), tracks, seqs, n, set(range(Tn)), order)
    for row, t in enumerate(order):
        for i in range(n - 1):
            _same(perm[i][row], full[i][t], ('permuted', t, i))


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_lost_track_does_not_stop_the_others(backend):
    """The refinement net that answers (0, 0, -2): from 300 mm with a 300 mm cube a track is lost on its first tick, from 700 mm it
    goes on (700 -> 400 -> 100 -> ...)."""
    from hipdp.multitrack import MultiTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di, cam, _, H, W, n, _, seqs = _setup('small')
    cube = (300., 300., 300.)
    frames = seqs[0][0]
    (snet2, _, _), (pnet2, _, _) = _nets(rt, backend, 2, zero_refine=True)
    (snet1, _, _), (pnet1, _, _) = _nets(rt, backend, 1, zero_refine=True)
    near, far = (75., 55., 300.), (75., 55., 700.)
    mt = MultiTracker(rt, di, pnet2, snet2, H, W, cube, [(0, False), (0, False)])
    mt.reset(0, near)
    mt.reset(1, far)
    a = mt.process([frames[0]], return_crop=True)
    assert a[0]['status'] == LOST and a[0]['com'][2] == 0. and not a[0]['crop'].any()
    assert a[1]['status'] == OK and a[1]['com'][2] == 400.
    for k in KEYS:
        assert np.isfinite(a[0][k]).all(), k
    one = MultiTracker(rt, di, pnet1, snet1, H, W, cube, [(0, False)])          # a tracker that holds only the surviving track
    one.reset(0, far)
    _same(one.process([frames[0]], return_crop=True)[0], a[1], 'alone')
    b = mt.process([frames[1]], return_crop=True)
    assert b[0]['status'] == LOST and b[1]['status'] == OK and b[1]['com'][2] == 100.
    assert b[0]['com'].tobytes() == a[0]['com'].tobytes()                       # refused: gated, its (meaningless) centre as it was
    _same(one.process([frames[1]], return_crop=True)[0], b[1], 'alone, second tick')
    mt.reset(0, far)
    mt.reset(1, far)
    c = mt.process([frames[2]], return_crop=True)
    fresh = MultiTracker(rt, di, pnet2, snet2, H, W, cube, [(0, False), (0, False)])
    fresh.reset(0, far)
    d = fresh.process([frames[2]], return_crop=True)
    assert c[0]['status'] == OK and d[1]['status'] == LOST
    _same(c[0], d[0], 'after reset')
    _same(c[0], c[1], 'two tracks on one hand')


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_source_without_a_frame_idles_its_tracks(backend):
    from hipdp.multitrack import MultiTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di, cam, cube, H, W, n, tracks, seqs = _setup('small')
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 3)

    def run(ticks):
        mt = MultiTracker(rt, di, pnet, snet, H, W, cube, tracks)
        for t, (c, _) in enumerate(tracks):
            mt.reset(t, seqs[c][1][0])
        return [mt.process(fr, return_crop=True) for fr in ticks]
    a1, a2, a3 = _tick(seqs, 1), _tick(seqs, 2), _tick(seqs, 3)
    idle = run([a1, [a2[0], None], a3])
    full = run([a1, a2, a3])
    skipped = run([a1, a3])
    assert [r['status'] for r in idle[1]] == [OK, OK, IDLE]
    assert idle[1][2]['com'].tobytes() == idle[0][2]['com'].tobytes()            # the centre: bit-unchanged
    for i in range(3):
        for t in (0, 1):                                                          # the other source's tracks: unaffected
            _same(idle[i][t], full[i][t], (i, t))
    _same(idle[2][2], skipped[1][2], 'the tick after the idle one')
    assert not np.array_equal(idle[2][2]['com'], full[2][2]['com'])              # (the skipped frame would have moved the centre)
    both = run([a1, [None, None]])
    assert [r['status'] for r in both[1]] == [IDLE] * 3


@pytest.mark.parametrize('backend', BACKENDS)
def test_multitrack_plan_structure(backend, monkeypatch):
    from hipdp.multitrack import MultiTracker
    from hipdp.tracker import HandTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di, cam, cube, H, W, n, _, seqs = _setup('small')
    (snet1, _, _), (pnet1, _, _) = _nets(rt, backend, 1)
    single = len(HandTracker(rt, di, pnet1, snet1, H, W, cube).plan(0).launches())
    for tracks in ([(0, False)], [(0, False), (0, True), (1, False)], [(3, False), (1, True), (0, False), (2, False)]):
        Tn, C = len(tracks), max(s for s, _ in tracks) + 1
        (snet, _, _), (pnet, _, _) = _nets(rt, backend, Tn)
        mt = MultiTracker(rt, di, pnet, snet, H, W, cube, tracks)
        launches = mt.plan().launches()
        assert len(launches) == single, (Tn, C)                       # the launch count of ONE tracker, whatever T and C are
        rng = [l for l in launches if l.fn is rt.lib.dpp_frame_range]
        assert len(rng) == 1 and rng[0].args[1] == C and launches[0] is rng[0]
        fns = [l.fn for l in launches]
        for fn in (rt.lib.dpp_crop_prepare_ranged_ix, rt.lib.dpp_crop_warp_ix, rt.lib.dpp_track_refine_ix, rt.lib.dpp_crop_warp_ex_ix,
                   rt.lib.dpp_pose_finish_ix):
            assert fns.count(fn) == 1
        for fn in (rt.lib.dpp_crop_prepare, rt.lib.dpp_crop_com, rt.lib.dpp_crop_prepare_ranged, rt.lib.dpp_track_refine, rt.lib.dpp_pose_finish):
            assert fn not in fns
    tracks = [(0, False), (0, True), (1, False)]
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 3)
    mt = MultiTracker(rt, di, pnet, snet, H, W, cube, tracks)
    for t, (c, _) in enumerate(tracks):
        mt.reset(t, seqs[c][1][0])
    plan = mt.plan()
    calls = dict(h2d=[], run=0, d2h=[])
    real_in, real_out, real_run = rt.copy_in, rt.download, ops.Plan.run
    monkeypatch.setattr(rt, 'copy_in', lambda buf, arr: (calls['h2d'].append(buf.ptr), real_in(buf, arr))[1], raising=False)
    monkeypatch.setattr(rt, 'download', lambda buf: (calls['d2h'].append(buf.ptr), real_out(buf))[1], raising=False)
    monkeypatch.setattr(ops.Plan, 'run', lambda self, r: (calls.__setitem__('run', calls['run'] + 1), real_run(self, r))[1])
    f0, f1 = mt.frames.ptr, mt.frames.ptr + 4 * H * W

    def tick(frames, h2d):
        calls.update(h2d=[], run=0, d2h=[])
        out = mt.process(frames)
        assert calls['h2d'] == h2d and calls['run'] == 1 and calls['d2h'] == [mt.res.ptr], (calls, h2d)
        return out
    r1 = tick(_tick(seqs, 1), [f0, f1, mt.gate.ptr])                  # the first tick opens the gates: one upload more
    r2 = tick(_tick(seqs, 2), [f0, f1])                               # one upload per fresh source, one plan, one download
    assert not np.array_equal(r1[0]['com'], r2[0]['com'])
    r3 = tick([None, seqs[1][0][3]], [f1, mt.gate.ptr])               # source 0 idles: the gates change
    assert [r['status'] for r in r3] == [IDLE, IDLE, OK]
    tick([None, seqs[1][0][4]], [f1])                                 # ... and stay as they are
    calls['h2d'] = []
    mt.set_hand(0, True)                                              # data, not a launch argument: the same plan
    assert calls['h2d'] == [mt.tflags.ptr] and mt.plan() is plan and len(plan.launches()) == single
    r5 = tick(_tick(seqs, 4), [f0, f1, mt.gate.ptr])
    _same(r5[0], r5[1], 'both tracks of source 0 are right hands now', keys=KEYS[:-1])
    monkeypatch.undo()
    with pytest.raises(ValueError):
        mt.process([seqs[0][0][0][:10], None])
    with pytest.raises(IndexError):
        mt.reset(3, seqs[0][1][0])


@pytest.mark.parametrize('backend', BACKENDS)
def test_sensor_frames_for_all_sources(backend):
    """Raw uint16 frames, mirrored and median-filtered on the device at B = C, against the float32 tracker fed filter_depth of the same
    raw frames."""
    from hipdp.multitrack import MultiTracker
    from util.cameradevice import filter_depth
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di, cam, cube, H, W, n, tracks, seqs = _setup('small')
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 3)
    raws = []
    for c, (f, _) in enumerate(seqs):
        raw = np.rint(f).astype(np.uint16)
        u = np.random.RandomState(50 + c).uniform(size=raw.shape)
        raw[u < 0.01] = 0
        raw[(u >= 0.01) & (u < 0.02)] = 3000
        raws.append(raw)
    filtered = [filter_depth(raw, median=True, mirror=True, runtime=rt) for raw in raws]
    assert filtered[0].dtype == np.float32 and (filtered[0] != raws[0][:, :, ::-1]).mean() > 0.005
    a = MultiTracker(rt, di, pnet, snet, H, W, cube, tracks)
    b = MultiTracker(rt, di, pnet, snet, H, W, cube, tracks, sensor=dict(dtype='uint16', median=True, mirror=True))
    for t, (c, _) in enumerate(tracks):
        c0 = seqs[c][1][0] * np.float32([-1., 1., 1.]) + np.float32([W - 1., 0., 0.])
        a.reset(t, c0)
        b.reset(t, c0)
    for i in range(1, n):
        ra = a.process([f[i] for f in filtered], return_crop=True)
        rb = b.process([r[i] for r in raws], return_crop=True)
        for t in range(3):
            assert ra[t]['status'] == OK
            _same(ra[t], rb[t], (i, t))
    assert np.array_equal(b.frames.get()[1], filtered[1][n - 1])
    with pytest.raises(ValueError):
        b.process([f[1] for f in filtered])                           # a raw frame is taken as it is or not at all


@pytest.mark.parametrize('backend', BACKENDS)
def test_acquire_seeds_a_track_from_its_source(backend):
    """acquire(t, frame) is HandTracker.acquire on track t's views: the same centre, and the same first tick after it."""
    from hipdp.multitrack import MultiTracker
    from hipdp.tracker import HandTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di, cam, cube, H, W, n, tracks, seqs = _setup('small')
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 3)
    (snet1, _, _), (pnet1, _, _) = _nets(rt, backend, 1)
    mt = MultiTracker(rt, di, pnet, snet, H, W, cube, tracks)
    tr = HandTracker(rt, di, pnet1, snet1, H, W, cube)
    got, want = mt.acquire(2, seqs[1][0][0]), tr.acquire(seqs[1][0][0])
    assert got['found'] and want['found'] and np.array_equal(got['com'], want['com']) and np.array_equal(got['cube'], want['cube'])
    res = mt.process(_tick(seqs, 1))
    assert [r['status'] for r in res] == [LOST, LOST, OK]
    assert np.array_equal(res[2]['com'], tr.process(seqs[1][0][1])['com'])
    assert not mt.acquire(0, np.zeros((H, W), np.float32))['found'] and mt.lost[0]


# ---- 9: the class API on top --------------------------------------------------------------------------------------------------------
def _two_icvl_sequences(tmp_path, n):
    from util.cameradevice import FileDevice
    cam, cube = A.Camera.icvl(), (250, 250, 250)
    base = str(tmp_path / 'ICVL')
    out = []
    for k, name in enumerate(('test_seq_1', 'test_seq_2')):
        frames, coms = T.drifting_sequence(np.random.RandomState(61 + k), n, cam, 240, 320, tuple(float(c) for c in cube))
        frames, _ = _write_icvl_sequence(base, name, frames, coms, cam, seed=3 + k)
        out.append((frames, coms, [os.path.join(base, 'Depth', '201403121135', '%s_%04d.png' % (name, i)) for i in range(n)]))
    return base, ICVLImporter(base, useCache=False), cube, out, FileDevice


@pytest.mark.parametrize('backend', BACKENDS)
def test_multi_stream_pipeline_on_two_file_sequences(backend, tmp_path):
    from hipdp.multitrack import MultiTracker
    from util.realtimehandposepipeline import MultiStreamPipeline
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    n = 3
    base, di, cube, seqs, FileDevice = _two_icvl_sequences(tmp_path, n)
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 3, J=16)
    config = {'fx': 241.42, 'fy': 241.42, 'cube': cube}
    L, Rr = MultiStreamPipeline.HAND_LEFT, MultiStreamPipeline.HAND_RIGHT
    hands = [(0, L), (0, Rr), (1, L)]
    init = [seqs[d][1][0] for d, _ in hands]
    msp = MultiStreamPipeline(pnet, dict(config), di, [FileDevice(s[2], di) for s in seqs], hands, snet, init_com=init)
    poses = msp.processVideos()
    assert len(poses) == 3 and all(p.shape == (n, 16, 3) and p.dtype == np.float32 and np.isfinite(p).all() for p in poses)
    assert len(msp.frame_times) == n
    # ... the poses of the tracker underneath, fed the same frames
    mt = MultiTracker(rt, di, pnet, snet, 240, 320, cube, [(d, h == Rr) for d, h in hands], fx=config['fx'], fy=config['fy'])
    for t in range(3):
        mt.reset(t, init[t])
    for i in range(n):
        res = mt.process([seqs[0][0][i], seqs[1][0][i]])
        for t in range(3):
            assert np.array_equal(res[t]['pose'], poses[t][i]), (i, t)
    # max_frames; seed_detect acquires the track that is alone on its device, and acquires it again after it is lost
    msp = MultiStreamPipeline(pnet, dict(config), di, [FileDevice(s[2], di) for s in seqs], hands, snet, init_com=init[:2] + [None],
                              seed_detect=True)
    p2 = msp.processVideos(max_frames=2)
    assert [p.shape for p in p2] == [(2, 16, 3)] * 3 and np.array_equal(p2[0], poses[0][:2])
    msp._tracker.lost[2] = True
    assert [r['status'] for r in msp.processFrames([seqs[0][0][2], seqs[1][0][2]])] == [OK, OK, OK]
    with pytest.raises(ValueError):
        MultiStreamPipeline(pnet, dict(config), di, [FileDevice(s[2], di) for s in seqs], hands, snet, init_com=init[:2] + [None])
    with pytest.raises(ValueError):
        MultiStreamPipeline(pnet, dict(config), di, [FileDevice(s[2], di) for s in seqs], hands[:2], snet, init_com=init[:2])


@pytest.mark.parametrize('backend', BACKENDS)
def test_realtime_multi_example_runs_end_to_end(backend, tmp_path):
    import importlib.util
    R.set_default_runtime(get_runtime(backend))
    base, _, _, _, _ = _two_icvl_sequences(tmp_path, 3)
    spec = importlib.util.spec_from_file_location('realtime_multi_driver', os.path.join(ROOT, 'examples', 'realtime_multi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = 'resnet' if backend == 'hip' else 'poseregnet'               # (the 128x128 ResNet is too slow for the SIMT emulator)
    common = ['--dataset', 'icvl', '--data', base, '--net', net, '--cache', str(tmp_path / 'cache')]
    poses, errs = mod.main(common)
    assert [p.shape for p in poses] == [(3, 16, 3)] * 3 and all(np.isfinite(p).all() for p in poses)
    assert errs[1] is None and np.isfinite(errs[0]) and errs[0] > 0 and np.isfinite(errs[2])
    poses2, _ = mod.main(common + ['--seed', 'detect', '--max-frames', '2'])
    assert [p.shape for p in poses2] == [(2, 16, 3)] * 3 and np.array_equal(poses2[0], poses[0][:2])
