"""Frame sources of unlike cameras and frame sizes in one MultiTracker plan (hipdp/multitrack.py; the *_src entry points of
csrc/crop.hip and csrc/ingest.hip, ABI v19), and MultiTracker.process_sequence.  Every *_src launch against its plain / *_ix sibling
run on one source's frame alone; the tracker over unlike sources against homogeneous trackers that each see one source and against
the restatement of tests/track_ref.py with each track's own camera; all-equal sequences are the homogeneous path; the plan's
structure; a detector per camera; process_sequence against a process() loop; validation.  Every test runs on the emulator (CPU tier)
and through libdpp_hip.so (-m gpu); the GPU tier adds one working-size case (T = 8 over C = 4, 480 x 640 beside 240 x 320)."""
import ctypes
import functools
import os

import numpy as np
import pytest

from data.importers import DepthImporter, ICVLImporter, MSRA15Importer, NYUImporter
from hipdp import lib, ops
from hipdp import runtime as R
from oracle import augment as A
from tests import track_ref as T
from tests.backends import BACKENDS, get_runtime
from tests.test_multitrack import _i32, _nets, _same
from tests.test_realtime import _oracle_forward, _records

OK, LOST, IDLE = 0, 1, 2
SETUPS = [pytest.param('emu', 'small', id='emu'), pytest.param('hip', 'small', marks=pytest.mark.gpu, id='hip'),
          pytest.param('hip', 'large', marks=pytest.mark.gpu, id='hip-480x640+240x320')]


def _camt(cam):
    return (cam.fx, cam.fy, cam.ux, cam.uy, int(cam.flip_y))


def _half(cam):
    return A.Camera(cam.fx * 0.5, cam.fy * 0.5, cam.ux * 0.5, cam.uy * 0.5, cam.flip_y)


# ---- 1: the *_src launches against their siblings ----------------------------------------------------------------------------------
def _launch_case():
    """T = 4 over C = 3: source 0 37 x 45 with the ICVL camera, source 1 48 x 64 (a multiple of 4 pixels: the 16-byte paths) with the
    MSRA15 camera (flip_y), source 2 37 x 45 with the ICVL intrinsics halved; src = (2, 0, 1, 0), track 3 gated."""
    cams = [A.Camera.icvl(), A.Camera.msra(), _half(A.Camera.icvl())]
    sizes = [(37, 45), (48, 64), (37, 45)]
    rng = np.random.RandomState(11)
    frames = []
    for c, (H, W) in enumerate(sizes):
        f = (1400. + rng.normal(0, 3., (H, W))).astype(np.float32)       # a far wall, a hand-sized patch of 450 .. 650 mm, holes,
        f[8:30, 5 + 4 * c:28 + 4 * c] = rng.uniform(450., 650., (22, 23))  # pixels beyond maxDepth and nearer than minDepth
        f[rng.uniform(size=f.shape) < 0.05] = 0.
        f[rng.uniform(size=f.shape) < 0.02] = 2500.
        f[rng.uniform(size=f.shape) < 0.02] = 3.
        frames.append(f)
    src = np.int32([2, 0, 1, 0])
    gate = np.int32([1, 1, 1, 0])
    tflags = np.int32([0, 1, 5, 2])
    coms = np.float32([[27., 14., 550.], [16., 19., 540.], [30.5, 21.25, 565.], [20., 15., 555.]])
    cubes = np.float32([[250, 250, 250], [300, 300, 300], [233, 241, 287], [250, 250, 250]])
    net_out = np.random.RandomState(12).normal(0, 0.08, (4, 3)).astype(np.float32)
    return cams, sizes, frames, src, gate, tflags, coms, cubes, net_out


def _table(rt, cams, sizes, raw_itemsize=None):
    return ops.SourceTable(rt, [_camt(c) for c in cams], [(abs(c.fx), abs(c.fy)) for c in cams], sizes, raw_itemsize)


def _ragged(rt, table, frames, dtype, raw=False):
    """The frames in a ragged buffer whose pad elements are NaN (float32) / 0xFFFF (uint16): a read of padding shows."""
    host = np.full(table.raw_elems if raw else table.frame_elems, np.nan if np.dtype(dtype) == np.float32 else 0xFFFF, dtype)
    for c, f in enumerate(frames):
        off = int(table.host['raw_off' if raw else 'frame_off'][c])
        host[off:off + f.size] = f.ravel()
    return rt.upload(host), host


def _pads(table, host, raw=False):
    keep = np.ones(host.size, bool)
    for c in range(table.C):
        H, W = table.size(c)
        off = int(table.host['raw_off' if raw else 'frame_off'][c])
        keep[off:off + H * W] = False
    return host[keep]


@pytest.mark.parametrize('backend', BACKENDS)
def test_src_launches_equal_their_siblings_on_each_source_alone(backend):
    rt = get_runtime(backend)
    cams, sizes, frames, src, gate, tflags, coms, cubes, net_out = _launch_case()
    Tn, C, rs, ds, J = 4, 3, 24, 19, 5
    nrec = int(rt.lib.dpp_crop_record_bytes())
    table = _table(rt, cams, sizes)
    assert table.host.dtype.itemsize == rt.lib.dpp_source_record_bytes()
    assert table.host['frame_off'].tolist() == [0, 1668, 1668 + 3072] and table.frame_elems == 1668 + 3072 + 1668   # 37 * 45 = 1665
    pose_out = np.random.RandomState(13).normal(0, 0.4, (Tn, J, 3)).astype(np.float32)

    def run(which):
        """The tracking launches in the plan's order.  which None: the *_src launches on the ragged buffer, all tracks; c: the *_ix
        launches (frame_range: the plain one) on source c's frame alone with c's scalars, the rows of c's tracks."""
        if which is None:
            rows = np.arange(Tn)
            fr, _ = _ragged(rt, table, frames, np.float32)
            nC = C
        else:
            rows = np.flatnonzero(src == which)
            fr = rt.upload(frames[which][None])
            nC = 1
            (H, W), cam = sizes[which], cams[which]
            camt, fx, fy = _camt(cam), abs(cam.fx), abs(cam.fy)
        n = len(rows)
        partial = ops.frame_range_workspace(rt, nC)
        co, cu, no, po = rt.upload(coms[rows]), rt.upload(cubes[rows]), rt.upload(net_out[rows]), rt.upload(pose_out[rows])
        s, g, tf = _i32(rt, src[rows] if which is None else np.zeros(n)), _i32(rt, gate[rows]), _i32(rt, tflags[rows])
        rec = rt.alloc(n * nrec, np.uint8)
        in0, crop = rt.alloc((n, rs, rs), zero=False), rt.alloc((n, ds, ds), zero=False)
        c3, M, st = rt.alloc((n, 3), zero=False), rt.alloc((n, 9), zero=False), rt.alloc((n,), np.int32)
        p3, pi = rt.alloc((n, J, 3), zero=False), rt.alloc((n, J, 3), zero=False)
        out = {}
        if which is None:
            ops.frame_range(rt, fr, None, None, None, partial, table=table)(rt.stream)
            ops.crop_prepare_ranged(rt, partial, n, co, cu, None, None, rs, rec, None, stretch=True, tracks=ops.TrackSet(n, s, g, table=table))(rt.stream)
            rt.synchronize()
            out['rec0'] = _records(rt, rec, n)
            ops.crop_warp(rt, fr, rec, n, None, None, rs, in0, normalize=True, nd_value=0.0, tracks=ops.TrackSet(n, s, table=table))(rt.stream)
            ops.track_refine(rt, fr, rec, n, None, None, co, cu, no, None, None, None, ds, co, c3, rec, st, M_out=M,
                             tracks=ops.TrackSet(n, s, g, table=table))(rt.stream)
            ops.crop_warp_ex(rt, fr, rec, n, None, None, ds, crop, flags=ops.CROP_NORMALIZE, nd_value=0.0,
                             tracks=ops.TrackSet(n, s, tflags=tf, table=table))(rt.stream)
            ops.pose_finish(rt, po, n, J, cu, c3, None, None, p3, pi, tracks=ops.TrackSet(n, s, tflags=tf, table=table))(rt.stream)
        else:
            ops.frame_range(rt, fr, 1, H, W, partial)(rt.stream)
            ops.crop_prepare_ranged(rt, partial, n, co, cu, fx, fy, rs, rec, None, stretch=True, tracks=ops.TrackSet(n, s, g))(rt.stream)
            rt.synchronize()
            out['rec0'] = _records(rt, rec, n)
            ops.crop_warp(rt, fr, rec, n, H, W, rs, in0, normalize=True, nd_value=0.0, tracks=ops.TrackSet(n, s))(rt.stream)
            ops.track_refine(rt, fr, rec, n, H, W, co, cu, no, camt, fx, fy, ds, co, c3, rec, st, M_out=M, tracks=ops.TrackSet(n, s, g))(rt.stream)
            ops.crop_warp_ex(rt, fr, rec, n, H, W, ds, crop, flags=ops.CROP_NORMALIZE, nd_value=0.0, tracks=ops.TrackSet(n, s, tflags=tf))(rt.stream)
            ops.pose_finish(rt, po, n, J, cu, c3, camt, None, p3, pi, tracks=ops.TrackSet(n, tflags=tf))(rt.stream)
        rt.synchronize()
        out.update(partial=partial.get().reshape(nC, -1), in0=in0.get(), com=co.get(), com3D=c3.get(), M=M.get(), status=st.get(),
                   rec1=_records(rt, rec, n), crop=crop.get(), pose=p3.get(), pose_img=pi.get())
        return out, rows

    got, _ = run(None)
    assert got['status'].tolist() == [OK, OK, OK, IDLE]
    assert np.isfinite(got['in0']).all() and np.isfinite(got['crop']).all()            # no pad element (NaN) was read
    assert np.isfinite(got['pose']).all() and not np.array_equal(got['com'][:3], coms[:3])
    for c in range(C):
        want, rows = run(c)
        assert want['partial'].tobytes() == got['partial'][c:c + 1].tobytes(), c
        for k in want:
            if k != 'partial':
                assert want[k].tobytes() == got[k][rows].tobytes(), (c, k)
    # the unlike cameras matter: source 2's tracks through source 0's camera give other centres
    wrong = _table(rt, [cams[0]] * 3, sizes)
    fr, _ = _ragged(rt, wrong, frames, np.float32)
    co, cu, no = rt.upload(coms), rt.upload(cubes), rt.upload(net_out)
    s, g = _i32(rt, src), _i32(rt, gate)
    partial, rec = ops.frame_range_workspace(rt, C), rt.alloc(Tn * nrec, np.uint8)
    c3, st = rt.alloc((Tn, 3), zero=False), rt.alloc((Tn,), np.int32)
    ops.frame_range(rt, fr, None, None, None, partial, table=wrong)(rt.stream)
    ops.crop_prepare_ranged(rt, partial, Tn, co, cu, None, None, rs, rec, None, stretch=True, tracks=ops.TrackSet(Tn, s, g, table=wrong))(rt.stream)
    ops.track_refine(rt, fr, rec, Tn, None, None, co, cu, no, None, None, None, ds, co, c3, rec, st, tracks=ops.TrackSet(Tn, s, g, table=wrong))(rt.stream)
    rt.synchronize()
    assert not np.array_equal(co.get()[0], got['com'][0]) and np.array_equal(co.get()[1], got['com'][1])


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('dtype,median,mirror', [('float32', False, False), ('uint16', True, True), ('uint16', False, True),
                                                 ('float32', True, False)])
def test_frame_ingest_src_equals_frame_ingest_on_each_source_alone(backend, dtype, median, mirror):
    """The odd width (45) makes the padded raw offset of the second and third source matter: 1665 uint16 are padded to 1672."""
    rt = get_runtime(backend)
    cams, sizes, frames = _launch_case()[:3]
    dt = np.dtype(dtype)
    raws = [np.rint(f).astype(dt) for f in frames]
    table = _table(rt, cams, sizes, dt.itemsize)
    if dtype == 'uint16':
        assert table.host['raw_off'].tolist() == [0, 1672, 1672 + 3072] and table.host['frame_off'].tolist() == [0, 1668, 1668 + 3072]
    raw, _ = _ragged(rt, table, raws, dt, raw=True)
    out, _ = _ragged(rt, table, [np.zeros(s, np.float32) for s in sizes], np.float32)
    partial = ops.frame_range_workspace(rt, 3)
    ops.frame_ingest(rt, raw, None, None, None, out, partial, median=median, mirror=mirror, table=table)(rt.stream)
    rt.synchronize()
    got, gp = out.get(), partial.get().reshape(3, -1)
    assert np.isnan(_pads(table, got)).all() and _pads(table, got).size == 6           # the pad elements: never written
    for c, (H, W) in enumerate(sizes):
        one, p1 = rt.alloc((1, H, W), zero=False), ops.frame_range_workspace(rt, 1)
        ops.frame_ingest(rt, rt.upload(raws[c][None]), 1, H, W, one, p1, median=median, mirror=mirror)(rt.stream)
        rt.synchronize()
        off = int(table.host['frame_off'][c])
        assert got[off:off + H * W].tobytes() == one.get().tobytes(), c
        assert gp[c].tobytes() == p1.get().tobytes(), c
        assert np.isfinite(got[off:off + H * W]).all() and got[off:off + H * W].max() < 60000.      # no pad element (0xFFFF) was read


# ---- 7: validation -----------------------------------------------------------------------------------------------------------------
def test_src_entry_points_refuse_bad_arguments_without_a_gpu():
    """Argument validation happens before any launch: callable on the product library without a GPU."""
    import __graft_entry__
    if not os.path.exists(lib.DEFAULT_LIB):
        __graft_entry__.build()
    so = lib.load()
    assert so.dpp_abi_version() == lib.ABI_VERSION >= 19
    assert so.dpp_source_record_bytes() == ops.SOURCE_RECORD.itemsize == 80
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    E = 10001
    assert so.dpp_frame_range_src(None, p, 1, p, None) == E and so.dpp_frame_range_src(p, None, 1, p, None) == E
    assert so.dpp_frame_range_src(p, p, 0, p, None) == E and so.dpp_frame_range_src(p, p, 1, None, None) == E
    assert so.dpp_frame_ingest_src(None, 1, p, 1, 0, p + 64, None, None) == E and so.dpp_frame_ingest_src(p, 1, None, 1, 0, p + 64, None, None) == E
    assert so.dpp_frame_ingest_src(p, 1, p, 0, 0, p + 64, None, None) == E and so.dpp_frame_ingest_src(p, 3, p, 1, 0, p + 64, None, None) == E
    assert so.dpp_frame_ingest_src(p, 1, p, 1, 4, p + 64, None, None) == E and so.dpp_frame_ingest_src(p, 1, p, 1, 0, p, None, None) == E
    assert so.dpp_crop_prepare_ranged_src(p, 1, p, p, None, p, p, 8, 0, p, None, None) == E
    assert so.dpp_crop_prepare_ranged_src(p, 0, p, p, p, p, p, 8, 0, p, None, None) == E
    assert so.dpp_crop_prepare_ranged_src(p, 1, p, p, p, p, p, 0, 0, p, None, None) == E
    assert so.dpp_crop_prepare_ranged_src(p, 1, None, p, p, p, p, 8, 0, p, None, None) == E
    assert so.dpp_crop_warp_src(p, p, 1, p, None, 8, 1, 0., p, None) == E and so.dpp_crop_warp_src(p, p, 0, p, p, 8, 1, 0., p, None) == E
    assert so.dpp_crop_warp_src(p, p, 1, p, p, 0, 1, 0., p, None) == E and so.dpp_crop_warp_src(None, p, 1, p, p, 8, 1, 0., p, None) == E
    assert so.dpp_track_refine_src(p, p, 1, p, p, None, p, p, p, 8, p, p, p, None, p, None) == E
    assert so.dpp_track_refine_src(p, p, 0, p, p, p, p, p, p, 8, p, p, p, None, p, None) == E
    assert so.dpp_track_refine_src(p, p, 1, p, p, p, p, p, p, 0, p, p, p, None, p, None) == E
    assert so.dpp_track_refine_src(p, p, 1, p, p, p, p, p, p, 8, p, p, p, None, None, None) == E
    assert so.dpp_crop_warp_ex_src(p, p, 1, p, p, None, 8, 0, 0., 0., 0., p, None) == E
    assert so.dpp_crop_warp_ex_src(p, p, 0, p, p, p, 8, 0, 0., 0., 0., p, None) == E
    assert so.dpp_crop_warp_ex_src(p, p, 1, p, p, p, 0, 0, 0., 0., 0., p, None) == E
    assert so.dpp_crop_warp_ex_src(p, p, 1, p, p, p, 8, ops.CROP_FLIP_X, 0., 0., 0., p, None) == E
    assert so.dpp_pose_finish_src(p, 1, 1, None, p, p, p, p, p, p, None) == E and so.dpp_pose_finish_src(p, 1, 1, p, p, None, p, p, p, p, None) == E
    assert so.dpp_pose_finish_src(p, 0, 1, p, p, p, p, p, p, p, None) == E and so.dpp_pose_finish_src(p, 1, 0, p, p, p, p, p, p, p, None) == E


# ---- the tracker over unlike sources ------------------------------------------------------------------------------------------------
TRACKS = [(0, False), (0, True), (1, False), (2, True)]


@functools.lru_cache(maxsize=None)
def _setup(size):
    """(importers, cameras, sizes, cube, ticks, tracks, sequences).  small: source 0 is tests.test_multitrack's small set-up (ICVL at
    120 x 160), source 1 MSRA15 at 96 x 128, source 2 ICVL at 96 x 128, tracks (0, L) (0, R) (1, L) (2, R), 4 ticks + the starting
    frame.  large: T = 8 over C = 4, two NYU sources at 480 x 640 and two at 240 x 320 with the ICVL camera, 4 ticks."""
    if size == 'small':
        dis = [ICVLImporter('../data/ICVL/'), MSRA15Importer('../data/MSRA15/'), ICVLImporter('../data/ICVL/')]
        cams, sizes, cube, tracks = [A.Camera.icvl(), A.Camera.msra(), A.Camera.icvl()], [(120, 160), (96, 128), (96, 128)], (250., 250., 250.), TRACKS
    else:
        dis = [NYUImporter('../data/NYU/'), ICVLImporter('../data/ICVL/'), NYUImporter('../data/NYU/'), ICVLImporter('../data/ICVL/')]
        cams, sizes, cube = [A.Camera.nyu(), A.Camera.icvl(), A.Camera.nyu(), A.Camera.icvl()], [(480, 640), (240, 320)] * 2, (300., 300., 300.)
        tracks = [(2, False), (0, True), (1, False), (0, False), (3, True), (3, False), (1, True), (2, True)]
    n = 5
    seqs = [T.drifting_sequence(np.random.RandomState(41 + c), n, cams[c], sizes[c][0], sizes[c][1], cube) for c in range(len(dis))]
    for f, c in seqs:
        f.setflags(write=False)
        c.setflags(write=False)
    return dis, cams, sizes, cube, n, tracks, seqs


def _hetero(rt, backend, size, **kw):
    from hipdp.multitrack import MultiTracker
    dis, cams, sizes, cube, n, tracks, seqs = _setup(size)
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, len(tracks), **({'zero_refine': True} if kw.pop('zero_refine', False) else {}))
    return MultiTracker(rt, dis, pnet, snet, [s[0] for s in sizes], [s[1] for s in sizes], kw.pop('cube', cube), tracks, **kw)


def _tick(seqs, i):
    return [f[i] for f, _ in seqs]


@pytest.mark.parametrize('backend,size', SETUPS)
def test_unlike_sources_equal_per_source_homogeneous_trackers(backend, size):
    """Free-running, 4 ticks: every key of every track-tick of the tracker over unlike sources has the bits of a homogeneous
    MultiTracker on the same T-row nets with that source's importer and size in which only that source delivers frames."""
    from hipdp.multitrack import MultiTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, cams, sizes, cube, n, tracks, seqs = _setup(size)
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, len(tracks))
    mt = _hetero(rt, backend, size)
    assert mt.hetero and mt.table is not None
    for t, (c, _) in enumerate(tracks):
        mt.reset(t, seqs[c][1][0])
    got = [mt.process(_tick(seqs, i), return_crop=True) for i in range(1, n)]
    assert all(r['status'] == OK for tick in got for r in tick)
    compared = 0
    for c in range(len(dis)):
        one = MultiTracker(rt, dis[c], pnet, snet, sizes[c][0], sizes[c][1], cube, tracks)
        assert not one.hetero and one.table is None
        mine = [t for t, (s, _) in enumerate(tracks) if s == c]
        for t in mine:
            one.reset(t, seqs[c][1][0])
        for i in range(1, n):
            res = one.process([seqs[c][0][i] if s == c else None for s in range(len(dis))], return_crop=True)
            for t in mine:
                assert res[t]['status'] == OK and got[i - 1][t]['status'] == OK
                _same(got[i - 1][t], res[t], (c, i, t))
                compared += 1
    assert compared == len(tracks) * (n - 1)
    if size == 'small':                                                # same size, unlike cameras: sources 1 and 2 must differ
        assert mt.sizes[1] == mt.sizes[2] and mt.cams[1] != mt.cams[2]


@pytest.mark.parametrize('backend,size', SETUPS)
def test_unlike_sources_match_restatement_teacher_forced(backend, size):
    """tests.test_multitrack.test_tracks_match_restatement_teacher_forced with each track's OWN camera and frame size, at its
    tolerances: the net inputs and the final crop exact, the centre to 2e-4, the pose within 1e-3 mm of the float64 oracle net,
    pose_img exact."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, cams, sizes, cube, n, tracks, seqs = _setup(size)
    Tn = len(tracks)
    (snet, sonet, sP), (pnet, ponet, pP) = _nets(rt, backend, Tn)
    sfwd, pfwd = _oracle_forward(sonet, sP), _oracle_forward(ponet, pP)
    mt = _hetero(rt, backend, size)
    pre = {}
    for i in range(1, n):
        for t, (c, _) in enumerate(tracks):
            mt.reset(t, seqs[c][1][i - 1])                            # teacher: the previous frame's true centre
        res = mt.process(_tick(seqs, i), return_crop=True)
        x_ins = [b.buf.get() for b in mt.ceng.x_ins]
        oracle_pose = size == 'small' or i == 1                       # (the float64 ResNet takes a second per crop)
        for t, (c, right) in enumerate(tracks):
            cam, fx, fy = cams[c], abs(cams[c].fx), abs(cams[c].fy)
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
            want = T.pose_input(crop, T.HAND_RIGHT if right else T.HAND_LEFT)[0, 0]
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


# ---- 3 / 4: all-equal sequences are today's path; the plan's structure ---------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_all_equal_sequences_are_the_homogeneous_path(backend):
    from hipdp.multitrack import MultiTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    di = ICVLImporter('../data/ICVL/')
    tracks = [(0, False), (0, True), (1, False)]
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 3)
    a = MultiTracker(rt, di, pnet, snet, 120, 160, (250., 250., 250.), tracks, fx=241.42, fy=241.42)
    b = MultiTracker(rt, [di, ICVLImporter('../data/ICVL/')], pnet, snet, [120, 120], (160, 160), (250., 250., 250.), tracks,
                     fx=[241.42, 241.42], fy=[241.42, None])
    assert not b.hetero and b.table is None and b.frames.shape == a.frames.shape == (2, 120, 160) and (b.H, b.W) == (120, 160)
    la, lb = a.plan().launches(), b.plan().launches()
    assert [l.name for l in la] == [l.name for l in lb] and [l.fn for l in la] == [l.fn for l in lb]

    def norm(l):                                                       # the trackers' own buffers differ: a pointer is a pointer
        return tuple('ptr' if isinstance(v, int) and v > 1 << 20 else v for v in l.args)
    assert [norm(l) for l in la] == [norm(l) for l in lb]
    assert la[0].args[1:4] == (2, 120, 160) and 'ptr' in norm(la[0])
    assert not any(l.fn in (rt.lib.dpp_frame_range_src, rt.lib.dpp_track_refine_src, rt.lib.dpp_pose_finish_src) for l in lb)


@pytest.mark.parametrize('backend', BACKENDS)
def test_unlike_sources_plan_structure(backend, monkeypatch):
    from hipdp.multitrack import MultiTracker
    from hipdp.tracker import HandTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, cams, sizes, cube, n, tracks, seqs = _setup('small')
    (snet1, _, _), (pnet1, _, _) = _nets(rt, backend, 1)
    single = len(HandTracker(rt, dis[0], pnet1, snet1, 120, 160, cube).plan(0).launches())
    for tr, srcs in (([(0, False), (1, True)], [0, 1]), (TRACKS, [0, 1, 2])):
        (snet, _, _), (pnet, _, _) = _nets(rt, backend, len(tr))
        mt = MultiTracker(rt, [dis[c] for c in srcs], pnet, snet, [sizes[c][0] for c in srcs], [sizes[c][1] for c in srcs], cube, tr)
        launches = mt.plan().launches()
        assert mt.hetero and len(launches) == single, (len(tr), len(srcs))   # the launch count of ONE tracker, whatever T and C are
        fns = [l.fn for l in launches]
        assert launches[0].fn is rt.lib.dpp_frame_range_src and launches[0].args[2] == len(srcs)
        for fn in (rt.lib.dpp_frame_range_src, rt.lib.dpp_crop_prepare_ranged_src, rt.lib.dpp_crop_warp_src, rt.lib.dpp_track_refine_src,
                   rt.lib.dpp_crop_warp_ex_src, rt.lib.dpp_pose_finish_src):
            assert fns.count(fn) == 1
        for fn in (rt.lib.dpp_frame_range, rt.lib.dpp_crop_prepare_ranged_ix, rt.lib.dpp_crop_warp_ix, rt.lib.dpp_track_refine_ix,
                   rt.lib.dpp_crop_warp_ex_ix, rt.lib.dpp_pose_finish_ix):
            assert fn not in fns
        assert launches[0].meta['bytes'] == 4.0 * sum(sizes[c][0] * sizes[c][1] for c in srcs)
        sens = MultiTracker(rt, [dis[c] for c in srcs], pnet, snet, [sizes[c][0] for c in srcs], [sizes[c][1] for c in srcs], cube, tr,
                            sensor=dict(dtype='uint16', median=True))
        ls = sens.plan().launches()
        assert len(ls) == single and ls[0].fn is rt.lib.dpp_frame_ingest_src and rt.lib.dpp_frame_range_src not in [l.fn for l in ls]
    for t, (c, _) in enumerate(tracks):
        mt.reset(t, seqs[c][1][0])
    calls = dict(h2d=[], run=0, d2h=[])
    real_in, real_out, real_run = rt.copy_in, rt.download, ops.Plan.run
    monkeypatch.setattr(rt, 'copy_in', lambda buf, arr: (calls['h2d'].append(buf.ptr), real_in(buf, arr))[1], raising=False)
    monkeypatch.setattr(rt, 'download', lambda buf: (calls['d2h'].append(buf.ptr), real_out(buf))[1], raising=False)
    monkeypatch.setattr(ops.Plan, 'run', lambda self, r: (calls.__setitem__('run', calls['run'] + 1), real_run(self, r))[1])
    f = [mt.frames.ptr + 4 * int(o) for o in mt.table.host['frame_off']]
    assert f[1] - f[0] == 4 * 120 * 160 and f[2] - f[1] == 4 * 96 * 128

    def tick(frames, h2d):
        calls.update(h2d=[], run=0, d2h=[])
        out = mt.process(frames)
        assert calls['h2d'] == h2d and calls['run'] == 1 and calls['d2h'] == [mt.res.ptr], (calls, h2d)
        return out
    tick(_tick(seqs, 1), f + [mt.gate.ptr])                           # the first tick opens the gates: one upload more
    tick(_tick(seqs, 2), f)                                           # one upload per fresh source, one plan, one download
    r3 = tick([None, seqs[1][0][3], None], [f[1], mt.gate.ptr])
    assert [r['status'] for r in r3] == [IDLE, IDLE, OK, IDLE]
    monkeypatch.undo()


# ---- 5: a detector per camera ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_acquire_runs_the_detector_of_the_tracks_own_camera(backend):
    from hipdp.detect import FrameDetector
    from hipdp.multitrack import MultiTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, cams, sizes, cube, n, tracks, seqs = _setup('small')
    mt = _hetero(rt, backend, 'small')
    frame = seqs[1][0][0]
    got = mt.acquire(2, frame)
    det = FrameDetector(rt, 96, 128, abs(cams[1].fx), abs(cams[1].fy), 1)
    coms, cubes, found = det.run(frame[None], [cube])[:3]
    assert got['found'] and found[0] and got['com'].tobytes() == np.float32(coms[0]).tobytes() and np.array_equal(got['cube'], np.float32(cube))
    assert not mt.lost[2] and mt.lost[0] and np.array_equal(mt.frames.get()[mt.table.host['frame_off'][1]:][:frame.size], frame.ravel())
    res = mt.process(_tick(seqs, 1))
    assert [r['status'] for r in res] == [LOST, LOST, OK, LOST]
    with pytest.raises(ValueError):
        mt.acquire(2, seqs[0][0][0])                                   # a frame of another source's shape
    # acquire_source: two tracks on one small source of a tracker over unlike sources, against the several-hands detector alone
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 3)
    two = MultiTracker(rt, [dis[0], dis[1]], pnet, snet, [120, 96], [160, 128], cube, [(0, False), (1, False), (1, True)])
    f2 = np.array(seqs[1][0][0])
    f2[10:40, 90:120] = 500.                                           # a second, nearer object
    out = two.acquire_source(1, f2)
    det2 = FrameDetector(rt, 96, 128, abs(cams[1].fx), abs(cams[1].fy), 1, hands=2)
    coms2, _, found2 = det2.run(f2[None], [cube])[:3]
    assert [o['found'] for o in out] == [bool(v) for v in found2[0]] and out[0]['found']
    for k, o in enumerate(out):
        if o['found']:
            assert o['com'].tobytes() == np.float32(coms2[0][k]).tobytes(), k


# ---- 6: process_sequence against a process() loop ------------------------------------------------------------------------------------
def _state(mt):
    return dict(lost=mt.lost.copy(), com_host=mt.com_host.copy(), gate_host=np.asarray(mt.gate_host).copy(), runs=mt.runs,
                com=mt.com.get(), gate=mt.gate.get())


def _compare_sequence(seq, loop, a, b):
    assert len(seq) == len(loop)
    live = 0
    for i, (ts, tl) in enumerate(zip(seq, loop)):
        for t, (rs, rl) in enumerate(zip(ts, tl)):
            assert rs['status'] == rl['status'], (i, t)
            if rs['status'] != LOST:
                _same(rs, rl, (i, t))
                live += 1
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    return live


@pytest.mark.parametrize('backend,size', SETUPS)
def test_process_sequence_equals_a_process_loop(backend, size):
    """6 ticks, source 1 delivering a frame only every second tick."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, cams, sizes, cube, n, tracks, seqs = _setup(size)
    ticks = []
    for i in range(6):
        fr = _tick(seqs, 1 + i % (n - 1))
        if i % 2:
            fr[1] = None
        ticks.append(fr)
    a, b = _hetero(rt, backend, size), _hetero(rt, backend, size)
    for mt in (a, b):
        for t, (c, _) in enumerate(tracks):
            mt.reset(t, seqs[c][1][0])
    loop = [b.process(fr, return_crop=True) for fr in ticks]
    seq = a.process_sequence(iter(ticks), return_crops=True)
    on1 = [t for t, (c, _) in enumerate(tracks) if c == 1]
    assert [[r['status'] for r in tick] for tick in loop] == [[IDLE if (i % 2 and t in on1) else OK for t in range(len(tracks))] for i in range(6)]
    assert _compare_sequence(seq, loop, a, b) == 6 * len(tracks)
    # ... and the tracker goes on ticking as the loop's does
    _same(a.process(_tick(seqs, 1), return_crop=True)[0], b.process(_tick(seqs, 1), return_crop=True)[0], 'the tick after')
    with pytest.raises(ValueError):
        a.process_sequence([[seqs[0][0][0]]])


@pytest.mark.parametrize('backend', BACKENDS)
def test_process_sequence_with_a_track_lost_on_the_way(backend):
    """The refinement net that answers (0, 0, -2) with a 300 mm cube: track 0 goes 900 -> 600 -> 300 -> 0 and is lost in tick 2, the
    others start at 2500 mm and go on.  The host learns it one tick late; the results are the process() loop's all the same."""
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, cams, sizes, cube, n, tracks, seqs = _setup('small')
    cube = (300., 300., 300.)
    ticks = [_tick(seqs, i % n) for i in range(6)]
    a, b = (_hetero(rt, backend, 'small', zero_refine=True, cube=cube) for _ in range(2))
    for mt in (a, b):
        mt.reset(0, (75., 55., 900.))
        for t in (1, 2, 3):
            mt.reset(t, (60., 45., 2500.))
    loop = [b.process(fr, return_crop=True) for fr in ticks]
    seq = a.process_sequence(ticks, return_crops=True)
    assert [tick[0]['status'] for tick in loop] == [OK, OK, LOST, LOST, LOST, LOST]
    assert all(tick[t]['status'] == OK for tick in loop for t in (1, 2, 3)) and loop[-1][1]['com'][2] == 2500. - 6 * 300.
    assert _compare_sequence(seq, loop, a, b) == 2 + 3 * 6
    assert a.lost.tolist() == [True, False, False, False] and a.gate_host.tolist() == [0, 1, 1, 1]


# ---- 7: validation of the constructor forms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_constructor_and_frames_are_validated(backend):
    from hipdp.multitrack import MultiTracker
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    dis, cams, sizes, cube, n, tracks, seqs = _setup('small')
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, len(tracks))
    Hs, Ws = [s[0] for s in sizes], [s[1] for s in sizes]
    with pytest.raises(ValueError):
        MultiTracker(rt, dis[:2], pnet, snet, Hs, Ws, cube, tracks)                   # two importers for three sources
    with pytest.raises(ValueError):
        MultiTracker(rt, dis, pnet, snet, Hs[:2], Ws, cube, tracks)
    with pytest.raises(ValueError):
        MultiTracker(rt, dis, pnet, snet, Hs, Ws + [64], cube, tracks)
    with pytest.raises(ValueError):
        MultiTracker(rt, dis, pnet, snet, [120, 0, 96], Ws, cube, tracks)             # a non-positive size
    with pytest.raises(ValueError):
        MultiTracker(rt, dis, pnet, snet, Hs, Ws, cube, tracks, fx=[241.42, 0., 241.42])   # a zero focal length
    with pytest.raises(ValueError):
        MultiTracker(rt, [dis[0], DepthImporter(0., 241.42, 160., 120.), dis[2]], pnet, snet, Hs, Ws, cube, tracks)
    with pytest.raises(ValueError):
        MultiTracker(rt, dis, pnet, snet, Hs, Ws, cube, tracks, fy=[241.42] * 4)
    mt = MultiTracker(rt, dis, pnet, snet, Hs, Ws, cube, tracks)
    with pytest.raises(ValueError):
        mt.process([seqs[0][0][0], seqs[0][0][0], seqs[2][0][0]])                     # source 1 handed a frame of source 0's shape
    with pytest.raises(ValueError):
        mt.process_sequence([[seqs[1][0][0], seqs[1][0][0], seqs[2][0][0]]])
    with pytest.raises(ValueError):
        ops.SourceTable(rt, [_camt(c) for c in cams], [(241.42, 241.42)] * 3, [(120, 160), (96, 128), (-1, 128)])
    with pytest.raises(ValueError):
        ops.SourceTable(rt, [_camt(c) for c in cams], [(241.42, 241.42), (0., 241.42), (241.42, 241.42)], sizes)
    sens = MultiTracker(rt, dis, pnet, snet, Hs, Ws, cube, tracks, sensor=dict(dtype='uint16'))
    with pytest.raises(ValueError):
        sens.process([f.astype(np.float32) for f in _tick(seqs, 0)])                  # the sensor's dtype, per source too


# ---- 8: the class API and the example on top -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_multi_stream_pipeline_on_devices_of_unlike_sizes_and_cameras(backend, tmp_path):
    """Two FileDevices: a 240 x 320 ICVL sequence and a 120 x 160 one recorded through the camera of half the intrinsics."""
    from hipdp.multitrack import MultiTracker
    from tests.test_multitrack import _two_icvl_sequences
    from tests.test_realtime import _write_icvl_sequence
    from util.cameradevice import FileDevice
    from util.realtimehandposepipeline import MultiStreamPipeline
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    n = 4
    base, di, cube, seqs, _ = _two_icvl_sequences(tmp_path, n)
    hcam = _half(A.Camera.icvl())
    hdi = DepthImporter(hcam.fx, hcam.fy, hcam.ux, hcam.uy)
    hframes, hcoms = T.drifting_sequence(np.random.RandomState(71), n, hcam, 120, 160, tuple(float(c) for c in cube))
    hframes, _ = _write_icvl_sequence(base, 'half_seq', hframes, hcoms, hcam, seed=9)
    hfiles = [os.path.join(base, 'Depth', '201403121135', 'half_seq_%04d.png' % i) for i in range(n)]
    (snet, _, _), (pnet, _, _) = _nets(rt, backend, 3, J=16)
    config = {'fx': [241.42, 120.71], 'fy': [241.42, 120.71], 'cube': cube}
    L, Rr = MultiStreamPipeline.HAND_LEFT, MultiStreamPipeline.HAND_RIGHT
    hands = [(0, L), (0, Rr), (1, L)]
    init = [seqs[0][1][0], seqs[0][1][0], hcoms[0]]

    def pipeline():
        return MultiStreamPipeline(pnet, dict(config), [di, hdi], [FileDevice(seqs[0][2], di), FileDevice(hfiles, di)], hands, snet, init_com=init)
    msp = pipeline()
    poses = msp.processVideos()
    assert [p.shape for p in poses] == [(n, 16, 3)] * 3 and all(np.isfinite(p).all() for p in poses) and len(msp.frame_times) == n
    assert msp._tracker.hetero and msp._tracker.sizes == [(240, 320), (120, 160)]
    mt = MultiTracker(rt, [di, hdi], pnet, snet, [240, 120], [320, 160], cube, [(d, h == Rr) for d, h in hands], fx=config['fx'], fy=config['fy'])
    for t in range(3):
        mt.reset(t, init[t])
    for i in range(n):
        res = mt.process([seqs[0][0][i], hframes[i]])
        for t in range(3):
            assert res[t]['status'] == OK and np.array_equal(res[t]['pose'], poses[t][i]), (i, t)
    over = pipeline()
    poses2 = over.processVideos(overlapped=True)
    assert over._tracker.runs == n and len(over.frame_times) == n
    for t in range(3):
        assert np.array_equal(poses2[t], poses[t]), t
    assert [p.shape for p in pipeline().processVideos(max_frames=3, overlapped=True)] == [(3, 16, 3)] * 3
    with pytest.raises(ValueError):
        MultiStreamPipeline(pnet, dict(config), [di], [FileDevice(seqs[0][2], di), FileDevice(hfiles, di)], hands, snet, init_com=init)


@pytest.mark.parametrize('backend', BACKENDS)
def test_realtime_multi_example_with_a_half_resolution_second_camera(backend, tmp_path):
    import importlib.util
    from tests.test_multitrack import ROOT, _two_icvl_sequences
    R.set_default_runtime(get_runtime(backend))
    base, _, _, _, _ = _two_icvl_sequences(tmp_path, 3)
    spec = importlib.util.spec_from_file_location('realtime_multi_driver', os.path.join(ROOT, 'examples', 'realtime_multi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = 'resnet' if backend == 'hip' else 'poseregnet'               # (the 128x128 ResNet is too slow for the SIMT emulator)
    common = ['--dataset', 'icvl', '--data', base, '--net', net, '--cache', str(tmp_path / 'cache')]
    full, _ = mod.main(common)
    poses, errs, diff = mod.main(common + ['--half-res-second'])
    assert [p.shape for p in poses] == [(3, 16, 3)] * 3 and all(np.isfinite(p).all() for p in poses)
    assert np.array_equal(poses[0], full[0]) and np.array_equal(poses[1], full[1])     # camera 0 is untouched by camera 1's change
    assert np.isfinite(diff) and not np.array_equal(poses[2], full[2])
    poses3, _, _ = mod.main(common + ['--half-res-second', '--overlapped'])
    for t in range(3):
        assert np.array_equal(poses3[t], poses[t]), t
