"""Sensor frames on the device (csrc/ingest.hip, ABI v15; HandTracker / FrameDetector / RealtimeHandposePipeline(sensor=...),
util.cameradevice.filter_depth / FilteredDevice): uint16 / float32 ingest, mirror and the 3x3 median of the reference's
CreativeCameraDevice.getDepth, against the NumPy restatement of tests/ingest_ref.py -- which is first held to
scipy.ndimage.median_filter(size=3, mode='nearest'), the border rule of cv2.medianBlur.  A median is a selection: every comparison
here is np.array_equal.  The device tests run on the SIMT emulator and, with -m gpu, on the card."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from data.importers import ICVLImporter
from hipdp import ops
from hipdp import runtime as R
from oracle import augment as A
from tests import ingest_ref as I
from tests import track_ref as T
from tests.backends import BACKENDS, get_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = FY = 241.42
BADARG = 10001
# the restatement's shapes (1: scipy), then: H below / not a multiple of / equal to FR_BANDS = 64 (empty bands), single rows and columns (all
# border), odd W (uint16 rows that lose their 16-byte alignment), W past a multiple of the vector width, B > 1
REF_SHAPES = [(1, 1, 1), (2, 1, 7), (2, 5, 1), (3, 3, 5), (2, 37, 53), (1, 65, 66), (1, 130, 131)]
KERNEL_SHAPES = REF_SHAPES + [(3, 63, 64), (1, 64, 64), (1, 129, 641)]
# beyond the median path's LDS tile: wider than its 1024 columns, bands taller than the rows it holds at that width
TILE_SHAPES = [(1, 70, 1100), (1, 700, 1030)]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]          # (median, mirror)
MAKERS = dict(uint16=I.u16_frames, float32=I.f32_frames)


def _sid(s):
    return 'x'.join(map(str, s))


@functools.lru_cache(maxsize=None)
def _raw(dtype, shape):
    a = MAKERS[dtype](np.random.RandomState(sum(shape) + len(dtype)), *shape)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(dtype, shape, median, mirror):
    out, mn, mx = I.ingest(_raw(dtype, shape), median, mirror)
    out.setflags(write=False)
    return out, mn, mx


# ---- 1: the restatement is the reference's filter ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['uint16', 'float32'])
@pytest.mark.parametrize('shape', REF_SHAPES, ids=_sid)
def test_restatement_is_scipy_median_filter(dtype, shape):
    from scipy import ndimage
    a = _raw(dtype, shape)
    m = I.median3(a)
    assert m.dtype == a.dtype and m.shape == a.shape
    for b in range(shape[0]):
        assert np.array_equal(m[b], ndimage.median_filter(a[b], size=3, mode='nearest')), b
    assert np.array_equal(I.median3(a[:, :, ::-1]), m[:, :, ::-1])      # the mirror commutes with the replicate-border median
    out, mn, mx = I.ingest(a, median=True, mirror=True)
    assert out.dtype == np.float32 and np.array_equal(out, m[:, :, ::-1].astype(np.float32))
    assert np.array_equal(mn, out.reshape(shape[0], -1).min(1)) and np.array_equal(mx, out.reshape(shape[0], -1).max(1))
    if dtype == 'uint16' and a.size > 1000:
        assert 0.25 < (a == 0).mean() < 0.35 and (a == 65535).any()
    if dtype == 'float32':
        assert not np.isnan(a).any() and not np.signbit(a).any()


# ---- 2: the kernel, bit for bit ------------------------------------------------------------------------------------------------
SENTINEL = np.float32(-7.25)


def _run_ingest(rt, raw, median, mirror, with_partial=True):
    B, H, W = raw.shape
    d = rt.upload(raw)
    out = rt.alloc((B, H, W), np.float32, zero=False)
    part = ops.frame_range_workspace(rt, B) if with_partial else None
    if with_partial:
        part.set(np.full(part.size, SENTINEL, np.float32))
    ops.frame_ingest(rt, d, B, H, W, out, part, median=median, mirror=mirror)(rt.stream)
    rt.synchronize()
    return out.get(), (part.get().reshape(B, -1, 2) if with_partial else None)


def _check_ingest(rt, dtype, shape, median, mirror):
    ref, mn, mx = _ref(dtype, shape, median, mirror)
    got, p = _run_ingest(rt, _raw(dtype, shape), median, mirror)
    assert got.dtype == np.float32 and np.array_equal(got, ref), (dtype, shape, median, mirror)
    assert p.shape[1] == 64 and not (p == SENTINEL).any()               # every band's pair was written
    assert np.array_equal(p[:, :, 0].min(axis=1), mn) and np.array_equal(p[:, :, 1].max(axis=1), mx)
    rows = -(-shape[1] // 64)
    empty = np.arange(64) * rows >= shape[1]                            # bands past the last row: frame_range's identities
    assert np.all(p[:, empty, 0] == np.float32(3.4e38)) and np.all(p[:, empty, 1] == np.float32(-3.4e38))


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('dtype', ['uint16', 'float32'])
@pytest.mark.parametrize('shape', KERNEL_SHAPES + TILE_SHAPES, ids=_sid)
def test_frame_ingest_bit_for_bit(backend, dtype, shape):
    rt = get_runtime(backend)
    for median, mirror in FLAGS:
        _check_ingest(rt, dtype, shape, median, mirror)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('dtype,median,mirror', [('uint16', True, True), ('float32', True, False)], ids=['u16', 'f32'])
def test_frame_ingest_working_size(backend, dtype, median, mirror):
    _check_ingest(get_runtime(backend), dtype, (1, 480, 640), median, mirror)


@pytest.mark.parametrize('backend', BACKENDS)
def test_frame_ingest_null_partial_and_refused_calls(backend):
    rt = get_runtime(backend)
    shape = (2, 37, 53)
    B, H, W = shape
    for dtype in ('uint16', 'float32'):
        got, _ = _run_ingest(rt, _raw(dtype, shape), True, True, with_partial=False)
        assert np.array_equal(got, _ref(dtype, shape, True, True)[0])
    assert (ops.INGEST_U16, ops.INGEST_F32, ops.INGEST_MEDIAN3, ops.INGEST_MIRROR_X) == (1, 2, 1, 2)
    raw = rt.upload(_raw('float32', shape))
    out = rt.alloc(shape, np.float32, zero=False)
    part = ops.frame_range_workspace(rt, B)
    out.set(np.full(shape, SENTINEL, np.float32))
    part.set(np.full(part.size, SENTINEL, np.float32))
    f = rt.lib.dpp_frame_ingest
    bad = [(raw.ptr, 2, 0, H, W, 0, out.ptr), (raw.ptr, 2, B, 0, W, 0, out.ptr), (raw.ptr, 2, B, H, -1, 0, out.ptr),      # B, H, W below 1
           (raw.ptr, 0, B, H, W, 0, out.ptr), (raw.ptr, 3, B, H, W, 1, out.ptr),                                         # unknown type
           (raw.ptr, 2, B, H, W, 4, out.ptr), (raw.ptr, 1, B, H, W, 7, out.ptr),                                         # unknown flag bits
           (None, 2, B, H, W, 0, out.ptr), (raw.ptr, 2, B, H, W, 0, None),
           (out.ptr, 2, B, H, W, 1, out.ptr),                                                                              # frames aliases raw
           (out.ptr + 4 * H * W, 2, 1, H, W, 1, out.ptr + 4 * (H * W - 1)), (out.ptr + 2 * H * W, 1, 1, H, W, 0, out.ptr)]  # ... partly
    for args in bad:
        assert f(*args, part.ptr, rt.stream) == BADARG, args
    rt.synchronize()
    assert np.all(out.get() == SENTINEL) and np.all(part.get() == SENTINEL)                                              # nothing was written
    assert f(out.ptr + 4 * H * W, 2, 1, H, W, 1, out.ptr, part.ptr, rt.stream) == 0                                       # adjacent is not aliasing
    rt.synchronize()
    m = ops.frame_ingest(rt, rt.alloc(shape, np.uint16, zero=False), B, H, W, out, part, median=True).meta
    assert m['kernel'] == 'frame_ingest' and m['bytes'] == (2 + 4) * B * H * W and m['flops'] > 0
    assert ops.frame_ingest(rt, raw, B, H, W, out, None).meta['bytes'] == (4 + 4) * B * H * W


# ---- 3: downstream equivalence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('size', [(37, 53), (240, 320)], ids=_sid)
def test_ranged_prepare_from_ingest_partials(backend, size):
    """crop_prepare_ranged fed frame_ingest's partials writes the record it writes from frame_range run on the reference-filtered frame."""
    from tests.test_realtime import _records
    rt = get_runtime(backend)
    H, W = size
    cam, cube = A.Camera.icvl(), (250., 250., 250.)
    frames, coms = A.synthetic_frames(np.random.RandomState(11), 1, cam, 240, 320, cube)
    raw = np.rint(np.ascontiguousarray(frames[:, :H, :W])).astype(np.uint16)
    raw[0][np.random.RandomState(3).uniform(size=(H, W)) < 0.02] = 3                       # below the detector's 10 mm
    coms = coms * np.float32([W / 320., H / 240., 1.])
    filt, _, _ = I.ingest(raw, median=True, mirror=False)
    co, cu = rt.upload(coms), rt.upload(np.float32([cube]))
    nrec = int(rt.lib.dpp_crop_record_bytes())
    recs, Ms = [], []
    for route in ('ingest', 'range'):
        part = ops.frame_range_workspace(rt, 1)
        fr = rt.alloc((1, H, W), np.float32, zero=False)
        if route == 'ingest':
            ops.frame_ingest(rt, rt.upload(raw), 1, H, W, fr, part, median=True)(rt.stream)
        else:
            fr.set(filt)
            ops.frame_range(rt, fr, 1, H, W, part)(rt.stream)
        rec, M = rt.alloc(nrec, np.uint8), rt.alloc((1, 9), zero=False)
        ops.crop_prepare_ranged(rt, part, 1, co, cu, cam.fx, cam.fy, 128, rec, M, stretch=True)(rt.stream)
        rt.synchronize()
        assert np.array_equal(fr.get(), filt)
        recs.append(_records(rt, rec, 1))
        Ms.append(M.get())
    assert np.array_equal(recs[0], recs[1]) and np.array_equal(Ms[0], Ms[1])
    assert recs[0].any()


# ---- 4 / 5: the tracker ------------------------------------------------------------------------------------------------------
NOISE = 0.02            # share of salt-and-pepper pixels in the sensor sequence
KEYS = ('pose', 'pose_img', 'com', 'com3D', 'M', 'status', 'crop')


@functools.lru_cache(maxsize=None)
def _sensor_sequence():
    """drifting_sequence at 240 x 320, 8 frames, as a 16-bit sensor with speckle delivers it, and the two reference-filtered versions."""
    cam, cube = A.Camera.icvl(), (250., 250., 250.)
    frames, coms = T.drifting_sequence(np.random.RandomState(37), 8, cam, 240, 320, cube)
    raw = np.rint(frames).astype(np.uint16)
    rng = np.random.RandomState(38)
    u = rng.uniform(size=raw.shape)
    raw[u < NOISE / 2] = 0
    raw[(u >= NOISE / 2) & (u < NOISE)] = 3000
    plain, _, _ = I.ingest(raw, median=True, mirror=False)
    mirrored, _, _ = I.ingest(raw, median=True, mirror=True)
    for a in (raw, plain, mirrored):
        a.setflags(write=False)
    return cam, cube, raw, coms, plain, mirrored


def _same(a, b, where):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (where, k)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('hand', [T.HAND_LEFT, T.HAND_RIGHT], ids=['left', 'right'])
def test_sensor_tracker_equals_tracker_on_filtered_frames(backend, hand):
    from hipdp.tracker import HandTracker
    from tests.test_realtime import _track_nets
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend)
    cam, cube, raw, coms, plain, mirrored = _sensor_sequence()
    di = ICVLImporter('../data/ICVL/')
    H, W = raw.shape[1:]
    assert (raw.astype(np.float32) != plain).mean() > NOISE / 2                # the filter has work to do
    right = hand == T.HAND_RIGHT
    a = HandTracker(rt, di, pnet, snet, H, W, cube, hand_right=right)
    b = HandTracker(rt, di, pnet, snet, H, W, cube, hand_right=right, sensor=dict(dtype='uint16', median=True, mirror=False))
    a.reset(coms[0])
    b.reset(coms[0])
    sa, sb = a.process_sequence(list(plain), return_crops=True), b.process_sequence(list(raw), return_crops=True)
    assert len(sa) == len(sb) == 8 and all(r['status'] == 0 for r in sa)        # route A tracks every frame: a property of the input
    for i in range(8):
        _same(sa[i], sb[i], ('sequence', i))
    b.reset(coms[0])
    for i in range(8):                                                          # frame by frame: the same values again
        _same(b.process(raw[i], return_crop=True), sa[i], ('process', i))
    assert np.array_equal(b.frames[0].get()[0], plain[7])                       # what hand_size() would look at: the filtered frame
    if hand == T.HAND_LEFT:                                                     # once: mirrored on the device, against the mirrored reference frames
        c0 = coms[0] * np.float32([-1., 1., 1.]) + np.float32([W - 1., 0., 0.])
        c = HandTracker(rt, di, pnet, snet, H, W, cube, sensor=dict(dtype='uint16', median=True, mirror=True))
        a.reset(c0)
        c.reset(c0)
        sa, sc = a.process_sequence(list(mirrored), return_crops=True), c.process_sequence(list(raw), return_crops=True)
        assert len(sa) == len(sc) == 8 and all(r['status'] == 0 for r in sa)
        for i in range(8):
            _same(sa[i], sc[i], ('mirror', i))


@pytest.mark.parametrize('backend', BACKENDS)
def test_sensor_plan_structure(backend, monkeypatch):
    from hipdp.tracker import HandTracker
    from tests.test_realtime import _track_nets
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend)
    cam, cube, raw, coms, plain, _ = _sensor_sequence()
    di = ICVLImporter('../data/ICVL/')
    H, W = raw.shape[1:]
    plain_tr = HandTracker(rt, di, pnet, snet, H, W, cube)
    names = [l.name for l in plain_tr.plan(0).launches()]
    # sensor=None: the parent's plan, launch by launch (hipdp/tracker.py of the parent commit; the nets' own launches in between)
    cnet, pnet_l = [l.name for l in plain_tr.ceng.fwd.launches()], [l.name for l in plain_tr.peng.fwd.launches()]
    assert len(plain_tr.ceng.x_ins) == 3
    assert names == ['frame_range', 'crop_prepare_ranged', 'track_in0', 'track_in1', 'track_in2'] + cnet + ['track_refine', 'track_crop'] + \
        pnet_l + ['pose_finish']
    fns = [l.fn for l in plain_tr.plan(0).launches()]
    lib = rt.lib
    assert fns[:5] == [lib.dpp_frame_range, lib.dpp_crop_prepare_ranged, lib.dpp_crop_warp, lib.dpp_crop_center, lib.dpp_crop_center]
    assert [fns[5 + len(cnet)], fns[6 + len(cnet)], fns[-1]] == [lib.dpp_track_refine, lib.dpp_crop_warp_ex, lib.dpp_pose_finish]
    kernels = [(l.meta or {}).get('kernel') for l in plain_tr.plan(0).launches()]
    assert names[0] == 'frame_range' and kernels.count('frame_range') == 1 and 'frame_ingest' not in kernels      # sensor=None: the parent's plan
    assert plain_tr.raw is None and [l.fn for l in plain_tr.plan(0).launches()].count(rt.lib.dpp_frame_ingest) == 0
    tr = HandTracker(rt, di, pnet, snet, H, W, cube, sensor=dict(dtype='uint16', median=True, mirror=False))
    for slot in (0, 1):
        launches = tr.plan(slot).launches()
        k = [(l.meta or {}).get('kernel') for l in launches]
        assert len(launches) == len(names) and k.count('frame_ingest') == 1 and k.count('frame_range') == 0
        assert launches[0].fn is rt.lib.dpp_frame_ingest and [l.name for l in launches[1:]] == names[1:]
        assert launches[0].args[0] == tr.raw[slot].ptr and launches[0].args[6] == tr.frames[slot].ptr
    assert tr.raw[0].dtype == np.uint16 and tr.raw[0].nbytes == H * W * 2
    tr.reset(coms[0])
    tr.process(raw[0])                                                  # records the plan
    calls = dict(h2d=[], run=0, d2h=[])
    real_in, real_out, real_run = rt.copy_in, rt.download, ops.Plan.run
    monkeypatch.setattr(rt, 'copy_in', lambda buf, arr: (calls['h2d'].append((buf.ptr, buf.nbytes)), real_in(buf, arr))[1], raising=False)
    monkeypatch.setattr(rt, 'download', lambda buf: (calls['d2h'].append(buf.ptr), real_out(buf))[1], raising=False)
    monkeypatch.setattr(ops.Plan, 'run', lambda self, r: (calls.__setitem__('run', calls['run'] + 1), real_run(self, r))[1])
    tr.process(raw[1])
    assert calls['h2d'] == [(tr.raw[0].ptr, H * W * 2)] and calls['run'] == 1 and calls['d2h'] == [tr.res.ptr]
    tr.process(raw[2])
    assert calls['h2d'] == [(tr.raw[0].ptr, H * W * 2)] * 2 and calls['run'] == 2 and calls['d2h'] == [tr.res.ptr] * 2
    monkeypatch.undo()
    with pytest.raises(ValueError):
        tr.process(plain[0])                                            # a float32 array is not silently converted
    with pytest.raises(ValueError):
        tr.acquire(raw[0].astype(np.int32))
    with pytest.raises(ValueError):
        tr.process(raw[0][:10])
    with pytest.raises(ValueError):
        HandTracker(rt, di, pnet, snet, H, W, cube, sensor=dict(dtype='uint8'))
    with pytest.raises(ValueError):
        HandTracker(rt, di, pnet, snet, H, W, cube, sensor=dict(dtype='uint16', blur=True))


# ---- 6: acquire ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _acquire_scene(H=120, W=160):
    """A hand blob in front of a noisy far wall, as uint16, and the reference-filtered frame."""
    from tests.test_detect import _scene
    f = _scene('a', H, W)
    rng = np.random.RandomState(44)
    u = rng.uniform(size=(H, W))
    f[u < 0.01] = 0.
    f[u > 0.985] = 400. + 900. * rng.uniform(size=int((u > 0.985).sum())).astype(np.float32)      # speckle anywhere between hand and wall
    raw = np.rint(f).astype(np.uint16)
    filt, _, _ = I.ingest(raw, median=True, mirror=False)
    raw.setflags(write=False)
    filt.setflags(write=False)
    return raw, filt


@pytest.mark.parametrize('backend', BACKENDS)
def test_sensor_acquire_and_detector(backend):
    from hipdp.detect import FrameDetector
    from hipdp.tracker import HandTracker
    from tests.test_realtime import _track_nets
    from util.handdetector import find_hands
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend)
    di, cube = ICVLImporter('../data/ICVL/'), (250., 250., 250.)
    raw, filt = _acquire_scene()
    H, W = raw.shape
    sensor = dict(dtype='uint16', median=True, mirror=False)
    a = HandTracker(rt, di, pnet, snet, H, W, cube, fx=FX, fy=FY)
    b = HandTracker(rt, di, pnet, snet, H, W, cube, fx=FX, fy=FY, sensor=sensor)
    for hs in (False, True):
        ra, rb = a.acquire(filt, do_hand_size=hs), b.acquire(raw, do_hand_size=hs)
        assert ra['found'] and rb['found'] and not b.lost
        assert np.array_equal(ra['com'], rb['com']) and np.array_equal(ra['cube'], rb['cube']), hs
    assert not np.array_equal(ra['cube'], np.float32(cube))                     # the measured cube
    assert np.array_equal(a.hand_size(), b.hand_size())                         # hand_size() reads the filtered frames[0]
    kernels = [(l.meta or {}).get('kernel') for l in b.detector().plan(False).launches()]
    assert kernels[0] == 'frame_ingest' and 'frame_range' not in kernels
    assert len(kernels) == len(a.detector().plan(False).launches())
    # the batched detector
    frames = np.stack([raw, raw[::-1], np.zeros_like(raw)])
    filtered = I.ingest(frames, median=True, mirror=True)[0]
    cubes = np.tile(np.float32(cube), (3, 1))
    det = FrameDetector(rt, H, W, FX, FY, 3, sensor=dict(dtype='uint16', median=True, mirror=True))
    coms, sizes, found, _, _ = det.run(frames, cubes, do_hand_size=True)
    c0, s0, f0 = find_hands(filtered, cubes, FX, FY, do_hand_size=True, runtime=rt)
    assert list(found) == list(f0) == [True, True, False]
    assert np.array_equal(coms, c0) and np.array_equal(sizes, s0)
    with pytest.raises(ValueError):
        det.run(filtered, cubes)


# ---- 7: the public API -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('dtype', ['uint16', 'float32'])
def test_filter_depth(backend, dtype):
    from util.cameradevice import filter_depth
    rt = get_runtime(backend)
    a = _raw(dtype, (2, 37, 53))
    for median, mirror in FLAGS:
        ref, mn, mx = _ref(dtype, (2, 37, 53), median, mirror)
        out, rng = filter_depth(a, median=median, mirror=mirror, runtime=rt, return_range=True)
        assert out.dtype == np.float32 and np.array_equal(out, ref) and np.array_equal(rng, np.stack([mn, mx], axis=1))
        one, r1 = filter_depth(a[1], median=median, mirror=mirror, runtime=rt, return_range=True)
        assert one.shape == (37, 53) and np.array_equal(one, ref[1]) and np.array_equal(r1, np.float32([mn[1], mx[1]]))
    assert np.array_equal(filter_depth(a, runtime=rt), _ref(dtype, (2, 37, 53), True, False)[0])       # defaults: median on, mirror off
    with pytest.raises(ValueError):
        filter_depth(a.astype(np.int32), runtime=rt)
    with pytest.raises(ValueError):
        filter_depth(a[0, 0], runtime=rt)


def _icvl_files(tmp_path, n=4, seed=35):
    from tests.test_realtime import _write_icvl_sequence
    cam, cube = A.Camera.icvl(), (250., 250., 250.)
    frames, coms = T.drifting_sequence(np.random.RandomState(seed), n, cam, 240, 320, cube)
    frames[1][np.random.RandomState(5).uniform(size=frames[1].shape) < 0.01] = 3000.
    base = str(tmp_path / 'ICVL')
    frames, _ = _write_icvl_sequence(base, 'test_seq_1', frames, coms, cam)
    files = [os.path.join(base, 'Depth', '201403121135', 'test_seq_1_%04d.png' % i) for i in range(n)]
    return base, files, frames, coms


@pytest.mark.parametrize('backend', BACKENDS)
def test_filtered_device_over_a_file_device(backend, tmp_path):
    from PIL import Image
    from util.cameradevice import FileDevice, FilteredDevice
    R.set_default_runtime(get_runtime(backend))
    base, files, frames, _ = _icvl_files(tmp_path)
    Image.fromarray(np.zeros((240, 320), np.uint16)).save(files[3])            # a frame without any depth
    di = ICVLImporter(base, useCache=False)
    dev = FilteredDevice(FileDevice(files, di))
    assert dev.mirror is False and dev.median is True
    dev.start()
    for i in range(3):
        ok, f = dev.getDepth()
        assert ok is True and f.dtype == np.float32 and np.array_equal(f, I.ingest(frames[i], median=True)[0]), i
    ok, f = dev.getDepth()
    assert ok is False and not f.any()
    assert dev.getLastDepthNum() == 4 and np.array_equal(dev.getDepthIntrinsics(), dev.device.getDepthIntrinsics())
    assert dev.filenames is dev.device.filenames                                # everything else is the wrapped device's
    with pytest.raises(IndexError):
        dev.getDepth()
    dev.stop()
    dev = FilteredDevice(FileDevice(files, di, mirror=True), median=False)      # mirror=None: the wrapped device's
    assert dev.mirror is True
    assert np.array_equal(dev.getDepth()[1], frames[0][:, ::-1])
    assert FilteredDevice(FileDevice(files, di, mirror=True), mirror=False).mirror is False


@pytest.mark.parametrize('backend', BACKENDS)
def test_pipeline_with_a_sensor(backend, tmp_path):
    from tests.test_detect import _ListDevice
    from tests.test_realtime import _track_nets
    from util.cameradevice import FileDevice
    from util.realtimehandposepipeline import RealtimeHandposePipeline
    rt = get_runtime(backend)
    R.set_default_runtime(rt)
    base, files, frames, coms = _icvl_files(tmp_path)
    di = ICVLImporter(base, useCache=False)
    (snet, _, _), (pnet, _, _) = _track_nets(rt, backend, J=16)
    config = {'fx': FX, 'fy': FY, 'cube': (250, 250, 250)}
    filtered = I.ingest(frames, median=True)[0]
    want = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=coms[0]).processVideo(_ListDevice(list(filtered)))
    assert want.shape == (4, 16, 3)
    # the files as they are (float32 from the importer), filtered on the device
    rtp = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=coms[0], sensor=dict(dtype='float32', median=True))
    assert np.array_equal(rtp.processVideo(FileDevice(files, di)), want)
    # ... and as uint16
    u16 = [f.astype(np.uint16) for f in frames]
    rtp = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=coms[0], sensor=dict(dtype='uint16', median=True))
    assert np.array_equal(rtp.processVideo(_ListDevice(u16)), want)
    assert rtp._tracker.sensor == (np.dtype('uint16'), True, False)
    # the per-call route sees the same frame
    rtp2 = RealtimeHandposePipeline(pnet, dict(config), di, comrefNet=snet, init_com=coms[0], sensor=dict(dtype='uint16', median=True))
    rtp2.initNets()
    for i in range(2):
        crop, M, com3D = rtp2.detect(u16[i])
        assert np.array_equal(rtp2.estimatePose(crop, com3D) * config['cube'][2] / 2. + com3D, want[i]), i
    with pytest.raises(ValueError):
        rtp2.detect(frames[0])
    with pytest.raises(ValueError):
        rtp.processFrame(frames[0])


@pytest.mark.parametrize('backend', BACKENDS)
def test_examples_with_sensor_flags(backend, tmp_path):
    R.set_default_runtime(get_runtime(backend))
    base, _, _, _ = _icvl_files(tmp_path, n=2, seed=36)
    net = 'resnet' if backend == 'hip' else 'poseregnet'               # (the 128x128 ResNet is too slow for the SIMT emulator)
    mods = {}
    for name in ('test_realtimepipeline', 'realtime_sensor', 'realtime_detect'):       # (realtime_sensor runs test_realtimepipeline's own main)
        spec = importlib.util.spec_from_file_location('ingest_' + name, os.path.join(ROOT, 'examples', name + '.py'))
        mods[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    common = ['--dataset', 'icvl', '--data', base, '--net', net, '--cache', str(tmp_path / 'cache')]
    main = mods['realtime_sensor'].main
    plain, err0 = mods['test_realtimepipeline'].main(common)
    same, err1 = main(common)
    assert np.array_equal(same, plain) and err1 == err0               # without the flags: the plain example's output
    u16, err = main(common + ['--sensor-u16'])
    assert np.array_equal(u16, plain) and np.isfinite(err)            # the recorded frames are whole millimetres: the uint16 route loses nothing
    med, _ = main(common + ['--sensor-u16', '--median'])
    assert med.shape == (2, 16, 3) and np.isfinite(med).all() and not np.array_equal(med, plain)
    mir, err = main(common + ['--median', '--mirror'])
    assert mir.shape == (2, 16, 3) and np.isfinite(mir).all() and not np.array_equal(mir, med)
    assert mods['realtime_sensor'].base.FileDevice is mods['realtime_sensor'].FileDevice       # the example's names are put back
    poses, size = mods['realtime_detect'].main(common + ['--sensor-u16', '--median', '--mirror'])
    assert poses.shape == (2, 16, 3) and np.isfinite(poses).all() and len(size) == 3
