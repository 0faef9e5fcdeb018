"""HandDetector crop helpers on the device (csrc/crop.hip, ABI v12): bilinearResize, resizeCrop, recropHand, getInverseCrop,
applyCrop3D and cropArea3D under resizeMethod = RESIZE_BILINEAR, and their batched forms.  The bilinear restatement
(tests/crop_ref.py) is pinned to the reference's own functions by tests/golden/resize.npz; the kernels are held to it and to
oracle/augment.py bit for bit.  Every body runs on the SIMT emulator (CPU tier) and on the MI355X (-m gpu)."""
import os

import numpy as np
import pytest

from oracle import augment as A
from tests import crop_ref as R
from tests.backends import BACKENDS, get_runtime

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resize.npz')


def _use(backend):
    from hipdp import runtime as RT
    rt = get_runtime(backend)
    RT.set_default_runtime(rt)
    return rt


def _hd(frame, fx=241.42, fy=241.42, method=None):
    from util.handdetector import HandDetector
    hd = HandDetector(np.asarray(frame, np.float32).copy(), fx, fy)
    if method is not None:
        hd.resizeMethod = method
    return hd


def _golden_bilinear():
    g = np.load(GOLDEN)
    return [(g['bl_src_%d' % i], tuple(int(v) for v in g['bl_dsize_%d' % i]), float(g['bl_nd_%d' % i]), g['bl_out_%d' % i])
            for i in range(int(g['bl_n']))]


def _golden_inverse():
    g = np.load(GOLDEN)
    out = []
    for i in range(int(g['inv_n'])):
        b = g['inv_bounds_%d' % i]
        out.append((g['inv_crop_%d' % i], tuple(int(v) for v in g['inv_sz_%d' % i]), tuple(int(v) for v in b[:4]), float(b[4]), float(b[5]),
                    bool(g['inv_thresh_%d' % i]), float(g['inv_bg_%d' % i]), g['inv_out_%d' % i]))
    return out, float(g['inv_nd'])


def _check_restatement():
    """bilinear_resize_ref and the bilinear getInverseCrop composition equal the reference's own outputs bit for bit."""
    for src, dsize, nd, ref in _golden_bilinear():
        out = R.bilinear_resize_ref(src, dsize, nd)
        assert out.dtype == np.float32 and np.array_equal(out, ref)
    cases, nd = _golden_inverse()
    for crop, sz, b, z0, z1, thresh, bg, ref in cases:
        out = R.inverse_crop_ref(crop, sz, *b, z0, z1, thresh_z=thresh, background=bg, bilinear=True, nd=nd)
        assert np.array_equal(out, ref)
    # the fixture reaches every rule: undefined-tap outputs, the all-zero case and interpolated values
    assert any((ref == 0.).any() and (ref != 0.).any() for _, _, _, ref in _golden_bilinear())
    with pytest.raises(UserWarning):
        R.bilinear_resize_ref(np.ones((4, 1), np.float32), (3, 3), 0.)


@pytest.mark.parametrize('backend', BACKENDS)
def test_bilinear_resize(backend):
    """The restatement against the reference's own outputs (resize.npz), then the device against both."""
    _check_restatement()
    from util.handdetector import HandDetector, resize_crops
    rt = _use(backend)
    for src, dsize, nd, ref in _golden_bilinear():
        out = HandDetector.bilinearResize(src, dsize, nd)
        assert out.dtype == np.float32 and out.shape == (dsize[1], dsize[0]) and np.array_equal(out, ref)
    rng = np.random.RandomState(3)
    crops = rng.uniform(300., 900., (5, 37, 29)).astype(np.float32)
    crops[rng.uniform(size=crops.shape) < 0.3] = 0.
    for sz in ((64, 48), (13, 11), (29, 37)):
        out = resize_crops(crops, sz, HandDetector.RESIZE_BILINEAR, 0., runtime=rt)
        for i in range(5):
            assert np.array_equal(out[i], R.bilinear_resize_ref(crops[i], sz, 0.)), (sz, i)
    for bad in (np.ones((6, 1), np.float32), np.ones((1, 6), np.float32)):
        with pytest.raises(UserWarning):
            HandDetector.bilinearResize(bad, (4, 4), 0.)
    # the C entry point refuses it too, without launching
    src, out = rt.upload(np.ones((1, 6, 1), np.float32)), rt.alloc((1, 4, 4))
    assert rt.lib.dpp_resize_crops(src.ptr, 1, 6, 1, 4, 4, 1, 0.0, out.ptr, rt.stream) == 10001


@pytest.mark.parametrize('backend', BACKENDS)
def test_resize_crop(backend):
    from util.handdetector import HandDetector, resize_crops
    rt = _use(backend)
    rng = np.random.RandomState(5)
    frame = rng.uniform(300., 900., (30, 40)).astype(np.float32)
    frame[:3, :3] = 2000.                                             # out of range: the most frequent undefined depth becomes 0
    crop = rng.uniform(300., 900., (21, 17)).astype(np.float32)
    crop[rng.uniform(size=crop.shape) < 0.25] = 0.
    hd = _hd(frame)
    assert hd.getNDValue() == 0.
    for sz in ((128, 128), (9, 30), (17, 21), (5, 4)):
        out = hd.resizeCrop(crop, sz)
        assert out.dtype == np.float32 and np.array_equal(out, A.resize_nn(crop, sz)), sz
    hd.resizeMethod = HandDetector.RESIZE_BILINEAR
    for sz in ((128, 128), (9, 30), (17, 21)):
        assert np.array_equal(hd.resizeCrop(crop, sz), R.bilinear_resize_ref(crop, sz, 0.)), sz
    with pytest.raises(UserWarning):
        hd.resizeCrop(crop[:, :1], (8, 8))
    hd.resizeMethod = HandDetector.RESIZE_CV2_LINEAR
    with pytest.raises(NotImplementedError):
        hd.resizeCrop(crop, (8, 8))
    crops = rng.uniform(300., 900., (4, 23, 31)).astype(np.float32)
    out = resize_crops(crops, (64, 50), HandDetector.RESIZE_CV2_NN, runtime=rt)
    for i in range(4):
        assert np.array_equal(out[i], A.resize_nn(crops[i], (64, 50)))


def _recrop_inputs(rng, cam, n, dsz=128, cube=(250., 250., 250.)):
    """Normalised crops from the augmentation's synthetic generator, turned back into mm, with their crop transforms."""
    imgs, com3d, cubes, M, _ = A.synthetic_augment_inputs(rng, n, cam, cube=cube, dsize=dsz)
    com = np.stack([cam.joint3DToImg(c) for c in com3d]).astype(np.float32)       # image coordinates, z in mm
    crops = (imgs * (cubes[:, 2] / 2.)[:, None, None] + com[:, 2][:, None, None]).astype(np.float32)
    return crops, com, cubes, M


@pytest.mark.parametrize('backend', BACKENDS)
def test_recrop_hand(backend):
    """recropHand / recrop_crops bit for bit against oracle.augment.recrop_hand (and its warp pieces for other target sizes)."""
    from util.handdetector import HandDetector, recrop_crops
    rt = _use(backend)
    rng = np.random.RandomState(17)
    cam = A.Camera.nyu()
    fx, fy = abs(cam.fx), abs(cam.fy)
    n = 6
    crops, com, cubes, M = _recrop_inputs(rng, cam, n, dsz=64)
    crops[:, 5:9, 5:9] = 32000.                                            # the nv_val rule
    crops[:, 20:23, 30:40] = (com[:, 2] - cubes[:, 2])[:, None, None]     # nearer than the cube
    crops[:, 40:44, 10:14] = (com[:, 2] + cubes[:, 2])[:, None, None]     # farther than the cube
    pairs = []
    for i in range(n):
        Minv = np.linalg.inv(M[i].astype(np.float64))
        if i % 3 == 0:       # moveCoM: crop transform of the moved centre
            nc = cam.joint3DToImg(cam.jointImgTo3D(com[i]) + rng.normal(0, 10., 3))
            Mnew = A.com_to_transform(nc, cubes[i], fx, fy, (64, 64))
        elif i % 3 == 1:     # scaleHand: crop transform of the scaled cube
            Mnew = A.com_to_transform(com[i], cubes[i] * 1.08, fx, fy, (64, 64))
        else:                # a general perspective map
            Mnew = A.com_to_transform(com[i], cubes[i], fx, fy, (64, 64)) + np.array([[0.01, 0.02, 0.3], [-0.015, 0., 0.2], [1e-4, -5e-5, 0.]])
        pairs.append((Mnew, Minv))
    hd = _hd(np.full((240, 320), 600., np.float32), fx, fy)
    for i, (Mnew, Minv) in enumerate(pairs):
        out = hd.recropHand(crops[i], Mnew, Minv, (64, 64), background_value=0., nv_val=32000., thresh_z=True, com=com[i], size=cubes[i])
        ref = A.recrop_hand(crops[i], Mnew, Minv, com[i], cubes[i], fx, fy, background_value=0., nv_val=32000.)
        assert out.dtype == np.float32 and np.array_equal(out, ref), i
    Ms = np.stack([p[0] for p in pairs])
    Mns = np.stack([p[1] for p in pairs])
    # batched, non-square target, a non-zero border value, with and without the z-threshold
    for ts, bg, thresh in (((64, 64), 0., True), ((80, 48), 0., True), ((48, 70), 700., True), ((64, 64), 0., False)):
        out = recrop_crops(crops, Ms, Mns, ts, com, cubes, fx, fy, background_value=bg, nv_val=32000., thresh_z=thresh, runtime=rt)
        assert out.shape == (n, ts[1], ts[0])
        for i in range(n):
            zr = A.com_to_bounds(com[i], cubes[i], fx, fy)[4:] if thresh else None
            assert np.array_equal(out[i], R.recrop_ref(crops[i], Ms[i], Mns[i], ts, bg, 32000., zr)), (ts, i)
            if ts == (64, 64) and bg == 0. and thresh:
                assert np.array_equal(out[i], A.recrop_hand(crops[i], Ms[i], Mns[i], com[i], cubes[i], fx, fy, 0., 32000.))
    # the ill-defined centre: comToBounds' z range is the detector's [minDepth, maxDepth]
    c0 = np.array([30., 40., 0.])
    frame = np.full((240, 320), 500., np.float32)
    frame[0, 0], frame[1, 1] = 420., 800.
    hd0 = _hd(frame, fx, fy)
    out = hd0.recropHand(crops[0], Ms[0], Mns[0], (64, 64), nv_val=32000., thresh_z=True, com=c0, size=cubes[0])
    assert np.array_equal(out, R.recrop_ref(crops[0], Ms[0], Mns[0], (64, 64), 0., 32000., (hd0.minDepth, hd0.maxDepth)))
    batched = recrop_crops(crops[:1], Ms[:1], Mns[:1], (64, 64), c0[None], cubes[:1], fx, fy, nv_val=32000., min_depth=hd0.minDepth,
                           max_depth=hd0.maxDepth, runtime=rt)
    assert np.array_equal(batched[0], out)
    with pytest.raises(AssertionError):
        hd.recropHand(crops[0], Ms[0], Mns[0], (64, 64), thresh_z=True, com=None)
    hd.resizeMethod = HandDetector.RESIZE_BILINEAR
    with pytest.raises(NotImplementedError):
        hd.recropHand(crops[0], Ms[0], Mns[0], (64, 64), com=com[0])


@pytest.mark.parametrize('backend', BACKENDS)
def test_inverse_crop(backend):
    from util.handdetector import HandDetector, inverse_crops
    rt = _use(backend)
    cases, nd = _golden_inverse()
    hd = _hd(np.full((40, 52), 600., np.float32), method=HandDetector.RESIZE_BILINEAR)
    assert hd.getNDValue() == nd
    for crop, sz, b, z0, z1, thresh, bg, ref in cases:
        out = hd.getInverseCrop(crop, sz, *b, z0, z1, thresh_z=thresh, background=bg)
        assert out.dtype == np.float32 and np.array_equal(out, ref), b
    hd.resizeMethod = HandDetector.RESIZE_CV2_NN
    for crop, sz, b, z0, z1, thresh, bg, _ in cases:
        out = hd.getInverseCrop(crop, sz, *b, z0, z1, thresh_z=thresh, background=bg)
        assert np.array_equal(out, R.inverse_crop_ref(crop, sz, *b, z0, z1, thresh_z=thresh, background=bg)), b
    # batched: every golden case in one launch (same crop size), both methods
    same = [c for c in cases if c[0].shape == (16, 16)]
    crops = np.stack([c[0] for c in same])
    bounds = np.array([c[2] + (c[3], c[4]) for c in same], np.float64)
    for method, bil in ((HandDetector.RESIZE_BILINEAR, True), (HandDetector.RESIZE_CV2_NN, False)):
        out = inverse_crops(crops, (40, 52), bounds, thresh_z=True, background=0., method=method, nd_value=nd, runtime=rt)
        for i, c in enumerate(same):
            assert np.array_equal(out[i], R.inverse_crop_ref(c[0], (40, 52), *c[2], c[3], c[4], True, 0., bil, nd)), (method, i)
    hd.resizeMethod = HandDetector.RESIZE_CV2_LINEAR
    with pytest.raises(NotImplementedError):
        hd.getInverseCrop(crops[0], (40, 52), 1, 20, 1, 20, 0., 1000.)


def _frames(rng, n, H=120, W=160):
    cam = A.Camera.nyu()
    frames, coms = A.synthetic_frames(rng, n, cam, H, W, (300., 300., 300.))
    return frames, coms, abs(cam.fx), abs(cam.fy)


@pytest.mark.parametrize('backend', BACKENDS)
def test_crop_area_3d_bilinear(backend):
    """cropArea3D with RESIZE_BILINEAR (with and without docom) and crop_frames(resize_method=RESIZE_BILINEAR) against
    oracle.augment's window -> bilinear restatement -> paste."""
    from util.handdetector import HandDetector, crop_frames
    rt = _use(backend)
    rng = np.random.RandomState(23)
    B = 4
    frames, coms, fx, fy = _frames(rng, B)
    cubes = np.tile(np.float32([300., 300., 300.]), (B, 1))
    cubes[1] = (240., 280., 260.)                                        # a non-square window
    for i in range(B):
        hd = _hd(frames[i], fx, fy, HandDetector.RESIZE_BILINEAR)
        nd = hd.getNDValue()
        crop, M, _ = hd.cropArea3D(com=coms[i], size=tuple(cubes[i]), dsize=(64, 64))
        assert crop.dtype == np.float32 and np.array_equal(crop, R.crop_area_3d_ref(frames[i], coms[i], cubes[i], fx, fy, 64, nd)), i
        crop_d, _, com_d = hd.cropArea3D(com=coms[i], size=tuple(cubes[i]), dsize=(64, 64), docom=True)
        ref_d = R.crop_area_3d_ref(frames[i], np.float32(com_d), cubes[i], fx, fy, 64, nd)
        assert np.array_equal(crop_d, ref_d), i
        _, _, com_nn = _hd(frames[i], fx, fy).cropArea3D(com=coms[i], size=tuple(cubes[i]), dsize=(64, 64), docom=True)
        assert np.array_equal(com_d, com_nn)                             # the re-centring itself does not depend on the resize
    # batched and normalised: the per-frame results, normalised like the training stacks
    nd = 0.
    crops, Ms = crop_frames(frames, coms, cubes, fx, fy, 64, normalize=True, nd_value=nd, runtime=rt, resize_method=HandDetector.RESIZE_BILINEAR)
    for i in range(B):
        ref = R.crop_area_3d_ref(frames[i], coms[i], cubes[i], fx, fy, 64, nd)
        assert np.array_equal(crops[i], A.normalize_crop(ref, coms[i][2], cubes[i][2])), i
    # the stretched window (the refinement net's input)
    rz, _ = crop_frames(frames, coms, cubes, fx, fy, 32, normalize=False, runtime=rt, stretch=True, resize_method=HandDetector.RESIZE_BILINEAR)
    for i in range(B):
        assert np.array_equal(rz[i], R.crop_area_3d_ref(frames[i], coms[i], cubes[i], fx, fy, 32, 0., stretch=True)), i
    with pytest.raises(UserWarning):                                    # a 1-pixel window
        crop_frames(frames[:1], coms[:1], np.float32([[0.5, 300., 300.]]), fx, fy, 64, runtime=rt, resize_method=HandDetector.RESIZE_BILINEAR)


@pytest.mark.parametrize('backend', BACKENDS)
def test_apply_crop_3d(backend):
    from util.handdetector import HandDetector
    _use(backend)
    rng = np.random.RandomState(29)
    frames, coms, fx, fy = _frames(rng, 3)
    coms[0, :2] = (4., 6.)                                               # the window leaves the frame: the pad value shows
    img = frames[1] * np.float32(1.0)
    img[::5, ::7] = 3000.                                                # beyond the detector's range: kept (no range test)
    size = (300., 300., 300.)
    for method in (HandDetector.RESIZE_CV2_NN, HandDetector.RESIZE_BILINEAR):
        hd = _hd(frames[2], fx, fy, method)
        nd = hd.getNDValue()
        for i in range(2):
            for thresh in (True, False):
                for bg in (None, 0., 650.):
                    out = hd.applyCrop3D(img if i else frames[0], coms[i], size, (64, 64), thresh_z=thresh, background=bg)
                    ref = R.apply_crop_3d_ref(img if i else frames[0], coms[i], size, fx, fy, 64, nd, method == HandDetector.RESIZE_BILINEAR,
                                              thresh_z=thresh, background=bg)
                    assert out.dtype == np.float32 and np.array_equal(out, ref, equal_nan=True), (method, i, thresh, bg)
                    if bg is None and i == 0:
                        assert np.isnan(out).any()                       # numpy.pad(constant_values=None) pads float32 with NaN
    hd.resizeMethod = HandDetector.RESIZE_CV2_LINEAR
    with pytest.raises(NotImplementedError):
        hd.applyCrop3D(frames[0], coms[0], size, (64, 64))


@pytest.mark.parametrize('backend', BACKENDS)
def test_crop_frames_default_is_unchanged(backend):
    """crop_frames with default arguments is still exactly one dpp_crop_prepare + dpp_crop_warp; dpp_crop_warp_ex with no flags
    gives the same crops."""
    from hipdp import ops
    from util.handdetector import crop_frames
    rt = _use(backend)
    rng = np.random.RandomState(31)
    frames, coms, fx, fy = _frames(rng, 3)
    cubes = np.tile(np.float32([300., 300., 300.]), (3, 1))
    out, Ms = crop_frames(frames, coms, cubes, fx, fy, 64, runtime=rt)
    fr, co, cu = rt.upload(frames), rt.upload(coms.astype(np.float32)), rt.upload(cubes)
    rec = rt.alloc(3 * rt.lib.dpp_crop_record_bytes(), np.uint8)
    M, o1, o2 = rt.alloc((3, 9)), rt.alloc((3, 64, 64)), rt.alloc((3, 64, 64))
    ops.crop_prepare(rt, fr, 3, 120, 160, co, cu, fx, fy, 64, rec, M)(rt.stream)
    ops.crop_warp(rt, fr, rec, 3, 120, 160, 64, o1, normalize=True, nd_value=0.)(rt.stream)
    ops.crop_warp_ex(rt, fr, rec, 3, 120, 160, 64, o2, flags=ops.CROP_NORMALIZE, nd_value=0.)(rt.stream)
    rt.synchronize()
    assert np.array_equal(out, o1.get()) and np.array_equal(o1.get(), o2.get())
    assert np.array_equal(Ms, M.get().reshape(3, 3, 3))


@pytest.mark.gpu
def test_working_size_on_gpu():
    """256 NYU-sized 480 x 640 frames through the bilinear crop and 256 recrops of 128 x 128 crops, every crop checked."""
    from util.handdetector import HandDetector, crop_frames, recrop_crops
    rt = _use('hip')
    rng = np.random.RandomState(37)
    cam = A.Camera.nyu()
    fx, fy = abs(cam.fx), abs(cam.fy)
    B = 256
    frames, coms = A.synthetic_frames(rng, B, cam, 480, 640, (300., 300., 300.))
    cubes = np.tile(np.float32([300., 300., 300.]), (B, 1))
    crops, _ = crop_frames(frames, coms, cubes, fx, fy, 128, normalize=False, runtime=rt, resize_method=HandDetector.RESIZE_BILINEAR)
    for i in range(B):
        assert np.array_equal(crops[i], R.crop_area_3d_ref(frames[i], coms[i], cubes[i], fx, fy, 128, 0.)), i
    mm, com, cb, M = _recrop_inputs(rng, cam, B, dsz=128)
    Mnew = np.stack([A.com_to_transform(cam.joint3DToImg(cam.jointImgTo3D(com[i]) + rng.normal(0, 8., 3)), cb[i], fx, fy) for i in range(B)])
    Minv = np.stack([np.linalg.inv(M[i].astype(np.float64)) for i in range(B)])
    out = recrop_crops(mm, Mnew, Minv, (128, 128), com, cb, fx, fy, nv_val=32000., runtime=rt)
    for i in range(B):
        assert np.array_equal(out[i], A.recrop_hand(mm[i], Mnew[i], Minv[i], com[i], cb[i], fx, fy, 0., 32000.)), i
