"""TEST INFRASTRUCTURE ONLY: NumPy restatements of the HandDetector crop helpers for tests/test_crop_helpers.py.

  bilinear_resize_ref   HandDetector.bilinearResize (/root/reference/src/util/handdetector.py:132-202) as the reference computed it
                        on NumPy 1: a float32 element times a Python float is a float64 there, so the weights and the weighted sum
                        are float64 and the result is rounded once to float32.  Vectorised, the same operations in the same order;
                        pinned bit for bit to the reference's own function by tests/golden/resize.npz (make_golden_r7.py).
  window                getCrop (:260-296) with applyCrop3D's options (pad value, z-threshold on / off).
  crop_area_3d_ref      cropArea3D (:382-490) under RESIZE_BILINEAR: oracle.augment's window -> bilinear_resize_ref -> paste.
  apply_crop_3d_ref     applyCrop3D (:353-380): window -> resize -> paste.
  inverse_crop_ref      getInverseCrop (:298-334) for nearest neighbour (oracle.augment.resize_nn) or bilinear_resize_ref.
  recrop_ref            recropHand (:782-803) for any target size from oracle.augment's warp pieces.
applyCrop3D and cropArea3D are composed here rather than run from the reference: their Python-2 integer divisions change meaning
under the lib2to3 import.
"""
import numpy as np

from oracle import augment as A


def bilinear_resize_ref(src, dsize, nd):
    src = np.asarray(src, np.float32)
    sh, sw = src.shape
    dw, dh = int(dsize[0]), int(dsize[1])
    x_ratio = float(sw - 1) / dw
    y_ratio = float(sh - 1) / dh
    fy = np.arange(dh, dtype=np.float64) * y_ratio
    fx = np.arange(dw, dtype=np.float64) * x_ratio
    y = fy.astype(np.int64)
    x = fx.astype(np.int64)
    if sw < 2 or sh < 2 or (x + 1 >= sw).any() or (y + 1 >= sh).any():
        raise UserWarning("Shape mismatch")
    y_diff = (fy - y)[:, None]
    x_diff = (fx - x)[None, :]
    y_diff_2 = 1. - y_diff
    x_diff_2 = 1. - x_diff
    y2x2 = y_diff_2 * x_diff_2
    y2x = y_diff_2 * x_diff
    yx2 = y_diff * x_diff_2
    yx = y_diff * x_diff
    a = src[y][:, x].astype(np.float64)
    b = src[y][:, x + 1].astype(np.float64)
    c = src[y + 1][:, x].astype(np.float64)
    d = src[y + 1][:, x + 1].astype(np.float64)
    nd32 = np.float32(nd)
    na, nb, nc, n4 = (src[y][:, x] == nd32), (src[y][:, x + 1] == nd32), (src[y + 1][:, x] == nd32), (src[y + 1][:, x + 1] == nd32)
    many = (na.astype(int) + nb + nc + n4) > 2
    y2x2 = np.where(na, 0., y2x2)
    y2x = np.where(na, 1. - yx - yx2, y2x)
    y2x = np.where(nb, 0., y2x)
    y2x2 = np.where(nb & (y2x2 != 0.), 1. - yx - yx2, y2x2)
    yx2 = np.where(nc, 0., yx2)
    yx = np.where(nc, 1. - y2x - y2x2, yx)
    yx = np.where(n4, 0., yx)
    yx2 = np.where(n4 & (yx2 != 0.), 1. - y2x - y2x2, yx2)
    zero = (y2x2 == 0.) & (y2x == 0.) & (yx2 == 0.) & (yx == 0.)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        sc = np.where(zero, 1., 1. / (yx + yx2 + y2x + y2x2))
        y2x2 = np.where(zero, y2x2, y2x2 * sc)
        y2x = np.where(zero, y2x, y2x * sc)
        yx2 = np.where(zero, yx2, yx2 * sc)
        yx = np.where(zero, yx, yx * sc)
        zero = (y2x2 == 0.) & (y2x == 0.) & (yx2 == 0.) & (yx == 0.)
        val = y2x2 * a + y2x * b + yx2 * c + yx * d
    out = np.where(zero | many, np.float64(nd32), val)
    return out.astype(np.float32)


def resize(src, sz, bilinear, nd=0.):
    return bilinear_resize_ref(src, sz, nd) if bilinear else A.resize_nn(np.asarray(src, np.float32), sz)


def window(dpt, xstart, xend, ystart, yend, zstart, zend, thresh_z=True, background=0.):
    """getCrop: the window of dpt padded with `background` where it leaves the frame, then (thresh_z) the z-threshold."""
    if thresh_z:
        return A.get_crop(dpt, xstart, xend, ystart, yend, zstart, zend, background=background)
    H, W = dpt.shape
    cropped = dpt[max(ystart, 0):min(yend, H), max(xstart, 0):min(xend, W)].copy()
    return np.pad(cropped, ((abs(ystart) - max(ystart, 0), abs(yend) - min(yend, H)),
                            (abs(xstart) - max(xstart, 0), abs(xend) - min(xend, W))), mode='constant', constant_values=background)


def _paste(rz, dsz, fill):
    ret = np.ones((dsz, dsz), np.float32) * np.float32(fill)
    xs = int(np.floor(dsz / 2. - rz.shape[1] / 2.))
    ys = int(np.floor(dsz / 2. - rz.shape[0] / 2.))
    ret[ys:ys + rz.shape[0], xs:xs + rz.shape[1]] = rz
    return ret


def _size(bounds, dsz, stretch=False):
    xstart, xend, ystart, yend = bounds[:4]
    wb, hb = xend - xstart, yend - ystart
    if stretch:
        return (dsz, dsz)
    return (dsz, hb * dsz // wb) if wb > hb else (wb * dsz // hb, dsz)


def crop_area_3d_ref(frame, com, cube, fx, fy, dsz, nd, stretch=False):
    """cropArea3D's crop (docom=False) under RESIZE_BILINEAR around a float32 centre, in mm."""
    d, _, _ = A.detector_preprocess(frame)
    b = A.com_to_bounds(np.asarray(com, np.float32), np.asarray(cube, np.float32), fx, fy)
    cropped = A.get_crop(d, *b)
    rz = bilinear_resize_ref(cropped, _size(b, dsz, stretch), nd)
    return rz if stretch else _paste(rz, dsz, nd)


def apply_crop_3d_ref(dpt, com, size, fx, fy, dsz, nd, bilinear, thresh_z=True, background=None):
    """applyCrop3D around a float32 centre: background=None pads with numpy.pad's None value and fills with nd."""
    b = A.com_to_bounds(np.asarray(com, np.float32), np.asarray(size, np.float32), fx, fy)
    pad = background
    if background is None:
        pad = np.pad(np.zeros((1, 1), np.float32), ((1, 0), (0, 0)), mode='constant', constant_values=None)[0, 0]
    cropped = window(np.asarray(dpt, np.float32), *b, thresh_z=thresh_z, background=pad)
    rz = resize(cropped, _size(b, dsz), bilinear, nd)
    return _paste(rz, dsz, nd if background is None else background)


def inverse_crop_ref(crop, sz, xstart, xend, ystart, yend, zstart, zend, thresh_z=True, background=0., bilinear=False, nd=0.):
    crop = np.asarray(crop, np.float32)
    dpt = np.ones(sz, dtype=np.float32) * np.float32(background)
    H, W = dpt.shape
    if (xend < 0 and xstart < 0) or (yend < 0 and ystart < 0):
        return dpt
    if (xend > W and xstart > W) or (yend > H and ystart > H):
        return dpt
    if xend == xstart or yend == ystart:
        return dpt
    cropped = resize(crop, (xend - xstart, yend - ystart), bilinear, nd)
    dpt[max(ystart, 0):min(yend, H), max(xstart, 0):min(xend, W)] = \
        cropped[max(-ystart, 0):cropped.shape[0] - max(yend - H, 0), max(-xstart, 0):cropped.shape[1] - max(xend - W, 0)]
    if thresh_z:
        z0, z1 = np.float32(zstart), np.float32(zend)
        msk1 = np.logical_and(dpt < z0, dpt != 0)
        msk2 = np.logical_and(dpt > z1, dpt != 0)
        dpt[msk1] = z0
        dpt[msk2] = 0.
    return dpt


def recrop_ref(crop, M, Mnew, target_size, background=0., nv_val=0., zrange=None):
    """recropHand with the augmentation's warp pieces (oracle.augment: mat3_mul, invert_3x3, warp_perspective_coords)."""
    crop = np.asarray(crop, np.float32)
    X, Y = A.warp_perspective_coords(A.invert_3x3(A.mat3_mul(M, Mnew)), int(target_size[0]), int(target_size[1]))
    warped = A._gather(crop, X, Y, border=float(background))
    warped[np.abs(warped.astype(np.float64) - nv_val) <= 1e-8 + 1e-5 * abs(nv_val)] = background
    if zrange is not None:
        z0, z1 = np.float32(zrange[0]), np.float32(zrange[1])
        msk1 = np.logical_and(warped < z0, warped != 0)
        msk2 = np.logical_and(warped > z1, warped != 0)
        warped[msk1] = z0
        warped[msk2] = 0.
    return warped
