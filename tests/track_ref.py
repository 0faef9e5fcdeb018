"""NumPy restatement of the reference's realtime path, composed from the oracle's pinned pieces (oracle/augment.py):
HandDetector.track / refineCoMIterative (/root/reference/src/util/handdetector.py:504-567) and RealtimeHandposePipeline.detect /
estimatePose and the caller's de-normalisation (/root/reference/src/util/realtimehandposepipeline.py:296-370, :198).
tests/golden/track.npz (make_golden_r8.py: the reference's own code run on seeded inputs) pins it; the kernel and plan tests of
tests/test_realtime.py are held to it."""
import numpy as np

from oracle import augment as A

HAND_LEFT, HAND_RIGHT = 0, 1


def refine_inputs(rz_mm, size, com):
    """refineCoM's input construction (handdetector.py:640-669): the three arrays the net is handed."""
    got = []
    A.refine_com(rz_mm, size, com, lambda ins: (got.extend(np.array(a) for a in ins), np.zeros((1, 3), np.float32))[1])
    return got


def track(dpt, com, size, cam, fx, fy, net_forward, rsize=(128, 128)):
    """track(com, size, dsize=rsize, doHandSize=False) on the detector-preprocessed frame `dpt`: (new centre float32, the window
    resized as it is (mm), the full window)."""
    xstart, xend, ystart, yend, zstart, zend = A.com_to_bounds(com, size, fx, fy)
    cropped = A.get_crop(dpt, xstart, xend, ystart, yend, zstart, zend)
    rz = A.resize_nn(cropped, rsize)
    newCom3D = A.refine_com(rz, size, com, net_forward) + cam.jointImgTo3D(com)
    com2 = cam.joint3DToImg(newCom3D)
    if np.allclose(com2, 0.):
        com2[2] = cropped[cropped.shape[0] // 2, cropped.shape[1] // 2]
    return com2, rz, cropped


def is_lost(com):
    """The centre cannot be cropped around on the device: comToBounds' "CoM ill-defined" test (handdetector.py:204)."""
    return bool(np.isclose(com[2], 0.))


def detect_tail(dpt, loc, cube, cam, fx, fy, dsize):
    """detect() after track (realtimehandposepipeline.py:326-337): cropArea3D(com=loc) and the normalisation.  The clip of :334
    discards its result; the ND value is 0 after the constructor's zeroing.  Returns (normalised crop, M, com3D, crop in mm)."""
    crop, M, com = A.crop_area_3d(dpt, loc, cube, fx, fy, dsize)
    com3D = cam.jointImgTo3D(com)
    return normalize_tail(crop, com3D, cube), M, com3D, crop


def normalize_tail(crop_mm, com3D, cube):
    """:332-336 on a crop in mm: 0 -> far plane, (a clip whose result is discarded,) minus com3D[2], divided by cube[2] / 2."""
    sc = cube[2] / 2.
    out = np.asarray(crop_mm, np.float32).copy()
    out[out == 0] = com3D[2] + sc
    out.clip(com3D[2] - sc, com3D[2] + sc)
    out -= com3D[2]
    out /= sc
    return out


def pose_input(crop, hand):
    """estimatePose's net input (:347-351)."""
    crop = np.asarray(crop, np.float32)
    return (crop if hand == HAND_LEFT else crop[:, ::-1])[None, None].astype(np.float32)


def pose_signs(jts, hand, invX, invY):
    """estimatePose after the net (:354-370): invX negates column 1 and invY column 0, as the reference has it."""
    jj = np.asarray(jts, np.float32).reshape(-1, 3).copy()
    if invX:
        jj[:, 1] *= (-1.)
    if invY:
        jj[:, 0] *= (-1.)
    if hand == HAND_RIGHT:
        jj[:, 0] *= (-1.)
    return jj


def denormalize(jj, cube_z, com3D):
    """pose * cube[2] / 2. + com3D (:198, :272) on float32 arrays: a float32 multiply, divide and add."""
    f32 = np.float32
    return ((np.asarray(jj, f32) * f32(cube_z)) / f32(2.) + np.asarray(com3D, f32)).astype(f32)


def refine_com_iterative(dpt, com, num_iter, size, fx, fy, min_depth, max_depth):
    """refineCoMIterative (handdetector.py:546-567) with the depth sum of calculateCoM taken in float64 (oracle.calculate_com);
    float64 state, the reference's max(xstart, 0).  Returns (centre float64, ill_defined)."""
    com = np.asarray(com, np.float64).copy()
    for _ in range(num_iter):
        if np.isclose(com[2], 0.):
            return com, True
        xstart, xend, ystart, yend, zstart, zend = A.com_to_bounds(com, size, fx, fy)
        cropped = A.get_crop(dpt, xstart, xend, ystart, yend, np.float32(zstart), np.float32(zend))
        com = A.calculate_com(cropped, min_depth, max_depth)
        if np.allclose(com, 0.):
            com[2] = cropped[cropped.shape[0] // 2, cropped.shape[1] // 2]
        com[0] += max(xstart, 0)
        com[1] += max(ystart, 0)
    return com, False


def drifting_sequence(rng, n, cam, H, W, cube, step_px=3.0, step_mm=4.0):
    """A blob that drifts a few pixels and millimetres per frame, from synthetic_frames' ingredients: a far wall with holes, a
    hand-sized blob, pixels nearer than the cube's front face and beyond maxDepth.  Returns (frames [n][H][W], centres [n][3])."""
    frames = np.zeros((n, H, W), np.float32)
    coms = np.zeros((n, 3), np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    u, v, d = W * 0.45, H * 0.5, 600.
    shape = rng.normal(0, 30., (H, W))
    for i in range(n):
        f = np.full((H, W), 1400., np.float32) + rng.normal(0, 3., (H, W)).astype(np.float32)
        f[rng.uniform(size=(H, W)) < 0.05] = 0.
        r = cube[0] / 2. * cam.fx / d * 0.7
        blob = (xx - u) ** 2 + (yy - v) ** 2 < r * r
        f[blob] = (d + shape)[blob].astype(np.float32)
        stick = np.abs(xx - u - r / 2) < 3
        f[stick & (rng.uniform(size=(H, W)) < 0.5)] = np.float32(d - cube[2])
        f[rng.uniform(size=(H, W)) < 0.01] = 2500.
        frames[i] = f
        coms[i] = (u, v, d)
        u += rng.uniform(-step_px, step_px)
        v += rng.uniform(-step_px, step_px)
        d += rng.uniform(-step_mm, step_mm)
    return frames, coms
