"""NumPy restatement of what the reference's live depth source does to a frame (CreativeCameraDevice.getDepth,
src/util/cameradevice.py:189-200 of the reference): optional mirror, cv2.medianBlur(depth, 3), conversion to float32.  medianBlur
replicates the border, as scipy.ndimage.median_filter(size=3, mode='nearest') does; tests/test_ingest.py pins median3 to the latter."""
import numpy as np


def median3(a):
    """3x3 median with a replicated border over the last two axes of `a` ((H, W) or (B, H, W)); keeps the dtype."""
    a = np.asarray(a)
    H, W = a.shape[-2:]
    pad = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)], mode='edge')
    stack = np.stack([pad[..., dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    return np.sort(stack, axis=0)[4].astype(a.dtype)


def ingest(raw, median=False, mirror=False):
    """(float32 frames, min, max) of raw (H, W) or (B, H, W): mirror, then the median, then float32 -- the reference's order.  min / max
    are per frame ((B,) arrays; scalars for one (H, W) frame)."""
    a = np.asarray(raw)
    if mirror:
        a = a[..., ::-1]
    if median:
        a = median3(a)
    out = np.ascontiguousarray(a, np.float32)
    return out, out.min(axis=(-2, -1)), out.max(axis=(-2, -1))


def u16_frames(rng, B, H, W):
    """Full-range uint16 frames with about 30 % zeros and some saturated pixels."""
    a = rng.randint(0, 65536, (B, H, W)).astype(np.uint16)
    u = rng.random_sample((B, H, W))
    a[u < 0.30] = 0
    a[u > 0.97] = 65535
    return a


def f32_frames(rng, B, H, W):
    """float32 frames of multiples of 37.5 with many ties and a far value; no NaN, no -0.0."""
    a = (rng.randint(0, 40, (B, H, W)) * 37.5).astype(np.float32)
    a[rng.random_sample((B, H, W)) > 0.95] = np.float32(32001.0)
    return a
