"""Guard bands for the kernel-parity tests (helpers only, no tests): an operand sits inside ONE allocation between two bands of sentinel
words, so that a store a kernel makes outside its problem lands in memory the test owns and can compare afterwards, and a load from
there returns a NaN that poisons whatever is computed from it.  The same code serves the emulator runtime and the MI355X runtime."""
import numpy as np

from hipdp.runtime import Buffer

f32 = np.float32
SENTINEL = np.uint32(0x7FC0DEAD)                            # a NaN: a canary that also poisons whatever reads it
_SBYTES = np.frombuffer(SENTINEL.tobytes(), np.uint8)       # its four bytes in memory order
BAND = 16384                                                # sentinel words per side: 64 KiB, more than a tile row of any kernel at test shapes


def _size(shape):
    return int(np.prod(shape)) if len(shape) else 1


def guarded(rt, arr=None, shape=None, dtype=f32, band=BAND, off=0):
    """(whole, view): one allocation of `band` sentinel words, the payload rounded up to 256 bytes, `band` sentinel words.  `view` is what a
    kernel gets: arr's (or shape's / dtype's) elements starting `off` ELEMENTS into the payload -- off = 0 is 16-byte aligned (256, in
    fact), off = 1 of a float32 operand is not.  The payload holds `arr`, or sentinel words for an output; so does its rounding slack."""
    if arr is not None:
        arr = np.ascontiguousarray(arr)
        shape, dtype = arr.shape, arr.dtype
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    dt = np.dtype(dtype)
    nbytes = _size(shape) * dt.itemsize
    start = band * 4 + off * dt.itemsize
    pay = -(-(off * dt.itemsize + max(nbytes, 1)) // 256) * 256
    words = np.full(band + pay // 4 + band, SENTINEL, np.uint32)
    if arr is not None:
        words.view(np.uint8)[start:start + nbytes] = arr.reshape(-1).view(np.uint8)
    whole = rt.upload(words.view(f32))                      # bits travel unchanged: uploads and downloads are plain copies
    assert whole.ptr % 16 == 0
    view = Buffer(rt, whole.ptr + start, shape, dt, whole.owner)
    view.keep = whole                                       # the helpers below find the allocation of a view here
    return whole, view


def _whole_bytes(whole):
    return whole.get().reshape(-1).view(np.uint8)


def fetch(view):
    """The view's elements as the device holds them now, whatever their dtype (a download of the whole allocation)."""
    raw = _whole_bytes(view.keep)
    lo = view.ptr - view.keep.ptr
    return raw[lo:lo + view.nbytes].copy().view(view.dtype).reshape(view.shape)


def band_damage(whole, view, raw=None):
    """None when every byte of the allocation outside the view still holds the sentinel pattern, else (first, last) damaged byte offset
    relative to the view's first byte (negative: in front of it).  raw: the allocation's bytes, when already downloaded."""
    raw = _whole_bytes(whole) if raw is None else raw
    bad = raw != np.resize(_SBYTES, raw.size)
    lo = view.ptr - whole.ptr
    bad[lo:lo + view.nbytes] = False
    at = np.flatnonzero(bad)
    return None if at.size == 0 else (int(at[0]) - lo, int(at[-1]) - lo)


def bands_intact(whole, view):
    return band_damage(whole, view) is None


def sentinel_mask(a):
    """Which elements of `a` still look like part of a sentinel word.  32-bit elements: the word itself.  uint16 / uint8 elements: one of the
    word's halves / bytes -- usable where no valid value equals one (argmax bytes < 4, tie masks < 512)."""
    a = np.asarray(a)
    if a.dtype.itemsize == 4:
        return np.ascontiguousarray(a).view(np.uint32) == SENTINEL
    part = np.frombuffer(SENTINEL.tobytes(), a.dtype)
    assert a.dtype.itemsize in (1, 2)
    return np.isin(a, part)


def all_written(a):
    """No sentinel word remains in (the valid region) `a` of a downloaded output."""
    return not sentinel_mask(a).any()


def untouched(a):
    """Every element of `a` (padding columns, rows a row map skips) still is the sentinel.  32-bit elements only."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return bool((a.view(np.uint32) == SENTINEL).all())


def unchanged(view, arr):
    """Bit comparison of an input with what was uploaded into it."""
    arr = np.ascontiguousarray(arr, dtype=view.dtype)
    return fetch(view).reshape(-1).view(np.uint8).tobytes() == arr.reshape(-1).view(np.uint8).tobytes()


class Guards(object):
    """The guarded operands of one launch (or a few): inp() / out() hand out views, check() asserts that every band is intact and
    every input still holds the bits it was given."""

    def __init__(self, rt):
        self.rt, self.items = rt, []

    def inp(self, arr, off=0, name=None, dtype=f32):
        arr = np.ascontiguousarray(arr, dtype=dtype)
        whole, view = guarded(self.rt, arr, off=off)
        self.items.append((name or 'input %d' % len(self.items), whole, view, arr))
        return view

    def out(self, shape, dtype=f32, off=0, name=None, init=None):
        """An output full of sentinel words -- or holding `init` (an accumulator, a residual aliasing the output)."""
        whole, view = guarded(self.rt, None if init is None else np.ascontiguousarray(init, dtype=dtype), shape=shape, dtype=dtype, off=off)
        self.items.append((name or 'output %d' % len(self.items), whole, view, None))
        return view

    def check(self):
        for name, whole, view, arr in self.items:
            raw = _whole_bytes(whole)
            bad = band_damage(whole, view, raw)
            assert bad is None, "%s (shape %r, %s): bytes %d .. %d relative to its first byte were written" % ((name, view.shape, view.dtype) + bad)
            if arr is not None:
                lo = view.ptr - whole.ptr
                assert raw[lo:lo + view.nbytes].tobytes() == arr.reshape(-1).view(np.uint8).tobytes(), "%s (shape %r): an input was modified" % (name, view.shape)


NAN = SENTINEL.view(f32)                                   # the sentinel as a float32 value, to plant in inputs


def padded(a, ld, fill=None):
    """A [rows][cols] matrix laid out with leading dimension `ld`: the padding columns hold `fill` (default: the sentinel NaN)."""
    a = np.asarray(a)
    rows, cols = a.shape
    out = np.full((rows, ld), SENTINEL, np.uint32).view(f32) if fill is None else np.full((rows, ld), fill, f32)
    out[:, :cols] = a
    return out
