"""TEST INFRASTRUCTURE ONLY: a runtime with the same interface as hipdp.runtime.TorchHipRuntime whose
"device" memory is host memory and whose library is the emulator build of the kernel sources
(tests/emu/_build/libdpp_emu.so).  Lets the CPU-only test tier drive the real kernel code.  Every allocation is guarded: sentinel bands
on both sides, compared at every synchronize() and download(), so a kernel that stores outside an operand fails the test that ran it."""
import os
import subprocess
import weakref

import numpy as np

from hipdp import lib as _lib
from hipdp.runtime import Buffer

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EMU_LIB = os.path.join(ROOT, 'tests', 'emu', '_build', 'libdpp_emu.so')


def build_emulator():
    """make emu (a no-op when the library is newer than the kernel sources), under a file lock: several test processes may ask."""
    import fcntl
    os.makedirs(os.path.dirname(EMU_LIB), exist_ok=True)
    with open(os.path.join(os.path.dirname(EMU_LIB), '.lock'), 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            subprocess.check_call(['make', '-s', '-j8', '-C', os.path.join(ROOT, 'deep-prior-pp_amd', 'csrc'), 'emu'])
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return EMU_LIB


BAND = 4096                                                 # guard bytes on each side of every allocation
_SENTINEL = np.frombuffer(np.uint32(0x7FC0DEAD).tobytes(), np.uint8)       # a NaN word: poisons whatever reads it as float32
_BAND_BYTES = {}                                            # band length -> the bytes an intact band holds


def _band_bytes(n):
    """n bytes of the sentinel pattern ENDING on a word boundary (n = 4096 + the 64-byte alignment slack in front of the payload)."""
    if n not in _BAND_BYTES:
        _BAND_BYTES[n] = np.resize(_SENTINEL, n + 3)[(-n) % 4:][:n].tobytes()
    return _BAND_BYTES[n]


class EmuRuntime(object):
    def __init__(self):
        build_emulator()
        self.lib = _lib.load(EMU_LIB)
        self.stream = None
        self.is_emulator = True
        self.has_side_stream = False
        self._live = {}                           # id(raw) -> (weak reference to raw, payload offset, payload bytes, shape, dtype)

    def alloc(self, shape, dtype=np.float32, zero=True):
        """Every buffer lies between two bands of >= BAND bytes of 0x7FC0DEAD words which synchronize() and download() compare: a kernel
        that stores outside an operand fails the test that launched it, and one that loads from there computes NaN."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = max(1, int(np.prod(shape)))
        nbytes = n * np.dtype(dtype).itemsize
        tail = BAND + (-nbytes) % 4               # the band behind the payload starts on a word boundary of the pattern too
        raw = np.empty(BAND + 64 + nbytes + tail, np.uint8)
        off = BAND + (-(raw.ctypes.data + BAND)) % 64
        raw[:off] = np.frombuffer(_band_bytes(off), np.uint8)
        raw[off + nbytes:] = np.frombuffer(_band_bytes(raw.size - off - nbytes), np.uint8)
        arr = raw[off:off + nbytes].view(dtype)
        arr.view(np.uint8)[:] = 0 if zero else 0x7F      # poison: 0x7F7F7F7F = 3.4e38 as float32 (0x7F for uint8)
        key = id(raw)
        self._live[key] = (weakref.ref(raw, lambda _, key=key, live=self._live: live.pop(key, None)), off, nbytes, shape, np.dtype(dtype))
        return Buffer(self, arr.ctypes.data, shape, dtype, (raw, arr))

    def check_bands(self):
        """AssertionError if anything was stored into the guard bands of a live allocation."""
        while True:
            try:
                live = list(self._live.items())
                break
            except RuntimeError:                  # a buffer was released (its weak reference's callback) or allocated by another thread meanwhile
                continue
        for key, (ref, off, nbytes, shape, dtype) in live:
            raw = ref()
            if raw is None:
                continue
            if raw[:off].tobytes() == _band_bytes(off) and raw[off + nbytes:].tobytes() == _band_bytes(raw.size - off - nbytes):
                continue
            self._live.pop(key, None)             # reported once: the failing test's traceback may keep the buffer alive into later tests
            want = np.concatenate([np.frombuffer(_band_bytes(off), np.uint8), raw[off:off + nbytes],
                                   np.frombuffer(_band_bytes(raw.size - off - nbytes), np.uint8)])
            at = np.flatnonzero(raw != want)
            raise AssertionError("a kernel wrote outside a buffer of shape %r, dtype %s (%d bytes): bytes %d .. %d relative to its first byte"
                                 % (shape, dtype, nbytes, int(at[0]) - off, int(at[-1]) - off))

    def upload(self, arr, dtype=None):
        arr = np.ascontiguousarray(arr, dtype=dtype or arr.dtype)
        b = self.alloc(arr.shape, arr.dtype, zero=False)
        self.copy_in(b, arr)
        return b

    def _arr(self, buf):
        raw, arr = buf.owner
        off = buf.ptr - arr.ctypes.data
        return arr.view(np.uint8)[off:off + buf.nbytes].view(buf.dtype)

    def tensor(self, buf):
        import torch
        return torch.from_numpy(self._arr(buf))

    def copy_in(self, buf, arr):
        arr = np.ascontiguousarray(arr, dtype=buf.dtype).reshape(-1)
        assert arr.size == buf.size, (arr.shape, buf.shape)
        self._arr(buf)[:] = arr

    def download(self, buf):
        self.check_bands()
        return self._arr(buf).reshape(buf.shape).copy()

    def zero(self, buf):
        self._arr(buf)[:] = 0

    def read_async(self, buf):
        val = self.download(buf)            # the emulator has already executed everything queued

        class _Done(object):
            def get(self_inner):
                return val
        return _Done()

    def copy(self, dst, src):
        self._arr(dst)[:] = self._arr(src)

    def download_async(self, buf, host=None):
        return self.read_async(buf), None

    # the stream-ordered upload interface of NetBase._compute_output_pipelined: everything executes in issue order here, so the events
    # are placeholders -- what the CPU tier exercises is the control flow (staging slots, padding of the last batch, late output reads)
    def staged_upload(self, buf, host, free_event=None):
        self.copy_in(buf, np.asarray(host).reshape(buf.shape) if np.asarray(host).size == buf.size else host)
        return object()

    def record_event(self):
        return object()

    def wait_event(self, ev):
        pass

    def synchronize(self):
        self.check_bands()
