"""The guarded device allocation of the buffer-bounds tests (tests/test_buffers_gpu.py, the bounds test of test_real_fir_gpu.py).  A
plain module: no tests, no fixtures."""
import numpy as np

GUARD = 128 * 1024             # bytes of guard on each side of every payload
POISON = 0x7FE5A5A5            # quiet NaN with a recognisable payload: guards and the bytes a call must leave alone


def poison(nbytes):
    return np.full(-(-nbytes // 4), POISON, np.uint32).view(np.uint8)[:nbytes].copy()


class Region:
    """One device allocation [guard | offset | payload | guard], all but the payload poisoned; `ptr` is the payload's address, `image`
    the bytes written to the whole allocation (with smfft_memcpy_h2d).  offset: bytes, a multiple of `align` (a float2 unless the
    caller's elements are smaller)."""

    def __init__(self, sm, payload, offset, align=8):
        assert offset >= 0 and offset % align == 0
        self.lo, self.n = GUARD + offset, len(payload)
        self.image = poison(self.lo + self.n + GUARD)
        self.image[self.lo:self.lo + self.n] = payload
        self.buf = sm.DeviceBuffer(len(self.image))
        assert sm.lib.smfft_memcpy_h2d(self.buf.ptr, self.image.ctypes.data, len(self.image)) == 0
        self.ptr = self.buf.ptr + self.lo

    def read(self):
        return self.buf.to_host(np.uint8, (len(self.image),))

    def outside_unchanged(self, whole):
        """the payload as it is now, after checking that nothing outside it (whole: nor inside it) differs from `image`"""
        now = self.read()
        keep = np.ones(len(now), bool)
        if not whole:
            keep[self.lo:self.lo + self.n] = False
        idx = np.flatnonzero((now != self.image) & keep)
        assert not len(idx), f"{len(idx)} bytes changed, the first at payload offset {int(idx[0]) - self.lo}"
        return now[self.lo:self.lo + self.n].copy()
