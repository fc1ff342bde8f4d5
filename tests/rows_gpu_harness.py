"""What the GPU tests of the eight row libraries share (tests/test_sm_bluestein_gpu.py, test_sm_czt_gpu.py, test_sm_rowconv_gpu.py,
test_sm_rowconv_real_gpu.py, test_sm_dct_gpu.py, test_sm_hilbert_gpu.py, test_sm_mdct_gpu.py, test_sm_stft_gpu.py): random rows, the
bits of an array, the upload of one, the guarded output buffer and its check, and the record of the worst figures of a run.  Each
file's run(), bounds and row norm stay its own: the bounds are relative to different things per library.  A plain module: no tests, no
fixtures.  `sm` is smfft_amd, or tests/host_device.HOST in its place (tests/test_rows_gpu_harness_cpu.py)."""
import numpy as np

from tests.fir_gpu_harness import GUARD


def rand(rng, shape, dtype=np.float32):
    """standard normal rows of float32, or of complex64 with standard normal parts"""
    if np.dtype(dtype).kind == "c":
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)
    return rng.standard_normal(shape).astype(dtype)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def upload(sm, a):
    """a device buffer of exactly a.nbytes with a in it (DeviceBuffer.from_host rounds 4 bytes up to 8)"""
    a = np.ascontiguousarray(a)
    buf = sm.DeviceBuffer(a.nbytes)
    assert buf.nbytes == a.nbytes and sm.lib.smfft_memcpy_h2d(buf.ptr, a.ctypes.data, a.nbytes) == 0
    return buf


def guarded(sm, count, elem_bytes, front=0):
    """a device buffer of [GUARD + front | count | GUARD] elements of elem_bytes: 0x5A, 0xFF, 0x5A; returns (buffer, the payload's
    address).  front: elements between the front guard and the payload's base"""
    front += GUARD
    buf = sm.DeviceBuffer((front + count + GUARD) * elem_bytes)
    assert sm.lib.smfft_memset(buf.ptr, 0x5A, buf.nbytes) == 0
    if count:
        assert sm.lib.smfft_memset(buf.ptr + elem_bytes * front, 0xFF, elem_bytes * count) == 0
    return buf, buf.ptr + elem_bytes * front


def collect(buf, count, dtype, front=0, finite=True):
    """the payload of a guarded(sm, count, itemsize of dtype, front) buffer as `count` elements of dtype, after checking that both
    guards are untouched and (finite) that no NaN of the prefill is left"""
    e = np.dtype(dtype).itemsize
    front += GUARD
    raw = buf.to_host(np.uint8, ((front + count + GUARD) * e,))
    assert np.all(raw[:e * front] == 0x5A), "the kernel wrote in front of its output"
    assert np.all(raw[e * (front + count):] == 0x5A), "the kernel wrote past its output"
    out = raw[e * front:e * (front + count)].view(dtype).copy()
    if finite:
        assert np.all(np.isfinite(out.view(np.float32))), "outputs left unwritten"
    return out


class Worst:
    """the worst row figures measured in a run, per key (a length, a kind): what the tests print in front of their assertions"""

    def __init__(self):
        self.seen = {}

    def record(self, key, l2, mx):
        """takes the per-row relL2 and max figures of one check in; returns [worst relL2, worst max] of `key` so far"""
        worst = self.seen.setdefault(key, [0.0, 0.0])
        worst[0], worst[1] = max(worst[0], float(l2.max())), max(worst[1], float(mx.max()))
        return worst
