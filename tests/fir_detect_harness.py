"""What the GPU tests of the detected FIR filter banks share (tests/test_run_fir_detect_gpu.py; libsmfft_fir_detect.so, smfft_amd.fir_detect):
the guarded runs of the two launches, the fp64 reference shared between the tests, and the bounds.  A plain module: no tests, no
fixtures.  The signals, the fp64 reference, ROW_MAX and the prepared spectra are tests/fir_gpu_harness.py's, the complex bank's.

Every run goes into outputs prefilled with 0xFF (a NaN power, index -1) and followed by a guard of GUARD elements of 0x5A that must
stay untouched, and every index must lie in [0, K).

The bound.  The complex bank's rows pass |y - y64| <= E per element, E = ROW_MAX * max(max |y64 row|, ||h_k|| max |x_c|)
(tests/test_fir_gpu.py derives it).  With y = y64 + d, |d| <= E:  |y|^2 - |y64|^2 = 2 Re(conj(y64) d) + |d|^2, at most 2 |y64| E + E^2
in magnitude; the two roundings of fmaf(re, re, im * im) add at most 2^-23 p each, 2^-22 p in all (to first order p = p64).  So
|p - p64| <= 2 |y64| E + E^2 + 2^-22 p64 per element: no new tolerance."""
import functools

import numpy as np

from tests.fir_gpu_harness import MODES, ROW_MAX, Bank, _rand, _reference  # noqa: F401  (puts tools/ on the path)

GUARD = 4096
SIZES = (256, 512, 1024, 2048, 4096)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def power_bound(y64, x, h):
    """(C, K, L): the bound of |p - p64| per element for y64 = (C, K, L) from x = (C, L), h = (K, M)"""
    xm = np.max(np.abs(x), axis=1)                                     # (C,)
    hn = np.linalg.norm(h.astype(np.complex128), axis=1)               # (K,)
    ya = np.abs(y64)
    E = ROW_MAX * np.maximum(np.max(ya, axis=2), hn[None, :] * xm[:, None])[:, :, None]
    return 2 * ya * E + E * E + 2.0 ** -22 * ya * ya


def power64(y64):
    return y64.real * y64.real + y64.imag * y64.imag


@functools.lru_cache(maxsize=None)
def case(N, mode, M, K, C=2):
    """the shared case of the fp64 tests: C = 2 channels of L = 3 V + 5 samples and K filters of M taps, with its fp64 rows; computed
    once and never changed (the arrays are read-only)"""
    rng = np.random.default_rng(1000 * N + 10 * M + K + (mode == "correlate"))
    L = 3 * (N - M + 1) + 5
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    y64 = _reference(x, h, mode == "correlate")
    for a in (x, h, y64):
        a.setflags(write=False)
    return x, h, y64


class Detect:
    """libsmfft_fir_detect.so behind the calls its GPU tests need.  sm: smfft_amd; fd: smfft_amd.fir_detect"""

    def __init__(self, sm, fd):
        self.sm, self.fd, self.bank = sm, fd, Bank.complex(sm)

    def prepared(self, h, N, mode):
        """the main library's spectra of the taps h, (K, N) complex64 on the host"""
        return self.bank.prepared(np.ascontiguousarray(h), N, mode)

    # ---- guarded outputs ------------------------------------------------------------------------------------------------------
    def guarded(self, count, front=0):
        """a device buffer of [front | count | GUARD] 4-byte elements: 0x5A, 0xFF, 0x5A; returns (buffer, the payload's address)"""
        sm = self.sm
        buf = sm.DeviceBuffer((front + count + GUARD) * 4)
        assert sm.lib.smfft_memset(buf.ptr, 0x5A, buf.nbytes) == 0
        if count:
            assert sm.lib.smfft_memset(buf.ptr + 4 * front, 0xFF, 4 * count) == 0
        return buf, buf.ptr + 4 * front

    def collect(self, buf, count, dtype, front=0):
        """the payload of a guarded buffer after checking the guards"""
        raw = buf.to_host(np.uint8, ((front + count + GUARD) * 4,))
        assert np.all(raw[:4 * front] == 0x5A), "the kernel wrote in front of its output"
        assert np.all(raw[4 * (front + count):] == 0x5A), "the kernel wrote past its output"
        return raw[4 * front:4 * (front + count)].view(dtype).copy()

    def run(self, x, h, N, mode, spectra=None, which=("power", "peak"), finite=True, front=0, exact_signal=False, launch=None):
        """the launches named in `which` through the device-pointer API on one copy of the signal and the spectra; returns
        {"power": (C, K, L) float32, "peak": (C, L) float32, "index": (C, L) int32}.  front: elements between an allocation's start and
        the output's base (an interior pointer); exact_signal: the signal ends where its allocation ends (DeviceBuffer.from_host pads a
        tiny one to 8 bytes: a complex64 sample is 8 bytes, so it never does); launch(name, dx, dspec, outputs): how to launch, when not
        on the null stream through the mirror"""
        sm, fd = self.sm, self.fd
        x, h = np.ascontiguousarray(x), np.ascontiguousarray(h)
        assert x.dtype == np.complex64 and h.dtype == np.complex64
        (C, L), (K, M) = x.shape, h.shape
        if spectra is None:
            spectra = self.prepared(h, N, mode)
        dx, dspec = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(np.ascontiguousarray(spectra, dtype=np.complex64))
        assert not exact_signal or dx.nbytes == x.nbytes
        out, bufs = {}, [dx, dspec]
        try:
            if "power" in which:
                bp, pp = self.guarded(C * K * L, front)
                bufs.append(bp)
                if launch is None:
                    fd.power_launch(dx.ptr, L, C, dspec.ptr, K, M, N, pp, mode)
                else:
                    launch("power", dx.ptr, dspec.ptr, (pp,))
            if "peak" in which:
                bb, pb = self.guarded(C * L, front)
                bi, pi = self.guarded(C * L, front)
                bufs += [bb, bi]
                if launch is None:
                    fd.peak_launch(dx.ptr, L, C, dspec.ptr, K, M, N, pb, pi, mode)
                else:
                    launch("peak", dx.ptr, dspec.ptr, (pb, pi))
            assert sm.lib.smfft_synchronize() == 0
            if "power" in which:
                out["power"] = self.collect(bp, C * K * L, np.float32, front).reshape(C, K, L)
            if "peak" in which:
                out["peak"] = self.collect(bb, C * L, np.float32, front).reshape(C, L)
                out["index"] = self.collect(bi, C * L, np.int32, front).reshape(C, L)
        finally:
            for b in bufs:
                b.free()
        if "peak" in which:
            assert np.all((out["index"] >= 0) & (out["index"] < K)), "an index outside [0, K), or left unwritten"
        if finite:
            for name in ("power", "peak"):
                if name in out:
                    assert np.all(np.isfinite(out[name])), f"{name}: outputs left unwritten"
        return out

    # ---- the checks --------------------------------------------------------------------------------------------------------------
    @staticmethod
    def check_power(got, y64, x, h, what):
        """test 1's bound, per element; prints the worst ratio to the bound before it asserts"""
        err, bound = np.abs(got.astype(np.float64) - power64(y64)), power_bound(y64, x, h)
        ratio = float(np.max(err / bound))
        print(f"{what}: max |p - p64| / bound = {ratio:.3f}")
        assert np.all(err <= bound), f"{what}: |p - p64| reaches {ratio:.3f} of its bound"

    @staticmethod
    def check_peak_is_own_power(out, what):
        """peak's bits are those of the maximum of the library's own power rows and the index is np.argmax's, everywhere"""
        p = out["power"]
        assert np.array_equal(bits(out["peak"]), bits(np.max(p, axis=1))), f"{what}: peak differs from the maximum of the power rows"
        assert np.array_equal(out["index"], np.argmax(p, axis=1)), f"{what}: index differs from np.argmax of the power rows"

    @staticmethod
    def check_peak(peak, index, y64, x, h, what):
        """test 3: the peak within the largest of the K row bounds of the fp64 maximum, and the fp64 power of the chosen filter within
        twice that bound of it"""
        p64 = power64(y64)
        bound = np.max(power_bound(y64, x, h), axis=1)                 # (C, L)
        top = np.max(p64, axis=1)
        err = np.abs(peak.astype(np.float64) - top)
        chosen = np.take_along_axis(p64, index[:, None, :].astype(np.int64), axis=1)[:, 0, :]
        print(f"{what}: max |peak - max p64| / bound = {float(np.max(err / bound)):.3f}, max (max p64 - p64[index]) / (2 bound) = "
              f"{float(np.max((top - chosen) / (2 * bound))):.3f}")
        assert np.all(err <= bound), what
        assert np.all(top - chosen <= 2 * bound), what
