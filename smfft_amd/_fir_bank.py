"""What the ctypes mirrors of the overlap-save FIR filter banks share (smfft_amd.api: complex data at N = 256 ... 4096, in the main
library; smfft_amd.fir_real: real signals and real taps at the same lengths; smfft_amd.large_fir: complex data at N = 8192 / 16384):
the three entry points' signatures, the mode check, the calls with their error messages, the rule for the transform length and the
host-array round trip.  The libraries' C ABIs are one for one the same; a bank differs by its prefix, its lengths and its dtype.  The
public functions, with the documentation of what each bank computes, are the mirrors'."""
import ctypes

import numpy as np

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)


def sigs(prefix):
    """name -> (restype, argtypes) of the three functions of a bank's header"""
    return {
        prefix + "_prepare": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
        prefix + "_launch": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
        prefix + "_benchmark": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _i, _vp, _dp]),
    }


def mode_flag(mode):
    if mode not in ("convolve", "correlate"):
        raise ValueError(f"mode must be 'convolve' or 'correlate', not {mode!r}")
    return int(mode == "correlate")


class Bank:
    def __init__(self, name, prefix, lib, sizes, real, kind="", refuses=True):
        """name: the mirror's, for messages ("fir_real"; "": the main library's); prefix: of its C functions ("smfft_fir_real"); lib: the
        mirror's lib(); sizes: the lengths the library serves; real: float32 signals, taps and outputs (else complex64); kind: the word
        in front of "filter banks" in messages; refuses: fir() refuses a length or a tap count the bank does not serve with a ValueError
        of its own (else the library's -1 becomes its RuntimeError)"""
        self.name, self.prefix, self.lib, self.sizes, self.real, self.kind, self.refuses = name, prefix, lib, sizes, real, kind, refuses
        self.dtype = np.float32 if real else np.complex64
        self.serves = f"N = {sizes[0]} and {sizes[1]}" if len(sizes) == 2 else f"N = {sizes[0]} ... {sizes[-1]}"

    def call(self, function, *args):
        return getattr(self.lib(), f"{self.prefix}_{function}")(*args)

    def prepare(self, d_taps, d_spectra, n_taps, n_filters, N, mode, stream):
        rc = self.call("prepare", d_taps, n_taps, n_filters, N, mode_flag(mode), d_spectra, stream)
        if rc != 0:
            raise RuntimeError(f"{self.prefix}_prepare(M={n_taps}, K={n_filters}, N={N}) -> {rc}")

    def launch(self, d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode, stream):
        rc = self.call("launch", d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, mode_flag(mode), d_output, stream)
        if rc != 0:
            raise RuntimeError(f"{self.prefix}_launch(L={L}, C={n_channels}, K={n_filters}, M={n_taps}, N={N}) -> {rc}")

    def benchmark(self, d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, d_output, mode):
        t = ctypes.c_double(0.0)
        rc = self.call("benchmark", d_signal, L, n_channels, d_spectra, n_filters, n_taps, N, mode_flag(mode), d_output, ctypes.byref(t))
        return rc, t.value

    def fir_fft_size(self, n_taps):
        """the next power of two >= 4 M, clamped to the bank's lengths"""
        lo, hi = self.sizes[0], self.sizes[-1]
        if not 1 <= n_taps < hi:
            raise ValueError(f"n_taps = {n_taps}: the {self.kind}filter banks take 1 ... {hi - 1} taps")
        return min(hi, max(lo, 1 << (4 * n_taps - 1).bit_length()))

    def fir(self, x, taps, mode, fft_size):
        """host arrays through prepare and one launch: validates x ((C, L) or (L,)) and taps ((K, M) or (M,)), casts them to the bank's
        dtype and copies them in, fills the (C, K, L) output, prefilled with 0xFF, waits and copies it back"""
        corr = mode_flag(mode)
        x, taps = np.asarray(x), np.asarray(taps)
        if self.real and (np.iscomplexobj(x) or np.iscomplexobj(taps)):
            raise TypeError("smfft_amd.fir_real.fir takes real signals and real taps; smfft_amd.fir serves complex ones")
        if x.ndim not in (1, 2) or taps.ndim not in (1, 2):
            raise ValueError("x must be (C, L) or (L,), taps (K, M) or (M,)")
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=self.dtype)
        taps = np.ascontiguousarray(np.atleast_2d(taps), dtype=self.dtype)
        (C, L), (K, M) = x.shape, taps.shape
        N = self.fir_fft_size(M) if fft_size is None else int(fft_size)      # (refuses M past the longest length before anything touches a device)
        if self.refuses and (N not in self.sizes or not 1 <= M < N):
            raise ValueError(f"smfft_amd.{self.name} serves {self.serves} with 1 <= M < N, not N = {N}, M = {M}")
        from . import api      # the device allocator and copies of libsmfft_amd.so
        din, dtaps = api.DeviceBuffer.from_host(x), api.DeviceBuffer.from_host(taps)
        dspec = api.DeviceBuffer(max(K * N * 8, 8))
        dout = api.DeviceBuffer(max(C * K * L * np.dtype(self.dtype).itemsize, 8))
        api.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes)   # NaN pattern: untouched outputs are caught
        rc = self.call("prepare", dtaps.ptr, M, K, N, corr, dspec.ptr, None)
        if rc == 0:
            rc = self.call("launch", din.ptr, L, C, dspec.ptr, K, M, N, corr, dout.ptr, None)
        if rc == 0:
            rc = api.lib.smfft_synchronize()
        if rc != 0:
            raise RuntimeError(f"{self.name + '.' if self.name else ''}fir(C={C}, L={L}, K={K}, M={M}, N={N}, {mode}) -> {rc}")
        out = dout.to_host(self.dtype, (C, K, L))
        for b in (din, dtaps, dspec, dout):
            b.free()
        return out
