"""What the ctypes mirrors of the polyphase filter banks share (smfft_amd.pfb: complex streams, smfft_amd.pfb_real: real streams;
smfft_amd.large_pfb, the complex bank at N = 8192 / 16384, takes the Bank below with its own lengths and its own tuned launch;
smfft_amd.pfb_spec, the integrated spectra of both, takes one Bank per kind of stream for its checks, prototype and round trip):
the five entry points' signatures, the calls with their error messages, the prototype and the host-array round trip.  The libraries'
C ABIs are one for one the same; a bank differs by its prefix, by the samples a frame takes per channel (1: N complex samples, 2: 2N
real samples) and by the signal's dtype.  The public functions, with the documentation of what each bank computes, are the mirrors'."""
import ctypes

import numpy as np

SIZES = (256, 512, 1024, 2048, 4096)
MAX_TAPS_PER_CHANNEL = 32

_vp, _i, _ll, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)


def sigs(prefix):
    """name -> (restype, argtypes) of the five functions of include/<prefix>.h"""
    return {
        prefix + "_frames": (_ll, [_ll, _i, _i]),
        prefix + "_launch": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _vp, _vp]),
        prefix + "_benchmark": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _vp, _dp]),
        prefix + "_launch_tuned": (_i, [_vp, _ll, _i, _vp, _i, _i, _i, _vp, _vp, _i]),
        prefix + "_default_tile_run": (_i, [_i, _i]),
    }


class Bank:
    def __init__(self, name, prefix, lib, real, sizes=SIZES):
        """name: the mirror's, for messages ("pfb"); prefix: of its C functions ("smfft_pfb"); lib: the mirror's lib(); real: real streams;
        sizes: the lengths the library serves"""
        self.name, self.prefix, self.lib, self.real, self.sizes = name, prefix, lib, real, sizes
        self.per_channel = 2 if real else 1           # samples of a frame per channel: a frame is `per_channel * N` samples
        self.chunk = "2N" if real else "N"

    def call(self, function, *args):
        return getattr(self.lib(), f"{self.prefix}_{function}")(*args)

    def frames(self, L, N, P):
        f = self.call("frames", L, N, P)
        if f < 0:
            raise ValueError(f"{self.prefix}_frames(L={L}, N={N}, P={P}) -> {f}: N must be one of {self.sizes}, "
                             f"1 <= P <= {MAX_TAPS_PER_CHANNEL}, L >= 0" + (" and even" if self.real else ""))
        return f

    def default_tile_run(self, N, P):
        r = self.call("default_tile_run", N, P)
        if r < 0:
            raise ValueError(f"{self.prefix}_default_tile_run(N={N}, P={P}) -> {r}")
        return r

    def launch(self, d_signal, L, C, d_taps, N, P, d_output, power, stream):
        rc = self.call("launch", d_signal, L, C, d_taps, N, P, int(bool(power)), d_output, stream)
        if rc != 0:
            raise RuntimeError(f"{self.prefix}_launch(L={L}, C={C}, N={N}, P={P}) -> {rc}")

    def launch_tuned(self, d_signal, L, C, d_taps, N, P, d_output, tile_run, power, stream):
        rc = self.call("launch_tuned", d_signal, L, C, d_taps, N, P, int(bool(power)), d_output, stream, tile_run)
        if rc != 0:
            raise RuntimeError(f"{self.prefix}_launch_tuned(L={L}, C={C}, N={N}, P={P}, R={tile_run}) -> {rc}")

    def benchmark(self, d_signal, L, C, d_taps, N, P, d_output, power):
        t = ctypes.c_double(0.0)
        rc = self.call("benchmark", d_signal, L, C, d_taps, N, P, int(bool(power)), d_output, ctypes.byref(t))
        return rc, t.value

    def prototype(self, n_channels, taps_per_channel, window):
        N, P = int(n_channels), int(taps_per_channel)
        if N < 1 or P < 1:
            raise ValueError(f"prototype(N={N}, P={P})")
        M = self.per_channel * P * N
        if window == "rectangular":
            w = np.ones(M)
        elif window in ("hamming", "hanning", "blackman", "bartlett"):
            w = getattr(np, window)(M)
        else:
            raise ValueError(f"unknown window {window!r}")
        m = np.arange(M, dtype=np.float64)
        return (np.sinc((m - (M - 1) / 2) / (self.per_channel * N)) * w).astype(np.float32)

    def round_trip(self, x, taps, n_channels, rows, dtype, launch, shape_error, real_error, function, extra=""):
        """host arrays through one launch: validates x ((C, L) or (L,)) and taps (P N real coefficients, P 2N for real streams), makes them
        contiguous and copies them in, lets launch(d_signal, L, C, d_taps, N, P, d_output) -> status fill the (C, rows(L, N, P), N) output
        of `dtype`, prefilled with 0xFF, waits and copies it back.  shape_error, real_error: the caller's ValueError texts; function,
        extra: its name and its own arguments, for the RuntimeError."""
        x, taps = np.asarray(x), np.asarray(taps)
        if x.ndim not in (1, 2) or taps.ndim != 1:
            raise ValueError(shape_error)
        if np.iscomplexobj(taps) or (self.real and np.iscomplexobj(x)):
            raise ValueError(real_error)
        N = int(n_channels)
        frame = self.per_channel * N
        if N not in self.sizes or taps.size % frame or not 1 <= taps.size // frame <= MAX_TAPS_PER_CHANNEL:
            raise ValueError(f"smfft_amd.{self.name} serves N in {self.sizes} with P {self.chunk} taps, 1 <= P <= {MAX_TAPS_PER_CHANNEL}, "
                             f"not N = {N} with {taps.size} taps")
        P = taps.size // frame
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float32 if self.real else np.complex64)
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        C, L = x.shape
        F = rows(L, N, P)
        if C * F == 0:
            return np.empty((C, F, N), dtype)
        from . import api      # the device allocator and copies of libsmfft_amd.so
        din, dtaps = api.DeviceBuffer.from_host(x), api.DeviceBuffer.from_host(taps)
        dout = api.DeviceBuffer(C * F * N * np.dtype(dtype).itemsize)
        api.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes)   # NaN pattern: untouched outputs are caught
        rc = launch(din.ptr, L, C, dtaps.ptr, N, P, dout.ptr)
        if rc == 0:
            rc = api.lib.smfft_synchronize()
        if rc != 0:
            raise RuntimeError(f"{self.name}.{function}(C={C}, L={L}, N={N}, P={P}{extra}) -> {rc}")
        out = dout.to_host(dtype, (C, F, N))
        for b in (din, dtaps, dout):
            b.free()
        return out

    def channelize(self, x, taps, n_channels, power):
        """host arrays -> the (C, F, N) rows as the device writes them"""
        return self.round_trip(
            x, taps, n_channels, self.frames, np.float32 if power else np.complex64,
            lambda d_signal, L, C, d_taps, N, P, d_output: self.call("launch", d_signal, L, C, d_taps, N, P, int(bool(power)), d_output, None),
            f"x must be (C, L) or (L,), taps a vector of P {self.chunk} coefficients",
            "the signal and the prototype must be real (complex signals: smfft_amd.pfb)" if self.real else "the prototype must be real", "channelize")
