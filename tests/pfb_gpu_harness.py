"""What the GPU tests of the polyphase filter bank family share (tests/test_pfb_gpu.py, test_pfb_real_gpu.py, test_large_pfb_gpu.py,
test_pfb_spec_gpu.py, test_pfb_probes_gpu.py, the probes of tests/pfb_spec_probes.py and the host run of test_large_pfb_hostsim.py): the
bounds, a description of a bank, the guarded run, the row checks, the periodic device signal of the 2^31 tests, bits and leakage.  A
plain module: no tests, no fixtures; it needs no device itself (tests/test_pfb_gpu_harness_cpu.py runs it on numpy memory).

Every run goes through guarded_run: the output is prefilled with 0xFF (NaN) and followed by a 4096-element guard of 0x5A that must stay
untouched; the signal buffer carries 0xFF -- NaN -- in 4096 samples before stream 0, after stream C - 1, and in every stream's unread
tail (for a channelizer [(F + P - 1) N, L); the tail belongs to its own stream, so this never touches another stream's frames), so that
a read outside the contract shows up as a non-finite output.

Tolerances, per output spectrum (one (c, f) row of N values).  With s[n] = sum_p |h[p N + n]| |x[(f + p) N + n]|, the scale the fp32
accumulation rounds at (by Parseval ||y_f|| <= sqrt(N) ||s||, with equality when the taps do not cancel):
  complex mode: ||got - ref||_2 / (sqrt(N) ||s||_2) <= 1e-6  and  max|got - ref| / max(max|ref|, ||s||_2) <= 5e-6 -- the FIR rows'
                bounds (tests/fir_gpu_harness.py), sized for two transforms and a product: room for one transform plus a 32-term sum;
  power mode, Gaussian signals (no cancellation): ||got - ref||_1 / ||ref||_1 <= 2e-6 and max|got - ref| / max(ref) <= 1e-5 -- twice the
                amplitude bounds, since | |y + d|^2 - |y|^2 | <= 2 |y| |d| + |d|^2 and sum |y| |d| <= ||y||_2 ||d||_2.
  power mode, tones (Bank.check_tone_power; the P branches of an off-centre tone do cancel, so sqrt(N) ||s|| exceeds ||y||): the same
                derivation before its last step, ||got - ref||_1 <= 2e-6 ||y||_2 sqrt(N) ||s||_2 and
                max|got - ref| <= 1e-5 max|y| max(max|y|, ||s||_2); without cancellation these are the two bounds above.
The real bank (tests/test_pfb_real_gpu.py derives it) takes the frame's 2N real samples in the place of the N complex ones, checks the
N + 1 values X[0 ... N] of a packed row, and element 0 of every row on its own as well.  The integrated spectra add gamma(T), the
sequential fp32 sum's own error, to the power bounds (tests/test_pfb_spec_gpu.py derives it).

A new bank gets the full set of GPU checks from an entry in Bank.MODELS (its mirror's name -> its fp64 model, which has frames, scale and
the transform of a stream) and a test module that calls tests/pfb_gpu_checks.py with its shapes."""
import contextlib
import ctypes
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import pfb_real_model as prm  # noqa: E402

SIZES = [256, 512, 1024, 2048, 4096]
TAPS = [1, 2, 4, 8, 16, 32]
ROW_REL_L2, ROW_MAX = 1e-6, 5e-6
POWER_L1, POWER_MAX = 2e-6, 1e-5
GUARD = 4096                   # samples around the signal that are NaN, elements around the output that must stay untouched

# (power outside channel 100) / (power in it) of a unit tone at channel 100.37 through the Hamming-windowed sinc of P N taps, from
# tools/large_pfb_model.py in fp64; the same to three digits at N = 8192 and 16384 (tests/test_large_pfb_cpu.py holds the model to it, the
# GPU test the device).  P = 1 is a Hamming-windowed single frame: it leaks more than the rectangular window's 0.60, because its main
# lobe is twice as wide.
LEAKAGE = {1: 0.757, 2: 0.325, 3: 0.180, 4: 0.0979, 5: 0.0514, 6: 0.0263, 7: 0.0123, 8: 5.61e-3, 9: 2.13e-3, 10: 7.76e-4, 11: 2.02e-4,
           12: 3.54e-5, 13: 3.45e-6, 14: 2.43e-6, 15: 4.50e-6, 16: 5.35e-6, 17: 2.49e-6, 18: 1.59e-6, 19: 5.78e-7, 20: 3.79e-7,
           21: 1.55e-6, 22: 4.12e-7, 23: 2.63e-6, 24: 4.21e-7, 25: 1.21e-6, 26: 5.25e-8, 27: 1.86e-8, 28: 2.39e-7, 29: 1.72e-6,
           30: 1.03e-6, 31: 2.86e-6, 32: 8.94e-7}


def gamma(T):
    u = 2.0 ** -24
    return (T - 1) * u / (1 - (T - 1) * u)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def leakage(power, channel):
    power = np.asarray(power, np.float64)
    return (power.sum(axis=-1) - power[..., channel]) / power[..., channel]


def chunk(N, real):
    """samples of a frame's hop, and the transform's length"""
    return 2 * N if real else N


def rand(rng, shape, real):
    if real:
        return rng.standard_normal(shape).astype(np.float32)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def length(N, P, frames, tail, real):
    """samples of a stream with `frames` whole frames and `tail` more samples (even for a real stream)"""
    assert tail < chunk(N, real) and not (real and tail % 2)
    return (frames + P - 1) * chunk(N, real) + tail


class Worst(dict):
    """the largest figures the row checks have seen; whoever runs the checks owns one and prints it when done"""

    def note(self, **figures):
        for key, value in figures.items():
            self[key] = max(self.get(key, 0.0), value)

    def rows_line(self):
        return (f"\nworst seen: complex relL2 {self.get('l2', 0.0):.3e} (bound {ROW_REL_L2}), max {self.get('max', 0.0):.3e} (bound {ROW_MAX}); "
                f"power L1 {self.get('pl1', 0.0):.3e} (bound {POWER_L1}), max {self.get('pmax', 0.0):.3e} (bound {POWER_MAX})")


# ------------------------------------------------------------------------------------------------ the guarded run
def guarded_run(sm, x, h, used, shape, dtype, launcher, in_off=0, tap_off=0, out_off=0, finite=True):
    """launcher(d_signal, d_taps, d_output) from a signal fenced with NaN into an output fenced with a guard; returns the result, of
    `shape` and `dtype`, after checking that the guards are untouched and nothing of the prefill is left.  x: (C, L), of which a launch
    may read the first `used` samples of each stream; h: float32 taps.  in_off (samples), tap_off (floats) and out_off (output elements)
    shift the three pointers by that many elements into their buffers.  finite=False is for runs whose inputs hold NaN or Inf on
    purpose: the guards are checked all the same, the output may be non-finite."""
    nan = np.nan + 1j * np.nan if np.iscomplexobj(x) else np.nan
    body = x.copy()
    body[:, used:] = nan
    fence = np.full(GUARD, nan, x.dtype)
    dx = sm.DeviceBuffer.from_host(np.concatenate([np.full(in_off, nan, x.dtype), fence, body.reshape(-1), fence]))
    dh = sm.DeviceBuffer.from_host(np.concatenate([np.full(tap_off, np.nan, np.float32), h]))
    width, total = np.dtype(dtype).itemsize, int(np.prod(shape))
    dout = sm.DeviceBuffer((out_off + total + GUARD) * width)
    for at, byte, n in ((0, 0x5A, out_off), (out_off, 0xFF, total), (out_off + total, 0x5A, GUARD)):
        if n:
            assert sm.lib.smfft_memset(dout.ptr + at * width, byte, n * width) == 0
    launcher(dx.ptr + (in_off + GUARD) * x.itemsize, dh.ptr + tap_off * 4, dout.ptr + out_off * width)
    assert sm.lib.smfft_synchronize() == 0
    raw = dout.to_host(np.uint8, ((out_off + total + GUARD) * width,))
    assert np.all(raw[:out_off * width] == 0x5A), "the kernel wrote before its output"
    assert np.all(raw[(out_off + total) * width:] == 0x5A), "the kernel wrote past its output"
    out = raw[out_off * width:(out_off + total) * width].view(dtype).reshape(shape)
    assert not finite or np.all(np.isfinite(out.view(np.float32))), "outputs left unwritten, or a sample read outside the contract"
    for b in (dx, dh, dout):
        b.free()
    return out


# ------------------------------------------------------------------------------------------------ the row checks
def unpack(packed):
    """(..., N) packed rows of the real bank, element 0 = (X[0], X[N]) -> (..., N + 1) complex128"""
    out = np.empty(packed.shape[:-1] + (packed.shape[-1] + 1,), np.complex128)
    out[..., :-1] = packed
    out[..., 0] = packed[..., 0].real
    out[..., -1] = packed[..., 0].imag
    return out


def check_complex(got, ref, s, what, worst):
    """got, ref: (C, F, N) spectra, s: (C, F, N) the accumulation's scale"""
    N = ref.shape[-1]
    d = got.astype(np.complex128) - ref
    sn = np.linalg.norm(s, axis=-1)
    l2 = np.linalg.norm(d, axis=-1) / np.maximum(np.sqrt(N) * sn, 1e-300)
    mx = np.abs(d).max(axis=-1) / np.maximum(np.maximum(np.abs(ref).max(axis=-1), sn), 1e-300)
    print(f"{what}: relL2 {l2.max():.3e} max {mx.max():.3e}")
    worst.note(l2=l2.max(), max=mx.max())
    assert l2.max() <= ROW_REL_L2 and mx.max() <= ROW_MAX, f"{what}: relL2={l2.max():.3e} max={mx.max():.3e}"


def check_power(got, ref, what, worst):
    """got: (C, F, N) powers, ref: (C, F, N) spectra"""
    ref = ref.real ** 2 + ref.imag ** 2
    d = np.abs(got.astype(np.float64) - ref)
    l1 = d.sum(axis=-1) / ref.sum(axis=-1)
    mx = d.max(axis=-1) / ref.max(axis=-1)
    print(f"{what}: L1 {l1.max():.3e} max {mx.max():.3e}")
    worst.note(pl1=l1.max(), pmax=mx.max())
    assert l1.max() <= POWER_L1 and mx.max() <= POWER_MAX, f"{what}: L1={l1.max():.3e} max={mx.max():.3e}"


def check_real_complex(got, ref, s, what, worst):
    """got: (C, F, N) packed rows of the device, ref: (C, F, N + 1) rfft rows, s: (C, F, 2N) the accumulation's scale"""
    N = got.shape[-1]
    assert ref.shape == got.shape[:-1] + (N + 1,) and s.shape == got.shape[:-1] + (2 * N,)
    d = unpack(got) - ref
    sn = np.linalg.norm(s, axis=-1)
    l2 = np.linalg.norm(d, axis=-1) / np.maximum(np.sqrt(2 * N) * sn, 1e-300)
    denom = np.maximum(np.maximum(np.abs(ref).max(axis=-1), sn), 1e-300)
    mx = np.abs(d).max(axis=-1) / denom
    # element 0 on its own: (X[0], X[N]), both real
    e0 = np.maximum(np.abs(got[..., 0].real.astype(np.float64) - ref[..., 0].real), np.abs(got[..., 0].imag.astype(np.float64) - ref[..., N].real)) / denom
    print(f"{what}: relL2 {l2.max():.3e} max {mx.max():.3e} element 0 {e0.max():.3e}")
    worst.note(l2=l2.max(), max=mx.max())
    assert l2.max() <= ROW_REL_L2 and mx.max() <= ROW_MAX and e0.max() <= ROW_MAX, f"{what}: relL2={l2.max():.3e} max={mx.max():.3e} element 0={e0.max():.3e}"


def check_real_power(got, ref, what, worst):
    """got: (C, F, N) powers of the device, ref: (C, F, N + 1) rfft rows"""
    refp = prm.power(ref)
    d = np.abs(got.astype(np.float64) - refp)
    l1 = d.sum(axis=-1) / refp.sum(axis=-1)
    mx = d.max(axis=-1) / refp.max(axis=-1)
    e0 = np.abs(got[..., 0].astype(np.float64) - ref[..., 0].real ** 2) / refp.max(axis=-1)       # DC alone: X[0]^2, no Nyquist in it
    print(f"{what}: L1 {l1.max():.3e} max {mx.max():.3e} element 0 {e0.max():.3e}")
    worst.note(pl1=l1.max(), pmax=mx.max())
    assert l1.max() <= POWER_L1 and mx.max() <= POWER_MAX and e0.max() <= POWER_MAX, f"{what}: L1={l1.max():.3e} max={mx.max():.3e} element 0={e0.max():.3e}"


def check_spectra(got, ref, m, T, what, worst):
    """integrated spectra: got, ref: (C, I, N); m: (C, I), the sum over the T frames of each frame's largest power"""
    assert got.shape == ref.shape and got.dtype == np.float32
    d = np.abs(got.astype(np.float64) - ref)
    l1 = d.sum(axis=-1) / ref.sum(axis=-1) / (POWER_L1 + gamma(T))
    mx = d.max(axis=-1) / m / (POWER_MAX + gamma(T))
    print(f"{what}: L1 {l1.max() * (POWER_L1 + gamma(T)):.3e} (bound {POWER_L1 + gamma(T):.3e}) max {mx.max() * (POWER_MAX + gamma(T)):.3e} "
          f"(bound {POWER_MAX + gamma(T):.3e})")
    worst.note(l1=l1.max(), max=mx.max())
    assert l1.max() <= 1.0 and mx.max() <= 1.0, f"{what}: L1 {l1.max():.3f} max {mx.max():.3f} of their bounds"


# ------------------------------------------------------------------------------------------------ a bank
class Bank:
    """one channelizer library behind the calls its GPU tests need: its ctypes mirror (smfft_amd.<name>), its fp64 model, its signals
    and its row checks, with the worst figures they have seen"""
    MODELS = {"pfb": "pfb_model", "pfb_real": "pfb_real_model", "large_pfb": "large_pfb_model"}
    LABELS = {"pfb": "PFB", "pfb_real": "real PFB", "large_pfb": "large PFB"}

    def __init__(self, name):
        self.name, self.real, self.label = name, name == "pfb_real", self.LABELS[name]
        self.model = importlib.import_module(self.MODELS[name])
        self.transform = self.model.pfb_real if self.real else self.model.pfb       # (C, L) stream, taps, N -> fp64 rows
        self.dtype = np.float32 if self.real else np.complex64
        self.worst = Worst()

    @property
    def lib(self):
        mirror = importlib.import_module("smfft_amd." + self.name)
        mirror.lib()
        return mirror

    def chunk(self, N):
        return chunk(N, self.real)

    def rand(self, rng, shape):
        return rand(rng, shape, self.real)

    def length(self, N, P, F, tail):
        return length(N, P, F, tail, self.real)

    def taps(self, rng, N, P):
        return rng.standard_normal(P * self.chunk(N)).astype(np.float32)

    def prototypes(self, rng, N, P):
        return {"windowed sinc": self.lib.prototype(N, P), "gaussian": self.taps(rng, N, P), "ones": np.ones(P * self.chunk(N), np.float32)}

    def reference(self, x, h, N):
        """(rows, scale) of a case: the fp64 model's (C, F, N) spectra -- (C, F, N + 1) for the real bank -- and s"""
        return self.transform(x, h, N), self.model.scale(x, h, N)

    def run(self, sm, x, h, N, power, launcher=None, **kw):
        """guarded_run through the device-pointer API: launcher(d_signal, L, C, d_taps, N, P, d_output, power), or the mirror's launch;
        returns the (C, F, N) result as the device wrote it"""
        C, L = x.shape
        P = h.size // self.chunk(N)
        F = self.model.frames(L, N, P)
        if launcher is None:
            lib = self.lib

            def launcher(*a):
                lib.launch(*a[:-1], power=a[-1])
        return guarded_run(sm, x, h, (F + P - 1) * self.chunk(N), (C, F, N), np.float32 if power else np.complex64,
                           lambda dx, dh, dy: launcher(dx, L, C, dh, N, P, dy, power), **kw)

    def tuned(self, R):
        """a launcher for run: the mirror's launch_tuned at run length R"""
        lib = self.lib
        return lambda *a: lib.launch_tuned(*a[:-1], R, power=a[-1])

    def check(self, got, ref, s, power, what):
        """the bank's row check of one mode against reference(x, h, N)"""
        if power:
            (check_real_power if self.real else check_power)(got, ref, what, self.worst)
        else:
            (check_real_complex if self.real else check_complex)(got, ref, s, what, self.worst)

    def check_rows(self, got, x, h, N, power, what):
        self.check(got, *self.reference(x, h, N), power, what)

    def check_both_modes(self, sm, x, h, N, what, launcher=None, power_what=" power"):
        ref, s = self.reference(x, h, N)
        self.check(self.run(sm, x, h, N, False, launcher=launcher), ref, s, False, what)
        self.check(self.run(sm, x, h, N, True, launcher=launcher), ref, s, True, what + power_what)

    def check_tone_power(self, gotp, ref, s, N, P):
        """the power rows of a signal whose branches cancel, against the bounds before their last step (the module's docstring)"""
        refp = prm.power(ref) if self.real else ref.real ** 2 + ref.imag ** 2
        d = np.abs(gotp.astype(np.float64) - refp)
        yn, ym, sn = np.linalg.norm(ref, axis=-1), np.abs(ref).max(axis=-1), np.linalg.norm(s, axis=-1)
        l1 = d.sum(axis=-1) / (yn * np.sqrt(self.chunk(N)) * sn)
        mx = d.max(axis=-1) / (ym * np.maximum(ym, sn))
        print(f"tones N={N} P={P} power: L1 {l1.max():.3e} max {mx.max():.3e}")
        assert l1.max() <= POWER_L1 and mx.max() <= POWER_MAX, (N, P, l1.max(), mx.max())


class Spectra:
    """the integrated power spectra (smfft_amd.pfb_spec) behind the calls their GPU test and its probes need"""

    def __init__(self, mirror):
        self.ps, self.model, self.worst = mirror, importlib.import_module("pfb_spec_model"), Worst()

    def run(self, sm, x, h, N, T, real, launcher=None, **kw):
        """guarded_run through the device-pointer API: launcher(d_signal, L, C, d_taps, N, P, T, d_output), or the mirror's launch; returns
        the (C, I, N) result.  A stream's unread tail starts at (I T + P - 1) frames: the trailing frames f >= I T are not computed."""
        C, L = x.shape
        P = h.size // chunk(N, real)
        n = self.model.spectra(L, N, P, T, real)
        if launcher is None:
            def launcher(*a):
                self.ps.launch(*a, real=real)
        return guarded_run(sm, x, h, (n * T + P - 1) * chunk(N, real) if n else 0, (C, n, N), np.float32,
                           lambda dx, dh, dy: launcher(dx, L, C, dh, N, P, T, dy), **kw)

    def check(self, got, x, h, N, T, real, what):
        ref, m = self.model.integrate(x, h, N, T, real)
        check_spectra(got, ref, m, T, what, self.worst)


# ------------------------------------------------------------------------------------------------ a caller's stream
@contextlib.contextmanager
def caller_stream():
    """a stream from hipStreamCreate -> (its handle, a function that waits for it)"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value

    def wait():
        assert hip.hipStreamSynchronize(stream) == 0
    yield stream.value, wait
    assert hip.hipStreamDestroy(stream) == 0


def benchmark_twice(fn, mirror_benchmark, seen):
    """a launcher body for the benchmark form: the C function adds to its total on both calls, the mirror returns a time of its own"""
    t = ctypes.c_double(5.0)
    assert fn(ctypes.byref(t)) == 0
    first = t.value
    assert first > 5.0
    assert fn(ctypes.byref(t)) == 0
    assert t.value > first
    rc, ms = mirror_benchmark()
    assert rc == 0 and ms > 0.0
    seen.append(ms)


# ------------------------------------------------------------------------------------------------ offsets beyond 2^31
class PeriodicLaunch:
    """One launch on more than 2^31 elements, complex streams.  The signal is made on the device: stream c is an uploaded Gaussian block of
    2^24 + 1 elements repeated from a stream-dependent phase, x_c[i] = B[(i + 4099 c + 17) mod (2^24 + 1)] -- the block length is odd and
    every sampled window starts at another phase of it, so no two sampled windows are equal.  C streams of L samples, the first `used`
    of each filled and the rest NaN, between GUARD samples of NaN; `rows` output rows of N elements of `dtype`, prefilled with 0xFF and
    followed by a guard that launch(d_signal, d_taps, d_output) must leave untouched."""
    B = (1 << 24) + 1

    def __init__(self, sm, seed, h, C, L, used, rows, N, dtype, launch):
        self.sm, self.L, self.N, self.dtype, self.seen = sm, L, N, np.dtype(dtype), set()
        self.block = rand(np.random.default_rng(seed), (self.B,), False)
        width, total = self.dtype.itemsize, rows * N
        dblock, dh = sm.DeviceBuffer.from_host(self.block), sm.DeviceBuffer.from_host(h)
        self.dx = sm.DeviceBuffer((C * L + 2 * GUARD) * 8)
        self.dout = sm.DeviceBuffer((total + GUARD) * width)
        self.buffers = (dblock, dh, self.dx, self.dout)
        assert sm.lib.smfft_memset(self.dx.ptr, 0xFF, self.dx.nbytes) == 0
        for c in range(C):
            i, phase = 0, (4099 * c + 17) % self.B
            while i < used:
                n = min(self.B - phase, used - i)
                assert sm.lib.smfft_memcpy_d2d(self.dx.ptr + (GUARD + c * L + i) * 8, dblock.ptr + phase * 8, n * 8) == 0
                i, phase = i + n, 0
        assert sm.lib.smfft_memset(self.dout.ptr, 0xFF, total * width) == 0
        assert sm.lib.smfft_memset(self.dout.ptr + total * width, 0x5A, GUARD * width) == 0
        launch(self.dx.ptr + GUARD * 8, dh.ptr, self.dout.ptr)
        assert sm.lib.smfft_synchronize() == 0
        guard = np.empty(GUARD * width, np.uint8)
        assert sm.lib.smfft_memcpy_d2h(guard.ctypes.data, self.dout.ptr + total * width, guard.nbytes) == 0
        assert np.all(guard == 0x5A), "the kernel wrote past its output"

    def window(self, c, start, n):
        """(1, n): samples start ... start + n of stream c, copied back; they are the block from a phase no other window had"""
        xs = np.empty((1, n), np.complex64)
        assert self.sm.lib.smfft_memcpy_d2h(xs.ctypes.data, self.dx.ptr + (GUARD + c * self.L + start) * 8, xs.nbytes) == 0
        phase = (start + 4099 * c + 17) % self.B
        assert np.array_equal(xs[0], np.take(self.block, np.arange(phase, phase + n), mode="wrap")) and phase not in self.seen
        self.seen.add(phase)
        return xs

    def row(self, g):
        """(1, 1, N): output row g, finite"""
        got = np.empty((1, 1, self.N), self.dtype)
        assert self.sm.lib.smfft_memcpy_d2h(got.ctypes.data, self.dout.ptr + g * self.N * self.dtype.itemsize, got.nbytes) == 0
        assert np.all(np.isfinite(got.view(np.float32)))
        return got

    def free(self):
        for b in self.buffers:
            b.free()
