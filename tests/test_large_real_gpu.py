"""The real N = 16384 / 32768 single-pass R2C / C2R kernels of libsmfft_large_real.so (include/smfft_large_real.h) on an MI355X,
against numpy in float64 / complex128 (oracle/np_reference.r2c_packed / c2r_packed): parity over ragged batches (one FFT to 2.5
persistent grids), the round trip, per-element DFT-matrix probes in both directions, constant and alternating inputs, zero-mean
accuracy, isolation and exact scaling, one row's bits in every position of a batch, guarded buffers, interior pointers, in-place
calls, batches around the persistent grid G in tests/test_buffers_gpu.py's regime, a caller's stream, two host threads launching
beside each other, the timed form, and 64-bit element offsets (16 GiB, both directions)."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (16384, 32768)
DIRS = (False, True)
F = 4           # bytes per real fp32 sample; an FFT is N * F bytes on both sides


@pytest.fixture(scope="module")
def sm():
    import smfft_amd as sm
    assert sm.lib.smfft_device_count() >= 1, "no HIP device visible"
    sm.FFT_init()
    return sm


@pytest.fixture(scope="module")
def lr(sm):
    from smfft_amd import large_real
    return large_real


def _ref(x, inverse):
    from oracle import np_reference as ref
    return ref.c2r_packed(x) if inverse else ref.r2c_packed(x)


def _input(rng, nffts, n, inverse):
    """R2C: real (nFFTs, N) float32; C2R: packed (nFFTs, N/2) complex64"""
    if inverse:
        return (rng.random((nffts, n // 2), dtype=np.float32) - 0.5 + 1j * (rng.random((nffts, n // 2), dtype=np.float32) - 0.5)).astype(np.complex64)
    return (rng.random((nffts, n), dtype=np.float32) - 0.5).astype(np.float32)


def _gaussian(rng, nffts, n, inverse):
    if inverse:
        return (rng.standard_normal((nffts, n // 2)) + 1j * rng.standard_normal((nffts, n // 2))).astype(np.complex64)
    return rng.standard_normal((nffts, n)).astype(np.float32)


def _call(lr, x, inverse):
    return lr.c2r(x) if inverse else lr.r2c(x)


def _out_shape(n, nffts, inverse):
    return ((nffts, n), np.float32) if inverse else ((nffts, n // 2), np.complex64)


def _assert_rows_close(got, x, inverse, what):
    from oracle import np_reference as ref
    want = _ref(x, inverse)
    for f in range(x.shape[0]):
        l2, mx = ref.fft_errors(got[f], want[f])
        assert l2 <= ref.REL_L2_TOL and mx <= ref.MAX_ABS_TOL, f"{what} FFT {f}: relL2={l2:.3e} maxabs={mx:.3e}"


def _batches(lr, n):
    g = lr.grid(n)
    assert g >= 1
    return [1, 2, 3, 7, (5 * g) // 2 + 3]      # the last: 2.5 grids and a ragged tail


def _ceiling(n):
    return 3 * (math.log2(n) + 2) * 2.0 ** -24


@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_real_parity(lr, n, inverse):
    rng = np.random.default_rng([n, int(inverse)])
    for nffts in _batches(lr, n):
        x = _input(rng, nffts, n, inverse)
        got = _call(lr, x, inverse)
        assert got.shape == _out_shape(n, nffts, inverse)[0]
        _assert_rows_close(got, x, inverse, f"N={n} inverse={inverse} nFFTs={nffts}")


@pytest.mark.parametrize("n", SIZES)
def test_large_real_round_trip(lr, n):
    from oracle import np_reference as ref
    x = _input(np.random.default_rng(3), 5, n, False)
    back = lr.c2r(lr.r2c(x))
    for f in range(5):
        l2, mx = ref.fft_errors(back[f], (n / 2) * x[f].astype(np.float64))
        assert l2 <= ref.REL_L2_TOL and mx <= ref.MAX_ABS_TOL, (f, l2, mx)


def _assert_probe(got, want, n, what):
    err = np.abs(got.astype(np.complex128 if np.iscomplexobj(got) else np.float64) - want)
    ceiling = _ceiling(n)
    assert err.max() <= ceiling, f"{what}: per-element {err.max():.3e} > {ceiling:.3e} (row {np.unravel_index(err.argmax(), err.shape)})"
    assert np.sqrt(np.mean(err ** 2)) <= ceiling, what


@pytest.mark.parametrize("n", SIZES)
def test_large_real_dft_matrix_probe_r2c(lr, n):
    """Real unit impulses at 0, 1, N/2 - 1, N/2, N - 1 and 40 random positions: every packed output element of row j is W_N^{jk}
    (element 0: (1, (-1)^j)); its error, per element and as rms, stays under the twiddle-chain ceiling 3 (log2 N + 2) 2^-24."""
    rng = np.random.default_rng(11)
    pos = np.unique(np.concatenate([[0, 1, n // 2 - 1, n // 2, n - 1], rng.integers(0, n, 40)]))
    x = np.zeros((len(pos), n), dtype=np.float32)
    x[np.arange(len(pos)), pos] = 1
    _assert_probe(lr.r2c(x), _ref(x, False), n, f"N={n} R2C impulses")


@pytest.mark.parametrize("n", SIZES)
def test_large_real_dft_matrix_probe_c2r(lr, n):
    """Spectra with one bin set: DC alone, Nyquist alone (element 0's imaginary part), bins 1, L - 1, L/2 and 40 random bins, each
    with a unit value and with a random unit phase; every output sample is within the probe ceiling of (N/2) irfft."""
    L = n // 2
    rng = np.random.default_rng(13)
    bins = np.unique(np.concatenate([[1, L - 1, L // 2], rng.integers(1, L, 40)]))
    rows = [(0, 1.0 + 0j), (0, 1j)]
    for k in bins:
        rows += [(k, 1.0 + 0j), (k, np.exp(2j * np.pi * rng.random()))]
    xp = np.zeros((len(rows), L), dtype=np.complex64)
    for r, (k, v) in enumerate(rows):
        xp[r, k] = v
    _assert_probe(lr.c2r(xp), _ref(xp, True), n, f"N={n} C2R single bins")


@pytest.mark.parametrize("n", SIZES)
def test_large_real_constant_and_alternating_inputs(lr, n):
    """x = 1/N gives DC = 1 alone, x = (-1)^n / N Nyquist = 1 alone, both in the packed slot 0; every other bin is zero within the
    probe ceiling."""
    x = np.stack([np.full(n, 1.0 / n), (-1.0) ** np.arange(n) / n]).astype(np.float32)
    got = lr.r2c(x).astype(np.complex128)
    ceiling = _ceiling(n)
    assert abs(got[0, 0] - 1) <= ceiling and abs(got[1, 0] - 1j) <= ceiling, got[:, 0]
    assert np.abs(got[:, 1:]).max() <= ceiling


@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_real_zero_mean_accuracy(lr, n, inverse):
    nffts = (1 << 21) // n + 1
    x = _gaussian(np.random.default_rng(5), nffts, n, inverse)
    want = _ref(x, inverse)
    got = _call(lr, x, inverse)
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert rel <= 5e-7, rel


@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_real_isolation_and_exact_scaling(lr, n, inverse):
    """A NaN in one FFT reaches exactly that FFT (in a batch that wraps the persistent grid); scaling the input by 2^e scales
    every output bit for bit."""
    nffts = lr.grid(n) + 5
    x = _input(np.random.default_rng(7), nffts, n, inverse)
    clean = _call(lr, x, inverse)
    assert np.isfinite(clean).all()
    bad = x.copy()
    victim = nffts - 3
    bad[victim, 1234] = np.nan
    got = _call(lr, bad, inverse)
    assert not np.isfinite(got[victim]).any()
    others = np.arange(nffts) != victim
    assert np.array_equal(got[others].view(np.uint32), clean[others].view(np.uint32))
    for e in (-3, 5):
        scaled = _call(lr, (x * np.float32(2.0 ** e)).astype(x.dtype), inverse)
        want = (clean * np.float32(2.0 ** e)).astype(clean.dtype)
        assert np.array_equal(scaled.view(np.uint32), want.view(np.uint32)), e


GUARD = 128 << 10      # bytes of NaN payload on each side of every buffer


def _guarded(sm, nbytes, fill):
    buf = sm.DeviceBuffer(nbytes + 2 * GUARD)
    sm.lib.smfft_memset(buf.ptr, fill, buf.nbytes)
    return buf


def _bytes(buf, off, nbytes):
    out = np.empty(nbytes, dtype=np.uint8)
    from smfft_amd import api
    api._ck(api.lib.smfft_memcpy_d2h(out.ctypes.data, buf.ptr + off, nbytes), "memcpy_d2h")
    return out


@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_real_guarded_buffers_and_interior_pointers(sm, lr, n, inverse):
    """Input and output are interior pointers (8 B past an allocation's guard); the output is prefilled with NaN and the guards
    before and after both buffers keep their bytes; the input is not modified; the bits are those of a call at allocation bases."""
    from smfft_amd import api
    nffts = lr.grid(n) + 3
    x = _input(np.random.default_rng(9), nffts, n, inverse)
    nbytes = x.nbytes
    assert nbytes == nffts * n * F
    din, dout = _guarded(sm, nbytes + 8, 0x7F), _guarded(sm, nbytes + 8, 0xFF)
    off = GUARD + 8
    api._ck(api.lib.smfft_memcpy_h2d(din.ptr + off, x.ctypes.data, nbytes), "memcpy_h2d")
    before_in = _bytes(din, 0, din.nbytes)
    before_out = _bytes(dout, 0, dout.nbytes)
    rc, ms = lr.benchmark(din.ptr + off, dout.ptr + off, n, nffts, inverse)
    assert rc == 0 and ms > 0
    after_out = _bytes(dout, 0, dout.nbytes)
    assert np.array_equal(_bytes(din, 0, din.nbytes), before_in), "the input buffer changed"
    assert np.array_equal(after_out[:off], before_out[:off]), "a write before the output"
    assert np.array_equal(after_out[off + nbytes:], before_out[off + nbytes:]), "a write past the output"
    shape, dtype = _out_shape(n, nffts, inverse)
    got = after_out[off:off + nbytes].view(dtype).reshape(shape)
    _assert_rows_close(got, x, inverse, f"N={n} interior")
    assert np.array_equal(got.view(np.uint32), _call(lr, x, inverse).view(np.uint32))
    din.free()
    dout.free()


@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_real_in_place(sm, lr, n, inverse):
    nffts = 2 * lr.grid(n) + 1
    x = _input(np.random.default_rng(13), nffts, n, inverse)
    buf = sm.DeviceBuffer.from_host(x)
    rc, _ = lr.benchmark(buf.ptr, buf.ptr, n, nffts, inverse)
    assert rc == 0
    shape, dtype = _out_shape(n, nffts, inverse)
    got = buf.to_host(dtype, shape)
    buf.free()
    assert np.array_equal(got.view(np.uint32), _call(lr, x, inverse).view(np.uint32))


@pytest.mark.parametrize("in_place", (False, True), ids=("out_of_place", "in_place"))
@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_real_position_invariance(sm, lr, n, inverse, in_place):
    """One Gaussian row in every position of a batch of 3G + G/2 + 1 rows (G = the persistent grid): every output row has the bits
    of the call on that row alone, whatever its round, its workgroup or (at 16384) the workgroup beside it on its CU."""
    g = lr.grid(n)
    nffts = 3 * g + g // 2 + 1
    row = _gaussian(np.random.default_rng([n, int(inverse), 23]), 1, n, inverse)
    alone = _call(lr, row, inverse)
    _assert_rows_close(alone, row, inverse, f"N={n} one FFT")
    x = np.repeat(row, nffts, axis=0)
    if in_place:
        buf = sm.DeviceBuffer.from_host(x)
        rc, _ = lr.benchmark(buf.ptr, buf.ptr, n, nffts, inverse)
        assert rc == 0
        shape, dtype = _out_shape(n, nffts, inverse)
        got = buf.to_host(dtype, shape)
        buf.free()
    else:
        got = _call(lr, x, inverse)
    bad = np.nonzero((got.view(np.uint32) != alone.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, f"N={n} inverse={inverse} G={g}: {bad.size} rows differ from the FFT alone, the first {bad[:8].tolist()}"


@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_real_guarded_batches_and_offsets(sm, lr, n, inverse):
    """tests/test_buffers_gpu.py's regime around the persistent grid G: batches of 1, G - 1, G + 1 and 3G + 1 FFTs on [guard |
    payload | guard] allocations whose guards hold a NaN payload, the payload 8 B past the guard (the largest batch also 4096 - 8 B),
    out of place and in place.  The input allocation holds two more FFTs of that NaN past nFFTs.  The written FFTs are within the fp64
    tolerances, no other byte of the output allocation changes, the input allocation does not change (out of place), and the result
    has the bits of the call at allocation bases."""
    from tests import test_buffers_gpu as tb
    g = lr.grid(n)
    rng = np.random.default_rng([n, int(inverse), 29])
    for nffts in (1, g - 1, g + 1, 3 * g + 1):
        x = _input(rng, nffts, n, inverse)
        want = _ref(x, inverse)
        shape, dtype = _out_shape(n, nffts, inverse)

        def call(d_in, d_out, nffts=nffts):
            return lr.lib().smfft_large_real_launch(d_in, d_out, n, nffts, int(inverse), None)
        base = tb._at_base(sm, call, x, dtype, shape)
        for offset in (tb.OFFSET,) + ((4096 - 8,) if nffts == 3 * g + 1 else ()):
            for in_place in (False, True):
                what = f"N={n} inverse={inverse} nFFTs={nffts} offset={offset}{' in place' if in_place else ''}"
                got = tb._guarded(sm, call, x, nffts + 2, n * F, nffts, offset, in_place)
                tb._within(got.view(dtype).reshape(shape), want, 1, what)
                tb._same_bits(got, base, what)


_STREAM_SCRIPT = r"""
import sys
import numpy as np
import torch                                  # first: torch initialises the HIP runtime before the library uses it
sys.path.insert(0, sys.argv[1])
from smfft_amd import large_real
from oracle import np_reference as ref
n, nffts = int(sys.argv[2]), 9
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(device=dev)
rng = np.random.default_rng(17)
x = (rng.random((nffts, n), dtype=np.float32) - 0.5).astype(np.float32)
with torch.cuda.stream(s):
    src = torch.from_numpy(x).to(dev)
    a = (src * 2).contiguous()                # queued on s before the R2C
    b = torch.empty((nffts, n // 2), dtype=torch.complex64, device=dev)
    large_real.launch(a.data_ptr(), b.data_ptr(), n, nffts, False, s.cuda_stream)
    c = (b * 0.5).contiguous()                # queued on s after it
    d = torch.empty((nffts, n), dtype=torch.float32, device=dev)
    large_real.launch(c.data_ptr(), d.data_ptr(), n, nffts, True, s.cuda_stream)
    e = (d * (2.0 / n)).contiguous()          # and after the C2R
s.synchronize()
got = c.cpu().numpy().astype(np.complex128)
want = ref.r2c_packed(x)
err = np.sqrt((np.abs(got - want) ** 2).sum(-1) / (np.abs(want) ** 2).sum(-1)).max()
back = e.cpu().numpy().astype(np.float64)
err2 = np.sqrt(((back - x) ** 2).sum(-1) / (x.astype(np.float64) ** 2).sum(-1)).max()
print("relL2", err, err2)
sys.exit(0 if err <= 5e-7 and err2 <= 5e-7 else 1)
"""


@pytest.mark.parametrize("n", SIZES)
def test_large_real_caller_stream_ordering(n):
    """Launches go on the caller's stream: torch work queued before, between and after an R2C and a C2R on that stream sees them in
    order.  (In a process of its own that imports torch first, as a torch user's program does.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _STREAM_SCRIPT, root, str(n)], capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stdout + p.stderr


def test_large_real_benchmark_accumulates_and_rejects(lr, sm):
    n, nffts = 16384, 4
    x = sm.DeviceBuffer.from_host(_input(np.random.default_rng(1), nffts, n, False))
    y = sm.DeviceBuffer(x.nbytes)
    t = ctypes.c_double(1000.0)
    assert lr.lib().smfft_large_real_benchmark(x.ptr, y.ptr, n, nffts, 0, ctypes.byref(t)) == 0
    assert t.value > 1000.0
    t0 = t.value
    assert lr.lib().smfft_large_real_benchmark(x.ptr, y.ptr, 32768, nffts // 2, 1, ctypes.byref(t)) == 0
    assert t.value > t0
    t1 = t.value
    assert lr.lib().smfft_large_real_benchmark(x.ptr, y.ptr, n, 0, 0, ctypes.byref(t)) == 0
    for bad_n in (8192, 4096, 65536):
        assert lr.lib().smfft_large_real_benchmark(x.ptr, y.ptr, bad_n, nffts, 0, ctypes.byref(t)) == -1
    assert lr.lib().smfft_large_real_benchmark(x.ptr, y.ptr, n, -1, 1, ctypes.byref(t)) == -1
    assert t.value == t1
    assert lr.lib().smfft_large_real_launch(x.ptr, y.ptr, n, -1, 0, None) == -1
    x.free()
    y.free()


def test_large_real_64bit_offsets(sm, lr):
    """N = 32768 (16384 float2 per FFT), 2^17 + 3 FFTs in place (16 GiB, 2^31 + 3 * 2^14 float2 elements): R2C, then C2R of its
    output; the FFTs whose elements lie past 2^31 and a sample before are transformed both ways."""
    from smfft_amd import api
    n = 32768
    half = n // 2
    f31 = (1 << 31) // half                    # the FFT that starts at float2 element 2^31
    nffts = f31 + 3
    rng = np.random.default_rng(19)
    buf = sm.DeviceBuffer(n * nffts * F)
    check = [0, 1, 77777, f31 - 1, f31, f31 + 1, f31 + 2]
    rows = {}
    try:
        assert sm.lib.smfft_memset(buf.ptr, 0, buf.nbytes) == 0
        for f in check:
            rows[f] = _input(rng, 1, n, False)
            api._ck(api.lib.smfft_memcpy_h2d(buf.ptr + f * n * F, rows[f].ctypes.data, n * F), "memcpy_h2d")
        rc, _ = lr.benchmark(buf.ptr, buf.ptr, n, nffts, False)
        assert rc == 0
        spectra = {}
        for f in check:
            got = np.empty((1, half), dtype=np.complex64)
            api._ck(api.lib.smfft_memcpy_d2h(got.ctypes.data, buf.ptr + f * n * F, n * F), "memcpy_d2h")
            _assert_rows_close(got, rows[f], False, f"R2C N={n} FFT {f}")
            spectra[f] = got
        rc, _ = lr.benchmark(buf.ptr, buf.ptr, n, nffts, True)
        assert rc == 0
        for f in check:
            got = np.empty((1, n), dtype=np.float32)
            api._ck(api.lib.smfft_memcpy_d2h(got.ctypes.data, buf.ptr + f * n * F, n * F), "memcpy_d2h")
            _assert_rows_close(got, spectra[f], True, f"C2R N={n} FFT {f}")
    finally:
        buf.free()


def test_large_real_concurrent_streams(sm, lr):
    """Two host threads, each with a stream of its own (hipStreamCreate), launch beside each other: one R2C of N = 16384 over 8G + 5
    FFTs, the other a C2R of N = 32768 over 4G + 3 FFTs and, behind it on the same stream, a C2C of N = 16384 from libsmfft_large.so.
    Each launch runs twice per round, so the kernels share the chip, and every output has the bits of its solo run on the null
    stream.  At most three streams exist at a time, and no graph."""
    import threading

    from smfft_amd import large
    hip = ctypes.CDLL("libamdhip64.so")
    g16, g32 = lr.grid(16384), lr.grid(32768)
    rng = np.random.default_rng(31)
    inputs = [_input(rng, 8 * g16 + 5, 16384, False), _input(rng, 4 * g32 + 3, 32768, True),
              (rng.random((large.grid(16384) + 7, 16384), dtype=np.float32) - 0.5).astype(np.complex64)]
    dins = [sm.DeviceBuffer.from_host(x) for x in inputs]
    douts = [sm.DeviceBuffer(x.nbytes) for x in inputs]
    wants = []
    try:
        solo = [lambda s: lr.launch(dins[0].ptr, douts[0].ptr, 16384, inputs[0].shape[0], False, s),
                lambda s: lr.launch(dins[1].ptr, douts[1].ptr, 32768, inputs[1].shape[0], True, s),
                lambda s: large.launch(dins[2].ptr, douts[2].ptr, 16384, inputs[2].shape[0], False, s)]
        for k, launch in enumerate(solo):
            assert sm.lib.smfft_memset(douts[k].ptr, 0xFF, douts[k].nbytes) == 0
            launch(0)
            assert sm.lib.smfft_synchronize() == 0
            wants.append(douts[k].to_host(np.uint32, (douts[k].nbytes // 4,)))
        assert all(np.isfinite(w.view(np.float32)).all() for w in wants)
        errors = []

        def work(mine):
            try:
                stream = ctypes.c_void_p()
                assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
                try:
                    for rep in range(4):
                        for k in mine:
                            assert hip.hipMemsetAsync(ctypes.c_void_p(douts[k].ptr), 0xFF, ctypes.c_size_t(douts[k].nbytes), stream) == 0
                        for _ in range(2):
                            for k in mine:
                                solo[k](stream.value)
                        assert hip.hipStreamSynchronize(stream) == 0
                        for k in mine:
                            got = douts[k].to_host(np.uint32, (douts[k].nbytes // 4,))
                            assert np.array_equal(got, wants[k]), f"job {k} round {rep}"
                finally:
                    hip.hipStreamDestroy(stream)
            except Exception as e:       # noqa: BLE001  (reported to the main thread)
                errors.append(repr(e))
        threads = [threading.Thread(target=work, args=(mine,)) for mine in ((0,), (1, 2))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
    finally:
        for b in dins + douts:
            b.free()
