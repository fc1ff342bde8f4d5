"""The N = 8192 / 16384 single-pass C2C kernels of libsmfft_large.so (include/smfft_large.h) on an MI355X, against numpy.fft in
complex128: parity over ragged batches (one FFT to 2.5 persistent grids), the round trip, per-element DFT-matrix probes, zero-mean
accuracy, isolation and exact scaling, one row's bits in every position of a batch, guarded buffers, interior pointers, in-place
calls, batches around the persistent grid G in tests/test_buffers_gpu.py's regime, a caller's stream, two host threads launching
beside each other, the timed form, and 64-bit element offsets (16 GiB) at both lengths.  (The full DFT-matrix probe, the ratchet
and the isolation test of every round are the `large` cases of tests/test_probes_gpu.py.)"""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (8192, 16384)
DIRS = (False, True)
F2 = 8          # bytes per complex fp32 element


@pytest.fixture(scope="module")
def sm():
    import smfft_amd as sm
    assert sm.lib.smfft_device_count() >= 1, "no HIP device visible"
    sm.FFT_init()
    return sm


@pytest.fixture(scope="module")
def lg(sm):
    from smfft_amd import large
    return large


def _ref(x, inverse):
    x = np.asarray(x, dtype=np.complex128)
    n = x.shape[-1]
    return np.fft.ifft(x, axis=-1) * n if inverse else np.fft.fft(x, axis=-1)


def _signal(rng, nffts, n):
    return (rng.random((nffts, n), dtype=np.float32) - 0.5 + 1j * (rng.random((nffts, n), dtype=np.float32) - 0.5)).astype(np.complex64)


def _assert_rows_close(got, x, inverse, what):
    from oracle import np_reference as ref
    want = _ref(x, inverse)
    for f in range(x.shape[0]):
        l2, mx = ref.fft_errors(got[f], want[f])
        assert l2 <= ref.REL_L2_TOL and mx <= ref.MAX_ABS_TOL, f"{what} FFT {f}: relL2={l2:.3e} maxabs={mx:.3e}"


def _batches(lg, n):
    g = lg.grid(n)
    assert g >= 1
    return [1, 2, 3, 7, (5 * g) // 2 + 3]      # the last: 2.5 grids and a ragged tail


@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_parity(lg, n, inverse):
    rng = np.random.default_rng(n + int(inverse))
    for nffts in _batches(lg, n):
        x = _signal(rng, nffts, n)
        got = lg.c2c(x, inverse)
        _assert_rows_close(got, x, inverse, f"N={n} inverse={inverse} nFFTs={nffts}")


@pytest.mark.parametrize("n", SIZES)
def test_large_round_trip(lg, n):
    x = _signal(np.random.default_rng(3), 5, n)
    back = lg.c2c(lg.c2c(x, False), True)
    from oracle import np_reference as ref
    for f in range(5):
        l2, mx = ref.fft_errors(back[f], n * x[f].astype(np.complex128))
        assert l2 <= ref.REL_L2_TOL and mx <= ref.MAX_ABS_TOL, (f, l2, mx)


@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_dft_matrix_probe(lg, n, inverse):
    """Unit impulses at 0, 1, N/2 - 1, N - 1 and 60 random positions: every output element of row k is W^{jk}; its error, per
    element and as rms, stays under the twiddle-chain ceiling 3 (log2 N + 2) 2^-24 of tests/probe_cases.py."""
    rng = np.random.default_rng(11)
    pos = np.unique(np.concatenate([[0, 1, n // 2 - 1, n - 1], rng.integers(0, n, 60)]))
    x = np.zeros((len(pos), n), dtype=np.complex64)
    x[np.arange(len(pos)), pos] = 1
    got = lg.c2c(x, inverse).astype(np.complex128)
    err = np.abs(got - _ref(x, inverse))
    ceiling = 3 * (math.log2(n) + 2) * 2.0 ** -24
    assert err.max() <= ceiling, f"per-element {err.max():.3e} > {ceiling:.3e}"
    assert np.sqrt(np.mean(err ** 2)) <= ceiling


@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_zero_mean_accuracy(lg, n, inverse):
    nffts = (1 << 21) // n + 1
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((nffts, n)) + 1j * rng.standard_normal((nffts, n))).astype(np.complex64)
    want = _ref(x, inverse)
    got = lg.c2c(x, inverse)
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert rel <= 5e-7, rel


@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_isolation_and_exact_scaling(lg, n, inverse):
    """A NaN in one FFT reaches exactly that FFT (in a batch that wraps the persistent grid); scaling the input by 2^e scales
    every output bit for bit."""
    nffts = lg.grid(n) + 5
    x = _signal(np.random.default_rng(7), nffts, n)
    clean = lg.c2c(x, inverse)
    assert np.isfinite(clean).all()
    bad = x.copy()
    victim = nffts - 3
    bad[victim, 1234] = np.nan
    got = lg.c2c(bad, inverse)
    assert not np.isfinite(got[victim]).any()
    others = np.arange(nffts) != victim
    assert np.array_equal(got[others].view(np.uint32), clean[others].view(np.uint32))
    for e in (-3, 5):
        scaled = lg.c2c((x * np.float32(2.0 ** e)).astype(np.complex64), inverse)
        want = (clean * np.float32(2.0 ** e)).astype(np.complex64)
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
def test_large_guarded_buffers_and_interior_pointers(sm, lg, n, inverse):
    """Input and output are interior pointers (8 B past an allocation's guard); the output is prefilled with NaN and the guards
    before and after both buffers keep their bytes; the input is not modified."""
    from smfft_amd import api
    nffts = lg.grid(n) + 3
    x = _signal(np.random.default_rng(9), nffts, n)
    nbytes = x.nbytes
    din, dout = _guarded(sm, nbytes + 8, 0x7F), _guarded(sm, nbytes + 8, 0xFF)
    off = GUARD + 8
    api._ck(api.lib.smfft_memcpy_h2d(din.ptr + off, x.ctypes.data, nbytes), "memcpy_h2d")
    before_in = _bytes(din, 0, din.nbytes)
    before_out = _bytes(dout, 0, dout.nbytes)
    rc, ms = lg.benchmark(din.ptr + off, dout.ptr + off, n, nffts, inverse)
    assert rc == 0 and ms > 0
    after_out = _bytes(dout, 0, dout.nbytes)
    assert np.array_equal(_bytes(din, 0, din.nbytes), before_in), "the input buffer changed"
    assert np.array_equal(after_out[:off], before_out[:off]), "a write before the output"
    assert np.array_equal(after_out[off + nbytes:], before_out[off + nbytes:]), "a write past the output"
    got = after_out[off:off + nbytes].view(np.complex64).reshape(nffts, n)
    _assert_rows_close(got, x, inverse, f"N={n} interior")
    # the same bits as a call at allocation bases
    assert np.array_equal(got.view(np.uint32), lg.c2c(x, inverse).view(np.uint32))


@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_in_place(sm, lg, n, inverse):
    nffts = 2 * lg.grid(n) + 1
    x = _signal(np.random.default_rng(13), nffts, n)
    buf = sm.DeviceBuffer.from_host(x)
    rc, _ = lg.benchmark(buf.ptr, buf.ptr, n, nffts, inverse)
    assert rc == 0
    got = buf.to_host(np.complex64, x.shape)
    assert np.array_equal(got.view(np.uint32), lg.c2c(x, inverse).view(np.uint32))


_STREAM_SCRIPT = r"""
import sys
import numpy as np
import torch                                  # first: torch initialises the HIP runtime before the library uses it
sys.path.insert(0, sys.argv[1])
from smfft_amd import large
n, nffts = 16384, 9
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(device=dev)
rng = np.random.default_rng(17)
x = (rng.random((nffts, n), dtype=np.float32) - 0.5 + 1j * (rng.random((nffts, n), dtype=np.float32) - 0.5)).astype(np.complex64)
with torch.cuda.stream(s):
    src = torch.from_numpy(x).to(dev)
    a = (src * 2).contiguous()                # queued on s before the transform
    b = torch.empty_like(a)
    large.launch(a.data_ptr(), b.data_ptr(), n, nffts, False, s.cuda_stream)
    c = (b * 0.5).contiguous()                # queued on s after it
s.synchronize()
got = c.cpu().numpy().astype(np.complex128)
want = np.fft.fft(x.astype(np.complex128), axis=-1)
err = np.sqrt((np.abs(got - want) ** 2).sum(-1) / (np.abs(want) ** 2).sum(-1)).max()
print("relL2", err)
sys.exit(0 if err <= 5e-7 else 1)
"""


def test_large_caller_stream_ordering():
    """Launches go on the caller's stream: torch work queued before and after on that stream sees them in order.  (In a process of
    its own that imports torch first, as a torch user's program does.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _STREAM_SCRIPT, root], capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stdout + p.stderr


def test_large_benchmark_accumulates_and_rejects(lg, sm):
    n, nffts = 8192, 4
    x = sm.DeviceBuffer.from_host(_signal(np.random.default_rng(1), nffts, n))
    y = sm.DeviceBuffer(x.nbytes)
    t = ctypes.c_double(1000.0)
    assert lg.lib().smfft_large_benchmark(x.ptr, y.ptr, n, nffts, 0, ctypes.byref(t)) == 0
    assert t.value > 1000.0
    t0 = t.value
    assert lg.lib().smfft_large_benchmark(x.ptr, y.ptr, n, nffts, 1, ctypes.byref(t)) == 0
    assert t.value > t0
    assert lg.lib().smfft_large_benchmark(x.ptr, y.ptr, n, 0, 0, ctypes.byref(t)) == 0
    assert lg.lib().smfft_large_benchmark(x.ptr, y.ptr, 4096, nffts, 0, ctypes.byref(t)) == -1
    assert lg.lib().smfft_large_launch(x.ptr, y.ptr, n, -1, 0, None) == -1


def _in_place_past_2_31(sm, lg, n, seed):
    """N-point transforms in place over 2^31 / N + 3 FFTs (16 GiB): the FFTs whose elements lie past 2^31 and a sample before are
    transformed"""
    f31 = (1 << 31) // n                       # the FFT that starts at element 2^31
    nffts = f31 + 3
    rng = np.random.default_rng(seed)
    from smfft_amd import api
    buf = sm.DeviceBuffer(n * nffts * F2)
    check = [0, 1, 77777, f31 - 1, f31, f31 + 1, f31 + 2]
    rows = {}
    sm.lib.smfft_memset(buf.ptr, 0, buf.nbytes)
    for f in check:
        rows[f] = _signal(rng, 1, n)
        api._ck(api.lib.smfft_memcpy_h2d(buf.ptr + f * n * F2, rows[f].ctypes.data, n * F2), "memcpy_h2d")
    rc, _ = lg.benchmark(buf.ptr, buf.ptr, n, nffts, False)
    assert rc == 0
    for f in check:
        got = np.empty((1, n), dtype=np.complex64)
        api._ck(api.lib.smfft_memcpy_d2h(got.ctypes.data, buf.ptr + f * n * F2, n * F2), "memcpy_d2h")
        _assert_rows_close(got, rows[f], False, f"N={n} FFT {f}")
    buf.free()


def test_large_64bit_offsets(sm, lg):
    """N = 16384, 2^17 + 3 FFTs in place (16 GiB): the FFTs whose elements lie past 2^31 and a sample before are transformed."""
    _in_place_past_2_31(sm, lg, 16384, 19)


def test_large_64bit_offsets_8192(sm, lg):
    """N = 8192 (an object of its own, with its own addressing code), 2^18 + 3 FFTs in place (16 GiB)."""
    _in_place_past_2_31(sm, lg, 8192, 37)


# ---------------------------------------------------------------------------------------------------- across the persistent loop
@pytest.mark.parametrize("in_place", (False, True), ids=("out_of_place", "in_place"))
@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_position_invariance(sm, lg, n, inverse, in_place):
    """One Gaussian row in every position of a batch of 3G + G/2 + 1 rows (G = the persistent grid): every output row has the bits
    of the call on that row alone, whatever its round, its workgroup or (at 8192) the workgroup beside it on its CU."""
    g = lg.grid(n)
    nffts = 3 * g + g // 2 + 1
    rng = np.random.default_rng([n, int(inverse), 23])
    row = (rng.standard_normal((1, n)) + 1j * rng.standard_normal((1, n))).astype(np.complex64)
    alone = lg.c2c(row, inverse)
    _assert_rows_close(alone, row, inverse, f"N={n} one FFT")
    x = np.repeat(row, nffts, axis=0)
    if in_place:
        buf = sm.DeviceBuffer.from_host(x)
        rc, _ = lg.benchmark(buf.ptr, buf.ptr, n, nffts, inverse)
        assert rc == 0
        got = buf.to_host(np.complex64, x.shape)
        buf.free()
    else:
        got = lg.c2c(x, inverse)
    bad = np.nonzero((got.view(np.uint32) != alone.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, f"N={n} inverse={inverse} G={g}: {bad.size} rows differ from the FFT alone, the first {bad[:8].tolist()}"


@pytest.mark.parametrize("inverse", DIRS)
@pytest.mark.parametrize("n", SIZES)
def test_large_guarded_batches_and_offsets(sm, lg, n, inverse):
    """tests/test_buffers_gpu.py's regime around the persistent grid G: batches of 1, G - 1, G + 1 and 3G + 1 FFTs on [guard |
    payload | guard] allocations whose guards hold a NaN payload, the payload 8 B past the guard (the largest batch also 4096 - 8 B),
    out of place and in place.  The input allocation holds two more FFTs of that NaN past nFFTs, so a kernel that reads FFT nFFTs
    and lets it reach an output fails the fp64 check.  The written FFTs are within the fp64 tolerances, no other byte of the output
    allocation changes, the input allocation does not change (out of place), and the result has the bits of the call at
    allocation bases."""
    from tests import test_buffers_gpu as tb
    g = lg.grid(n)
    rng = np.random.default_rng([n, int(inverse), 29])
    for nffts in (1, g - 1, g + 1, 3 * g + 1):
        x = _signal(rng, nffts, n)
        want = _ref(x, inverse)

        def call(d_in, d_out, nffts=nffts):
            return lg.lib().smfft_large_launch(d_in, d_out, n, nffts, int(inverse), None)
        base = tb._at_base(sm, call, x, np.complex64, x.shape)
        for offset in (tb.OFFSET,) + ((4096 - 8,) if nffts == 3 * g + 1 else ()):
            for in_place in (False, True):
                what = f"N={n} inverse={inverse} nFFTs={nffts} offset={offset}{' in place' if in_place else ''}"
                got = tb._guarded(sm, call, x, nffts + 2, n * F2, nffts, offset, in_place)
                tb._within(got.view(np.complex64).reshape(nffts, n), want, 1, what)
                tb._same_bits(got, base, what)


def test_large_concurrent_streams_and_co_residency(sm, lg):
    """Two host threads, each with a stream of its own (hipStreamCreate; second pass: hipStreamPerThread, one handle that names a
    different stream in each thread), launch beside each other: one N = 8192 (forward) over 8G + 5 FFTs, the other N = 16384
    (inverse) over 4G + 3 FFTs and, behind it on the same stream, an external N = 1024 batch of libsmfft_amd.so.  Each launch runs
    twice per round, so the kernels share the chip -- a CU holds two 8192 workgroups, or one beside a 16384 or a 1024 workgroup --
    and every output has the bits of its solo run on the null stream.  At most three streams exist at a time, and no graph."""
    import threading
    hip = ctypes.CDLL("libamdhip64.so")
    g8, g16 = lg.grid(8192), lg.grid(16384)
    jobs = [(8192, 8 * g8 + 5, False), (16384, 4 * g16 + 3, True), (1024, 16384, False)]      # (N, nFFTs, inverse)
    rng = np.random.default_rng(31)
    dins, douts, wants = [], [], []
    try:
        for n, nffts, inverse in jobs:
            dins.append(sm.DeviceBuffer.from_host(_signal(rng, nffts, n)))
            douts.append(sm.DeviceBuffer(nffts * n * F2))
        solo = [lambda s: lg.launch(dins[0].ptr, douts[0].ptr, 8192, jobs[0][1], jobs[0][2], s),
                lambda s: lg.launch(dins[1].ptr, douts[1].ptr, 16384, jobs[1][1], jobs[1][2], s),
                lambda s: sm.launch("ct", "external", dins[2].ptr, douts[2].ptr, 1024, jobs[2][1], jobs[2][2], True, stream=s)]
        for k, launch in enumerate(solo):
            assert sm.lib.smfft_memset(douts[k].ptr, 0xFF, douts[k].nbytes) == 0
            launch(0)
            assert sm.lib.smfft_synchronize() == 0
            wants.append(douts[k].to_host(np.uint32, (douts[k].nbytes // 4,)))
        assert all(np.isfinite(w.view(np.float32)).all() for w in wants)
        errors = []

        def work(mine, use_per_thread):
            try:
                stream = ctypes.c_void_p(2) if use_per_thread else ctypes.c_void_p()       # 2: hipStreamPerThread
                if not use_per_thread:
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
                            assert np.array_equal(got, wants[k]), f"job {jobs[k][:2]} round {rep} per-thread={use_per_thread}"
                finally:
                    if not use_per_thread:
                        hip.hipStreamDestroy(stream)
            except Exception as e:       # noqa: BLE001  (reported to the main thread)
                errors.append(repr(e))
        for use_per_thread in (False, True):
            threads = [threading.Thread(target=work, args=(mine, use_per_thread)) for mine in ((0,), (1, 2))]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            assert not errors, errors
    finally:
        for b in dins + douts:
            b.free()
