"""The overlap-save FIR filter banks for real signals and real taps on an MI355X (smfft_fir_real_prepare / smfft_fir_real_launch,
smfft_amd.fir_real) against fp64 NumPy: both modes at every transform length over a grid of taps, channels, filters and signal lengths
(odd segment counts put a pair without a second segment into the middle of a workgroup tile); the filter-group split, uneven groups
included; the grid-stride loop past the grid cap; the prepared spectra and spectra from elsewhere; a caller's stream, the benchmark form
and fir(); 64-bit output offsets; three probes (exact scaling, a NaN sample, a NaN tap); guarded buffers at offset bases.

The reference is tests/fir_gpu_harness.py's _reference on the real arrays and the check its _check_rows with its bounds unchanged
(relL2 <= 1e-6, max <= 5e-6 per (channel, filter) row, with the denominators tests/test_fir_gpu.py derives): the transforms, the
product and their rounding are the complex bank's, run on two real segments at once.  Outputs are prefilled with 0xFF, so an unwritten
one shows as NaN, and are followed by a guard of 4096 floats."""
import ctypes

import numpy as np
import pytest

from oracle.np_reference import MAX_ABS_TOL, REL_L2_TOL
from tests.fir_gpu_harness import MODES, _check_rows, _reference      # (puts tools/ on the path)

import fir_plan_model as fm  # noqa: E402
import fir_real_model as frm  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]
GUARD = 4096                   # floats after the output that must stay untouched
GRID_CAP = 12288               # smfft_fir_real.hip kFirGridCap: workgroups along the pair tiles; more tiles are grid-strided
GROUP_TARGET = 2048            # smfft_fir_real.hip kFirTargetWorkgroups: the filter-group rule's target


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def fr():
    from smfft_amd import fir_real
    fir_real.lib()
    return fir_real


def _rand(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def _prepared(sm, fr, h, N, mode):
    K, M = h.shape
    dh, dspec = sm.DeviceBuffer.from_host(h), sm.DeviceBuffer(K * N * 8)
    try:
        fr.prepare(dh.ptr, dspec.ptr, M, K, N, mode)
        assert sm.lib.smfft_synchronize() == 0
        return dspec.to_host(np.complex64, (K, N))
    finally:
        dh.free()
        dspec.free()


def _run(sm, fr, x, h, N, mode, spectra=None, finite=True):
    """prepare + launch through the device-pointer API into a NaN-prefilled output followed by a guard region; returns the (C, K, L)
    float32 result after checking that the guard is untouched and (finite) that no NaN of the prefill is left"""
    C, L = x.shape
    K, M = h.shape
    assert x.dtype == np.float32 and h.dtype == np.float32
    if spectra is None:
        spectra = _prepared(sm, fr, h, N, mode)
    dx, dspec = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(np.ascontiguousarray(spectra, dtype=np.complex64))
    total = C * K * L
    dout = sm.DeviceBuffer((total + GUARD) * 4)
    try:
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, total * 4) == 0
        assert sm.lib.smfft_memset(dout.ptr + total * 4, 0x5A, GUARD * 4) == 0
        fr.launch(dx.ptr, L, C, dspec.ptr, K, M, N, dout.ptr, mode)
        assert sm.lib.smfft_synchronize() == 0
        raw = dout.to_host(np.uint8, ((total + GUARD) * 4,))
    finally:
        for b in (dx, dspec, dout):
            b.free()
    assert np.all(raw[total * 4:] == 0x5A), "the kernel wrote past its output"
    out = raw[:total * 4].view(np.float32).reshape(C, K, L)
    if finite:
        assert np.all(np.isfinite(out)), "outputs left unwritten"
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_reference_is_numpys_definition_on_real_arrays():
    rng = np.random.default_rng(1)
    x, h = _rand(rng, (2, 300)), _rand(rng, (3, 17))
    for corr in (False, True):
        want = fm.direct(x, h, corr)
        assert np.max(np.abs(_reference(x, h, corr) - want)) <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_filter_bank_matches_numpy(sm, fr, N, mode):
    rng = np.random.default_rng(N + (mode == "correlate"))
    F = 4096 // N                                    # pairs per workgroup tile
    for M in (1, 17, N // 4 + 1, N - 1):
        V = N - M + 1
        # L < M; one segment (a pair without a partner); a pair and a lone segment; 2F + 1 segments per channel, the last one ragged:
        # F + 1 pairs, so with 3 channels an absent partner sits in mid-tile and tiles straddle channel boundaries
        for L in (max(1, M // 2), V, 2 * V + 1, (2 * F + 1) * V - 3):
            for C, K in ((1, 1), (3, 5), (3, 64)):
                x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
                got = _run(sm, fr, x, h, N, mode)
                _check_rows(got, _reference(x, h, mode == "correlate"), f"N={N} {mode} M={M} L={L} C={C} K={K}", x, h)


# ---- the filter groups and the grid-stride loop -------------------------------------------------------------------------------
def _group_plan(tiles, K):
    """(group size, grid rows) of a launch: the rule of smfft_fir.hpp fir_filter_group_size, restated"""
    groups = max(1, min(K, -(-GROUP_TARGET // tiles)))
    size = -(-K // groups)
    return size, -(-K // size)


@pytest.mark.parametrize("N,M", [(256, 65), (1024, 257), (4096, 1025)])
def test_filter_group_split_is_bit_exact(sm, fr, N, M):
    """K = 200 on a signal of 20 workgroup tiles of pairs: the launch splits the filters into 100 groups of 2; every row equals the
    K = 1 launch of its filter to the bit"""
    rng = np.random.default_rng(N)
    V, F, K = N - M + 1, 4096 // N, 200
    L = 2 * 20 * F * V - 7
    assert frm.tiles(L, 1, N, M) == 20 and _group_plan(20, K) == (2, 100)
    x, h = _rand(rng, (1, L)), _rand(rng, (K, M))
    for mode in MODES:
        spectra = _prepared(sm, fr, h, N, mode)
        all_rows = _run(sm, fr, x, h, N, mode, spectra=spectra)[0]
        dx, dspec, d1 = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(spectra), sm.DeviceBuffer(L * 4)
        for k in range(K):
            fr.launch(dx.ptr, L, 1, dspec.ptr + k * N * 8, 1, M, N, d1.ptr, mode)
            assert sm.lib.smfft_synchronize() == 0
            assert np.array_equal(_bits(d1.to_host(np.float32, (L,))), _bits(all_rows[k])), (mode, k)
        for b in (dx, dspec, d1):
            b.free()
        _check_rows(all_rows[None, ::37], _reference(x, h[::37], mode == "correlate"), f"K=200 N={N} {mode}", x, h[::37])


@pytest.mark.parametrize("N,P,K,plan", [
    (4096, 700, 7, (3, 3)),              # 3 groups of 3 filters asked and launched; the last holds one
    (4096, 450, 12, (3, 4)),             # 5 groups asked, group size 3: 4 grid rows
    (256, 699 * 16 + 5, 7, (3, 3)),
    (256, 449 * 16 + 7, 12, (3, 4)),
])
@pytest.mark.parametrize("mode", MODES)
def test_uneven_filter_groups(sm, fr, N, P, K, plan, mode):
    """The uneven-group cases of tests/test_fir_gpu.py with L rescaled to pairs: M = N - 1 (V = 2) and P pairs -- S = 2 P - 1 segments,
    so the last pair has no partner, and L = 2 S - 1 leaves the last segment one output -- on 700 / 450 tiles: filter groups of the
    rule's size with a shorter last group, and a grid of fewer rows than the groups the rule asked for.  Every row equals the K = 1
    launch of its filter (the same spectrum) to the bit and is within bounds against fp64."""
    M = N - 1
    L = 2 * (2 * P - 1) - 1
    tiles = frm.tiles(L, 1, N, M)
    assert frm.Pairs(L, N, M, False).pairs() == P and tiles == (700 if K == 7 else 450) and _group_plan(tiles, K) == plan
    asked = min(K, -(-GROUP_TARGET // tiles))
    if K == 7:
        assert asked == plan[1] and K - (plan[1] - 1) * plan[0] == 1       # the last group holds one filter
    else:
        assert asked == 5 and plan[1] == 4                                 # fewer grid rows than groups asked for
    rng = np.random.default_rng(N + K + (mode == "correlate"))
    x, h = _rand(rng, (1, L)), _rand(rng, (K, M))
    spectra = _prepared(sm, fr, h, N, mode)
    got = _run(sm, fr, x, h, N, mode, spectra=spectra)
    for k in range(K):
        one = _run(sm, fr, x, h[k:k + 1], N, mode, spectra=spectra[k:k + 1])
        assert np.array_equal(_bits(one[0, 0]), _bits(got[0, k])), (N, K, mode, k)
    _check_rows(got, _reference(x, h, mode == "correlate"), f"groups N={N} K={K} {mode}", x, h)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_grid_stride_loop_with_wrapped_prefetch(sm, fr, N, mode):
    """M = N - 1 (V = 2 outputs per segment), C = 3, K = 3, P = 10240 F + 1 pairs per channel (F = 4096 / N per tile): about 2.5 x 12288
    tiles, so every workgroup runs two or three tiles and after its last filter prefetches the first filter's spectrum for its next
    tile.  S = 2 P - 1: the last pair of every channel has no partner; tiles straddle channel boundaries for N < 4096 and the last one
    is partial; L = 2 S - 1 leaves the last segment one output.  Every row against fp64."""
    M, C, K = N - 1, 3, 3
    F = 4096 // N
    P = 10240 * F + 1
    L = 2 * (2 * P - 1) - 1
    tiles = frm.tiles(L, C, N, M)
    assert frm.Pairs(L, N, M, mode == "correlate").pairs() == P
    assert 2 * GRID_CAP < tiles < 3 * GRID_CAP and _group_plan(tiles, K) == (3, 1)
    assert F == 1 or (P % F and C * P % F)
    rng = np.random.default_rng(12288 + N + (mode == "correlate"))
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    got = _run(sm, fr, x, h, N, mode)
    _check_rows(got, _reference(x, h, mode == "correlate"), f"grid-stride N={N} {mode}", x, h)


# ---- spectra ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_prepared_spectra(sm, fr, N):
    """smfft_fir_real_prepare = fft(pad(g)) / N of the real taps within the per-FFT tolerances; a launch with NumPy-prepared spectra and
    a launch with the spectra smfft_fir_prepare makes of the taps cast to complex64 each pass the row check"""
    rng = np.random.default_rng(3 * N)
    K = 7
    for mode in MODES:
        for M in (1, 17, N // 4 + 1, N - 1):
            h = _rand(rng, (K, M))
            got = _prepared(sm, fr, h, N, mode)
            want = frm.spectra(h, N, mode == "correlate")
            for k in range(K):
                d = got[k] - want[k]
                l2 = np.linalg.norm(d) / np.linalg.norm(want[k])
                mx = np.max(np.abs(d)) / np.max(np.abs(want[k]))
                assert l2 <= REL_L2_TOL and mx <= MAX_ABS_TOL, (mode, M, k, l2, mx)
            hc = h.astype(np.complex64)
            dh, dspec = sm.DeviceBuffer.from_host(hc), sm.DeviceBuffer(K * N * 8)
            sm.fir_prepare(dh.ptr, dspec.ptr, M, K, N, mode)
            assert sm.lib.smfft_synchronize() == 0
            complex_banks = dspec.to_host(np.complex64, (K, N))
            dh.free()
            dspec.free()
            x = _rand(rng, (2, 3 * (N - M + 1) + 5))
            want_y = _reference(x, h, mode == "correlate")
            _check_rows(_run(sm, fr, x, h, N, mode), want_y, f"own spectra N={N} {mode} M={M}", x, h)
            _check_rows(_run(sm, fr, x, h, N, mode, spectra=want.astype(np.complex64)), want_y, f"NumPy spectra N={N} {mode} M={M}", x, h)
            _check_rows(_run(sm, fr, x, h, N, mode, spectra=complex_banks), want_y, f"smfft_fir_prepare's spectra N={N} {mode} M={M}", x, h)


# ---- entry forms -----------------------------------------------------------------------------------------------------------------
def test_caller_stream(sm, fr):
    """prepare and launch on a stream from hipStreamCreate, then hipStreamSynchronize"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    rng = np.random.default_rng(11)
    N, M, C, K, L = 1024, 257, 2, 9, 50000
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    for mode in MODES:
        dx, dh = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(h)
        dspec, dout = sm.DeviceBuffer(K * N * 8), sm.DeviceBuffer(C * K * L * 4)
        assert sm.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes) == 0
        assert sm.lib.smfft_synchronize() == 0
        fr.prepare(dh.ptr, dspec.ptr, M, K, N, mode, stream=stream.value)
        fr.launch(dx.ptr, L, C, dspec.ptr, K, M, N, dout.ptr, mode, stream=stream.value)
        assert hip.hipStreamSynchronize(stream) == 0
        _check_rows(dout.to_host(np.float32, (C, K, L)), _reference(x, h, mode == "correlate"), f"stream {mode}", x, h)
        for b in (dx, dh, dspec, dout):
            b.free()
    assert hip.hipStreamDestroy(stream) == 0


def test_benchmark_form_adds_to_the_timer(sm, fr):
    rng = np.random.default_rng(12)
    N, M, K, L = 512, 100, 3, 20000
    x, h = _rand(rng, (1, L)), _rand(rng, (K, M))
    dx, dspec = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(_prepared(sm, fr, h, N, "convolve"))
    dout = sm.DeviceBuffer(K * L * 4)
    assert sm.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes) == 0
    t = ctypes.c_double(1.0)
    assert fr.lib().smfft_fir_real_benchmark(dx.ptr, L, 1, dspec.ptr, K, M, N, 0, dout.ptr, ctypes.byref(t)) == 0
    assert t.value > 1.0
    _check_rows(dout.to_host(np.float32, (1, K, L)), _reference(x, h, False), "benchmark form", x, h)
    rc, ms = fr.benchmark(dx.ptr, L, 1, dspec.ptr, K, M, N, dout.ptr)
    assert rc == 0 and ms > 0.0
    for b in (dx, dspec, dout):
        b.free()


def test_host_convenience(sm, fr):
    """fir(): 1-D and (C, L) inputs, float64 input, the default transform length, the (C, K, L) float32 result"""
    rng = np.random.default_rng(7)
    x = rng.standard_normal(5000)
    h = rng.standard_normal(65)
    x32, h32 = x.astype(np.float32), h.astype(np.float32)
    for mode in MODES:
        got = fr.fir(x, h, mode)
        assert got.shape == (1, 1, 5000) and got.dtype == np.float32
        _check_rows(got, _reference(x32[None], h32[None], mode == "correlate"), f"fir() {mode}", x32[None], h32[None])
    x2, h2 = _rand(rng, (2, 3000)), _rand(rng, (3, 33))
    got = fr.fir(x2, h2, fft_size=1024)
    assert got.shape == (2, 3, 3000) and got.dtype == np.float32
    _check_rows(got, _reference(x2, h2, False), "fir() (C, L)", x2, h2)


# ---- 64-bit offsets ----------------------------------------------------------------------------------------------------------------
def test_output_offsets_beyond_two_to_the_31(sm, fr):
    """C = 1, K = 64, L = 2^25 + 1000: 2^31 + 64000 output floats (8 GiB); sampled windows of the last two filter rows against
    np.convolve / np.correlate on the matching input slice.  Row K - 1 crosses element 2^31 at n = 2^31 - (K - 1) L: one window
    straddles it, the last ones lie beyond it."""
    N, M, K, L = 1024, 257, 64, (1 << 25) + 1000
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, L), dtype=np.float32)
    h = _rand(rng, (K, M))
    W = 3000
    cross = (1 << 31) - (K - 1) * L
    starts = [0, L // 2 + 17, cross - 700, L - 5 * N, L - W]
    assert all(0 <= n0 and n0 + W <= L for n0 in starts) and cross - 700 < cross < cross - 700 + W and (K - 1) * L + L - W >= 1 << 31
    dx, dout = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer(K * L * 4)
    try:
        for mode in MODES:
            corr = mode == "correlate"
            dspec = sm.DeviceBuffer.from_host(_prepared(sm, fr, h, N, mode))
            assert sm.lib.smfft_memset(dout.ptr, 0xFF, dout.nbytes) == 0
            fr.launch(dx.ptr, L, 1, dspec.ptr, K, M, N, dout.ptr, mode)
            assert sm.lib.smfft_synchronize() == 0
            dspec.free()
            for k in (K - 2, K - 1):
                hk = h[k].astype(np.float64)
                for n0 in starts:
                    got = np.empty(W, np.float32)
                    assert sm.lib.smfft_memcpy_d2h(got.ctypes.data, dout.ptr + (k * L + n0) * 4, W * 4) == 0
                    if corr:
                        seg = np.r_[x[0, n0:n0 + W + M - 1].astype(np.float64), np.zeros(max(0, n0 + W + M - 1 - L))]
                        want = np.correlate(seg, hk, "valid")
                    else:
                        lo = max(0, n0 - (M - 1))
                        seg = x[0, lo:n0 + W].astype(np.float64)
                        want = np.convolve(seg, hk)[n0 - lo:n0 - lo + W]
                    _check_rows(got[None, None], want[None, None], f"{mode} k={k} n0={n0}", seg[None], hk[None])
    finally:
        dx.free()
        dout.free()


# ---- probes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_probe_exact_scaling(sm, fr, N):
    """every channel scaled by a power of two of its own scales its outputs exactly: the channels do not mix, and nothing in the
    kernel depends on the magnitude of the data"""
    rng = np.random.default_rng(40 + N)
    M, C, K = N // 4 + 1, 3, 4
    L = 5 * (N - M + 1) - 3
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    exps = np.array([-9, 0, 14])
    scaled = np.ldexp(x, exps[:, None]).astype(np.float32)
    for mode in MODES:
        spectra = _prepared(sm, fr, h, N, mode)
        base = _run(sm, fr, x, h, N, mode, spectra=spectra)
        got = _run(sm, fr, scaled, h, N, mode, spectra=spectra)
        assert np.array_equal(_bits(got), _bits(np.ldexp(base, exps[:, None, None]).astype(np.float32))), (N, mode)


def _pairs_reading(pr, n):
    return [p for p in range(pr.pairs()) if pr.load_range(p)[0] <= n < pr.load_range(p)[1]]


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_probe_nan_sample(sm, fr, N, mode):
    """A NaN at one sample of channel 1 of 3 makes NaN exactly the outputs of the pairs whose load range contains it (the footprint of
    tools/fir_real_model.py), for every filter and in that channel only; every other output is bit-identical to the clean run.  S = 5
    segments: pairs (0, 1), (2, 3) and a lone segment 4.  The NaN sits in the overlap of two pairs; in the lone last segment; and in
    the second segment of pair 0 only, which poisons segment 0's outputs too (the pair is the scope) and none of pair 1's."""
    corr = mode == "correlate"
    rng = np.random.default_rng(50 + N + corr)
    M, C, K = N // 4 + 1, 3, 3
    V = N - M + 1
    L = 5 * V - 3
    pr = frm.Pairs(L, N, M, corr)
    assert pr.w.segments() == 5 and pr.pairs() == 3 and not pr.present(2, 1)
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    spectra = _prepared(sm, fr, h, N, mode)
    clean = _run(sm, fr, x, h, N, mode, spectra=spectra)
    overlap = 2 * V if corr else 2 * V - 1               # the look-ahead of segment 1 / the history of segment 2
    second = V + M - 1 if corr else V                    # read by segment 1, not by segment 0, not by pair 1
    assert _pairs_reading(pr, overlap) == [0, 1] and _pairs_reading(pr, L - 1) == [2] and _pairs_reading(pr, second) == [0]
    a0 = pr.load_start(0, 0)
    assert not (a0 <= second < a0 + N) and pr.load_start(0, 1) <= second < pr.load_start(0, 1) + N
    for n, hit_outputs in ((overlap, (0, 4 * V)), (L - 1, (4 * V, L)), (second, (0, 2 * V))):
        foot = frm.nan_footprint(L, N, M, corr, n)
        assert foot[hit_outputs[0]:hit_outputs[1]].all() and foot.sum() == hit_outputs[1] - hit_outputs[0]
        bad = x.copy()
        bad[1, n] = np.nan
        got = _run(sm, fr, bad, h, N, mode, spectra=spectra, finite=False)
        for k in range(K):
            assert np.array_equal(np.isnan(got[1, k]), foot), (N, mode, n, k)
            assert np.array_equal(_bits(got[1, k][~foot]), _bits(clean[1, k][~foot])), (N, mode, n, k)
        assert np.array_equal(_bits(got[[0, 2]]), _bits(clean[[0, 2]])), (N, mode, n)


@pytest.mark.parametrize("N", SIZES)
def test_probe_nan_tap(sm, fr, N):
    """a NaN tap of one filter reaches exactly that filter's spectrum and rows, in every channel; the others are bit-identical"""
    rng = np.random.default_rng(60 + N)
    M, C, K = 17, 2, 5
    L = 3 * (N - M + 1) + 5
    x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
    bad = h.copy()
    bad[3, 5] = np.nan
    for mode in MODES:
        spectra, bad_spectra = _prepared(sm, fr, h, N, mode), _prepared(sm, fr, bad, N, mode)
        others = [0, 1, 2, 4]
        assert np.isnan(bad_spectra[3]).all()            # every element, in a part at least: real taps keep some imaginary parts +0
        assert np.array_equal(bad_spectra[others].view(np.uint32), spectra[others].view(np.uint32))
        clean = _run(sm, fr, x, h, N, mode, spectra=spectra)
        got = _run(sm, fr, x, bad, N, mode, spectra=bad_spectra, finite=False)
        assert np.isnan(got[:, 3]).all(), (N, mode)
        assert np.array_equal(_bits(got[:, others]), _bits(clean[:, others])), (N, mode)


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
REGION_GUARD = 128 * 1024      # bytes of guard on each side of every payload
POISON = 0x7FE5A5A5            # quiet NaN with a recognisable payload: guards and the bytes a call must leave alone


class _Region:
    """One device allocation [guard | offset | payload | guard], all but the payload poisoned; `ptr` is the payload's address"""

    def __init__(self, sm, payload, offset):
        self.lo, self.n = REGION_GUARD + offset, len(payload)
        self.image = np.full(-(-(self.lo + self.n + REGION_GUARD) // 4), POISON, np.uint32).view(np.uint8)[:self.lo + self.n + REGION_GUARD].copy()
        self.image[self.lo:self.lo + self.n] = payload
        self.buf = sm.DeviceBuffer(len(self.image))
        assert sm.lib.smfft_memcpy_h2d(self.buf.ptr, self.image.ctypes.data, len(self.image)) == 0
        self.ptr = self.buf.ptr + self.lo

    def outside_unchanged(self, whole):
        now = self.buf.to_host(np.uint8, (len(self.image),))
        keep = np.ones(len(now), bool)
        if not whole:
            keep[self.lo:self.lo + self.n] = False
        idx = np.flatnonzero((now != self.image) & keep)
        assert not len(idx), f"{len(idx)} bytes changed, the first at payload offset {int(idx[0]) - self.lo}"
        return now[self.lo:self.lo + self.n].copy()


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_bounds(sm, fr, N, mode):
    """prepare and launch separately, every buffer a guarded allocation of its own whose payload ends where the NaN guard begins, at
    offset bases (signal and output at an odd float, taps at a float of their own, spectra at an odd float2): the guard in front of
    channel 0 is what a convolution's history would read, the one behind channel C - 1 what a correlation's look-ahead -- or a
    partner that is not there -- would read; both must come in as zeros, never as NaN.  Nothing outside spectra[0, K N) and
    out[0, C K L) changes, and the result does not depend on the placement."""
    corr = 1 if mode == "correlate" else 0
    rng = np.random.default_rng(70 + N + corr)
    for M in (1, N // 4 + 1, N - 1):
        V = N - M + 1
        for L in (max(1, M - 1), V, 3 * V + V // 3 + 1):
            for C, K in ((1, 1), (3, 5)):
                x, h = _rand(rng, (C, L)), _rand(rng, (K, M))
                what = f"N={N} {mode} M={M} L={L} C={C} K={K}"
                sig, taps = _Region(sm, x.view(np.uint8).reshape(-1), 4), _Region(sm, h.view(np.uint8).reshape(-1), 12)
                spec = _Region(sm, np.full(K * N * 8, 0xFF, np.uint8), 8)
                out = _Region(sm, np.full(C * K * L * 4, 0xFF, np.uint8), 20)
                try:
                    assert fr.lib().smfft_fir_real_prepare(taps.ptr, M, K, N, corr, spec.ptr, None) == 0
                    assert sm.lib.smfft_synchronize() == 0
                    spectra = spec.outside_unchanged(False).view(np.complex64).reshape(K, N)
                    for r in (sig, taps, out):
                        r.outside_unchanged(True)
                    assert np.array_equal(spectra.view(np.uint32), _prepared(sm, fr, h, N, mode).view(np.uint32)), f"{what}: spectra depend on placement"
                    spec.image[spec.lo:spec.lo + spec.n] = spectra.view(np.uint8).reshape(-1)
                    assert fr.lib().smfft_fir_real_launch(sig.ptr, L, C, spec.ptr, K, M, N, corr, out.ptr, None) == 0
                    assert sm.lib.smfft_synchronize() == 0
                    got = out.outside_unchanged(False).view(np.float32).reshape(C, K, L)
                    for r in (sig, taps, spec):
                        r.outside_unchanged(True)
                finally:
                    for r in (sig, taps, spec, out):
                        r.buf.free()
                assert np.all(np.isfinite(got)), f"{what}: a guard was read, or an output left unwritten"
                _check_rows(got, _reference(x, h, bool(corr)), what, x, h)
                assert np.array_equal(_bits(got), _bits(fr.fir(x, h, mode, fft_size=N))), f"{what}: result depends on placement"
