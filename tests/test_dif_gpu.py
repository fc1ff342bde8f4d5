"""The decimation-in-frequency transform on an MI355X: the library's SMFFT_DIF_external (c2c_dif / smfft_ct_dif_*), the device functions
do_SMFFT_CT_DIF / do_SMFFT_CT_DIF_registers in user kernels of the reference's shape (examples/dif_convolution.hip), and the reorder-free
convolution chain DIF forward -> .* Hb -> no-reorder DIT inverse -- against numpy in fp64."""
import ctypes

import numpy as np
import pytest

from oracle.np_reference import assert_close_fp32, bitrev_indices, fft_errors

pytestmark = pytest.mark.gpu

SIZES = [32, 64, 128, 256, 512, 1024, 2048, 4096]
vp, ci = ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def sm():
    import smfft_amd
    smfft_amd.FFT_init()
    return smfft_amd


@pytest.fixture(scope="module")
def ex(sm):
    import os
    path = os.path.join(os.path.dirname(sm.LIB_PATH), "libsmfft_examples.so")
    if not os.path.exists(path):
        pytest.fail("libsmfft_examples.so is missing: it is built by smfft_amd/csrc/Makefile")
    lib = ctypes.CDLL(path)
    lib.smfft_example_dif_ct.argtypes = [vp, vp, ci, ci, ci, ci, vp]
    lib.smfft_example_reference_shape_convolve_dif.argtypes = [vp, vp, vp, ci, ci, vp]
    lib.smfft_example_reference_shape_convolve_1024_registers.argtypes = [vp, vp, vp, ci, vp]
    return lib


def _rand(rng, rows, n):
    return (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))).astype(np.complex64)


def _dif_ref(x, inverse):
    x = np.asarray(x, dtype=np.complex128)
    n = x.shape[-1]
    spec = np.fft.ifft(x, axis=-1) * n if inverse else np.fft.fft(x, axis=-1)
    return spec[..., bitrev_indices(n)]


def _circular(x, h):
    return np.fft.ifft(np.fft.fft(x.astype(np.complex128), axis=-1) * np.fft.fft(h.astype(np.complex128)), axis=-1)


# ------------------------------------------------------------------------------------------------ library transform
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("inverse", [0, 1])
def test_library_dif_is_the_bit_reversed_dft(sm, n, inverse):
    """c2c_dif = fft(x)[bitrev] for one transform, a batch that leaves the last block partly empty, and a few thousand; nothing of the
    NaN-filled output buffer survives"""
    rng = np.random.default_rng(100 * n + inverse)
    for nffts in (1, 37, 3001 if n <= 1024 else 1001):
        x = _rand(rng, nffts, n)
        got = sm.c2c_dif(x, inverse=bool(inverse))
        assert np.all(np.isfinite(got.view(np.float32))), (n, nffts)
        assert_close_fp32(got, _dif_ref(x, inverse), f"c2c_dif N={n} inverse={inverse} nFFTs={nffts}")


@pytest.mark.parametrize("n", SIZES)
def test_library_round_trip_through_the_no_reorder_transform(sm, n):
    """the no-reorder transform of the other direction inverts the DIF transform: c2c(c2c_dif(x), inverse, reorder=False) = N x, and the
    same with the directions swapped"""
    x = _rand(np.random.default_rng(n), 29, n)
    for inverse in (0, 1):
        y = sm.c2c(sm.c2c_dif(x, inverse=bool(inverse)), inverse=not inverse, reorder=False)
        assert_close_fp32(y, n * x.astype(np.complex128), f"round trip N={n} DIF inverse={inverse}")


@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_library_convolution_without_reordering(sm, n):
    rng = np.random.default_rng(7 * n)
    x = _rand(rng, 33, n)
    h = np.zeros((1, n), np.complex64)
    h[0, :7] = [0.4, 0.3, 0.2, 0.1, -0.05j, 0.02, 0.01 + 0.01j]
    prod = sm.c2c_dif(x) * sm.c2c_dif(h)
    y = sm.c2c(prod, inverse=True, reorder=False) / n
    l2, mx = fft_errors(y, _circular(x, h[0]))
    assert l2 < 1e-6 and mx < 2e-6, (n, l2, mx)


def test_library_dif_config2_batch(sm):
    """N = 1024, 524 288 transforms (4 GiB in, 4 GiB out) on a smfft_malloc_pair pair: seeded rows spread over the batch -- the last ones
    more than 2^31 bytes into either buffer -- are the bit-reversed DFTs of their inputs"""
    n, nffts = 1024, 524288
    nbytes = n * nffts * 8
    pa, pb = ctypes.c_void_p(), ctypes.c_void_p()
    assert sm.lib.smfft_malloc_pair(nbytes, ctypes.byref(pa), ctypes.byref(pb)) == 0
    try:
        assert sm.lib.smfft_memset(pa.value, 0, nbytes) == 0
        rng = np.random.default_rng(2024)
        rows = np.unique(np.concatenate([rng.integers(0, nffts, 24), [0, nffts // 2, (1 << 31) // (n * 8) + 5, nffts - 2, nffts - 1]]))
        xs = _rand(rng, len(rows), n)
        for r, x in zip(rows, xs):
            assert sm.lib.smfft_memcpy_h2d(pa.value + int(r) * n * 8, x.ctypes.data, x.nbytes) == 0
        assert sm.lib.smfft_memset(pb.value, 0xFF, nbytes) == 0
        sm.launch_dif(pa.value, pb.value, n, nffts)
        assert sm.lib.smfft_synchronize() == 0
        got = np.empty((len(rows), n), np.complex64)
        for i, r in enumerate(rows):
            assert sm.lib.smfft_memcpy_d2h(got[i].ctypes.data, pb.value + int(r) * n * 8, n * 8) == 0
        assert_close_fp32(got, _dif_ref(xs, 0), "config-2 batch, sampled rows")
        zero_row = np.empty(n, np.complex64)            # a row nobody wrote: DIF of zeros is zeros (the NaN fill is gone everywhere)
        other = int(np.setdiff1d(np.arange(1, 100), rows)[0])
        sm.lib.smfft_memcpy_d2h(zero_row.ctypes.data, pb.value + other * n * 8, n * 8)
        assert np.all(zero_row == 0)
    finally:
        sm.lib.smfft_free_pair(pa.value)


# ------------------------------------------------------------------------------------------------ device functions (examples/)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("inverse", [0, 1])
def test_device_function_dif(sm, ex, n, inverse):
    """smfft_example_dif_ct: which = 0 fill / do_SMFFT_CT_DIF / drain, 1 do_SMFFT_CT_DIF_registers (N >= 256), 2 the _wave64 classes
    (N <= 128), whole blocks of the reference's shape"""
    rng = np.random.default_rng(300 * n + inverse)
    for which in ((0, 1) if n >= 256 else (0, 2)):
        per_block = (256 if which == 2 else max(n, 128)) // n
        nffts = 13 * per_block
        x = _rand(rng, nffts, n)
        dx, dy = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer(x.nbytes)
        sm.lib.smfft_memset(dy.ptr, 0xFF, x.nbytes)
        assert ex.smfft_example_dif_ct(dx.ptr, dy.ptr, n, nffts, inverse, which, None) == 0
        assert sm.lib.smfft_synchronize() == 0
        got = dy.to_host(np.complex64, x.shape)
        assert_close_fp32(got, _dif_ref(x, inverse), f"device DIF N={n} inverse={inverse} which={which}")
        dx.free()
        dy.free()


def _convolve_dif(sm, ex, x, hb, n):
    dx, dh, dy = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(hb), sm.DeviceBuffer(x.nbytes)
    sm.lib.smfft_memset(dy.ptr, 0xFF, x.nbytes)
    assert ex.smfft_example_reference_shape_convolve_dif(dx.ptr, dh.ptr, dy.ptr, n, x.shape[0], None) == 0
    assert sm.lib.smfft_synchronize() == 0
    return dy.to_host(np.complex64, x.shape)


@pytest.mark.parametrize("n", [256, 512, 1024, 2048, 4096])
def test_register_chain_dif_then_no_reorder_dit(sm, ex, n):
    """do_SMFFT_CT_DIF_registers' output fed unchanged to do_SMFFT_CT_DIT_registers<FFT_<N>_inverse_noreorder> is N x: the chain kernel with a
    filter of ones (its 1/N is exact) returns x -- the no-reorder register input of the DIT function at every length"""
    x = _rand(np.random.default_rng(n + 1), 21, n)
    got = _convolve_dif(sm, ex, x, np.ones(n, np.complex64), n)
    assert_close_fp32(got, x.astype(np.complex128), f"DIF -> DIT no-reorder chain N={n}")


@pytest.mark.parametrize("n", [256, 512, 1024, 2048, 4096])
def test_contract_convolution_dif(sm, ex, n):
    rng = np.random.default_rng(5 * n)
    x = _rand(rng, 3 * (4096 // n) + 1, n)
    h = np.zeros((1, n), np.complex64)
    h[0, :5] = [0.4, 0.3, 0.2, 0.1, -0.05j]
    hb = sm.c2c_dif(h)[0]                                   # the filter through the same DIF transform, once
    got = _convolve_dif(sm, ex, x, hb, n)
    l2, mx = fft_errors(got, _circular(x, h[0]))
    assert l2 < 1e-6 and mx < 2e-6, (n, l2, mx)
    if n == 1024:                                           # and the natural-order register chain of reference_shape_kernel.hip agrees
        H = np.fft.fft(h[0].astype(np.complex128)).astype(np.complex64)
        dx, dH, dy = sm.DeviceBuffer.from_host(x), sm.DeviceBuffer.from_host(H), sm.DeviceBuffer(x.nbytes)
        assert ex.smfft_example_reference_shape_convolve_1024_registers(dx.ptr, dH.ptr, dy.ptr, x.shape[0], None) == 0
        assert sm.lib.smfft_synchronize() == 0
        natural = dy.to_host(np.complex64, x.shape)
        l2, mx = fft_errors(got, natural.astype(np.complex128))
        assert l2 < 1e-6 and mx < 2e-6, (l2, mx)
