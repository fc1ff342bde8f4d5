"""The polyphase filter bank channelizer for real streams (smfft_amd/csrc/smfft_pfb_real.hip, include/smfft_pfb_real.h) on the CPU: the
fp64 model's two forms of the definition agree, with one tap of ones it is np.fft.rfft, and it equals channels 0 ... N of the complex
bank's model at 2N channels; the gfx950 code keeps the library's rules (no scratch, no v_sin / v_cos, no packed f32, the VGPRs of three
workgroups per compute unit, the sixteen signal loads of a tap together); the C ABI declares, exports and validates without a device; every shipped kernel is in tests/pfb_inventory.py with its tests.
No GPU code is run (hipcc cross-compiles gfx950)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pfb_model as pm  # noqa: E402
import pfb_real_model as prm  # noqa: E402

from tests import addon_checks as ac  # noqa: E402
from tests import pfb_inventory as pinv  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
SIZES = (256, 512, 1024, 2048, 4096)


# ------------------------------------------------------------------------------------------------ the model
def test_models_two_forms_agree():
    rng = np.random.default_rng(0)
    N = 256
    for P, C, L in ((1, 1, 512), (2, 2, 5 * 512 + 18), (4, 1, 7 * 512 + 510), (32, 1, 34 * 512 + 2)):
        x, h = rng.standard_normal((C, L)), rng.standard_normal(P * 2 * N)
        a, b = prm.pfb_real(x, h, N), prm.pfb_real_direct(x, h, N)
        assert a.shape == (C, L // (2 * N) - P + 1, N + 1)
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), (P, C, L)
        # packing and power: element 0 holds DC and Nyquist / the DC power, the others are the spectrum's
        p, w = prm.pack(a), prm.power(a)
        assert p.shape == w.shape == a.shape[:-1] + (N,)
        assert np.array_equal(p[..., 1:], a[..., 1:N]) and np.array_equal(p[..., 0].real, a[..., 0].real)
        assert np.array_equal(p[..., 0].imag, a[..., N].real)
        assert np.allclose(w, np.abs(a[..., :N]) ** 2, rtol=1e-12)
        assert np.max(np.abs(a[..., 0].imag)) <= 1e-9 * np.max(np.abs(a)) and np.max(np.abs(a[..., N].imag)) <= 1e-9 * np.max(np.abs(a))


@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_model_with_one_tap_of_ones_is_the_plain_rfft(N):
    rng = np.random.default_rng(N)
    x = rng.standard_normal((2, 5 * 2 * N + 12))
    want = np.fft.rfft(x[:, :5 * 2 * N].reshape(2, 5, 2 * N), axis=-1)
    got = prm.pfb_real(x, np.ones(2 * N), N)
    assert got.shape == want.shape == (2, 5, N + 1)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("N", SIZES)
def test_model_is_the_lower_half_of_the_complex_banks_model(N):
    """channels 0 ... N of pfb_model.pfb(x + 0j, h, 2N): the new definition is the shipped one on a real signal"""
    rng = np.random.default_rng(7 * N)
    for P, C, tail in ((1, 1, 0), (3, 2, 2 * N - 2), (8, 1, 6)):
        L = (P + 2) * 2 * N + tail
        x, h = rng.standard_normal((C, L)), rng.standard_normal(P * 2 * N)
        want = pm.pfb(x + 0j, h, 2 * N)
        got = prm.pfb_real(x, h, N)
        assert got.shape == (C, 3, N + 1) and want.shape == (C, 3, 2 * N)
        assert prm.frames(L, N, P) == pm.frames(L, 2 * N, P) == pm.Plan(L // 2, N, P, C).frames() == 3
        assert np.max(np.abs(got - want[..., :N + 1])) <= 1e-12 * np.max(np.abs(want)), (N, P)
        assert np.allclose(prm.scale(x, h, N), pm.scale(x, h, 2 * N), rtol=1e-13)


# ------------------------------------------------------------------------------------------------ gfx950 code
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return ac.addon_isa("smfft_pfb_real", "PFB_REAL", ac.PFB_SIZES, tmp_path_factory.mktemp("pfb_real_isa"))


def test_kernels_fit_three_workgroups_per_cu_without_scratch(isa):
    ac.check_pfb_kernel_rules(isa, "pfb_real_kernel")


def test_signal_loads_of_a_tap_are_issued_together(isa):
    """the signal loads are the kernel's only non-temporal loads; the coefficient pairs are plain 8-byte loads"""
    ac.check_pfb_signal_loads(isa, "pfb_real_kernel", signal=r"global_load_dwordx2 v\[\d+:\d+\], v\[\d+:\d+\], off( offset:-?\d+)? nt$",
                              tap=r"global_load_dwordx2 v\[\d+:\d+\], v\[\d+:\d+\], off( offset:-?\d+)?$",
                              arithmetic=r"(v_add|v_addc|v_lshl|v_lshlrev|v_mov|v_mad|v_ashr|v_and|v_or|s_add|s_addc|s_lshl|s_mov|s_nop|s_mul|s_waitcnt lgkmcnt|;)")


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def pr():
    from smfft_amd import pfb_real
    pfb_real.lib()
    return pfb_real


def test_header_declarations_equal_the_ctypes_signatures(pr):
    from smfft_amd import pfb
    ac.check_pfb_declarations(pr, "smfft_pfb_real", ("Out of scope", "oversampled", "complex prototypes", "synthesis", "Nyquist power", "NOT output", "N <= 128",
                                                     "N >= 8192", "EVEN"))
    # one for one the complex bank's functions, in arguments and results
    for name in ac.pfb_names("smfft_pfb_real"):
        assert pr.SIGS[name] == pfb.SIGS[name.replace("pfb_real", "pfb")], name
    assert pr.SIZES == SIZES
    # the complex bank's header points real input here
    assert "smfft_pfb_real.h" in open(os.path.join(ROOT, "include", "smfft_pfb.h")).read()


def test_library_exports_exactly_the_five_symbols(pr):
    ac.check_pfb_exports(pr, "smfft_pfb_real")


def test_unsupported_combinations_return_minus_one_without_a_device(pr):
    ac.check_pfb_rejections(pr, "smfft_pfb_real", samples=2, bad_lengths=[(-2, 1, 1024, 4), (-1, 1, 1024, 4),
                                                                          ((1 << 20) + 1, 1, 1024, 4), (8 * 2048 + 1, 2, 1024, 4), (1, 1, 256, 1), (3, 1, 1024, 4)])      # negative, odd
    with pytest.raises(ValueError):
        pr.frames(1000, 100, 4)
    with pytest.raises(ValueError):
        pr.frames(8 * 2048 + 1, 1024, 4)
    with pytest.raises(RuntimeError):
        pr.launch(None, 1 << 20, 1, None, 8192, 4, None)
    with pytest.raises(ValueError):
        pr.channelize(np.zeros(4096, np.float32), np.zeros(100, np.float32), 256)
    with pytest.raises(ValueError):
        pr.channelize(np.zeros(4096, np.complex64), np.zeros(512, np.float32), 256)
    assert pr.channelize(np.zeros((2, 1000), np.float32), np.zeros(1024, np.float32), 256).shape == (2, 0, 257)
    assert pr.channelize(np.zeros((2, 1000), np.float32), np.zeros(1024, np.float32), 256, packed=True).shape == (2, 0, 256)
    assert pr.channelize(np.zeros((2, 1000), np.float32), np.zeros(1024, np.float32), 256, power=True).shape == (2, 0, 256)


def test_every_pfb_real_kernel_is_in_the_inventory_with_its_tests(pr):
    """the rule of tests/test_kernel_inventory.py, without the "host" kind (tests/pfb_inventory.py says why)"""
    ac.check_inventory(pr.LIB_PATH, pinv.REAL_KERNELS, "smfft_pfb_real_", 10, kinds=("tests", "bounds", "probes"))


def test_frames_over_ragged_lengths_and_default_tile_run(pr):
    for N in SIZES:
        for P in (1, 4, 32):
            assert pr.default_tile_run(N, P) >= 1
            for L in (0, 2 * N - 2, 2 * P * N - 2, 2 * P * N, 2 * P * N + 2, (P + 9) * 2 * N + 2 * N - 2, (1 << 34) + 6):
                assert pr.frames(L, N, P) == max(L // (2 * N) - P + 1, 0) == prm.frames(L, N, P) == pm.frames(L // 2, N, P)


def test_prototype(pr):
    for N, P in ((256, 1), (256, 4), (1024, 8), (4096, 32), (512, 3)):
        h = pr.prototype(N, P)
        M = 2 * P * N
        assert h.dtype == np.float32 and h.shape == (M,)
        assert np.array_equal(h, h[::-1]), "symmetric to the bit"
        assert h[M // 2 - 1] == h[M // 2] == h.max()
        m = np.arange(M, dtype=np.float64)
        want = np.sinc((m - (M - 1) / 2) / (2 * N)) * (0.54 - 0.46 * np.cos(2 * np.pi * m / (M - 1)))
        assert np.array_equal(h, want.astype(np.float32)) or np.max(np.abs(h.astype(np.float64) - want)) <= 2.0 ** -24 * np.max(np.abs(want))
    assert np.array_equal(pr.prototype(256, 2, "rectangular"), np.sinc((np.arange(1024) - 511.5) / 512).astype(np.float32))
    with pytest.raises(ValueError):
        pr.prototype(256, 2, "kaiser")
    # unpack: the device's rows -> np.fft.rfft layout
    rows = (np.arange(12) + 1j * np.arange(12, 24)).reshape(3, 4).astype(np.complex64)
    un = pr.unpack(rows)
    assert un.shape == (3, 5) and np.array_equal(un[:, 1:4], rows[:, 1:]) and np.array_equal(un[:, 0], rows[:, 0].real) and np.array_equal(un[:, 4], rows[:, 0].imag)
