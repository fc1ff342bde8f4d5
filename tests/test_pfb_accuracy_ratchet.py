"""tests/pfb_accuracy_ratchet.json, the figures tests/test_pfb_probes_gpu.py holds the tap-matrix probe of the two polyphase filter banks
to, has exactly one entry per case of tests/pfb_probe_cases.py, and every entry is within the case's fixed ceiling; the cases are the
ones the probe's design asks for (every kernel, every position or every thread and register index, no case above 2^25 output elements),
and the closed form the probe compares with is the fp64 models' output.  CPU only."""
import json
import os
import sys

import numpy as np
import pytest

from tests import pfb_inventory as pinv
from tests import pfb_probe_cases as ppc
from tests import probe_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pfb_model as pm  # noqa: E402
import pfb_real_model as prm  # noqa: E402

KEYS = {"probe_max", "probe_rms"}


def _table():
    with open(os.path.join(ROOT, "tests", "pfb_accuracy_ratchet.json")) as f:
        return json.load(f)


def test_ratchet_keys_are_the_probe_cases():
    table = _table()
    ids = {c.id for c in ppc.CASES}
    assert set(table) == ids, (sorted(ids - set(table))[:8], sorted(set(table) - ids)[:8])
    for cid, entry in table.items():
        assert set(entry) == KEYS, cid


def test_ratchet_entries_are_within_the_fixed_ceilings():
    table = _table()
    for c in ppc.CASES:
        e = table[c.id]
        assert 0 < e["probe_rms"] <= e["probe_max"] <= c.ceiling, (c.id, e, c.ceiling)


def test_ceilings_are_the_transform_probes():
    for c in ppc.CASES:
        base = pc.probe_ceiling(2 * c.n if c.real else c.n, 1)
        assert c.ceiling == (2 * base + 2.0 ** -22 if c.power else base), c.id


def test_cases_run_every_kernel_and_cover_every_index():
    kernels = set()
    for c in ppc.CASES:
        kernels.add(f"smfft::{c.bank}::{c.bank}_kernel<{c.n}, {c.power}>")
        pos = c.positions()
        assert len(set(pos)) == len(pos) and 0 <= min(pos) and max(pos) < c.chunk, c.id
        assert c.frames * c.n <= ppc.MAX_OUTPUT_ELEMENTS, c.id
        t = c.n // 16
        pairs = [m // 2 if c.real else m for m in pos]           # the float2 a thread loads: n = u + T q
        assert {n % t for n in pairs} == set(range(t)) and {n // t for n in pairs} == set(range(16)), c.id
        if c.real:
            assert {m % 2 for m in pos} == {0, 1}, c.id
        if c.tag == "all":
            assert pos == list(range(c.chunk)) and (c.n == 256 or not c.power), c.id
        else:
            assert len(pos) == 256 and c.p == 32, c.id
    assert kernels == set(pinv.KERNELS) | set(pinv.REAL_KERNELS) and len(kernels) == 20
    for bank in ("pfb", "pfb_real"):
        for n in ppc.SIZES:
            mine = [c for c in ppc.CASES if c.bank == bank and c.n == n]
            assert sum(c.tag == "all" and not c.power and c.p == ppc.ALL_TAPS[bank][n] for c in mine) == 1
            assert sorted(c.power for c in mine if c.tag == "sub") == [0, 1]
        small = {(c.p, c.tag, c.power) for c in ppc.CASES if c.bank == bank and c.n == 256}
        assert {(p, "all", power) for p in (1, 32) for power in (0, 1)} <= small


@pytest.mark.parametrize("case", [ppc.Case("pfb", 256, 3, "all", 0), ppc.Case("pfb_real", 256, 3, "all", 0), ppc.Case("pfb", 256, 1, "all", 0),
                                  ppc.Case("pfb_real", 256, 1, "all", 0), ppc.Case("pfb", 512, 32, "sub", 0), ppc.Case("pfb_real", 512, 32, "sub", 0)],
                         ids=lambda c: c.id)
def test_closed_form_is_the_models_output(case):
    """every frame sees one nonzero sample, at the branch and position the closed form says, and the model's spectrum is the closed form"""
    x, h, pos = ppc.inputs(case)
    assert case in ppc.CASES and np.all((np.abs(h) >= 0.5) & (np.abs(h) <= 1)) and len(set(h.tolist())) > 0.99 * h.size
    W, P, F = case.chunk, case.p, case.frames
    chunks = x.reshape(-1, W)
    assert chunks.shape[0] == F + P - 1 and np.count_nonzero(x) == len(pos)
    f = np.arange(F)
    n, hf = ppc.frame_taps(case, h, pos, f)
    p = P - 1 - f % P
    assert np.all(chunks[f + p, n] == 1) and all(np.count_nonzero(chunks[g:g + P]) == 1 for g in f)
    assert np.array_equal(hf, h.astype(np.float64)[p * W + n])
    ref = (prm.pfb_real if case.real else pm.pfb)(x, h, case.n)[0]
    want = ppc.expected(case, h, pos, f)
    assert ref.shape == want.shape == (F, case.n + 1 if case.real else case.n)
    assert np.max(np.abs(ref - want)) <= 1e-14
    if case.real:
        assert np.max(np.abs(want[:, 0] - hf)) <= 1e-15 and np.max(np.abs(want[:, -1] - hf * (1 - 2 * (n & 1)))) <= 1e-14
