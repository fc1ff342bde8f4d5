"""tests/accuracy_ratchet.json, the accuracy figures tests/test_probes_gpu.py and tests/test_device_probes_gpu.py hold the kernels and
the header's device functions to, has exactly one entry per case those modules run (tests/probe_cases.py, CASES and HEADER_CASES),
and every entry is within the fixed bounds: the Gaussian relL2 within 5e-7 sqrt(k), the probe's per-element maximum and rms within the
twiddle-chain ceiling k * 3 * (log2 N + 2) * 2^-24.  CPU only."""
import json
import os

from tests import probe_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"gauss_rel_l2", "probe_max", "probe_rms"}


def _table():
    with open(os.path.join(ROOT, "tests", "accuracy_ratchet.json")) as f:
        return json.load(f)


def test_ratchet_keys_are_the_gpu_cases():
    table = _table()
    ids = {c.id for c in pc.CASES} | {c.id for c in pc.HEADER_CASES}
    assert len(ids) == len(pc.CASES) + len(pc.HEADER_CASES)
    assert set(table) == ids, (sorted(ids - set(table))[:8], sorted(set(table) - ids)[:8])
    for cid, entry in table.items():
        assert set(entry) == KEYS, cid


def test_ratchet_entries_are_within_the_fixed_bounds():
    table = _table()
    for c in pc.CASES:
        e = table[c.id]
        assert 0 < e["gauss_rel_l2"] <= pc.gauss_bound(c.k), (c.id, e)
        assert 0 <= e["probe_rms"] <= e["probe_max"] <= pc.probe_ceiling(c.n, c.k), (c.id, e)


def test_header_ratchet_entries_are_within_the_fixed_bounds():
    table = _table()
    for c in pc.HEADER_CASES:
        e = table[c.id]
        assert 0 < e["gauss_rel_l2"] <= pc.gauss_bound(c.k), (c.id, e)
        assert 0 <= e["probe_rms"] <= e["probe_max"] <= pc.probe_ceiling(c.length, c.k), (c.id, e)
