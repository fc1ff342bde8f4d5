"""The twiddle table every kernel reads (include/smfft/smfft_twiddles.inc) is what tools/gen_twiddles.py generates, and every entry
is W_4096^m = (cos, -sin)(2 pi m / 4096) correctly rounded to fp32: within 0.5 ulp of the fp64 value, with the quarter-turn entries
exact.  CPU only."""
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_twiddles  # noqa: E402

TABLE = os.path.join(ROOT, "include", "smfft", "smfft_twiddles.inc")


def _entries():
    pairs = re.findall(r"\{(\S+)f, (\S+)f\}", open(TABLE).read())
    return np.array([[float.fromhex(a), float.fromhex(b)] for a, b in pairs])


def _half_ulp_fp32(v):
    """half the fp32 ulp in the binade of the exact value v (v != 0, normal)"""
    return 2.0 ** (math.frexp(abs(v))[1] - 1 - 23) / 2


def test_committed_table_is_the_generators_output():
    assert os.path.abspath(gen_twiddles.PATH) == os.path.abspath(TABLE)
    assert open(TABLE).read() == gen_twiddles.table_text(), "include/smfft/smfft_twiddles.inc differs from tools/gen_twiddles.py's output"


def test_every_entry_is_the_fp32_rounding_of_the_twiddle():
    t = _entries()
    assert t.shape == (4096, 2)
    assert np.array_equal(t, t.astype(np.float32).astype(np.float64)), "an entry is not an fp32 value"
    ang = 2 * np.pi * np.arange(4096) / 4096
    exact = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
    for m in range(4096):
        for j in range(2):
            v = exact[m, j]
            if abs(v) < 1e-12:                       # the quarter turns: fp64 leaves ~1e-16 where the value is 0
                assert t[m, j] == 0.0, (m, j, t[m, j])
                continue
            assert abs(t[m, j] - v) <= _half_ulp_fp32(v), (m, j, t[m, j], v)


def test_quarter_turns_are_exact():
    t = _entries()
    want = {0: (1.0, 0.0), 1024: (0.0, -1.0), 2048: (-1.0, 0.0), 3072: (0.0, 1.0)}
    for m, (c, s) in want.items():
        assert (t[m, 0], t[m, 1]) == (c, s), (m, t[m])
