"""Measures the figures of tests/accuracy_ratchet.json on the GPU: per case of tests/probe_cases.py, the DFT-matrix probe's largest
per-element error and its rms relL2, and the zero-mean Gaussian batch's rms relL2 -- with the functions tests/test_probes_gpu.py
checks them with.  Rerun after a deliberate change of a kernel's arithmetic (or of the compiler), and commit the table it writes.
    python tools/accuracy_ratchet.py [out.json]          (default: tests/accuracy_ratchet.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import smfft_amd  # noqa: E402
from tests import probe_cases as pc  # noqa: E402
from tests import test_probes_gpu as tp  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else tp.RATCHET
    smfft_amd.FFT_init()
    table = {}
    for case in pc.CASES:
        probe_max, probe_rms = tp.probe_errors(smfft_amd, case)
        gauss = tp.gauss_error(smfft_amd, case)
        table[case.id] = {"gauss_rel_l2": float(f"{gauss:.4g}"), "probe_max": float(f"{probe_max:.4g}"), "probe_rms": float(f"{probe_rms:.4g}")}
        print(f"{case.id:40s} gauss {gauss:.3e}  probe max {probe_max:.3e} (ceiling {pc.probe_ceiling(case.n, case.k):.2e})  rms {probe_rms:.3e}", flush=True)
    with open(out, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
