"""Measures the figures of tests/accuracy_ratchet.json on the GPU: per case of tests/probe_cases.py, the DFT-matrix probe's largest
per-element error and its rms relL2, and the zero-mean Gaussian batch's rms relL2 -- with the functions tests/test_probes_gpu.py
(library cases) and tests/test_device_probes_gpu.py (HEADER_CASES) check them with.  Rerun after a deliberate change of a kernel's
arithmetic (or of the compiler), and commit the table it writes.
    python tools/accuracy_ratchet.py [--header] [out.json]          (default: tests/accuracy_ratchet.json)
    python tools/accuracy_ratchet.py --pfb [out.json]               (default: tests/pfb_accuracy_ratchet.json)
--header measures only the header's cases and merges them into the table that is there (the library's entries stay as they are);
without it the library's cases are measured and the header's entries of the table are kept.
--pfb measures the table of its own that the two polyphase filter banks have: per case of tests/pfb_probe_cases.py, the tap-matrix
probe's largest per-element error and its rms, with the function tests/test_pfb_probes_gpu.py checks them with."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import smfft_amd  # noqa: E402
from tests import probe_cases as pc  # noqa: E402
from tests import test_device_probes_gpu as hp  # noqa: E402
from tests import test_probes_gpu as tp  # noqa: E402


def pfb_main(args):
    from tests import pfb_probe_cases as ppc
    from tests import test_pfb_probes_gpu as pp
    out = args[0] if args else pp.RATCHET
    smfft_amd.FFT_init()
    table = {}
    for case in ppc.CASES:
        probe_max, probe_rms = pp.probe_errors(smfft_amd, case)
        table[case.id] = {"probe_max": float(f"{probe_max:.4g}"), "probe_rms": float(f"{probe_rms:.4g}")}
        print(f"{case.id:36s} probe max {probe_max:.3e} (ceiling {case.ceiling:.2e})  rms {probe_rms:.3e}", flush=True)
    with open(out, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print("wrote", out)


def main():
    args = sys.argv[1:]
    if "--pfb" in args:
        return pfb_main([a for a in args if a != "--pfb"])
    header = "--header" in args
    args = [a for a in args if a != "--header"]
    out = args[0] if args else tp.RATCHET
    smfft_amd.FFT_init()
    with open(tp.RATCHET) as f:
        old = json.load(f)
    header_ids = {c.id for c in pc.HEADER_CASES}
    if header:
        table = {k: v for k, v in old.items() if k not in header_ids}
        cases, mod = pc.HEADER_CASES, hp
    else:
        table = {}
        cases, mod = pc.CASES, tp
    for case in cases:
        probe_max, probe_rms = mod.probe_errors(smfft_amd, case)
        gauss = mod.gauss_error(smfft_amd, case)
        table[case.id] = {"gauss_rel_l2": float(f"{gauss:.4g}"), "probe_max": float(f"{probe_max:.4g}"), "probe_rms": float(f"{probe_rms:.4g}")}
        ceiling = pc.probe_ceiling(case.length if header else case.n, case.k)
        print(f"{case.id:48s} gauss {gauss:.3e}  probe max {probe_max:.3e} (ceiling {ceiling:.2e})  rms {probe_rms:.3e}", flush=True)
    if not header:
        table.update({k: v for k, v in old.items() if k in header_ids})
    with open(out, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
