"""The integrated power spectra of the polyphase filter banks (smfft_pfb_spec_launch / smfft_pfb_real_spec_launch) in both accumulator
forms against the kernel they grew from, against the pipeline they replace and against a copy, in one process, timed round robin so that
drift of the box hits all alike (median and quartiles of --reps event-timed launches each, every function warmed up before the timed
window):
  spec      the shipped library (smfft_amd/libsmfft_pfb_spec.so or SMFFT_PFB_SPEC_LIB) and every other build given with --alt NAME=PATH
            -- the other accumulator form, the other load policy, built beside it:
                make -C smfft_amd/csrc PFB_SPEC_LIB=../../build_ab/libsmfft_pfb_spec_regs.so PFB_SPEC_OBJDIR=../../build_ab/pfb_spec_regs \\
                     PFB_SPEC_ACC_LDS=0 ../../build_ab/libsmfft_pfb_spec_regs.so          (PFB_SPEC_ACC_LDS=1: _lds; PFB_SPEC_NT_LOADS=1: _nt)
            all builds must give the same bits: the sum's order is the definition's in every one
  power     the same bank's power-mode launch on the same input (smfft_pfb_launch / smfft_pfb_real_launch, power = 1): the kernel
            without the sum, which writes 4 bytes per sample
  pipeline  that launch + torch's sum over the T frames of every spectrum: what a caller did before (its result differs from spec's in
            the order of the sum; the largest difference is printed)
  copy      a device copy of the input bytes (reads them and writes them once): the same-run bandwidth figure
Shapes: C = 1, 4 GiB of signal (2^29 complex samples, 2^30 real ones), P = 8, T = 64, N in {1024, 4096}, both banks.  The rates are
input bytes per second: what spec moves, and a lower bound of what the others move.
    python tools/ab_pfb_spec.py [--reps 30] [--alt regs=build_ab/libsmfft_pfb_spec_regs.so] [--small]"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import ab_pfb_common as ab  # noqa: E402

P, T = 8, 64


def main():
    ap = argparse.ArgumentParser()
    ab.add_arguments(ap, "libsmfft_pfb_spec.so")
    args = ap.parse_args()

    import torch

    from smfft_amd import pfb, pfb_real, pfb_spec

    ses = ab.Session(pfb_spec, None, args)
    sp, gen = ses.sp, ses.gen
    libs = {"shipped": pfb_spec.lib()}
    libs.update(ses.load(item) for item in args.alt)
    print(f"device: {torch.cuda.get_device_name(0)}, {ses.cus} compute units; {ses.reps} reps round robin; builds: {', '.join(libs)}", flush=True)

    def shape(N, real):
        bytes_in = (1 << 32) // (16 if args.small else 1)
        bank, prefix = (pfb_real, pfb_spec.PREFIXES[1]) if real else (pfb, pfb_spec.PREFIXES[0])
        L = bytes_in // (4 if real else 8)
        x = torch.randn(bytes_in // 4, dtype=torch.float32, device="cuda", generator=gen)
        h = torch.from_numpy(bank.prototype(N, P)).cuda()
        F, n = bank.frames(L, N, P), pfb_spec.spectra(L, N, P, T, real=real)
        tiles = -(-n // (4096 // N))
        what = f"{'real' if real else 'complex'} bank C=1 N={N} P={P} T={T}"
        print(f"--- {what}: {bytes_in / 2**30:.2f} GiB in, F = {F}, I = {n} spectra ({n * N * 4 / 2**20:.1f} MiB out), {tiles} tiles; "
              f"power mode writes {F * N * 4 / 2**30:.2f} GiB", flush=True)
        out = torch.empty((n, N), dtype=torch.float32, device="cuda")
        frames = torch.empty((F, N), dtype=torch.float32, device="cuda")
        summed = torch.empty((n, N), dtype=torch.float32, device="cuda")

        def spec(lib):
            launch = getattr(lib, prefix + "_launch")

            def run():
                rc = launch(x.data_ptr(), L, 1, h.data_ptr(), N, P, T, out.data_ptr(), sp)
                assert rc == 0, rc
            return run

        def power():
            bank.launch(x.data_ptr(), L, 1, h.data_ptr(), N, P, frames.data_ptr(), power=True, stream=sp)

        def pipeline():
            power()
            torch.sum(frames[:n * T].view(n, T, N), dim=1, out=summed)

        fns = {f"spec {name}": spec(lib) for name, lib in libs.items()}
        base = ab.compare_outputs(fns, out, lambda name: True)
        print("all builds: identical bits", flush=True)
        pipeline()
        torch.cuda.synchronize()
        print(f"max |pipeline - spec| / max |spec| = {((summed - base).abs().max() / base.abs().max()).item():.2e}", flush=True)
        del base
        pw, pl = "power mode, same input (no sum)", "pipeline: power mode + torch.sum over T"
        fns[pw], fns[pl] = power, pipeline
        fns[ab.COPY] = ses.copy_of(2 * bytes_in)

        def spread(name, q):
            lo, med, hi = q[name]
            return f"  spread (upper - lower quartile) / median = {(hi - lo) / med:.4f}"
        q = ab.report(ses.round_robin(fns), bytes_in, 44, True, spread)
        for name in libs:
            med = q[f"spec {name}"][1]
            print(f"RATIO  {what}: spec {name} / power mode = {med / q[pw][1]:.4f}, / pipeline = {med / q[pl][1]:.4f}, / copy = {med / q[ab.COPY][1]:.4f}", flush=True)
        ab.report_builds(q, [(what, "spec shipped", {b: f"spec {b}" for b in libs if b != "shipped"})])

    for real in (False, True):
        for N in (1024, 4096):
            torch.cuda.empty_cache()
            shape(N, real)
    return 0


if __name__ == "__main__":
    sys.exit(main())
