"""The polyphase filter bank channelizer for real streams (smfft_pfb_real_launch) against its ceiling, against the complex bank at the same
bytes and against the same result from the library's public pieces, in one process, timed round robin so that drift of the box hits
all alike (median and quartiles of --reps event-timed launches each, every shape warmed up before its timed window):
  fused     smfft_pfb_real_launch_tuned of the shipped library for the run length R in {1, 4, 16, whole run = ceil(tiles / grid)} and
            R = 0 (the shipped default), and R = 0 of every other build given with --alt NAME=PATH (the other split form, the other
            load policy; the shipped one is smfft_amd/libsmfft_pfb_real.so or SMFFT_PFB_REAL_LIB):
                make -C smfft_amd/csrc PFB_REAL_LIB=../../build_ab/libsmfft_pfb_real_lds.so PFB_REAL_OBJDIR=../../build_ab/pfb_real_lds \\
                     PFB_REAL_SPLIT=0 ../../build_ab/libsmfft_pfb_real_lds.so          (PFB_REAL_SPLIT=1: _regs; PFB_REAL_NT_LOADS=0: _plain)
            the schedules of one build must give the same bits; the builds are compared by their largest difference on the timed inputs
  unfused   torch weights the frames into a (C F, 2N) float buffer (P strided multiply-add kernels), smfft_launch(family = rc)
            transforms it (2N <= 4096; torch.fft.rfft at N = 4096, which also drops the packing: N + 1 values per row)
  complex   smfft_pfb_launch of the complex bank at the same N and F: the same bytes in and out, no split
  copy      a device copy that moves the same bytes, C L 4 + C F N 8 (power mode: C F N 4): the same-run ceiling
Main configuration: C = 1, N = 1024, P = 8, F = 524288 (4 GiB in, 4 GiB out, complex mode); then power mode there and N in {256, 4096}
x P in {4, 16}.
    python tools/ab_pfb_real.py [--reps 30] [--alt lds=build_ab/libsmfft_pfb_real_lds.so --alt regs=...] [--small]"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import ab_pfb_common as ab  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ab.add_arguments(ap, "libsmfft_pfb_real.so")
    ap.add_argument("--main-only", action="store_true")
    args = ap.parse_args()

    import torch

    import smfft_amd as sm
    from smfft_amd import pfb, pfb_real

    ses = ab.Session(pfb_real, "smfft_pfb_real", args)
    sp, gen = ses.sp, ses.gen
    libs = {"shipped": pfb_real.lib()}
    libs.update(ses.load(item) for item in args.alt)

    def shape(C, N, P, F, power, gate=False):
        if args.small:
            F //= 16
        L = (F + P - 1) * 2 * N
        width = 4 if power else 8
        moved = C * L * 4 + C * F * N * width
        x = torch.randn((C, L), dtype=torch.float32, device="cuda", generator=gen)
        h = torch.from_numpy(pfb_real.prototype(N, P)).cuda()
        out = torch.empty((C, F, N), dtype=torch.float32 if power else torch.complex64, device="cuda")
        default = pfb_real.default_tile_run(N, P)
        what, runs = ses.start_shape(C, N, P, F, power, C * L * 4, default)

        fns = {f"fused shipped {label}": ses.fused(libs["shipped"], x, L, C, h, N, P, power, out, R) for label, R in runs}
        for name, lib in libs.items():
            fns[f"fused {name} R=0 (default = {default})"] = ses.fused(lib, x, L, C, h, N, P, power, out, 0)
        ship = f"fused shipped R=0 (default = {default})"

        # the schedules of the shipped build: the same bits; the other builds: their largest difference from it
        base = ab.compare_outputs(fns, out, lambda name: name.startswith("fused shipped"))
        print("all schedules of the shipped build: identical bits", flush=True)

        # the unfused pipeline from public pieces
        buf = torch.empty((C, F, 2 * N), dtype=torch.float32, device="cuda")
        blocks = x[:, :(F + P - 1) * 2 * N].view(C, F + P - 1, 2 * N)
        hp = h.view(P, 1, 1, 2 * N)
        packed = 2 * N <= 4096
        spectrum = torch.empty((C, F, N), dtype=torch.complex64, device="cuda") if packed else torch.empty((C, F, N + 1), dtype=torch.complex64, device="cuda")

        def unfused():
            torch.mul(blocks[:, 0:F], hp[0], out=buf)
            for p in range(1, P):
                buf.addcmul_(blocks[:, p:p + F], hp[p])
            if packed:
                sm.launch("rc", "external", buf.data_ptr(), spectrum.data_ptr(), 2 * N, C * F, False, True, stream=sp)
            else:
                torch.fft.rfft(buf, dim=-1, out=spectrum)
        uname = "unfused: torch weighting + " + ("smfft_launch(rc)" if packed else "torch.fft.rfft")
        if not power:
            fns[uname] = unfused
            unfused()
            torch.cuda.synchronize()
            if packed:
                diff = (spectrum - base).abs().max()
            else:
                diff = torch.maximum((spectrum[..., 1:N] - base[..., 1:]).abs().max(),
                                     torch.maximum((spectrum[..., 0].real - base[..., 0].real).abs().max(), (spectrum[..., N].real - base[..., 0].imag).abs().max()))
            print(f"max |unfused - fused| / max |fused| = {(diff / base.abs().max()).item():.2e}", flush=True)
        del base

        # the complex bank at the same N and F: the same bytes in and out
        # (the signal read as (F + P - 1) N float2 per stream, the first P N taps)
        fns["complex bank smfft_pfb_launch, same N and F (same bytes)"] = lambda: pfb.launch(x.data_ptr(), (F + P - 1) * N, C, h.data_ptr(), N, P, out.data_ptr(), power=power, stream=sp)
        fns[ab.COPY] = ses.copy_of(moved)

        q = ab.report(ses.round_robin(fns), moved, 62, True)
        ab.report_builds(q, [(what + " R=0", ship, {b: f"fused {b} R=0 (default = {default})" for b in libs if b != "shipped"})])
        fm = q[ship][1]
        print(f"fused (shipped) / complex bank at the same bytes = {fm / q['complex bank smfft_pfb_launch, same N and F (same bytes)'][1]:.3f}", flush=True)
        if not power:
            print(f"unfused / fused (shipped) = {q[uname][1] / fm:.2f} x", flush=True)
            if gate:
                ok = q[ship][2] < q[uname][0]
                print(f"GATE  fused upper quartile {q[ship][2]:.3f} ms < unfused lower quartile {q[uname][0]:.3f} ms: {'PASS' if ok else 'FAIL'}", flush=True)
                return ok
        return True

    ses.headline(libs)
    C, N, P, F = ab.MAIN
    ok = shape(C, N, P, F, False, gate=True)
    if not args.main_only:
        torch.cuda.empty_cache()
        shape(C, N, P, F, True)
        for N in (256, 4096):
            for P in (4, 16):
                torch.cuda.empty_cache()
                shape(1, N, P, (1 << 29) // N, False)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
