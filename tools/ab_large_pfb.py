"""The polyphase filter bank channelizer for N = 8192 / 16384 channels (smfft_large_pfb_launch) against its floors and against the same
result from the library's public pieces, in one process, timed round robin so that drift of the box hits all alike (median and
quartiles of --reps event-timed launches each, every shape warmed up before its timed window):
  fused     smfft_large_pfb_launch_tuned under schedule 1 (stride) and 2 (XCD-blocked), and the plain launch (the shipped default), of
            the shipped library (smfft_amd/libsmfft_large_pfb.so or SMFFT_LARGE_PFB_LIB) and of every other build given with
            --alt NAME=PATH (the other signal-load policy; a bare PATH takes that name):
                make -C smfft_amd/csrc LARGE_PFB_LIB=../../build_ab/libsmfft_large_pfb_nt.so LARGE_PFB_OBJDIR=../../build_ab/large_pfb_nt \\
                     LARGE_PFB_NT_LOADS=1 ../../build_ab/libsmfft_large_pfb_nt.so
            the outputs of all fused variants are compared to the bit on the timed inputs
  bare      smfft_large_launch (forward) of the same C F transforms on the same buffers: what the weighting costs on top (floor 1.0)
  unfused   torch weights the frames into a (C F, N) buffer (P strided multiply-add kernels), smfft_large_launch transforms it
  copy      a device copy that moves the same bytes, (C L + C F N) 8 (power mode: C L 8 + C F N 4): the same-run ceiling
Main configurations: C = 1, P = 8, 4 GiB in (L = 2^29), at N = 8192 and N = 16384, complex mode; then P in {4, 16, 32} and power mode.
The gate, at both main configurations: the fused kernel's upper quartile lies below the unfused pipeline's lower quartile.
    python tools/ab_large_pfb.py [--reps 30] [--alt build_ab/libsmfft_large_pfb_nt.so] [--alt NAME=PATH ...] [--small] [--main-only]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ab_large_pfb.py --trace     three launches of each kernel, nothing timed
    rocprofv3 --pmc FETCH_SIZE -d DIR -- python tools/ab_large_pfb.py --pmc             counters only, in a run of their own (WRITE_SIZE: another)"""
import argparse
import os
import re
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import ab_pfb_common as ab  # noqa: E402

SIZES = (8192, 16384)
MAIN_P, MAIN_L = 8, 1 << 29      # 4 GiB of complex64 in
LAUNCHES = 3                     # of each kernel under --trace / --pmc
SCHEDULES = (("stride", 1), ("blocked", 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--main-only", action="store_true")
    ab.add_arguments(ap, "libsmfft_large_pfb.so (a bare PATH: the other signal-load policy)")
    args = ap.parse_args()

    import torch

    from smfft_amd import large, large_pfb

    ses = ab.Session(large_pfb, "smfft_large_pfb", args)
    sp, gen = ses.sp, ses.gen
    # the shipped library's load policy is taken to be the default of its source: a library named by SMFFT_LARGE_PFB_LIB that was built
    # with the other policy is labelled wrongly here (give such a build with --alt NAME=PATH instead)
    src = open(os.path.join(ROOT, "smfft_amd", "csrc", "smfft_large_pfb.hip")).read()
    shipped = "nt" if re.search(r"#define SMFFT_LARGE_PFB_NT_LOADS (\d)", src).group(1) == "1" else "plain"
    libs = {shipped: large_pfb.lib()}
    libs.update(ses.load(item, "plain" if shipped == "nt" else "nt") for item in args.alt)

    def buffers(C, N, P, L, power):
        F = large_pfb.frames(L, N, P)
        x = torch.view_as_complex(torch.randn((C, L, 2), dtype=torch.float32, device="cuda", generator=gen))
        h = torch.from_numpy(large_pfb.prototype(N, P)).cuda()
        out = torch.empty((C, F, N), dtype=torch.float32 if power else torch.complex64, device="cuda")
        return F, x, h, out

    def fused(lib, x, L, C, h, N, P, power, out, schedule):
        def run():
            rc = lib.smfft_large_pfb_launch_tuned(x.data_ptr(), L, C, h.data_ptr(), N, P, int(power), out.data_ptr(), sp, schedule, 0)
            assert rc == 0, rc
        return run

    def shape(C, N, P, L, power, gate=False):
        """one shape: allocate, check, time, report; returns whether the gate holds (True where there is none)"""
        if args.small:
            L //= 16
        F, x, h, out = buffers(C, N, P, L, power)
        width = 4 if power else 8
        moved = C * L * 8 + C * F * N * width
        default = large_pfb.default_schedule(N, P)
        what = f"C={C} N={N} P={P} F={F} {'power' if power else 'complex'}"
        print(f"--- {what}: {C * L * 8 / 2**30:.2f} GiB in, {C * F * N * width / 2**30:.2f} GiB out, grid {large.grid(N)} workgroups, "
              f"shipped schedule = {default}, shipped loads = {shipped}", flush=True)
        fns = {f"fused {policy:5s} {label}": fused(lib, x, L, C, h, N, P, power, out, s) for policy, lib in libs.items() for label, s in SCHEDULES}
        ship = f"fused {shipped:5s} default (schedule {default})"
        fns[ship] = fused(libs[shipped], x, L, C, h, N, P, power, out, 0)
        base = ab.compare_outputs(fns, out, lambda name: True)
        print("all fused variants: identical bits", flush=True)
        bare = "bare smfft_large_launch, same C F transforms"
        uname = "unfused: torch weighting + smfft_large_launch"
        if not power:
            fns[bare] = lambda: large.launch(x.data_ptr(), out.data_ptr(), N, C * F, False, stream=sp)
            buf = torch.empty((C, F, N), dtype=torch.complex64, device="cuda")
            blocks = torch.view_as_real(x[:, :(F + P - 1) * N].view(C, F + P - 1, N))
            hp = h.view(P, 1, 1, N, 1)
            bufr = torch.view_as_real(buf)

            def unfused():
                torch.mul(blocks[:, 0:F], hp[0], out=bufr)
                for p in range(1, P):
                    bufr.addcmul_(blocks[:, p:p + F], hp[p])
                large.launch(buf.data_ptr(), out.data_ptr(), N, C * F, False, stream=sp)
            fns[uname] = unfused
            unfused()
            torch.cuda.synchronize()
            print(f"max |unfused - fused| / max |fused| = {((out - base).abs().max() / base.abs().max()).item():.2e}", flush=True)
        del base
        fns[ab.COPY] = ses.copy_of(moved)
        q = ab.report(ses.round_robin(fns), moved, 52, True,
                      lambda n, q: f"  {q[n][1] / q[bare][1]:.3f} x bare" if bare in q and n.startswith("fused") else "")
        ab.report_builds(q, [(f"{what} {label}", f"fused {shipped:5s} {label}", {b: f"fused {b:5s} {label}" for b in libs if b != shipped})
                             for label, _ in SCHEDULES])
        ok = True
        if not power:
            print(f"unfused / fused (shipped) = {q[uname][1] / q[ship][1]:.2f} x", flush=True)
            if gate:
                ok = q[ship][2] < q[uname][0]
                print(f"GATE  fused upper quartile {q[ship][2]:.3f} ms < unfused lower quartile {q[uname][0]:.3f} ms: {'PASS' if ok else 'FAIL'}", flush=True)
        return ok

    if args.trace or args.pmc:
        # a few launches of each kernel in a fixed order, per length: bare, stride, blocked (and the power kernel under --trace)
        for N in SIZES:
            L = MAIN_L // 16 if args.small else MAIN_L
            F, x, h, out = buffers(1, N, MAIN_P, L, False)
            for _ in range(LAUNCHES):
                large.launch(x.data_ptr(), out.data_ptr(), N, F, False, stream=sp)
            for _, s in SCHEDULES:
                for _ in range(LAUNCHES):
                    fused(libs[shipped], x, L, 1, h, N, MAIN_P, False, out, s)()
            if args.trace:
                powers = torch.empty((1, F, N), dtype=torch.float32, device="cuda")
                for _ in range(LAUNCHES):
                    fused(libs[shipped], x, L, 1, h, N, MAIN_P, True, powers, 0)()
            torch.cuda.synchronize()
            print(f"{'trace' if args.trace else 'pmc'}: {LAUNCHES} launches each of bare, fused stride, fused blocked at C=1 N={N} P={MAIN_P} F={F}", flush=True)
            del x, h, out
            torch.cuda.empty_cache()
        return 0

    print(f"device: {torch.cuda.get_device_name(0)}, {ses.cus} compute units; {ses.reps} reps round robin; builds: {', '.join(libs)}", flush=True)
    ok = True
    for N in SIZES:
        torch.cuda.empty_cache()
        ok = shape(1, N, MAIN_P, MAIN_L, False, gate=True) and ok
    if not args.main_only:
        for N in SIZES:
            for P in (4, 16, 32):
                torch.cuda.empty_cache()
                shape(1, N, P, MAIN_L, False)
            torch.cuda.empty_cache()
            shape(1, N, MAIN_P, MAIN_L, True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
