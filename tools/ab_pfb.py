"""The polyphase filter bank channelizer (smfft_pfb_launch) against its floors and against the same result from the library's public
pieces, in one process, timed round robin so that drift of the box hits all alike (median of --reps event-timed launches each, every
shape warmed up before its timed window):
  fused     smfft_pfb_launch_tuned for the run length R in {1, 4, 16, whole run = ceil(tiles / grid)} x signal loads {nt, plain}: the
            second load policy is a second build of the library, given with --alt PATH (the shipped one is smfft_amd/libsmfft_pfb.so
            or SMFFT_PFB_LIB); further builds with --alt NAME=PATH (a parent commit's, say); all builds' outputs are compared to the bit
            on the timed inputs, and every build's median is set against the shipped one's at the same R
                make -C smfft_amd/csrc PFB_LIB=../../build_ab/libsmfft_pfb_plain.so PFB_OBJDIR=../../build_ab/pfb_plain PFB_NT_LOADS=0 \\
                     ../../build_ab/libsmfft_pfb_plain.so
  bare      smfft_launch (forward, external) of the same C F transforms on the same buffers: what the weighting costs on top (floor 1.0)
  unfused   torch weights the frames into a (C F, N) buffer (P strided multiply-add kernels), smfft_launch transforms it -- main
            configuration only
  copy      a device copy that moves the same bytes, (C L + C F N) 8 (power mode: C L 8 + C F N 4): the same-run ceiling
Main configuration: C = 1, N = 1024, P = 8, F = 524288 (4 GiB in, 4 GiB out, complex mode), the output from plain hipMalloc and from
smfft_malloc_written_for; then N in {256, 4096} x P in {4, 8, 16} and power mode at the main shape.
    python tools/ab_pfb.py [--reps 30] [--alt build_ab/libsmfft_pfb_plain.so] [--alt NAME=PATH ...] [--small]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ab_pfb.py --trace        three launches of each kernel, nothing timed
    rocprofv3 --pmc FETCH_SIZE -d DIR -- python tools/ab_pfb.py --pmc                counters only (WRITE_SIZE: a run of its own)
    python tools/ab_pfb.py --pmc-report DIR [DIR ...]                                 fetched bytes / (C L 8) for R = 1 and the shipped R
The counters are calibrated on the bare transform of the same run, which reads C F N 8 bytes with the same 8-byte-per-lane loads
(FETCH_SIZE has been calibrated for 16-byte-per-lane streaming reads only: DESIGN.md section 5.1)."""
import argparse
import csv
import glob
import os
import re
import sys
import types

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import ab_pfb_common as ab  # noqa: E402

PMC_LAUNCHES = 3


def pmc_report(dirs):
    """per counter: mean per dispatch of the bare transform, the R = 1 launches and the shipped-R launches (dispatch order of --pmc)"""
    C, N, P, F = ab.MAIN
    L = (F + P - 1) * N
    for d in dirs:
        files = sorted(glob.glob(d + "/**/*counter_collection.csv", recursive=True), key=os.path.getmtime)[-1:]
        if not files:
            print(f"{d}: no counter_collection.csv")
            continue
        rows = list(csv.DictReader(open(files[0])))
        for counter in sorted({r["Counter_Name"] for r in rows}):
            mine = sorted((r for r in rows if r["Counter_Name"] == counter), key=lambda r: int(r["Dispatch_Id"]))
            fused = [float(r["Counter_Value"]) for r in mine if "pfb_kernel" in r["Kernel_Name"]]
            bare = [float(r["Counter_Value"]) for r in mine if "pfb_kernel" not in r["Kernel_Name"] and "FFT" in r["Kernel_Name"]]
            if len(fused) != 2 * PMC_LAUNCHES or not bare:
                print(f"{d} {counter}: {len(fused)} fused and {len(bare)} bare dispatches, expected {2 * PMC_LAUNCHES} and {PMC_LAUNCHES}")
                continue
            b = sum(bare) / len(bare)
            r1, rs = sum(fused[:PMC_LAUNCHES]) / PMC_LAUNCHES, sum(fused[PMC_LAUNCHES:]) / PMC_LAUNCHES
            # the bare transform moves C F N 8 bytes each way; the fused kernel should read C L 8 and write C F N 8
            ideal = (C * L) / (C * F * N) if counter == "FETCH_SIZE" else 1.0
            print(f"{counter}: bare {b:.6g}  R=1 {r1:.6g}  shipped R {rs:.6g}  (counter units per dispatch)")
            print(f"  {counter} / bare, over the ideal ratio {ideal:.6f}:  R=1 {r1 / b / ideal:.4f}   shipped R {rs / b / ideal:.4f}"
                  + ("   = fetched bytes / (C L 8)" if counter == "FETCH_SIZE" else "   = written bytes / (C F N 8)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--pmc-report", nargs="+")
    ab.add_arguments(ap, "libsmfft_pfb.so (a bare PATH: the other signal-load policy)")
    args = ap.parse_args()
    if args.pmc_report:
        return pmc_report(args.pmc_report)

    import ctypes

    import torch

    import smfft_amd as sm
    from smfft_amd import pfb

    ses = ab.Session(pfb, "smfft_pfb", args)
    sp, gen = ses.sp, ses.gen
    # the shipped library's load policy is the default of its source
    src = open(os.path.join(ROOT, "smfft_amd", "csrc", "smfft_pfb.hip")).read()
    shipped = "nt" if re.search(r"#define SMFFT_PFB_NT_LOADS (\d)", src).group(1) == "1" else "plain"
    libs = {shipped: pfb.lib()}
    libs.update(ses.load(item, "plain" if shipped == "nt" else "nt") for item in args.alt)

    def shape(C, N, P, F, power, unfused=False, placed=False):
        """one shape: allocate, check, time, report; returns the medians"""
        if args.small:
            F //= 16
        L = (F + P - 1) * N
        width = 4 if power else 8
        moved = C * L * 8 + C * F * N * width
        x = torch.view_as_complex(torch.randn((C, L, 2), dtype=torch.float32, device="cuda", generator=gen))
        h = torch.from_numpy(pfb.prototype(N, P)).cuda()
        out = torch.empty((C, F, N), dtype=torch.float32 if power else torch.complex64, device="cuda")
        default = pfb.default_tile_run(N, P)
        what, runs = ses.start_shape(C, N, P, F, power, C * L * 8, default, f", shipped loads = {shipped}")

        def fused(lib, R, o):
            return ses.fused(lib, x, L, C, h, N, P, power, o, R)

        fns = {f"fused {policy:5s} {label}": fused(lib, R, out) for policy, lib in libs.items() for label, R in runs}
        pw = ctypes.c_void_p()
        if placed:
            assert sm.lib.smfft_malloc_written_for(x.data_ptr(), out.numel() * width, ctypes.byref(pw)) == 0
            fns[f"fused {shipped:5s} R=0 (shipped), output of smfft_malloc_written_for"] = fused(libs[shipped], 0, types.SimpleNamespace(data_ptr=lambda: pw.value))
        fns[f"fused {shipped:5s} R=0 (shipped = {default})"] = fused(libs[shipped], 0, out)
        bare = "bare smfft_launch, same C F transforms"
        if not power:
            fns[bare] = lambda: sm.launch("ct", "external", x.data_ptr(), out.data_ptr(), N, C * F, False, True, stream=sp)
        fns[ab.COPY] = ses.copy_of(moved)
        if unfused:
            buf = torch.empty((C, F, N), dtype=torch.complex64, device="cuda")
            blocks = torch.view_as_real(x[:, :(F + P - 1) * N].view(C, F + P - 1, N))
            hp = h.view(P, 1, 1, N, 1)
            bufr = torch.view_as_real(buf)

            def run():
                torch.mul(blocks[:, 0:F], hp[0], out=bufr)
                for p in range(1, P):
                    bufr.addcmul_(blocks[:, p:p + F], hp[p])
                sm.launch("ct", "external", buf.data_ptr(), out.data_ptr(), N, C * F, False, True, stream=sp)
            fns["unfused: torch weighting + smfft_launch"] = run
            # the unfused pipeline computes the same thing
            run()
            ref = out.clone()
            fused(libs[shipped], 0, out)()
            torch.cuda.synchronize()
            print(f"max |fused - unfused| / max |unfused| = {((out - ref).abs().max() / ref.abs().max()).item():.2e}", flush=True)
            del ref
        # every schedule and every build give the same bits on the timed inputs
        ab.compare_outputs({n: fn for n, fn in fns.items() if n.startswith("fused") and "malloc_written_for" not in n}, out, lambda name: True)
        print("all fused variants: identical bits", flush=True)
        if args.trace or args.pmc:
            return None
        q = ab.report(ses.round_robin(fns), moved, 66, False,
                      lambda n, q: f"  {q[n][1] / q[bare][1]:.3f} x bare" if bare in q and n.startswith("fused") else "")
        ab.report_builds(q, [(f"{what} {label}", f"fused {shipped:5s} {label}", {b: f"fused {b:5s} {label}" for b in libs if b != shipped})
                             for label, _ in runs])
        ship = q[f"fused {shipped:5s} R=0 (shipped = {default})"][1]
        if unfused:
            print(f"GATE  unfused / fused (shipped) = {q['unfused: torch weighting + smfft_launch'][1] / ship:.2f} x  (must be >= 2)", flush=True)
        if pw.value:
            sm.lib.smfft_free_written(pw.value)
        return {n: v[1] for n, v in q.items()}

    if args.trace or args.pmc:
        # a few launches of each kernel, in a fixed order: bare, R = 1, shipped R (tools/ab_pfb.py --pmc-report relies on it)
        C, N, P, F = ab.MAIN
        if args.small:
            F //= 16
        L = (F + P - 1) * N
        x = torch.view_as_complex(torch.randn((C, L, 2), dtype=torch.float32, device="cuda", generator=gen))
        h = torch.from_numpy(pfb.prototype(N, P)).cuda()
        out = torch.empty((C, F, N), dtype=torch.complex64, device="cuda")
        lib = libs[shipped]
        for _ in range(PMC_LAUNCHES):
            sm.launch("ct", "external", x.data_ptr(), out.data_ptr(), N, C * F, False, True, stream=sp)
        for R in (1, 0):
            for _ in range(PMC_LAUNCHES):
                assert lib.smfft_pfb_launch_tuned(x.data_ptr(), L, C, h.data_ptr(), N, P, 0, out.data_ptr(), sp, R) == 0
        if args.trace:
            powers = torch.empty((C, F, N), dtype=torch.float32, device="cuda")
            for _ in range(PMC_LAUNCHES):
                assert lib.smfft_pfb_launch(x.data_ptr(), L, C, h.data_ptr(), N, P, 1, powers.data_ptr(), sp) == 0
        torch.cuda.synchronize()
        print(f"{'trace' if args.trace else 'pmc'}: {PMC_LAUNCHES} launches each of bare, fused R=1, fused shipped R "
              f"({pfb.default_tile_run(N, P)}) at C={C} N={N} P={P} F={F}", flush=True)
        return

    ses.headline(libs)
    C, N, P, F = ab.MAIN
    shape(C, N, P, F, False, unfused=True, placed=True)
    torch.cuda.empty_cache()
    shape(C, N, P, F, True)
    for N in (256, 4096):
        for P in (4, 8, 16):
            torch.cuda.empty_cache()
            shape(1, N, P, (1 << 29) // N, False)


if __name__ == "__main__":
    main()
