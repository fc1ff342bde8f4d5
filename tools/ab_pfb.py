"""The polyphase filter bank channelizer (smfft_pfb_launch) against its floors and against the same result from the library's public
pieces, in one process, timed round robin so that drift of the box hits all alike (median of --reps event-timed launches each, every
shape warmed up before its timed window):
  fused     smfft_pfb_launch_tuned for the run length R in {1, 4, 16, whole run = ceil(tiles / grid)} x signal loads {nt, plain}: the
            second load policy is a second build of the library, given with --alt (the shipped one is smfft_amd/libsmfft_pfb.so or
            SMFFT_PFB_LIB); the two builds' outputs are compared to the bit on the timed inputs
                make -C smfft_amd/csrc PFB_LIB=../../build_ab/libsmfft_pfb_plain.so PFB_OBJDIR=../../build_ab/pfb_plain PFB_NT_LOADS=0 \\
                     ../../build_ab/libsmfft_pfb_plain.so
  bare      smfft_launch (forward, external) of the same C F transforms on the same buffers: what the weighting costs on top (floor 1.0)
  unfused   torch weights the frames into a (C F, N) buffer (P strided multiply-add kernels), smfft_launch transforms it -- main
            configuration only
  copy      a device copy that moves the same bytes, (C L + C F N) 8 (power mode: C L 8 + C F N 4): the same-run ceiling
Main configuration: C = 1, N = 1024, P = 8, F = 524288 (4 GiB in, 4 GiB out, complex mode), the output from plain hipMalloc and from
smfft_malloc_written_for; then N in {256, 4096} x P in {4, 8, 16} and power mode at the main shape.
    python tools/ab_pfb.py [--reps 30] [--alt build_ab/libsmfft_pfb_plain.so]
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

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

WORKGROUPS_PER_CU = 3          # smfft_pfb.hip, kWorkgroupsPerCu
MAIN = (1, 1024, 8, 1 << 19)   # C, N, P, F
PMC_LAUNCHES = 3


def pmc_report(dirs):
    """per counter: mean per dispatch of the bare transform, the R = 1 launches and the shipped-R launches (dispatch order of --pmc)"""
    C, N, P, F = MAIN
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--alt", help="a second build of libsmfft_pfb.so (the other signal-load policy)")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--pmc-report", nargs="+")
    ap.add_argument("--small", action="store_true", help="a sixteenth of every shape (a rehearsal, not a measurement)")
    args = ap.parse_args()
    if args.pmc_report:
        return pmc_report(args.pmc_report)

    import ctypes

    import torch

    import smfft_amd as sm
    from smfft_amd import pfb

    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # the shipped library's load policy is the default of its source
    src = open(os.path.join(ROOT, "smfft_amd", "csrc", "smfft_pfb.hip")).read()
    libs = {"nt" if re.search(r"#define SMFFT_PFB_NT_LOADS (\d)", src).group(1) == "1" else "plain": pfb.lib()}
    if args.alt:
        libs["plain" if "nt" in libs else "nt"] = pfb.load(os.path.abspath(args.alt))
    shipped = next(iter(libs))
    gen = torch.Generator(device="cuda").manual_seed(0)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def round_robin(fns, reps):
        ts = {n: [] for n in fns}
        for fn in fns.values():
            fn(), fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for name, fn in fns.items():
                ts[name].append(timed(fn))
        return {n: sorted(v) for n, v in ts.items()}

    def shape(C, N, P, F, power, unfused=False, placed=False, only=None):
        """one shape: allocate, check, time, report; returns the medians"""
        if args.small:
            F //= 16
        L = (F + P - 1) * N
        width = 4 if power else 8
        moved = C * L * 8 + C * F * N * width
        x = torch.view_as_complex(torch.randn((C, L, 2), dtype=torch.float32, device="cuda", generator=gen))
        h = torch.from_numpy(pfb.prototype(N, P)).cuda()
        out = torch.empty((C, F, N), dtype=torch.float32 if power else torch.complex64, device="cuda")
        tiles = -(-(C * F) // (4096 // N))
        whole = -(-tiles // (cus * WORKGROUPS_PER_CU))
        default = pfb.default_tile_run(N, P)
        what = f"C={C} N={N} P={P} F={F} {'power' if power else 'complex'}"
        print(f"--- {what}: {C * L * 8 / 2**30:.2f} GiB in, {C * F * N * width / 2**30:.2f} GiB out, {tiles} tiles, whole run = {whole}, "
              f"shipped R = {default}, shipped loads = {shipped}", flush=True)

        def fused(lib, R, o):
            def run():
                rc = lib.smfft_pfb_launch_tuned(x.data_ptr(), L, C, h.data_ptr(), N, P, int(power), o.data_ptr(), sp, R)
                assert rc == 0, rc
            return run

        fns = {}
        runs = (("R=1", 1), ("R=4", 4), ("R=16", 16), (f"R=whole({whole})", whole))
        for policy, lib in libs.items():
            for label, R in runs:
                fns[f"fused {policy:5s} {label}"] = fused(lib, R, out)
        if only:
            fns = {k: v for k, v in fns.items() if only(k)}
        pw = ctypes.c_void_p()
        if placed:
            assert sm.lib.smfft_malloc_written_for(x.data_ptr(), out.numel() * width, ctypes.byref(pw)) == 0
            fns[f"fused {shipped:5s} R=0 (shipped), output of smfft_malloc_written_for"] = fused(libs[shipped], 0, _Ptr(pw.value))
        fns[f"fused {shipped:5s} R=0 (shipped = {default})"] = fused(libs[shipped], 0, out)
        if not power:
            fns["bare smfft_launch, same C F transforms"] = lambda: sm.launch("ct", "external", x.data_ptr(), out.data_ptr(), N, C * F, False, True, stream=sp)
        src = torch.empty(moved // 8, dtype=torch.float32, device="cuda").normal_(generator=gen)
        dst = torch.empty_like(src)
        fns["copy of the same bytes"] = lambda: dst.copy_(src)
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
        # every schedule and both builds give the same bits on the timed inputs
        base = None
        for name, fn in fns.items():
            if name.startswith("fused") and "malloc_written_for" not in name:
                out.fill_(0)
                fn()
                torch.cuda.synchronize()
                bits = out.view(torch.float32).view(torch.int32)
                if base is None:
                    base = bits.clone()
                else:
                    assert torch.equal(bits, base), f"{name}: bits differ"
        print("all fused variants: identical bits", flush=True)
        del base
        if args.trace or args.pmc:
            return None
        ts = round_robin(fns, args.reps)
        med = {n: v[len(v) // 2] for n, v in ts.items()}
        copy = med["copy of the same bytes"]
        for n, v in ts.items():
            line = f"{n:66s} median {med[n]:8.3f} ms  min {v[0]:8.3f}  {moved / med[n] / 1e9:7.3f} TB/s  {copy / med[n]:.3f} of the copy"
            if "bare smfft_launch, same C F transforms" in med and n.startswith("fused"):
                line += f"  {med[n] / med['bare smfft_launch, same C F transforms']:.3f} x bare"
            print(line, flush=True)
        ship = med[f"fused {shipped:5s} R=0 (shipped = {default})"]
        if unfused:
            print(f"GATE  unfused / fused (shipped) = {med['unfused: torch weighting + smfft_launch'] / ship:.2f} x  (must be >= 2)", flush=True)
        if pw.value:
            sm.lib.smfft_free_written(pw.value)
        return med

    class _Ptr:
        def __init__(self, p):
            self.p = p

        def data_ptr(self):
            return self.p

    if args.trace or args.pmc:
        # a few launches of each kernel, in a fixed order: bare, R = 1, shipped R (tools/ab_pfb.py --pmc-report relies on it)
        C, N, P, F = MAIN
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

    print(f"device: {torch.cuda.get_device_name(0)}, {cus} compute units, persistent grid {cus * WORKGROUPS_PER_CU} workgroups; {args.reps} reps round robin",
          flush=True)
    C, N, P, F = MAIN
    shape(C, N, P, F, False, unfused=True, placed=True)
    torch.cuda.empty_cache()
    shape(C, N, P, F, True)
    for N in (256, 4096):
        for P in (4, 8, 16):
            torch.cuda.empty_cache()
            shape(1, N, P, (1 << 29) // N, False)


if __name__ == "__main__":
    main()
