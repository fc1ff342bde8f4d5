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

WORKGROUPS_PER_CU = 3          # smfft_pfb_real.hip, kWorkgroupsPerCu
MAIN = (1, 1024, 8, 1 << 19)   # C, N, P, F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libsmfft_pfb_real.so")
    ap.add_argument("--small", action="store_true", help="a sixteenth of every shape (a rehearsal, not a measurement)")
    ap.add_argument("--main-only", action="store_true")
    args = ap.parse_args()

    import torch

    import smfft_amd as sm
    from smfft_amd import pfb, pfb_real

    sm.FFT_init()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    libs = {"shipped": pfb_real.lib()}
    for item in args.alt:
        name, path = item.split("=", 1)
        libs[name] = pfb_real.load(os.path.abspath(path))
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

    def shape(C, N, P, F, power, gate=False):
        if args.small:
            F //= 16
        L = (F + P - 1) * 2 * N
        width = 4 if power else 8
        moved = C * L * 4 + C * F * N * width
        x = torch.randn((C, L), dtype=torch.float32, device="cuda", generator=gen)
        h = torch.from_numpy(pfb_real.prototype(N, P)).cuda()
        out = torch.empty((C, F, N), dtype=torch.float32 if power else torch.complex64, device="cuda")
        tiles = -(-(C * F) // (4096 // N))
        whole = -(-tiles // (cus * WORKGROUPS_PER_CU))
        default = pfb_real.default_tile_run(N, P)
        what = f"C={C} N={N} P={P} F={F} {'power' if power else 'complex'}"
        print(f"--- {what}: {C * L * 4 / 2**30:.2f} GiB in, {C * F * N * width / 2**30:.2f} GiB out, {tiles} tiles, whole run = {whole}, "
              f"shipped R = {default}", flush=True)

        def fused(lib, R, o=out):
            def run():
                rc = lib.smfft_pfb_real_launch_tuned(x.data_ptr(), L, C, h.data_ptr(), N, P, int(power), o.data_ptr(), sp, R)
                assert rc == 0, rc
            return run

        fns = {}
        for label, R in (("R=1", 1), ("R=4", 4), ("R=16", 16), (f"R=whole({whole})", whole)):
            fns[f"fused shipped {label}"] = fused(libs["shipped"], R)
        for name, lib in libs.items():
            fns[f"fused {name} R=0 (default = {default})"] = fused(lib, 0)
        ship = f"fused shipped R=0 (default = {default})"

        # the schedules of the shipped build: the same bits; the other builds: their largest difference from it
        base = None
        for name, fn in fns.items():
            out.fill_(0)
            fn()
            torch.cuda.synchronize()
            if base is None:
                base = out.clone()
            elif name.startswith("fused shipped"):
                assert torch.equal(out.view(torch.float32).view(torch.int32), base.view(torch.float32).view(torch.int32)), f"{name}: bits differ"
            else:
                print(f"max |{name} - shipped| / max |shipped| = {((out - base).abs().max() / base.abs().max()).item():.2e}", flush=True)
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
        src = torch.empty(moved // 8, dtype=torch.float32, device="cuda").normal_(generator=gen)
        dst = torch.empty_like(src)
        fns["copy of the same bytes"] = lambda: dst.copy_(src)

        ts = round_robin(fns, args.reps)
        q = {n: (v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]) for n, v in ts.items()}
        copy = q["copy of the same bytes"][1]
        for n, v in ts.items():
            lo, med, hi = q[n]
            print(f"{n:62s} median {med:8.3f} ms  quartiles {lo:8.3f} {hi:8.3f}  min {v[0]:8.3f}  {moved / med / 1e9:7.3f} TB/s  {copy / med:.3f} of the copy", flush=True)
        fm = q[ship][1]
        print(f"fused (shipped) / complex bank at the same bytes = {fm / q['complex bank smfft_pfb_launch, same N and F (same bytes)'][1]:.3f}", flush=True)
        if not power:
            print(f"unfused / fused (shipped) = {q[uname][1] / fm:.2f} x", flush=True)
            if gate:
                ok = q[ship][2] < q[uname][0]
                print(f"GATE  fused upper quartile {q[ship][2]:.3f} ms < unfused lower quartile {q[uname][0]:.3f} ms: {'PASS' if ok else 'FAIL'}", flush=True)
                return ok
        return True

    print(f"device: {torch.cuda.get_device_name(0)}, {cus} compute units, persistent grid {cus * WORKGROUPS_PER_CU} workgroups; {args.reps} reps round robin; "
          f"builds: {', '.join(libs)}", flush=True)
    C, N, P, F = MAIN
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
