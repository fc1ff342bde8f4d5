"""What tools/ab_pfb.py and tools/ab_pfb_real.py share: the device and its persistent grid, the builds given with --alt, the fused launch
of a build, the run lengths of a shape, the event-timed round robin, the copy of the same bytes and the lines of the report."""
import os

import torch

WORKGROUPS_PER_CU = 3          # smfft_pfb_kernel.hpp, kWorkgroupsPerCu
MAIN = (1, 1024, 8, 1 << 19)   # C, N, P, F
COPY = "copy of the same bytes"


def add_arguments(ap, library):
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help=f"another build of {library}")
    ap.add_argument("--small", action="store_true", help="a sixteenth of every shape (a rehearsal, not a measurement)")


class Session:
    """one process, one stream, one generator; mirror = smfft_amd.pfb or smfft_amd.pfb_real"""

    def __init__(self, mirror, prefix, args):
        import smfft_amd as sm
        sm.FFT_init()
        torch.cuda.init()
        self.mirror, self.prefix, self.reps = mirror, prefix, args.reps
        self.stream = torch.cuda.current_stream()
        self.sp = self.stream.cuda_stream
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.gen = torch.Generator(device="cuda").manual_seed(0)

    def load(self, item, default_name=None):
        """(name, handle) of an --alt item NAME=PATH; a bare PATH takes default_name"""
        name, path = item.split("=", 1) if "=" in item else (default_name, item)
        assert name, f"--alt {item}: NAME=PATH"
        return name, self.mirror.load(os.path.abspath(path))

    def headline(self, libs):
        print(f"device: {torch.cuda.get_device_name(0)}, {self.cus} compute units, persistent grid {self.cus * WORKGROUPS_PER_CU} workgroups; "
              f"{self.reps} reps round robin; builds: {', '.join(libs)}", flush=True)

    def start_shape(self, C, N, P, F, power, bytes_in, default, extra=""):
        """prints the shape's headline; returns (its name, the (label, R) the fused kernel is timed at)"""
        tiles = -(-(C * F) // (4096 // N))
        whole = -(-tiles // (self.cus * WORKGROUPS_PER_CU))
        what = f"C={C} N={N} P={P} F={F} {'power' if power else 'complex'}"
        print(f"--- {what}: {bytes_in / 2**30:.2f} GiB in, {C * F * N * (4 if power else 8) / 2**30:.2f} GiB out, {tiles} tiles, whole run = {whole}, "
              f"shipped R = {default}{extra}", flush=True)
        return what, (("R=1", 1), ("R=4", 4), ("R=16", 16), (f"R=whole({whole})", whole))

    def fused(self, lib, x, L, C, h, N, P, power, out, R):
        launch = getattr(lib, self.prefix + "_launch_tuned")

        def run():
            rc = launch(x.data_ptr(), L, C, h.data_ptr(), N, P, int(power), out.data_ptr(), self.sp, R)
            assert rc == 0, rc
        return run

    def copy_of(self, moved):
        """a device copy that moves `moved` bytes: the same-run ceiling"""
        src = torch.empty(moved // 8, dtype=torch.float32, device="cuda").normal_(generator=self.gen)
        dst = torch.empty_like(src)
        return lambda: dst.copy_(src)

    def round_robin(self, fns):
        """{name: the sorted times of self.reps event-timed launches}, every fn warmed up first"""
        ts = {n: [] for n in fns}
        for fn in fns.values():
            fn(), fn()
        torch.cuda.synchronize()
        for _ in range(self.reps):
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(self.stream)
                fn()
                b.record(self.stream)
                b.synchronize()
                ts[name].append(a.elapsed_time(b))
        return {n: sorted(v) for n, v in ts.items()}


def compare_outputs(fns, out, strict):
    """run every fn into `out`: against the first one's result, the same bits where strict(name), else the largest difference is printed.
    Returns the first one's result."""
    base = None
    for name, fn in fns.items():
        out.fill_(0)
        fn()
        torch.cuda.synchronize()
        if base is None:
            base = out.clone()
        elif strict(name):
            assert torch.equal(out.view(torch.float32).view(torch.int32), base.view(torch.float32).view(torch.int32)), f"{name}: bits differ"
        else:
            print(f"max |{name} - shipped| / max |shipped| = {((out - base).abs().max() / base.abs().max()).item():.2e}", flush=True)
    return base


def report(ts, moved, width, with_quartiles, suffix=lambda name, q: ""):
    """one line per timed function of round_robin's ts, ended by suffix(name, q); ts[COPY] is the ceiling.  Returns q = {name: (lower
    quartile, median, upper quartile)}"""
    q = {n: (v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]) for n, v in ts.items()}
    copy = q[COPY][1]
    for n, v in ts.items():
        lo, med, hi = q[n]
        spread = f"quartiles {lo:8.3f} {hi:8.3f}  " if with_quartiles else ""
        print(f"{n:{width}s} median {med:8.3f} ms  {spread}min {v[0]:8.3f}  {moved / med / 1e9:7.3f} TB/s  {copy / med:.3f} of the copy{suffix(n, q)}", flush=True)
    return q


def report_builds(q, pairs):
    """pairs: (label, name of the shipped build's entry, {build: name of its entry}): the medians' ratios build / shipped"""
    for label, shipped, others in pairs:
        for build, name in others.items():
            print(f"BUILDS  {label}: shipped {q[shipped][1]:.4f} ms, {build} {q[name][1]:.4f} ms, shipped / {build} = {q[shipped][1] / q[name][1]:.4f}", flush=True)
