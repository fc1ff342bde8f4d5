#!/usr/bin/env python3
"""Do the kernels of a base commit compile to the same gfx950 code on the working tree?  (CPU only: hipcc cross-compiles.)

Compiles, on a checkout of BASE (git archive into a temporary directory) and on the working tree, with the Makefile's flags:
  smfft_amd/csrc/smfft_inst.hip   both objects (SMFFT_INST_PART = 1, 2 with tools/inst_flags.py) of all 8 lengths
  smfft_amd/csrc/smfft_fir.hip    the main library's FIR object (all five lengths in one unit, the main library's flags)
  smfft_amd/csrc/smfft_large.hip, smfft_large_real.hip, smfft_large_fir.hip, smfft_pfb.hip, smfft_pfb_real.hip, smfft_large_pfb.hip, smfft_pfb_spec.hip,
  smfft_fir_real.hip, smfft_fir_detect.hip, smfft_bluestein.hip, smfft_czt.hip, smfft_rowconv.hip, smfft_rowconv_real.hip, smfft_dct.hip, smfft_hilbert.hip, smfft_mdct.hip, smfft_stft.hip, smfft_welch.hip, smfft_bands.hip   the per-length objects of the nineteen add-on libraries, each with its <PREFIX>_FLAGS_<N> of the Makefile
                                  (and the -I. of the seventeen that include headers of that directory), where BASE has the file
  examples/*.hip                  the files BASE has
to device assembly (hipcc -S --cuda-device-only) and compares every kernel BASE has, text of its body and its .amdhsa descriptor,
with the basic-block labels (.LBB<f>_<n>) and the function-local symbols renumbered in order of appearance.  A kernel whose text differs
gets a second verdict, "same up to scheduling": the same .amdhsa descriptor, instruction count and opcode histogram, and the same
sequence of labels, memory instructions, barriers, waits and branches with register numbers blanked -- what is left to differ is the order
of independent ALU and move instructions, register numbers and the operand order of commutative operations.  It still counts as differing.
    python tools/isa_identity.py [BASE=HEAD]        exit status 0: every kernel identical"""
import collections
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from inst_flags import part_flags  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-Wall", "-Wno-unused-function"]
SIZES = (32, 64, 128, 256, 512, 1024, 2048, 4096)
# the add-on libraries: source without .hip, the Makefile's prefix, its lengths, whether the Makefile compiles it with -I.
ADDONS = (("smfft_large", "LARGE", (8192, 16384), False), ("smfft_large_real", "LARGE_REAL", (16384, 32768), False),
          ("smfft_large_fir", "LARGE_FIR", (8192, 16384), True), ("smfft_pfb", "PFB", (256, 512, 1024, 2048, 4096), True),
          ("smfft_pfb_real", "PFB_REAL", (256, 512, 1024, 2048, 4096), True), ("smfft_large_pfb", "LARGE_PFB", (8192, 16384), True),
          ("smfft_pfb_spec", "PFB_SPEC", (256, 512, 1024, 2048, 4096), True), ("smfft_fir_real", "FIR_REAL", (256, 512, 1024, 2048, 4096), True),
          ("smfft_fir_detect", "FIR_DETECT", (256, 512, 1024, 2048, 4096), True), ("smfft_bluestein", "BLUESTEIN", (256, 512, 1024, 2048, 4096), True),
          ("smfft_czt", "CZT", (256, 512, 1024, 2048, 4096), True), ("smfft_rowconv", "ROWCONV", (256, 512, 1024, 2048, 4096), True),
          ("smfft_rowconv_real", "ROWCONV_REAL", (256, 512, 1024, 2048, 4096), True), ("smfft_dct", "DCT", (256, 512, 1024, 2048, 4096), True),
          ("smfft_hilbert", "HILBERT", (256, 512, 1024, 2048, 4096), True), ("smfft_mdct", "MDCT", (256, 512, 1024, 2048, 4096), True),
          ("smfft_stft", "STFT", (256, 512, 1024, 2048, 4096), True), ("smfft_welch", "WELCH", (256, 512, 1024, 2048, 4096), True),
          ("smfft_bands", "BANDS", (256, 512, 1024, 2048, 4096), True))


def addon_flags(prefix, n):
    """the words of the line `<prefix>_FLAGS_<n> :=` of the working tree's Makefile"""
    for line in open(os.path.join(ROOT, "smfft_amd", "csrc", "Makefile")):
        m = re.match(rf"{prefix}_FLAGS_{n}\s*:=(.*)", line)
        if m:
            return m.group(1).split()
    raise SystemExit(f"{prefix}_FLAGS_{n} missing from the Makefile")


def units(tree):
    out = []
    for n in SIZES:
        for part in (1, 2):
            out.append((f"smfft_inst_{n}_part{part}", "smfft_amd/csrc/smfft_inst.hip", part_flags(n, part) + [f"-DSMFFT_N={n}"]))
    if os.path.exists(os.path.join(tree, "smfft_amd/csrc/smfft_fir.hip")):
        out.append(("smfft_fir", "smfft_amd/csrc/smfft_fir.hip", []))
    for stem, prefix, sizes, local in ADDONS:
        rel = f"smfft_amd/csrc/{stem}.hip"
        if os.path.exists(os.path.join(tree, rel)):
            for n in sizes:       # ("{tree}": compile_unit puts the tree it compiles there)
                out.append((f"{stem}_{n}", rel, (["-I{tree}/smfft_amd/csrc"] if local else []) + addon_flags(prefix, n) + [f"-DSMFFT_{prefix}_N={n}"]))
    for ex in sorted(os.listdir(os.path.join(tree, "examples"))):
        if ex.endswith(".hip"):
            out.append((ex, "examples/" + ex, []))
    return out


def compile_unit(tree, rel, extra, dst):
    cmd = [HIPCC] + FLAGS + ["-I" + os.path.join(tree, "include")] + [e.replace("{tree}", tree) for e in extra]
    cmd += ["-S", "--cuda-device-only", os.path.join(tree, rel), "-o", dst]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError(p.stderr[-3000:])
    return open(dst).read()


def kernels(asm):
    """{mangled name: normalised text of the function body + its kernel descriptor}"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*(?:;[^\n]*)?\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
        name, body = m.group(1), m.group(2)
        d = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), asm, re.S)
        out[name] = normalise(body + (d.group(1) if d else ""))
    return out


def normalise(text):
    seen = {}

    def label(m):
        return seen.setdefault(m.group(0), f".L{len(seen)}")
    text = re.sub(r"\.LBB\d+_\d+|\.Ltmp\d+|\.Lfunc_begin\d+|\.Lfunc_end\d+", label, text)
    lines = (re.sub(r"\s*;.*$", "", l).rstrip() for l in text.split("\n"))       # comments (they name blocks by number too)
    return "\n".join(l for l in lines if l.strip())


ORDERED = re.compile(r"(global_|ds_|buffer_|flat_|scratch_|s_load|s_buffer_load|s_barrier|s_waitcnt|s_cbranch|s_branch|s_setpc|s_endpgm|\.L\d+:)")


def same_up_to_scheduling(a, b):
    """the relaxed verdict on two normalised kernel texts: (True, "") or (False, what differs first)"""
    def parts(text):
        lines = [l.strip() for l in text.split("\n")]
        desc = [l for l in lines if l.startswith(".amdhsa_")]
        code = [l for l in lines if not l.startswith(".") or re.match(r"\.L\d+:", l)]
        insts = [l for l in code if not l.endswith(":")]
        ordered = [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", lambda m: m.group(1) + ("2+" if ":" in m.group(2) else ""), l) for l in code if ORDERED.match(l)]
        return desc, insts, collections.Counter(l.split()[0] for l in insts), ordered
    (da, ia, ha, oa), (db, ib, hb, ob) = parts(a), parts(b)
    if da != db:
        return False, "descriptor: " + "; ".join(f"{x} -> {y}" for x, y in zip(da, db) if x != y)
    if len(ia) != len(ib) or ha != hb:
        return False, f"{len(ia)} -> {len(ib)} instructions, opcodes " + ", ".join(f"{k} {ha[k]} -> {hb[k]}" for k in sorted(set(ha) | set(hb)) if ha[k] != hb[k])
    if oa != ob:
        i = next((i for i, (x, y) in enumerate(zip(oa, ob)) if x != y), min(len(oa), len(ob)))
        return False, f"ordered instruction {i}: {oa[i:i + 1]} -> {ob[i:i + 1]}"
    return True, ""


def main():
    base = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    with tempfile.TemporaryDirectory() as tmp:
        base_tree = os.path.join(tmp, "base")
        os.makedirs(base_tree)
        archive = subprocess.run(["git", "-C", ROOT, "archive", base], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", base_tree], input=archive, check=True)
        jobs = []
        for tag, tree in (("base", base_tree), ("tree", ROOT)):
            for name, rel, extra in units(base_tree):
                jobs.append((tag, name, tree, rel, extra, os.path.join(tmp, f"{tag}_{name}.s")))
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            asm = dict(zip([(j[0], j[1]) for j in jobs], ex.map(lambda j: compile_unit(*j[2:]), jobs)))
    total, differ = 0, []
    for name in sorted({j[1] for j in jobs}):
        a, b = kernels(asm[("base", name)]), kernels(asm[("tree", name)])
        for k, text in a.items():
            total += 1
            if k not in b:
                differ.append((name, k, "missing"))
            elif b[k] != text:
                same, what = same_up_to_scheduling(text, b[k])
                differ.append((name, k, "differs, same up to scheduling" if same else "differs (" + what + ")"))
        added = sorted(set(b) - set(a))
        print(f"{name:32s} {len(a):4d} kernels of {base}: {len(a) - sum(1 for d in differ if d[0] == name):4d} identical"
              + (f"; {len(added)} new" if added else ""))
    for name, k, why in differ:
        print(f"  {why}: {name} {k}")
    print(f"{total} kernels of {base} compared, {len(differ)} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
