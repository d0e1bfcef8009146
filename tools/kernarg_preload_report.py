#!/usr/bin/env python3
"""How many kernel-argument dwords each kernel receives in preloaded SGPRs (no GPU needed).

    python tools/kernarg_preload_report.py conv_cb.hip [conv_gemm_rs.hip ...]      (names relative to syncfusion_amd/csrc, or paths)

Compiles each source to gfx950 assembly with the Makefile's HIPCC / CXXFLAGS into a temporary directory and prints, per `.amdhsa_kernel`,
the two metadata values `.amdhsa_user_sgpr_count` and `.amdhsa_user_sgpr_kernarg_preload_length`:

    <file> <TAB> <user SGPRs> <TAB> <preloaded dwords> <TAB> <demangled kernel name>

The kernarg segment pointer takes two of the 16 user SGPRs, so at most 14 dwords are preloaded; the compiler preloads LEADING scalar and
pointer parameters only and stops at the first by-value struct (syncfusion_amd/csrc/Makefile).  The tool reads these
two metadata lines and nothing else of the assembly.

    python tools/kernarg_preload_report.py --resources conv_gemm_sk.hip [...]

prints instead, from the same `.amdhsa_` block and the compiler's comments behind it, what a refactor of a kernel must not move:

    <file> <TAB> next_free_vgpr <TAB> accum_offset <TAB> next_free_sgpr <TAB> private_segment_fixed_size (scratch) <TAB>
    group_segment_fixed_size (static LDS) <TAB> occupancy (waves per SIMD) <TAB> code bytes <TAB> <demangled kernel name>

Compare two trees with `diff` on the two outputs (profiles/gemm_epilogue_resources.txt)."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "syncfusion_amd", "csrc")


def makefile_vars():
    """HIPCC, ARCH and CXXFLAGS as the Makefile defines them (environment overrides for the `?=` ones, as in make)."""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    v = {}
    for name in ("HIPCC", "ARCH", "CXXFLAGS"):
        m = re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, re.M)
        v[name] = m.group(1).strip()
    for name in ("HIPCC", "ARCH"):
        v[name] = os.environ.get(name, v[name])
    flags = v["CXXFLAGS"].replace("$(ARCH)", v["ARCH"]).split()
    return v["HIPCC"], flags


def demangle(names):
    tool = next((t for t in ("/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt")) if t and os.path.exists(t)), None)
    if not tool or not names:
        return list(names)
    # an older c++filt does not know the 16-bit float manglings: DF16_ -> Dh (half); DF16b -> t (unsigned short, no kernel here takes one), renamed back
    subst = [n.replace("DF16_", "Dh").replace("DF16b", "t") for n in names]
    out = subprocess.run([tool], input="\n".join(subst) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    out = [o.replace("unsigned short", "bf16") for o in out]
    return out if len(out) == len(names) else list(names)


RES_KEYS = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def report(source, resources=False):
    """[(kernel name, user SGPR count, preload length)] of one .hip source, in the order of the assembly; resources: [(kernel name, the five
    RES_KEYS values, occupancy, code bytes)]."""
    hipcc, flags = makefile_vars()
    path = source if os.path.exists(source) else os.path.join(CSRC, source)
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "device.s")
        subprocess.run([hipcc] + flags + ["-I", CSRC, "--cuda-device-only", "-S", path, "-o", asm], check=True, cwd=tmp)
        rows, cur, res, last = [], None, {}, None
        for line in open(asm):
            w = line.split()
            if not w:
                continue
            if w[0] == ";" and len(w) >= 3 and w[1] in ("Occupancy:", "codeLenInByte") and last:   # the compiler's summary behind the kernel's .amdhsa_ block
                res[last][w[1].rstrip(":")] = int(w[-1])
            elif cur is not None and w[0].startswith(".amdhsa_") and w[0][8:] in RES_KEYS:
                res[cur[0]][w[0][8:]] = int(w[1])
            if w[0] == ".amdhsa_kernel":
                cur = [w[1], 0, 0]
                res[w[1]] = {}
                last = w[1]
            elif cur is not None and w[0] == ".amdhsa_user_sgpr_count":
                cur[1] = int(w[1])
            elif cur is not None and w[0] == ".amdhsa_user_sgpr_kernarg_preload_length":
                cur[2] = int(w[1])
            elif cur is not None and w[0] == ".end_amdhsa_kernel":
                rows.append(cur)
                cur = None
    names = demangle([r[0] for r in rows])
    if resources:
        return [(n,) + tuple(res[r[0]].get(k, -1) for k in RES_KEYS + ("Occupancy", "codeLenInByte")) for n, r in zip(names, rows)]
    return [(n, r[1], r[2]) for n, r in zip(names, rows)]


def main(argv):
    if not argv:
        print(__doc__)
        return 2
    resources = argv[0] == "--resources"
    for src in argv[resources:]:
        for row in report(src, resources):
            print("\t".join([os.path.basename(src)] + [str(v) for v in row[1:]] + [row[0]]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
