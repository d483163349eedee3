#!/usr/bin/env python3
"""Which kernels get their leading arguments preloaded into SGPRs, and how many dwords of them.

Compiles the kernel sources of sparse_gslam_amd/csrc to assembly with the Makefile's own command line (make -n, with
-c replaced by -S --cuda-device-only) and prints, per kernel, the value of .amdhsa_user_sgpr_kernarg_preload_length in its
descriptor block: 0 = the kernel waits for the load of its arguments, n = the first n dwords of the argument block arrive
in user SGPRs before the first wave starts.  A by-value struct in front of the pointers a kernel reads first gives 0
(DESIGN.md section 4).  Runs on the CPU; the output is kept as profiles/kernarg_preload.txt:
    python scripts/kernarg_preload_report.py > profiles/kernarg_preload.txt
so that a reordering of a parameter list that loses the preload shows up in a diff."""
import os
import re
import shlex
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparse_gslam_amd", "csrc")
SOURCES = sys.argv[1:] or ["sgo_kernels", "sgo_amg", "sgo_mfront"]


def compile_line(stem):
    """the Makefile's recipe for stem.o as an argument list that writes device assembly to stdout"""
    out = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, stem + ".o"], text=True)
    line = next(ln for ln in out.splitlines() if stem + ".hip" in ln and " -c " in ln)
    args = shlex.split(line)
    k = args.index("-o")
    del args[k:k + 2]
    args[args.index("-c")] = "-S"
    return args + ["--cuda-device-only", "-o", "-"]


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    for cand in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"):
        if tool is None and os.path.exists(cand):
            tool = cand
    if tool is None or not names:
        return list(names)
    return subprocess.check_output([tool], input="\n".join(names) + "\n", text=True).splitlines()


def short(name):
    """k_spmv<2>(BsrDev, SpmvArgs) without the 'void ' and with the parameter list kept: it is what decides the preload"""
    return re.sub(r"^void ", "", name).replace("sgo::(anonymous namespace)::", "").replace("sgo::", "")


for stem in SOURCES:
    asm = subprocess.check_output(compile_line(stem), cwd=CSRC, text=True, stderr=subprocess.DEVNULL)
    rows, cur = [], None
    for ln in asm.splitlines():
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", ln)
        if m and cur is not None:
            rows.append((cur, int(m.group(1))))
            cur = None
    names = demangle([r[0] for r in rows])
    print(f"# {stem}.hip: {sum(1 for r in rows if r[1])} of {len(rows)} kernels preloaded")
    for name, (_, n) in sorted(zip(names, rows), key=lambda t: short(t[0])):
        print(f"{n:2d}  {short(name)}")
