"""Register, scratch and scalar-load figures of k_direct's MANY instantiations next to the UNTIL ones of the same XG / KINDS
(NOTES.md section 51; profiles/direct_many_resources.txt is this script's output).

    hipcc -O3 -std=c++17 -fPIC -I../../include --offload-arch=gfx950 -fno-gpu-rdc --save-temps -c -o sgo_direct.o sgo_direct.hip
    python scripts/direct_many_resources.py sgo_direct-hip-amdgcn-amd-amdhsa-gfx950.s

Per kernel: the compiler's own resource summary, the scalar and the vector loads from global memory in the prologue (everything
before the first LDS or barrier instruction: where the MANY instantiations read their job record), and whether the MANY row stays
within the UNTIL row (no more VGPRs, no more scratch).  Exit code 1 when one does not.  Needs c++filt on the PATH; no GPU."""
import re
import subprocess
import sys

KEYS = ["NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "Occupancy"]


def kernels(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r"\n(_ZN3sgo\S*k_direct\S*):[^\n]*\n(.*?)\n; Kernel info:(.*?)\n\t\.(?:section|text)", s, re.S):
        name, code, info = m.groups()
        dm = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout
        a = [{"true": "1", "false": "0"}.get(x.strip(), x.strip()) for x in re.search(r"k_direct<([^>]*)>", dm).group(1).split(",")]
        a += ["0"] * (6 - len(a))
        row = {k: int(re.search(k + r": (\d+)", info).group(1)) for k in KEYS}
        pro = re.split(r"\n\t(?:ds_|s_barrier)", code, 1)[0]
        row["prologue s_load"] = len(re.findall(r"\n\ts_load_dword", pro))
        row["prologue global_load"] = len(re.findall(r"\n\t(?:global|flat)_load", pro))
        out[tuple(a)] = row
    return out


def main(path):
    K = kernels(path)
    cols = KEYS + ["prologue s_load", "prologue global_load"]
    print("# k_direct<XG, KINDS, UNTIL, BATCH, DUMP, MANY>: the UNTIL row, then the MANY row of the same XG / KINDS")
    print("# " + "  ".join(cols))
    ok = True
    for xg in "01":
        for kinds in "01":
            u, m = K[(xg, kinds, "1", "0", "0", "0")], K[(xg, kinds, "1", "0", "0", "1")]
            for tag, r in (("UNTIL", u), ("MANY ", m)):
                print(f"k_direct<XG={xg},KINDS={kinds}> {tag}  " + "  ".join(f"{c.split()[-1]} {r[c]}" for c in cols))
            fits = m["NumVgprs"] <= u["NumVgprs"] and m["NumAgprs"] <= u["NumAgprs"] and m["ScratchSize"] <= u["ScratchSize"]
            print(f"    MANY within UNTIL (VGPRs, AGPRs, scratch): {'yes' if fits else 'NO'}")
            ok = ok and fits
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
