"""Register, scratch and LDS figures of every k_direct instantiation of two builds side by side (NOTES.md section 39).

    hipcc -O3 -std=c++17 -fPIC -I../../include --offload-arch=gfx950 -fno-gpu-rdc -Rpass-analysis=kernel-resource-usage \
          -c -o /dev/null sgo_direct.hip 2> remarks.txt          (in sparse_gslam_amd/csrc of each tree)
    python scripts/direct_resources.py parent/remarks.txt this/remarks.txt

Prints a markdown table (parent / this per figure) and EQUAL when every kernel both builds have reports the same figures.
Needs c++filt on the PATH; no GPU."""
import re
import subprocess
import sys

KEYS = ["VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
        "Occupancy [waves/SIMD]"]


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: (.*)", line)
        if not m:
            continue
        t = m.group(1).strip()
        fn = re.match(r"Function Name: (\S+)", t)
        if fn:
            cur = subprocess.run(["c++filt", fn.group(1)], capture_output=True, text=True).stdout.strip()
            cur = re.sub(r"\(.*", "", re.sub(r"^void sgo::\(anonymous namespace\)::", "", cur))
            out[cur] = {}
        elif cur:
            k, _, v = t.partition(":")
            out[cur][k.strip()] = v.split("[-R")[0].strip()
    return out


def norm(name):
    """k_direct<a, b, ...> with the defaulted template arguments written out."""
    m = re.match(r"k_direct<(.*)>", name)
    if not m:
        return name
    a = [{"true": "1", "false": "0"}.get(x.strip(), x.strip()) for x in m.group(1).split(",")]
    a += ["0"] * (5 - len(a))
    return "k_direct<XG=%s,KINDS=%s,UNTIL=%s,BATCH=%s,DUMP=%s>" % tuple(a)


def main(parent, this):
    P = {norm(k): v for k, v in parse(parent).items()}
    N = {norm(k): v for k, v in parse(this).items()}
    print("| kernel | " + " | ".join(k.split(" [")[0] for k in KEYS) + " |")
    print("|---|" + "---|" * len(KEYS))
    same = all(k in N for k in P)
    for k in N:
        row = []
        for q in KEYS:
            a, b = P.get(k, {}).get(q, "-"), N[k].get(q, "-")
            row.append(f"{a} / {b}")
            same = same and (k not in P or a == b)
        print(f"| `{k}` | " + " | ".join(row) + " |")
    print("EQUAL" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
