"""Per-kernel comparison of the gfx950 code of two builds of some HIP sources (a refactor's proof
that kernels it did not mean to change did not change).

Each side is one or more device assembly files, made with the library's flags plus
`-S --cuda-device-only`:
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-gpu-rdc \
        -S --cuda-device-only marl_sap_amd/csrc/asg_env.hip -o new_env.s
(the parent's from `git archive REV marl_sap_amd include` unpacked elsewhere), then
    python tools/kernel_code_diff.py parent_env.s -- new_env.s new_env_mt.s

A kernel's code is the text between its `<symbol>:` label and its `.Lfunc_end` label, comments
stripped.  Local labels carry the function's index within its file (`.LBB12_3`), which moves when
functions are added, removed or moved to another unit, so the index is dropped before comparing;
nothing else is normalised: "identical" means the same instructions, registers, operands and
order.  Kernels are matched by demangled name (c++filt), so one that moved between files or lost
a parameter still pairs up when its name is the same, and shows as removed / added otherwise.
"""
import re
import subprocess
import sys


def kernels(paths):
    out = {}
    for path in paths:
        lines = open(path).read().split("\n")
        names = {m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))}
        cur, body = None, []
        for l in lines:
            m = re.match(r"(\S+):", l)
            if cur is None:
                if m and m.group(1) in names:
                    cur, body = m.group(1), []
                continue
            if l.startswith(".Lfunc_end"):
                out[cur] = body
                cur = None
                continue
            l = re.sub(r"\s*;.*", "", l)
            l = re.sub(r"\.L(BB|tmp|JTI)\d+_", r".L\1_", l)
            if l.strip():
                body.append(l)
    dem = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True).stdout.split("\n")
    return {d: out[k] for k, d in zip(out, dem)}


def mnemonics(body):
    return sorted(l.split()[0] for l in body)


if __name__ == "__main__":
    sep = sys.argv.index("--")
    a, b = kernels(sys.argv[1:sep]), kernels(sys.argv[sep + 1:])
    same = [k for k in a if k in b and a[k] == b[k]]
    print(f"{len(a)} -> {len(b)} kernels, {len(same)} identical")
    for k in sorted(set(a) | set(b)):
        if k in same:
            continue
        if k not in b:
            print("removed  ", k)
        elif k not in a:
            print("added    ", k)
        else:
            how = "scheduling / registers only" if mnemonics(a[k]) == mnemonics(b[k]) else "instructions differ"
            print(f"differs   {k}: {len(a[k])} -> {len(b[k])} lines, {how}")
