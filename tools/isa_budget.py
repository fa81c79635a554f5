"""Register budgets of every kernel of two builds of the library, side by side.

    python tools/isa_budget.py <build dir before> <build dir after>

The arguments are object directories of csrc/Makefile (B=...; default
csrc/build).  For every gfx950 kernel in objects of the same name: VGPRs in
all (of which AGPRs), spilled VGPR + SGPR dwords and waves per SIMD (512
registers per SIMD lane, allocated in blocks of 8), before | after, read from
the code objects' metadata (no GPU).  A kernel that spills more VGPRs or holds
fewer waves is marked, and the exit status is 1 if there is one: the check
behind deep_stats_transposed (csrc/conv_deep.h) and profiles/stat_tail_isa.txt."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def meta(build, name, tmp):
    """{kernel: metadata fields} of build/name.o (None: no device code)"""
    fb, co = os.path.join(tmp, name + ".fatbin"), os.path.join(tmp, name + ".co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", os.path.join(build, name + ".o"), fb],
                   check=True)
    r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fb,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], capture_output=True)
    if r.returncode != 0:
        return None
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                         text=True).stdout
    out, cur = {}, {}
    for line in txt.splitlines():
        m = re.match(r"\s*(?:- )?\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "agpr_count" and cur.get("name"):      # the first field of the next kernel
            out[cur["name"]] = cur
            cur = {}
        cur[k] = v
    if cur.get("name"):
        out[cur["name"]] = cur
    return out


def waves(d):
    tot = (int(d["vgpr_count"]) + 7) // 8 * 8
    return min(8, 512 // max(tot, 8))


def main(before, after):
    objs = sorted(x[:-2] for x in os.listdir(after) if x.endswith(".o") and os.path.exists(os.path.join(before, x)))
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for n in objs:
            os.makedirs(os.path.join(tmp, "a"), exist_ok=True)
            os.makedirs(os.path.join(tmp, "b"), exist_ok=True)
            a, b = meta(before, n, os.path.join(tmp, "a")), meta(after, n, os.path.join(tmp, "b"))
            if a is None or b is None:
                continue
            rows += [(n, k, a[k], b[k]) for k in a if k in b]
    names = subprocess.run(["c++filt"], input="\n".join(r[1] for r in rows), capture_output=True,
                           text=True).stdout.splitlines()
    fmt = lambda q: "%4s(%3s) %3s+%3s  %d" % (q["vgpr_count"], q["agpr_count"], q["vgpr_spill_count"],  # noqa: E731
                                              q["sgpr_spill_count"], waves(q))
    print("kernel | before: vgpr(agpr) spilled vgpr+sgpr waves | after | note")
    bad = 0
    for (n, _, x, y), dn in zip(rows, names):
        dn = re.sub(r"\(.*\)$", "", dn.replace("(anonymous namespace)::", "").replace("void ", ""))
        note = []
        if waves(y) < waves(x):
            note.append("LOSES A WAVE")
        if int(y["vgpr_spill_count"]) > int(x["vgpr_spill_count"]):
            note.append("VGPR SPILLS")
        if waves(y) > waves(x):
            note.append("gains a wave")
        bad += bool(note) and note != ["gains a wave"]
        print("%s: %s | %s | %s | %s" % (n, dn, fmt(x), fmt(y), " ".join(note)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
