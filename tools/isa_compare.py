#!/usr/bin/env python3
"""Compare the gfx950 device assembly of .hip files between two source trees.

    tools/isa_compare.py PARENT_TREE THIS_TREE [file.hip ...] [--md]

Each file is compiled in <tree>/mri-to-speech_amd/csrc with that tree's Makefile flags for the file (NOSLP files get
-fno-slp-vectorize) plus --cuda-device-only -S.  Per kernel symbol it prints `identical`, `same instructions`
(equal opcode multiset; the lines that moved or changed operands are listed) or `different` (the opcode counts that
changed), the s_waitcnt order, and the resource counts of the code-object metadata.  Symbol names that differ between
trees only by design (the zero page, the per-TU __hip_cuid_*) are normalised first.  A host-side tool: it needs hipcc
and no GPU.
"""
import collections, difflib, os, re, subprocess, sys, tempfile

CSRC = "mri-to-speech_amd/csrc"
DEFAULT = ("conv_gemm conv_halo gemm128 mrf_fused er_fused er2_fused ers2_fused er_sp_fused er8_fused er8w_fused "
           "ir_ws se_ws conv1d_halo dwse kernels lstm_persistent lstm_window").split()
RES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
       ".vgpr_spill_count", ".sgpr_spill_count")


def make_var(text, name):
    m = re.search(r"^%s\s*=\s*(.*)$" % name, text, re.M)
    return m.group(1).split() if m else []


def compile_asm(tree, hip, out):
    d = os.path.join(tree, CSRC)
    mk = open(os.path.join(d, "Makefile")).read()
    flags = [f.replace("$(ARCH)", "gfx950") for f in make_var(mk, "FLAGS") if f != "$(EXTRA)"]
    if hip in make_var(mk, "NOSLP"):
        flags.append("-fno-slp-vectorize")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", hip, "-o", out], cwd=d, check=True,
                   stderr=subprocess.DEVNULL)
    s = open(out).read()
    s = re.sub(r"_ZN3m2s\w*?\d+g_\w*zero\w*?E", "ZERO_PAGE", s)
    return re.sub(r"__hip_cuid_\w+", "__hip_cuid", s)


def kernels(asm):
    """{symbol: (body lines, {resource: value})} of every kernel in one assembly file."""
    meta = {}
    for block in re.split(r"\n  - \.agpr_count:", asm.split(".amdgpu_metadata")[-1])[1:]:
        block = "    .agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in RES}
    out = {}
    for name, res in meta.items():
        body = re.search(r"^%s:.*?\n(.*?)^\s*\.section\s+\.rodata" % re.escape(name), asm, re.M | re.S).group(1)
        lines = [l.split(";")[0].strip() for l in body.splitlines()]
        out[name] = ([l for l in lines if l], res)
    return out


def opcode(line):
    return line.split()[0]


def compare(a, b):
    if a == b:
        return "identical", []
    ca = collections.Counter(opcode(l) for l in a if not l.endswith(":"))
    cb = collections.Counter(opcode(l) for l in b if not l.endswith(":"))
    if ca != cb:
        return "different", ["%s %d -> %d" % (k, ca[k], cb[k]) for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]]
    moved = [l for l in difflib.unified_diff(a, b, "parent", "this", n=0, lineterm="") if l[0] in "+-" and l[:3] not in ("+++", "---")]
    return "same instructions", moved


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    md = "--md" in sys.argv
    if len(args) < 2:
        sys.exit(__doc__)
    parent, this = args[0], args[1]
    files = [f if f.endswith(".hip") else f + ".hip" for f in (args[2:] or DEFAULT)]
    worst = 0
    with tempfile.TemporaryDirectory() as tmp:
        for hip in files:
            ka = kernels(compile_asm(parent, hip, os.path.join(tmp, "a.s")))
            kb = kernels(compile_asm(this, hip, os.path.join(tmp, "b.s")))
            for name in sorted(set(ka) | set(kb)):
                if name not in ka or name not in kb:
                    print("%s %s: only in %s" % (hip, name, "parent" if name in ka else "this tree"))
                    worst = 2
                    continue
                (la, ra), (lb, rb) = ka[name], kb[name]
                verdict, detail = compare(la, lb)
                waits = [l for l in la if l.startswith("s_waitcnt")] == [l for l in lb if l.startswith("s_waitcnt")]
                res = " ".join("%s=%d" % (k.strip(".").replace("_count", "").replace("_segment_fixed_size", ""), rb[k]) for k in RES)
                if ra != rb:
                    res += "  (parent: " + " ".join("%s=%d" % (k, ra[k]) for k in RES if ra[k] != rb[k]) + ")"
                short = subprocess.run(["c++filt", "-p", name], capture_output=True, text=True).stdout.strip() or name
                short = short.replace("m2s::(anonymous namespace)::", "").replace("m2s::", "")
                if md:
                    print("| `%s` | `%s` | %s | %s |" % (hip, short, verdict, res))
                else:
                    print("%-18s %-60s %-18s %s%s" % (hip, short, verdict, res, "" if waits else "  s_waitcnt order differs"))
                    for d in detail:
                        print("      " + d)
                worst = max(worst, 0 if verdict == "identical" else 1 if ra == rb and waits and verdict[0] == "s" else 2)
    sys.exit(worst)


if __name__ == "__main__":
    main()
