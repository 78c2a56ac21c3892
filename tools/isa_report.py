#!/usr/bin/env python
"""ISA-level report of the HIP kernels (tuning aid, CPU only: hipcc cross-compiles gfx950).

    python tools/isa_report.py                      # registers / scratch / occupancy of every kernel
    python tools/isa_report.py --gaps k_sweep6ILi0ELi12ELi2   # instructions between consecutive MFMAs in its hot loop
    python tools/isa_report.py --json FILE          # per kernel: resources, instruction count, hashes of its code
    python tools/isa_report.py --compare A.json B.json   # two such files: identical / reordered / different, per kernel

Compiles ptq4vit_amd/csrc/p4v_api.hip with the flags of __graft_entry__.build() plus -save-temps into a scratch
directory and reads the generated assembly (--asm FILE reads one that exists already).  The "gaps" view is what DESIGN.md s5.1 argues with: a wave that is alone
on its SIMD hides about five single-issue instructions per 32x32x32 MFMA.

--json records numbers and hashes only: registers, scratch, occupancy, LDS bytes, the instruction count, a sha256 of the
instruction stream (comments dropped, basic-block labels renumbered per kernel), a sha256 of that stream sorted (equal
for two kernels that differ in instruction order only), and a sha256 of the opcode sequence of the MFMA-heaviest basic
block -- the block --gaps shows.  --compare classes every kernel as (I) identical stream, (R) same multiset of
instructions in another order, (D) different, and checks what a refactor of the kernels must keep: the same symbols, no
more scratch, no lower occupancy, the same LDS bytes, the same hot block.
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++20", "-fPIC", "-shared", "-Wno-unused-value",
         "-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize"]


def compile_asm(workdir):
    src = os.path.join(ROOT, "ptq4vit_amd", "csrc", "p4v_api.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + ["-save-temps=obj", src, "-o", os.path.join(workdir, "lib.so")]
    subprocess.run(cmd, cwd=workdir, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.join(workdir, "p4v_api-hip-amdgcn-amd-amdhsa-gfx950.s")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def resources(lines):
    res, name = {}, None
    for l in lines:
        m = re.match(r"^(_ZN3p4v\S+):", l)
        if m:
            name = m.group(1)
        m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", l)
        if m and name:
            res.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return res


def basic_blocks(body):
    """[(label, [instruction text])] of one kernel's lines; comments and directives dropped"""
    blocks, cur, label = [], [], "entry"
    for l in body:
        s = l.strip()
        if re.match(r"^\.LBB\d+_\d+:", s):
            blocks.append((label, cur))
            cur, label = [], s.split(":")[0]
            continue
        if not s or s[0] in ";.":
            continue
        cur.append(" ".join(s.split(";")[0].split()))
    blocks.append((label, cur))
    return blocks


def hot_block(blocks):
    """(label, opcodes) of the basic block with the most MFMAs"""
    label, seq = max(blocks, key=lambda b: sum("mfma" in i.split()[0] for i in b[1]))
    return label, [i.split()[0] for i in seq]


def kernel_bodies(lines):
    """mangled name -> the lines between its label and its .Lfunc_end"""
    out, name, start = {}, None, 0
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN3p4v\S+):", l)
        if m:
            name, start = m.group(1), i + 1
        elif name and l.startswith(".Lfunc_end"):
            out[name], name = lines[start:i], None
    return out


def fingerprints(lines):
    """demangled name -> resources, LDS bytes, instruction count and the three hashes (see the module docstring)"""
    res, extra, name = resources(lines), {}, None
    for l in lines:
        m = re.match(r"^(_ZN3p4v\S+):", l)
        if m:
            name = m.group(1)
        m = re.match(r"^; (TotalNumSgprs|LDSByteSize): (\d+)", l)
        if m and name:
            extra.setdefault(name, {})[m.group(1)] = int(m.group(2))
    sha = lambda seq: hashlib.sha256("\n".join(seq).encode()).hexdigest()[:8]      # compared kernel by kernel only
    out = {}
    bodies = kernel_bodies(lines)
    names = demangle(list(res))
    for k, r in res.items():
        blocks = basic_blocks(bodies[k])
        stream = [re.sub(r"\.LBB\d+_", ".LBB_", i) for _, b in blocks for i in b]
        hot = hot_block(blocks)[1]
        out[names[k]] = {"vgpr": r.get("NumVgprs", 0), "agpr": r.get("NumAgprs", 0), "sgpr": extra.get(k, {}).get("TotalNumSgprs", 0),
                         "scratch": r.get("ScratchSize", 0), "occupancy": r.get("Occupancy", 0), "lds": extra.get(k, {}).get("LDSByteSize", 0),
                         "instructions": len(stream), "stream": sha(stream), "multiset": sha(sorted(stream)),
                         "hot_block": sha(hot), "hot_block_len": len(hot)}
    return out


FIELDS = ("vgpr", "agpr", "sgpr", "scratch", "occupancy", "lds", "instructions", "hot_block_len", "stream", "multiset", "hot_block")


def dump(prints, path):
    """one kernel per line, its FIELDS as a list; "p4v::", the return type and -- where the names stay distinct -- the argument
    lists are dropped from the demangled names"""
    short = {k: re.sub(r"\(.*\)$", "", k.replace("void ", "").replace("p4v::", "")) for k in prints}
    if len(set(short.values())) < len(short):
        short = {k: k.replace("p4v::", "") for k in prints}
    rows = [" %s: %s" % (json.dumps(short[k]), json.dumps([v[f] for f in FIELDS], separators=(",", ":"))) for k, v in sorted(prints.items())]
    with open(path, "w") as fh:
        fh.write('{"fields": %s, "kernels": {\n%s\n}}\n' % (json.dumps(list(FIELDS)), ",\n".join(rows)))


def load(path):
    doc = json.load(open(path))
    return {k: dict(zip(doc["fields"], v)) for k, v in doc["kernels"].items()}


def compare(a, b):
    """prints the classes of two --json files; returns the number of kernels that break what a refactor must keep"""
    row = lambda r: "vgpr %d agpr %d sgpr %d scratch %d occ %d lds %d" % tuple(r[k] for k in ("vgpr", "agpr", "sgpr", "scratch", "occupancy", "lds"))
    bad = 0
    if sorted(a) != sorted(b):
        bad += 1
        print("symbols differ: only in A", sorted(set(a) - set(b)), "only in B", sorted(set(b) - set(a)))
    cls = {"I": [], "R": [], "D": []}
    for k in sorted(set(a) & set(b)):
        x, y = a[k], b[k]
        cls["I" if x["stream"] == y["stream"] else "R" if x["multiset"] == y["multiset"] else "D"].append(k)
        broken = [what for what, ok in (("scratch grew", y["scratch"] <= x["scratch"]), ("occupancy fell", y["occupancy"] >= x["occupancy"]),
                                        ("LDS bytes differ", y["lds"] == x["lds"]), ("hot block differs", y["hot_block"] == x["hot_block"])) if not ok]
        if broken:
            bad += 1
            print(f"BROKEN {k}: {', '.join(broken)} (hot block {x['hot_block_len']} -> {y['hot_block_len']} opcodes)\n   A: {row(x)}\n   B: {row(y)}")
    for k in cls["D"]:
        x, y = a[k], b[k]
        print(f"(D) {k}: {x['instructions']} -> {y['instructions']} instructions, hot block {'equal' if x['hot_block'] == y['hot_block'] else 'DIFFERS'}"
              f"\n   A: {row(x)}\n   B: {row(y)}")
    for k in cls["R"]:
        print(f"(R) {k}: {a[k]['instructions']} instructions, hot block {'equal' if a[k]['hot_block'] == b[k]['hot_block'] else 'DIFFERS'}")
    print(f"{len(set(a) & set(b))} kernels: (I) {len(cls['I'])} identical, (R) {len(cls['R'])} reordered, (D) {len(cls['D'])} different; {bad} broken")
    return bad


def gaps(lines, sym):
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN3p4v") and sym in l and l.rstrip().endswith(":") is False and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    label, seq = hot_block(basic_blocks(lines[start:end]))
    g, run = [], 0
    for o in seq:
        if "mfma" in o:
            g.append(run)
            run = 0
        else:
            run += 1
    g.append(run)
    n = sum("mfma" in o for o in seq)
    print(f"{label}: {len(seq)} instructions, {n} MFMAs, {(len(seq) - n) / max(1, n):.2f} others per MFMA")
    print("instructions between consecutive MFMAs:", g)
    mix = {}
    for o in seq:
        mix[o] = mix.get(o, 0) + 1
    print("mix:", sorted(mix.items(), key=lambda kv: -kv[1])[:14])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaps", metavar="SUBSTR", help="mangled-name substring of one kernel, e.g. k_sweep6ILi0ELi12ELi2")
    ap.add_argument("--json", metavar="FILE", help="write every kernel's resources, instruction count and code hashes")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"), help="class every kernel of two --json files")
    ap.add_argument("--asm", metavar="FILE", help="read this gfx950 assembly instead of compiling")
    a = ap.parse_args()
    if a.compare:
        return 1 if compare(*(load(f) for f in a.compare)) else 0
    if a.asm:
        lines = open(a.asm).read().split("\n")
    else:
        with tempfile.TemporaryDirectory() as d:
            lines = open(compile_asm(d)).read().split("\n")
    if a.json:
        dump(fingerprints(lines), a.json)
        return
    if a.gaps:
        gaps(lines, a.gaps)
        return
    res = resources(lines)
    names = demangle(list(res))
    print(f"{'kernel':72s} {'VGPR':>5s} {'AGPR':>5s} {'scratch':>8s} {'waves/SIMD':>10s}")
    for k, r in res.items():
        flag = "  <-- scratch" if r.get("ScratchSize", 0) else ""
        print(f"{names[k][:72]:72s} {r.get('NumVgprs', 0):5d} {r.get('NumAgprs', 0):5d} {r.get('ScratchSize', 0):8d} {r.get('Occupancy', 0):10d}{flag}")


if __name__ == "__main__":
    sys.exit(main())
