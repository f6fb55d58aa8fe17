"""What the compiler made of kernel files, per kernel, without a GPU: registers, LDS, scratch,
occupancy, the number of instructions and a hash of the instruction stream.

Each file is compiled for the device alone with the build script's flags (the files of
``_NO_PACKED_FP32_FILES`` with theirs) to assembly.  Per kernel the assembler's own figures
(NumVgprs, NumAgprs, TotalNumSgprs, ScratchSize, LDSByteSize, Occupancy) are printed with the
instruction count and the first 16 hex digits of a SHA-256 over the instructions, after comments
and directives are dropped and symbol and label names are replaced by their order of appearance:
two builds of a kernel with the same hash execute the same instructions on the same registers.

With ``--vs CSRC`` the same files of a second source tree (its ``csrc`` directory) are compiled
too; each kernel gets a row per tree, and a kernel whose stream differs gets a line that says how
(register allocation only, order only, or the opcode counts that differ).

Usage: python tools/kernel_isa.py FILE.hip ... [--csrc DIR] [--vs OTHER_CSRC] [--out FILE]
"""
from __future__ import annotations

import argparse
import collections
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

_FIGURES = {"NumVgprs": "vgprs", "NumAgprs": "agprs", "TotalNumSgprs": "sgprs",
            "ScratchSize": "scratch", "LDSByteSize": "lds", "Occupancy": "occ"}


def assembly(csrc: str, name: str) -> str:
    """Device assembly of csrc/kernels/<name>, compiled as the build compiles it."""
    from tools.build_ext import ARCH, HIPCC, _NO_PACKED_FP32, _NO_PACKED_FP32_FILES
    extra = _NO_PACKED_FP32 if name in _NO_PACKED_FP32_FILES else []
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        r = subprocess.run(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", f"-I{csrc}", "-DNDEBUG", "-Wno-unused-result",
             f"--offload-arch={ARCH}", "-munsafe-fp-atomics", *extra, "--cuda-device-only", "-S",
             os.path.join(csrc, "kernels", name), "-o", out],
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"compiling {name} of {csrc} failed:\n{r.stdout}")
        with open(out) as f:
            return f.read()


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if filt is None:
        return dict(zip(names, names))
    r = subprocess.run([filt], input="\n".join(names), stdout=subprocess.PIPE, text=True,
                       check=True)
    short = [re.sub(r"\(.*\)$", "", re.sub(r"^void ", "", s)).split("::")[-1]
             for s in r.stdout.splitlines()]
    return dict(zip(names, short))


def kernels(asm: str) -> dict:
    """{mangled name: {figures..., instrs, code, ops (opcode list), norm (normalised lines)}}"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, cur, lines = {}, None, None
    for raw in asm.splitlines():
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", raw)
        if m and m.group(1) in names:
            cur, lines = m.group(1), []
            out[cur] = {"lines": lines}
            continue
        if cur is None:
            continue
        if lines is not None:
            if re.match(r"^\s*\.amdhsa_kernel\b", raw) or re.match(r"^\.Lfunc_end", raw):
                lines = None  # the body is over; the figures follow as comments
                continue
            s = raw.split(";", 1)[0].strip()
            if not s or (s.startswith(".") and not s.endswith(":")):
                continue
            lines.append(s)
            continue
        m = re.match(r"^;\s*(\w+):\s*(\d+)\b", raw)
        if m and m.group(1) in _FIGURES:
            out[cur][_FIGURES[m.group(1)]] = int(m.group(2))
    for rec in out.values():
        labels, syms, norm, ops = {}, {}, [], []

        def lab(m):
            return labels.setdefault(m.group(0), f"L{len(labels)}")

        def sym(m):
            return syms.setdefault(m.group(0), f"S{len(syms)}")

        for s in rec.pop("lines"):
            s = re.sub(r"\.L[\w.$]+", lab, s)
            s = re.sub(r"\b_Z\w+", sym, s)
            s = re.sub(r"\s+", " ", s)
            norm.append(s)
            if not s.endswith(":"):
                ops.append(s.split(" ", 1)[0])
        rec["norm"], rec["ops"], rec["instrs"] = norm, ops, len(ops)
        rec["code"] = hashlib.sha256("\n".join(norm).encode()).hexdigest()[:16]
    return out


def difference(a: dict, b: dict) -> str:
    if a["ops"] == b["ops"]:
        return "same opcode sequence, operands differ"
    ca, cb = collections.Counter(a["ops"]), collections.Counter(b["ops"])
    if ca == cb:
        return "same opcodes, scheduled in another order"
    d = [f"{op} {cb[op] - ca[op]:+d}" for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]]
    return "opcode counts differ: " + ", ".join(d)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("files", nargs="+", help="kernel files, by name (csrc/kernels/NAME)")
    ap.add_argument("--csrc", default=os.path.join(REPO, "csrc"))
    ap.add_argument("--vs", default="", help="csrc directory of a second tree to compare with")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    trees = ([("parent", a.vs)] if a.vs else []) + [("new" if a.vs else "", a.csrc)]
    rows = [f"{'kernel':<34}{'tree':<8}{'VGPR':>5}{'AGPR':>5}{'SGPR':>5}{'scratch':>8}{'LDS':>7}"
            f"{'occ':>4}{'instrs':>7}  code"]
    notes, same, total = [], 0, 0
    for name in a.files:
        name = os.path.basename(name)
        per_tree = [(tag, kernels(assembly(csrc, name))) for tag, csrc in trees]
        short = demangle(sorted({k for _, ks in per_tree for k in ks}))
        # a kernel is matched across the trees by its demangled short name (argument types may move)
        by_short = collections.defaultdict(dict)
        for tag, ks in per_tree:
            for k, rec in ks.items():
                by_short[short[k]][tag] = rec
        for kname in sorted(by_short):
            recs = by_short[kname]
            for tag, _ in trees:
                r = recs.get(tag)
                if r is None:
                    rows.append(f"{kname:<34}{tag:<8}  (no such kernel)")
                    continue
                rows.append(f"{kname:<34}{tag:<8}{r['vgprs']:>5}{r.get('agprs', 0):>5}"
                            f"{r['sgprs']:>5}{r['scratch']:>8}{r['lds']:>7}{r['occ']:>4}"
                            f"{r['instrs']:>7}  {r['code']}")
            if a.vs and len(recs) == 2:
                total += 1
                if recs["parent"]["code"] == recs["new"]["code"]:
                    same += 1
                else:
                    notes.append(f"  differs: {kname:<32} "
                                 f"{difference(recs['parent'], recs['new'])}")
    if a.vs:
        rows.append(f"identical after normalising symbols and labels: {same} of {total}")
        rows += notes
    text = "\n".join(rows) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
