#!/usr/bin/env python3
"""Per-kernel ISA comparison of two source trees (CPU host, no GPU): the proof that a kernel-file refactor moved code and
changed none.

    python tools/kernel_isa_diff.py OLD_TREE NEW_TREE [--flags "-DMP_GEOM_PROF ..."]

Every multiply_amd/csrc/*.hip of both trees is compiled to gfx950 assembly with the build's own flags (multiply_amd/build.py
FLAGS + --cuda-device-only -S).  Each .s is cut into one record per function symbol: the instruction text from the symbol's label
to its .Lfunc_end, plus the .amdhsa_kernel descriptor block of a kernel (registers, LDS, scratch).  Only what depends on a
function's POSITION in its file is normalised away: the function index in local labels (.LBB<n>_<k>), the .Lfunc_begin / .Lfunc_end
numbers, and comments.  Records are matched by mangled symbol and reported as identical / differs / only in old / only in new,
grouped by old file -> new file.  Exit status 0 only when every record is identical and both trees define the same symbols."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiply_amd.build import FLAGS  # noqa: E402

_LOCAL = [(re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1")]


def _normalise(lines):
    out = []
    for line in lines:
        line = line.split(";", 1)[0].strip()
        if not line:
            continue
        for pat, rep in _LOCAL:
            line = pat.sub(rep, line)
        out.append(line)
    return out


def records(asm):
    """{symbol: normalised text} of every function in one .s file"""
    lines = asm.split("\n")
    label = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"([A-Za-z_$][\w$.]*):", l))}
    desc = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            desc[m.group(1)] = lines[i:end + 1]
    recs = {}
    for l in lines:
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", l)
        if not m or m.group(1) not in label:
            continue
        sym, i = m.group(1), label[m.group(1)]
        end = next(j for j in range(i, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[j]))
        recs[sym] = "\n".join(_normalise(lines[i:end + 1] + desc.get(sym, [])))
    return recs


def compile_tree(tree, flags, tmp, tag):
    """[(file, symbol, text)] over the tree's csrc/*.hip"""
    csrc = os.path.join(tree, "multiply_amd", "csrc")
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    hipcc = os.environ.get("HIPCC", "hipcc")

    def one(f):
        out = os.path.join(tmp, f"{tag}_{f[:-4]}.s")
        r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, f), "-o", out], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {tree}: {f}\n{r.stdout}{r.stderr}")
        with open(out) as fh:
            return [(f, sym, text) for sym, text in records(fh.read()).items()]

    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as ex:
        return [rec for recs in ex.map(one, srcs) for rec in recs]


def compare(old, new):
    """[(old file or None, new file or None, symbol, verdict)]; a symbol defined by several files of a tree (kernels of equal name
    in anonymous namespaces) pairs with the record of the same file first"""
    by_sym = defaultdict(lambda: ([], []))
    for side, recs in enumerate((old, new)):
        for f, sym, text in recs:
            by_sym[sym][side].append((f, text))
    rows = []
    for sym, (o, n) in sorted(by_sym.items()):
        pairs = []
        for fo, to in list(o):
            hit = next(((fn, tn) for fn, tn in n if fn == fo), None)
            if hit:
                pairs.append(((fo, to), hit))
                o.remove((fo, to))
                n.remove(hit)
        while o and n:
            pairs.append((o.pop(0), n.pop(0)))
        rows += [(fo, fn, sym, "identical" if to == tn else "differs") for (fo, to), (fn, tn) in pairs]
        rows += [(fo, None, sym, "only in old") for fo, _ in o] + [(None, fn, sym, "only in new") for fn, _ in n]
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--flags", default="", help="extra compiler flags for both trees")
    args = ap.parse_args()
    flags = FLAGS + args.flags.split()
    with tempfile.TemporaryDirectory() as tmp:
        old = compile_tree(args.old_tree, flags, tmp, "old")
        new = compile_tree(args.new_tree, flags, tmp, "new")
    rows = compare(old, new)
    groups = defaultdict(list)
    for fo, fn, sym, verdict in rows:
        groups[(fo or "-", fn or "-")].append((sym, verdict))
    print("hipcc " + " ".join(flags) + " --cuda-device-only -S")
    for (fo, fn), items in sorted(groups.items()):
        print(f"\n{fo} -> {fn}")
        for sym, verdict in items:
            print(f"  {verdict:<12} {sym}")
    verdicts = ("identical", "differs", "only in old", "only in new")
    print("\n" + f"{'old file -> new file':<34}" + "".join(f"{v:>13}" for v in verdicts))
    for key, items in sorted(groups.items()):
        print(f"{key[0] + ' -> ' + key[1]:<34}" + "".join(f"{sum(v == w for _, w in items):>13}" for v in verdicts))
    total = [sum(v == w for _, _, _, w in rows) for v in verdicts]
    print(f"{'total':<34}" + "".join(f"{c:>13}" for c in total))
    ok = total[0] == len(rows)
    print("RESULT: " + ("every function identical, same symbols in both trees" if ok else "NOT a pure move"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
