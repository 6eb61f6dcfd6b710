"""Compares the gfx950 device assembly of one .hip file of gtcrn_micro_amd/csrc (kernels.hip, train_kernels.hip,
metrics.hip, batch.hip, reverb.hip) between two source trees, kernel by kernel.

    hipcc --offload-arch=gfx950 <the flags gtcrn_micro_amd/build.py gives that file: the common ones and its per_file
          entry, if it has one> --cuda-device-only -S OLD/gtcrn_micro_amd/csrc/FILE.hip -o old.s
          (and the same for the new tree -> new.s)
    python tools/asm_compare.py old.s new.s [--drop-arg false] [--rename PATTERN REPLACEMENT]...

A kernel is its instruction lines in order: comments and assembler directives dropped, branch labels renumbered by
position.  Kernels pair up by demangled name without the argument list (cut at the first bracket outside the template
arguments: an enum argument demangles as (gtk::Synth)3).  --drop-arg VALUE: a kernel template of the
new file that gained one trailing template argument pairs with the old kernel when that argument is VALUE (only where
the old file has no kernel of the full name).  --rename PATTERN REPLACEMENT (any number of them): an old kernel whose name
the regular expression matches pairs with the new kernel of the name re.sub gives, e.g. a template whose flags became one
enum: --rename '<(\w+), false, true>' '<\1, (ns::Mode)2>'.  Kernels only the new file has are counted, not compared.
Prints one row per kernel of the old file and a summary line; exit status 1 if any kernel differs or is missing.
Needs c++filt on the PATH and no GPU.
"""
import argparse
import re
import subprocess
import sys


def kernels(path):
    out = {}
    for m in re.finditer(r"^(\S+):\s*; @\S+\n(.*?)^\.Lfunc_end\d+:", open(path).read(), re.S | re.M):
        lines, labels = [], {}
        for ln in m.group(2).splitlines():
            ln = ln.split(";")[0].strip()
            if not ln or (ln.startswith(".") and not ln.startswith(".LBB")):
                continue
            ln = re.sub(r"\.LBB\d+_\d+", lambda t: labels.setdefault(t.group(0), f".L{len(labels)}"), ln)
            lines.append(ln)
        out[m.group(1)] = lines
    return out


def demangled(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    # (batch.hip keeps its kernels in an unnamed namespace: that bracket is part of the name, not an argument list)
    return [without_args(d.replace("(anonymous namespace)", "{anonymous}")) for d in r.stdout.splitlines()]


def without_args(d):
    depth = 0
    for i, c in enumerate(d):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            return d[:i]
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--drop-arg", default=None)
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("PATTERN", "REPLACEMENT"))
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    old = dict(zip(demangled(list(old)), old.values()))
    new = dict(zip(demangled(list(new)), new.values()))
    if a.drop_arg:
        for k in list(new):
            short = re.sub(r", %s>$" % re.escape(a.drop_arg), ">", k)
            if short != k and k not in old and short in old and short not in new:
                new[short] = new.pop(k)
    was = {}                 # new name -> old name of the kernels --rename pairs (the first pattern that matches)
    for k in list(old):
        to = next((re.sub(pat, repl, k) for pat, repl in a.rename if re.search(pat, k)), k)
        if to != k:
            if to in old:
                sys.exit(f"--rename gives two old kernels the name {to}")
            old[to], was[to] = old.pop(k), k
    same = bad = 0
    for k in sorted(old):
        name = f"{was[k]} -> {k}" if k in was else k
        if k not in new:
            bad += 1
            print(f"MISSING {len(old[k]):6d}            {name}")
        elif old[k] == new[k]:
            same += 1
            print(f"same    {len(old[k]):6d}            {name}")
        else:
            bad += 1
            print(f"DIFFER  {len(old[k]):6d} -> {len(new[k]):6d}  {name}")
    print(f"{same} of {len(old)} kernels compile to the same instructions ({sum(map(len, old.values()))} lines); "
          f"{bad} differ or are missing; {len(set(new) - set(old))} kernels are new")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
