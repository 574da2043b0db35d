#!/usr/bin/env python3
"""Compare the device code of two trees of assembly files, function by function.

    compare_asm.py OLD_DIR NEW_DIR [--rename RENAMES]

Each directory holds NAME.s (hipcc HIPFLAGS --cuda-device-only -S) and NAME.remarks (the same command's stderr under
-Rpass-analysis=kernel-resource-usage) of any number of translation units; which file a function is in does not matter.
Every kernel and non-inlined device function is matched by demangled name and compared in three parts: its
instruction text (comments dropped and local label numbers normalised: both carry the function's index in its module),
its .amdhsa_* block with the .set resource symbols, and its resource remark. RENAMES has one "old<TAB>new" pair of
demangled names per line, for functions whose name changed on purpose. Prints the counts and each differing row;
exits 1 if anything differs.
"""
import argparse
import glob
import os
import re
import subprocess
import sys

LABEL = re.compile(r"\.L(BB|JTI|CPI|func_begin|func_end|tmp)\d+")


def parse_asm(path, funcs, dups):
    name, part, cur = None, None, None
    for line in open(path):
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            name, part = m.group(1), None
            cur = {"text": [], "hsa": [], "remark": []}
            (dups if name in funcs else funcs)[name] = cur
            continue
        s = line.split(";")[0].strip()   # comments name basic blocks by the function's index
        if s.startswith(".set ") and "." in s[5:].split(",")[0]:   # resource symbols, wherever the compiler puts them
            owner, _, field = s[5:].split(",")[0].rpartition(".")
            if owner in funcs:
                funcs[owner]["hsa"].append(".set ." + field + "," + s.split(",", 1)[1])
            continue
        if name is None:
            continue
        if "; -- End function" in line:
            name = None
        elif s == name + ":" or s.startswith(name + ":"):
            part = "text"
        elif s.startswith(".amdhsa_kernel"):
            part = "hsa"
        elif s.startswith(".end_amdhsa_kernel"):
            part = "after"
        elif s.startswith(".Lfunc_end"):
            part = "after"
        elif part == "text" and s and not s.startswith(".section") and not s.startswith(".p2align"):
            cur["text"].append(LABEL.sub(r".L\1", s))
        elif part == "hsa":
            cur["hsa"].append(s)


def parse_remarks(path, funcs):
    cur = None
    for line in open(path):
        m = re.search(r"remark: (.*) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        f = re.match(r"Function Name: (\S+)", m.group(1))
        if f:
            cur = funcs.get(f.group(1))
        elif cur is not None:
            cur["remark"].append(m.group(1).strip())


def load(d):
    funcs, dups = {}, {}
    for p in sorted(glob.glob(os.path.join(d, "*.s"))):
        parse_asm(p, funcs, dups)
    for p in sorted(glob.glob(os.path.join(d, "*.remarks"))):
        parse_remarks(p, funcs)
    names = list(funcs)
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(out.split("\n"), (funcs[n] for n in names))), sorted(dups)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename")
    a = ap.parse_args()
    old, old_dups = load(a.old)
    new, new_dups = load(a.new)
    if a.rename:
        for line in open(a.rename):
            if line.strip():
                o, n = line.rstrip("\n").split("\t")
                old[n] = old.pop(o)
    kern = lambda t: sum(1 for f in t.values() if f["hsa"] and f["hsa"][0].startswith(".amdhsa"))
    print(f"old: {len(old)} functions, {kern(old)} kernels; new: {len(new)} functions, {kern(new)} kernels")
    bad = 0
    for n in old_dups + new_dups:
        print("defined twice:", n)
        bad += 1
    for n in sorted(set(old) - set(new)):
        print("only in old:", n)
        bad += 1
    for n in sorted(set(new) - set(old)):
        print("only in new:", n)
        bad += 1
    equal = 0
    for n in sorted(set(old) & set(new)):
        parts = [p for p in ("text", "hsa", "remark") if old[n][p] != new[n][p]]
        if not parts:
            equal += 1
            continue
        bad += 1
        print(f"differs ({', '.join(parts)}): {n}")
        for p in parts:
            if p == "text":
                print(f"    instructions: old {len(old[n][p])} lines, new {len(new[n][p])} lines")
            else:
                for x in sorted(set(old[n][p]) - set(new[n][p])):
                    print("    old", x)
                for x in sorted(set(new[n][p]) - set(old[n][p])):
                    print("    new", x)
    print(f"{len(set(old) & set(new))} matched by name, {equal} equal in instructions, .amdhsa block and resources")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
