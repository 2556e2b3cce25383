#!/usr/bin/env python3
"""Compare the gfx950 instruction streams of two builds of the kernel translation unit, kernel by kernel.

    hipcc --offload-arch=gfx950 <HIPFLAGS of csrc/Makefile> --cuda-device-only -S -o old.s selection_kernels.hip     (in the old tree)
    hipcc ... --cuda-device-only -S -o new.s selection_kernels.hip                                                  (in the new tree)
    scripts/compare_kernel_isa.py old.s new.s [--strip ", false"] [--rename OLD=NEW ...]

Every kernel of old.s must be in new.s with the same instructions (labels renumbered, comments and directives dropped).  A kernel that
gained a trailing template argument is matched by its demangled name with `--strip` taken off the end of the argument list: the
count kernels' `EMIT = false` instantiations are `--strip ", false"`.  A kernel whose template argument was renamed is matched with
`--rename OLD=NEW` (repeatable), applied as whole words to the demangled names of old.s before matching.  Prints what differs and the
kernels that only new.s has; exit status 1 if a kernel of old.s is missing or differs.  Needs no GPU.
"""
import argparse
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: [instruction lines]} of the .amdhsa kernels of an assembly file"""
    out, name, body = {}, None, []
    kernel_names = set()
    lines = open(path, errors="replace").read().split("\n")
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            kernel_names.add(m.group(1))
    for ln in lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
        if m and m.group(1) in kernel_names:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", ln):
            out[name] = body
            name = None
            continue
        code = ln.split(";")[0].strip()
        if not code or (code.startswith(".") and not code.startswith(".LBB")):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", code))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.split("\n")))


def template_head(demangled):
    """`name<arguments>` of a demangled template kernel (the text in front of its parameter list), None for any other"""
    i = demangled.rfind(">(")
    return demangled[:i + 1] if i >= 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--strip", default=", false", help="trailing template argument text a kernel may have gained")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="a name of the old build that the new build spells NEW")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    d_old, d_new = demangle(list(old)), demangle(list(new))
    for o, n in (r.split("=", 1) for r in a.rename):
        d_old = {m: re.sub(rf"\b{re.escape(o)}\b", n, dn) for m, dn in d_old.items()}
    by_name = {}
    for mangled, dn in d_new.items():
        by_name[dn] = mangled
        head = template_head(dn)
        if head and head.endswith(a.strip + ">"):
            by_name.setdefault(("stripped", head[:-len(a.strip) - 1] + ">"), mangled)
    bad, matched = 0, set()
    for mangled, dn in sorted(d_old.items(), key=lambda kv: kv[1]):
        tgt = by_name.get(dn)
        if tgt is None:
            tgt = by_name.get(("stripped", template_head(dn)))
        if tgt is None:
            print(f"MISSING  {dn}")
            bad += 1
            continue
        matched.add(tgt)
        if old[mangled] != new[tgt]:
            n = next((i for i, (x, y) in enumerate(zip(old[mangled], new[tgt])) if x != y), min(len(old[mangled]), len(new[tgt])))
            print(f"DIFFERS  {dn}: {len(old[mangled])} -> {len(new[tgt])} instructions, first difference at {n}")
            bad += 1
    only_new = sorted(template_head(d_new[k]) or d_new[k] for k in new if k not in matched)
    print(f"{len(old)} kernels in the old build, {len(old) - bad} identical in the new one, {bad} missing or different")
    print(f"{len(only_new)} kernels only in the new build:")
    for n in only_new:
        print("  " + n)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
