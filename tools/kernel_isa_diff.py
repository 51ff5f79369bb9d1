#!/usr/bin/env python3
"""Compare the instruction streams of kernels in two assembly listings (`make -C csrc asm`).

    python tools/kernel_isa_diff.py OLD.s NEW.s k_blk_sweep

For every function whose (mangled or demangled) name matches the filter, a regular expression, the
instruction lines of both files are compared as text after dropping comments and assembler
directives and normalising the function number in local labels (.LBB<n>_<k> -> .LBB_<k>).  One
line per kernel: `identical` or `different`, with both instruction counts (labels not counted).
Exit status 1 if any kernel differs or is missing from one file, else 0.  --show N prints the
first N lines of a unified diff for each kernel that differs.

--rename REGEX=REPL (repeatable, applied in order with re.sub) rewrites the demangled names of the
OLD listing before matching, and kernels are then matched by demangled name: a kernel whose symbol
changed is reported `identical` / `different` instead of `missing`.

    python tools/kernel_isa_diff.py OLD.s NEW.s . --rename 'k_batch_wg_dual[(]=k_batch_wg<1>('
"""
import argparse
import difflib
import re
import shutil
import subprocess
import sys

_FUNC = re.compile(r"^([A-Za-z_$][\w$.]*):")
_END = re.compile(r"^\.Lfunc_end\d+:")
_LOCAL = re.compile(r"\.LBB\d+_")


def kernels(path):
    """{name: [normalised instruction and label lines]} of every function in the listing."""
    out, name, body = {}, None, None
    with open(path, errors="replace") as f:
        for raw in f:
            if name is None:
                m = _FUNC.match(raw)
                if m:
                    name, body = m.group(1), []
                continue
            if _END.match(raw):
                out[name] = body
                name = None
                continue
            line = raw.split(";", 1)[0].strip()
            if not line:
                continue
            if line.startswith(".") and not line.endswith(":"):
                continue   # an assembler directive
            body.append(_LOCAL.sub(".LBB_", line))
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    lines = res.stdout.splitlines()
    return dict(zip(names, lines)) if len(lines) == len(names) else {n: n for n in names}


def count(body):
    return sum(1 for l in body if not l.endswith(":"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("filter", help="regular expression on the kernel's name")
    ap.add_argument("--show", type=int, default=0, metavar="N",
                    help="print the first N diff lines of each kernel that differs")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL",
                    help="rewrite the old listing's demangled names before matching (repeatable)")
    a = ap.parse_args(argv)
    ko, kn = kernels(a.old), kernels(a.new)
    if a.rename:   # match by demangled name, the old side's after the renames
        subs = [r.split("=", 1) for r in a.rename]
        if any(len(sub) != 2 for sub in subs):
            ap.error("--rename takes REGEX=REPL")
        po, pn = demangle(sorted(ko)), demangle(sorted(kn))
        for rx, repl in subs:
            po = {n: re.sub(rx, repl, p) for n, p in po.items()}
        ko = {po[n]: body for n, body in ko.items()}
        kn = {pn[n]: body for n, body in kn.items()}
    names = sorted(set(ko) | set(kn))
    pretty = {n: n for n in names} if a.rename else demangle(names)
    pat = re.compile(a.filter)
    names = [n for n in names if pat.search(n) or pat.search(pretty[n])]
    if not names:
        print(f"no kernel matches {a.filter!r}", file=sys.stderr)
        return 1
    same = 0
    for n in names:
        if n not in ko or n not in kn:
            print(f"missing in {'old' if n not in ko else 'new'}  {pretty[n]}")
            continue
        o, w = ko[n], kn[n]
        if o == w:
            same += 1
            print(f"identical  {count(o):6d} {count(w):6d}  {pretty[n]}")
            continue
        print(f"different  {count(o):6d} {count(w):6d}  {pretty[n]}")
        for k, l in enumerate(difflib.unified_diff(o, w, "old", "new", n=2, lineterm="")):
            if k >= a.show:
                break
            print("    " + l)
    print(f"{same} of {len(names)} kernels identical")
    return 0 if same == len(names) else 1


if __name__ == "__main__":
    sys.exit(main())
