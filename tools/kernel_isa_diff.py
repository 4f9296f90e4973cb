#!/usr/bin/env python3
"""Compare two device assembly files kernel by kernel: the instructions and the kernel descriptor of every kernel.

    python tools/kernel_isa_diff.py OLD.s NEW.s [OLD_NAME=NEW_NAME ...]

The .s files come from the Makefile's compile line with `--cuda-device-only -S` in place of `-c`:

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fvisibility=hidden \\
          [-fno-slp-vectorize for the scorer's units] --cuda-device-only -S <unit>.hip -o <unit>.s

A kernel is the text from its label to its `.end_amdhsa_kernel` (code, then the descriptor: VGPR / SGPR / LDS / scratch),
comments stripped and the compiler's numbered labels (basic blocks, function ends, temporaries) mapped to a common form, so
that a kernel that moved inside its file compares equal.  OLD=NEW pairs (mangled or demangled names) match a kernel whose name
changed, e.g. one that lost a template parameter.  Prints SAME or DIFF per kernel (with the first differing lines) and the
kernels present on one side only; exit status 1 on any DIFF.  Needs no GPU.
"""
import re
import subprocess
import sys

SHOW = 6                                     # differing lines printed per kernel


def demangle(names):
    if not names:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    # kernels differ in their template arguments, not in their parameter lists: drop the latter
    return {n: re.sub(r"\((?!anonymous namespace\)).*", "", d) for n, d in zip(names, out)}


def kernels(path):
    """mangled name -> normalised lines of the kernel (label .. .end_amdhsa_kernel)"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    found = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        body = []
        for l in lines[start:end + 1]:
            l = re.sub(r"\s*(;|//).*", "", l).strip()
            if not l:
                continue
            l = re.sub(r"\.?LBB\d+_", "LBB_", l)                    # basic blocks: function number dropped, block number kept
            l = re.sub(r"\.L(func_end|func_begin|tmp)\d+", r".L\1", l)
            body.append(re.sub(r"\s+", " ", l))
        found[name] = body
    return found


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    dold, dnew = demangle(list(old)), demangle(list(new))
    renamed = dict(p.split("=", 1) for p in sys.argv[3:])
    by_dem = {d: n for n, d in dnew.items()}
    n_same = n_diff = 0
    only_old, matched = [], set()
    for name, body in old.items():
        want = renamed.get(name, renamed.get(dold[name]))
        other = name if want is None else (want if want in new else by_dem.get(want))
        if other not in new:
            only_old.append(dold[name])
            continue
        matched.add(other)
        # the kernel's own name occurs in its text (label, descriptor, symbol arithmetic): one spelling for both sides
        a = [l.replace(name, "KERNEL") for l in body]
        b = [l.replace(other, "KERNEL") for l in new[other]]
        label = dold[name] if other == name else f"{dold[name]} = {dnew[other]}"
        if a == b:
            n_same += 1
            print(f"SAME  {label}  ({len(a)} lines)")
            continue
        n_diff += 1
        print(f"DIFF  {label}  ({len(a)} / {len(b)} lines)")
        shown = 0
        for i in range(max(len(a), len(b))):
            la, lb = (a[i] if i < len(a) else "<end>"), (b[i] if i < len(b) else "<end>")
            if la != lb:
                print(f"      line {i + 1}:  - {la}\n      {' ' * len(str(i + 1))}        + {lb}")
                shown += 1
                if shown == SHOW:
                    break
    for d in only_old:
        print(f"ONLY IN {sys.argv[1]}:  {d}")
    for n in new:
        if n not in matched:
            print(f"ONLY IN {sys.argv[2]}:  {dnew[n]}")
    print(f"{n_same} same, {n_diff} differ, {len(only_old)} only old, {len(new) - len(matched)} only new")
    sys.exit(1 if n_diff else 0)


if __name__ == "__main__":
    main()
