#!/usr/bin/env python3
"""isa_diff.py OLD.s NEW.s — "same kernels, same ISA" as a command.

Compares two device assembly files (`make asm`) function by function: prints
the functions found on one side only and those whose bodies differ, and
exits non-zero if there are any.  Comments, trailing whitespace and the
function index in local labels (which follows instantiation order) are
ignored."""
import re
import sys

FUNC = re.compile(r"; -- Begin function (\S+)\n(.*?)\n\s*; -- End function", re.S)
LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+")


def functions(path):
    out = {}
    for name, body in FUNC.findall(open(path).read()):
        lines = (LABEL.sub(r".\1", ln.split(";")[0]).rstrip() for ln in body.splitlines())
        out[name] = [ln for ln in lines if ln]
    return out


def main(old_path, new_path):
    old, new = functions(old_path), functions(new_path)
    only = [("only in " + p, n) for p, a, b in ((old_path, old, new), (new_path, new, old)) for n in sorted(a.keys() - b.keys())]
    differ = [("differs", n) for n in sorted(old.keys() & new.keys()) if old[n] != new[n]]
    for what, name in only + differ:
        print(f"{what}: {name}")
    print(f"{new_path}: {len(new)} functions, {len(old)} before, {len(only)} on one side only, {len(differ)} differ")
    return 1 if only or differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
