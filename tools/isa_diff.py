#!/usr/bin/env python3
"""isa_diff.py [--by-body] OLD.s NEW.s — "same kernels, same ISA" as a command.

Compares two device assembly files (`make asm`) function by function: prints
the functions found on one side only and those whose bodies differ, and
exits non-zero if there are any.  Comments, trailing whitespace and the
function index in local labels (which follows instantiation order) are
ignored.

--by-body is for a change that renames kernels (other template parameters,
other argument types).  A function's own name is masked inside its body and
the bodies of the two files are compared as multisets: a body found on both
sides is "identical" whatever it is called.  What is left is paired by name
pattern — the function's plain name and the integer and bool literals of its
mangled name, in order — and a pair is of "same memory behaviour" when
  * .amdhsa_next_free_vgpr, .amdhsa_accum_offset and the group and private
    segment sizes are unchanged, and
  * the multiset of mnemonics of every instruction that accesses memory or
    synchronises (global_*, buffer_*, ds_*, *load*, *waitcnt*, *barrier*) is
    unchanged;
a function whose pattern has no counterpart (a renamed family, another
parameter list) is paired with any unpaired function of OLD.s of the same
memory behaviour.  Everything else is "other".  Prints the three counts (per
kernel family too) and the functions of OLD.s left without a counterpart, and
exits non-zero if there is anything in "other" or without a counterpart."""
import collections
import re
import sys

FUNC = re.compile(r"; -- Begin function (\S+)\n(.*?)\n\s*; -- End function", re.S)
LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+")
LITERAL = re.compile(r"L[a-z](n?\d+)E")
RESOURCES = (".amdhsa_next_free_vgpr", ".amdhsa_accum_offset", ".amdhsa_group_segment_fixed_size",
             ".amdhsa_private_segment_fixed_size")


def functions(path, mask_name=False):
    out = {}
    for name, body in FUNC.findall(open(path).read()):
        if mask_name:
            body = body.replace(name, "@SELF")
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


def family(name):
    """Plain name of a mangled function: _ZN3sml15k_quantize_packI... -> k_quantize_pack."""
    m = re.match(r"_ZN3sml(\d+)", name) or re.match(r"_Z(\d+)", name)
    if not m:
        return name
    return name[m.end():m.end() + int(m.group(1))]


def pattern(name):
    return (family(name), tuple(LITERAL.findall(name)))


def memory_behaviour(lines):
    res, mnemonics = {}, collections.Counter()
    for ln in lines:
        tok = ln.split()
        if tok[0] in RESOURCES:
            res[tok[0]] = tok[1]
        elif ln[0].isspace() and not tok[0].startswith(".") and not tok[0].endswith(":"):
            m = tok[0]
            if m.startswith(("global_", "buffer_", "ds_")) or any(w in m for w in ("load", "waitcnt", "barrier")):
                mnemonics[m] += 1
    return res, mnemonics


def main_by_body(old_path, new_path, verbose):
    old, new = functions(old_path, True), functions(new_path, True)
    pool = collections.defaultdict(list)            # body -> old names not yet paired
    for name, lines in old.items():
        pool[tuple(lines)].append(name)
    counts = collections.defaultdict(lambda: [0, 0, 0])   # family -> identical, same memory behaviour, other
    left_new = []
    for name, lines in new.items():
        names = pool.get(tuple(lines))
        if names:
            names.pop()
            counts[family(name)][0] += 1
        else:
            left_new.append(name)
    left_old = collections.defaultdict(list)        # pattern -> old names without an identical body
    for names in pool.values():
        for name in names:
            left_old[pattern(name)].append(name)
    notes, unpaired = [], []
    for name in left_new:
        before = left_old.get(pattern(name))
        if not before:
            unpaired.append(name)
        elif memory_behaviour(old[before.pop()]) == memory_behaviour(new[name]):
            counts[family(name)][1] += 1
            notes.append(("same memory behaviour", name))
        else:
            counts[family(name)][2] += 1
            notes.append(("other", name))
    # a renamed family or a changed parameter list leaves no pattern to pair by:
    # such functions are paired like the bodies, as a multiset of memory behaviours
    behaviours = collections.defaultdict(list)
    for names in left_old.values():
        for name in names:
            res, mnemonics = memory_behaviour(old[name])
            behaviours[(tuple(sorted(res.items())), tuple(sorted(mnemonics.items())))].append(name)
    for name in unpaired:
        res, mnemonics = memory_behaviour(new[name])
        before = behaviours.get((tuple(sorted(res.items())), tuple(sorted(mnemonics.items()))))
        if before:
            gone_name = before.pop()
            left_old[pattern(gone_name)].remove(gone_name)
            counts[family(name)][1] += 1
            notes.append(("same memory behaviour", name))
        else:
            counts[family(name)][2] += 1
            notes.append(("other", name))
    gone = sorted(name for names in left_old.values() for name in names)   # no counterpart after
    notes += [("before only", name) for name in gone]
    for what, name in sorted(notes):
        if verbose or what != "same memory behaviour":
            print(f"{what}: {name}")
    for fam in sorted(counts):
        print("  %-24s identical %4d, same memory behaviour %4d, other %4d" % (fam, *counts[fam]))
    total = [sum(c[i] for c in counts.values()) for i in range(3)]
    print(f"{new_path}: {len(new)} functions, {len(old)} before: identical {total[0]}, "
          f"same memory behaviour {total[1]}, other {total[2]}; {len(gone)} before only")
    return 1 if total[2] or gone else 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("-")]
    flags = set(sys.argv[1:]) - set(args)
    if len(args) != 2 or flags - {"--by-body", "-v"}:
        sys.exit(__doc__)
    sys.exit(main_by_body(*args, "-v" in flags) if "--by-body" in flags else main(*args))
