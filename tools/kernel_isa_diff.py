#!/usr/bin/env python3
"""Compare the kernels of two device listings opcode by opcode (runs without a GPU).
usage: kernel_isa_diff.py OLD.s NEW.s MAP
OLD.s / NEW.s: the library's device code as assembly, built with the flags of sslap_amd/build.py:
    hipcc <build.FLAGS without -shared> --cuda-device-only -S sslap_amd/csrc/misslap.hip -o OLD.s
MAP: a text file, one `old new` pair per line ('#' starts a comment): substrings of MANGLED kernel names.  Every kernel
of OLD.s whose name holds `old` is compared with the kernel of NEW.s of that name with `old` replaced by `new` (a kernel
struct's entry, k_batched and k_batched_ptr forms all hold the struct's name).  Every other kernel is compared with the
kernel of the same name.
Of an instruction only the opcode is kept: comments, directives, labels and operands (register and label numbers, LDS
offsets) differ between two builds of the same program.  Per mapped kernel: the instruction count of each side and the
unified diff of the two opcode sequences, each hunk header naming the basic block of OLD.s it starts in and the
compiler's loop comment of that block; for the rest: the names of the kernels that differ or exist on one side."""
import difflib
import re
import sys


class Ops(list):
    """the opcodes of a kernel; where[i]: the basic block of instruction i as the listing names it, with the compiler's
    loop comment ("in Loop: Header=BB139_14 Depth=1"; none: the block lies in no loop, i.e. in entry or exit code)"""
    def __init__(self):
        super().__init__()
        self.where = []


def kernels(path):
    """mangled name -> Ops, for every function of the listing"""
    out, name, block = {}, None, ""
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, block = m.group(1), "entry block"
            out[name] = Ops()
            continue
        if name is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            name = None
            continue
        m = re.match(r"(?:\.(LBB\d+_\d+):|; %bb\.(\d+):)\s*(?:;\s*(.*))?", line)
        if m:
            block = ("%s %s" % (m.group(1) or "bb." + m.group(2), (m.group(3) or "").strip())).strip()
            continue
        code = line.split(";")[0].strip()
        if code and not code.startswith(".") and not code.endswith(":"):
            out[name].append(code.split()[0])
            out[name].where.append(block)
    return out


def hunks(a, b):
    """unified diff of two Ops, two lines of context; a hunk's header names the block of the old listing it starts in"""
    for group in difflib.SequenceMatcher(None, a, b, autojunk=False).get_grouped_opcodes(2):
        i1, i2, j1, j2 = group[0][1], group[-1][2], group[0][3], group[-1][4]
        first = next((g[1] for g in group if g[0] != "equal"), i1)
        yield "@@ -%d,%d +%d,%d @@ old: %s" % (i1 + 1, i2 - i1, j1 + 1, j2 - j1, a.where[min(first, len(a) - 1)])
        for tag, x1, x2, y1, y2 in group:
            if tag == "equal":
                yield from (" " + op for op in a[x1:x2])
            else:
                yield from ("-" + op for op in a[x1:x2])
                yield from ("+" + op for op in b[y1:y2])


def main():
    if len(sys.argv) != 4:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    pairs = [ln.split("#")[0].split() for ln in open(sys.argv[3])]
    pairs = [p for p in pairs if p]
    if any(len(p) != 2 for p in pairs):
        sys.exit("MAP: two names per line")
    mapped_old, mapped_new = set(), set()
    for o, n in pairs:
        names = sorted(k for k in old if o in k)
        if not names:
            print(f"## {o}: no kernel of the old listing holds this name")
        for k in names:
            k2 = k.replace(o, n)
            mapped_old.add(k)
            if k2 not in new:
                print(f"## {k} -> {k2}: not in the new listing")
                continue
            mapped_new.add(k2)
            a, b = old[k], new[k2]
            print(f"## {k} -> {k2}: {len(a)} -> {len(b)} instructions")
            for d in hunks(a, b):
                print(d)
    rest_old, rest_new = set(old) - mapped_old, set(new) - mapped_new
    differing = sorted(k for k in rest_old & rest_new if old[k] != new[k])
    for k in differing:
        print(f"## outside the map, differs: {k} ({len(old[k])} -> {len(new[k])} instructions)")
    for k in sorted(rest_old - rest_new):
        print(f"## outside the map, only in the old listing: {k}")
    for k in sorted(rest_new - rest_old):
        print(f"## outside the map, only in the new listing: {k}")
    print(f"## {len(mapped_old)} mapped kernels; outside the map: {len(rest_old & rest_new)} compared, "
          f"{len(differing)} differ, {len(rest_old - rest_new)} only old, {len(rest_new - rest_old)} only new")


if __name__ == "__main__":
    main()
