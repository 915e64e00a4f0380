#!/usr/bin/env python3
"""tools/isa_same.py OLD.s NEW.s FILTER -- do two builds' kernels run the same instruction streams?

OLD.s / NEW.s: device assembly of two builds (hipcc $(HIPFLAGS) --cuda-device-only -S).  Per kernel whose (mangled) name
matches the regular expression FILTER, three comparisons:
  count   the instruction counts are equal
  mnem    the mnemonics are equal as multisets, the eq / lg forms of a scalar compare and the two polarities of a scalar
          conditional branch counting as one name each (the compiler swaps them freely with the order of the blocks)
  mem     the ordered sequence of memory mnemonics (global_*, flat_*, ds_*, s_load*, buffer_*, scratch_*) is identical
Every other kernel must be the same text up to label numbers, and both files must hold the same kernels.  Exit status 1 on
any mismatch.  It compares; it does not look for any particular instruction."""
import collections
import re
import sys


def kernels(path):
    """{name: [instruction lines, comments stripped]} for every .amdhsa_kernel of the file"""
    text = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S).group(1)
        lines = [re.sub(r"\s*;.*", "", l).strip() for l in body.split("\n")]
        out[name] = [l for l in lines if l and not l.startswith(".") and not l.endswith(":")]
    return out


def mnemonic(line):
    m = line.split()[0]
    m = re.sub(r"^s_cmp_(eq|lg)_", "s_cmp_eqlg_", m)
    return re.sub(r"^s_cbranch_(scc|vcc|exec)(0|1|z|nz)$", r"s_cbranch_\1", m)


def memory(lines):
    return [l.split()[0] for l in lines if re.match(r"(global_|flat_|ds_|s_load|s_buffer_load|buffer_|scratch_)", l)]


def main():
    old, new, filt = kernels(sys.argv[1]), kernels(sys.argv[2]), re.compile(sys.argv[3])
    bad = 0
    for name in sorted(set(old) ^ set(new)):
        print("ONLY IN %s  %s" % ("OLD" if name in old else "NEW", name))
        bad += 1
    same_text = 0
    for name in sorted(set(old) & set(new)):
        a, b = old[name], new[name]
        if not filt.search(name):
            strip = lambda ls: [re.sub(r"\.L\w*\d\w*", ".L", l) for l in ls]
            if strip(a) != strip(b):
                print("CHANGED  %s (outside the filter: must be the same text)" % name)
                bad += 1
            same_text += 1
            continue
        res = (len(a) == len(b), collections.Counter(map(mnemonic, a)) == collections.Counter(map(mnemonic, b)), memory(a) == memory(b))
        print("%-4s count %5d %5d %s  mnem %s  mem %4d %s  identical %s  %s" % (
            "ok" if all(res) else "FAIL", len(a), len(b), "=" if res[0] else "!", "=" if res[1] else "!", len(memory(a)),
            "=" if res[2] else "!", "yes" if a == b else "no", name))
        bad += not all(res)
    print("%d kernels outside the filter compared as text; %d mismatches in all" % (same_text, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
