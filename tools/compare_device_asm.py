#!/usr/bin/env python3
"""Function-by-function comparison of gfx950 assembly before and after a move of kernels between translation units.
    python3 tools/compare_device_asm.py --old OLD.s [OLD.s ...] --new NEW.s [NEW.s ...]
Each .s is the output of the tests/test_codegen.py command line (hipcc -S --cuda-device-only) for one unit.  A function is its
text from `.type NAME,@function` to its `.end_amdhsa_kernel` (its kernel descriptor included), instructions and directives, with
comments, .loc / .file lines and the per-unit ordinals of local labels normalised -- the rule of DESIGN.md section 7e.  Every
function of the old units must stand in exactly one new unit, unchanged.  Exit status 1 if one is missing, doubled or differs."""
import argparse
import os
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for ln in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            name, body = m.group(1), []
            assert name not in out, (path, name)
        if name is None:
            continue
        ln = ln.split(";")[0].strip()
        if not ln or ln.startswith((".loc", ".file")):
            continue
        body.append(re.sub(r"\.L(BB|func_begin|func_end|tmp)\d+", r".L\1", ln))
        if ln == ".end_amdhsa_kernel":
            out[name], name = "\n".join(body), None
    assert name is None, (path, name, "a function that is no kernel: extend the rule")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    new = {os.path.basename(p): functions(p) for p in a.new}
    for unit, fns in new.items():
        print("new %-24s %4d functions" % (unit, len(fns)))
    bad, seen = 0, set()
    for p in a.old:
        old = functions(p)
        seen |= set(old)
        homes = {n: [u for u, fns in new.items() if n in fns] for n in old}
        missing = [n for n, h in homes.items() if not h]
        doubled = [n for n, h in homes.items() if len(h) > 1]
        differ = [n for n, h in homes.items() if len(h) == 1 and new[h[0]][n] != old[n]]
        print("old %-24s %4d functions: %d missing, %d in more than one new unit, n of m differ: %d of %d" %
              (os.path.basename(p), len(old), len(missing), len(doubled), len(differ), len(old)))
        for n in sorted(set(h[0] for h in homes.values() if len(h) == 1)):
            print("    %4d now in %s" % (sum(1 for h in homes.values() if h == [n]), n))
        for kind, names in (("missing", missing), ("doubled", doubled), ("differs", differ)):
            for n in names:
                print("    %s: %s" % (kind, n))
        bad += len(missing) + len(doubled) + len(differ)
    extra = sorted(n for fns in new.values() for n in fns if n not in seen)
    print("functions only in the new units: %d" % len(extra))
    for n in extra:
        print("    %s" % n)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
