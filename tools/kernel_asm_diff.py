#!/usr/bin/env python3
"""Which kernels compile to the same gfx950 code in two trees: the evidence a refactor needs before it carries
profiles/pmc_traffic.json's source digest forward.  Every unit is compiled to device assembly with the flags of its tree's
build.UNITS (`--cuda-device-only -S`; works without a GPU), cut into its functions, and the BODIES are compared -- from a
function's label to its .Lfunc_end, with the function number of local labels (.LBB12_3) normalised, since a new helper renumbers
them; data symbols, kernel descriptors and the metadata notes are left out.  The functions of all units given are POOLED per tree
and compared by name, so a kernel that moved to another unit is still compared with itself; of the units given, a tree compiles
those its own build.UNITS has.  A name that occurs in two units of one tree is keyed `name [unit]`; where B's unit of such a name
is not one of A's (units folded or renamed), B's function is compared with one of A's that is still free, an equal one first.

usage: kernel_asm_diff.py A B UNIT [UNIT ...] [--show NAME]
  A, B    a directory that holds sushi_amd/ and include/ (a checkout, an export), or a commit (exported to a scratch copy);
          `.` is the working tree
  UNIT    sushi_fft, sushi_curve, ... (build.UNITS of either tree)
  --show NAME   also print a unified diff of the bodies of the functions whose name contains NAME
prints per function `same`, `differs` (with the bodies' line counts), `only in A`, `only in B`; exit status 1 if anything differs
example: tools/kernel_asm_diff.py HEAD . sushi_fft sushi_curve"""
import collections
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sushi_amd import build  # noqa: E402


def tree_of(spec, scratch):
    """The directory of a tree: `spec` itself, or an export of the commit `spec`."""
    if os.path.isdir(os.path.join(spec, "sushi_amd", "csrc")):
        return os.path.abspath(spec)
    out = os.path.join(scratch, "tree_" + re.sub(r"\W", "_", spec))
    os.makedirs(out)
    tar = subprocess.Popen(["git", "-C", ROOT, "archive", spec, "sushi_amd", "include"], stdout=subprocess.PIPE)
    subprocess.check_call(["tar", "-x", "-C", out], stdin=tar.stdout)
    if tar.wait() != 0:
        raise SystemExit("git archive %s failed" % spec)
    return out


# what `tree`'s own build.py is asked, in a process of its own (argv: unit, output file)
ASSEMBLE = """
import subprocess, sys
from sushi_amd import build as b
unit, out = sys.argv[1:]
if hasattr(b, "compile_command"):
    b.write_generated()
    cmd = b.compile_command(unit, out, "asm")
else:       # a commit before build.compile_command: its four writers by name, its flags from UNITS, the command spelled out
    b.write_twiddles(); b.write_dft16_operands(); b.write_dft16_bound_operands(); b.write_dft16_bound_low_operands()
    flags = next(u[1] for u in b.UNITS if u[0] == unit)
    cmd = [b._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall"] + flags + \\
          ["--cuda-device-only", "-S", b.CSRC + "/" + unit + ".hip", "-o", out]
sys.exit(subprocess.call(cmd))
"""


def assembly(tree, unit, out):
    """Device assembly of one unit of `tree`, by that tree's own build.py (its flags, its generated tables)."""
    subprocess.check_call([sys.executable, "-c", ASSEMBLE, unit, out], cwd=tree)
    return open(out).read()


def units_of(tree):
    """The unit names of `tree`'s own build.UNITS ((name, flags) pairs; (name, flags, deps) before build.unit_deps)."""
    code = "from sushi_amd import build as b; print(' '.join(u[0] for u in b.UNITS))"
    return subprocess.check_output([sys.executable, "-c", code], cwd=tree, text=True).split()


def pooled(tree, units, scratch, tag):
    """[(unit, name, body)] of every function of those of `units` that `tree` has."""
    have = units_of(tree)
    return [(unit, name, body) for unit in units if unit in have
            for name, body in functions(assembly(tree, unit, os.path.join(scratch, "%s_%s.s" % (unit, tag)))).items()]


def keyed(pool, by_unit, partner=None):
    """{key: body}: a name that occurs in two units of a tree is keyed `name [unit]`.  With `partner` (the other tree's keyed
    functions) such a function whose own unit the other tree does not have under that name is keyed by the unit of a function
    there that is still free, one with the same body first: units that were folded or renamed are still compared."""
    out, moved = {}, []
    for unit, name, body in pool:
        key = "%s [%s]" % (name, unit) if name in by_unit else name
        if partner is not None and name in by_unit and key not in partner:
            moved.append((name, key, body))
        else:
            out[key] = body
    for name, key, body in moved:
        free = [k for k in partner if k.startswith(name + " [") and k not in out]
        free.sort(key=lambda k: partner[k] != body)
        out[free[0] if free else key] = body
    return out


def demangle(names):
    if not names:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(anonymous namespace\)::|^void ", "", d).split("(")[0] for n, d in zip(names, out)}


def functions(text):
    """{demangled name: body lines} of every function of an assembly file (kernels and the device functions left out of line)."""
    lines = text.split("\n")
    types = set(re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M))
    names = demangle(sorted(types))
    out, cur, body = {}, None, []
    for line in lines:
        m = re.match(r"^([A-Za-z_$.][\w$.]*):", line)
        if cur is None:
            if m and m.group(1) in types:
                cur, body = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[names[cur]] = body
            cur = None
            continue
        line = re.sub(r"\.L(BB|JTI|tmp|func_begin)\d+(_\d+)?", lambda k: ".L%s#%s" % (k.group(1), k.group(2) or ""), line)
        line = re.sub(r"\s*;.*$", "", line).rstrip()            # (comments name source lines and basic blocks)
        if line.strip() and not re.match(r"^\s*\.(loc|file|cfi_\w+|p2align)\b", line):
            body.append(line)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("units", nargs="+")
    ap.add_argument("--show", action="append", default=[])
    args = ap.parse_args()
    differs = 0
    with tempfile.TemporaryDirectory(prefix="sushi_asm_diff_") as scratch:
        ta, tb = tree_of(args.a, scratch), tree_of(args.b, scratch)
        pa, pb = pooled(ta, args.units, scratch, "a"), pooled(tb, args.units, scratch, "b")
        # (a name in two units of one tree: keyed by its unit, in both trees)
        by_unit = {name for pool in (pa, pb) for name, n in collections.Counter(name for _, name, _ in pool).items() if n > 1}
        fa = keyed(pa, by_unit)
        fb = keyed(pb, by_unit, fa)
        for tag, pool in (("A", pa), ("B", pb)):
            print("%s: %d functions in %s" % (tag, len(pool), ", ".join(sorted({unit for unit, _, _ in pool}))))
        for name in sorted(set(fa) | set(fb)):
            if name not in fb or name not in fa:
                verdict = "only in A" if name in fa else "only in B"
            elif fa[name] == fb[name]:
                verdict = "same"
            else:
                verdict = "differs (%d lines against %d)" % (len(fa[name]), len(fb[name]))
            differs += verdict != "same"
            print("  %-60s %s" % (name[:60], verdict))
            if name in fa and name in fb and fa[name] != fb[name] and any(s in name for s in args.show):
                print("\n".join(difflib.unified_diff(fa[name], fb[name], "A", "B", lineterm="", n=2)))
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
