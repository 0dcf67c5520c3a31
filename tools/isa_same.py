#!/usr/bin/env python3
"""Whether two builds of a HIP unit are the same machine code, kernel by kernel (no GPU needed).

    hipcc <the library's flags> -S --cuda-device-only ffx_trace.hip -o parent.s     (once per tree)
    python tools/isa_same.py parent.s new.s [--map 'OLD=NEW' ...]

--map (repeatable) compares a renamed kernel against its predecessor: OLD and NEW are demangled kernel names without return type and
argument list, e.g. --map 'k_old<true>=k_new<true, false>'.  For that, every kernel's own symbol is masked in its instruction text, with
or without --map: without it both sides hold the same symbol there, so the verdicts are what they were.

Per kernel symbol it compares the instruction text (labels and directives included; comments, blank lines, .file / .loc / .ident
dropped, the function's ordinal in local labels — .LBB<n>_<m>, .Lfunc_end<n> — taken out, since it shifts when a kernel is
added in front) and the resource fields of the code object's metadata: vgpr_count, sgpr_count, sgpr_spill_count,
vgpr_spill_count, private_segment_fixed_size, group_segment_fixed_size.  Prints one line per kernel — "same", or the counts that
differ — and exits non-zero on any difference, a kernel present on one side only included.  It looks for nothing but equality.
"""
import re
import subprocess
import sys

FIELDS = ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
SKIP = (".file", ".loc", ".ident")


def parse(path):
    """-> {symbol: (instruction lines, {field: value})} of every kernel of an assembly file"""
    lines = open(path).read().split("\n")
    body, cur = {}, None
    for raw in lines:
        l = raw.split(";")[0].rstrip()
        if cur is None:
            m = re.match(r"^(\w+):\s*$", l)
            if m and not m.group(1).startswith(".L"):
                cur = m.group(1)
                body[cur] = []
            continue
        s = l.strip()
        if not s or s.split()[0] in SKIP:
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", s)).replace(cur, "<kernel>"))  # (its own symbol masked: --map)
    meta, name, fields = {}, None, {}
    for raw in lines:  # the metadata note: one "- .args: ... .name: sym ..." entry per kernel, keys sorted, the fields flat
        m = re.match(r"^\s+(?:- )?\.(\w+):\s*(\S*)\s*$", raw)
        if raw.startswith("  - .") and (name or fields):
            if name:
                meta[name] = fields
            name, fields = None, {}
        if not m:
            continue
        if m.group(1) == "name" and raw.startswith("    .name:"):
            name = m.group(2)
        elif m.group(1) in FIELDS and raw.startswith("    ."):
            fields[m.group(1)] = int(m.group(2))
    if name:
        meta[name] = fields
    return {k: (body.get(k, []), meta[k]) for k in meta}


def short(name):
    """a demangled kernel name as --map spells it: no return type, no argument list, no blanks"""
    return re.sub(r"\(.*", "", name).removeprefix("void ").replace(" ", "")


def main():
    argv, renames = sys.argv[1:], {}
    while "--map" in argv:  # --map OLD=NEW (repeatable): parent kernel OLD is compared against the new build's kernel NEW
        i = argv.index("--map")
        old, eq, new = (argv[i + 1] if i + 1 < len(argv) else "").partition("=")
        if not eq or not old or not new:
            raise SystemExit(__doc__)
        renames[short(old)] = short(new)
        del argv[i:i + 2]
    if len(argv) != 2:
        raise SystemExit(__doc__)
    path_a, path_b = argv
    a, b = parse(path_a), parse(path_b)
    if not a or not b:
        raise SystemExit("no kernels found in " + (path_a if not a else path_b))
    syms = sorted(set(a) | set(b))
    names = dict(zip(syms, subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")))
    for old, new in renames.items():  # the parent's kernel takes the new kernel's symbol, and is then compared like any other
        src = [k for k in a if short(names.get(k) or k) == old]
        dst = [k for k in b if short(names.get(k) or k) == new]
        if len(src) != 1 or len(dst) != 1 or (dst[0] in a and dst[0] != src[0]):
            raise SystemExit(f"--map {old}={new}: {len(src)} such kernels in {path_a}, {len(dst)} in {path_b} (need one each, and no {new} in the former)")
        a[dst[0]] = a.pop(src[0])
        names[dst[0]] = f"{old} -> {new}"
    syms = sorted(set(a) | set(b))
    n_diff = 0
    for k in syms:
        label = re.sub(r"\(.*", "", names.get(k) or k)[:110]
        if k not in a or k not in b:
            n_diff += 1
            print(f"DIFF  {label}: only in {path_b if k in b else path_a}")
            continue
        (ia, fa), (ib, fb) = a[k], b[k]
        what = [f"{f} {fa.get(f)} -> {fb.get(f)}" for f in FIELDS if fa.get(f) != fb.get(f)]
        if ia != ib:
            first = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            what.insert(0, f"instruction text ({len(ia)} -> {len(ib)} lines, first difference at line {first})")
        if what:
            n_diff += 1
            print(f"DIFF  {label}: " + "; ".join(what))
        else:
            print(f"same  {label}  [{len(ia)} lines, vgpr {fa.get('vgpr_count')}, sgpr {fa.get('sgpr_count')}, spills {fa.get('sgpr_spill_count')}/{fa.get('vgpr_spill_count')}, "
                  f"scratch {fa.get('private_segment_fixed_size')}, lds {fa.get('group_segment_fixed_size')}]")
    print(f"{len(syms)} kernels, {n_diff} differ")
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
