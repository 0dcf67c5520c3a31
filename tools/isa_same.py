#!/usr/bin/env python3
"""Whether two builds of a HIP unit are the same machine code, kernel by kernel (no GPU needed).

    hipcc <the library's flags> -S --cuda-device-only ffx_trace.hip -o parent.s     (once per tree)
    python tools/isa_same.py parent.s new.s

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
        body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", s)))
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


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    if not a or not b:
        raise SystemExit("no kernels found in " + (sys.argv[1] if not a else sys.argv[2]))
    syms = sorted(set(a) | set(b))
    names = dict(zip(syms, subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")))
    n_diff = 0
    for k in syms:
        label = re.sub(r"\(.*", "", names.get(k) or k)[:110]
        if k not in a or k not in b:
            n_diff += 1
            print(f"DIFF  {label}: only in {sys.argv[2] if k in b else sys.argv[1]}")
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
