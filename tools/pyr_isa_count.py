#!/usr/bin/env python3
"""VALU counts of k_pyr_rows from its gfx950 assembly, by loop depth.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I include --cuda-device-only \
        -S -x hip multicol-slam-annotation_amd/csrc/k_pyramid.hip -o k_pyramid.s
  tools/pyr_isa_count.py k_pyramid.s

Per instantiation it splits the basic blocks by the loop comments the compiler leaves
("in Loop: Header=... Depth=n"): depth 0 runs once per wave (setup, both vertical forms'
prologues included although a wave runs one), depth 1 is the source-row loop (kPF unrolled
slots), depth 2 the output rows of one source row (RESIZE only).  Inside a row's blocks the
ones that hold the border emit (the only users of v_cndmask between a v_lshlrev of the window
and the blur store) are rare paths; they are reported apart as "border" by the marker below.
Prints one JSON object.
"""
import json
import re
import sys

KPF = 6


def kernels(text):
    out, name, buf = {}, None, []
    for ln in text.split("\n"):
        m = re.match(r"^(_ZN3mcs10k_pyr_rowsILb([01])ELi(\d)EEEvNS_7PyrArgsE):", ln)
        if m:
            name, buf = "k_pyr_rows<%s, %s>" % ("true" if m.group(2) == "1" else "false", m.group(3)), []
            continue
        if name:
            if ln.startswith("\t.section"):
                out[name], name = buf, None
                continue
            buf.append(ln)
    return out


def blocks(lines):
    """[(label, depth, header, [instructions])]"""
    res, cur = [], ["entry", 0, None, []]
    for ln in lines:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", ln)
        if m:
            res.append(tuple(cur))
            d = re.search(r"Depth=(\d)", m.group(2))
            h = re.search(r"Header[:=] ?(BB\d+_\d+)?", m.group(2))
            inner = "Inner Loop Header" in m.group(2) or "Loop Header" in m.group(2)
            cur = [m.group(1), int(d.group(1)) if d else 0,
                   m.group(1)[2:] if inner else (h.group(1) if h and h.group(1) else None), []]
            continue
        s = ln.strip()
        if s and not s.startswith((";", ".")):
            cur[3].append(s.split()[0])
    res.append(tuple(cur))
    return res


def is_valu(op):
    return op.startswith("v_") and not op.startswith(("v_readlane", "v_readfirstlane"))


def count(lines):
    bl = blocks(lines)
    by_depth = {0: 0, 1: 0, 2: 0}
    border = {1: 0, 2: 0}
    loops = {}
    for label, depth, header, ins in bl:
        n = sum(is_valu(o) for o in ins)
        d = min(depth, 2)
        # the border emit is the only code that selects (v_cndmask) window rows by weight bits
        if d and sum(o.startswith("v_cndmask") for o in ins) >= 8:
            border[d] += n
        else:
            by_depth[d] += n
        if d:
            loops.setdefault((d, header), 0)
            loops[(d, header)] += 0 if sum(o.startswith("v_cndmask") for o in ins) >= 8 else n
    return by_depth, border, loops


def main():
    ks = kernels(open(sys.argv[1]).read())
    out = {}
    for name, lines in sorted(ks.items()):
        by_depth, border, loops = count(lines)
        resize = "true" in name
        d1 = [v for (d, _), v in loops.items() if d == 1]
        d2 = [v for (d, _), v in loops.items() if d == 2]
        e = {"valu_once_per_wave": by_depth[0],
             "valu_source_row_loop_all_slots": sum(d1), "source_row_loops": len(d1),
             "valu_border_emit_blocks": border[1] + border[2]}
        if resize:
            # two forms x kPF slots of each loop
            e["valu_output_row_loops_all_slots"] = sum(d2)
            e["output_row_loops"] = len(d2)
            e["valu_per_output_row"] = round(sum(d2) / max(len(d2), 1), 1)
            e["valu_per_source_row"] = round(sum(d1) / (KPF * max(len(d1), 1)), 1)
        else:
            e["valu_per_output_row"] = round(sum(d1) / (KPF * max(len(d1), 1)), 1)
        out[name] = e
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
