#!/usr/bin/env python3
"""Compare the gfx950 assembly of two builds of one .hip file, kernel by kernel and whole.

    python tools/asm_compare.py PARENT.s NEW.s [label] [--rename OLD=NEW ...]

Both files come from `hipcc <flags of build.py> --save-temps -x hip -c csrc/FILE.hip` with the source at one and the same path (the
*-hip-amdgcn-amd-amdhsa-gfx950.s file).  Names are masked where a refactor may change them: the dump page, the compilation-unit id, and
the function index of a basic-block label (.LBB<function>_<block> is compared as .LBB_<block>: the index counts the functions in front
of the kernel, so removing or adding one above it renumbers every label below; the block number still counts).  Everything else counts.  A kernel whose instruction stream differs is listed with its per-mnemonic histogram and its resource
metadata next to the parent's; "renumbered" means equal histogram and equal metadata.  --rename OLD=NEW reads the parent's file with the
(mangled) symbol OLD spelled NEW, so that a kernel the refactor renamed is compared with its successor.  Exit status 1 when any kernel
differs."""
import argparse
import collections
import re
import sys

KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def mask(line):
    line = line.split(";")[0].rstrip()
    line = re.sub(r"_ZN12_GLOBAL__N_1\d+g_\w*dump\w*E|_ZL\d+g_dump_page", "DUMP", line)
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)          # a block label counts the functions in front of it: a kernel removed above renumbers it
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", line)


def parse(path, renames=()):
    """kernel name -> its instruction lines; kernel name -> resource metadata; all masked lines"""
    text = open(path).read()
    for old, new in renames:
        text = re.sub(r"\b%s\b" % re.escape(old), new, text)
    named = set(re.findall(r"^\s+\.name:\s+(_Z\w+)\s*$", text, re.M))      # the kernels of the metadata: a static one is _ZL...
    text = text.split("\n")
    body, meta, cur, entry = collections.OrderedDict(), {}, None, None
    for ln in text:
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None and (m.group(1) in named or not m.group(1).startswith("_ZL")):
            cur = m.group(1)
            body[cur] = []
        elif cur is not None:
            if ln.startswith(".Lfunc_end"):
                cur = None
            else:
                s = mask(ln).strip()
                if s and not s.startswith(".p2align"):
                    body[cur].append(s)
        if re.match(r"  - \.agpr_count:", ln):
            entry = {}
        if entry is not None:
            for key in KEYS:
                mm = re.match(r"\s+(- )?%s:\s+(\d+)" % re.escape(key), ln)
                if mm:
                    entry[key] = int(mm.group(2))
            mm = re.match(r"\s+\.name:\s+(_Z\w+)\s*$", ln)
            if mm:
                meta[mm.group(1)] = entry
    kernels = collections.OrderedDict((k, v) for k, v in body.items() if k in meta)      # (a global data symbol has a label too)
    return kernels, meta, [mask(x) for x in text]


def histogram(lines):
    return collections.Counter(s.split()[0] for s in lines if not s.endswith(":") and not s.startswith("."))


def main():
    def pair(text):
        old, eq, new = text.partition("=")
        if not (old and eq and new):
            raise argparse.ArgumentTypeError("expected OLD=NEW, got %r" % text)
        return old, new
    ap = argparse.ArgumentParser(description="compare the gfx950 assembly of two builds of one .hip file")
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("label", nargs="?")
    ap.add_argument("--rename", action="append", type=pair, default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    pa, ma, la = parse(args.parent, args.rename)
    pb, mb, lb = parse(args.new)
    label = args.label or args.new
    missing = [k for k in pa if k not in pb] + [k for k in pb if k not in pa]
    renumbered, different = [], []
    for k in pa:
        if k not in pb or (pa[k] == pb[k] and ma.get(k) == mb.get(k)):
            continue
        ha, hb = histogram(pa[k]), histogram(pb[k])
        (renumbered if ha == hb and ma.get(k) == mb.get(k) else different).append((k, ha, hb))
    n_ins = sum(sum(histogram(v).values()) for v in pb.values())
    if not missing and not renumbered and not different:
        rest = [(x.strip(), y.strip()) for x, y in zip(la, lb) if x != y]
        print("%s: identical: %d instructions in %d kernels, %d lines of assembly%s" % (
            label, n_ins, len(pb), len(lb), "" if not rest else "; %d data lines differ: %s" % (len(rest), "; ".join("%s -> %s" % r for r in rest))))
        return 0
    print("%s: %d kernels, %d renumbered (equal histogram and metadata), %d DIFFERENT; kernels on one side only: %s; lines: %d against %d" % (
        label, len(pb), len(renumbered), len(different), missing or "none", len(la), len(lb)))
    for k, ha, hb in renumbered + different:
        print("  %s %s" % ("renumbered" if (k, ha, hb) in renumbered else "DIFFERENT ", k))
        print("     parent %s" % " ".join("%s=%s" % (key[1:], ma.get(k, {}).get(key)) for key in KEYS))
        print("     new    %s" % " ".join("%s=%s" % (key[1:], mb.get(k, {}).get(key)) for key in KEYS))
        for op in sorted(set(ha) | set(hb)):
            if ha[op] != hb[op]:
                print("     %-26s parent %6d  new %6d" % (op, ha[op], hb[op]))
    return 1 if different or missing else 0


if __name__ == "__main__":
    sys.exit(main())
