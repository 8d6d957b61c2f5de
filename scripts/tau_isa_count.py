#!/usr/bin/env python3
"""ISA-level instruction counts of one tau_kernel instantiation by phase and loop depth (the tables of profiles/r06_tau_isa_counts.txt
and profiles/tau_lean2_isa_counts.txt), with the machinery of scripts/isa_count.py: kernels_gibbs.hip is compiled for gfx950 with
-DDSM_ISA_MARKS (dsm_device.h: ISA_MARK; marks in tau_body, sweep_screen and sweep_screen32) and every instruction is charged to the last
mark seen in layout order.  Depth 0 = once per wavefront, 1 = per variant, 2 = per (variant, haplotype) step, 3 = inner loops.

usage: tau_isa_count.py [--src PATH] [--extra "-DX ..."] [--kernel REGEX]"""
import argparse
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_count as ic

SCREENED = ("step_setup", "screen_prefix_cvt", "screen_links", "screen_candidates", "screen_reduce", "screen_certify", "step_commit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ic.ROOT, "desman_amd", "csrc", "kernels_gibbs.hip"))
    ap.add_argument("--extra", default="")
    ap.add_argument("--kernel", default=r"_Z10tau_kernelILi32ELi2ELb1ELb1EEv9TauParams", help="regex of the mangled kernel name")
    a = ap.parse_args()
    name, lines = ic.kernel_body(ic.compile_asm(a.src, a.extra.split(), True), a.kernel)
    tab, ops = {}, collections.defaultdict(collections.Counter)
    for b in ic.blocks(lines):
        ic.add(tab.setdefault((b["phase"], b["depth"]), {}), ic.tally(b["ops"]))
        if b["depth"] >= 2:
            ops[b["phase"]].update(b["ops"])
    print("# %s  %s" % (name, a.extra))
    print("%-22s %5s %6s %6s %6s %5s %5s %6s" % ("phase", "depth", "valu", "fp64", "salu", "lds", "vmem", "branch"))
    for ph, d in sorted(tab):
        t = tab[(ph, d)]
        print("%-22s %5d %6d %6d %6d %5d %5d %6d" % (ph, d, t.get("valu", 0), t.get("valu_fp64", 0), t.get("salu", 0), t.get("lds", 0), t.get("vmem", 0), t.get("branch", 0)))
    for ph in SCREENED:
        print(ph, dict(ops[ph].most_common(16)))
    n = sum(k for ph in SCREENED for o, k in ops[ph].items() if o.startswith(("v_cvt_f32_f64", "v_fma_f64", "v_fmac_f64")))
    print("v_cvt_f32_f64 + v_fma_f64 / v_fmac_f64 in the screened path (%s; depth >= 2): %d" % (", ".join(SCREENED), n))


if __name__ == "__main__":
    main()
