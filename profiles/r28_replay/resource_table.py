#!/usr/bin/env python3
"""Tabulates a -Rpass-analysis=kernel-resource-usage log of navsim_kernels.hip for the kernels that share
kernels_replay.hpp: one line per kernel form.  Usage: resource_table.py LOG [LOG2]; with two logs, also lists
the forms whose occupancy, scratch, VGPR spills or static LDS differ (there must be none)."""
import re
import subprocess
import sys

KERNELS = ("lookahead_kernel", "lookahead_obs_kernel", "rollout_kernel", "rollout_obs_kernel", "ped_forecast_kernel",
           "scan_labels_kernel")
FIELDS = (("VGPRs", "vgpr"), ("Occupancy [waves/SIMD]", "occ"), ("ScratchSize [bytes/lane]", "scratch"),
          ("VGPRs Spill", "vspill"), ("SGPRs Spill", "sspill"), ("LDS Size [bytes/block]", "lds"))
HELD = ("occ", "scratch", "vspill", "lds")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return out.splitlines()


def parse(path):
    forms, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = forms.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m:
                cur[key] = int(m.group(1))
    names = list(forms)
    table = {}
    for mangled, plain in zip(names, demangle(names)):
        m = re.search(r"::(\w+)<(.*?)>\(", plain)
        if m and m.group(1) in KERNELS:
            form = m.group(2).replace("(anonymous namespace)::", "")
            table[(m.group(1), form)] = forms[mangled]
    return table


def show(table):
    print("%-22s %-28s %5s %4s %8s %7s %7s %6s" % ("kernel", "form", "VGPRs", "occ", "scratch", "Vspill", "Sspill", "LDS"))
    for (kernel, form), r in sorted(table.items(), key=lambda kv: (KERNELS.index(kv[0][0]), kv[0][1])):
        print("%-22s %-28s %5d %4d %8d %7d %7d %6d" % (kernel, form, r["vgpr"], r["occ"], r["scratch"], r["vspill"],
                                                      r["sspill"], r["lds"]))


if __name__ == "__main__":
    a = parse(sys.argv[1])
    show(a)
    if len(sys.argv) > 2:
        b = parse(sys.argv[2])
        print()
        show(b)
        bad = [(k, key, a[k][key], b[k][key]) for k in sorted(a) if k in b for key in HELD if a[k][key] != b[k][key]]
        missing = sorted(set(a) ^ set(b))
        print("\nforms: %d and %d; only in one log: %s" % (len(a), len(b), missing or "none"))
        print("differences in occupancy / scratch / VGPR spills / static LDS: %s" % (bad or "none"))
        sys.exit(1 if bad or missing else 0)
