"""bench_ab.py DIR: medians and ranges of the bench.py result lines DIR/bench_{plain,full}_{parent,new}_<i>.json, the lines that go
through staged worlds and their host time: one row per figure, PARENT's median and range, NEW's median and range, and whether
NEW's median lies inside PARENT's range."""
import glob
import json
import statistics
import sys


def figures(d):
    """{name: number} of one result line: the headline, the pipelined c5 lines, the next-step line, the reference-default lines"""
    out = {"headline value": d["value"]}
    for k, w in d.get("other_workloads", {}).items():
        if k.startswith("c5_"):
            out[k + " value"] = w["value"]
            if "host_ms_per_step" in w:
                out[k + " host_ms_per_step"] = w["host_ms_per_step"]
    for k, w in d.get("gym_api", {}).get("reference_defaults", {}).items():
        if isinstance(w, dict) and "value" in w:
            out[k + " value"] = w["value"]
            if "host_ms_per_step" in w:
                out[k + " host_ms_per_step"] = w["host_ms_per_step"]
    return out


def main(where):
    for tag in ("plain", "full"):
        runs = {}
        for tree in ("parent", "new"):
            files = sorted(glob.glob("%s/bench_%s_%s_*.json" % (where, tag, tree)))
            runs[tree] = [figures(json.loads([ln for ln in open(f) if ln.startswith("{")][-1])) for f in files]
        if not runs["parent"]:
            continue
        print("bench.py --gpus 1 --steps 200 --warmup 20%s: %d PARENT and %d NEW runs, alternating"
              % (" --full" if tag == "full" else "", len(runs["parent"]), len(runs["new"])))
        for name in runs["parent"][0]:
            a, b = ([r[name] for r in runs[t] if name in r] for t in ("parent", "new"))
            ma, mb = statistics.median(a), statistics.median(b)
            print("  %-52s PARENT %.6g (%.6g .. %.6g)  NEW %.6g (%.6g .. %.6g)  %s" % (
                name, ma, min(a), max(a), mb, min(b), max(b), "inside" if min(a) <= mb <= max(a) else "OUTSIDE PARENT'S RANGE"))


if __name__ == "__main__":
    main(sys.argv[1])
