#!/usr/bin/env python3
"""Reduce hipcc's -Rpass-analysis=kernel-resource-usage remarks to one markdown table row per kernel instantiation.

    hipcc ... -Rpass-analysis=kernel-resource-usage -c bm25_probe.hip -o /dev/null 2> probe.log
    python tools/resource_table.py bm25_probe_kernel probe.log [other.log ...]

With two logs per translation unit (parent first, branch second: `--pair`) the rows show both side by side."""
import re
import subprocess
import sys

FIELDS = [("VGPRs", "VGPRs"), ("SGPRs Spill", "SGPR spill"), ("VGPRs Spill", "VGPR spill"), ("ScratchSize [bytes/lane]", "scratch B/lane"),
          ("Occupancy [waves/SIMD]", "occupancy")]


def parse(path, prefix):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: (?:\s*)Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[-Rpass", line)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    names = sorted(out)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    res = {}
    for n, d in zip(names, dem):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(.*$", "", d)
        if d.startswith(prefix):
            res[d] = out[n]
    return res


def main():
    args = [a for a in sys.argv[1:] if a != "--pair"]
    pair = "--pair" in sys.argv
    prefix, logs = args[0], args[1:]
    tabs = [parse(p, prefix) for p in logs]
    if pair:
        assert len(tabs) == 2
        print("| kernel | " + " | ".join(f"{h} (parent -> branch)" for _, h in FIELDS) + " |")
        print("|---|" + "---|" * len(FIELDS))
        for k in sorted(set(tabs[0]) | set(tabs[1])):
            a, b = tabs[0].get(k, {}), tabs[1].get(k, {})
            print(f"| `{k}` | " + " | ".join(f"{a.get(f, '-')} -> {b.get(f, '-')}" for f, _ in FIELDS) + " |")
    else:
        print("| kernel | " + " | ".join(h for _, h in FIELDS) + " |")
        print("|---|" + "---|" * len(FIELDS))
        for t in tabs:
            for k in sorted(t):
                print(f"| `{k}` | " + " | ".join(t[k].get(f, "-") for f, _ in FIELDS) + " |")


if __name__ == "__main__":
    main()
