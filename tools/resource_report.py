#!/usr/bin/env python3
"""Compare two `-Rpass-analysis=kernel-resource-usage` logs of the engine.

    hipcc ... -Rpass-analysis=kernel-resource-usage pencilhip.hip 2> new.log
    python tools/resource_report.py [--none-policy NAME] parent.log new.log

``--none-policy NAME`` (repeatable) compares by demangled name with every
``, NAME`` dropped: a kernel that gained a defaulted policy template parameter
is then matched with its parent form under the policy's "none" instance NAME.

Prints one line per kernel (demangled name, SGPRs, VGPRs, AGPRs, scratch
bytes per lane, occupancy, spills, LDS bytes), the kernels only the second
log has, and every kernel whose figures differ between the two.  Exits 1
when an existing kernel moved or a new kernel has scratch or spills.
"""

import re
import subprocess
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]",
          "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]
SHORT = ["sgpr", "vgpr", "agpr", "scratch", "occ", "sspill", "vspill", "lds"]


def parse(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
        if m and name and m.group(1) in FIELDS:
            out[name][m.group(1)] = m.group(2)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), text=True,
                           capture_output=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def row(v):
    return " ".join(f"{s}={v.get(f, '?')}" for s, f in zip(SHORT, FIELDS))


def rekey(table, dm, none):
    """Key ``table`` by demangled name with every ``, POLICY`` of ``none``
    dropped, so that a kernel which only gained a defaulted policy parameter
    meets its parent form under that parameter's "none" instance."""
    out = {}
    for n, v in table.items():
        k = dm[n]
        for pol in none:
            k = k.replace(", " + pol, "")
        out[k] = v
    return out


def main():
    args = sys.argv[1:]
    none = []   # --none-policy NAME, repeatable
    while "--none-policy" in args:
        i = args.index("--none-policy")
        none.append(args[i + 1])
        del args[i:i + 2]
    old, new = parse(args[0]), parse(args[1])
    dm = demangle(sorted(set(old) | set(new)))
    if none:
        old, new = rekey(old, dm, none), rekey(new, dm, none)
        dm = {k: k for k in set(old) | set(new)}
    bad = 0
    moved = [n for n in old if n in new and old[n] != new[n]]
    gone = [n for n in old if n not in new]
    added = [n for n in new if n not in old]
    print("# hipcc --offload-arch=gfx950 -O3 -std=c++17 "
          "-Rpass-analysis=kernel-resource-usage pencilhip.hip, parent "
          "against this change (tools/resource_report.py)")
    print(f"kernels: parent {len(old)}, this change {len(new)}; "
          f"moved {len(moved)}, removed {len(gone)}, added {len(added)}")
    for n in moved:
        bad = 1
        print(f"MOVED {dm[n]}\n  parent: {row(old[n])}\n  now:    {row(new[n])}")
    for n in gone:
        bad = 1
        print(f"REMOVED {dm[n]}")
    print("\nadded kernels:")
    for n in added:
        v = new[n]
        if (v.get(FIELDS[3]) != "0" or v.get(FIELDS[5]) != "0"
                or v.get(FIELDS[6]) != "0"):
            bad = 1
        print(f"  {dm[n]}\n    {row(v)}")
    print("\nexisting kernels (identical in both logs):")
    for n in old:
        if n in new and old[n] == new[n]:
            print(f"  {dm[n]}\n    {row(new[n])}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
