#!/usr/bin/env python3
"""Writes profiles/patch_d1_resources.txt: the resource figures of every kernel of csrc/rbt_color.hip at a parent commit against the working tree, from
hipcc -Rpass-analysis=kernel-resource-usage (cross-compiled for gfx950, no GPU needed). The parent's sources are taken with `git archive` into a temporary directory.

    python tools/patch_d1_resources.py --parent HEAD~1 --out profiles/patch_d1_resources.txt
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "rabbit-transcoding_amd"
KEYS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-O3", "-fPIC", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage"]


def remarks(tree, tmp):
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + ["-c", "csrc/rbt_color.hip", "-o", os.path.join(tmp, "x.o")], cwd=os.path.join(tree, PKG), capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1); out[name] = {}; continue
        m = re.search(r"remark:\s+([^:]+(?:\[[^\]]*\])?): (\S+) \[-Rpass", line)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    return out


def plain(n):
    return subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().split("(")[0].replace("rbtk::", "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD"); ap.add_argument("--out", default="")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run("git archive %s | tar -x -C %s" % (a.parent, tmp), shell=True, check=True, cwd=ROOT)
        old, new = remarks(tmp, tmp), remarks(ROOT, tmp)
    lines = ["Kernel resource usage of csrc/rbt_color.hip (hipcc %s), the parent commit against this change." % " ".join(FLAGS), "",
             "%-20s %-7s %5s %5s %5s %8s %6s %4s" % ("kernel", "build", "VGPR", "AGPR", "SGPR", "scratch", "LDS", "occ")]
    same = True
    for n in sorted(new, key=plain):
        for tag, src in (("parent", old), ("change", new)):
            if n not in src:
                lines.append("%-20s %-7s %s" % (plain(n), tag, "-  (new kernel)")); continue
            lines.append("%-20s %-7s %5s %5s %5s %8s %6s %4s" % ((plain(n), tag) + tuple(src[n].get(k, "?") for k in KEYS)))
        if n in old and old[n] != new[n]:
            same = False; lines.append("  ^^^ DIFFERS")
    lines += ["", "existing kernels unchanged: %s (%d kernels compared, every remark field)" % (same, len(old))]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            f.write(text)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
