#!/usr/bin/env python3
"""Writes profiles/patch_d1_resources.txt: the resource figures of every kernel of csrc/rbt_color.hip (or of the files given with --src, each with the flags the
Makefile builds it with) at a parent commit against the working tree, from
hipcc -Rpass-analysis=kernel-resource-usage (cross-compiled for gfx950, no GPU needed). The parent's sources are taken with `git archive` into a temporary directory.

    python tools/patch_d1_resources.py --parent HEAD~1 --out profiles/patch_d1_resources.txt
    python tools/patch_d1_resources.py --parent HEAD --src csrc/rbt_kernels.hip csrc/rbt_color.hip --out profiles/metric_fold_resources.txt
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
FLAGS_OF = {"csrc/rbt_color.hip": FLAGS, "csrc/rbt_kernels.hip": ["--offload-arch=gfx950", "-std=c++17", "-O3", "-fPIC", "-Os", "-Rpass-analysis=kernel-resource-usage"]}      # as the Makefile builds them (rabbit-transcoding_amd/Makefile, the librbt.so rule: -Os for rbt_kernels.hip, COLOR_FLAGS for rbt_color.hip): keep in step with it


def remarks(tree, tmp, src="csrc/rbt_color.hip"):
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS_OF[src] + ["-c", src, "-o", os.path.join(tmp, "x.o")], cwd=os.path.join(tree, PKG), capture_output=True, text=True)
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
    ap.add_argument("--parent", default="HEAD"); ap.add_argument("--out", default=""); ap.add_argument("--src", nargs="+", default=["csrc/rbt_color.hip"], choices=sorted(FLAGS_OF))
    a = ap.parse_args()
    lines, same, compared = [], True, 0
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run("git archive %s | tar -x -C %s" % (a.parent, tmp), shell=True, check=True, cwd=ROOT)
        for src in a.src:
            old, new = remarks(tmp, tmp, src), remarks(ROOT, tmp, src)
            lines += ["Kernel resource usage of %s (hipcc %s), the parent commit against this change." % (src, " ".join(FLAGS_OF[src])), "",
                      "%-20s %-7s %5s %5s %5s %8s %6s %4s" % ("kernel", "build", "VGPR", "AGPR", "SGPR", "scratch", "LDS", "occ")]
            for n in sorted(set(old) | set(new), key=plain):
                for tag, have in (("parent", old), ("change", new)):
                    if n not in have:
                        lines.append("%-20s %-7s %s" % (plain(n), tag, "-  (new kernel)" if have is old else "-  (removed)")); continue
                    lines.append("%-20s %-7s %5s %5s %5s %8s %6s %4s" % ((plain(n), tag) + tuple(have[n].get(k, "?") for k in KEYS)))
                if n in old and n in new:
                    compared += 1
                    if old[n] != new[n]:
                        same = False; lines.append("  ^^^ DIFFERS")
            lines.append("")
    lines.append("kernels in both builds unchanged: %s (%d kernels compared, every remark field)" % (same, compared))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            f.write(text)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
