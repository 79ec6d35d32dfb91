#!/usr/bin/env python3
"""Writes profiles/patch_color_resources.txt: what the colour figures per patch changed in the device code, the parent commit against the working tree, cross-compiled
for gfx950 (no GPU needed).

  1. every .hip file of the Makefile's librbt.so rule other than csrc/rbt_color.hip, compiled with that rule's flags in both trees: the objects are compared bytewise;
  2. csrc/rbt_color.hip: the resource remarks of every kernel (tools/patch_d1_resources.py: VGPR, AGPR, SGPR, scratch, LDS, occupancy) in both trees - the kernels that exist
     in both must keep every field - and the new kernel's own figures, with a line that says whether it spills.

    python tools/patch_color_resources.py --parent HEAD --out profiles/patch_color_resources.txt
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patch_d1_resources as PR

ROOT, PKG = PR.ROOT, PR.PKG
BASE = ["--offload-arch=gfx950", "-std=c++17", "-O3", "-fPIC", "-Wall", "-Wno-unused-function"]
# as the Makefile builds them (rabbit-transcoding_amd/Makefile, the librbt.so rule): keep in step with it
OTHERS = {"csrc/rbt_kernels_parse.hip": [], "csrc/rbt_kernels.hip": ["-Os"], "csrc/rbt_hash.hip": [], "csrc/rbt_normals.hip": ["-ffp-contract=off"], "csrc/rbt_rate.hip": [],
          "csrc/rbt_quality.hip": [], "csrc/rbt_cloudmaps.hip": []}
NEW = "k_pc_sums"


def object_hash(tree, tmp, src, extra):
    out = os.path.join(tmp, "o.o")
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + BASE + extra + ["-c", src, "-o", out], cwd=os.path.join(tree, PKG), capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    with open(out, "rb") as f:
        b = f.read()
    return hashlib.sha256(b).hexdigest(), len(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD"); ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines, ok = [], True
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run("git archive %s | tar -x -C %s" % (a.parent, tmp), shell=True, check=True, cwd=ROOT)
        lines += ["Device objects other than csrc/rbt_color.hip's (hipcc %s and the Makefile's flags per file), the parent commit against this change, compared bytewise." % " ".join(BASE), "",
                  "%-28s %10s  %-16s %-16s %s" % ("object of", "bytes", "sha256 parent", "sha256 change", "")]
        for src, extra in OTHERS.items():
            (h0, n0), (h1, n1) = object_hash(tmp, tmp, src, extra), object_hash(ROOT, tmp, src, extra)
            same = h0 == h1 and n0 == n1
            ok &= same
            lines.append("%-28s %10d  %-16s %-16s %s" % (src, n1, h0[:16], h1[:16], "identical" if same else "DIFFERS"))
        lines.append("")
        old, new = PR.remarks(tmp, tmp), PR.remarks(ROOT, tmp)
        lines += ["Kernel resource usage of csrc/rbt_color.hip (hipcc %s)." % " ".join(PR.FLAGS), "", "%-20s %-7s %5s %5s %5s %8s %6s %4s" % ("kernel", "build", "VGPR", "AGPR", "SGPR", "scratch", "LDS", "occ")]
        compared = 0
        for n in sorted(set(old) | set(new), key=PR.plain):
            for tag, have in (("parent", old), ("change", new)):
                if n not in have:
                    lines.append("%-20s %-7s %s" % (PR.plain(n), tag, "-  (new kernel)" if have is old else "-  (removed)")); continue
                lines.append("%-20s %-7s %5s %5s %5s %8s %6s %4s" % ((PR.plain(n), tag) + tuple(have[n].get(k, "?") for k in PR.KEYS)))
            if n in old and n in new:
                compared += 1
                if old[n] != new[n]:
                    ok = False; lines.append("  ^^^ DIFFERS")
        lines += ["", "kernels in both builds unchanged: %s (%d kernels compared, every remark field)" % (all(old[n] == new[n] for n in old if n in new), compared)]
        for n in new:
            if PR.plain(n) == NEW:
                r = new[n]
                lines.append("%s: %s VGPRs, %s SGPRs, %s bytes of scratch per lane (%s), %s bytes of LDS, occupancy %s waves per SIMD" % (
                    NEW, r.get(PR.KEYS[0]), r.get(PR.KEYS[2]), r.get(PR.KEYS[3]), "no spill" if r.get(PR.KEYS[3]) == "0" else "SPILLS", r.get(PR.KEYS[4]), r.get(PR.KEYS[5])))
    lines.append("other objects bytewise identical and existing kernels unchanged: %s" % ok)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
