#!/usr/bin/env python3
"""Resource table of the encoder kernels, two builds side by side (no GPU needed).

    hipcc --offload-arch=gfx950 -std=c++17 -O3 -fPIC -Os --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
        csrc/rbt_kernels.hip -o kernels.s 2> res.log        # once in each tree (the Makefile's flags for this file)
    tools/qp_map_resources.py parent/res.log change/res.log [parent/kernels.s change/kernels.s]

Prints, for every kernel whose name contains k_enc_ or k_entropy, what the compiler reports - SGPRs, VGPRs, scratch bytes per lane, spills, LDS bytes per workgroup,
waves per SIMD - for both builds, with the instruction count of the kernel's assembly when the .s files are given, and marks every figure that grew. The change's constant-QP instantiations (<.., false>) stand
in the row of the parent's kernel of that name; a kernel only one build has - the map instantiations, k_enc_qp_fix - is listed with the other side empty. The figures of a run are kept in profiles/qp_map.txt."""
import re
import subprocess
import sys

KEYS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("SGPRs Spill", "s_spill"), ("VGPRs Spill", "v_spill"),
        ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ")]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, short in KEYS:
            m = re.search(r"remark:\s+" + re.escape(key) + r": (\d+)", line)
            if m:
                cur[short] = int(m.group(1))
    return out


def instructions(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = 0
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur and re.match(r"^\t[a-z]", line):
            out[cur] += 1
    return out


def demangle(names):
    try:
        txt = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: re.sub(r"\(.*", "", re.sub(r"^(void )?rbtk::", "", t)) for n, t in zip(names, txt)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def plain(name):
    """the constant-QP instantiation under the name the parent build has for it: k<5, false> -> k<5>, k<false> -> k (the map instantiations, <.., true>, keep their names)"""
    return re.sub(r"<false>$", "", re.sub(r", false>$", ">", name))


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    ia, ib = (instructions(sys.argv[3]), instructions(sys.argv[4])) if len(sys.argv) > 4 else ({}, {})
    names = sorted(n for n in set(a) | set(b) if "k_enc_" in n or "k_entropy" in n)
    pretty = demangle(names)
    rows = {}      # kernel -> [parent figures, change figures]
    parent_names = {pretty[n] for n in names if n in a}
    for n in names:
        for side, (res, ins) in enumerate(((a, ia), (b, ib))):
            if n in res:
                r = dict(res[n])
                if n in ins: r["insts"] = ins[n]
                # (a parent from before the map instantiations has k<5> where the change has k<5, false>; a later parent has the same names as the change)
                name = plain(pretty[n]) if side and pretty[n] not in parent_names and plain(pretty[n]) in parent_names else pretty[n]
                rows.setdefault(name, [{}, {}])[side] = r
    cols = [s for _, s in KEYS] + (["insts"] if ia else [])
    print("%-28s %s" % ("kernel (parent -> change)", " ".join("%13s" % c for c in cols)))
    grew = 0
    for k in sorted(rows):
        ra, rb = rows[k]
        cells = []
        for c in cols:
            va, vb = ra.get(c), rb.get(c)
            worse = va is not None and vb is not None and (vb < va if c == "occ" else vb > va)
            grew += worse
            cells.append("%13s" % ("%s->%s%s" % ("-" if va is None else va, "-" if vb is None else vb, "!" if worse else "")))
        print("%-28s %s" % (k[:28], " ".join(cells)))
    print("figures of an existing instantiation that grew (marked !): %d" % grew)
    return 1 if grew else 0


if __name__ == "__main__":
    sys.exit(main())
