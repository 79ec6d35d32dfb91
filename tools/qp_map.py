#!/usr/bin/env python3
"""Measures the QP per CTB (rbt_transcode_gof_qp_map, include/rbt.h "a QP per CTB") on the benchmark GOF - the committed 1280x1280 32-frame fixture
(tests/golden/hm_r5_1280x1280_f32_*.annexb) transcoded to R3 - on one GPU. The measurement is a child process of its own with a time limit; the tool itself never opens the GPU.

  constant  rbt_transcode_gof
  uniform   every CTB of the geometry / attribute entry at the entry's QP: what the PPS flag and the zero deltas cost in bytes, what the map instantiations, the upload and
            the two launches of k_enc_qp_fix cost in time
  patches   rbt_qp_map_from_patches: the CTBs a patch meets at the entry's QP, the background at + 10
  patch0    the same with patch 0 of every frame at - 6
Per run: the bytes of the geometry and the attribute stream; the luma PSNR against the decoded input over the whole stream, over the CTBs a patch meets, over the background
CTBs and over the CTBs patch 0 meets; --samples wall times, the four calls interleaved in one process. Patches: synth.atlas_patches of the four base atlases; frames 4..31 are
those atlases rolled by a few pixels, their rectangles are not rolled with them (a CTB is 32 samples). All samples are kept. No threshold is set.

    python tools/qp_map.py --out FILE
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LIMIT_S = 560
W = H = 1280
SEED = 1051
GEO_QP, ATTR_QP = 24, 32          # R3
L2 = 5


def fixture():
    return [open(os.path.join(GOLD, "hm_r5_1280x1280_f32_%s.annexb" % k), "rb").read() for k in ("occ", "geo", "attr")]


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import rbt_lib
    import synth
    R = rbt_lib.module(); ctx = R.Context(device=0)
    src = fixture()
    P = [R.StreamParams(0, 8, 4, L2, -1, 0, 0, 0, 0), R.StreamParams(1, GEO_QP, 4, L2, -1, 0, 0, 0, 0), R.StreamParams(19, ATTR_QP, 4, L2, -1, 0, 0, 0, 0)]
    dec_in = [None] + [ctx.decode(s, verify_md5=False)[0] for s in src[1:]]
    n_pc = dec_in[1].shape[0] // 2
    ctb = 1 << L2; wc, hc = W // ctb, H // ctb
    atlas = R.AtlasParams(W, H, 16, 4, 2, 1, 1, 0)
    pats = [synth.atlas_patches(R, W, H, SEED + f % 4) for f in range(n_pc)]

    def from_patches(qp, first):
        return np.stack([R.qp_map_from_patches(atlas, p, [first] + [qp] * (len(p) - 1), min(51, qp + 10), L2, lib=ctx.L) for p in pats])
    maps = {"constant": None}
    for name in ("uniform", "patches", "patch0"):
        maps[name] = [None] + [np.full((n_pc, hc, wc), qp, np.int8) if name == "uniform" else from_patches(qp, qp - 6 if name == "patch0" else qp) for qp in (GEO_QP, ATTR_QP)]
    # regions, per frame and CTB: a patch meets it / background / patch 0 meets it (the same for both entries)
    in_patch = maps["patches"][1] == GEO_QP; in_p0 = maps["patch0"][1] == GEO_QP - 6
    regions = {"all": np.ones_like(in_patch), "patches": in_patch, "background": ~in_patch, "patch0": in_p0}
    calls = {k: (lambda m=m: ctx.transcode_gof(src, P) if m is None else ctx.transcode_gof_qp_map(src, P, m)) for k, m in maps.items()}

    def psnr(ref, got, sel):
        d = (ref[:, :W * H].astype(np.int32) - got[:, :W * H].astype(np.int32)).reshape(-1, hc, ctb, wc, ctb) ** 2
        sse = d.sum(axis=(2, 4), dtype=np.int64)[np.repeat(sel, 2, axis=0)].sum(); n = int(np.repeat(sel, 2, axis=0).sum()) * ctb * ctb
        return None if not n else (99.0 if sse == 0 else 10 * np.log10(1023.0 ** 2 * n / sse))
    rec = {"runs": {}, "ms": {k: [] for k in calls}, "ctbs": {k: int(v.sum()) for k, v in regions.items()}}
    for k, f in calls.items():
        outs = f()
        rec["runs"][k] = {"bytes": [len(outs[1]), len(outs[2])], "psnr": {}}
        for i, name in ((1, "geometry"), (2, "attribute")):
            got = ctx.decode(outs[i], verify_md5=False)[0]
            rec["runs"][k]["psnr"][name] = {r: psnr(dec_in[i], got, sel) for r, sel in regions.items()}
        if k == "constant":
            const = outs
    rec["no_map_equals_constant"] = ctx.transcode_gof_qp_map(src, P, [None] * 3) == const
    for _ in range(a.samples):
        for k, f in calls.items():
            t0 = time.perf_counter(); f(); rec["ms"][k].append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    print("RESULT " + json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--samples", str(a.samples)], capture_output=True, text=True, timeout=LIMIT_S)
    line = next((x for x in r.stdout.splitlines() if x.startswith("RESULT ")), None)
    if r.returncode or line is None:
        sys.stderr.write(r.stdout + r.stderr); sys.exit(1)
    rec = json.loads(line[7:])
    c = rec["runs"]["constant"]["bytes"]
    text = ["qp_map: a QP per CTB on the benchmark GOF (1280x1280, 32 frames), R3 (geometry QP %d, attribute QP %d), CTBs of %d, %d samples a time" % (GEO_QP, ATTR_QP, 1 << L2, a.samples),
            "CTBs per stream (frames x rows x columns): all %d, a patch meets %d, background %d, patch 0 meets %d" % tuple(rec["ctbs"][k] for k in ("all", "patches", "background", "patch0")),
            "a call with no map equals rbt_transcode_gof byte for byte: %s" % rec["no_map_equals_constant"]]
    fmt = lambda v: "   -  " if v is None else "%6.2f" % v
    for k in ("constant", "uniform", "patches", "patch0"):
        g = rec["runs"][k]; ms = rec["ms"][k]
        text.append("%-9s geometry %8d B (%+7d, %.4f)  attribute %8d B (%+7d, %.4f)  median %.1f ms  samples %s" % (
            k, g["bytes"][0], g["bytes"][0] - c[0], g["bytes"][0] / c[0], g["bytes"][1], g["bytes"][1] - c[1], g["bytes"][1] / c[1], statistics.median(ms), " ".join("%.1f" % x for x in ms)))
        for name in ("geometry", "attribute"):
            p = g["psnr"][name]
            text.append("          %-9s luma PSNR dB: all %s  patch CTBs %s  background CTBs %s  patch 0 CTBs %s" % (name, fmt(p["all"]), fmt(p["patches"]), fmt(p["background"]), fmt(p["patch0"])))
    med = {k: statistics.median(v) for k, v in rec["ms"].items()}
    text.append("uniform - constant: %+.1f ms (median); scatter of the constant call's samples: %.1f ms" % (med["uniform"] - med["constant"], max(rec["ms"]["constant"]) - min(rec["ms"]["constant"])))
    out = "\n".join(text) + "\n"
    sys.stdout.write(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
