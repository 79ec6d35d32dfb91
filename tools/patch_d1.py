#!/usr/bin/env python3
"""Measures D1 per patch (rbt_score_patches) and D1 floors held patch by patch (rbt_transcode_gof_d1_patches; include/rbt.h) on one GPU. The measurement is
a child process of its own with a time limit; the tool itself never opens the GPU.

  cost      device_ms of rbt_score_patches against rbt_score(.., RBT_SCORE_D1) on the same clouds in the same process, alternating: a 1024 x 1024 height field cut into
            patches of 32 x 32 points, the decoded side with +-1 depth noise, points in patch order (1 048 576 points, 1024 patches). The invariants of include/rbt.h are
            asserted on the way. (--leg cost alone is what a rocprofv3 --kernel-trace --stats run wraps for the kernels' own time.)
  gof       the committed 1280x1280 32-frame CTC fixture (tests/golden/hm_r5ctc_1280x1280_f32_*.annexb) at R3, patches as in tools/frame_floor.py. Floor: the minimum over
            the frames of the D1 at R3, the floor profiles/frame_floor.txt used. Constant QP (rbt_transcode_gof), frame by frame (rbt_transcode_gof_d1_frames), patch by
            patch (rbt_transcode_gof_d1_patches), and patch by patch with background_qp 51: bytes, the whole-frame D1 per frame, passes, pictures encoded, the histogram
            of the final patch QPs, --samples wall times a GOF of each, interleaved
All samples are kept. No threshold is set.

    python tools/patch_d1.py --out profiles/patch_d1.txt
"""
import argparse
import collections
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LIMIT_S = 900
W = H = 1280
SEED = 1051
GEO_QP, ATTR_QP = 24, 32          # R3


def fixture():
    return [open(os.path.join(GOLD, "hm_r5ctc_1280x1280_f32_%s.annexb" % k), "rb").read() for k in ("occ", "geo", "attr")]


def clouds(side, tile, seed=3):
    import numpy as np
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:side, 0:side]
    z = (300 + 120 * np.sin(x / 91.0) + 90 * np.cos(y / 67.0)).astype(np.int64)
    lab = ((y // tile) * (side // tile) + x // tile).ravel()
    order = np.argsort(lab, kind="stable")                                # points in patch order, as a reconstruction emits them
    a = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)[order].astype(np.int16)
    b = a.copy(); b[:, 2] += r.integers(-1, 2, len(b)).astype(np.int16)
    return a, b, lab[order].astype(np.uint32), int(lab.max()) + 1


def leg_cost(R, ctx, a):
    xa, xb, lab, n = clouds(1024, 32)
    ha, hb = ctx.pcloud_upload(xa), ctx.pcloud_upload(xb); hb.set_labels(lab)
    whole, per = [], []
    for k in range(a.samples + 1):                                        # the first pair warms up
        s = ctx.score(ha, hb, 1023, R.RBT_SCORE_D1); got, w, ms = ctx.score_patches(ha, hb, n)
        assert w == s["d1"] and sum(g["sse_ab"] for g in got) == w["sse_ab"] and sum(g["sse_ba"] for g in got) == w["sse_ba"] and sum(g["n_ba"] for g in got) == w["n_b"]
        if k: whole.append(s["device_ms"]); per.append(ms)
    ha.release(); hb.release()
    return {"points": len(xa), "patches": n, "score_d1_ms": whole, "score_patches_ms": per}


def leg_gof(R, ctx, a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    src = fixture()
    P = [R.StreamParams(0, 8, 4, 5, -1, 0, 0, 0, 0), R.StreamParams(1, GEO_QP, 4, 5, -1, 0, 0, 0, 0), R.StreamParams(19, ATTR_QP, 4, 5, -1, 0, 0, 0, 0)]
    n_pc = 32
    atlas = R.ctc_smoothing(R.AtlasParams(W, H, 16, 4, 2, 1, 1, 0)); patches = [synth.atlas_patches(R, W, H, SEED + f % 4) for f in range(n_pc)]
    d1t = lambda floor: [R.D1Target(), R.D1Target(atlas, patches, floor), R.D1Target()]
    pdt = lambda floor, bg=-1: [R.PatchD1Target(), R.PatchD1Target(atlas, patches, floor, background_qp=bg), R.PatchD1Target()]
    const = ctx.transcode_gof(src, P)
    rep0 = ctx.transcode_gof_d1(src, P, d1t(0))[1][1]
    floor = int(rep0["min_d1"] * 1000)
    rep_p = ctx.transcode_gof_d1_patches(src, P, pdt(0))[1][1]            # report only: which patch sets a frame's D1 at R3
    fo, fr = ctx.transcode_gof_d1_frames(src, P, d1t(floor))
    po, pr = ctx.transcode_gof_d1_patches(src, P, pdt(floor))
    bo, br = ctx.transcode_gof_d1_patches(src, P, pdt(floor, 51))
    calls = {"constant": lambda: ctx.transcode_gof(src, P), "d1_frames": lambda: ctx.transcode_gof_d1_frames(src, P, d1t(floor)),
             "d1_patches": lambda: ctx.transcode_gof_d1_patches(src, P, pdt(floor)), "d1_patches_bg51": lambda: ctx.transcode_gof_d1_patches(src, P, pdt(floor, 51))}
    ms = {k: [] for k in calls}
    for _ in range(a.samples):
        for k, f in calls.items():
            t0 = time.perf_counter(); f(); ms[k].append((time.perf_counter() - t0) * 1e3)

    def patch_leg(outs, r):
        r = r[1]
        qs = [p["qp"] for fr_ in r["frames"] for p in fr_["patches"]]
        return {"bytes": r["bytes"], "met_all": r["met_all"], "n_passes": r["n_passes"], "pictures_encoded": r["pictures_encoded"], "cloud_ms": r["cloud_ms"],
                "frame_d1": [round(float(f["d1"]["psnr"]), 3) for f in r["frames"]], "trials": [f["n_trials"] for f in r["frames"]],
                "worst_patch": [round(min(p["figure"] for p in f["patches"]), 3) for f in r["frames"]], "unmet": sum(1 - p["met"] for f in r["frames"] for p in f["patches"]),
                "qp_hist": sorted(collections.Counter(qs).items()), "n_patches": len(qs),
                "stream_is_the_maps": outs[1] == ctx.transcode_gof_qp_map(src, P, [None, r["map"], None])[1]}
    return {"floor_mdb": floor, "constant_bytes": len(const[1]), "r3_frames": [round(float(f["psnr"]), 3) for f in rep0["frames"]],
            "r3_worst_patch": [round(min(p["figure"] for p in f["patches"]), 3) for f in rep_p["frames"]],
            "r3_worst_index": [min(range(f["n_patches"]), key=lambda k: f["patches"][k]["figure"]) for f in rep_p["frames"]],
            "frames": {"qp": [f["qp"] for f in fr[1]["frames"]], "met_all": fr[1]["met_all"], "n_passes": fr[1]["n_passes"], "pictures_encoded": fr[1]["pictures_encoded"], "bytes": fr[1]["bytes"],
                       "figure": [round(f["figure"], 3) for f in fr[1]["frames"]], "cloud_ms": fr[1]["cloud_ms"]},
            "patches": patch_leg(po, pr), "patches_bg51": patch_leg(bo, br), "ms": ms}


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rbt_lib
    R = rbt_lib.module(); ctx = R.Context(device=0)
    rec = {}
    if a.leg in ("all", "cost"): rec["cost"] = leg_cost(R, ctx, a)
    if a.leg in ("all", "gof"): rec["gof"] = leg_gof(R, ctx, a)
    ctx.close()
    print("RESULT " + json.dumps(rec))


def hist(h):
    return " ".join("%d:%d" % (q, n) for q, n in h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--leg", default="all", choices=("all", "cost", "gof"))
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--samples", str(a.samples), "--leg", a.leg], capture_output=True, text=True, timeout=LIMIT_S)
    line = next((x for x in r.stdout.splitlines() if x.startswith("RESULT ")), None)
    if r.returncode or line is None:
        sys.stderr.write(r.stdout + r.stderr); sys.exit(1)
    rec = json.loads(line[7:])
    text = ["patch_d1: D1 per patch and D1 floors held patch by patch, %d samples a figure" % a.samples]
    if "cost" in rec:
        c = rec["cost"]; m0, m1 = statistics.median(c["score_d1_ms"]), statistics.median(c["score_patches_ms"])
        text.append("cost of the per-patch sums: %d points a cloud, %d patches, points in patch order" % (c["points"], c["patches"]))
        text.append("  rbt_score D1      device_ms median %.3f  samples %s" % (m0, " ".join("%.3f" % x for x in c["score_d1_ms"])))
        text.append("  rbt_score_patches device_ms median %.3f  samples %s" % (m1, " ".join("%.3f" % x for x in c["score_patches_ms"])))
        text.append("  difference of the medians (k_pd_sums twice, between the same events): %.3f ms, %.2fx" % (m1 - m0, m1 / m0))
    if "gof" in rec:
        g = rec["gof"]; med = {k: statistics.median(v) for k, v in g["ms"].items()}
        text.append("1280x1280 32-frame CTC fixture, geometry at R3 (QP %d): floor %.3f dB (the minimum over the frames of the D1 at R3); constant QP %d B" % (GEO_QP, g["floor_mdb"] / 1000.0, g["constant_bytes"]))
        text.append("  D1 per frame at R3            " + " ".join("%.2f" % x for x in g["r3_frames"]))
        text.append("  worst patch per frame at R3   " + " ".join("%.2f" % x for x in g["r3_worst_patch"]))
        text.append("  its index in the frame's list " + " ".join(str(x) for x in g["r3_worst_index"]))
        f = g["frames"]
        text.append("  frame by frame : %d B (%.4f of constant QP), met_all %d, %d passes, %d pictures encoded, clouds %.1f ms" % (f["bytes"], f["bytes"] / g["constant_bytes"], f["met_all"], f["n_passes"], f["pictures_encoded"], f["cloud_ms"]))
        text.append("    q*_f        " + " ".join(str(q) for q in f["qp"]))
        text.append("    D1_f        " + " ".join("%.2f" % q for q in f["figure"]))
        for key, name in (("patches", "patch by patch"), ("patches_bg51", "patch by patch, background_qp 51")):
            p = g[key]
            text.append("  %s : %d B (%.4f of constant QP, %.4f of frame by frame), met_all %d (%d of %d patches unmet), %d passes, %d pictures encoded, clouds %.1f ms, stream equals the final map's: %s" % (
                name, p["bytes"], p["bytes"] / g["constant_bytes"], p["bytes"] / f["bytes"], p["met_all"], p["unmet"], p["n_patches"], p["n_passes"], p["pictures_encoded"], p["cloud_ms"], p["stream_is_the_maps"]))
            text.append("    trials_f    " + " ".join(str(q) for q in p["trials"]))
            text.append("    D1_f        " + " ".join("%.2f" % q for q in p["frame_d1"]))
            text.append("    worst patch " + " ".join("%.2f" % q for q in p["worst_patch"]))
            text.append("    final patch QPs (qp:count) " + hist(p["qp_hist"]))
        for k in ("constant", "d1_frames", "d1_patches", "d1_patches_bg51"):
            text.append("ms a GOF %-16s median %.1f  samples %s" % (k, med[k], " ".join("%.1f" % x for x in g["ms"][k])))
    out = "\n".join(text) + "\n"
    sys.stdout.write(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(out)


if __name__ == "__main__":
    main()
