#!/usr/bin/env python3
"""Measures D2 per patch (rbt_score_patches_d2) and the D2 floors on the stream and patch by patch (rbt_transcode_gof_d2, rbt_transcode_gof_d2_patches; include/rbt.h,
DESIGN.md 22) on one GPU. The measurement is a child process of its own with a time limit; the tool itself never opens the GPU.

  cost      device_ms of rbt_score_patches_d2 against rbt_score(.., RBT_SCORE_D2) on the same clouds in the same process, alternating: frame 0 of the committed 1280x1280
            32-frame CTC fixture - A the cloud of the decoded input with estimated normals, B the cloud of rbt_transcode_gof's output at R3 with its labels. The relations
            of include/rbt.h are asserted on the way. (--leg cost alone is what a rocprofv3 --kernel-trace --stats run wraps for the kernels' own time.)
  gof       the same fixture at R3, patches as in tools/patch_d1.py, references NULL (the decoded input with estimated normals). Floor: the minimum over the frames of
            the stream's own D2 at R3. On the stream: q*, encodes, the frames' D2; patch by patch: bytes, passes, the histogram of the final patch QPs; --samples wall
            times a GOF of each and of rbt_transcode_gof, interleaved; the device time of estimating the normals of the 32 reference clouds on their own
  slope     mean D1 and mean D2 over the frames at constant geometry QPs 20, 24, 28, 32 (floor-0 reports): dB per QP step of either figure
All samples are kept. No threshold is set.

    python tools/patch_d2.py --out profiles/patch_d2.txt
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
SLOPE_QPS = (20, 24, 28, 32)


def fixture():
    return [open(os.path.join(GOLD, "hm_r5ctc_1280x1280_f32_%s.annexb" % k), "rb").read() for k in ("occ", "geo", "attr")]


def setup(R):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    P = lambda q: [R.StreamParams(0, 8, 4, 5, -1, 0, 0, 0, 0), R.StreamParams(1, q, 4, 5, -1, 0, 0, 0, 0), R.StreamParams(19, ATTR_QP, 4, 5, -1, 0, 0, 0, 0)]
    atlas = R.ctc_smoothing(R.AtlasParams(W, H, 16, 4, 2, 1, 1, 0)); patches = [synth.atlas_patches(R, W, H, SEED + f % 4) for f in range(32)]
    return fixture(), P, atlas, patches


def frame_cloud(R, ctx, atlas, patches, occ_stream, geo_stream, f):
    """the cloud of frame f of a pair of streams through rbt_pcloud_from_maps (grey attribute pictures: positions and labels do not depend on them)"""
    import numpy as np
    om, ow, oh, *_ = ctx.decode(occ_stream); g, w, h, *_ = ctx.decode(geo_stream)
    a = R.AtlasParams(*[getattr(atlas, n) for n, _ in R.AtlasParams._fields_]); a.occupancy_precision = w // ow
    grey = np.full(w * h * 3 // 2, 512, np.uint16)
    luma = lambda fr, ww, hh: fr[:ww * hh].reshape(hh, ww)
    return ctx.pcloud_from_maps(a, patches[f], luma(om[f], ow, oh), luma(g[2 * f], w, h), luma(g[2 * f + 1], w, h), 10, grey, grey, 10)


def leg_cost(R, ctx, a):
    src, P, atlas, patches = setup(R)
    out = ctx.transcode_gof(src, P(GEO_QP))
    ha = frame_cloud(R, ctx, atlas, patches, src[0], src[1], 0); hb = frame_cloud(R, ctx, atlas, patches, out[0], out[1], 0)
    _, nrm_ms = ha.estimate_normals(None, copy=False)
    n = len(patches[0]); whole, per, d1p = [], [], []
    for k in range(a.samples + 1):                                        # the first round warms up
        s = ctx.score(ha, hb, 1023, R.RBT_SCORE_D2); got, w, ms = ctx.score_patches_d2(ha, hb, n); _, _, ms1 = ctx.score_patches(ha, hb, n)
        assert w == s["d2"] and sum(g["n_ab"] for g in got) == w["n_a"] and sum(g["n_ba"] for g in got) == w["n_b"] and max(g["max_ba"] for g in got) == w["max_ba"] and max(g["max_ab"] for g in got) == w["max_ab"]
        assert abs(sum(g["sse_ba"] for g in got) - w["sse_ba"]) <= 1e-9 * w["sse_ba"] and abs(sum(g["sse_ab"] for g in got) - w["sse_ab"]) <= 1e-9 * w["sse_ab"]
        if k: whole.append(s["device_ms"]); per.append(ms); d1p.append(ms1)
    rec = {"points_a": ha.points()[0], "points_b": hb.points()[0], "patches": n, "score_d2_ms": whole, "score_patches_d2_ms": per, "score_patches_d1_ms": d1p, "normals_ms": nrm_ms,
           "d2_psnr": w["psnr"], "worst_patch": min(g["psnr"] for g in got)}
    ha.release(); hb.release()
    return rec


def leg_gof(R, ctx, a):
    src, P, atlas, patches = setup(R); PS = P(GEO_QP)
    st = lambda floor: [R.D2Target(), R.D2Target(atlas, patches, floor), R.D2Target()]
    pt = lambda floor: [R.PatchD2Target(), R.PatchD2Target(atlas, patches, floor), R.PatchD2Target()]
    const = ctx.transcode_gof(src, PS)
    rep0 = ctx.transcode_gof_d2(src, PS, st(0))[1][1]
    floor = int(rep0["min_d2"] * 1000)
    rep_p = ctx.transcode_gof_d2_patches(src, PS, pt(0))[1][1]
    so, sr = ctx.transcode_gof_d2(src, PS, st(floor))
    po, pr = ctx.transcode_gof_d2_patches(src, PS, pt(floor))
    nrm = []
    for f in range(32):                                                   # the estimation a job runs once per reference cloud, on its own
        h = frame_cloud(R, ctx, atlas, patches, src[0], src[1], f); nrm.append(h.estimate_normals(None, copy=False)[1]); h.release()
    calls = {"constant": lambda: ctx.transcode_gof(src, PS), "d2": lambda: ctx.transcode_gof_d2(src, PS, st(floor)), "d2_patches": lambda: ctx.transcode_gof_d2_patches(src, PS, pt(floor))}
    ms = {k: [] for k in calls}
    for _ in range(a.samples):
        for k, f in calls.items():
            t0 = time.perf_counter(); f(); ms[k].append((time.perf_counter() - t0) * 1e3)
    s, r = sr[1], pr[1]
    qs = [p["qp"] for fr in r["frames"] for p in fr["patches"]]
    return {"floor_mdb": floor, "constant_bytes": len(const[1]), "r3_frames": [round(float(f["psnr"]), 3) for f in rep0["frames"]], "report_cloud_ms": rep0["cloud_ms"],
            "r3_worst_patch": [round(min(p["figure"] for p in f["patches"]), 3) for f in rep_p["frames"]], "normals_ms": nrm,
            "stream": {"qp": s["qp"], "qp_start": s["qp_start"], "met": s["met"], "n_encodes": s["n_encodes"], "bytes": s["bytes"], "min_d2": s["min_d2"], "mean_d2": s["mean_d2"], "cloud_ms": s["cloud_ms"],
                       "stream_is_transcode_gof": so == ctx.transcode_gof(src, P(s["qp"]))},
            "patches": {"bytes": r["bytes"], "met_all": r["met_all"], "n_passes": r["n_passes"], "pictures_encoded": r["pictures_encoded"], "cloud_ms": r["cloud_ms"],
                        "frame_d2": [round(float(f["d2"]["psnr"]), 3) for f in r["frames"]], "trials": [f["n_trials"] for f in r["frames"]],
                        "worst_patch": [round(min(p["figure"] for p in f["patches"]), 3) for f in r["frames"]], "unmet": sum(1 - p["met"] for f in r["frames"] for p in f["patches"]),
                        "qp_hist": sorted(collections.Counter(qs).items()), "n_patches": len(qs), "stream_is_the_maps": po[1] == ctx.transcode_gof_qp_map(src, PS, [None, r["map"], None])[1]},
            "ms": ms}


def leg_slope(R, ctx, a):
    src, P, atlas, patches = setup(R)
    out = {}
    for q in SLOPE_QPS:
        d1 = ctx.transcode_gof_d1(src, P(q), [R.D1Target(), R.D1Target(atlas, patches), R.D1Target()])[1][1]
        d2 = ctx.transcode_gof_d2(src, P(q), [R.D2Target(), R.D2Target(atlas, patches), R.D2Target()])[1][1]
        out[str(q)] = {"mean_d1": d1["mean_d1"], "min_d1": d1["min_d1"], "mean_d2": d2["mean_d2"], "min_d2": d2["min_d2"], "bytes": d2["bytes"]}
    return out


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rbt_lib
    R = rbt_lib.module(); ctx = R.Context(device=0)
    rec = {}
    if a.leg in ("all", "cost"): rec["cost"] = leg_cost(R, ctx, a)
    if a.leg in ("all", "gof"): rec["gof"] = leg_gof(R, ctx, a)
    if a.leg in ("all", "slope"): rec["slope"] = leg_slope(R, ctx, a)
    ctx.close()
    print("RESULT " + json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--leg", default="all", choices=("all", "cost", "gof", "slope"))
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
    fl = lambda v: " ".join("%.3f" % x for x in v)
    text = ["patch_d2: D2 per patch and D2 floors on the stream and patch by patch, %d samples a figure" % a.samples]
    if "cost" in rec:
        c = rec["cost"]; m0, m1, m2 = (statistics.median(c[k]) for k in ("score_d2_ms", "score_patches_d2_ms", "score_patches_d1_ms"))
        text.append("cost of the per-patch D2 sums: frame 0 of the 1280x1280 CTC fixture at R3, %d points (decoded input) against %d (output), %d patches; D2 %.3f dB, worst patch %.3f dB" % (
            c["points_a"], c["points_b"], c["patches"], c["d2_psnr"], c["worst_patch"]))
        text.append("  rbt_score D2         device_ms median %.3f  samples %s" % (m0, fl(c["score_d2_ms"])))
        text.append("  rbt_score_patches_d2 device_ms median %.3f  samples %s" % (m1, fl(c["score_patches_d2_ms"])))
        text.append("  difference of the medians (k_p2_block, k_p2_cols, k_p2_fold twice, between the same events): %.3f ms, %.2fx" % (m1 - m0, m1 / m0))
        text.append("  rbt_score_patches (D1) device_ms median %.3f  samples %s;  normals of the source cloud %.3f ms" % (m2, fl(c["score_patches_d1_ms"]), c["normals_ms"]))
    if "gof" in rec:
        g = rec["gof"]; med = {k: statistics.median(v) for k, v in g["ms"].items()}; s, p = g["stream"], g["patches"]
        text.append("1280x1280 32-frame CTC fixture, geometry at R3 (QP %d): floor %.3f dB (the minimum over the frames of the D2 at R3); constant QP %d B" % (GEO_QP, g["floor_mdb"] / 1000.0, g["constant_bytes"]))
        text.append("  D2 per frame at R3            " + " ".join("%.2f" % x for x in g["r3_frames"]))
        text.append("  worst patch per frame at R3   " + " ".join("%.2f" % x for x in g["r3_worst_patch"]))
        text.append("  normal estimation of the 32 reference clouds on their own: %.1f ms device time in all (%.2f ms a cloud); clouds of the floor-0 report %.1f ms" % (
            sum(g["normals_ms"]), sum(g["normals_ms"]) / len(g["normals_ms"]), g["report_cloud_ms"]))
        text.append("  on the stream  : q* %d (qs %d), met %d, %d encodes, %d B (%.4f of constant QP), min D2 %.3f, mean D2 %.3f, clouds %.1f ms (normals: %.3f of it), stream equals rbt_transcode_gof's at q*: %s" % (
            s["qp"], s["qp_start"], s["met"], s["n_encodes"], s["bytes"], s["bytes"] / g["constant_bytes"], s["min_d2"], s["mean_d2"], s["cloud_ms"], sum(g["normals_ms"]) / s["cloud_ms"], s["stream_is_transcode_gof"]))
        text.append("  patch by patch : %d B (%.4f of constant QP), met_all %d (%d of %d patches unmet), %d passes, %d pictures encoded, clouds %.1f ms, stream equals the final map's: %s" % (
            p["bytes"], p["bytes"] / g["constant_bytes"], p["met_all"], p["unmet"], p["n_patches"], p["n_passes"], p["pictures_encoded"], p["cloud_ms"], p["stream_is_the_maps"]))
        text.append("    trials_f    " + " ".join(str(q) for q in p["trials"]))
        text.append("    D2_f        " + " ".join("%.2f" % q for q in p["frame_d2"]))
        text.append("    worst patch " + " ".join("%.2f" % q for q in p["worst_patch"]))
        text.append("    final patch QPs (qp:count) " + " ".join("%d:%d" % (q, n) for q, n in p["qp_hist"]))
        for k in ("constant", "d2", "d2_patches"):
            text.append("ms a GOF %-12s median %.1f  samples %s" % (k, med[k], " ".join("%.1f" % x for x in g["ms"][k])))
    if "slope" in rec:
        text.append("constant geometry QP, means over the 32 frames (floor-0 reports of rbt_transcode_gof_d1 / rbt_transcode_gof_d2):")
        qs = sorted(rec["slope"], key=int)
        for q in qs:
            v = rec["slope"][q]
            text.append("  QP %s: mean D1 %.3f (min %.3f)  mean D2 %.3f (min %.3f)  %d B" % (q, v["mean_d1"], v["min_d1"], v["mean_d2"], v["min_d2"], v["bytes"]))
        first, last = rec["slope"][qs[0]], rec["slope"][qs[-1]]; steps = int(qs[-1]) - int(qs[0])
        text.append("  dB per QP step from QP %s to %s: D1 %.3f, D2 %.3f" % (qs[0], qs[-1], (first["mean_d1"] - last["mean_d1"]) / steps, (first["mean_d2"] - last["mean_d2"]) / steps))
    out = "\n".join(text) + "\n"
    sys.stdout.write(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(out)


if __name__ == "__main__":
    main()
