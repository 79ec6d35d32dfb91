#!/usr/bin/env python3
"""Measures the colour PSNR per patch (rbt_score_patches_color, rbt_score_pair_patches_color) and the colour floors held patch by patch (rbt_transcode_gof_color_patches;
include/rbt.h) on one GPU. The measurement is a child process of its own with a time limit; the tool itself never opens the GPU.

  kernel    frame 0 of the committed 1280x1280 32-frame CTC fixture - A the cloud of the decoded input, B the cloud of rbt_transcode_gof's output at R3, both through
            rbt_pcloud_from_maps with their attribute pictures - as one score pair; rounds of rbt_score_pair_color (two k_sc_color_walk launches),
            rbt_score_pair_patches_color (two k_pc_sums launches) and rbt_score_patches (k_pd_sums behind its searches), alternating, the relations of include/rbt.h asserted
            on the way. The kernels' own device times come from a kernel trace of this leg: run it as
                rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python tools/patch_color.py --child --leg kernel --samples 7
            and hand DIR/kt_kernel_trace.csv to --trace; the medians per kernel and direction are taken over the rounds behind the first. Beside that, in the same process,
            device_ms (events) of rbt_score_patches_color against rbt_score(.., RBT_SCORE_COLOR): both with the two searches in front.
  trial     the time between the clouds' events (cloud_ms) of a floor-0 report against a walk capped at --cap trials on the same GOF: the difference per further trial and
            cloud, against the colour job's recolour route (profiles/color_target.txt)
  gof       the fixture at R3, all 32 frames, the floor of every patch the stream's own colour Y-PSNR at R3 (43.712 dB): bytes, passes, pictures encoded and, with
            --samples wall times interleaved, ms a GOF of rbt_transcode_gof_color_patches against rbt_transcode_gof_color on the stream with the same floor,
            rbt_transcode_gof_quality_patches on the attribute entry (luma PSNR floor 44.416 dB, profiles/patch_floor.txt) and the constant-QP call
All samples are kept. No threshold is set.

    python tools/patch_color.py --out profiles/patch_color.txt [--trace DIR/kt_kernel_trace.csv]
"""
import argparse
import collections
import csv
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
FLOOR = 43712                     # the stream's own colour Y-PSNR at R3, minimum over the frames (profiles/color_target.txt)
LUMA_FLOOR = 44416                # the attribute stream's own luma PSNR at R3 (profiles/patch_floor.txt)


def fixture():
    return [open(os.path.join(GOLD, "hm_r5ctc_1280x1280_f32_%s.annexb" % k), "rb").read() for k in ("occ", "geo", "attr")]


def setup(R):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    PS = [R.StreamParams(0, 8, 4, 5, -1, 0, 0, 0, 0), R.StreamParams(1, GEO_QP, 4, 5, -1, 0, 0, 0, 0), R.StreamParams(19, ATTR_QP, 4, 5, -1, 0, 0, 0, 0)]
    atlas = R.ctc_smoothing(R.AtlasParams(W, H, 16, 4, 2, 1, 1, 0)); patches = [synth.atlas_patches(R, W, H, SEED + f % 4) for f in range(32)]
    return fixture(), PS, atlas, patches


def frame_cloud(R, ctx, atlas, patches, streams, f):
    """the cloud of frame f of [occupancy, geometry, attribute] streams through rbt_pcloud_from_maps, colours and labels included"""
    om, ow, oh, *_ = ctx.decode(streams[0]); g, w, h, *_ = ctx.decode(streams[1]); t, *_ = ctx.decode(streams[2])
    a = R.AtlasParams(*[getattr(atlas, n) for n, _ in R.AtlasParams._fields_]); a.occupancy_precision = w // ow
    luma = lambda fr, ww, hh: fr[:ww * hh].reshape(hh, ww)
    return ctx.pcloud_from_maps(a, patches[f], luma(om[f], ow, oh), luma(g[2 * f], w, h), luma(g[2 * f + 1], w, h), 10, t[2 * f], t[2 * f + 1], 10, 0, 1)


def leg_kernel(R, ctx, a):
    src, PS, atlas, patches = setup(R)
    out = ctx.transcode_gof(src, PS)
    ha = frame_cloud(R, ctx, atlas, patches, src, 0); hb = frame_cloud(R, ctx, atlas, patches, out, 0)
    n = len(patches[0]); pair = ctx.score_pair(ha, hb)
    whole_ms, per_ms = [], []
    for k in range(a.samples + 1):                                        # the first round warms up
        c = pair.color(); got, w = pair.patches_color(n); d1 = ctx.score_patches(ha, hb, n)[0]
        s = ctx.score(ha, hb, 1023, R.RBT_SCORE_COLOR); g2, w2, ms = ctx.score_patches_color(ha, hb, n)
        assert w == c == s["color"] == w2 and got == g2 and [(g["n_ab"], g["n_ba"]) for g in got] == [(p["n_ab"], p["n_ba"]) for p in d1]
        assert all(sum(g["sse_ab"][ch] for g in got) == c["sse_ab"][ch] and sum(g["sse_ba"][ch] for g in got) == c["sse_ba"][ch] for ch in range(3))
        if k: whole_ms.append(s["device_ms"]); per_ms.append(ms)
    rec = {"points_a": ha.points()[0], "points_b": hb.points()[0], "merged_a": c["n_a"], "merged_b": c["n_b"], "patches": n, "rounds": a.samples + 1, "score_color_ms": whole_ms,
           "score_patches_color_ms": per_ms, "psnr": c["psnr"], "worst_patch_y": min(g["psnr"][0] for g in got), "best_patch_y": max(g["psnr"][0] for g in got)}
    pair.release(); ha.release(); hb.release()
    return rec


def targets(R, atlas, patches, **kw):
    return [R.PatchColorTarget(), R.PatchColorTarget(), R.PatchColorTarget(atlas, patches, **kw)]


def leg_trial(R, ctx, a):
    src, PS, atlas, patches = setup(R)
    ctx.transcode_gof_color_patches(src, PS, targets(R, atlas, patches, min_psnr_mdb=FLOOR, max_trials=a.cap))      # warm-up: arenas and volumes cached
    rep, walk, extra = [], [], 0
    for _ in range(a.samples):
        rep.append(ctx.transcode_gof_color_patches(src, PS, targets(R, atlas, patches))[1][2]["cloud_ms"])
        r = ctx.transcode_gof_color_patches(src, PS, targets(R, atlas, patches, min_psnr_mdb=FLOOR, max_trials=a.cap))[1][2]
        walk.append(r["cloud_ms"]); extra = sum(f["n_trials"] - 1 for f in r["frames"])
    return {"report_cloud_ms": rep, "walk_cloud_ms": walk, "further_cloud_trials": extra, "cap": a.cap}


def leg_gof(R, ctx, a):
    src, PS, atlas, patches = setup(R)
    plain_atlas = R.AtlasParams(W, H, 16, 4, 2, 1, 1, 0)                    # the atlas of tools/patch_floor.py: the PSNR floor reads sizes and rectangles only
    ct = [R.ColorTarget(), R.ColorTarget(), R.ColorTarget(atlas, patches, FLOOR, 0, 0)]
    qt = [R.PatchFloorTarget(), R.PatchFloorTarget(), R.PatchFloorTarget(plain_atlas, patches, min_psnr_mdb=LUMA_FLOOR)]
    pt = lambda: targets(R, atlas, patches, min_psnr_mdb=FLOOR)
    const = ctx.transcode_gof(src, PS)
    rep = ctx.transcode_gof_color_patches(src, PS, targets(R, atlas, patches))[1][2]
    co, cr = ctx.transcode_gof_color(src, PS, ct)
    qo, qr = ctx.transcode_gof_quality_patches(src, PS, qt)
    po, pr = ctx.transcode_gof_color_patches(src, PS, pt())
    calls = {"constant": lambda: ctx.transcode_gof(src, PS), "color": lambda: ctx.transcode_gof_color(src, PS, ct), "quality_patches": lambda: ctx.transcode_gof_quality_patches(src, PS, qt),
             "color_patches": lambda: ctx.transcode_gof_color_patches(src, PS, pt())}
    ms = {k: [] for k in calls}
    for _ in range(a.samples):
        for k, f in calls.items():
            t0 = time.perf_counter(); f(); ms[k].append((time.perf_counter() - t0) * 1e3)
    r = pr[2]; qs = [p["qp"] for fr in r["frames"] for p in fr["patches"]]
    # the colour of the cloud under the luma-PSNR map, patch by patch: the same job as a report run cannot take a map, so the map's stream is rescored through the public calls on frame 0
    return {"floor_mdb": FLOOR, "constant_bytes": [len(x) for x in const], "r3_frame_y": [round(float(f["color"]["psnr"][0]), 3) for f in rep["frames"]],
            "r3_worst_patch_y": [round(min(p["figure"] for p in f["patches"]), 3) for f in rep["frames"]], "report_cloud_ms": rep["cloud_ms"],
            "color": {"qp": cr[2]["qp"], "met": cr[2]["met"], "n_encodes": cr[2]["n_encodes"], "bytes": cr[2]["bytes"], "min_y": cr[2]["min_psnr"][0], "mean_y": cr[2]["mean_psnr"][0], "cloud_ms": cr[2]["cloud_ms"]},
            "quality_patches": {"bytes": qr[2]["bytes"], "met_all": qr[2]["met_all"], "n_passes": qr[2]["n_passes"], "pictures_encoded": qr[2]["pictures_encoded"]},
            "color_patches": {"bytes": r["bytes"], "met_all": r["met_all"], "n_passes": r["n_passes"], "pictures_encoded": r["pictures_encoded"], "cloud_ms": r["cloud_ms"],
                              "frame_y": [round(float(f["color"]["psnr"][0]), 3) for f in r["frames"]], "trials": [f["n_trials"] for f in r["frames"]],
                              "worst_patch_y": [round(min(p["figure"] for p in f["patches"]), 3) for f in r["frames"]], "unmet": sum(1 - p["met"] for f in r["frames"] for p in f["patches"]),
                              "qp_hist": sorted(collections.Counter(qs).items()), "n_patches": len(qs), "geometry_is_constant": po[:2] == const[:2],
                              "stream_is_the_maps": po[2] == ctx.transcode_gof_qp_map(src, PS, [None, None, r["map"]])[2]},
            "ms": ms}


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rbt_lib
    R = rbt_lib.module(); ctx = R.Context(device=0)
    rec = {}
    if a.leg in ("all", "kernel"): rec["kernel"] = leg_kernel(R, ctx, a)
    if a.leg in ("all", "trial"): rec["trial"] = leg_trial(R, ctx, a)
    if a.leg in ("all", "gof"): rec["gof"] = leg_gof(R, ctx, a)
    ctx.close()
    print("RESULT " + json.dumps(rec))


def trace_lines(path):
    """per kernel of the scoring and launch parity (even: A -> B, odd: B -> A) the durations in dispatch order, the warm-up round dropped -> text lines"""
    per = collections.defaultdict(list)
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        for k in ("k_pc_sums", "k_sc_color_walk", "k_pd_sums", "k_sc_search", "k_sc_walk"):
            if "rbtk::" + k + "(" in r["Kernel_Name"]: per[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out, med = ["kernels' own time from the kernel trace (us; per direction the median over the rounds behind the first, all samples kept):"], {}
    for k in ("k_sc_color_walk", "k_pc_sums", "k_pd_sums"):
        for d, name in ((0, "A -> B"), (1, "B -> A")):
            v = per[k][d::2][1:]
            if not v: continue
            med[k, d] = statistics.median(v)
            out.append("  %-16s %s  median %8.1f  samples %s" % (k, name, med[k, d], " ".join("%.1f" % x for x in v)))
    if all((k, d) in med for k in ("k_sc_color_walk", "k_pc_sums", "k_pd_sums") for d in (0, 1)):
        cw, pc, pd = (med[k, 0] + med[k, 1] for k in ("k_sc_color_walk", "k_pc_sums", "k_pd_sums"))
        out.append("  both directions: k_sc_color_walk %.1f, k_pc_sums %.1f (%.3fx), k_pd_sums %.1f; the colour walks plus k_pd_sums %.1f: the single walk costs %.3f of the two walks it replaces" % (
            cw, pc, pc / cw, pd, cw + pd, pc / (cw + pd)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--cap", type=int, default=3)
    ap.add_argument("--leg", default="all", choices=("all", "kernel", "trial", "gof"))
    ap.add_argument("--trace", default="", help="kt_kernel_trace.csv of a rocprofv3 --kernel-trace run of --child --leg kernel")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--samples", str(a.samples), "--cap", str(a.cap), "--leg", a.leg], capture_output=True, text=True, timeout=LIMIT_S)
    line = next((x for x in r.stdout.splitlines() if x.startswith("RESULT ")), None)
    if r.returncode or line is None:
        sys.stderr.write(r.stdout + r.stderr); sys.exit(1)
    rec = json.loads(line[7:])
    fl = lambda v: " ".join("%.3f" % x for x in v)
    text = ["patch_color: colour PSNR per patch and colour floors held patch by patch (tools/patch_color.py, one MI355X), %d samples a figure" % a.samples]
    if "kernel" in rec:
        c = rec["kernel"]; m0, m1 = statistics.median(c["score_color_ms"]), statistics.median(c["score_patches_color_ms"])
        text.append("frame 0 of the 1280x1280 CTC fixture at R3: %d points (decoded input, %d merged) against %d (output, %d merged), %d patches; colour PSNR Y %.3f U %.3f V %.3f dB, patches' Y from %.3f to %.3f dB" % (
            c["points_a"], c["merged_a"], c["points_b"], c["merged_b"], c["patches"], c["psnr"][0], c["psnr"][1], c["psnr"][2], c["worst_patch_y"], c["best_patch_y"]))
        text.append("  with the two searches in front, device_ms between events: rbt_score colour median %.3f  samples %s" % (m0, fl(c["score_color_ms"])))
        text.append("                                                            rbt_score_patches_color median %.3f  samples %s  (%.3fx)" % (m1, fl(c["score_patches_color_ms"]), m1 / m0))
    if a.trace:
        text += trace_lines(a.trace)
    if "trial" in rec:
        t = rec["trial"]; per = [(w - r0) / t["further_cloud_trials"] for w, r0 in zip(t["walk_cloud_ms"], t["report_cloud_ms"])] if t["further_cloud_trials"] else []
        text.append("time between the clouds' events on the benchmark GOF: floor-0 report (geometry half, 32 references, one trial of 32 clouds) ms %s; floor %.3f dB capped at %d trials (%d further clouds) ms %s" % (
            fl(t["report_cloud_ms"]), FLOOR / 1000.0, t["cap"], t["further_cloud_trials"], fl(t["walk_cloud_ms"])))
        if per: text.append("  per further trial and cloud ms %s (median %.2f); the colour job's recolour route: 5.83 (profiles/color_target.txt)" % (fl(per), statistics.median(per)))
    if "gof" in rec:
        g = rec["gof"]; med = {k: statistics.median(v) for k, v in g["ms"].items()}; p, q, c = g["color_patches"], g["quality_patches"], g["color"]; cb = g["constant_bytes"][2]
        text.append("1280x1280 32-frame CTC fixture at R3 (geometry QP %d, attribute QP %d): floor %.3f dB on the colour Y-PSNR of every patch; constant QP: attribute %d B, geometry %d B" % (GEO_QP, ATTR_QP, g["floor_mdb"] / 1000.0, cb, g["constant_bytes"][1]))
        text.append("  colour Y per frame at R3           " + " ".join("%.2f" % x for x in g["r3_frame_y"]))
        text.append("  worst patch per frame at R3 (Y)    " + " ".join("%.2f" % x for x in g["r3_worst_patch_y"]))
        text.append("  rbt_transcode_gof_color on the stream      : q* %d, met %d, %d encodes, %d B (%.4f of constant QP), min Y %.3f, mean Y %.3f, clouds %.1f ms" % (
            c["qp"], c["met"], c["n_encodes"], c["bytes"], c["bytes"] / cb, c["min_y"], c["mean_y"], c["cloud_ms"]))
        text.append("  rbt_transcode_gof_quality_patches (luma PSNR floor %.3f dB): %d B (%.4f of constant QP), met_all %d, %d passes, %d pictures encoded" % (
            LUMA_FLOOR / 1000.0, q["bytes"], q["bytes"] / cb, q["met_all"], q["n_passes"], q["pictures_encoded"]))
        text.append("  rbt_transcode_gof_color_patches            : %d B (%.4f of constant QP), met_all %d (%d of %d patches unmet), %d passes, %d pictures encoded, clouds %.1f ms (floor-0 report %.1f), "
                    "geometry stream equals the constant-QP call's: %s, attribute stream equals the final map's: %s" % (
                        p["bytes"], p["bytes"] / cb, p["met_all"], p["unmet"], p["n_patches"], p["n_passes"], p["pictures_encoded"], p["cloud_ms"], g["report_cloud_ms"], p["geometry_is_constant"], p["stream_is_the_maps"]))
        text.append("    trials_f    " + " ".join(str(x) for x in p["trials"]))
        text.append("    Y_f         " + " ".join("%.2f" % x for x in p["frame_y"]))
        text.append("    worst patch " + " ".join("%.2f" % x for x in p["worst_patch_y"]))
        text.append("    final patch QPs (qp:count) " + " ".join("%d:%d" % (x, n) for x, n in p["qp_hist"]))
        for k in ("constant", "color", "quality_patches", "color_patches"):
            text.append("ms a GOF %-16s median %.1f  samples %s" % (k, med[k], " ".join("%.1f" % x for x in g["ms"][k])))
    out = "\n".join(text) + "\n"
    sys.stdout.write(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(out)


if __name__ == "__main__":
    main()
