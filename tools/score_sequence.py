#!/usr/bin/env python3
"""Scores the benchmark GOF's point-cloud frames on the GPU with rbt_pcloud_from_maps + rbt_score (D1, D2, colour PSNR per frame, and the sequence summary of
rbt_score_summary), and times that route against the host-array calls, which are three separate upload-and-score calls on the same index and search.

Frames: 0..3, the GOF's four base atlases (tests/synth.py make_maps(w, h, 1051 + k)). The later frames of the fixture are these atlases rolled by a few pixels, so their
patches do not lie on the 16-pixel block grid and tests/synth.py has no patch list for them - tools/color_quality.py stops at frame 3 for the same reason. Pairs: the
decoded R5 input and the R5 -> R3 transcode, each against the source cloud (rbt_reconstruct_rgb of the synthetic maps, normals = the projection axis of each point's
patch). Decoded clouds go through the decoder's geometry smoothing and attribute transfer (CTC: grid 8, threshold 64, attr_transfer 1).

Timing, per frame of the R3 pair, both routes in this one process, alternating, a warm-up of each and then 5 samples, host clock around calls that end in a synchronise:
  (a) host arrays: reconstruct_decoded to the host, then d1 + d2 + color_metric: three separate upload-and-score calls, each uploading and indexing both clouds,
      scoring its one part and releasing them (profiles/score_sequence.json was recorded when these calls still had kernels of their own)
  (b) device clouds: pcloud_from_maps + score against the source handle uploaded beforehand + release of the decoded handle
Also recorded: rbt_frame_score.device_ms of (b) and the colour stage's rbt_color_stage_ms figure of (a) for the same pair. All samples are kept. "faster" holds for a
frame when median(a) - median(b) exceeds the spread (max - min) of (a)'s samples. Prints the per-frame lines and the summaries, then one JSON line; --out also writes it.

--estimate-normals scores D2 a second time with source normals estimated by rbt_pcloud_estimate_normals (k = 16, oriented towards the origin) beside the projection-axis
normals: per frame "d2_estimated_db" and the estimation's device time, and the sequence summary under "<pair>_estimated_normals". Without the option nothing changes.

    python tools/score_sequence.py --out profiles/score_sequence.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4, help="point-cloud frames 0..n-1 (at most 4: the GOF's base atlases)")
    ap.add_argument("--time-frames", type=int, default=4, help="how many of them the two routes are timed on")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--estimate-normals", action="store_true", help="also score D2 with source normals estimated on the GPU")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import rbt_lib
    import synth
    R = rbt_lib.module(); gs = rbt_lib.module_file("gof_shard")
    ctx = R.Context(device=0)
    w = h = 1280
    nfr = max(1, min(4, args.frames))
    man = json.load(open(os.path.join(ROOT, "tests", "golden", "hm_r5_manifest.json")))["1280x1280_f32"]
    gof = [gs.first_pictures(open(os.path.join(ROOT, "tests", "golden", man["streams"][k]["file"]), "rb").read(), nfr * (1 if k == "occ" else 2)) for k in ("occ", "geo", "attr")]
    ctx.set_depth(1)
    streams = {"r5_input": (gof, 2), "r3": (ctx.transcode_gof(gof, gs.rate_params(R, 3)), 4)}

    def frame_args(st, prec):
        occ = ctx.decode(st[0])[0]; geo = ctx.decode(st[1])[0]; att = ctx.decode(st[2])[0]
        return [(R.AtlasParams(w, h, 16, prec, 2, 1, 1, 0, 1, 8, 64), synth.atlas_patches(R, w, h, 1051 + k), occ[k][: (w // prec) * (h // prec)].reshape(h // prec, w // prec),
                 geo[2 * k][: w * h].reshape(h, w), geo[2 * k + 1][: w * h].reshape(h, w), 10, att[2 * k], att[2 * k + 1], 10) for k in range(nfr)]
    decoded = {name: frame_args(st, prec) for name, (st, prec) in streams.items()}

    source, handles = [], []
    for k in range(nfr):
        m = synth.make_maps(w, h, 1051 + k)
        c = ctx.reconstruct_rgb(R.AtlasParams(w, h, 16, 1, 2, 1, 1, 0), synth.atlas_patches(R, w, h, 1051 + k), m["occ_full"].astype(np.uint16), m["geo"][0][: w * h].reshape(h, w),
                                m["geo"][1][: w * h].reshape(h, w), 10, m["attr"][0], m["attr"][1], 10)
        xyz, nrm = synth.source_normals(R, ctx.reconstruct, w, h, 1051 + k, m["occ_full"], m["geo"])
        assert np.array_equal(xyz, c[0])
        source.append((c[0], c[4], nrm)); handles.append(ctx.pcloud_upload(c[0], c[4], nrm))
    estimated, estimate_ms = [], []
    if args.estimate_normals:
        for sx, srgb, _ in source:
            hn = ctx.pcloud_upload(sx, srgb); estimate_ms.append(hn.estimate_normals(copy=False)[1]); estimated.append(hn)

    scores, summaries = {}, {}
    for name in streams:
        raw, raw_est = [], []
        for k in range(nfr):
            hb = ctx.pcloud_from_maps(*decoded[name][k], attr_transfer=1)
            raw.append(ctx.score(handles[k], hb, raw=True))
            if estimated: raw_est.append(ctx.score(estimated[k], hb, raw=True))
            hb.release()
        per = [R.frame_score_dict(s) for s in raw]
        scores[name + "_vs_source"] = [{"frame": k, "points": [s["n_points_a"], s["n_points_b"]], "merged": [s["n_merged_a"], s["n_merged_b"]], "d1_db": round(s["d1"]["psnr"], 4),
                                        "d2_db": round(s["d2"]["psnr"], 4), "yuv_db": [round(x, 4) for x in s["color"]["psnr"]], "device_ms": round(s["device_ms"], 4)} for k, s in enumerate(per)]
        summaries[name + "_vs_source"] = R.score_summary(raw)
        for k, e in enumerate(raw_est):
            scores[name + "_vs_source"][k].update({"d2_estimated_db": round(e.d2.psnr, 4), "estimate_normals_device_ms": round(estimate_ms[k], 4)})
        if raw_est: summaries[name + "_vs_source_estimated_normals"] = R.score_summary(raw_est)
        for line in scores[name + "_vs_source"]: print(name, line)
        print(name, "summary", summaries[name + "_vs_source"])

    timing = []
    for k in range(min(nfr, max(0, args.time_frames))):
        a_args = decoded["r3"][k]; sx, srgb, sn = source[k]
        t = {"host_arrays_ms": [], "device_clouds_ms": [], "score_device_ms": [], "color_metric_stage_ms": []}
        for i in range(args.samples + 1):
            t0 = time.perf_counter()
            c = ctx.reconstruct_decoded(*a_args, attr_transfer=1)
            old = (ctx.d1(sx, c[0]), ctx.d2(sx, sn, c[0]), ctx.color_metric(sx, srgb, c[0], c[4]))
            t1 = time.perf_counter()
            stage = ctx.color_stage_ms()["metric"]
            t2 = time.perf_counter()
            hb = ctx.pcloud_from_maps(*a_args, attr_transfer=1); new = ctx.score(handles[k], hb); hb.release()
            t3 = time.perf_counter()
            assert new["d1"] == old[0] and new["color"] == old[2] and new["d2"] == old[1]
            if i:
                t["host_arrays_ms"].append(1e3 * (t1 - t0)); t["device_clouds_ms"].append(1e3 * (t3 - t2)); t["score_device_ms"].append(new["device_ms"]); t["color_metric_stage_ms"].append(stage)
        med = {n: statistics.median(v) for n, v in t.items()}
        spread = max(t["host_arrays_ms"]) - min(t["host_arrays_ms"])
        timing.append({"frame": k, "median_ms": {n: round(v, 4) for n, v in med.items()}, "samples_ms": {n: [round(x, 4) for x in v] for n, v in t.items()},
                       "host_arrays_spread_ms": round(spread, 4), "ratio_host_arrays_over_device_clouds": round(med["host_arrays_ms"] / med["device_clouds_ms"], 3),
                       "faster_by_more_than_the_spread": bool(med["host_arrays_ms"] - med["device_clouds_ms"] > spread)})
        print("timing", timing[-1]["frame"], timing[-1]["median_ms"], "spread", timing[-1]["host_arrays_spread_ms"], "ratio", timing[-1]["ratio_host_arrays_over_device_clouds"])
    for hd in handles + estimated: hd.release()
    line = {"tool": "score_sequence", "size": [w, h], "frames": nfr, "scores": scores, "summary": summaries, "timing_r3_vs_source": timing,
            "timing_note": "host clock around calls that end in a synchronise, both routes alternating in one process, one warm-up of each, then the samples; host_arrays: "
                           "reconstruct_decoded to the host, then d1 + d2 + color_metric; device_clouds: pcloud_from_maps + score against the source handle uploaded beforehand + "
                           "release of the decoded handle; score_device_ms: events around the score's kernels; color_metric_stage_ms: rbt_color_stage_ms of the host-array route"}
    s = json.dumps(line)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
