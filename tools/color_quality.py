#!/usr/bin/env python3
"""Colour PSNR (Y, U, V) of the benchmark GOF's point-cloud frames 0..3 on the GPU, and the device time of the four colour stages.

The source cloud with colours of frame k is rbt_reconstruct_rgb of the synthetic maps (tests/synth.py make_maps(w, h, 1051 + k), geometry and attributes, occupancy at
full resolution). Scored against it: the decoded R5 input, the R5 -> R3 transcode, the same with occupancy-aware coding (occupancy_rd) and with RBT_PRESET_FAST; and the
transcode against the R5 input. Decoded clouds go through the decoder's geometry smoothing (CTC: grid 8, threshold 64), as in bench.py's quality leg. The R5 input and the
R3 transcode are scored a second time with the attribute transfer the reference decoder runs after its smoothing (rbt_reconstruct_decoded, attr_transfer 1): rows
"..._transfer_vs_source", with the number of moved and of re-coloured points per frame. Stage times: events around the launches (rbt_color_stage_ms, rbt_transfer_stage),
median of 5 calls after a warm-up, per point-cloud frame (up-conversion: its two attribute pictures; RGB: its points; metric: source against the R3 cloud, both directions,
the score's kernels without the index building; transfer: frame 0 of the R3 transcode inside rbt_reconstruct_decoded, kernels only). Prints one JSON line; --out also writes it to a file.

    python tools/color_quality.py --out profiles/color_quality.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4, help="point-cloud frames 0..n-1 (at most 4: the GOF's base atlases)")
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
    variants = {"r3": gs.rate_params(R, 3), "r3_occupancy_rd": gs.rate_params(R, 3, occupancy_rd=1), "r3_preset_fast": gs.rate_params(R, 3, preset=R.RBT_PRESET_FAST)}
    ctx.set_depth(1)
    streams = {"r5_input": (gof, 2)}
    sizes = {"r5_input": [len(s) for s in gof]}
    for name, params in variants.items():
        streams[name] = (ctx.transcode_gof(gof, params), 4)
        sizes[name] = [len(s) for s in streams[name][0]]

    counts = {}

    def frame_args(st, prec):
        occ = ctx.decode(st[0])[0]; geo = ctx.decode(st[1])[0]; att = ctx.decode(st[2])[0]
        return [(R.AtlasParams(w, h, 16, prec, 2, 1, 1, 0, 1, 8, 64), synth.atlas_patches(R, w, h, 1051 + k), occ[k][: (w // prec) * (h // prec)].reshape(h // prec, w // prec),
                 geo[2 * k][: w * h].reshape(h, w), geo[2 * k + 1][: w * h].reshape(h, w), 10, att[2 * k], att[2 * k + 1], 10) for k in range(nfr)]

    def clouds(st, prec, transfer=None):
        out = []
        for a in frame_args(st, prec):
            if transfer is None:
                c = ctx.reconstruct_rgb(*a)
            else:
                c = ctx.reconstruct_decoded(*a, attr_transfer=1)
                counts.setdefault(transfer, {"moved": [], "changed": []})
                counts[transfer]["moved"].append(int(c[5].sum())); counts[transfer]["changed"].append(int(ctx.n_changed))
            out.append((c[0], c[4]))
        return out
    source = []
    for k in range(nfr):
        m = synth.make_maps(w, h, 1051 + k)
        c = ctx.reconstruct_rgb(R.AtlasParams(w, h, 16, 1, 2, 1, 1, 0), synth.atlas_patches(R, w, h, 1051 + k), m["occ_full"].astype(np.uint16), m["geo"][0][: w * h].reshape(h, w),
                                m["geo"][1][: w * h].reshape(h, w), 10, m["attr"][0], m["attr"][1], 10)
        source.append((c[0], c[4], m["attr"], c[1]))
    dec = {name: clouds(st, prec) for name, (st, prec) in streams.items()}
    dec_t = {name + "_transfer": clouds(*streams[name], transfer=name) for name in ("r5_input", "r3")}

    def table(ref, test):
        per = [ctx.color_metric(a[0], a[1], b[0], b[1])["psnr"] for a, b in zip(ref, test)]
        return {"frames_yuv_db": [[round(float(x), 3) for x in p] for p in per], "mean_yuv_db": [round(float(np.mean([p[c] for p in per])), 3) for c in range(3)]}
    psnr = {name + "_vs_source": table(source, dec[name]) for name in streams}
    psnr["r3_vs_r5_input"] = table(dec["r5_input"], dec["r3"])
    for name in dec_t:
        psnr[name + "_vs_source"] = table(source, dec_t[name])

    # stage times, frame 0
    t = {"upconvert": [], "rgb": [], "metric": [], "transfer": []}
    yuv = source[0][3]
    r3_frame0 = frame_args(*streams["r3"])[0]
    for i in range(6):
        ctx.yuv420_to_yuv444(source[0][2], w, h, 10); a = ctx.color_stage_ms()["upconvert"]
        ctx.yuv16_to_rgb8(yuv); b = ctx.color_stage_ms()["rgb"]
        ctx.color_metric(source[0][0], source[0][1], dec["r3"][0][0], dec["r3"][0][1]); c = ctx.color_stage_ms()["metric"]
        ctx.reconstruct_decoded(*r3_frame0, attr_transfer=1); d = ctx.color_stage_ms()["transfer"]
        if i:
            t["upconvert"].append(a); t["rgb"].append(b); t["metric"].append(c); t["transfer"].append(d)
    line = {"tool": "color_quality", "size": [w, h], "frames": nfr, "points_source": [int(s[0].shape[0]) for s in source], "points_r3": [int(c[0].shape[0]) for c in dec["r3"]],
            "bytes_occupancy_geometry_attribute": sizes, "colour_psnr": psnr, "attr_transfer_points": counts,
            "stage_ms_per_frame": {k: round(statistics.median(v), 4) for k, v in t.items()}, "stage_ms_samples": {k: [round(x, 4) for x in v] for k, v in t.items()},
            "stage_note": "device time between events around the launches, median of 5 after a warm-up; upconvert: the frame's two 1280x1280 10-bit attribute pictures; rgb: the source "
                          "cloud's points; metric: source cloud against the R3 cloud, both directions: the device_ms of the call's score - the search, the walks and the sums between one pair of events (the uploads, the building of the two indices and the volume clears are outside); "
                          "transfer: the attribute transfer inside rbt_reconstruct_decoded of frame 0 of the R3 transcode: the two copies that keep the unsmoothed cloud (one pair of events) plus the "
                          "per-point flag pass, index building, forward, backward, lists and sums (a second pair); the clears of the two 128 MB volumes and of the maps, the allocations and the "
                          "read-back of the counters are outside"}
    s = json.dumps(line)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
