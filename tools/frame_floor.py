#!/usr/bin/env python3
"""Measures PSNR floors held frame by frame (rbt_transcode_gof_quality_frames, include/rbt.h "floors held frame by frame") and the QP list per point-cloud frame
(rbt_transcode_gof_frame_qp) on the committed 1280x1280 32-frame CTC fixture (tests/golden/hm_r5ctc_1280x1280_f32_*.annexb), on one GPU. The measurement is a child process
of its own with a time limit; the tool itself never opens the GPU.

  floors    the luma PSNRs the constant-QP R3 transcode reaches for the geometry and the attribute stream (rbt_transcode_gof_quality without floors), truncated to 1/1000 dB
  stream    those floors on the stream's sums through the existing call (rbt_transcode_gof_quality): q*, the bytes, the encodes
  frames    the same floors held by every frame (rbt_transcode_gof_quality_frames): q*_f per frame, the bytes against the call above, the passes, the pictures encoded
  time      --samples wall times of both calls, of rbt_transcode_gof at R3 and of rbt_transcode_gof_frame_qp with the identity list, interleaved in one process. The last two
            issue the same launches: any difference beyond the scatter of the samples is reported as it is
  d1        geometry with the minimum over the frames of the D1 the R3 transcode reaches as the floor: through the existing call with RBT_D1_MIN (rbt_transcode_gof_d1: the
            worst frame dictates the QP of all) and frame by frame (rbt_transcode_gof_d1_frames): bytes, q*_f, passes, pictures encoded, milliseconds. Patches as in
            tools/d1_target.py: synth.atlas_patches of the four base atlases, the rectangles of frames 4..31 not rolled with their pictures - clouds of the benchmark's size
All samples are kept. No threshold is set.

    python tools/frame_floor.py --out profiles/frame_floor.txt
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


def fixture():
    return [open(os.path.join(GOLD, "hm_r5ctc_1280x1280_f32_%s.annexb" % k), "rb").read() for k in ("occ", "geo", "attr")]


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rbt_lib
    R = rbt_lib.module(); ctx = R.Context(device=0)
    src = fixture()
    P = [R.StreamParams(0, 8, 4, 5, -1, 0, 0, 0, 0), R.StreamParams(1, GEO_QP, 4, 5, -1, 0, 0, 0, 0), R.StreamParams(19, ATTR_QP, 4, 5, -1, 0, 0, 0, 0)]
    none = [R.QualityTarget()] * 3
    outs, res = ctx.transcode_gof_quality(src, P, none)
    floors = [0, int(res[1]["psnr"][0] * 1000), int(res[2]["psnr"][0] * 1000)]
    tg = [R.QualityTarget(f) if f else R.QualityTarget() for f in floors]
    n_pc = len(ctx.transcode_gof_quality_frames(src, P, none)[1][1]["frames"])
    ident = [None, [GEO_QP] * n_pc, [ATTR_QP] * n_pc]
    so, sr = ctx.transcode_gof_quality(src, P, tg)
    fo, fr = ctx.transcode_gof_quality_frames(src, P, tg)
    const = ctx.transcode_gof(src, P)
    calls = {"stream": lambda: ctx.transcode_gof_quality(src, P, tg), "frames": lambda: ctx.transcode_gof_quality_frames(src, P, tg),
             "constant": lambda: ctx.transcode_gof(src, P), "identity_list": lambda: ctx.transcode_gof_frame_qp(src, P, ident)}
    ms = {k: [] for k in calls}
    for _ in range(a.samples):
        for k, f in calls.items():
            t0 = time.perf_counter(); f(); ms[k].append((time.perf_counter() - t0) * 1e3)
    rec = {"floors_mdb": floors[1:], "constant_bytes": [len(const[1]), len(const[2])], "identity_equals_constant": ctx.transcode_gof_frame_qp(src, P, ident) == const,
           "frames_equals_list": fo == ctx.transcode_gof_frame_qp(src, P, [None] + [[f["qp"] for f in fr[k]["frames"]] for k in (1, 2)]), "ms": ms}
    for k, name in ((1, "geometry"), (2, "attribute")):
        rec[name] = {"stream": {x: sr[k][x] for x in ("qp", "qp_start", "met", "n_encodes", "bytes")}, "stream_psnr": sr[k]["psnr"][0],
                     "frames": {"qp": [f["qp"] for f in fr[k]["frames"]], "met_all": fr[k]["met_all"], "n_passes": fr[k]["n_passes"], "pictures_encoded": fr[k]["pictures_encoded"],
                                "bytes": fr[k]["bytes"], "n_encodes": [f["n_encodes"] for f in fr[k]["frames"]], "figure": [round(f["figure"], 3) for f in fr[k]["frames"]],
                                "psnr": fr[k]["sums"]["psnr"][0]}}
    # the D1 leg
    import synth
    atlas = R.ctc_smoothing(R.AtlasParams(W, H, 16, 4, 2, 1, 1, 0)); patches = [synth.atlas_patches(R, W, H, SEED + f % 4) for f in range(n_pc)]
    d1t = lambda floor: [R.D1Target(), R.D1Target(atlas, patches, floor), R.D1Target()]
    rep0 = ctx.transcode_gof_d1(src, P, d1t(0))[1][1]
    dfloor = int(rep0["min_d1"] * 1000)
    mo, mr = ctx.transcode_gof_d1(src, P, d1t(dfloor))
    po, pr = ctx.transcode_gof_d1_frames(src, P, d1t(dfloor))
    dms = {"d1_minimum": [], "d1_frames": []}
    for _ in range(a.samples):
        for k, f in (("d1_minimum", lambda: ctx.transcode_gof_d1(src, P, d1t(dfloor))), ("d1_frames", lambda: ctx.transcode_gof_d1_frames(src, P, d1t(dfloor)))):
            t0 = time.perf_counter(); f(); dms[k].append((time.perf_counter() - t0) * 1e3)
    rec["ms"].update(dms)
    rec["d1"] = {"floor_mdb": dfloor, "r3_frames": [round(float(f["psnr"]), 3) for f in rep0["frames"]],
                 "minimum": {x: mr[1][x] for x in ("qp", "qp_start", "met", "n_encodes", "bytes", "min_d1", "mean_d1", "cloud_ms")},
                 "frames": {"qp": [f["qp"] for f in pr[1]["frames"]], "met_all": pr[1]["met_all"], "n_passes": pr[1]["n_passes"], "pictures_encoded": pr[1]["pictures_encoded"], "bytes": pr[1]["bytes"],
                            "n_encodes": [f["n_encodes"] for f in pr[1]["frames"]], "figure": [round(f["figure"], 3) for f in pr[1]["frames"]], "cloud_ms": pr[1]["cloud_ms"]},
                 "frames_equals_list": po[1] == ctx.transcode_gof_frame_qp(src, P, [None, [f["qp"] for f in pr[1]["frames"]], None])[1]}
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
    med = {k: statistics.median(v) for k, v in rec["ms"].items()}
    text = ["frame_floor: floors held frame by frame on the 1280x1280 32-frame CTC fixture, R3 (geometry QP %d, attribute QP %d), %d samples a figure" % (GEO_QP, ATTR_QP, a.samples)]
    for i, name in enumerate(("geometry", "attribute")):
        g = rec[name]
        text.append("%s: floor %.3f dB (the stream's luma PSNR at R3); constant QP %d B" % (name, rec["floors_mdb"][i] / 1000.0, rec["constant_bytes"][i]))
        text.append("  on the stream's sums : q* %d (start %d), met %d, %d encodes, %d B, %.3f dB" % (g["stream"]["qp"], g["stream"]["qp_start"], g["stream"]["met"], g["stream"]["n_encodes"], g["stream"]["bytes"], g["stream_psnr"]))
        f = g["frames"]
        text.append("  frame by frame      : %d B (%.4f of the call above), %.3f dB over the stream, met_all %d, %d passes, %d pictures encoded" % (f["bytes"], f["bytes"] / g["stream"]["bytes"], f["psnr"], f["met_all"], f["n_passes"], f["pictures_encoded"]))
        text.append("    q*_f       " + " ".join(str(q) for q in f["qp"]))
        text.append("    encodes_f  " + " ".join(str(q) for q in f["n_encodes"]))
        text.append("    figure_f   " + " ".join("%.2f" % q for q in f["figure"]))
    text.append("stream of the per-frame call equals rbt_transcode_gof_frame_qp at the picks: %s; identity list equals rbt_transcode_gof: %s" % (rec["frames_equals_list"], rec["identity_equals_constant"]))
    d = rec["d1"]; m = d["minimum"]; f = d["frames"]
    text.append("geometry, D1: floor %.3f dB (the minimum over the frames of the D1 at R3; per frame at R3: %s)" % (d["floor_mdb"] / 1000.0, " ".join("%.2f" % x for x in d["r3_frames"])))
    text.append("  on the minimum (RBT_D1_MIN): q* %d (start %d), met %d, %d encodes, %d B, min %.3f mean %.3f dB, clouds %.1f ms" % (m["qp"], m["qp_start"], m["met"], m["n_encodes"], m["bytes"], m["min_d1"], m["mean_d1"], m["cloud_ms"]))
    text.append("  frame by frame             : %d B (%.4f of the call above), met_all %d, %d passes, %d pictures encoded, clouds %.1f ms, stream equals the QP list's: %s" % (f["bytes"], f["bytes"] / m["bytes"], f["met_all"], f["n_passes"], f["pictures_encoded"], f["cloud_ms"], d["frames_equals_list"]))
    text.append("    q*_f       " + " ".join(str(q) for q in f["qp"]))
    text.append("    encodes_f  " + " ".join(str(q) for q in f["n_encodes"]))
    text.append("    figure_f   " + " ".join("%.2f" % q for q in f["figure"]))
    for k in ("constant", "identity_list", "stream", "frames", "d1_minimum", "d1_frames"):
        text.append("ms %-14s median %.1f  samples %s" % (k, med[k], " ".join("%.1f" % x for x in rec["ms"][k])))
    text.append("identity list - constant: %.1f ms (median); scatter of the constant call's samples: %.1f ms" % (med["identity_list"] - med["constant"], max(rec["ms"]["constant"]) - min(rec["ms"]["constant"])))
    out = "\n".join(text) + "\n"
    sys.stdout.write(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
