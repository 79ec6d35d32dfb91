#!/usr/bin/env python3
"""Measures the transcode of attributes to a colour PSNR floor (rbt_transcode_gof_color, include/rbt.h "transcoding attributes to a colour PSNR floor") on the committed
1280x1280 32-frame CTC fixture (tests/golden/hm_r5ctc_1280x1280_f32_*.annexb: 32 point-cloud frames, 64 geometry and 64 attribute pictures), on one GPU. Every step is a
child process of its own with a time limit of its own; the tool itself never opens the GPU, and a step that fails ends the run.

Patches: as tools/d1_target.py takes them - synth.atlas_patches of the GOF's four base atlases, not rolled with frames 4..31: clouds of the benchmark's size for a cost
figure, not a colour PSNR to report for those frames.

  encodes   the colour Y-PSNR the constant-QP R3 transcode reaches (report only), then its minimum and its mean over the frames as floors: q*, qs, the encodes, bytes
  time      --samples wall times of the call with the floor on the minimum against rbt_transcode_gof at R3 in the same process
  clouds    the time between the clouds' events (cloud_ms) of the report-only call (geometry half, references, one trial) and of the call with the floor (the same and
            n_encodes trials): the difference per further trial and cloud is the recolour route's cost; against the public route for the same frames in the same
            process, rbt_pcloud_from_maps + rbt_score(RBT_SCORE_COLOR) on the decoded streams of the R3 transcode, wall time per cloud over --route-frames frames
All samples are kept. No threshold is set.

    python tools/color_target.py --out profiles/color_target.txt
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
STEP_LIMIT_S = {"encodes": 300, "time": 400, "clouds": 400}
W = H = 1280
N_FRAMES = 32
SEED = 1051


def fixture():
    return [open(os.path.join(GOLD, "hm_r5ctc_1280x1280_f32_%s.annexb" % k), "rb").read() for k in ("occ", "geo", "attr")]


def timed(f, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter(); f(); out.append((time.perf_counter() - t0) * 1e3)
    return out


def open_ctx():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rbt_lib
    R = rbt_lib.module(); gs = rbt_lib.module_file("gof_shard")
    return R, gs, R.Context(device=0)


def atlas_and_patches(R):
    import synth
    return R.ctc_smoothing(R.AtlasParams(W, H, 16, 4, 2, 1, 1, 0)), [synth.atlas_patches(R, W, H, SEED + f % 4) for f in range(N_FRAMES)]


def targets(R, floor=0, stat=0):
    atlas, patches = atlas_and_patches(R)
    return [R.ColorTarget(), R.ColorTarget(), R.ColorTarget(atlas, patches, floor, 0, stat)]


PICK = ("qp", "qp_probe", "qp_start", "met", "n_encodes", "bytes", "mean_psnr", "min_psnr", "cloud_ms")


def step_encodes(a):
    R, gs, ctx = open_ctx()
    streams = fixture(); P = gs.rate_params(R, 3)
    _, r3 = ctx.transcode_gof_color(streams, P, targets(R))
    pick = lambda r: {k: r[k] for k in PICK}
    out = {"r3": pick(r3[2]), "points": [r3[2]["frames"][0]["n_a"], r3[2]["frames"][0]["n_b"]]}
    for name, stat, db in (("min", 0, r3[2]["min_psnr"][0]), ("mean", 1, r3[2]["mean_psnr"][0])):
        floor = int(db * 1000)                         # truncated: the constant-QP stream itself meets it
        out[name] = dict(pick(ctx.transcode_gof_color(streams, P, targets(R, floor, stat))[1][2]), floor_mdb=floor)
    ctx.close()
    return out


def step_time(a):
    R, gs, ctx = open_ctx()
    streams = fixture(); P = gs.rate_params(R, 3); tg = targets(R, int(a.floor))
    ctx.transcode_gof_color(streams, P, tg); ctx.transcode_gof(streams, P)                 # warm-up: arenas and volumes cached
    out = {"color_ms": [], "plain_ms": []}
    for _ in range(a.samples):                                                           # interleaved
        out["color_ms"] += timed(lambda: ctx.transcode_gof_color(streams, P, tg), 1)
        out["plain_ms"] += timed(lambda: ctx.transcode_gof(streams, P), 1)
    ctx.close()
    return out


def step_clouds(a):
    import numpy as np
    R, gs, ctx = open_ctx()
    streams = fixture(); P = gs.rate_params(R, 3); tg = targets(R, int(a.floor)); rep = targets(R)
    ctx.transcode_gof_color(streams, P, tg)                                              # warm-up
    out = {"report_cloud_ms": [], "walk_cloud_ms": [], "n_encodes": 0, "route_ms_per_cloud": [], "route_frames": a.route_frames}
    for _ in range(a.samples):
        out["report_cloud_ms"].append(ctx.transcode_gof_color(streams, P, rep)[1][2]["cloud_ms"])
        r = ctx.transcode_gof_color(streams, P, tg)[1][2]
        out["walk_cloud_ms"].append(r["cloud_ms"]); out["n_encodes"] = r["n_encodes"]
    # the public route on the decoded output of the R3 transcode, against the clouds of the decoded input
    atlas, patches = atlas_and_patches(R)
    luma = lambda fr: fr[:W * H].reshape(H, W)
    def maps(s, prec):
        om, ow, oh, *_ = ctx.decode(s[0], verify_md5=False); g, *_ = ctx.decode(s[1], verify_md5=False); t, *_ = ctx.decode(s[2], verify_md5=False)
        at = R.AtlasParams(*[getattr(atlas, n) for n, _ in R.AtlasParams._fields_]); at.occupancy_precision = prec
        return at, [om[f][:ow * oh].reshape(oh, ow) for f in range(N_FRAMES)], g, t
    outs = ctx.transcode_gof(streams, P)
    ain, occ_in, g_in, t_in = maps(streams, 2)
    aout, occ_out, g_out, t_out = maps(outs, 4)
    nf = a.route_frames
    A = [ctx.pcloud_from_maps(ain, patches[f], occ_in[f], luma(g_in[2 * f]), luma(g_in[2 * f + 1]), 10, t_in[2 * f], t_in[2 * f + 1], 10) for f in range(nf)]
    def route():
        for f in range(nf):
            b = ctx.pcloud_from_maps(aout, patches[f], occ_out[f], luma(g_out[2 * f]), luma(g_out[2 * f + 1]), 10, t_out[2 * f], t_out[2 * f + 1], 10)
            ctx.score(A[f], b, parts=R.RBT_SCORE_COLOR)
            b.release()
    route()
    out["route_ms_per_cloud"] = [x / nf for x in timed(route, a.samples)]
    for h in A: h.release()
    ctx.close()
    return out


STEPS = {"encodes": step_encodes, "time": step_time, "clouds": step_clouds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--route-frames", type=int, default=8)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    ap.add_argument("--floor", default="0", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        print(json.dumps(STEPS[a.step](a)))
        return
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def run(step, extra=()):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--samples", str(a.samples), "--route-frames", str(a.route_frames)] + list(extra)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S[step])
        except subprocess.TimeoutExpired:
            say("step %s did not end within %d s: the run ends here" % (step, STEP_LIMIT_S[step])); return None
        if r.returncode:
            say("step %s failed (exit status %d): the run ends here\n%s" % (step, r.returncode, r.stderr[-600:])); return None
        return json.loads(r.stdout.strip().splitlines()[-1])

    def finish():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    med = statistics.median
    fmt = lambda v: "[%s] (median %.1f, min %.1f, max %.1f)" % (", ".join("%.1f" % x for x in v), med(v), min(v), max(v))
    say("Transcode of attributes to a colour PSNR floor (rbt_transcode_gof_color), one MI355X, tools/color_target.py, one session; all samples kept; every step a process of its own.")
    say("Benchmark GOF: 32 point-cloud frames of 1280x1280, geometry smoothing on (grid 8, threshold 64), attribute transfer on; all 32 frames scored, patch rectangles of the base atlases not rolled (see the tool's text).")
    e = run("encodes")
    if e is None:
        return finish()
    r3 = e["r3"]
    say("constant QP %d (R3): attribute stream %d B, colour PSNR Y mean %.3f dB, min %.3f dB (U %.3f / %.3f, V %.3f / %.3f) over 32 frames (frame 0: %d reference points, %d trial points after merging); clouds: %.1f ms between the clouds' events" %
        (r3["qp"], r3["bytes"], r3["mean_psnr"][0], r3["min_psnr"][0], r3["mean_psnr"][1], r3["min_psnr"][1], r3["mean_psnr"][2], r3["min_psnr"][2], e["points"][0], e["points"][1], r3["cloud_ms"]))
    for name in ("min", "mean"):
        wk = e[name]
        say("(a) floor %d mdB on the %s of Y -> probe %d, start %d, q* %d, met %d, %d encodes, |q* - qs| %d, %d B, Y mean %.3f dB, min %.3f dB; clouds: %.1f ms between the clouds' events" %
            (wk["floor_mdb"], name, wk["qp_probe"], wk["qp_start"], wk["qp"], wk["met"], wk["n_encodes"], abs(wk["qp"] - wk["qp_start"]), wk["bytes"], wk["mean_psnr"][0], wk["min_psnr"][0], wk["cloud_ms"]))
    t = run("time", ["--floor", str(e["min"]["floor_mdb"])])
    if t is None:
        return finish()
    say("(a) one GOF with the floor on the minimum: ms %s; rbt_transcode_gof at R3 in the same process, interleaved: ms %s; ratio of the medians %.2f" %
        (fmt(t["color_ms"]), fmt(t["plain_ms"]), med(t["color_ms"]) / med(t["plain_ms"])))
    c = run("clouds", ["--floor", str(e["min"]["floor_mdb"])])
    if c is None:
        return finish()
    n = max(1, c["n_encodes"] - 1)
    per = [(w - r) / n / N_FRAMES for w, r in zip(c["walk_cloud_ms"], c["report_cloud_ms"])]
    say("(b) time between the clouds' events: report only (geometry half, 32 references, one trial of 32 clouds) ms %s; with the floor (%d trials) ms %s; per further trial and cloud ms %s" %
        (fmt(c["report_cloud_ms"]), c["n_encodes"], fmt(c["walk_cloud_ms"]), "[%s] (median %.2f)" % (", ".join("%.2f" % x for x in per), med(per))))
    rt = c["route_ms_per_cloud"]
    say("(b) the public route in the same process, rbt_pcloud_from_maps + rbt_score(RBT_SCORE_COLOR) on the decoded R3 output, wall time per cloud over %d frames: ms %s; spread %.2f; the recolour route per trial and cloud is %.2f of it" %
        (c["route_frames"], "[%s] (median %.2f)" % (", ".join("%.2f" % x for x in rt), med(rt)), max(rt) - min(rt), med(per) / med(rt)))
    finish()


if __name__ == "__main__":
    main()
