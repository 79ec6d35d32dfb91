#!/usr/bin/env python3
"""Measures the transcode of geometry to a D1 floor (rbt_transcode_gof_d1, include/rbt.h "transcoding geometry to a D1 floor") on the committed 1280x1280 32-frame CTC
fixture (tests/golden/hm_r5ctc_1280x1280_f32_*.annexb: 32 point-cloud frames, 64 geometry pictures), on one GPU. Every step is a child process of its own with a time limit
of its own; the tool itself never opens the GPU, and a step that fails ends the run.

Patches: synth.atlas_patches of the GOF's four base atlases (seed 1051 + frame % 4). Frames 4..31 are the base atlases rolled by 2 * (frame // 4) pixels (synth.make_gof_maps);
the patch rectangles lie on the 16-pixel block grid and are NOT rolled with them: all 32 frames are scored, frames 4..31 with the rectangles of their base frame, so the few
columns of samples the roll moves out of a rectangle are no points - on both sides, the reference cloud and the trial's. That is a cloud of the benchmark's size for a cost
figure, not a D1 to report for those frames.

  encodes   the D1 the constant-QP R3 transcode reaches (report only), then its minimum over the frames as the floor: q*, qs, the encodes, bytes, and the time between the
            clouds' events per trial encode
  time      --samples wall times of the call with the floor, alone and as a walk of --walk-gofs one-GOF jobs with --depth in flight; and of the report-only call against the
            PSNR floor's report-only call (one encode each, with and without the 64 clouds): what the clouds add to the call while the attribute pipeline's decoder runs
            beside them
  share     the same two report-only calls on the occupancy and geometry streams alone, so that nothing runs on the GPU beside the clouds: their wall time and the
            time between the events around them; how much of that is kernels and how much the host's waits, a kernel trace of this step says (rocprofv3 --kernel-trace --stats)
  baseline  the constant-QP call (rbt_transcode_gof / rbt_submit_gof) with --baseline-tree's build - a checkout of the parent commit, built -, alone and as the same walk; and
            the parent's PSNR-floor call at the luma PSNR its R3 transcode reaches
All samples are kept. No threshold is set for the time ratios.

    python tools/d1_target.py --baseline-tree <built checkout of the parent commit> --out profiles/d1_target.txt
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
STEP_LIMIT_S = {"encodes": 300, "time": 560, "share": 200, "baseline": 400}
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


def walk_ms(submit, wait, n_gofs, depth):
    """n_gofs one-GOF jobs, `depth` in flight, collected in order"""
    t0 = time.perf_counter(); q = []
    for _ in range(n_gofs):
        if len(q) == depth:
            wait(q.pop(0))
        q.append(submit())
    while q:
        wait(q.pop(0))
    return (time.perf_counter() - t0) * 1e3


def open_ctx(tree):
    sys.path.insert(0, os.path.join(tree, "tests"))
    import rbt_lib
    R = rbt_lib.module(); gs = rbt_lib.module_file("gof_shard")
    return R, gs, R.Context(device=0)


def targets(R, floor=0):
    import synth
    atlas = R.ctc_smoothing(R.AtlasParams(W, H, 16, 4, 2, 1, 1, 0))
    patches = [synth.atlas_patches(R, W, H, SEED + f % 4) for f in range(N_FRAMES)]
    return [R.D1Target(), R.D1Target(atlas, patches, floor), R.D1Target()]


def step_encodes(a):
    R, gs, ctx = open_ctx(ROOT)
    streams = fixture(); P = gs.rate_params(R, 3)
    _, r3 = ctx.transcode_gof_d1(streams, P, targets(R))
    floor = int(r3[1]["min_d1"] * 1000)            # truncated: the constant-QP stream itself meets it
    _, res = ctx.transcode_gof_d1(streams, P, targets(R, floor))
    pick = lambda r: {k: r[k] for k in ("qp", "qp_probe", "qp_start", "met", "n_encodes", "bytes", "mean_d1", "min_d1", "cloud_ms")}
    out = {"floor_mdb": floor, "r3": pick(r3[1]), "walk": pick(res[1]), "points": [r3[1]["frames"][0]["n_a"], r3[1]["frames"][0]["n_b"]]}
    ctx.close()
    return out


def step_time(a):
    R, gs, ctx = open_ctx(ROOT)
    streams = fixture(); P = gs.rate_params(R, 3); tg = targets(R, int(a.floor)); rep = targets(R)
    ctx.set_depth(4); ctx.transcode_gof_d1(streams, P, tg)                                # warm-up: arenas and volumes cached
    out = {"gof_ms": timed(lambda: ctx.transcode_gof_d1(streams, P, tg), a.samples)}
    ctx.transcode_gof_quality(streams, P, [R.QualityTarget()] * 3)
    out["report_d1_ms"] = timed(lambda: ctx.transcode_gof_d1(streams, P, rep), a.samples)
    out["report_d1_cloud_ms"] = ctx.transcode_gof_d1(streams, P, rep)[1][1]["cloud_ms"]
    out["report_psnr_ms"] = timed(lambda: ctx.transcode_gof_quality(streams, P, [R.QualityTarget()] * 3), a.samples)
    ctx.set_depth(a.depth)
    sub, wait = (lambda: ctx.submit_gof_d1(streams, P, tg)), ctx.wait_gof_d1
    walk_ms(sub, wait, a.depth, a.depth)
    out["walk_ms"] = [walk_ms(sub, wait, a.walk_gofs, a.depth) for _ in range(a.walk_samples)]
    ctx.close()
    return out


def step_share(a):
    R, gs, ctx = open_ctx(ROOT)
    streams = fixture()[:2]; P = gs.rate_params(R, 3)[:2]; rep = targets(R)[:2]; q = [R.QualityTarget()] * 2
    ctx.transcode_gof_d1(streams, P, rep); ctx.transcode_gof_quality(streams, P, q)     # warm-up
    out = {"d1_ms": [], "cloud_ms": []}
    for _ in range(a.samples):
        t0 = time.perf_counter(); res = ctx.transcode_gof_d1(streams, P, rep)[1]; out["d1_ms"].append((time.perf_counter() - t0) * 1e3); out["cloud_ms"].append(res[1]["cloud_ms"])
    out["psnr_ms"] = timed(lambda: ctx.transcode_gof_quality(streams, P, q), a.samples)
    ctx.close()
    return out


def say_share(say, fmt, med, s):
    say("occupancy and geometry alone, report only, one encode: with the 64 clouds ms %s; the PSNR floor's report-only call ms %s: the clouds cost %.1f ms of wall time; the time between the events "
        "around them on the pipeline's stream is ms %s - kernels and the gaps in which the stream waits for the host's read-backs and launches; a kernel trace of this step (rocprofv3 --kernel-trace --stats "
        "-- python tools/d1_target.py --step share) says how much of it is kernels" % (fmt(s["d1_ms"]), fmt(s["psnr_ms"]), med(s["d1_ms"]) - med(s["psnr_ms"]), fmt(s["cloud_ms"])))


def step_baseline(a):
    R, gs, ctx = open_ctx(a.baseline_tree)
    streams = fixture(); P = gs.rate_params(R, 3)
    ctx.set_depth(4); ctx.transcode_gof(streams, P)
    out = {"gof_ms": timed(lambda: ctx.transcode_gof(streams, P), a.samples)}
    _, r3 = ctx.transcode_gof_quality(streams, P, [R.QualityTarget()] * 3)
    tg = [R.QualityTarget(), R.QualityTarget(int(r3[1]["psnr"][0] * 1000)), R.QualityTarget()]
    ctx.transcode_gof_quality(streams, P, tg)
    out["psnr_gof_ms"] = timed(lambda: ctx.transcode_gof_quality(streams, P, tg), a.samples)
    ctx.set_depth(a.depth)
    sub, wait = (lambda: ctx.submit_gof(streams, P)), ctx.wait_gof
    walk_ms(sub, wait, a.depth, a.depth)
    out["walk_ms"] = [walk_ms(sub, wait, a.walk_gofs, a.depth) for _ in range(a.walk_samples)]
    sub, wait = (lambda: ctx.submit_gof_quality(streams, P, tg)), ctx.wait_gof_quality
    walk_ms(sub, wait, a.depth, a.depth)
    out["psnr_walk_ms"] = [walk_ms(sub, wait, a.walk_gofs, a.depth) for _ in range(a.walk_samples)]
    ctx.close()
    return out


STEPS = {"encodes": step_encodes, "time": step_time, "share": step_share, "baseline": step_baseline}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--walk-samples", type=int, default=2)
    ap.add_argument("--walk-gofs", type=int, default=16)
    ap.add_argument("--depth", type=int, default=16)
    ap.add_argument("--baseline-tree", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    ap.add_argument("--floor", default="0", help=argparse.SUPPRESS)
    ap.add_argument("--only-share", action="store_true", help="the share step alone, its line appended to --out")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(STEPS[a.step](a)))
        return
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def run(step, extra=()):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--samples", str(a.samples), "--walk-samples", str(a.walk_samples), "--walk-gofs", str(a.walk_gofs), "--depth", str(a.depth),
               "--baseline-tree", a.baseline_tree] + list(extra)
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

    def finish_append():
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")

    med = statistics.median
    fmt = lambda v: "[%s] (median %.1f, min %.1f, max %.1f)" % (", ".join("%.1f" % x for x in v), med(v), min(v), max(v))
    if a.only_share:
        s = run("share")
        if s is not None:
            say("(the share step, run alone in a second session:)"); say_share(say, fmt, med, s)
        return finish_append()
    say("Transcode of geometry to a D1 floor (rbt_transcode_gof_d1), one MI355X, tools/d1_target.py, one session; all samples kept; every step a process of its own.")
    say("Benchmark GOF: 32 point-cloud frames of 1280x1280, geometry smoothing on (grid 8, threshold 64); all 32 frames scored, patch rectangles of the base atlases not rolled (see the tool's text).")
    e = run("encodes")
    if e is None:
        return finish()
    r3, wk = e["r3"], e["walk"]
    say("constant QP %d (R3): %d B, D1 mean %.3f dB, min %.3f dB over 32 frames (frame 0: %d reference points, %d trial points after merging); clouds: %.1f ms between the clouds' events for 32 reference and 32 trial clouds" %
        (r3["qp"], r3["bytes"], r3["mean_d1"], r3["min_d1"], e["points"][0], e["points"][1], r3["cloud_ms"]))
    say("floor %d mdB on the minimum -> probe %d, start %d, q* %d, met %d, %d encodes, |q* - qs| %d, %d B, D1 mean %.3f dB, min %.3f dB; clouds: %.1f ms between the clouds' events, %.1f ms per trial encode (32 clouds each; the 32 reference clouds included once)" %
        (e["floor_mdb"], wk["qp_probe"], wk["qp_start"], wk["qp"], wk["met"], wk["n_encodes"], abs(wk["qp"] - wk["qp_start"]), wk["bytes"], wk["mean_d1"], wk["min_d1"], wk["cloud_ms"], wk["cloud_ms"] / max(1, wk["n_encodes"])))
    t = run("time", ["--floor", str(e["floor_mdb"])])
    if t is None:
        return finish()
    say("one GOF with the floor: ms %s; %d GOFs, %d in flight: ms %s" % (fmt(t["gof_ms"]), a.walk_gofs, a.depth, fmt(t["walk_ms"])))
    say("report only, one encode: with the 64 clouds ms %s; the PSNR floor's report-only call ms %s: the clouds add %.1f ms to the call; their device time between events is %.1f ms (they run beside the attribute pipeline's decoder, "
        "which slows their kernels down and hides part of them)" % (fmt(t["report_d1_ms"]), fmt(t["report_psnr_ms"]), med(t["report_d1_ms"]) - med(t["report_psnr_ms"]), t["report_d1_cloud_ms"]))
    s = run("share")
    if s is None:
        return finish()
    say_share(say, fmt, med, s)
    b = run("baseline") if a.baseline_tree else None
    if b:
        say("build of the parent commit: constant QP one GOF ms %s; walk ms %s; PSNR floor one GOF ms %s; walk ms %s" % (fmt(b["gof_ms"]), fmt(b["walk_ms"]), fmt(b["psnr_gof_ms"]), fmt(b["psnr_walk_ms"])))
        say("ratios of the medians: D1 floor / constant QP %.2f (one GOF) and %.2f (walk); D1 floor / PSNR floor %.2f (one GOF) and %.2f (walk)" %
            (med(t["gof_ms"]) / med(b["gof_ms"]), med(t["walk_ms"]) / med(b["walk_ms"]), med(t["gof_ms"]) / med(b["psnr_gof_ms"]), med(t["walk_ms"]) / med(b["psnr_walk_ms"])))
    finish()


if __name__ == "__main__":
    main()
