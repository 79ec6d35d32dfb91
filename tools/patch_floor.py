#!/usr/bin/env python3
"""Measures the PSNR floors held patch by patch (rbt_transcode_gof_quality_patches, include/rbt.h "PSNR floors held patch by patch") on the benchmark GOF - the committed
1280x1280 32-frame fixture (tests/golden/hm_r5_1280x1280_f32_*.annexb) transcoded to R3 - on one GPU. Every step is a child process of its own with a time limit of its own;
the tool itself never opens the GPU, and a step that fails ends the run.

  kernel   device time between events around the launches of k_ctb_sse + k_patch_fold (rbt_get_stats after rbt_ctb_sse) for 64 pictures of 1280x1280 with a map of scale 4 and
           the rectangles of the first atlas, and of k_picture_sse (rbt_picture_sse) on the same pictures in the same process
  bytes    the floors are the stream's own luma PSNR at R3 (rbt_transcode_gof_quality without floors, truncated to 1/1000 dB). Three walks side by side: the floor per patch,
           the floor per frame (rbt_transcode_gof_quality_frames), the floor on the stream (rbt_transcode_gof_quality): bytes, met, the encodes; for the floor per patch the
           histogram of the patches' QPs, the trials per frame and the passes
  time     --samples wall times per GOF of the three calls and of rbt_transcode_gof, interleaved in one process
  bench    with --baseline-tree (a built checkout of the parent commit): bench.py --gpus 1 --steps 20 --warmup 5 of this tree and of that one, three runs each, interleaved,
           all six values; this tree's median may lie below the parent's median by no more than max - min of the parent's own three runs
Patches: synth.atlas_patches of the four base atlases; frames 4..31 are those atlases rolled by a few pixels, their rectangles are not rolled with them (a CTB is 32
samples). All samples are kept. Whether the floor per patch is cheaper than the floor per frame is the finding, whichever way it falls: no threshold is set.

    python tools/patch_floor.py [--baseline-tree <built checkout of the parent commit>] --out profiles/patch_floor.txt
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
STEP_LIMIT_S = {"kernel": 120, "bytes": 300, "time": 420, "bench": 240}
W = H = 1280
SEED = 1051
GEO_QP, ATTR_QP = 24, 32          # R3
L2 = 5


def fixture():
    return [open(os.path.join(GOLD, "hm_r5_1280x1280_f32_%s.annexb" % k), "rb").read() for k in ("occ", "geo", "attr")]


def open_ctx():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rbt_lib
    import synth
    R = rbt_lib.module()
    return R, synth, R.Context(device=0)


def params(R):
    return [R.StreamParams(0, 8, 4, L2, -1, 0, 0, 0, 0), R.StreamParams(1, GEO_QP, 4, L2, -1, 0, 0, 0, 0), R.StreamParams(19, ATTR_QP, 4, L2, -1, 0, 0, 0, 0)]


def patch_targets(R, synth, floors, n_pc=32):
    atlas = R.AtlasParams(W, H, 16, 4, 2, 1, 1, 0)
    pats = [synth.atlas_patches(R, W, H, SEED + f % 4) for f in range(n_pc)]
    return [R.PatchFloorTarget()] + [R.PatchFloorTarget(atlas, pats, min_psnr_mdb=f) for f in floors]


def step_kernel(a):
    import numpy as np
    R, synth, ctx = open_ctx()
    n = 64
    r = np.random.default_rng(1)
    pa = r.integers(0, 1024, (n, W * H * 3 // 2)).astype(np.uint16)
    pb = np.clip(pa.astype(np.int32) + r.integers(-6, 7, pa.shape), 0, 1023).astype(np.uint16)
    occ = (r.random((n, H // 4, W // 4)) < 0.45).astype(np.uint16)
    rects = []
    for p in synth.atlas_patches(R, W, H, SEED):
        rects.append([(p.u0 * 16) >> L2, (p.v0 * 16) >> L2, (((p.u0 + p.size_u0) * 16 - 1) >> L2) + 1, (((p.v0 + p.size_v0) * 16 - 1) >> L2) + 1])
    out = {"n_rects": len(rects), "bytes": int((pa.nbytes + pb.nbytes) * 2 // 3), "ctb": [], "picture": []}      # luma alone: two thirds of a 4:2:0 picture
    ctx.ctb_sse(pa, pb, W, H, L2, occ, rects); ctx.picture_sse(pa, pb, W, H, occ)
    for _ in range(a.samples):
        ctx.ctb_sse(pa, pb, W, H, L2, occ, rects); out["ctb"].append(ctx.stats()["gpu_ms"])
        ctx.picture_sse(pa, pb, W, H, occ); out["picture"].append(ctx.stats()["gpu_ms"])
    ctx.close()
    return out


def step_bytes(a):
    R, synth, ctx = open_ctx()
    src, P = fixture(), params(R)
    outs, r3 = ctx.transcode_gof_quality(src, P, [R.QualityTarget()] * 3)
    floors = [int(r3[i]["psnr"][0] * 1000) for i in (1, 2)]          # truncated: the constant-QP stream itself meets them
    out = {"floors": floors, "r3": [{k: r3[i][k] for k in ("qp", "bytes")} for i in (1, 2)]}
    _, rs = ctx.transcode_gof_quality(src, P, [R.QualityTarget()] + [R.QualityTarget(f) for f in floors])
    out["stream"] = [{k: rs[i][k] for k in ("qp", "met", "n_encodes", "bytes")} for i in (1, 2)]
    _, rf = ctx.transcode_gof_quality_frames(src, P, [R.QualityTarget()] + [R.QualityTarget(f) for f in floors])
    out["frames"] = [{"bytes": rf[i]["bytes"], "met_all": rf[i]["met_all"], "n_passes": rf[i]["n_passes"], "pictures": rf[i]["pictures_encoded"], "qp": [x["qp"] for x in rf[i]["frames"]]} for i in (1, 2)]
    _, rp = ctx.transcode_gof_quality_patches(src, P, patch_targets(R, synth, floors))
    out["patches"] = []
    for i in (1, 2):
        hist = {}
        for fr in rp[i]["frames"]:
            for p in fr["patches"]:
                hist[p["qp"]] = hist.get(p["qp"], 0) + 1
        out["patches"].append({"bytes": rp[i]["bytes"], "met_all": rp[i]["met_all"], "n_passes": rp[i]["n_passes"], "pictures": rp[i]["pictures_encoded"],
                               "trials": [fr["n_trials"] for fr in rp[i]["frames"]], "qp_hist": sorted(hist.items()), "not_met": sum(1 for fr in rp[i]["frames"] for p in fr["patches"] if not p["met"]),
                               "n_patches": sum(fr["n_patches"] for fr in rp[i]["frames"])})
    ctx.close()
    return out


def step_time(a):
    R, synth, ctx = open_ctx()
    src, P = fixture(), params(R); floors = json.loads(a.floors)
    QT = [R.QualityTarget()] + [R.QualityTarget(f) for f in floors]; PT = patch_targets(R, synth, floors)
    calls = {"patches": lambda: ctx.transcode_gof_quality_patches(src, P, PT), "frames": lambda: ctx.transcode_gof_quality_frames(src, P, QT),
             "stream": lambda: ctx.transcode_gof_quality(src, P, QT), "constant": lambda: ctx.transcode_gof(src, P)}
    out = {k: [] for k in calls}
    for f in calls.values():
        f()                                                            # warm-up: arenas cached
    for _ in range(a.samples):
        for k, f in calls.items():
            t0 = time.perf_counter(); f(); out[k].append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    return out


STEPS = {"kernel": step_kernel, "bytes": step_bytes, "time": step_time}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--baseline-tree", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    ap.add_argument("--floors", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(STEPS[a.step](a)))
        return
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def finish():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def run(step, extra=()):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--samples", str(a.samples)] + list(extra)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S[step])
        except subprocess.TimeoutExpired:
            say("step %s did not end within %d s: the run ends here" % (step, STEP_LIMIT_S[step])); return None
        line = next((x for x in r.stdout.splitlines() if x.startswith("RESULT ")), None)
        if r.returncode or line is None:
            say("step %s failed (exit status %d): the run ends here\n%s" % (step, r.returncode, r.stderr[-600:])); return None
        return json.loads(line[7:])

    med = statistics.median
    fm = lambda v: " ".join("%.3f" % x for x in v)
    say("PSNR floors held patch by patch (rbt_transcode_gof_quality_patches) on the benchmark GOF (1280x1280, 32 frames), R3 (geometry QP %d, attribute QP %d), CTBs of %d, one MI355X, "
        "tools/patch_floor.py, one session; all samples kept; every step a process of its own." % (GEO_QP, ATTR_QP, 1 << L2))
    k = run("kernel")
    if k is None:
        return finish()
    say("k_ctb_sse + k_patch_fold, 64 pictures of 1280x1280, map of scale 4, %d rectangles a frame: device ms %s (median %.3f): %.0f GB/s of luma bytes" % (k["n_rects"], fm(k["ctb"]), med(k["ctb"]), k["bytes"] / med(k["ctb"]) / 1e6))
    say("k_picture_sse on the same pictures (three planes), same process: device ms %s (median %.3f)" % (fm(k["picture"]), med(k["picture"])))
    b = run("bytes")
    if b is None:
        return finish()
    for i, kind in enumerate(("geometry", "attribute")):
        p, f, s, r3 = b["patches"][i], b["frames"][i], b["stream"][i], b["r3"][i]
        say("%-9s floor %d mdB (the constant-QP stream's own luma PSNR at QP %d, %d B):" % (kind, b["floors"][i], r3["qp"], r3["bytes"]))
        say("          floor per patch  %8d B (%.4f of constant), met_all %d (%d of %d patches miss it), %d passes, %d pictures encoded, trials per frame %s" %
            (p["bytes"], p["bytes"] / r3["bytes"], p["met_all"], p["not_met"], p["n_patches"], p["n_passes"], p["pictures"], " ".join(str(x) for x in p["trials"])))
        say("                           QP histogram of the patches (QP:count) %s" % " ".join("%d:%d" % (q, c) for q, c in p["qp_hist"]))
        say("          floor per frame  %8d B (%.4f of constant), met_all %d, %d passes, %d pictures encoded, QPs %s" % (f["bytes"], f["bytes"] / r3["bytes"], f["met_all"], f["n_passes"], f["pictures"], " ".join(str(x) for x in f["qp"])))
        say("          floor on stream  %8d B (%.4f of constant), met %d, q* %d, %d encodes" % (s["bytes"], s["bytes"] / r3["bytes"], s["met"], s["qp"], s["n_encodes"]))
        say("          per patch / per frame: %.4f" % (p["bytes"] / f["bytes"]))
    t = run("time", ["--floors", json.dumps(b["floors"])])
    if t is None:
        return finish()
    for name, label in (("patches", "floor per patch"), ("frames", "floor per frame"), ("stream", "floor on stream"), ("constant", "rbt_transcode_gof")):
        say("%-17s one GOF: ms %s (median %.1f, %.2f x rbt_transcode_gof)" % (label, " ".join("%.1f" % x for x in t[name]), med(t[name]), med(t[name]) / med(t["constant"])))
    if a.baseline_tree:
        fps = {"this tree": [], "parent": []}
        for _ in range(3):
            for name, tree in (("this tree", ROOT), ("parent", os.path.abspath(a.baseline_tree))):
                try:
                    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree, capture_output=True, text=True, timeout=STEP_LIMIT_S["bench"])
                except subprocess.TimeoutExpired:
                    say("bench.py of %s did not end within %d s: the run ends here" % (name, STEP_LIMIT_S["bench"])); return finish()
                if r.returncode:
                    say("bench.py of %s failed (exit status %d): the run ends here\n%s" % (name, r.returncode, r.stderr[-600:])); return finish()
                fps[name].append(float(json.loads(r.stdout.strip().splitlines()[-1])["value"]))
                print("  bench.py of %s: %.1f" % (name, fps[name][-1]), file=sys.stderr, flush=True)
        spread = max(fps["parent"]) - min(fps["parent"]); gap = med(fps["parent"]) - med(fps["this tree"])
        say("bench.py --gpus 1 --steps 20 --warmup 5, point-cloud frames/s, interleaved: this tree %s (median %.1f) | build of the parent commit %s (median %.1f, spread %.1f): this tree's median is %.1f %s, %s" %
            (" ".join("%.1f" % x for x in fps["this tree"]), med(fps["this tree"]), " ".join("%.1f" % x for x in fps["parent"]), med(fps["parent"]), spread, abs(gap), "below" if gap > 0 else "above",
             "within the parent's spread" if gap <= spread else "MORE THAN THE PARENT'S SPREAD BELOW"))
    else:
        say("bench.py against a build of the parent commit: not measured (no --baseline-tree)")
    finish()


if __name__ == "__main__":
    main()
