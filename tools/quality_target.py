#!/usr/bin/env python3
"""Measures the transcode to a PSNR floor (rbt_transcode_gof_quality, include/rbt.h "transcoding to a PSNR floor") on the committed 1280x1280 32-frame CTC fixture
(tests/golden/hm_r5ctc_1280x1280_f32_*.annexb), on one GPU. Every step is a child process of its own with a time limit of its own; the tool itself never opens the GPU, and
a step that fails ends the run.

  kernel    device time between events around the launches of k_picture_sse (rbt_get_stats after rbt_picture_sse) for 64 pictures of 1280x1280, with and without an occupancy map
  encodes   the luma PSNRs the constant-QP R3 transcode reaches (geometry and attribute, all samples and occupied - rbt_transcode_gof_quality without floors), then those
            PSNRs as floors: q*, qs, |q* - qs|, the encodes; all samples, and occupied (with occupancy_rd, against the R3 transcode with occupancy_rd)
  time      --samples wall times of the call with floors, alone and as a walk of --walk-gofs one-GOF jobs with --depth in flight
  baseline  the constant-QP call (rbt_transcode_gof / rbt_submit_gof) with --baseline-tree's build - a checkout of the parent commit, built -, alone and as the same walk: the
            time ratios are against that build, never against this branch's own constant-QP path
  bench     the constant-QP path must not slow down: bench.py --gpus 1 --steps 20 --warmup 5 of this tree and of --baseline-tree, three runs each, interleaved, all six
            values; this tree's median may lie below the baseline's median by no more than max - min of the baseline's own three runs
All samples are kept. No threshold is set for the time ratios.

    python tools/quality_target.py --baseline-tree <built checkout of the parent commit> --out profiles/quality_target.txt
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
STEP_LIMIT_S = {"kernel": 120, "encodes": 240, "time": 420, "baseline": 240, "bench": 240}


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


def step_kernel(a):
    import numpy as np
    R, gs, ctx = open_ctx(ROOT)
    w = h = 1280; n = 64
    r = np.random.default_rng(1)
    pa = r.integers(0, 1024, (n, w * h * 3 // 2)).astype(np.uint16)
    pb = np.clip(pa.astype(np.int32) + r.integers(-6, 7, pa.shape), 0, 1023).astype(np.uint16)
    occ = (r.random((n, h // 4, w // 4)) < 0.45).astype(np.uint16)
    out = {}
    for name, m in (("no_map", None), ("map_scale_4", occ)):
        ctx.picture_sse(pa, pb, w, h, m)
        ms = []
        for _ in range(a.samples):
            ctx.picture_sse(pa, pb, w, h, m); ms.append(ctx.stats()["gpu_ms"])
        out[name] = ms
    out["bytes"] = int(pa.nbytes + pb.nbytes)
    ctx.close()
    return out


def floors_of(res, k, key):
    return int(res[k][key][0] * 1000)          # truncated: the constant-QP stream itself meets it


def step_encodes(a):
    R, gs, ctx = open_ctx(ROOT)
    streams = fixture(); out = {}
    for rd, region, name in ((0, R.RBT_QUALITY_ALL, "all"), (1, R.RBT_QUALITY_OCCUPIED, "occupied")):
        P = gs.rate_params(R, 3, occupancy_rd=rd)
        outs, r3 = ctx.transcode_gof_quality(streams, P, [R.QualityTarget()] * 3)
        key = "psnr_occ" if region else "psnr"
        tg = [R.QualityTarget(), R.QualityTarget(floors_of(r3, 1, key), region), R.QualityTarget(floors_of(r3, 2, key), region)]
        outs2, res = ctx.transcode_gof_quality(streams, P, tg)
        out[name] = {"occupancy_rd": rd, "r3": [{k: r3[i][k] for k in ("qp", "bytes", "psnr", "psnr_occ")} for i in (1, 2)],
                     "floor_mdb": [tg[1].min_psnr_mdb, tg[2].min_psnr_mdb],
                     "walk": [{k: res[i][k] for k in ("qp", "qp_probe", "qp_start", "met", "n_encodes", "bytes", "psnr", "psnr_occ")} for i in (1, 2)]}
    ctx.close()
    return out


def step_time(a):
    R, gs, ctx = open_ctx(ROOT)
    streams = fixture(); floors = json.loads(a.floors); out = {}
    for name, rd, region in (("all", 0, R.RBT_QUALITY_ALL), ("occupied", 1, R.RBT_QUALITY_OCCUPIED)):
        P = gs.rate_params(R, 3, occupancy_rd=rd)
        tg = [R.QualityTarget(), R.QualityTarget(floors[name][0], region), R.QualityTarget(floors[name][1], region)]
        ctx.set_depth(4); ctx.transcode_gof_quality(streams, P, tg)                       # warm-up: arenas cached
        one = timed(lambda: ctx.transcode_gof_quality(streams, P, tg), a.samples)
        ctx.set_depth(a.depth)
        sub, wait = (lambda: ctx.submit_gof_quality(streams, P, tg)), ctx.wait_gof_quality
        walk_ms(sub, wait, a.depth, a.depth)
        out[name] = {"gof_ms": one, "walk_ms": [walk_ms(sub, wait, a.walk_gofs, a.depth) for _ in range(a.walk_samples)]}
    ctx.close()
    return out


def step_baseline(a):
    R, gs, ctx = open_ctx(a.baseline_tree)
    streams = fixture(); out = {}
    for name, rd in (("all", 0), ("occupied", 1)):
        P = gs.rate_params(R, 3, occupancy_rd=rd)
        ctx.set_depth(4); ctx.transcode_gof(streams, P)
        one = timed(lambda: ctx.transcode_gof(streams, P), a.samples)
        ctx.set_depth(a.depth)
        sub, wait = (lambda: ctx.submit_gof(streams, P)), ctx.wait_gof
        walk_ms(sub, wait, a.depth, a.depth)
        out[name] = {"gof_ms": one, "walk_ms": [walk_ms(sub, wait, a.walk_gofs, a.depth) for _ in range(a.walk_samples)]}
    ctx.close()
    return out


STEPS = {"kernel": step_kernel, "encodes": step_encodes, "time": step_time, "baseline": step_baseline}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--walk-samples", type=int, default=2)
    ap.add_argument("--walk-gofs", type=int, default=48)
    ap.add_argument("--depth", type=int, default=16)
    ap.add_argument("--baseline-tree", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    ap.add_argument("--floors", default="", help=argparse.SUPPRESS)
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

    med = statistics.median
    say("Transcode to a PSNR floor (rbt_transcode_gof_quality), one MI355X, tools/quality_target.py, one session; all samples kept; every step a process of its own.")
    k = run("kernel")
    if k is None:
        return finish()
    for name in ("no_map", "map_scale_4"):
        say("k_picture_sse, 64 pictures of 1280x1280, %s: device ms %s (median %.3f): %.0f GB/s of picture bytes" % (name, ["%.3f" % x for x in k[name]], med(k[name]), k["bytes"] / med(k[name]) / 1e6))
    e = run("encodes")
    if e is None:
        return finish()
    for name in ("all", "occupied"):
        v = e[name]
        for i, kind in enumerate(("geometry", "attribute")):
            r3, wk = v["r3"][i], v["walk"][i]
            say("%-8s samples%s %-9s: constant QP %d: %d B, Y %.3f dB (occupied %.3f); floor %d mdB -> probe %d, start %d, q* %d, met %d, %d encodes, |q* - qs| %d, %d B, Y %.3f dB (occupied %.3f)" %
                (name, ", occupancy_rd" if v["occupancy_rd"] else "", kind, r3["qp"], r3["bytes"], r3["psnr"][0], r3["psnr_occ"][0], v["floor_mdb"][i], wk["qp_probe"], wk["qp_start"], wk["qp"], wk["met"],
                 wk["n_encodes"], abs(wk["qp"] - wk["qp_start"]), wk["bytes"], wk["psnr"][0], wk["psnr_occ"][0]))
    t = run("time", ["--floors", json.dumps({n: e[n]["floor_mdb"] for n in e})])
    if t is None:
        return finish()
    b = run("baseline") if a.baseline_tree else None
    for name in ("all", "occupied"):
        say("%-8s one GOF with floors: %s ms (median %.1f); %d GOFs, %d in flight: %s ms (median %.1f)" %
            (name, ["%.1f" % x for x in t[name]["gof_ms"]], med(t[name]["gof_ms"]), a.walk_gofs, a.depth, ["%.1f" % x for x in t[name]["walk_ms"]], med(t[name]["walk_ms"])))
        if b:
            say("%-8s constant QP, build of the parent commit: one GOF %s ms (median %.1f); walk %s ms (median %.1f): ratios %.2f and %.2f" %
                (name, ["%.1f" % x for x in b[name]["gof_ms"]], med(b[name]["gof_ms"]), ["%.1f" % x for x in b[name]["walk_ms"]], med(b[name]["walk_ms"]),
                 med(t[name]["gof_ms"]) / med(b[name]["gof_ms"]), med(t[name]["walk_ms"]) / med(b[name]["walk_ms"])))
    if a.baseline_tree and b is None:
        return finish()
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
        spread = max(fps["parent"]) - min(fps["parent"]); gap = med(fps["parent"]) - med(fps["this tree"])
        say("bench.py --gpus 1 --steps 20 --warmup 5, point-cloud frames/s, interleaved: this tree %s (median %.1f) | build of the parent commit %s (median %.1f, spread %.1f): this tree's median is %.1f %s, %s" %
            (["%.1f" % x for x in fps["this tree"]], med(fps["this tree"]), ["%.1f" % x for x in fps["parent"]], med(fps["parent"]), spread, abs(gap), "below" if gap > 0 else "above",
             "within the parent's spread" if gap <= spread else "MORE THAN THE PARENT'S SPREAD BELOW"))
    finish()


if __name__ == "__main__":
    main()
