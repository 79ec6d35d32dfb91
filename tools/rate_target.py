#!/usr/bin/env python3
"""Measures the rate-targeted transcode (rbt_transcode_gof_rate, include/rbt.h "transcoding to a byte budget") on the committed 1280x1280 32-frame CTC fixture
(tests/golden/hm_r5ctc_1280x1280_f32_*.annexb), on one GPU:

  1. the sizes of the constant-QP R3 geometry and attribute outputs; for budgets of 1x, 0.5x and 2x those sizes: the estimate, q*, the trial encodes and the rounds they
     came in (three QPs in the first round, two in every later one), per stream;
  2. the device time of the census (events around the kernel), per stream, from rbt_rate_estimate;
  3. the median of --samples wall times of the rate-targeted GOF (budgets = the R3 sizes) next to the same GOF through rbt_transcode_gof at the q* it found;
  4. the same for a walk of --walk-gofs GOFs (the fixture again and again) with --depth jobs in flight, one GOF per job.
--baseline-lib PATH: 3 and 4 at constant QP once more in a child process with that build of the library (a build of the parent commit), so that the constant-QP path of
both builds stands side by side. All samples are kept; a ratio is called "outside the spread" when the difference of the medians exceeds max - min of the constant-QP samples.

    python tools/rate_target.py --out profiles/rate_target.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")


def fixture():
    return [open(os.path.join(GOLD, "hm_r5ctc_1280x1280_f32_%s.annexb" % k), "rb").read() for k in ("occ", "geo", "attr")]


def timed(f, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter(); f(); out.append((time.perf_counter() - t0) * 1e3)
    return out


def walk_ms(ctx, R, streams, params, targets, n_gofs, depth):
    """n_gofs one-GOF jobs, `depth` in flight, collected in order"""
    t0 = time.perf_counter(); q = []
    for g in range(n_gofs):
        if len(q) == depth:
            (ctx.wait_gof_rate if targets else ctx.wait_gof)(q.pop(0))
        q.append(ctx.submit_gof_rate(streams, params, targets) if targets else ctx.submit_gof(streams, params))
    while q:
        (ctx.wait_gof_rate if targets else ctx.wait_gof)(q.pop(0))
    ms = (time.perf_counter() - t0) * 1e3
    print("  walk of %d GOFs%s: %.1f ms" % (n_gofs, " with budgets" if targets else "", ms), file=sys.stderr, flush=True)
    return ms


def constant_samples(ctx, R, gs, streams, qg, qa, samples, walk_gofs, depth):
    P = gs.rate_params(R, 3); P[1].qp, P[2].qp = qg, qa
    ctx.transcode_gof(streams, P)                       # warm-up: arenas cached
    one = timed(lambda: ctx.transcode_gof(streams, P), samples)
    ctx.set_depth(depth); walk_ms(ctx, R, streams, P, None, depth, depth)
    walk = [walk_ms(ctx, R, streams, P, None, walk_gofs, depth) for _ in range(samples)]
    ctx.set_depth(4)
    return {"gof_ms": one, "walk_ms": walk}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--walk-gofs", type=int, default=48)
    ap.add_argument("--depth", type=int, default=16)
    ap.add_argument("--baseline-lib", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--child-constant", default="", help=argparse.SUPPRESS)      # "qg,qa": print the constant-QP samples as JSON and leave
    a = ap.parse_args()
    import rbt_lib
    R = rbt_lib.module(); gs = rbt_lib.module_file("gof_shard")
    streams = fixture()
    if a.child_constant:
        # the baseline build predates the entry points this binding declares: give the binding a placeholder for what that library does not export (none of it is called here)
        import ctypes

        class OlderLibrary(ctypes.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if not name.startswith("rbt_"):
                        raise
                    return type("Missing", (), {})()
        R.C.CDLL = OlderLibrary
    ctx = R.Context(device=0)
    if a.child_constant:
        qg, qa = (int(x) for x in a.child_constant.split(","))
        print(json.dumps(constant_samples(ctx, R, gs, streams, qg, qa, a.samples, a.walk_gofs, a.depth)))
        return
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    P = gs.rate_params(R, 3)
    r3 = ctx.transcode_gof(streams, P)
    say("fixture 1280x1280, 64 pictures per stream; constant-QP R3 (QP %d / %d): geometry %d B, attribute %d B" % (P[1].qp, P[2].qp, len(r3[1]), len(r3[2])))
    found = {}
    for f in (1.0, 0.5, 2.0):
        tg = [R.RateTarget(), R.RateTarget(int(len(r3[1]) * f)), R.RateTarget(int(len(r3[2]) * f))]
        outs, res = ctx.transcode_gof_rate(streams, P, tg)
        for k, name in ((1, "geometry"), (2, "attribute")):
            r = res[k]; first = 3 - (r["qp_estimate"] == 0) - (r["qp_estimate"] == 51)
            rounds = 1 + (max(0, r["n_encodes"] - first) + 1) // 2
            say("budget %.1fx %-9s T %8d B: estimate QP %2d (E %8d B), q* %2d, %8d B, met %d, %2d encodes in %d rounds, |estimate - q*| %d" %
                (f, name, tg[k].target_bytes, r["qp_estimate"], r["estimate_bytes"], r["qp"], r["bytes"], r["met"], r["n_encodes"], rounds, abs(r["qp"] - r["qp_estimate"])))
        if f == 1.0:
            found = {"geo": res[1]["qp"], "attr": res[2]["qp"]}
    for k, name, vt in ((1, "geometry", 1), (2, "attribute", 19)):
        t = ctx.rate_estimate(streams[k], vt)
        ms = [ctx.rate_estimate(streams[k], vt)["census_ms"] for _ in range(a.samples)]
        h = t["hist"].sum(axis=(0, 1))
        say("census %-9s: device ms %s (median %.3f); %d levels; bins (all pictures and planes) %s" % (name, ["%.3f" % x for x in ms], statistics.median(ms), int(h.sum()), " ".join("%d:%d" % (b, int(v)) for b, v in enumerate(h) if v)))
        say("estimate %-9s: E(q) for q = 16..44 step 4: %s" % (name, " ".join("%d:%d" % (q, int(t["estimate"][q])) for q in range(16, 45, 4))))
    tg = [R.RateTarget(), R.RateTarget(len(r3[1])), R.RateTarget(len(r3[2]))]
    ctx.transcode_gof_rate(streams, P, tg)
    rate_one = timed(lambda: ctx.transcode_gof_rate(streams, P, tg), a.samples)
    ctx.set_depth(a.depth); walk_ms(ctx, R, streams, P, tg, a.depth, a.depth)
    rate_walk = [walk_ms(ctx, R, streams, P, tg, a.walk_gofs, a.depth) for _ in range(a.samples)]
    ctx.set_depth(4)
    const = constant_samples(ctx, R, gs, streams, found["geo"], found["attr"], a.samples, a.walk_gofs, a.depth)

    def compare(name, rate, base, what):
        mr, mb = statistics.median(rate), statistics.median(base); spread = max(base) - min(base)
        say("%s: rate-targeted %s ms (median %.1f) | %s %s ms (median %.1f, spread %.1f): ratio %.2f, %s the spread" %
            (name, ["%.1f" % x for x in rate], mr, what, ["%.1f" % x for x in base], mb, spread, mr / mb, "outside" if abs(mr - mb) > spread else "inside"))
    compare("one GOF", rate_one, const["gof_ms"], "constant QP %d / %d, this build" % (found["geo"], found["attr"]))
    compare("%d GOFs, %d in flight" % (a.walk_gofs, a.depth), rate_walk, const["walk_ms"], "constant QP, this build")
    ctx.close()
    if a.baseline_lib:
        env = dict(os.environ, RBT_LIB_PATH=os.path.abspath(a.baseline_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-constant", "%d,%d" % (found["geo"], found["attr"]), "--samples", str(a.samples), "--walk-gofs", str(a.walk_gofs),
                            "--depth", str(a.depth)], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode:
            say("baseline build failed to run: " + r.stderr[-400:])
        else:
            base = json.loads(r.stdout.strip().splitlines()[-1])
            compare("one GOF", rate_one, base["gof_ms"], "constant QP, baseline build")
            compare("%d GOFs, %d in flight" % (a.walk_gofs, a.depth), rate_walk, base["walk_ms"], "constant QP, baseline build")
            compare("constant QP one GOF, this build against the baseline build", const["gof_ms"], base["gof_ms"], "baseline build")
            compare("constant QP walk, this build against the baseline build", const["walk_ms"], base["walk_ms"], "baseline build")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
