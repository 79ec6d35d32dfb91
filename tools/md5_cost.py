"""What the decoded-picture-hash options cost on the full-size GOF: md5_sei (hash SEI in the output) and verify_md5 (check of the input's hash SEIs),
for each kind of hash (MD5, CRC, checksum; the input's SEIs rewritten in that kind), as one blocking GOF and as a long walk (16 jobs of 3 GOFs in flight).
On the GPU box: python tools/md5_cost.py [--walk-gofs 96] [--reps 5]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rbt_lib
import picture_hash_cases as H

ap = argparse.ArgumentParser()
ap.add_argument("--walk-gofs", type=int, default=96)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
R = rbt_lib.module()
ctx = R.Context(device=0)
man = json.load(open(os.path.join(ROOT, "tests", "golden", "hm_r5_manifest.json")))["1280x1280_f32"]
s = {k: open(os.path.join(ROOT, "tests", "golden", v["file"]), "rb").read() for k, v in man["streams"].items()}
src = [s["occ"], s["geo"], s["attr"]]
names = {1: "MD5", 2: "CRC", 3: "checksum"}
inputs = {}                       # per kind: the GOF with its hash SEIs in that kind (streams without hash SEIs as they are)
for st in src:
    dec, w, h, bd, chk, _ = ctx.decode(st, verify_md5=False)
    for kind in (1, 2, 3):
        inputs.setdefault(kind, []).append(H.rewrite_hashes(st, ctx.picture_hash(dec, w, h, bd, kind), kind) if H.read_hash_seis(st) else st)
    del dec


def params(md5_sei, verify):
    P = R.StreamParams
    return [P(0, 8, 4, 5, -1, md5_sei, verify), P(1, 24, 4, 5, -1, md5_sei, verify), P(19, 32, 4, 5, -1, md5_sei, verify)]


def blocking(streams, md5_sei, verify):
    ctx.set_depth(1)
    ctx.transcode_gof(streams, params(md5_sei, verify))
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter(); ctx.transcode_gof(streams, params(md5_sei, verify)); ts.append(1000 * (time.perf_counter() - t0))
    return sorted(ts)[len(ts) // 2]


def walk(streams, md5_sei, verify, n_gofs, per_job=3, depth=16):
    ctx.set_depth(depth)
    jobs = [(streams * per_job, params(md5_sei, verify) * per_job) for _ in range(n_gofs // per_job)]
    t0 = time.perf_counter()
    q = []
    for st, p in jobs:
        if len(q) == depth:
            ctx.wait_gof(q.pop(0))
        q.append(ctx.submit_gof(st, p))
    while q:
        ctx.wait_gof(q.pop(0))
    return n_gofs * man["frames"] / (time.perf_counter() - t0)


print(f"blocking GOF, median of {a.reps}:")
base = blocking(src, 0, 0)
print(f"  no hash: {base:.1f} ms")
for kind in (1, 2, 3):
    e, v, b = blocking(inputs[kind], kind, 0), blocking(inputs[kind], 0, 1), blocking(inputs[kind], kind, 1)
    print(f"  {names[kind]:8s}: md5_sei {e:.1f} ms ({e - base:+.1f}), verify_md5 {v:.1f} ms ({v - base:+.1f}), both {b:.1f} ms ({b - base:+.1f})")
print(f"walk of {a.walk_gofs} GOFs, 16 jobs of 3 GOFs in flight (point-cloud frames/s, best of 2):")
walk(src, 0, 0, 48)                                            # warm-up: arenas of this shape
res = {}
for _ in range(2):
    for key, (st, m, v) in {"none": (src, 0, 0), "md5_sei=MD5": (inputs[1], 1, 0), "md5_sei=CRC": (inputs[2], 2, 0), "md5_sei=checksum": (inputs[3], 3, 0),
                            "md5_sei=MD5 + verify_md5": (inputs[1], 1, 1)}.items():
        res[key] = max(res.get(key, 0), walk(st, m, v, a.walk_gofs))
for key, fps in res.items():
    print(f"  {key:26s} {fps:7.1f} fps ({100 * (fps / res['none'] - 1):+.1f} %)")
