"""Child process of the arena-sharing tests (RBT_ARENA_SHARE is read once per process): a fixed list of transcodes in which the encoder's levels and reconstruction do or
do not live in the decoder's dead buffers (rbt_transcode.cpp setup_encode), each checked against the oracle where that is quick, and a digest of every output printed for
the parent to compare between RBT_ARENA_SHARE=0 and =1. argv[1]: "hostemu" or "gpu" (the GPU run adds the first GOF of the committed 1280x1280 fixture).
Prints one "DIGEST <case> <sha256 of the outputs>" line per case, "MEM <device bytes of the first case's job>", then "OK <cases>"."""
import hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import oracle_lib as O
import rbt_lib
from parity_cases import r5_gof

R = rbt_lib.module(); gs = rbt_lib.module_file("gof_shard")
gpu = sys.argv[1] == "gpu"
ctx = R.Context(device=0) if gpu else R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
P = R.StreamParams
n = 0


def digest(name, outs):
    global n
    h = hashlib.sha256()
    for o in outs:
        h.update(len(o).to_bytes(8, "little")); h.update(o)
    print("DIGEST", name, h.hexdigest(), flush=True)
    n += 1


def oracle(streams, params):
    return [O.transcode_substream(s, p.video_type, p.qp, occupancy_precision=p.occupancy_precision, log2_ctb=p.log2_ctb, rows_per_slice=p.ctb_rows_per_slice, md5_sei=p.md5_sei)
            for s, p in zip(streams, params)]


# 1. an ordinary GOF: every geometry / attribute picture of the output aliases its decoded input picture
(so, sg, sa), _ = r5_gof(192, 128, 2, 77)
ps = [P(0, 8, 4, 5, -1, 1, 0), P(1, 24, 4, 5, -1, 1, 0), P(19, 32, 4, 5, -1, 1, 0)]
job = ctx.submit_gof([so, sg, sa], ps); mem = ctx.job_memory(job); outs = ctx.wait_gof(job)
assert outs == oracle([so, sg, sa], ps)
digest("gof", outs)
# 2. a fan-out: more streams than pipelines, so the streams are grouped by video type and an input given twice (the same buffer) is decoded once; only the first target
#    rate of each input may take the decoded pictures' buffers, the second allocates its own
streams = [so, sg, sg, sa, sa]
ps5 = [P(0, 8, 4, 5, -1, 1, 0), P(1, 24, 4, 5, -1, 1, 0), P(1, 32, 4, 5, -1, 1, 0), P(19, 32, 4, 5, -1, 1, 0), P(19, 42, 4, 5, -1, 1, 0)]
outs = ctx.transcode_gof(streams, ps5)
assert outs == oracle(streams, ps5)
digest("fanout", outs)
# 3. conformance windows. An I,P input of 152 x 104 is coded 160 x 112 and so is the output: it aliases, and the encoder reads its source through the padding copy of the
#    decoded pictures. An all-intra input of 148 x 100 is coded 152 x 104, the output 160 x 112: another geometry, aliasing must not happen.
fr = np.random.default_rng(3).integers(0, 1024, (4, 152 * 104 * 3 // 2)).astype(np.uint16); fr[1] = fr[0]; fr[3] = fr[2]
s_pair, _ = O.encode(fr, 152, 104, 10, 16, gop=2, log2_ctb=6, rows_per_slice=0)
fr = np.random.default_rng(4).integers(0, 1024, (4, 148 * 100 * 3 // 2)).astype(np.uint16); fr[1] = fr[0]
s_intra, _ = O.encode(fr, 148, 100, 10, 16, gop=1, log2_ctb=5, rows_per_slice=0)
outs = [ctx.transcode_substream(s_pair, R.RBT_VIDEO_GEOMETRY, 24, rows_per_slice=-1), ctx.transcode_substream(s_intra, R.RBT_VIDEO_ATTRIBUTE, 32, rows_per_slice=1)]
assert outs == [O.transcode_substream(s_pair, 1, 24, rows_per_slice=-1), O.transcode_substream(s_intra, 19, 32, rows_per_slice=1)]
digest("window", outs)
# 4. the input's hashes checked behind the decoder's last filter (they read the decoded pictures while the encoder already writes into their dead buffers) and the
#    output's hashes made from the encoder's reconstruction
psv = [P(0, 8, 4, 5, -1, 1, 1), P(1, 24, 4, 5, -1, 1, 1), P(19, 32, 4, 5, -1, 1, 1)]
outs = ctx.transcode_gof([so, sg, sa], psv)
assert outs == oracle([so, sg, sa], psv)
for o in outs[1:]:
    dec, w, h, bd, chk, fail = ctx.decode(o)
    assert (w, h, chk, fail) == (192, 128, 4, 0)
digest("md5", outs)
# 5. sixteen jobs in flight: one HIP stream per job, the pipelines of a job behind each other in merged launches
a, b = r5_gof(128, 128, 1, 303)[0], r5_gof(128, 64, 2, 404)[0]
want_a, want_b = oracle(a, ps), oracle(b, ps)
ctx.set_depth(16)
jobs = [ctx.submit_gof(a if i % 2 == 0 else b, ps) for i in range(16)]
outs = [ctx.wait_gof(j) for j in jobs]
assert all(o == (want_a if i % 2 == 0 else want_b) for i, o in enumerate(outs))
digest("depth16", [x for o in outs for x in o])
ctx.set_depth(4)
# 6. the first GOF of the benchmark fixture (GPU only: 160 pictures of 1280 x 1280)
if gpu:
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    man = json.load(open(os.path.join(gold, "hm_r5_manifest.json")))["1280x1280_f32"]
    gof = [gs.split_pairs(open(os.path.join(gold, man["streams"][k]["file"]), "rb").read())[0] for k in ("occ", "geo", "attr")]
    job = ctx.submit_gof(gof, gs.rate_params(R, 3)); mem = ctx.job_memory(job); outs = ctx.wait_gof(job)
    assert all(len(o) > 0 for o in outs)
    digest("fixture", outs)
print("MEM", mem)
print("OK", n)
