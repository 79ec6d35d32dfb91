"""Child process of tests/arena_footprint_cases.py run, for tests/test_arena_footprint.py and tests/golden/make_arena_footprints.py (RBT_ARENA_SHARE is read once per process): a fixed list of calls on the host
emulation, each submitted as a job whose device bytes (Context.job_memory: every allocation between submit and the return of submit - the decoder's and the encoder's
arenas, pooled planes, occupancy maps, hash sets, merged launch lists) are printed as "MEM <case> <bytes>"; every output is held against the oracle. Ends with "OK <cases>"."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import oracle_lib as O
import rbt_lib
import synth
import v3c_synth as V

R = rbt_lib.module(); gs = rbt_lib.module_file("gof_shard")
ctx = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
P = R.StreamParams
n = 0


def oracle(streams, params):
    return [O.transcode_substream(s, p.video_type, p.qp, occupancy_precision=p.occupancy_precision, log2_ctb=p.log2_ctb, rows_per_slice=p.ctb_rows_per_slice, md5_sei=p.md5_sei)
            for s, p in zip(streams, params)]


def case(name, streams, params):
    global n
    job = ctx.submit_gof(streams, params); mem = ctx.job_memory(job); outs = ctx.wait_gof(job)
    assert outs == oracle(streams, params), name
    print("MEM", name, mem, flush=True)
    n += 1


# one GOF (occupancy, geometry, attribute) at rate point 3, two sizes
g128 = V.gof_streams(128, 128, 2, 501); g256 = V.gof_streams(256, 256, 2, 502)
case("gof128_r3", g128, gs.rate_params(R, 3))
case("gof256_r3", g256, gs.rate_params(R, 3))
# windowed inputs: an 80 x 88 occupancy video pooled to 40 x 44 (coded 40 x 48), and an I,P input of 152 x 104 coded 160 x 112 that the encoder reads through the padding copy
occ = synth.make_gof(160, 176, 2, 5)[2]
so = O.encode(occ, 80, 88, 8, 8, gop=1, lossless=1, i_qp_offset=0, log2_ctb=6, rows_per_slice=0)[0]
case("window_occ_40x44", [so], [P(R.RBT_VIDEO_OCCUPANCY, 8, 4, 5, 1, 1, 0)])
fr = np.random.default_rng(3).integers(0, 1024, (4, 152 * 104 * 3 // 2)).astype(np.uint16); fr[1] = fr[0]; fr[3] = fr[2]
sw = O.encode(fr, 152, 104, 10, 16, gop=2, log2_ctb=6, rows_per_slice=0)[0]
case("window_geo_152x104", [sw], [P(R.RBT_VIDEO_GEOMETRY, 24, 4, 5, -1, 1, 0)])
# a rate fan-out: one input to several QPs (more streams than pipelines: grouped by video type, the same buffer decoded once)
o, g, a = g128
case("fanout", [o, g, g, g, a, a], [P(0, 8, 4, 5, -1, 1, 0), P(1, 24, 4, 5, -1, 1, 0), P(1, 32, 4, 5, -1, 1, 0), P(1, 40, 4, 5, -1, 1, 0), P(19, 32, 4, 5, -1, 1, 0), P(19, 42, 4, 5, -1, 1, 0)])
# the encoder in wavefront mode (row progress words and row contexts in its arena) and with one slice per CTB row
case("rows_wave", [g], [P(R.RBT_VIDEO_GEOMETRY, 24, 4, 5, -1, 0, 0)])
case("rows_1", [g], [P(R.RBT_VIDEO_GEOMETRY, 24, 4, 5, 1, 0, 0)])
# the input's hashes checked and the output's hashes made: two hash sets
case("md5", g128, [P(0, 8, 4, 5, -1, 1, 1), P(1, 24, 4, 5, -1, 1, 1), P(19, 32, 4, 5, -1, 1, 1)])
# sixteen jobs announced: one HIP stream per job, so the job's pipelines go into merged parse and reconstruction launches with lists of their own
ctx.set_depth(16)
case("depth16_merged", g128, gs.rate_params(R, 3))
ctx.set_depth(4)
print("OK", n)
