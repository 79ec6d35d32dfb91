"""Flat chroma: a decoded picture with no coded chroma block, no chroma SAO, default weighting and flat references has both chroma planes at
v = 1 << (bit_depth - 1); its Cb / Cr are filled instead of reconstructed, its chroma loop filters are skipped, and the encoder does not code the chroma of a picture
whose source is flat. The cases are shared by the host build of the kernel bodies (test_flat_chroma.py) and the HIP build (test_gpu_flat_chroma.py): a case means the
same on both. Every case holds bytes or samples against the oracle - which has no fast path - and the number of pictures the decoder took as flat
(rbt_flat_pictures) against what H.265's text says about the stream.

Unless a case says otherwise: 128x128 pictures, two point-cloud frames (I, P, I, P), input from the oracle's encoder.

Not built: a P slice with explicit chroma weights over a flat reference. The oracle's encoder writes pred_weight_table only into its random-syntax streams
(oracle_enc_params.weighted_pred with a stress_seed), whose pictures carry random chroma residuals throughout: it cannot make that stream. What the rule does
with explicit weights is one host-side line (decode_build: wp_on sets chroma_unknown); the random-syntax streams with weights are decoded against the oracle by
tests/ctc_cases.py."""
import functools
import os
import subprocess
import sys
import numpy as np
import oracle_lib as O
import synth

W = H = 128
YS, CS = W * H, W * H // 4
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def maps(w=W, h=H, seed=21):
    """(geometry, attribute, occupancy) source frames of two point-cloud frames"""
    geo, attr, occ = synth.make_gof(w, h, 2, seed)
    for a in (geo, attr, occ): a.setflags(write=False)
    return geo, attr, occ


@functools.lru_cache(maxsize=None)
def geo_stream(log2_ctb=6, rows=0, w=W, h=H):
    return O.encode(maps(w, h)[0], w, h, 10, 16, gop=2, log2_ctb=log2_ctb, rows_per_slice=rows)


@functools.lru_cache(maxsize=None)
def attr_stream():
    return O.encode(maps()[1], W, H, 10, 22, gop=2, log2_ctb=6, rows_per_slice=0)


@functools.lru_cache(maxsize=None)
def occ_stream():
    return O.encode(maps()[2], W // 2, H // 2, 8, 8, gop=1, lossless=1, i_qp_offset=0, log2_ctb=6, rows_per_slice=0)


def decode_is(ctx, stream, rec, n_flat):
    """the decode alone: samples == the oracle's reconstruction, the hashes check, n_flat pictures were taken as flat"""
    dec, _, _, _, chk, fail = ctx.decode(stream)
    assert fail == 0 and chk == rec.shape[0] and np.array_equal(dec, rec)
    assert ctx.flat_pictures() == n_flat


def transcode_is(ctx, stream, vt, qp, n_flat, **kw):
    """transcode_substream == the oracle's, n_flat decoded pictures were taken as flat"""
    got = ctx.transcode_substream(stream, vt, qp, **kw)
    assert got == O.transcode_substream(stream, int(vt), qp, **kw)
    assert ctx.flat_pictures() == n_flat
    return got


# ---- 1. geometry GOF
def check_geometry(ctx, R, log2_ctb, rows):
    s, rec = geo_stream()
    assert (rec[:, YS:] == 512).all()                      # what the count rests on: the oracle's pictures are flat
    decode_is(ctx, s, rec, 4)
    transcode_is(ctx, s, R.RBT_VIDEO_GEOMETRY, 24, 4, log2_ctb=log2_ctb, rows_per_slice=rows)


def check_geometry_partial_ctbs(ctx, R):
    """200x120: partial CTBs at the right and bottom edge; the re-encode pads to 208x128 behind a conformance window"""
    s, rec = geo_stream(5, 0, 200, 120)
    decode_is(ctx, s, rec, 4)
    for rows in (-1, 0, 1):
        out = transcode_is(ctx, s, R.RBT_VIDEO_GEOMETRY, 24, 4, log2_ctb=5, rows_per_slice=rows)
    decode_is(ctx, out, O.decode(out)[0], 4)               # the window of a flat picture and its padding are flat: so is what was coded from them


# ---- 2. attribute GOF
def check_attribute(ctx, R):
    s, rec = attr_stream()
    decode_is(ctx, s, rec, 0)
    transcode_is(ctx, s, R.RBT_VIDEO_ATTRIBUTE, 32, 0, log2_ctb=5, rows_per_slice=-1)
    # the second map equal to the first: the P picture is all skip - no chroma block of its own, and a reference that is not flat
    a = maps()[1].copy(); a[1] = a[0]; a[3] = a[2]
    s2, rec2 = O.encode(a, W, H, 10, 22, gop=2, log2_ctb=6, rows_per_slice=0)
    assert np.array_equal(rec2[1], rec2[0])
    decode_is(ctx, s2, rec2, 0)
    transcode_is(ctx, s2, R.RBT_VIDEO_ATTRIBUTE, 32, 0, log2_ctb=5, rows_per_slice=-1)


# ---- 3. near-flat geometry (lossless input: a single v + 1 survives no quantiser)
NEAR = {"first": (0, YS), "last": (0, YS + CS - 1), "cr_only": (0, YS + CS + 37 * (W // 2) + 11)}


def check_near_flat(ctx, R, which):
    """one chroma sample of picture 0 at v + 1: in the first CTB, as the last sample of the last CTB (Cb), somewhere in Cr only. Picture 0 is not flat, nor is the P
    picture that references it; pictures 2 and 3 are."""
    g = maps()[0].copy(); pic, at = NEAR[which]; g[pic, at] = 513
    s, rec = O.encode(g, W, H, 10, 8, gop=2, lossless=1, i_qp_offset=0, log2_ctb=5, rows_per_slice=0)
    assert rec[0, at] == 513 and (rec[2:, YS:] == 512).all()
    decode_is(ctx, s, rec, 2)
    transcode_is(ctx, s, R.RBT_VIDEO_GEOMETRY, 24, 2, log2_ctb=5, rows_per_slice=-1)


# ---- 4. constant at another value: the first block carries a residual
def check_other_constant(ctx, R, cb, cr):
    g = maps()[0].copy(); g[:, YS:YS + CS] = cb; g[:, YS + CS:] = cr
    s, rec = O.encode(g, W, H, 10, 16, gop=2, log2_ctb=6, rows_per_slice=0)
    assert np.abs(rec[:, YS:YS + CS].astype(int) - cb).max() <= 3 and np.abs(rec[:, YS + CS:].astype(int) - cr).max() <= 3      # (a lossy stream: near the constant, away from 512)
    decode_is(ctx, s, rec, 0)
    transcode_is(ctx, s, R.RBT_VIDEO_GEOMETRY, 24, 0, log2_ctb=5, rows_per_slice=-1)


# ---- 5. 8 bit, lossless, chroma 128, as an occupancy transcode
def check_occupancy(ctx, R, w, h):
    r = np.random.default_rng(w * 7 + h)
    y = (r.integers(0, 2, (2, h // 8, w // 8)).repeat(8, 1).repeat(8, 2) | (r.integers(0, 16, (2, h, w)) == 0)).reshape(2, -1)
    fr = np.concatenate([y, np.full((2, w * h // 2), 128)], axis=1).astype(np.uint16)
    s, rec = O.encode(fr, w, h, 8, 8, gop=1, lossless=1, i_qp_offset=0, log2_ctb=5, rows_per_slice=0)
    assert np.array_equal(rec, fr)
    decode_is(ctx, s, rec, 2)
    for prec in (4, 2):                                    # pooled (flat by construction), passed through (flat because the decode is)
        transcode_is(ctx, s, R.RBT_VIDEO_OCCUPANCY, 8, 2, occupancy_precision=prec, log2_ctb=5, rows_per_slice=-1)


# ---- 6. one slice per CTB row, wavefront input
def check_row_slices(ctx, R, rows):
    s, rec = geo_stream(5, rows)
    assert len(O.slice_headers(s)) == 16                   # four pictures of four CTB rows
    decode_is(ctx, s, rec, 4)
    transcode_is(ctx, s, R.RBT_VIDEO_GEOMETRY, 24, 4, log2_ctb=5, rows_per_slice=-1)
    # chroma in the bottom row's slice only: the picture is not flat; the samples of its flat slices still equal the oracle's
    g = maps()[0].copy()
    for k in range(4):
        cb = g[k, YS:YS + CS].reshape(H // 2, W // 2); cb[H // 2 - 8:, 8:24] = 500
    s2, rec2 = O.encode(g, W, H, 10, 16, gop=2, log2_ctb=5, rows_per_slice=rows)
    top = rec2[:, YS:YS + CS].reshape(4, H // 2, W // 2)[:, :H // 2 - 16]
    assert (top == 512).all() and (rec2[:, YS:] != 512).any()
    decode_is(ctx, s2, rec2, 0)
    transcode_is(ctx, s2, R.RBT_VIDEO_GEOMETRY, 24, 0, log2_ctb=5, rows_per_slice=-1)


# ---- 8. occupancy_rd on, over a flat geometry stream
def check_occupancy_rd(ctx, R):
    P = R.StreamParams
    streams = [occ_stream()[0], geo_stream()[0], attr_stream()[0]]
    params = [P(0, 8, 4, 5, -1, 0, 0, 0), P(1, 24, 4, 5, -1, 0, 0, 1), P(19, 32, 4, 5, -1, 0, 0, 1)]
    got = ctx.transcode_gof(streams, params)
    assert got == O.transcode_data(streams, [(p.video_type, p.qp, p.occupancy_precision, p.log2_ctb, p.ctb_rows_per_slice, p.md5_sei, p.occupancy_rd) for p in params])
    assert ctx.flat_pictures() == 2 + 4 + 0                # occupancy, geometry, attribute


# ---- 10. jobs in flight, fan-out, walks
def r3(R):
    P = R.StreamParams
    return [P(0, 8, 4, 5, -1, 1, 0), P(1, 24, 4, 5, -1, 1, 0), P(19, 32, 4, 5, -1, 1, 0)]


def oracle_gof(streams, params):
    return [O.transcode_substream(s, p.video_type, p.qp, occupancy_precision=p.occupancy_precision, log2_ctb=p.log2_ctb, rows_per_slice=p.ctb_rows_per_slice, md5_sei=p.md5_sei) for s, p in zip(streams, params)]


def check_sixteen_jobs(ctx, R):
    """depth 16, sixteen jobs collected out of order: every job reports its own count"""
    a = [occ_stream()[0], geo_stream()[0], attr_stream()[0]]; b = [attr_stream()[0]]
    pa = r3(R); pb = pa[2:]
    want_a, want_b = oracle_gof(a, pa), oracle_gof(b, pb)
    ctx.set_depth(16)
    try:
        jobs = [ctx.submit_gof(a if i % 3 else b, pa if i % 3 else pb) for i in range(16)]
        for i in [5, 0, 15, 3, 9, 1, 12, 7, 2, 14, 4, 11, 6, 13, 8, 10]:
            assert ctx.wait_gof(jobs[i]) == (want_a if i % 3 else want_b)
            assert ctx.flat_pictures() == (6 if i % 3 else 0)
    finally:
        ctx.set_depth(4)


def check_fan_out(ctx, R):
    """several rates from one decode (more entries than pipelines: the entries of one video type share a pipeline, and an input given again is decoded once): the
    flags of the four decoded pictures serve every encoder. Two entries alone get a pipeline and a decode each."""
    P = R.StreamParams; s = geo_stream()[0]
    ps = [P(1, 24, 4, 5, -1, 0, 0), P(1, 32, 4, 6, -1, 0, 0), P(1, 28, 4, 5, -1, 0, 0), P(1, 30, 4, 4, -1, 0, 0), P(1, 34, 4, 5, -1, 0, 0)]
    assert ctx.transcode_gof([s] * 5, ps) == oracle_gof([s] * 5, ps)
    assert ctx.flat_pictures() == 4
    assert ctx.transcode_gof([s] * 2, ps[:2]) == oracle_gof([s] * 2, ps[:2])
    assert ctx.flat_pictures() == 8


def check_walks(ctx, R):
    """a rate walk and a quality walk over a flat geometry entry: trial encodes read the decoded pictures' flags again and again"""
    P = R.StreamParams; s = geo_stream()[0]; p = P(1, 24, 4, 5, -1, 0, 0)
    T = len(O.transcode_substream(s, 1, 30, log2_ctb=5, rows_per_slice=-1, md5_sei=0))
    outs, res = ctx.transcode_gof_rate([s], [p], [R.RateTarget(T, 16, 44)])
    assert res[0]["met"] and len(outs[0]) <= T and outs[0] == O.transcode_substream(s, 1, res[0]["qp"], log2_ctb=5, rows_per_slice=-1, md5_sei=0)
    assert ctx.flat_pictures() == 4
    _, rep = ctx.transcode_gof_quality([s], [P(1, 30, 4, 5, -1, 0, 0)], [R.QualityTarget()])          # the luma PSNR of QP 30 as the floor
    floor = int(rep[0]["psnr"][0] * 1000)
    outs, res = ctx.transcode_gof_quality([s], [p], [R.QualityTarget(floor, R.RBT_QUALITY_ALL, 16, 44)])
    assert outs[0] == O.transcode_substream(s, 1, res[0]["qp"], log2_ctb=5, rows_per_slice=-1, md5_sei=0)
    assert ctx.flat_pictures() == 4
    assert res[0]["sse"][1] == 0 and res[0]["sse"][2] == 0          # flat source, flat reconstruction


# ---- 9. and the arena switch: settings a process reads once (tests/flat_chroma_worker.py)
def run_worker(backend, case, env):
    r = subprocess.run([sys.executable, os.path.join(HERE, "flat_chroma_worker.py"), backend, case], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK " + case), (r.stdout[-1000:], r.stderr[-2000:])


def worker_banded(ctx, R):
    """RBT_PARSE_BANDS=2: the reconstruction of a band starts before the picture is parsed, so no picture is taken as flat; the samples are the same"""
    s, rec = geo_stream(5, 0, 128, 192)
    assert ctx.transcode_substream(s, R.RBT_VIDEO_GEOMETRY, 24) == O.transcode_substream(s, 1, 24)
    assert ctx.flat_pictures() == 0
    decode_is(ctx, s, rec, 4)                              # (rbt_decode parses in one go)


def worker_arena(ctx, R):
    """the same GOF with the encoder's buffers in the decoder's dead ones (RBT_ARENA_SHARE=1) and in memory of its own (=0)"""
    a = [occ_stream()[0], geo_stream()[0], attr_stream()[0]]
    assert ctx.transcode_gof(a, r3(R)) == oracle_gof(a, r3(R))
    assert ctx.flat_pictures() == 6
