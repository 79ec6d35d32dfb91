"""How one intra transform block is coded (the prediction lives in the tile, one pass over a block where there were four, quarters read in place):
one set of cases for the host build of the kernel bodies (tests/test_intra_tb.py) and the HIP build (tests/test_gpu_intra_tb.py): a case means the same on both.
Nothing of this is a decision of the encoder, so every case holds the encoder's or the transcoder's bytes against the oracle's. The one exception is the QP map, which
the oracle's encoder does not have: there the oracle's decoder checks the MD5 of the encoder's reconstruction in every picture, and a uniform map must decode to the
pictures of the oracle's constant-QP stream (tests/qp_map_cases.py).

Sizes: 128x128 and 96x80 (whose last CTB row and column are partial at 32 and at 64), two point-cloud frames (I, P, I, P) of synth.make_gof.

The host build counts what the cases reach (csrc/rbt_encode.h, rbt_hostemu_intra_tb), so that a green run says the changed code ran. Over the whole set, in the order
of COUNTERS, the parent's decisions - which are the oracle's - gave:
    whole_after_four  2220      CUs coded as one block after being tried as four
    kept_as_four      2177      CUs kept as four
    runner_up_won     1114      coded mode trials that took the SATD's runner-up
    ts_4x4            1490      4x4 luma blocks of CUs kept as four that took transform skip
    trial_poisoned    3933      trials that left only the prediction in the tile (poisoned in the host build until the block is coded again)
"""
import functools
import numpy as np
import oracle_lib as O
import synth
import qp_map_cases as MC

COUNTERS = ("whole_after_four", "kept_as_four", "runner_up_won", "ts_4x4", "trial_poisoned")
SIZES = ((128, 128), (96, 80))


@functools.lru_cache(maxsize=None)
def maps(w, h, seed=21):
    """(geometry, attribute, occupancy) source frames of two point-cloud frames"""
    out = synth.make_gof(w, h, 2, seed)
    for a in out: a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_encode(kind, w, h, bd, qp, log2_ctb, rows, lossless=0):
    fr = source(kind, w, h, bd)
    if lossless:
        return O.encode(fr, w, h, bd, qp, gop=1, lossless=1, i_qp_offset=0, log2_ctb=log2_ctb, rows_per_slice=rows)
    return O.encode(fr, w, h, bd, qp, gop=2, log2_ctb=log2_ctb, rows_per_slice=rows)


@functools.lru_cache(maxsize=None)
def source(kind, w, h, bd=10):
    """source frames by name: the maps of synth.make_gof; 'steps' (a depth map of plateaus and lone samples, where transform skip wins, with chroma that is not flat); 'occ8' (an 8-bit
    block map with noisy chroma: lossless input whose chroma blocks carry residuals)"""
    r = np.random.default_rng(w * 7 + h + bd)
    if kind == "geo": return maps(w, h)[0]
    if kind == "attr": return maps(w, h)[1]
    if kind == "steps":
        # plateaus of 8x8 with steps between them and single samples that stand out: a 4x4 block with one such sample is cheaper without the transform
        y = (r.integers(0, 4, (h // 8, w // 8)) * 50 + 300).repeat(8, 0).repeat(8, 1) + (r.integers(0, 12, (h, w)) == 0) * 120
        c = r.integers(500, 524, (h, w // 2))                                                                 # Cb over Cr, 4:2:0
        fr = (np.concatenate([y.ravel(), c.ravel()]) >> (10 - bd)).astype(np.uint16)[None, :].repeat(2, 0)
    else:
        assert kind == "occ8" and bd == 8
        y = (r.integers(0, 2, (2, h // 8, w // 8)).repeat(8, 1).repeat(8, 2) | (r.integers(0, 16, (2, h, w)) == 0)).reshape(2, -1)
        fr = np.concatenate([y, r.integers(120, 136, (2, w * h // 2))], axis=1).astype(np.uint16)
    fr.setflags(write=False)
    return fr


def encode_is(ctx, kind, w, h, bd, qp, log2_ctb, rows, lossless=0):
    """the encoder's bytes are the oracle's, and the decoder reads them back to the oracle's reconstruction"""
    want, rec = oracle_encode(kind, w, h, bd, qp, log2_ctb, rows, lossless)
    fr = source(kind, w, h, bd)
    got = ctx.encode(fr, w, h, bd, qp, gop=1 if lossless else 2, lossless=lossless, log2_ctb=log2_ctb, rows_per_slice=rows)
    assert got == want, (kind, w, h, bd, qp, log2_ctb, rows)
    dec, _, _, _, chk, fail = ctx.decode(got)
    assert (chk, fail) == (fr.shape[0], 0) and np.array_equal(dec, rec)


# ---- 1. 10 bit at QP 24 / 32, every CTB size and slice structure
def check_ten_bit(ctx, log2_ctb, rows):
    for w, h in SIZES:
        encode_is(ctx, "geo", w, h, 10, 24, log2_ctb, rows)
        encode_is(ctx, "attr", w, h, 10, 32, log2_ctb, rows)


# ---- 2. 8 bit lossless occupancy
def check_lossless(ctx, log2_ctb):
    for w, h in SIZES:
        encode_is(ctx, "occ8", w, h, 8, 8, log2_ctb, 0, lossless=1)


# ---- 3. transform skip
def check_transform_skip(ctx, bd, log2_ctb, rows):
    for w, h in SIZES:
        encode_is(ctx, "steps", w, h, bd, 24 if bd == 10 else 27, log2_ctb, rows)


# ---- 4. occupancy-aware coding with partly occupied blocks, and 5. the transcode path with the input's modes as hints
@functools.lru_cache(maxsize=None)
def hm_gof(w, h):
    """[occupancy, geometry, attribute] with HM-like geometry and attribute input (NxN, 35 modes): the transcoder hands the input's intra modes to the analysis"""
    m = synth.make_gof_maps(w, h, 2, 9)
    so = O.encode(m[2], w // 2, h // 2, 8, 8, gop=1, i_qp_offset=0, lossless=1, log2_ctb=5, rows_per_slice=0)[0]
    return [so, O.encode_hm(m[0], w, h, 10, 16)[0], O.encode_hm(m[1], w, h, 10, 22)[0]]


def check_occupancy_aware(ctx, R, w, h, log2_ctb):
    P = R.StreamParams
    streams = hm_gof(w, h)
    params = [P(0, 8, 4, 5, -1, 0, 0, 0), P(1, 24, 4, log2_ctb, -1, 0, 0, 1), P(19, 32, 4, log2_ctb, -1, 0, 0, 1)]
    got = ctx.transcode_gof(streams, params)
    assert got == O.transcode_data(streams, [(p.video_type, p.qp, p.occupancy_precision, p.log2_ctb, p.ctb_rows_per_slice, p.md5_sei, p.occupancy_rd) for p in params])
    # the pooled occupancy picture has one sample per 4x4 luma unit: there are 8x8 luma blocks with occupied and unoccupied units - partly occupied transform blocks
    u = (O.decode(got[0])[0][:, : (w // 4) * (h // 4)] > 0).reshape(-1, h // 8, 2, w // 8, 2)
    assert (u.any(axis=(2, 4)) & ~u.all(axis=(2, 4))).any()


def check_transcode_hints(ctx, R, w, h, log2_ctb, rows):
    streams = hm_gof(w, h)
    for s, vt, qp in ((streams[1], R.RBT_VIDEO_GEOMETRY, 24), (streams[2], R.RBT_VIDEO_ATTRIBUTE, 32)):
        assert ctx.transcode_substream(s, vt, qp, log2_ctb=log2_ctb, rows_per_slice=rows, md5_sei=0) == O.transcode_substream(s, int(vt), qp, 4, log2_ctb, rows, 0)


# ---- 6. a QP per CTB: the QPMAP instantiations of the intra kernels
QP_MAP_DECODES = [k for k, c in enumerate(MC.DECODE_CASES) if (c[0], c[1], c[3]) in (("128", "attr", "ramp"), ("96", "attr", "checker"), ("96", "geo", "wrap"))]
QP_MAP_UNIFORM = [k for k, c in enumerate(MC.UNIFORM_CASES) if c[0] == "96"]


def check_qp_map_decodes(ctx, R, k):
    MC.check_decodes(R, ctx, k)


def check_qp_map_uniform(ctx, R, k):
    MC.check_uniform(R, ctx, k)
