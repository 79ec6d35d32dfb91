"""Worst-case content for the encoder, the transcoder and the decoder: pictures that cost as many bits as a picture can (noise in all three planes), at slice QPs on
both sides of every band of the encoder's output sizing (rbt_transcode.cpp encode_build: slice QP below 16 / 16..33 / 34 and above / lossless) and at the ends of the QP
range, large enough (1280 x 256 x 2 pictures) that the fixed slack of the output buffers does not hide the bound. One table, shared by tests/test_worst_case_content.py
(host emulation) and tests/test_gpu_worst_case_content.py (MI355X). The oracle has no output caps; DESIGN.md 9.5 holds what it needs for these cases, in bytes per luma sample.

With the output sizing of round 4 (3 / 2 / 1 bytes per luma sample of a slice, the packed buffer half of their sum + 64 KB) 45 of the 61 cases of the table failed with
"out of memory": every lossless one, and every lossy one but these 16, which are kept for what else they are - uniform noise at qp 15, 18 (an I picture below the band edge
halves the pair's packed size need) and at qp 33, 34, 36, 37 (the sides of the upper band edge, I and P), two-level noise at qp 33 and 36, both at qp 51 (the coarsest
quantiser: the end of the QP range), heavy-tailed noise at qp 37, and the lossy checkerboards (cheap after the first CTB row, but every sample sits at a clipping limit)."""
from collections import namedtuple
import numpy as np
import oracle_lib as O
import rbt_lib
from parity_cases import r5_gof

RBT_ERR_OUTPUT = -8                      # RBT_ERR_OUTPUT (include/rbt.h): coded data larger than the output buffer sized for it

KINDS = ("uniform", "two_level", "checker", "heavy_tail")
Case = namedtuple("Case", "kind bd w h n qp lossless log2_ctb rows")
W, H, N = 1280, 256, 2                   # the smallest size at which the packed buffer's 64 KB of slack stop covering a noise picture


def frames(kind, bd, w, h, n, seed=0):
    """n planar 4:2:0 pictures [n, w*h*3/2] uint16, seeded by everything that names them"""
    mx = (1 << bd) - 1
    fs = w * h * 3 // 2
    r = np.random.default_rng([KINDS.index(kind), bd, w, h, n, seed])
    if kind == "uniform":
        return r.integers(0, mx + 1, (n, fs)).astype(np.uint16)
    if kind == "two_level":              # every sample 0 or the maximum
        return (r.integers(0, 2, (n, fs)) * mx).astype(np.uint16)
    if kind == "heavy_tail":             # Cauchy around mid-grey, scale 1/16 of the range, clipped: most samples near the middle, a few per cent at the limits
        return np.clip(np.rint((mx + 1) / 2 + r.standard_cauchy((n, fs)) * ((mx + 1) / 16)), 0, mx).astype(np.uint16)
    assert kind == "checker"             # per-sample checkerboard of 0 and the maximum; the phase of each plane of each picture is drawn
    out = np.zeros((n, fs), np.uint16)
    for k in range(n):
        o = 0
        for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            out[k, o:o + pw * ph] = (((xx + yy + int(r.integers(0, 2))) & 1) * mx).ravel()
            o += pw * ph
    return out


def slice_qps(c):
    """(QP of the I slices, QP of the P slices) as rbt_encode codes them: I pictures at qp - 3"""
    return (None, None) if c.lossless else (min(51, max(0, c.qp - 3)), min(51, max(0, c.qp)) if c.n > 1 else None)


# rbt_encode's qp for a lossy stream: I slices at qp - 3, P slices at qp. Band edges at slice QP 16 and 34:
#   qp  0: I  0, P  0      qp  3: I  0, P  3      qp 15: I 12, P 15     qp 16: I 13, P 16     qp 18: I 15, P 18     qp 19: I 16, P 19
#   qp 33: I 30, P 33      qp 34: I 31, P 34      qp 36: I 33, P 36     qp 37: I 34, P 37     qp 51: I 48, P 51
QPS = (0, 3, 15, 16, 18, 19, 33, 34, 36, 37, 51)


def _table():
    t = []
    for kind in ("uniform", "two_level"):                       # every QP, the product's default structure (CTB 32, wavefront rows)
        for qp in QPS:
            t.append(Case(kind, 10, W, H, N, qp, 0, 5, -1))
        t.append(Case(kind, 10, W, H, N, 0, 1, 5, -1))
    for kind, qps in (("checker", (0, 19, 51)), ("heavy_tail", (0, 19, 37))):      # the other contents: the most expensive QP of a band, and lossless
        for qp in qps:
            t.append(Case(kind, 10, W, H, N, qp, 0, 5, -1))
        t.append(Case(kind, 10, W, H, N, 0, 1, 5, -1))
    for kind in KINDS:                                          # 8-bit: the QP is relative to the bit depth, the costs are those of 10-bit
        for qp in (0, 19):
            t.append(Case(kind, 8, W, H, N, qp, 0, 5, -1))
    t.append(Case("two_level", 8, W, H, N, 37, 0, 5, -1))
    t.append(Case("two_level", 8, W, H, N, 0, 1, 5, -1))
    t.append(Case("uniform", 8, W, H, N, 0, 1, 5, -1))
    for log2_ctb, rows in ((4, -1), (6, -1), (5, 0), (5, 1), (4, 1), (6, 0), (4, 0), (6, 1)):     # slice structures: one slice per picture, one per CTB row, wavefront rows; CTB 16 / 32 / 64
        t.append(Case("two_level", 10, W, H, N, 19, 0, log2_ctb, rows))
        t.append(Case("two_level", 10, W, H, N, 0, 1, log2_ctb, rows))
    t.append(Case("uniform", 10, W, H, N, 0, 0, 4, 1))
    t.append(Case("uniform", 10, W, H, N, 37, 0, 6, 0))
    return t


CASES = _table()
# the benchmark's picture size (GPU test only): one I/P pair each, slice QPs 19/22 and 34/37
FULL_SIZE = [Case("uniform", 10, 1280, 1280, 2, 22, 0, 5, -1), Case("two_level", 10, 1280, 1280, 2, 37, 0, 5, -1)]


def case_id(c):
    return "%s-%dbit-%s-ctb%d-rows%d" % (c.kind, c.bd, "lossless" if c.lossless else "qp%d" % c.qp, 1 << c.log2_ctb, c.rows) + ("-%dx%d" % (c.w, c.h) if (c.w, c.h) != (W, H) else "")


def oracle_encode(c):
    """-> (pictures, the oracle's stream, the oracle's reconstruction)"""
    fr = frames(c.kind, c.bd, c.w, c.h, c.n)
    s, rec = O.encode(fr, c.w, c.h, c.bd, c.qp, gop=1 if c.lossless else 2, i_qp_offset=0 if c.lossless else -3, lossless=c.lossless, log2_ctb=c.log2_ctb, rows_per_slice=c.rows)
    return fr, s, rec


def check_decode(ctx, c, stream, rec):
    dec, w, h, bd, chk, fail = ctx.decode(stream)
    assert (w, h, bd, chk, fail) == (c.w, c.h, c.bd, c.n, 0), (w, h, bd, chk, fail)
    assert np.array_equal(dec, rec), "decoded pictures differ from the oracle's reconstruction"
    ref, *_r = O.decode(stream)
    assert _r[-1] == 0 and np.array_equal(dec, ref), "decoded pictures differ from the oracle's decoder"
    if c.lossless:
        assert np.array_equal(dec, frames(c.kind, c.bd, c.w, c.h, c.n))


def check_case(ctx, c):
    """encoder == oracle byte for byte; the decoder reads the stream back to the oracle's reconstruction with every picture hash right"""
    fr, want, rec = oracle_encode(c)
    got = ctx.encode(fr, c.w, c.h, c.bd, c.qp, gop=1 if c.lossless else 2, lossless=c.lossless, log2_ctb=c.log2_ctb, rows_per_slice=c.rows)
    assert got == want, "stream differs from the oracle's (%d / %d bytes)" % (len(got), len(want))
    check_decode(ctx, c, want, rec)


# ---------------------------------------------------------------------------------------------------- transcodes
def input_stream(kind, bd=10, w=W, h=H, n=N):
    """the oracle's stream of the content at QP 16, in the structure of the inputs (CTB 64, one slice per picture)"""
    s, _ = O.encode(frames(kind, bd, w, h, n), w, h, bd, 16, gop=2, log2_ctb=6, rows_per_slice=0)
    return s


TRANSCODES = [(kind, vt, qp) for kind in ("uniform", "two_level") for vt in (1, 19) for qp in (24, 32)] + [("checker", 1, 24), ("heavy_tail", 19, 24)]


def check_transcode(ctx, kind, video_type, qp):
    src = input_stream(kind)
    assert ctx.transcode_substream(src, video_type, qp, rows_per_slice=-1) == O.transcode_substream(src, video_type, qp, rows_per_slice=-1)


def check_transcode_gof(ctx):
    """three noise streams in one call"""
    R = rbt_lib.module()
    P = R.StreamParams
    srcs = [input_stream("uniform"), input_stream("two_level"), input_stream("checker")]
    outs = ctx.transcode_gof(srcs, [P(1, 24, 4, 5, -1, 1, 0), P(19, 32, 4, 5, -1, 1, 0), P(1, 32, 4, 5, -1, 1, 0)])
    for o, s, (vt, qp) in zip(outs, srcs, ((1, 24), (19, 32), (1, 32))):
        assert o == O.transcode_substream(s, vt, qp, rows_per_slice=-1), (vt, qp)


def check_noise_between_ordinary_gofs(ctx):
    """submit / wait at depth 4: a GOF of noise between two ordinary ones; the ordinary ones come out as they do alone"""
    R = rbt_lib.module()
    P = R.StreamParams
    a, b = r5_gof(192, 128, 2, 303)[0], r5_gof(128, 192, 2, 404)[0]
    ps = [P(0, 8, 4, 5, -1, 1, 0), P(1, 24, 4, 5, -1, 1, 0), P(19, 32, 4, 5, -1, 1, 0)]
    noise = [a[0], input_stream("two_level"), input_stream("uniform")]
    want = [[O.transcode_substream(s, p.video_type, p.qp, rows_per_slice=-1) for s, p in zip(g, ps)] for g in (a, noise, b)]
    ctx.set_depth(4)
    jobs = [ctx.submit_gof(g, ps) for g in (a, noise, b)]
    got = [ctx.wait_gof(j) for j in jobs]
    assert got[1] == want[1], "the noise GOF differs from the oracle"
    assert got[0] == want[0] and got[2] == want[2], "an ordinary GOF next to the noise GOF changed"
    assert ctx.transcode_gof(a, ps) == want[0]
