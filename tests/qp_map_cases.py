"""A QP per CTB (include/rbt.h: rbt_qp_map, rbt_submit_gof_qp_map, rbt_transcode_gof_qp_map, rbt_qp_map_from_patches): one set of cases for the host emulation
(tests/test_qp_map.py) and the GPU (tests/test_gpu_qp_map.py). The oracle's encoder has no QP per CTB: the anchors are its constant-QP streams C(q) and its decoder.
  identity     no map: rbt_transcode_gof's bytes, which are the oracle's
  uniform      every M[f][r][c] == q, or == Q[f]: decoded pictures and hash SEIs of C(q) / C(Q[f]) frame by frame, parameter sets equal up to the PPS, slice QPs of rule 3
  decodes      arbitrary maps with md5_sei: the oracle's decoder and rbt_decode check every picture's MD5 - the stream decodes to the encoder's reconstruction (rules 4-6)
  placement    a 22 / 40 pattern: the CTBs at 22 are coded far better than in C(40), the CTBs at 40 far worse than in C(22)
  refusals     every RBT_ERR_PARAM of rule 10 submits nothing and leaves the context usable
  jobs         maps at depth 4 and 16, two GOFs in shared pipelines
  patches      rbt_qp_map_from_patches against a numpy restatement
The GOFs are frame_qp_cases' (64x64 with 3 frames, 128x128 with 4) and one atlas of 96x80, whose last CTB row is half a CTB at 32 and whose CTBs of 64 are partial on both
edges. Everything the oracle computes is cached in frame_qp_cases, so the host and the GPU tests of one run share it."""
import functools
import numpy as np
import pytest
import oracle_lib as O
import synth
import frame_qp_cases as FC
from frame_qp_cases import variant, source, occupancy, constant, constant_decoded, pictures, params, occ_params, QP

FC.GOFS.setdefault("96", (96, 80, 3, 9))        # w, h, point-cloud frames, seed: the cache of frame_qp_cases keys on the name


def grid(gof, v=variant()):
    """(point-cloud frames, CTB rows, CTB columns, CTB size) of the entry's output pictures"""
    w, h, n_pc, _ = FC.GOFS[gof]
    ctb = 1 << dict(v)["log2_ctb"]
    return n_pc, -(-h // ctb), -(-w // ctb), ctb


def _checker(f, r, c):
    # 22 / 40; differs from frame to frame and is not symmetric under transposition: off the diagonal exactly one of (r, c), (c, r) takes the + 1
    return np.where((r + c + f + (c > r)) % 2, 40, 22)


def _rowstart(f, r, c, wc):
    # the first CTB of every row differs from the last CTB of the row above: what wavefront's restart from SliceQpY and a slice's run-on predictor tell apart
    step = (24 * c) // max(1, wc - 1)
    return np.where(r % 2 == 0, 20 + step, 47 - step) - f


PATTERNS = {
    "checker": lambda f, r, c, wc, hc: _checker(f, r, c),
    "ramp": lambda f, r, c, wc, hc: 18 + (30 * c) // max(1, wc - 1) + 0 * r,                       # left to right, 18 .. 48
    "perframe": lambda f, r, c, wc, hc: [_checker(f, r, c), 18 + (30 * r) // max(1, hc - 1) + 0 * c, 27 + 0 * r][f % 3],
    "wrap": lambda f, r, c, wc, hc: np.where((r + c + f) % 2, 51, 0),                              # 0 next to 51: the delta wraps (rule 4)
    "low": lambda f, r, c, wc, hc: (r * wc + c + f) % 4,                                           # below 3: the I picture's T clamps at 0
    "spike_hi": lambda f, r, c, wc, hc: np.where((r == hc - 1) & (c == (f % wc)), 51, 22),
    "spike_lo": lambda f, r, c, wc, hc: np.where((r == (f % hc)) & (c == wc - 1), 22, 51),
    "rowstart": lambda f, r, c, wc, hc: _rowstart(f, r, c, wc),
}


def make_map(name, gof, v=variant()):
    n_pc, hc, wc, _ = grid(gof, v)
    r, c = np.mgrid[0:hc, 0:wc]
    m = np.stack([np.broadcast_to(PATTERNS[name](f, r, c, wc, hc), (hc, wc)) for f in range(n_pc)]).astype(np.int8)
    assert m.min() >= 0 and m.max() <= 51
    if name == "rowstart" and hc > 1:
        assert (m[:, 1:, 0] != m[:, :-1, -1]).all()
    return m


def patch_map(R, gof, v, patch_qp, background_qp):
    """per frame the map rbt_qp_map_from_patches derives from the patches of the frame's base atlas (synth.make_gof_maps: frame i is base i % 4, rolled by 2 * (i // 4))"""
    w, h, n_pc, seed = FC.GOFS[gof]
    out = []
    for f in range(n_pc):
        pats = synth.atlas_patches(R, w, h, seed + f % min(4, n_pc))
        out.append(R.qp_map_from_patches(atlas(R, w, h), pats, [patch_qp] * len(pats), background_qp, dict(v)["log2_ctb"], lib=_lib(R)))
    return np.stack(out)


_LIB = []


def _lib(R):
    """rbt_qp_map_from_patches is host code: the host emulation's library serves it here and on the GPU machine alike"""
    if not _LIB:
        import rbt_lib
        _LIB.append(R.load(rbt_lib.HOSTEMU_LIB))
    return _LIB[0]


def atlas(R, w, h):
    return R.AtlasParams(w, h, 16, 4, 2, 1, 1, 0)


def run(R, ctx, gof, kind, M, v=variant()):
    """the entry with the map M through rbt_transcode_gof_qp_map; with occupancy_rd behind its pooled occupancy entry"""
    if dict(v)["occupancy_rd"]:
        return ctx.transcode_gof_qp_map([occupancy(gof), source(gof, kind)], [occ_params(R), params(R, kind, v)], [None, M])[1]
    return ctx.transcode_gof_qp_map([source(gof, kind)], [params(R, kind, v)], [M])[0]


def targets(M):
    """T per picture: [2 * frames, rows, columns]"""
    M = np.asarray(M, np.int32)
    return np.stack([np.maximum(0, M - 3), M], axis=1).reshape(-1, M.shape[1], M.shape[2])


def check_slice_qps(out, M, v):
    """rule 3: SliceQpY of every independent slice segment is T of its first CTB"""
    T = targets(M); wc = T.shape[2]
    hs = O.slice_headers(out)
    pic = -1
    for hd in hs:
        if hd["address"] == 0:
            pic += 1
        if not hd["dependent"]:
            assert hd["qp"] == T[pic].ravel()[hd["address"]], (pic, hd["address"], hd["qp"])
    assert pic + 1 == T.shape[0]
    rows = dict(v)["rows_per_slice"]
    per = 1 if rows == 0 else -(-T.shape[1] // abs(rows))
    assert len(hs) == per * T.shape[0]
    del wc


# ------------------------------------------------------------------------------------------------ 1. identity
def check_identity(R, ctx, gof, kind, other=None):
    """rule 7: an entry without a map, and a call without maps, is rbt_transcode_gof's stream, which is the oracle's"""
    src, p = source(gof, kind), params(R, kind)
    want = ctx.transcode_gof([src], [p])[0]
    assert want == constant(gof, kind, QP)
    assert ctx.transcode_gof_qp_map([src], [p], [None])[0] == want
    assert ctx.transcode_gof_qp_map([src], [p], None)[0] == want
    if other is not None:
        assert other.transcode_gof_qp_map([src], [p], [None])[0] == want


# ------------------------------------------------------------------------------------------------ 2. uniform maps
def check_uniform_stream(out, gof, kind, Q, v):
    """frame f of `out` against C(Q[f]): decoded pictures equal, hash SEI NAL units equal; VPS and SPS those of C(params.qp), the PPS its own; the slice QPs of rule 3"""
    n_pc, hc, wc, _ = grid(gof, v); md5 = dict(v)["md5_sei"]
    got, got_pics = O.decode(out), pictures(out)
    assert got[0].shape[0] == 2 * n_pc == len(got_pics)
    if md5:
        assert (got[4], got[5]) == (2 * n_pc, 0)
    base = pictures(constant(gof, kind, QP, v))
    for f, q in enumerate(Q):
        ref, ref_pics = constant_decoded(gof, kind, q, v), pictures(constant(gof, kind, q, v))
        for k in (2 * f, 2 * f + 1):
            assert np.array_equal(got[0][k], ref[k]), (Q, f, k)
            assert got_pics[k]["sei"] == ref_pics[k]["sei"] and len(got_pics[k]["sei"]) == (1 if md5 else 0), (Q, k)
            assert len(got_pics[k]["sets"]) == len(base[k]["sets"]) == (3 if k % 2 == 0 else 0)
            if k % 2 == 0:
                assert got_pics[k]["sets"][:2] == base[k]["sets"][:2]            # VPS, SPS
                assert got_pics[k]["sets"][2] != base[k]["sets"][2]              # the PPS says cu_qp_delta_enabled_flag
                assert got_pics[k]["sets"][2] == got_pics[0]["sets"][2]
            assert len(got_pics[k]["slices"]) == len(ref_pics[k]["slices"])
    check_slice_qps(out, np.broadcast_to(np.asarray(Q, np.int8)[:, None, None], (n_pc, hc, wc)), v)


UNIFORM_QS = (QP, 20, 45, 2)
UNIFORM_CASES = [("128", "geo", variant(md5_sei=1)), ("64", "attr", variant(md5_sei=1, rows_per_slice=1)), ("128", "attr", variant()), ("64", "geo", variant(md5_sei=1, rows_per_slice=0, log2_ctb=4)),
                 ("96", "geo", variant(md5_sei=1, log2_ctb=6))]


def check_uniform(R, ctx, k, other=None):
    """rule 8: uniform maps at q = params.qp, 20, 45, 2, and maps constant per frame with the lists of frame_qp_cases"""
    gof, kind, v = UNIFORM_CASES[k]
    n_pc, hc, wc, _ = grid(gof, v)
    lists = [(q,) * n_pc for q in UNIFORM_QS] + [tuple(Q) for Q in FC.LISTS.get(gof, [(20, 33, 45)])]
    for Q in lists:
        M = np.broadcast_to(np.asarray(Q, np.int8)[:, None, None], (n_pc, hc, wc))
        out = run(R, ctx, gof, kind, M, v)
        check_uniform_stream(out, gof, kind, Q, v)
        if other is not None:
            assert run(R, other, gof, kind, M, v) == out, Q


# ------------------------------------------------------------------------------------------------ 3. arbitrary maps decode to the encoder's reconstruction
DECODE_CASES = [
    ("128", "geo", variant(md5_sei=1), "checker"),                                       # wavefront, CTBs of 32
    ("128", "attr", variant(md5_sei=1, rows_per_slice=1), "ramp"),
    ("64", "geo", variant(md5_sei=1, rows_per_slice=2, log2_ctb=4), "perframe"),
    ("128", "attr", variant(md5_sei=1, rows_per_slice=0), "wrap"),
    ("64", "attr", variant(md5_sei=1, log2_ctb=4), "low"),
    ("128", "geo", variant(md5_sei=1, log2_ctb=6, rows_per_slice=0), "spike_hi"),
    ("128", "attr", variant(md5_sei=1, log2_ctb=6), "spike_lo"),
    ("128", "geo", variant(md5_sei=1, rows_per_slice=1, log2_ctb=4), "rowstart"),
    ("128", "attr", variant(md5_sei=1), "rowstart"),                                     # wavefront: the predictor restarts from SliceQpY at every row
    ("128", "attr", variant(md5_sei=1, rows_per_slice=2), "rowstart"),                   # two rows a slice: it runs on from the row above
    ("128", "geo", variant(md5_sei=1, preset=1, rows_per_slice=2), "checker"),
    ("128", "attr", variant(md5_sei=1, preset=1), "wrap"),
    ("128", "geo", variant(md5_sei=1, occupancy_rd=1), "patches"),                       # patches at 24 in a background of 51: CTBs without any cbf (rule 6)
    ("128", "attr", variant(md5_sei=1, occupancy_rd=1, rows_per_slice=0), "patches"),
    ("128", "geo", variant(md5_sei=1, occupancy_rd=1, rows_per_slice=1, log2_ctb=4), "checker"),
    ("64", "geo", variant(md5_sei=1, rows_per_slice=1), "wrap"),
    ("96", "geo", variant(md5_sei=1), "ramp"),                                           # 3 x 3 CTBs, the bottom row half a CTB
    ("96", "attr", variant(md5_sei=1, log2_ctb=6, rows_per_slice=1), "checker"),         # 2 x 2 CTBs of 64, partial on both edges
    ("96", "geo", variant(md5_sei=1, log2_ctb=4, rows_per_slice=0), "wrap"),
    ("96", "attr", variant(md5_sei=1, log2_ctb=6), "spike_lo"),
]


def case_map(R, k):
    gof, kind, v, name = DECODE_CASES[k]
    return patch_map(R, gof, v, 24, 51) if name == "patches" else make_map(name, gof, v)


def copied_ctbs(dec, gof, v):
    """CTBs of the P pictures whose luma is the I picture's sample for sample: nothing was coded there (skipped CUs copy the reference at zero motion)"""
    w, h, n_pc, _ = FC.GOFS[gof]
    _, hc, wc, ctb = grid(gof, v)
    n = 0
    for f in range(n_pc):
        a, b = dec[2 * f][:w * h].reshape(h, w), dec[2 * f + 1][:w * h].reshape(h, w)
        for r in range(hc):
            for c in range(wc):
                n += np.array_equal(a[r * ctb:(r + 1) * ctb, c * ctb:(c + 1) * ctb], b[r * ctb:(r + 1) * ctb, c * ctb:(c + 1) * ctb])
    return n


def check_decodes(R, ctx, k, other=None, same_as=None):
    """rules 4-6 against two independent decoders: with md5_sei the stream carries the MD5 of the encoder's reconstruction of every picture. same_as: another context (the
    host emulation beside the GPU) that must produce the same bytes"""
    gof, kind, v, name = DECODE_CASES[k]
    n_pc = FC.GOFS[gof][2]
    M = case_map(R, k)
    out = run(R, ctx, gof, kind, M, v)
    got = O.decode(out)
    assert got[0].shape[0] == 2 * n_pc and (got[4], got[5]) == (2 * n_pc, 0), (k, got[4], got[5])
    dec, w, h, bd, checked, failed = ctx.decode(out, verify_md5=True)
    assert (checked, failed) == (2 * n_pc, 0) and np.array_equal(dec, got[0])
    check_slice_qps(out, M, v)
    if name == "patches":
        assert (M == 51).any() and (M == 24).any()
        assert copied_ctbs(got[0], gof, v) >= 1          # rule 6's second case is met: a CTB without any cbf
    if other is not None:
        assert run(R, other, gof, kind, M, v) == out
    if same_as is not None:
        assert run(R, same_as, gof, kind, M, v) == out, k


# ------------------------------------------------------------------------------------------------ 4. the map is applied where it says
def luma_sse_per_ctb(a, b, gof, v):
    """uint64 [pictures, rows, columns]: squared luma error per CTB"""
    w, h, _, _ = FC.GOFS[gof]
    _, hc, wc, ctb = grid(gof, v)
    d = (a[:, :w * h].astype(np.int64) - b[:, :w * h].astype(np.int64)).reshape(-1, h, w) ** 2
    out = np.zeros((d.shape[0], hc, wc), np.int64)
    for r in range(hc):
        for c in range(wc):
            out[:, r, c] = d[:, r * ctb:(r + 1) * ctb, c * ctb:(c + 1) * ctb].sum(axis=(1, 2))
    return out


@functools.lru_cache(maxsize=None)
def placement_reference(gof, kind):
    """per CTB the squared luma error of C(22) and of C(40) against the decoded input"""
    v = variant()
    src = O.decode(source(gof, kind))[0]
    return src, luma_sse_per_ctb(src, constant_decoded(gof, kind, 22, v), gof, v), luma_sse_per_ctb(src, constant_decoded(gof, kind, 40, v), gof, v)


PLACEMENT_CASES = [("128", "geo"), ("128", "attr")]


def check_placement_premise(gof, kind):
    """what the orderings rest on, from the oracle alone: on each set of CTBs C(22) and C(40) differ by more than 4x"""
    M = make_map("checker", gof); at22 = np.repeat(M == 22, 2, axis=0)
    _, e22, e40 = placement_reference(gof, kind)
    for sel in (at22, ~at22):
        assert e40[sel].sum() > 4 * e22[sel].sum() > 0, (e22[sel].sum(), e40[sel].sum())


def check_placement(R, ctx, gof, kind):
    v = variant()
    M = make_map("checker", gof, v); at22 = np.repeat(M == 22, 2, axis=0)      # per picture
    assert not np.array_equal(M[0], M[0].T) and not np.array_equal(M[0], M[1])
    src, e22, e40 = placement_reference(gof, kind)
    err = luma_sse_per_ctb(src, O.decode(run(R, ctx, gof, kind, M, v))[0], gof, v)
    assert err[at22].sum() < e40[at22].sum(), (err[at22].sum(), e40[at22].sum())
    assert err[~at22].sum() > e22[~at22].sum(), (err[~at22].sum(), e22[~at22].sum())


# ------------------------------------------------------------------------------------------------ 5. refusals
def check_arguments(R, ctx):
    """rule 10: every refusal is RBT_ERR_PARAM with its reason, submits nothing and leaves the context usable"""
    geo, occ = source("64", "geo"), occupancy("64")
    good = make_map("checker", "64")

    def refused(streams, ps, maps, word):
        with pytest.raises(R.RbtError) as e:
            ctx.transcode_gof_qp_map(streams, ps, maps)
        assert e.value.code == -4 and word in str(e.value), str(e.value)
    P = [params(R, "geo")]
    bad = R.QpMap(good); bad.struct_size += 8
    refused([geo], P, [bad], "struct_size")
    unset = R.QpMap(); unset.struct_size = 0
    refused([geo], P, [unset], "struct_size")
    refused([occ, geo], [occ_params(R), params(R, "geo")], [np.full((3, 1, 1), 8, np.int8), good], "occupancy")
    for n in (2, 4, 1, 6):                                                   # not pictures / 2
        refused([geo], P, [np.full((n, 2, 2), 30, np.int8)], "n_frames")
    odd = O.encode_hm(synth.make_gof_maps(64, 64, 3, 5)[0][:5], 64, 64, 10, 16)[0]      # a stream with an odd picture count
    refused([odd], P, [np.full((2, 2, 2), 30, np.int8)], "n_frames")
    for shape in ((3, 2, 3), (3, 3, 2), (3, 1, 1), (3, 4, 4)):               # not the CTB grid of a 64 x 64 picture at 32
        refused([geo], P, [np.full(shape, 30, np.int8)], "w_ctb")
    refused([geo], [params(R, "geo", variant(log2_ctb=4))], [good], "w_ctb")  # the grid follows the entry's log2_ctb
    for val in (52, -1, 127, -128):
        m = good.copy(); m[1, 1, 0] = val
        refused([geo], P, [m], "0..51")
    half = R.QpMap(good); half.n_frames = 0                                   # a map without its counts, counts without a map
    refused([geo], P, [half], "counts")
    half = R.QpMap(good); half.w_ctb = 0
    refused([geo], P, [half], "counts")
    none = R.QpMap(); none.n_frames = 3
    refused([geo], P, [none], "counts")
    none = R.QpMap(); none.w_ctb = none.h_ctb = 2
    refused([geo], P, [none], "counts")
    # the wrong count is found once the pictures are known, behind the other entries' decoders: the job is still refused whole
    refused([occ, geo, source("64", "attr")], [occ_params(R), params(R, "geo"), params(R, "attr")], [None, good, good[:2]], "entry 2")
    # a refused call took no job slot and left nothing behind: depth 1 still takes a job
    old = ctx.get_depth(); ctx.set_depth(1)
    try:
        out = ctx.wait_gof(ctx.submit_gof_qp_map([geo], P, [good]))[0]
    finally:
        ctx.set_depth(old)
    assert out == run(R, ctx, "64", "geo", good)
    # a corrupt input fails in the wait half as it does without a map, and the context goes on
    with pytest.raises(R.RbtError):
        ctx.transcode_gof_qp_map([geo[:len(geo) // 2]], P, [good])
    assert ctx.transcode_gof([geo], P)[0] == constant("64", "geo", QP)


# ------------------------------------------------------------------------------------------------ 6. jobs
def _job_map(gof, k):
    n_pc, hc, wc, _ = grid(gof)
    f, r, c = np.mgrid[0:n_pc, 0:hc, 0:wc]
    return (18 + (7 * k + 11 * f + 5 * r + 3 * c) % 29).astype(np.int8)      # 29 is prime: sixteen jobs, sixteen maps


def check_jobs_in_flight(R, ctx, depth, n_jobs):
    """n_jobs jobs in flight at the given depth, every one with a map of its own, collected out of order by rbt_wait_gof"""
    old = ctx.get_depth()
    ctx.set_depth(depth)
    try:
        gof, kind = ("64", "geo") if n_jobs > 4 else ("128", "attr")
        src, v = source(gof, kind), variant(md5_sei=1)
        jobs = [ctx.submit_gof_qp_map([src], [params(R, kind, v)], [_job_map(gof, k)]) for k in range(n_jobs)]
        with pytest.raises(R.RbtError) as e:
            ctx.submit_gof_qp_map([src], [params(R, kind, v)], [_job_map(gof, 0)])
        assert e.value.code == -7         # RBT_ERR_BUSY: the depth holds for these jobs too
        assert ctx.job_memory(jobs[0]) > 0
        with pytest.raises(R.RbtError) as e:      # the job is one of rbt_submit_gof's kind: the floors' wait calls refuse it and it stays collectable
            ctx.wait_gof_quality(jobs[0])
        assert e.value.code == -4
        outs = {}
        for k in list(range(1, n_jobs, 2)) + list(range(0, n_jobs, 2))[::-1]:
            outs[k] = ctx.wait_gof(jobs[k])[0]
            got = O.decode(outs[k])
            assert (got[4], got[5]) == (2 * FC.GOFS[gof][2], 0)
            check_slice_qps(outs[k], _job_map(gof, k), v)
        assert len(set(outs.values())) == n_jobs                      # every job its own map
        assert outs[1] == run(R, ctx, gof, kind, _job_map(gof, 1), v)   # ... and what the entry gives alone
    finally:
        ctx.set_depth(old)


def check_two_gofs(R, ctx, other=None):
    """two GOFs in one job: six entries share three pipelines; some carry maps, some nothing - and through the other call some carry lists. An entry alone gives what it
    gives in company"""
    v = variant(occupancy_rd=1, md5_sei=1)
    streams = [occupancy("64"), source("64", "geo"), source("64", "attr"), occupancy("128"), source("128", "geo"), source("128", "attr")]
    ps = [occ_params(R), params(R, "geo", v), params(R, "attr", v), occ_params(R), params(R, "geo", v), params(R, "attr", v)]
    maps = [None, make_map("checker", "64"), None, None, make_map("wrap", "128"), patch_map(R, "128", v, 24, 51)]
    outs = ctx.transcode_gof_qp_map(streams, ps, maps)
    want = ctx.transcode_gof(streams, ps)
    assert outs[0] == want[0] and outs[3] == want[3] and outs[2] == want[2] == constant("64", "attr", QP, v)
    for i, (gof, kind) in ((1, ("64", "geo")), (4, ("128", "geo")), (5, ("128", "attr"))):
        got = O.decode(outs[i])
        assert (got[4], got[5]) == (2 * FC.GOFS[gof][2], 0)
        assert outs[i] == run(R, ctx, gof, kind, maps[i], v), i
    lists = [None, [20, 33, 45], None, None, None, [20, 33, 45, 27]]
    louts = ctx.transcode_gof_frame_qp(streams, ps, lists)          # the other call, same pipelines: untouched by this one
    assert louts[2] == want[2] and louts[4] == want[4]
    FC.check_composed(louts[1], "64", "geo", lists[1], v); FC.check_composed(louts[5], "128", "attr", lists[5], v)
    if other is not None:
        assert other.transcode_gof_qp_map(streams, ps, maps) == outs


# ------------------------------------------------------------------------------------------------ 7. rbt_qp_map_from_patches
def np_from_patches(w, h, res, rects, qps, background, log2_ctb):
    """numpy restatement: rects in blocks of res"""
    ctb = 1 << log2_ctb
    hc, wc = -(-h // ctb), -(-w // ctb)
    best = np.full((h, w), 99, np.int32)
    for (u0, v0, su, sv), q in zip(rects, qps):
        sel = best[max(0, v0 * res):max(0, (v0 + sv) * res), max(0, u0 * res):max(0, (u0 + su) * res)]
        np.minimum(sel, q, out=sel)
    out = np.full((hc, wc), background, np.int8)
    for r in range(hc):
        for c in range(wc):
            m = best[r * ctb:(r + 1) * ctb, c * ctb:(c + 1) * ctb].min()
            if m < 99:
                out[r, c] = m
    return out


def check_from_patches(R):
    L = _lib(R)
    for (w, h, seed) in ((128, 128, 21), (64, 64, 5), (96, 80, 9), (320, 208, 3)):      # 96 x 80, 320 x 208: partial CTBs
        pats = synth.atlas_patches(R, w, h, seed)
        assert len(pats) >= 2
        qps = [(20 + 7 * i) % 52 for i in range(len(pats))]
        rects = [(p.u0, p.v0, p.size_u0, p.size_v0) for p in pats]
        for l2 in (4, 5, 6):
            got = R.qp_map_from_patches(atlas(R, w, h), pats, qps, 45, l2, lib=L)
            assert np.array_equal(got, np_from_patches(w, h, 16, rects, qps, 45, l2)), (w, h, l2)
    # a patch that ends on a CTB edge does not reach the next CTB; one sample more does; overlapping patches give the minimum; a patch beyond the atlas is clipped
    P = lambda u0, v0, su, sv: R.Patch(u0, v0, su, sv, 0, 0, 0, 0, 1, 2, 0, 0, 1, 1)
    a = atlas(R, 96, 80)
    got = R.qp_map_from_patches(a, [P(0, 0, 2, 2)], [10], 40, 5, lib=L)
    assert got.tolist() == [[10, 40, 40], [40, 40, 40], [40, 40, 40]]
    got = R.qp_map_from_patches(a, [P(0, 0, 3, 2), P(2, 1, 4, 4)], [10, 5], 40, 5, lib=L)
    assert got.tolist() == [[10, 5, 5], [40, 5, 5], [40, 5, 5]]
    got = R.qp_map_from_patches(a, [P(5, 4, 9, 9), P(7, 7, 1, 1)], [33, 1], 40, 6, lib=L)
    assert got.tolist() == [[40, 40], [40, 33]]
    assert R.qp_map_from_patches(a, [], [], 17, 4, lib=L).tolist() == [[17] * 6] * 5
    for bad in (lambda: R.qp_map_from_patches(a, [P(0, 0, 1, 1)], [52], 40, 5, lib=L), lambda: R.qp_map_from_patches(a, [P(0, 0, 1, 1)], [20], 60, 5, lib=L),
                lambda: R.qp_map_from_patches(a, [P(0, 0, 1, 1)], [20], 40, 3, lib=L), lambda: R.qp_map_from_patches(a, [P(0, 0, 1, 1)], [20], 40, 7, lib=L)):
        with pytest.raises(R.RbtError) as e:
            bad()
        assert e.value.code == -4
    out = np.zeros((3, 3), np.int8)
    import ctypes as C
    assert L.rbt_qp_map_from_patches(C.byref(a), None, 0, None, 40, 5, out.ctypes.data_as(C.POINTER(C.c_int8)), 3, 4) == -4      # not the atlas's grid
    assert L.rbt_qp_map_from_patches(C.byref(a), None, 0, None, 40, 5, out.ctypes.data_as(C.POINTER(C.c_int8)), 3, 3) == 0 and (out == 40).all()
