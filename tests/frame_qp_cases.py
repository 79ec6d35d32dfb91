"""A QP per point-cloud frame (include/rbt.h: rbt_frame_qp, rbt_submit_gof_frame_qp, rbt_transcode_gof_frame_qp): one set of cases for the host emulation
(tests/test_frame_qp.py) and the GPU (tests/test_gpu_frame_qp.py).
  identity     every Q[f] equal to the entry's QP: byte for byte the constant-QP stream, which is the oracle's
  composition  C(q) = the oracle's constant-QP stream at q. Frame f of the output decodes (O.decode) to pictures 2f, 2f + 1 of C(Q[f]); its hash SEI NAL units are those of
               C(Q[f]); every slice NAL is within 2 bytes of its counterpart in C(Q[f]); the parameter sets are those of C(params.qp)
  refusals     every RBT_ERR_PARAM of rule 7 submits nothing and leaves the context usable
  jobs         lists at depth 4 and 16, two GOFs in shared pipelines, collected by rbt_wait_gof only
  floors       rbt_submit_gof_quality_frames / rbt_wait_gof_quality_frames / rbt_transcode_v3c_quality_frames (second half of the file): the oracle's constant-QP streams for
               q = 18..45 give a table of sums per frame; the definition's walk on each frame's table, with its rounds restated, gives q*_f, qs_f, met_f, n_encodes_f, the
               passes, the pictures encoded; the stream must be rbt_transcode_gof_frame_qp's at the picks
The streams hold 3 or 4 point-cloud frames from different base atlases (synth.make_gof_maps). Everything the oracle computes is cached in this module, so the host and the
GPU tests of one run share it."""
import functools
import numpy as np
import pytest
import oracle_lib as O
import synth

KINDS = {"geo": (1, 16, 0), "attr": (19, 22, 1)}           # video type, QP of the HM-like input, index into synth.make_gof_maps
BASE = dict(log2_ctb=5, rows_per_slice=-1, md5_sei=0, preset=0, occupancy_rd=0)
GOFS = {"64": (64, 64, 3, 5), "128": (128, 128, 4, 21), "d1": (128, 128, 3, 21)}     # w, h, point-cloud frames, seed ("d1": the atlas of the D1 cases only)
LIST_GOFS = ["128", "64"]
QP = 30                                                     # params[i].qp of every case: what the parameter sets carry
OCC_P = (0, 8, 4, 5, -1, 0, 0, 0)


def variant(**kw):
    return tuple(sorted({**BASE, **kw}.items()))


@functools.lru_cache(maxsize=None)
def source(gof, kind):
    w, h, n_pc, seed = GOFS[gof]
    return O.encode_hm(synth.make_gof_maps(w, h, n_pc, seed)[KINDS[kind][2]], w, h, 10, KINDS[kind][1])[0]


@functools.lru_cache(maxsize=None)
def occupancy(gof):
    w, h, n_pc, seed = GOFS[gof]
    return O.encode(synth.make_gof_maps(w, h, n_pc, seed)[2], w // 2, h // 2, 8, 8, gop=1, i_qp_offset=0, lossless=1, log2_ctb=5, rows_per_slice=0)[0]


@functools.lru_cache(maxsize=None)
def constant(gof, kind, q, v=variant()):
    """C(q): the oracle's stream of the entry at the constant QP q; with occupancy_rd, behind the pooled occupancy entry"""
    d = dict(v)
    if d["occupancy_rd"]:
        return O.transcode_data([occupancy(gof), source(gof, kind)], [OCC_P, (KINDS[kind][0], q, 4, d["log2_ctb"], d["rows_per_slice"], d["md5_sei"], 1, d["preset"])])[1]
    return O.transcode_substream(source(gof, kind), KINDS[kind][0], q, 4, d["log2_ctb"], d["rows_per_slice"], d["md5_sei"], d["preset"])


@functools.lru_cache(maxsize=None)
def constant_decoded(gof, kind, q, v=variant()):
    return O.decode(constant(gof, kind, q, v))[0]


def params(R, kind, v=variant(), qp=QP):
    d = dict(v)
    return R.StreamParams(KINDS[kind][0], qp, 4, d["log2_ctb"], d["rows_per_slice"], d["md5_sei"], 0, d["occupancy_rd"], d["preset"])


def occ_params(R):
    return R.StreamParams(0, 8, 4, 5, -1, 0, 0, 0, 0)


def split_annexb(data):
    """NAL units of an Annex-B stream: between start codes, trailing zero bytes dropped"""
    pos, out = [], []
    i = data.find(b"\x00\x00\x01")
    while i >= 0:
        pos.append(i); i = data.find(b"\x00\x00\x01", i + 3)
    for k, p in enumerate(pos):
        out.append(data[p + 3:pos[k + 1] if k + 1 < len(pos) else len(data)].rstrip(b"\x00"))
    return out


def pictures(data):
    """per picture {'sets': parameter set NALs in front of it, 'slices': its slice segment NALs, 'sei': the suffix SEI NALs behind it}"""
    out, sets = [], []
    for nal in split_annexb(data):
        t = (nal[0] >> 1) & 0x3F
        if t < 32:
            if nal[2] & 0x80:                      # first_slice_segment_in_pic_flag
                out.append({"sets": sets, "slices": [], "sei": []}); sets = []
            out[-1]["slices"].append(nal)
        elif t in (32, 33, 34):
            sets.append(nal)
        else:
            assert t == 40, t                      # suffix SEI: the picture hash
            out[-1]["sei"].append(nal)
    assert not sets
    return out


def run(R, ctx, gof, kind, Q, v=variant()):
    """the entry with the list Q through rbt_transcode_gof_frame_qp; with occupancy_rd behind its pooled occupancy entry"""
    if dict(v)["occupancy_rd"]:
        return ctx.transcode_gof_frame_qp([occupancy(gof), source(gof, kind)], [occ_params(R), params(R, kind, v)], [None, Q])[1]
    return ctx.transcode_gof_frame_qp([source(gof, kind)], [params(R, kind, v)], [Q])[0]


def check_composed(out, gof, kind, Q, v=variant()):
    """rule 5 of the definition, and rule 3: the parameter sets are those of C(params.qp)"""
    n_pc = GOFS[gof][2]; md5 = dict(v)["md5_sei"]
    assert len(Q) == n_pc
    got, got_pics = O.decode(out), pictures(out)
    assert got[0].shape[0] == 2 * n_pc == len(got_pics)
    if md5:
        assert (got[4], got[5]) == (2 * n_pc, 0)                    # the oracle's decoder checked every MD5 of the mixed stream
    base = pictures(constant(gof, kind, QP, v))
    for f, q in enumerate(Q):
        ref, ref_pics = constant_decoded(gof, kind, q, v), pictures(constant(gof, kind, q, v))
        for k in (2 * f, 2 * f + 1):
            assert np.array_equal(got[0][k], ref[k]), (Q, f, k)
            assert got_pics[k]["sets"] == base[k]["sets"] and len(got_pics[k]["sets"]) == (3 if k % 2 == 0 else 0), (Q, k)
            assert got_pics[k]["sei"] == ref_pics[k]["sei"] and len(got_pics[k]["sei"]) == (1 if md5 else 0), (Q, k)
            assert len(got_pics[k]["slices"]) == len(ref_pics[k]["slices"])
            for a, b in zip(got_pics[k]["slices"], ref_pics[k]["slices"]):
                assert abs(len(a) - len(b)) <= 2, (Q, k, len(a), len(b))
                assert a[:2] == b[:2]                                # the same NAL unit type
            if q == QP:
                assert got_pics[k]["slices"] == ref_pics[k]["slices"]   # a frame at the entry's own QP carries the constant-QP stream's bytes


def check_identity(R, ctx, gof, kind, other=None):
    """rule 4: all Q[f] == params.qp is rbt_transcode_gof's stream, and the oracle's"""
    n_pc = GOFS[gof][2]
    out = run(R, ctx, gof, kind, [QP] * n_pc)
    assert out == ctx.transcode_gof([source(gof, kind)], [params(R, kind)])[0] == constant(gof, kind, QP)
    assert ctx.transcode_gof_frame_qp([source(gof, kind)], [params(R, kind)], [None])[0] == out          # no list: the entry's own QP
    if other is not None:
        assert run(R, other, gof, kind, [QP] * n_pc) == out


LISTS = {"64": [(20, 33, 45), (44, 31, 19), (1, 30, 2), (30, 51, 0)], "128": [(20, 33, 45, 27), (45, 38, 30, 21), (2, 36, 0, 29)]}


def check_lists(R, ctx, gof, kind, other=None):
    """rule 5 on an ascending list, a descending list and lists with Q[f] < 3 (the I picture's QP clamps at 0)"""
    for Q in LISTS[gof]:
        out = run(R, ctx, gof, kind, list(Q))
        check_composed(out, gof, kind, Q)
        if other is not None:
            assert run(R, other, gof, kind, list(Q)) == out, Q


VARIANTS = [("64", "geo", variant(rows_per_slice=1)), ("128", "attr", variant(rows_per_slice=0)), ("128", "geo", variant(log2_ctb=4)), ("64", "attr", variant(log2_ctb=4, rows_per_slice=1)),
            ("128", "attr", variant(preset=1)), ("64", "geo", variant(md5_sei=1)), ("128", "attr", variant(md5_sei=1, rows_per_slice=2)), ("64", "geo", variant(md5_sei=1, rows_per_slice=0)),
            ("64", "geo", variant(occupancy_rd=1)), ("128", "attr", variant(occupancy_rd=1, md5_sei=1))]


def check_variant(R, ctx, k, other=None):
    """rule 5 with independent slices of one CTB row, one slice per picture, log2_ctb 4 (5 is the base), RBT_PRESET_FAST, hash SEIs, occupancy_rd behind a pooled occupancy entry"""
    gof, kind, v = VARIANTS[k]
    Q = LISTS[gof][0] if k % 2 == 0 else LISTS[gof][1]
    out = run(R, ctx, gof, kind, list(Q), v)
    check_composed(out, gof, kind, Q, v)
    if dict(v)["md5_sei"]:                 # rbt_decode with verify_md5 accepts the mixed stream and decodes what the oracle decodes
        dec, w, h, bd, checked, failed = ctx.decode(out, verify_md5=True)
        assert (checked, failed) == (2 * GOFS[gof][2], 0) and np.array_equal(dec, O.decode(out)[0])
    if other is not None:
        assert run(R, other, gof, kind, list(Q), v) == out


def check_verify_md5(R, ctx):
    """verify_md5 on an entry with a list: the input's hashes are checked as in the constant-QP path, a wrong one fails the job"""
    import picture_hash_cases as H
    src = source("64", "geo"); Q = list(LISTS["64"][0])
    frames, w, h, bd, _, _ = O.decode(src)
    p = params(R, "geo"); p.verify_md5 = 1
    out = ctx.transcode_gof_frame_qp([src], [p], [Q])[0]
    assert out == run(R, ctx, "64", "geo", Q)
    bad = H.rewritten(src, frames, w, h, bd, H.MD5, flip=1)
    with pytest.raises(R.RbtError) as e:
        ctx.transcode_gof_frame_qp([bad], [p], [Q])
    assert e.value.code == H.RBT_ERR_MD5
    assert ctx.transcode_gof_frame_qp([bad], [params(R, "geo")], [Q])[0] == out


def check_arguments(R, ctx):
    """rule 7: every refusal is RBT_ERR_PARAM with its reason, submits nothing and leaves the context usable"""
    geo, occ = source("64", "geo"), occupancy("64")

    def refused(streams, ps, lists, word):
        with pytest.raises(R.RbtError) as e:
            ctx.transcode_gof_frame_qp(streams, ps, lists)
        assert e.value.code == -4 and word in str(e.value), str(e.value)
    refused([occ, geo], [occ_params(R), params(R, "geo")], [[8, 8, 8], [30, 30, 30]], "occupancy")
    bad = R.FrameQp([30, 30, 30]); bad.struct_size += 8
    refused([geo], [params(R, "geo")], [bad], "struct_size")
    unset = R.FrameQp(); unset.struct_size = 0
    refused([geo], [params(R, "geo")], [unset], "struct_size")
    for Q in ([30, 30], [30, 30, 30, 30], [30], [30] * 6):
        refused([geo], [params(R, "geo")], [Q], "n_frames")
    half = R.FrameQp([30, 30, 30]); half.n_frames = 0          # a list without its count, a count without its list
    refused([geo], [params(R, "geo")], [half], "n_frames")
    none = R.FrameQp(); none.n_frames = 3
    refused([geo], [params(R, "geo")], [none], "n_frames")
    for Q in ([30, 52, 30], [-1, 30, 30], [30, 30, 127], [-128, 30, 30]):
        refused([geo], [params(R, "geo")], [Q], "0..51")
    # the wrong count is found once the pictures are known, behind the other entries' decoders: the job is still refused whole
    refused([occ, geo, source("64", "attr")], [occ_params(R), params(R, "geo"), params(R, "attr")], [None, [30, 31, 32], [30, 31]], "entry 2")
    # a refused call took no job slot and left nothing behind: depth 1 still takes a job
    old = ctx.get_depth(); ctx.set_depth(1)
    try:
        out = ctx.wait_gof(ctx.submit_gof_frame_qp([geo], [params(R, "geo")], [[QP, QP, QP]]))[0]
    finally:
        ctx.set_depth(old)
    assert out == constant("64", "geo", QP)
    # a corrupt input fails in the wait half as it does without a list, and the context goes on
    with pytest.raises(R.RbtError):
        ctx.transcode_gof_frame_qp([geo[:len(geo) // 2]], [params(R, "geo")], [[30, 30, 30]])
    assert ctx.transcode_gof([geo], [params(R, "geo")])[0] == constant("64", "geo", QP)


def _job_list(gof, k):
    n_pc = GOFS[gof][2]
    return [18 + (7 * k + 11 * f) % 28 for f in range(n_pc)]


def check_jobs_in_flight(R, ctx, depth, n_jobs):
    """n_jobs jobs in flight at the given depth, every one with a list of its own, collected out of order by rbt_wait_gof"""
    old = ctx.get_depth()
    ctx.set_depth(depth)
    try:
        gof, kind = ("64", "geo") if n_jobs > 4 else ("128", "attr")
        src = source(gof, kind)
        jobs = [ctx.submit_gof_frame_qp([src], [params(R, kind)], [_job_list(gof, k)]) for k in range(n_jobs)]
        with pytest.raises(R.RbtError) as e:
            ctx.submit_gof_frame_qp([src], [params(R, kind)], [_job_list(gof, 0)])
        assert e.value.code == -7         # RBT_ERR_BUSY: the depth holds for these jobs too
        assert ctx.job_memory(jobs[0]) > 0
        # the job is one of rbt_submit_gof's kind: the floors' wait calls refuse it and it stays collectable
        with pytest.raises(R.RbtError) as e:
            ctx.wait_gof_quality(jobs[0])
        assert e.value.code == -4
        for k in list(range(1, n_jobs, 2)) + list(range(0, n_jobs, 2))[::-1]:
            check_composed(ctx.wait_gof(jobs[k])[0], gof, kind, _job_list(gof, k))
    finally:
        ctx.set_depth(old)


def check_two_gofs(R, ctx, other=None):
    """two GOFs in one job: six entries share three pipelines, four of them carry lists (of 3 and of 4 frames), with occupancy_rd behind their pooled occupancy entries"""
    v = variant(occupancy_rd=1)
    streams = [occupancy("64"), source("64", "geo"), source("64", "attr"), occupancy("128"), source("128", "geo"), source("128", "attr")]
    ps = [occ_params(R), params(R, "geo", v), params(R, "attr", v), occ_params(R), params(R, "geo", v), params(R, "attr", v)]
    lists = [None, [20, 33, 45], None, None, [45, 38, 30, 21], [20, 33, 45, 27]]
    outs = ctx.transcode_gof_frame_qp(streams, ps, lists)
    want = ctx.transcode_gof(streams, ps)
    assert outs[0] == want[0] and outs[3] == want[3] and outs[2] == want[2] == constant("64", "attr", QP, v)
    check_composed(outs[1], "64", "geo", lists[1], v); check_composed(outs[4], "128", "geo", lists[4], v); check_composed(outs[5], "128", "attr", lists[5], v)
    assert outs[1] == run(R, ctx, "64", "geo", lists[1], v)       # ... and what each entry gives alone
    if other is not None:
        assert other.transcode_gof_frame_qp(streams, ps, lists) == outs


# ------------------------------------------------------------------------------------------------ floors held frame by frame (rbt_submit_gof_quality_frames)
Q_LO, Q_HI = 18, 45
ALL, OCCUPIED = 0, 1


@functools.lru_cache(maxsize=None)
def pooled_map(gof):
    """the luma planes of the output occupancy stream, one per point-cloud frame"""
    w, h, n_pc, _ = GOFS[gof]
    om, ow, oh, _, _, _ = O.decode(O.transcode_data([occupancy(gof)], [OCC_P])[0])
    assert (ow, oh, om.shape[0]) == (w // 4, h // 4, n_pc)
    return om[:, :ow * oh].reshape(n_pc, oh, ow)


@functools.lru_cache(maxsize=None)
def floor_table(gof, kind, rd=0):
    """q -> (the oracle's constant-QP stream at q, uint64 [frames, 3, 3]: per point-cloud frame the sums of its two pictures against the decoded input, with the pooled
    output map), for q = 18..45, tabulated once"""
    import quality_cases as QC
    w, h, n_pc, _ = GOFS[gof]
    a = O.decode(source(gof, kind))[0]
    m = np.repeat(pooled_map(gof), 2, 0)                   # picture k belongs to occupancy frame k * n_occ / cnt = k // 2
    out = {}
    for q in range(Q_LO, Q_HI + 1):
        s = constant(gof, kind, q, variant(occupancy_rd=rd))
        sums = QC.np_sse(a, O.decode(s)[0], w, h, m)
        out[q] = (s, sums.reshape(n_pc, 2, 3, 3).sum(axis=1))
    return out


def frame_figures(t, f, region, n_all):
    """plane 0 of the region for frame f: q -> (sse, samples)"""
    return {q: (int(v[1][f][0, 1]), int(v[1][f][0, 2])) if region == OCCUPIED else (int(v[1][f][0, 0]), n_all) for q, v in t.items()}


def pick_frame_floor(ds, near_db, qp_list, lo=Q_LO, hi=Q_HI):
    """the siblings' pick_floor over the tables of all frames: no figure of any frame within rounding of the floor"""
    import quality_cases as QC
    f = int(round(near_db * 1000))
    for _ in range(2000):
        try:
            for d in ds:
                QC.check_margins({q: d[q] for q in range(lo, hi + 1)}, f, qp_list, lo, hi)
            return f
        except AssertionError:
            f += 3
    raise AssertionError("no floor with the margins near %r" % near_db)


def frame_walk(d, qp, floor_mdb, lo, hi):
    """the definition's walk of one frame (quality_cases.walk) and the rounds it is encoded in: -> (q0, qs, q*, met, [QPs named per round])"""
    import quality_cases as QC
    q0, qs, qstar, met = QC.walk(d, qp, floor_mdb, lo, hi)
    return q0, qs, qstar, met, walk_rounds(q0, qs, lambda q: QC.meets(d[q][0], d[q][1], floor_mdb), lo, hi)


def walk_rounds(q0, qs, ok, lo, hi):
    """the QPs a frame's walk names round by round: the probe q0; then qs - 1, qs, qs + 1; then two at a time where the walk is going; never one out of range or tried"""
    tried, rounds = {q0}, [[q0]]

    def step():
        if qs not in tried:
            return qs, 0
        q = qs
        if ok(q):
            while q != hi:
                if q + 1 not in tried:
                    return q + 1, 1
                if not ok(q + 1):
                    break
                q += 1
            return None
        while q != lo and not ok(q):
            q -= 1
            if q not in tried:
                return q, -1
        return None
    while True:
        st = step()
        if st is None:
            break
        need, dr = st
        names = [q for q in ([need - 1, need, need + 1] if dr == 0 else [need, need + dr]) if lo <= q <= hi and q not in tried]
        tried |= set(names); rounds.append(names)
    return rounds


def carries_a_later_frame_without_an_earlier_one(walks):
    """some pass holds frame g and not a frame f < g: the frames behind the gap change their place in the pass, so every table picked by "picture k of the pass" instead of
    through the picture list would be wrong for them (a pass that only drops the last frames would not tell)"""
    r = [wk[4] for wk in walks]
    return any(len(r[g][k]) > (len(r[f][k]) if k < len(r[f]) else 0) for g in range(len(r)) for f in range(g) for k in range(len(r[g])))


def frame_sizes(stream):
    """bytes of every point-cloud frame of a stream of closed pairs, start codes included: a frame starts at its video parameter set"""
    at, i = [], stream.find(b"\x00\x00\x00\x01\x40\x01")
    while i >= 0:
        at.append(i); i = stream.find(b"\x00\x00\x00\x01\x40\x01", i + 6)
    assert at and at[0] == 0
    return [b - a for a, b in zip(at, at[1:] + [len(stream)])]


def check_frames_result(R, ctx, gof, kind, rd, region, floor_mdb, qp, lo, hi, out, res, want_distinct=False):
    """one entry's result against the Python walk on the oracle-derived per-frame tables"""
    import quality_cases as QC
    w, h, n_pc, _ = GOFS[gof]; t = floor_table(gof, kind, rd); v = variant(occupancy_rd=rd)
    if not floor_mdb:
        lo = hi = qp                                           # rule 7: no floor is the entry's own QP for every frame, the figures reported
    walks = [frame_walk(frame_figures(t, f, region, 2 * w * h), qp, floor_mdb, lo, hi) for f in range(n_pc)]
    Q = [wk[2] for wk in walks]
    assert res["n_frames"] == n_pc and res["qp_probe"] == walks[0][0] and res["d1"] is None
    for f, (wk, r) in enumerate(zip(walks, res["frames"])):
        d = frame_figures(t, f, region, 2 * w * h)
        assert (r["qp"], r["qp_start"], r["met"]) == (wk[2], wk[1], wk[3]), (floor_mdb, qp, lo, hi, f, r, wk)
        assert r["n_encodes"] == sum(len(x) for x in wk[4]) and 1 <= r["n_encodes"] <= abs(wk[2] - wk[1]) + 5, (f, r, wk)
        want = QC.psnr(*d[wk[2]])
        assert r["figure"] == want or abs(r["figure"] - want) < 1e-9
        if r["met"] and floor_mdb:
            assert QC.meets(d[wk[2]][0], d[wk[2]][1], floor_mdb) and (d[wk[2]][0] == 0 or d[wk[2]][1] == 0 or r["figure"] >= floor_mdb / 1000.0)
    n_rounds = max(len(wk[4]) for wk in walks)
    assert res["n_passes"] == sum(max(len(wk[4][k]) if k < len(wk[4]) else 0 for wk in walks) for k in range(n_rounds))
    assert res["pictures_encoded"] == 2 * sum(r["n_encodes"] for r in res["frames"])
    assert res["met_all"] == int(all(r["met"] for r in res["frames"]))
    # the stream is rbt_transcode_gof_frame_qp's at the picks, which composes from the oracle's constant-QP streams
    p = params(R, kind, v, qp)
    if rd:
        assert out == ctx.transcode_gof_frame_qp([occupancy(gof), source(gof, kind)], [occ_params(R), p], [None, Q])[1]
    else:
        assert out == ctx.transcode_gof_frame_qp([source(gof, kind)], [p], [Q])[0]
    if qp == QP:
        check_composed(out, gof, kind, Q, v)
    assert [r["bytes"] for r in res["frames"]] == frame_sizes(out) and res["bytes"] == len(out) == sum(frame_sizes(out))
    # the sums of the returned stream: the frames' sums at their picks
    assert all(lo <= q <= hi for q in Q)
    tot = sum(t[q][1][f] for f, q in enumerate(Q))
    assert res["sums"]["sse"] == [int(tot[c, 0]) for c in range(3)] and res["sums"]["samples"] == [2 * n_pc * w * h, n_pc * w * h // 2, n_pc * w * h // 2]
    assert (res["sums"]["qp"], res["sums"]["qp_probe"], res["sums"]["qp_start"]) == (-1, -1, -1)
    if want_distinct:
        assert len(set(Q)) >= 2, ("a degenerate input: every frame settles at one QP", Q)
    return Q


def frame_floor_cases(gof, kind, region=ALL, rd=0):
    """(floor, params.qp, lo, hi, at least two q*_f must differ): the midpoint between the worst and the best frame's figure at QP 32, started from 30, 20 and 44; a floor that lo misses for the
    worst frame only; floor 0; a narrow range"""
    import quality_cases as QC
    w, h, n_pc, _ = GOFS[gof]; t = floor_table(gof, kind, rd)
    ds = [frame_figures(t, f, region, 2 * w * h) for f in range(n_pc)]
    at = lambda q: sorted(QC.psnr(*d[q]) for d in ds)
    mid = pick_frame_floor(ds, (at(32)[0] + at(32)[-1]) / 2, [20, 30, 44])
    cases = [(mid, qp, Q_LO, Q_HI, True) for qp in (30, 20, 44)]
    top = at(Q_LO)
    cases.append((pick_frame_floor(ds, (top[0] + top[1]) / 2, [30]), 30, Q_LO, Q_HI, False))      # the worst frame misses even at lo, the others do not
    cases.append((0, 30, Q_LO, Q_HI, False))
    cases.append((pick_frame_floor(ds, (at(34)[0] + at(34)[-1]) / 2, [30], 32, 36), 30, 32, 36, False))
    return cases


def check_frame_floors(R, ctx, gof, kind, other=None):
    for floor, qp, lo, hi, distinct in frame_floor_cases(gof, kind):
        tg = [R.QualityTarget(floor, ALL, lo, hi)]
        outs, res = ctx.transcode_gof_quality_frames([source(gof, kind)], [params(R, kind, qp=qp)], tg)
        check_frames_result(R, ctx, gof, kind, 0, ALL, floor, qp, lo, hi, outs[0], res[0], distinct)
        if floor and not distinct and lo == Q_LO:
            assert [r["met"] for r in res[0]["frames"]].count(0) == 1 and res[0]["met_all"] == 0      # lo misses for one frame only, and the call returned RBT_OK
        if not floor:
            assert outs[0] == constant(gof, kind, qp) and all((r["qp"], r["qp_start"], r["met"], r["n_encodes"]) == (qp, qp, 1, 1) for r in res[0]["frames"]) and res[0]["n_passes"] == 1
        if other is not None:
            assert other.transcode_gof_quality_frames([source(gof, kind)], [params(R, kind, qp=qp)], tg) == (outs, res), (floor, qp)


def check_subset_passes(R, ctx, rd, region, other=None):
    """[occ, geo, attr] of the 3-frame GOF: the frames settle after different numbers of rounds, so the later passes carry frames 0 and 2 without frame 1 (or another
    strict subset) - every table indexed by "picture k of the stream" has to go through the pass's picture list: sources, hints, flat words, the maps of occupancy_rd, the
    occupancy frame of the sums"""
    gof = "64"; n_pc = GOFS[gof][2]
    streams = [occupancy(gof), source(gof, "geo"), source(gof, "attr")]
    v = variant(occupancy_rd=rd)
    ps = [occ_params(R), params(R, "geo", v), params(R, "attr", v)]
    floors = [frame_floor_cases(gof, k, region, rd)[0][0] for k in ("geo", "attr")]
    tg = [R.QualityTarget(), R.QualityTarget(floors[0], region, Q_LO, Q_HI), R.QualityTarget(floors[1], region, Q_LO, Q_HI)]
    for outs, res in (ctx.transcode_gof_quality_frames(streams, ps, tg), ctx.wait_gof_quality_frames(ctx.submit_gof_quality_frames(streams, ps, tg))):
        assert outs[0] == ctx.transcode_gof(streams[:1], ps[:1])[0] and (res[0]["n_frames"], res[0]["frames"], res[0]["qp_probe"], res[0]["bytes"]) == (0, [], 8, len(outs[0]))
        for k, kind in ((1, "geo"), (2, "attr")):
            check_frames_result(R, ctx, gof, kind, rd, region, floors[k - 1], QP, Q_LO, Q_HI, outs[k], res[k], True)
            w, h = GOFS[gof][:2]; tb = floor_table(gof, kind, rd)
            walks = [frame_walk(frame_figures(tb, f, region, 2 * w * h), QP, floors[k - 1], Q_LO, Q_HI) for f in range(n_pc)]      # (check_frames_result held the library to these rounds)
            assert carries_a_later_frame_without_an_earlier_one(walks), [wk[4] for wk in walks]
            n = [r["n_encodes"] for r in res[k]["frames"]]
            assert min(n) < max(n) and res[k]["pictures_encoded"] < 2 * n_pc * res[k]["n_passes"]      # some pass carried a strict subset of the frames
            t = floor_table(gof, kind, rd); Q = [r["qp"] for r in res[k]["frames"]]
            tot = sum(t[q][1][f] for f, q in enumerate(Q))
            assert res[k]["sums"]["sse_occ"] == [int(tot[c, 1]) for c in range(3)] and res[k]["sums"]["samples_occ"] == [int(tot[c, 2]) for c in range(3)]
    if other is not None:
        assert other.transcode_gof_quality_frames(streams, ps, tg) == (outs, res)


def check_floor_jobs_in_flight(R, ctx, depth, n_jobs):
    """n_jobs jobs in flight at the given depth, each with a floor of its own, collected out of order; the wrong pairing is refused and the job stays collectable"""
    old = ctx.get_depth()
    ctx.set_depth(depth)
    try:
        gof, kind = ("64", "geo") if n_jobs > 4 else ("128", "attr")
        src = source(gof, kind); base = frame_floor_cases(gof, kind)
        floors = [base[k % 3 + 3][0] if k % 2 else base[0][0] for k in range(n_jobs)]
        rng = [(base[k % 3 + 3][2], base[k % 3 + 3][3]) if k % 2 else (Q_LO, Q_HI) for k in range(n_jobs)]
        jobs = [ctx.submit_gof_quality_frames([src], [params(R, kind)], [R.QualityTarget(floors[k], ALL, *rng[k])]) for k in range(n_jobs)]
        if n_jobs == depth:
            with pytest.raises(R.RbtError) as e:
                ctx.submit_gof_quality_frames([src], [params(R, kind)], [R.QualityTarget(floors[0], ALL, Q_LO, Q_HI)])
            assert e.value.code == -7         # RBT_ERR_BUSY
        assert ctx.job_memory(jobs[0]) > 0
        for wrong in (ctx.wait_gof, ctx.wait_gof_quality, ctx.wait_gof_rate):
            with pytest.raises(R.RbtError) as e:
                wrong(jobs[0])
            assert e.value.code == -4
        plain = ctx.submit_gof_quality([src], [params(R, kind)], [R.QualityTarget()]) if depth > n_jobs else None
        for k in list(range(1, n_jobs, 2)) + list(range(0, n_jobs, 2))[::-1]:
            outs, res = ctx.wait_gof_quality_frames(jobs[k])
            check_frames_result(R, ctx, gof, kind, 0, ALL, floors[k], QP, rng[k][0], rng[k][1], outs[0], res[0])
        if plain is not None:
            with pytest.raises(R.RbtError) as e:
                ctx.wait_gof_quality_frames(plain)
            assert e.value.code == -4
            ctx.wait_gof_quality(plain)
    finally:
        ctx.set_depth(old)


def check_floor_two_gofs(R, ctx, other=None):
    """two GOFs in shared pipelines: the entries of one type share a pipeline, every one walks its frames on its own"""
    streams = [occupancy("64"), source("64", "geo"), source("64", "attr"), occupancy("128"), source("128", "geo"), source("128", "attr")]
    ps = [occ_params(R), params(R, "geo"), params(R, "attr"), occ_params(R), params(R, "geo"), params(R, "attr")]
    keys = [None, ("64", "geo"), ("64", "attr"), None, ("128", "geo"), ("128", "attr")]
    floors = [0 if k is None else frame_floor_cases(*k)[0][0] for k in keys]
    floors[2] = 0                                              # an entry without a floor among them
    tg = [R.QualityTarget(f, ALL, Q_LO, Q_HI) if f else R.QualityTarget() for f in floors]
    outs, res = ctx.transcode_gof_quality_frames(streams, ps, tg)
    for i, k in enumerate(keys):
        if k is not None:
            check_frames_result(R, ctx, k[0], k[1], 0, ALL, floors[i], QP, Q_LO if floors[i] else QP, Q_HI if floors[i] else QP, outs[i], res[i], bool(floors[i]))
    if other is not None:
        assert other.transcode_gof_quality_frames(streams, ps, tg) == (outs, res)


@functools.lru_cache(maxsize=None)
def odd_source():
    """a geometry stream of three pictures: a frame and a half"""
    w, h, n_pc, seed = GOFS["64"]
    return O.encode_hm(synth.make_gof_maps(w, h, n_pc, seed)[0][:3], w, h, 10, 16)[0]


def check_floor_arguments(R, ctx):
    """the PSNR floor's refusals hold for the per-frame call, and the whole-stream call keeps its own pairing"""
    geo, occ = source("64", "geo"), occupancy("64")

    def refused(streams, ps, ts, word):
        with pytest.raises(R.RbtError) as e:
            ctx.transcode_gof_quality_frames(streams, ps, ts)
        assert e.value.code == -4 and word in str(e.value), str(e.value)
    refused([occ], [occ_params(R)], [R.QualityTarget(40000)], "occupancy")
    bad = R.QualityTarget(40000); bad.struct_size += 4
    refused([geo], [params(R, "geo")], [bad], "struct_size")
    refused([geo], [params(R, "geo")], [R.QualityTarget(40000, ALL, 31, 30)], "range")
    refused([geo], [params(R, "geo")], [R.QualityTarget(-1)], "negative")
    refused([geo], [params(R, "geo")], [R.QualityTarget(40000, OCCUPIED, Q_LO, Q_HI)], "occupancy source")
    refused([odd_source()], [params(R, "geo")], [R.QualityTarget(40000, ALL, Q_LO, Q_HI)], "two pictures per point-cloud frame")
    refused([odd_source()], [params(R, "geo")], [R.QualityTarget()], "two pictures per point-cloud frame")
    with pytest.raises(R.RbtError) as e:                      # ... and so is a QP list on such a stream, whatever its length
        ctx.transcode_gof_frame_qp([odd_source()], [params(R, "geo")], [[30, 30]])
    assert e.value.code == -4 and "n_frames" in str(e.value)
    assert len(O.decode(ctx.transcode_gof([odd_source()], [params(R, "geo")])[0])[0]) == 3      # (the constant-QP path codes the lone picture)
    outs, res = ctx.transcode_gof_quality_frames([geo], [params(R, "geo")], [R.QualityTarget()])
    assert outs[0] == constant("64", "geo", QP)


def check_floor_container(R, ctx):
    """rbt_transcode_v3c_quality_frames on the siblings' two-GOF file equals the per-GOF calls; without floors it is rbt_transcode_v3c's bytes"""
    import rate_cases as RC
    import v3c_synth as V
    data, gofs = RC.v3c_file()
    gf, af = 38000, 36000
    out, per = ctx.transcode_v3c_quality_frames(data, 30, 34, gf, af)
    _, got = V.parse(out); _, src_units = V.parse(data)
    assert len(got) == len(src_units) == 10 and len(per) == 2
    P = [R.StreamParams(0, 8, 4, 5, -1, 0, 0, 0, 0), R.StreamParams(1, 30, 4, 5, -1, 0, 0, 0, 0), R.StreamParams(19, 34, 4, 5, -1, 0, 0, 0, 0)]
    for g, st in enumerate(gofs):
        want, res = ctx.transcode_gof_quality_frames(st, P, [R.QualityTarget(), R.QualityTarget(gf), R.QualityTarget(af)])
        for k, (t, i) in enumerate(((V.OVD, 2), (V.GVD, 3), (V.AVD, 4))):
            assert got[5 * g + i] == V.unit_header(t) + O.byte_to_sample_stream(want[k]), (g, k)
        assert got[5 * g] == src_units[5 * g] and got[5 * g + 1] == src_units[5 * g + 1]
        assert per[g][0] == res[1] and per[g][1] == res[2]
        assert per[g][0]["n_frames"] == 1 and (per[g][0]["frames"][0]["qp"] != 30 or per[g][1]["frames"][0]["qp"] != 34)      # the floors, not the constant QPs, decided
    assert ctx.transcode_v3c_quality_frames(data, 30, 34, gofs_per_job=2)[0] == ctx.transcode_v3c(data, 30, 34)
    assert ctx.transcode_v3c_quality_frames(data, 30, 34, gf, af, gofs_per_job=2) == (out, per)
    with pytest.raises(R.RbtError) as e:
        ctx.transcode_v3c_quality_frames(data, 30, 34, -1, 0)
    assert e.value.code == -4


FLOOR_VARIANTS = [("64", "geo", variant(md5_sei=1, rows_per_slice=1)), ("128", "attr", variant(md5_sei=1, log2_ctb=4)), ("64", "attr", variant(preset=1, rows_per_slice=0))]


def check_floor_variant(R, ctx, k, other=None):
    """the passes under other slice structures, CTB sizes, the fast preset and with hash SEIs behind every picture: whatever the frames pick, the assembled stream is the QP
    list's at the picks, composes from the oracle's constant-QP streams of the variant, and rbt_decode verifies its hashes"""
    gof, kind, v = FLOOR_VARIANTS[k]
    floor = frame_floor_cases(gof, kind)[0][0]
    tg = [R.QualityTarget(floor, ALL, Q_LO, Q_HI)]
    outs, res = ctx.transcode_gof_quality_frames([source(gof, kind)], [params(R, kind, v)], tg)
    Q = [r["qp"] for r in res[0]["frames"]]
    assert len(set(Q)) >= 2 and res[0]["pictures_encoded"] == 2 * sum(r["n_encodes"] for r in res[0]["frames"])
    assert outs[0] == run(R, ctx, gof, kind, Q, v) and [r["bytes"] for r in res[0]["frames"]] == frame_sizes(outs[0])
    check_composed(outs[0], gof, kind, Q, v)
    if dict(v)["md5_sei"]:
        dec, w, h, bd, checked, failed = ctx.decode(outs[0], verify_md5=True)
        assert (checked, failed) == (2 * GOFS[gof][2], 0)
    if other is not None:
        assert other.transcode_gof_quality_frames([source(gof, kind)], [params(R, kind, v)], tg) == (outs, res)


# ------------------------------------------------------------------------------------------------ D1 floors frame by frame (rbt_submit_gof_d1_frames)
D_LO, D_HI = 24, 40


@functools.lru_cache(maxsize=None)
def d1_case():
    """the recipe of d1_floor_cases.case("synth") with three point-cloud frames from three base atlases: src [occupancy, geometry], the OUTPUT atlas (precision 4), the patch
    list of every frame"""
    import rbt_lib
    R = rbt_lib.module(); w, h, n_pc, seed = GOFS["d1"]
    return dict(src=[occupancy("d1"), source("d1", "geo")], atlas=R.AtlasParams(w, h, 16, 4, 2, 1, 1, 0), patches=[synth.atlas_patches(R, w, h, seed + f) for f in range(n_pc)], w=w, h=h, n_frames=n_pc)


@functools.lru_cache(maxsize=None)
def d1_table(rd):
    """q -> ([occupancy, geometry] of the oracle at QP q, [O.d1(A_f, B_f(q)) per frame]) for q = 24..40; A_f: the reconstruction on the decoded input (D1 rule 4)"""
    import d1_floor_cases as DC
    c = d1_case(); w, h, n = c["w"], c["h"], c["n_frames"]
    om, ow, oh, *_ = O.decode(c["src"][0]); g = O.decode(c["src"][1])[0]
    a_in = DC._copy_atlas(c["atlas"], occupancy_precision=w // ow)
    A = [O.reconstruct(a_in, c["patches"][f], DC.luma(om[f], ow, oh), DC.luma(g[2 * f], w, h), DC.luma(g[2 * f + 1], w, h), 10)[0] for f in range(n)]
    out = {}
    for q in range(D_LO, D_HI + 1):
        o = O.transcode_data(c["src"], [OCC_P, (1, q, 4, 5, -1, 0, rd, 0)])
        pm, pw, ph, *_ = O.decode(o[0]); b = O.decode(o[1])[0]
        out[q] = (o, [O.d1(A[f], O.reconstruct(c["atlas"], c["patches"][f], DC.luma(pm[f], pw, ph), DC.luma(b[2 * f], w, h), DC.luma(b[2 * f + 1], w, h), 10)[0], 1023) for f in range(n)])
    return out


def d1_curves(rd):
    t = d1_table(rd)
    return [{q: float(v[1][f]["psnr"]) for q, v in t.items()} for f in range(d1_case()["n_frames"])]


def d1_floor(rd, near_db, qp_list, lo=D_LO, hi=D_HI):
    """a floor with the siblings' margins on the curve of every frame"""
    import d1_floor_cases as DC
    f = int(round(near_db * 1000))
    for _ in range(3000):
        try:
            for D in d1_curves(rd):
                DC.check_margins({q: D[q] for q in range(lo, hi + 1)}, f, qp_list, lo, hi)
            return f
        except AssertionError:
            f += 3
    raise AssertionError("no floor with the margins near %r" % near_db)


def d1_params(R, qp, rd):
    return [occ_params(R), params(R, "geo", variant(occupancy_rd=rd), qp)]


def d1_target(R, floor, lo=D_LO, hi=D_HI, stat=0):
    c = d1_case()
    return [R.D1Target(), R.D1Target(c["atlas"], c["patches"], floor, stat, lo, hi, 0, None)]


def check_d1_result(R, ctx, rd, floor, qp, lo, hi, outs, res, want_distinct=False):
    """the geometry entry's result against the Python walk on the oracle's D1 table of every frame; -> the walks"""
    import d1_floor_cases as DC
    c = d1_case(); t = d1_table(rd); n = c["n_frames"]; curves = d1_curves(rd)
    if not floor:
        lo = hi = qp
    walks = []
    for D in curves:
        q0, qs, qstar, met = DC.walk(D, qp, floor, lo, hi) if floor else (qp, qp, qp, 1)
        walks.append((q0, qs, qstar, met, walk_rounds(q0, qs, lambda q, D=D: D[q] >= floor / 1000.0, lo, hi)))
    r = res[1]; Q = [wk[2] for wk in walks]
    assert r["n_frames"] == n and r["qp_probe"] == walks[0][0] and r["cloud_ms"] >= 0
    for f, (wk, p) in enumerate(zip(walks, r["frames"])):
        assert (p["qp"], p["qp_start"], p["met"]) == (wk[2], wk[1], wk[3]), (floor, qp, f, p, wk)
        assert p["n_encodes"] == sum(len(x) for x in wk[4]) and 1 <= p["n_encodes"] <= abs(wk[2] - wk[1]) + 5, (f, p, wk)
        assert p["figure"] == float(r["d1"][f]["psnr"]) and abs(p["figure"] - curves[f][wk[2]]) < 1e-4
        if p["met"] and floor:
            assert p["figure"] >= floor / 1000.0
    DC.same_frames(r["d1"], [t[q][1][f] for f, q in enumerate(Q)])                # the rbt_d1_result of every frame at its pick: the oracle's of the constant-QP stream there
    n_rounds = max(len(wk[4]) for wk in walks)
    assert r["n_passes"] == sum(max(len(wk[4][k]) if k < len(wk[4]) else 0 for wk in walks) for k in range(n_rounds))
    assert r["pictures_encoded"] == 2 * sum(p["n_encodes"] for p in r["frames"]) and r["met_all"] == int(all(p["met"] for p in r["frames"]))
    assert outs[1] == ctx.transcode_gof_frame_qp(c["src"], d1_params(R, qp, rd), [None, Q])[1]
    assert outs[0] == t[D_LO][0][0] and (res[0]["n_frames"], res[0]["frames"], res[0]["d1"]) == (0, [], None)
    assert [p["bytes"] for p in r["frames"]] == frame_sizes(outs[1]) and r["bytes"] == len(outs[1])
    got = O.decode(outs[1])[0]
    for f, q in enumerate(Q):                                                     # composition: frame f is the oracle's constant-QP stream's frame at its pick
        assert np.array_equal(got[2 * f:2 * f + 2], O.decode(t[q][0][1])[0][2 * f:2 * f + 2]), (f, q)
    if want_distinct:
        assert len(set(Q)) >= 2, ("a degenerate input: every frame settles at one QP", Q)
    return walks


def d1_floor_cases(rd):
    """(floor, params.qp, lo, hi, distinct): between the worst and the best frame at QP 32 from 30 and 24; a floor that lo misses for the worst frame only; floor 0"""
    curves = d1_curves(rd)
    at = lambda q: sorted(D[q] for D in curves)
    mid = d1_floor(rd, (at(32)[0] + at(32)[-1]) / 2, [30, 24])
    top = at(D_LO)
    return [(mid, 30, D_LO, D_HI, True), (mid, 24, D_LO, D_HI, True), (d1_floor(rd, (top[0] + top[1]) / 2, [30]), 30, D_LO, D_HI, False), (0, 30, D_LO, D_HI, False)]


def check_d1_frames(R, ctx, rd, other=None):
    """every frame walks on the D1 of its own cloud. The frames settle after different numbers of rounds, so the clouds of the later passes are made of a subset of the
    frames: the gather descriptors go by the coded picture of the pass, the maps, the patch lists and the references by the frame - three different patch lists here"""
    c = d1_case(); subset = False
    for floor, qp, lo, hi, distinct in d1_floor_cases(rd):
        tg = d1_target(R, floor, lo, hi)
        calls = [ctx.transcode_gof_d1_frames(c["src"], d1_params(R, qp, rd), tg)]
        if distinct and qp == 30:
            calls.append(ctx.wait_gof_d1_frames(ctx.submit_gof_d1_frames(c["src"], d1_params(R, qp, rd), tg)))
        for outs, res in calls:
            walks = check_d1_result(R, ctx, rd, floor, qp, lo, hi, outs, res, distinct)
        subset |= carries_a_later_frame_without_an_earlier_one(walks)
        if floor and not distinct:
            assert [p["met"] for p in res[1]["frames"]].count(0) == 1 and res[1]["met_all"] == 0
        if not floor:
            assert outs[1] == d1_table(rd)[qp][0][1] and res[1]["n_passes"] == 1
        if other is not None:
            o2, r2 = other.transcode_gof_d1_frames(c["src"], d1_params(R, qp, rd), tg)
            for r in res + r2:
                r["cloud_ms"] = 0.0                                              # (a time)
            assert (o2, r2) == (outs, res), (floor, qp)
    assert subset, "no pass carried a later frame without an earlier one"


def check_d1_arguments(R, ctx):
    """stat must be 0; the pairing; the existing calls keep refusing stat 2"""
    c = d1_case()

    def refused(fn, tg, word):
        with pytest.raises(R.RbtError) as e:
            fn(c["src"], d1_params(R, 30, 0), tg)
        assert e.value.code == -4 and word in str(e.value), str(e.value)
    refused(ctx.transcode_gof_d1_frames, d1_target(R, 60000, stat=1), "stat")
    refused(ctx.transcode_gof_d1_frames, d1_target(R, 60000, stat=2), "stat")
    refused(ctx.transcode_gof_d1, d1_target(R, 60000, stat=2), "stat")
    refused(ctx.transcode_gof_d1_frames, d1_target(R, -1), "negative")
    refused(ctx.transcode_gof_d1_frames, d1_target(R, 60000, 31, 30), "range")
    one = R.D1Target(R.AtlasParams(c["w"], c["h"], 16, 4, 1, 1, 1, 0), c["patches"] * 2, 60000, 0, D_LO, D_HI, 0, None)      # map_count 1: six frames of one picture
    refused(ctx.transcode_gof_d1_frames, [R.D1Target(), one], "map_count")
    job = ctx.submit_gof_d1_frames(c["src"], d1_params(R, 30, 0), d1_target(R, 0))
    for wrong in (ctx.wait_gof, ctx.wait_gof_d1, ctx.wait_gof_quality, ctx.wait_gof_quality_frames):
        with pytest.raises(R.RbtError) as e:
            wrong(job)
        assert e.value.code == -4
    assert ctx.job_memory(job) > 0
    outs, res = ctx.wait_gof_d1_frames(job)
    assert outs[1] == d1_table(0)[30][0][1]
    job = ctx.submit_gof_d1(c["src"], d1_params(R, 30, 0), d1_target(R, 0))
    with pytest.raises(R.RbtError) as e:
        ctx.wait_gof_d1_frames(job)
    assert e.value.code == -4
    ctx.wait_gof_d1(job)
