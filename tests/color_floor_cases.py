"""Cases and checks of the transcode of attributes to a colour PSNR floor (rbt_submit_gof_color / rbt_wait_gof_color / rbt_transcode_gof_color; second half of this file)
and of the recolouring route under it (rbt_pcloud_set_colors, rbt_score_pair_*, rbt_gather_420; csrc/rbt_score.h, csrc/rbt_cloudmaps.h; first half), shared by
tests/test_color_floor.py (serial host emulation of the kernel bodies) and tests/test_gpu_color_floor.py (the GPU build). A recoloured cloud is held against a fresh
upload of the same points with the new colours, field for field and bit for bit, and against the brute-force restatements of tests/color_cases.py (merge, one_way,
derived); a pair's colour result against the colour part of rbt_score; the 4:2:0 gather against NumPy slicing. Everything is exact: integer sums, and float fields that
come from the one host routine all these calls share."""
import functools
import numpy as np
import pytest
import oracle_lib as O
import rbt_lib
import synth
import pcc_cases
import quality_cases as QC
import color_cases as CC
import score_cases as SC
import d1_floor_cases as DC

F32 = np.float32
SET_SIZES = (1, 255, 256, 257)
GATHER_WIDTHS = (2, 14, 72, 264)           # chroma rows of 1, 7, 36 and 132 samples
GATHER_WINDOWS = ((0, 0), (2, 4), (18, 6), (8, 2))


def rng(seed):
    return np.random.default_rng(9100 + seed)


def crowded_cloud():
    """-> (xyz, rgb): voxels of 1, 2 and 300 points (a count that does not fit a byte), and 200 points drawn from a 5 x 5 x 5 cube (duplicates of different colours), shuffled"""
    r = rng(0)
    xyz = np.concatenate([np.tile([[40, 41, 42]], (300, 1)), np.tile([[44, 41, 42]], (2, 1)), [[47, 47, 47]], r.integers(50, 55, (200, 3))]).astype(np.int16)
    rgb = r.integers(0, 256, (len(xyz), 3)).astype(np.uint8)
    rgb[:300] = r.integers(225, 256, (300, 3))           # (the 300-point voxel's sums pass 65535)
    p = r.permutation(len(xyz))
    xyz, rgb = xyz[p], rgb[p]
    _, cnt = np.unique(xyz, axis=0, return_counts=True)
    assert 1 in cnt and 2 in cnt and cnt.max() > 255 and rgb[(xyz == [40, 41, 42]).all(1)].astype(np.int64).sum(0).min() > 65535
    return xyz, rgb


def sized_cloud(n):
    """n points from a 4 x 4 x 4 cube: duplicates from a handful of points on"""
    r = rng(n)
    return r.integers(60, 64, (n, 3)).astype(np.int16), r.integers(0, 256, (n, 3)).astype(np.uint8)


def source_cloud():
    """the other side of every score: 400 points around the clouds above, with colours and normals"""
    r = rng(1)
    xyz = r.integers(38, 66, (400, 3)).astype(np.int16)
    return xyz, r.integers(0, 256, (400, 3)).astype(np.uint8), SC.normals(0, 400)


def new_colors(n, seed):
    return rng(100 + seed).integers(0, 256, (n, 3)).astype(np.uint8)


def brute_color(a, ca, b, cb):
    """(sse_ab, sse_ba, n_a, n_b) by tests/color_cases.py"""
    A, mA, _ = CC.merge(a, ca); B, mB, _ = CC.merge(b, cb)
    return CC.one_way(A, mA, B, mB)[0], CC.one_way(B, mB, A, mA)[0], len(A), len(B)


def check_color_against_brute_force(col, a, ca, b, cb):
    sab, sba, na, nb = brute_color(a, ca, b, cb)
    assert (col["sse_ab"], col["sse_ba"], col["n_a"], col["n_b"]) == (sab, sba, na, nb), (col, sab, sba)
    CC.check_derived(col)


def check_set_colors(ctx, xyz, rgb, other=None):
    """recoloured == fresh upload in all parts and both roles, D1 and D2 untouched, twice the same colours change nothing, a cloud without colours gets them; -> the results
    (for GPU == host emulation)"""
    sx, sc, sn = source_cloud()
    n = len(xyz)
    c1, c2 = new_colors(n, 1), new_colors(n, 2)
    hs, hb, plain = ctx.pcloud_upload(sx, sc, sn), ctx.pcloud_upload(xyz, rgb, SC.normals(1, n)), ctx.pcloud_upload(xyz)
    fresh = [ctx.pcloud_upload(xyz, c, SC.normals(1, n)) for c in (c1, c2)]
    out = []
    try:
        before = ctx.score(hs, hb)
        assert before["parts"] == 7 and hb.points() == fresh[0].points()
        for c, hf in ((c1, fresh[0]), (c2, fresh[1]), (c2, fresh[1])):          # (the third round: the same colours again)
            hb.set_colors(c)
            assert hb.points() == hf.points()
            got, want = ctx.score(hs, hb), ctx.score(hs, hf)
            assert SC.same_result(got, want), (got, want)
            assert got["d1"] == before["d1"] and got["d2"] == before["d2"]
            back, wback = ctx.score(hb, hs), ctx.score(hf, hs)                    # the recoloured cloud as the source: its own merged colour is the query's
            assert SC.same_result(back, wback), (back, wback)
            check_color_against_brute_force(got["color"], sx, sc, xyz, c)
            out += [got, back]
        assert ctx.score(hs, plain)["parts"] == 3                              # no colours yet: the clouds do not allow the colour part
        plain.set_colors(c1)
        got = ctx.score(hs, plain)
        assert got["parts"] == 7 and got["color"] == ctx.score(hs, fresh[0])["color"]
        out.append(got)
    finally:
        for h in [hs, hb, plain] + fresh: h.release()
    if other is not None:
        theirs = check_set_colors(other, xyz, rgb)
        assert all(SC.same_result(x, y) for x, y in zip(out, theirs))
    return out


def check_pair(ctx, k, other=None):
    """base cloud k of tests/score_cases.py (tie shares of 0.15 and more in both directions): the pair's colour result == the colour part of rbt_score, before and after
    either cloud gets new colours, and == the brute force"""
    a, ca, na, b, cb = SC.base(k)
    ref = SC.reference(("base", k), SC.base(k))
    assert ref["ties"][0] >= 0.15 and ref["ties"][1] >= 0.15                      # tie sets larger than 1 are under test
    ha, hb = ctx.pcloud_upload(a, ca, na), ctx.pcloud_upload(b, cb)
    pair = ctx.score_pair(ha, hb)
    out = []
    try:
        got = pair.color()
        assert got == ctx.score(ha, hb, parts=SC.COLOR)["color"]
        assert (got["sse_ab"], got["sse_ba"]) == tuple(ref["color"])
        out.append(got)
        cb2, ca2 = new_colors(len(b), 3 + k), new_colors(len(a), 13 + k)
        hb.set_colors(cb2)
        got = pair.color()
        assert got == ctx.score(ha, hb, parts=SC.COLOR)["color"] and got != out[0]
        check_color_against_brute_force(got, a, ca, b, cb2)
        out.append(got)
        ha.set_colors(ca2)
        got = pair.color()
        assert got == ctx.score(ha, hb, parts=SC.COLOR)["color"] and got != out[1]
        check_color_against_brute_force(got, a, ca2, b, cb2)
        out.append(got)
        assert pair.color() == got                                                # (a second look changes nothing: the result block is the call's own)
    finally:
        pair.release(); ha.release(); hb.release()
    if other is not None:
        assert out == check_pair(other, k)
    return out


def check_pair_single_points(ctx, other=None):
    """a single-point cloud on either side and on both"""
    a, ca, _, b, cb = SC.base(1)
    out = []
    for (x, cx), (y, cy) in (((a[:1], ca[:1]), (b, cb)), ((a, ca), (b[:1], cb[:1])), ((a[:1], ca[:1]), (b[:1], cb[:1]))):
        hx, hy = ctx.pcloud_upload(x, cx), ctx.pcloud_upload(y, cy)
        pair = ctx.score_pair(hx, hy)
        try:
            got = pair.color()
            assert got == ctx.score(hx, hy, parts=SC.COLOR)["color"]
            check_color_against_brute_force(got, x, cx, y, cy)
            hy.set_colors(new_colors(len(y), 30))
            assert pair.color() == ctx.score(hx, hy, parts=SC.COLOR)["color"]
            out.append(got)
        finally:
            pair.release(); hx.release(); hy.release()
    if other is not None:
        assert out == check_pair_single_points(other)
    return out


def check_arguments(R, ctx, make_ctx):
    """every refusal leaves the context usable"""
    a, ca, na, b, cb = SC.small_pair()
    ha, hb, bare = ctx.pcloud_upload(a, ca, na), ctx.pcloud_upload(b, cb), ctx.pcloud_upload(b)
    c2 = make_ctx()
    theirs = c2.pcloud_upload(b, cb)
    try:
        SC.refused(R, lambda: theirs.__class__(ctx, theirs.h).set_colors(cb))      # a cloud of another context
        assert ctx.L.rbt_pcloud_set_colors(ctx.h, theirs.h, cb.ctypes.data) == -4 and b"not a cloud of this context" in ctx.L.rbt_last_error(ctx.h)
        assert ctx.L.rbt_pcloud_set_colors(ctx.h, hb.h, None) == -4
        SC.refused(R, lambda: ctx.score_pair(ha, theirs))
        SC.refused(R, lambda: ctx.score_pair(None, hb))
        pair = ctx.score_pair(ha, bare)
        SC.refused(R, lambda: pair.color())                                       # a cloud without colours
        bare.set_colors(cb)
        assert pair.color() == ctx.score(ha, bare, parts=SC.COLOR)["color"]       # ... which has them now
        assert ctx.L.rbt_score_pair_color(c2.h, pair.h, R.C.byref(R.ColorResult())) == -4     # a pair of another context
        bare.release()
        SC.refused(R, lambda: pair.color())                                       # a cloud of the pair has gone
        pair.release()
        SC.check_still_works(ctx)
        left = ctx.score_pair(ha, hb)                                             # (outstanding when its context goes: released with it)
        assert left.color() == ctx.score(ha, hb, parts=SC.COLOR)["color"]
        lost = c2.score_pair(theirs, theirs)
        assert lost.color()["sse_ab"] == [0, 0, 0]
        left.release()
    finally:
        for h in (ha, hb, theirs): h.release()
        c2.close()


def coded_pictures(n, stride, rows, cstride, crows, seed):
    return rng(200 + seed).integers(0, 1024, (n, stride * rows + 2 * cstride * crows)).astype(np.uint16)


def gather_want(src, stride, rows, cstride, crows, x0, y0, w, h):
    n = src.shape[0]
    y = src[:, :stride * rows].reshape(n, rows, stride)[:, y0:y0 + h, x0:x0 + w].reshape(n, -1)
    c = src[:, stride * rows:].reshape(n, 2, crows, cstride)[:, :, y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2].reshape(n, -1)
    return np.concatenate([y, c], axis=1)


def check_gather(ctx, w, n_pics):
    """padded pictures whose chroma stride is not half the luma stride, every misalignment, windows at the origin and offset in both directions"""
    h = 6
    stride, rows, cstride, crows = w + 18, h + 6, w // 2 + 11, h // 2 + 4
    src = coded_pictures(n_pics, stride, rows, cstride, crows, w)
    for mis in range(8):
        for x0, y0 in GATHER_WINDOWS:
            got = ctx.gather_420(src, stride, rows, cstride, crows, x0, y0, w, h, mis)
            assert np.array_equal(got, gather_want(src, stride, rows, cstride, crows, x0, y0, w, h)), (w, mis, x0, y0)
    # packed pictures (stride == width, chroma stride == half of it), and two rows only
    src = coded_pictures(n_pics, w, 2, w // 2, 1, w + 1)
    for mis in (0, 3):
        assert np.array_equal(ctx.gather_420(src, w, 2, w // 2, 1, 0, 0, w, 2, mis), src)


def check_gather_feeds_upconversion(ctx):
    """the packed pictures are what the up-conversion reads: 72 x 40 cut out of padded 10-bit pictures == the up-conversion of the sliced pictures"""
    w, h, stride, rows = 72, 40, 80, 48
    src = coded_pictures(2, stride, rows, stride // 2, rows // 2, 7)
    got = ctx.gather_420(src, stride, rows, stride // 2, rows // 2, 0, 0, w, h, 5)
    want = gather_want(src, stride, rows, stride // 2, rows // 2, 0, 0, w, h)
    assert np.array_equal(got, want)
    up = ctx.yuv420_to_yuv444(got, w, h, 10)
    assert np.array_equal(up, CC.up444(want, w, h, 10))


def check_gather_arguments(R, ctx):
    src = coded_pictures(1, 16, 8, 8, 4, 0)
    good = lambda **k: ctx.gather_420(src, *[k.get(n, v) for n, v in (("stride", 16), ("rows", 8), ("cstride", 8), ("crows", 4), ("x0", 0), ("y0", 0), ("w", 8), ("h", 4), ("mis", 0))])
    good()
    for bad in ({"w": 7}, {"h": 3}, {"x0": 1}, {"y0": 1}, {"w": 0}, {"x0": 10}, {"y0": 6}, {"mis": 8}, {"mis": -1}, {"x0": -2}):
        SC.refused(R, lambda: good(**bad))
    SC.refused(R, lambda: ctx.gather_420(coded_pictures(1, 16, 8, 6, 4, 0), 16, 8, 6, 4, 0, 0, 14, 4))      # half the window outside the chroma plane
    good()


# ================================================================================================ the job: rbt_submit_gof_color / rbt_wait_gof_color / rbt_transcode_gof_color
# The definition is a composition of public calls (include/rbt.h, "transcoding attributes to a colour PSNR floor"): for every q of the range rbt_transcode_gof at q ->
# rbt_decode -> rbt_pcloud_from_maps -> rbt_score(RBT_SCORE_COLOR), the same for A_f on the input streams; that gives D(q), and the walk restated in
# tests/d1_floor_cases.py gives q0, qs, q* and met. The tables are computed once per library and shared by the tests of a run.
MIN, MEAN = 0, 1
LO, HI = 30, 40
GEO_QP = 28                                  # the geometry source is coded at its own QP, whatever the attribute QP
walk, check_margins, pick_floor, luma = DC.walk, DC.check_margins, DC.pick_floor, DC.luma


def _R():
    return rbt_lib.module()


@functools.lru_cache(maxsize=None)
def job_case(name):
    """-> dict: src [occupancy, geometry, attribute stream], atlas (the OUTPUT atlas, precision 4), patches (one list per frame), w, h, n_frames, transfer"""
    c = dict(DC.case(name))
    w, h = c["w"], c["h"]
    if name == "synth":
        attr = QC.gof_source(w, h, 21)[2]
    elif name == "seam_smooth":                # the atlas' own random attribute pictures for frame 0, fresh ones for frame 1
        t0, t1 = pcc_cases.seam_atlas(_R(), 0, tiles=3, prec=2)[6:8]
        r = rng(300)
        attr = O.encode_hm(np.stack([t0, t1, smooth_attr(r, w, h), smooth_attr(r, w, h)]), w, h, 10, 16)[0]
    else:                                      # 72 x 40 cut out of the 128 x 128 attribute maps: coded padded, the chroma planes are 36 x 20
        assert name == "cropped"
        big = synth.make_maps(128, 128, 21)["attr"]
        fr = np.stack([np.concatenate([p[:hh, :ww].ravel() for p, (ww, hh) in zip(QC.planes(f, 128, 128), ((w, h), (w // 2, h // 2), (w // 2, h // 2)))]) for f in big])
        attr = O.encode_hm(fr, w, h, 10, 16)[0]
    c["src"] = list(c["src"]) + [attr]
    c["transfer"] = 1
    return c


def smooth_attr(r, w, h):
    """a 4:2:0 picture of smooth ramps with a little noise (10 bits)"""
    yy, xx = np.mgrid[0:h, 0:w]
    y = np.clip(300 + 3 * xx + 2 * yy + r.integers(-8, 9, (h, w)), 0, 1023)
    u = np.clip(400 + 4 * xx[:h // 2, :w // 2] + r.integers(-6, 7, (h // 2, w // 2)), 0, 1023)
    v = np.clip(600 - 3 * yy[:h // 2, :w // 2] + r.integers(-6, 7, (h // 2, w // 2)), 0, 1023)
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()]).astype(np.uint16)


def job_params(R, qp, rd=0):
    return [R.StreamParams(*QC.OCC_P, 0), QC.params(R, "geo", GEO_QP, rd), QC.params(R, "attr", qp, rd)]


def job_target(R, name, floor=0, stat=MIN, channel=0, lo=LO, hi=HI, reference=None, **kw):
    c = job_case(name)
    return [R.ColorTarget(), R.ColorTarget(), R.ColorTarget(kw.get("atlas", c["atlas"]), c["patches"], floor, channel, stat, lo, hi, kw.get("filter", 0), kw.get("transfer", c["transfer"]), reference)]


def clouds_of(ctx, name, streams, prec, transfer=None):
    """rbt_decode + rbt_pcloud_from_maps on [occupancy, geometry, attribute] streams -> ([PCloud per frame], [(n_smoothed, n_changed) per frame])"""
    c = job_case(name); w, h = c["w"], c["h"]
    om, ow, oh, *_ = ctx.decode(streams[0], verify_md5=False); g, *_ = ctx.decode(streams[1], verify_md5=False); t, tw, th, *_ = ctx.decode(streams[2], verify_md5=False)
    assert (tw, th, ow * prec) == (w, h, w)
    a = pcc_cases._copy_atlas(_R(), c["atlas"], occupancy_precision=prec)
    out, moved = [], []
    for f in range(c["n_frames"]):
        cloud, host = ctx.pcloud_from_maps(a, c["patches"][f], luma(om[f], ow, oh), luma(g[2 * f], w, h), luma(g[2 * f + 1], w, h), 10, t[2 * f], t[2 * f + 1], 10, 0,
                                           c["transfer"] if transfer is None else transfer, host_copy=True)
        out.append(cloud); moved.append((ctx.n_smoothed, ctx.n_changed))
    return out, moved


_TABLES = {}


def job_table(ctx, name, rd=0, ref="input"):
    """q -> ([stream bytes x 3] of rbt_transcode_gof at attribute QP q, [colour dict per frame], [(n_smoothed, n_changed) per frame]); ref: "input" (rule 4's own
    reference) or "source" (another cloud with colours: the decoded input moved by one voxel and recoloured)"""
    key = (ctx.lib_path, name, rd, ref)
    if key in _TABLES: return _TABLES[key]
    R = _R(); c = job_case(name)
    A, _ = clouds_of(ctx, name, c["src"], c["w"] // (ctx.decode(c["src"][0], verify_md5=False)[1]))
    if ref == "source":
        for h in A: h.release()
        A = [ctx.pcloud_upload(x, rgb) for x, rgb in other_reference(ctx, name)]
    out = {}
    try:
        for q in range(LO, HI + 1):
            streams = ctx.transcode_gof(c["src"], job_params(R, q, rd))
            B, moved = clouds_of(ctx, name, streams, 4)
            try:
                out[q] = (streams, [ctx.score(A[f], B[f], parts=SC.COLOR)["color"] for f in range(c["n_frames"])], moved)
            finally:
                for h in B: h.release()
    finally:
        for h in A: h.release()
    _TABLES[key] = out
    return out


_OTHER = {}


def other_reference(ctx, name):
    """[(xyz, rgb) per frame]: the cloud of the decoded input with every coordinate one further along x and its colours reversed - a reference that is not rule 4's"""
    if name not in _OTHER:
        c = job_case(name); w, h = c["w"], c["h"]
        om, ow, oh, *_ = ctx.decode(c["src"][0], verify_md5=False); g, *_ = ctx.decode(c["src"][1], verify_md5=False); t, *_ = ctx.decode(c["src"][2], verify_md5=False)
        a = pcc_cases._copy_atlas(_R(), c["atlas"], occupancy_precision=w // ow)
        out = []
        for f in range(c["n_frames"]):
            cloud, host = ctx.pcloud_from_maps(a, c["patches"][f], luma(om[f], ow, oh), luma(g[2 * f], w, h), luma(g[2 * f + 1], w, h), 10, t[2 * f], t[2 * f + 1], 10, 0, c["transfer"], host_copy=True)
            cloud.release()
            out.append(((host[0] + np.array([1, 0, 0], np.int16)).astype(np.int16), host[4][:, ::-1].copy()))
        _OTHER[name] = out
    return _OTHER[name]


def figure(frames, stat, channel=0):
    p = [float(f["psnr"][channel]) for f in frames]
    return sum(p) / len(p) if stat == MEAN else min(p)


def curve(t, stat=MIN, channel=0):
    return {q: figure(v[1], stat, channel) for q, v in t.items()}


def strip(x):
    return (x[0], [{k: v for k, v in r.items() if k != "cloud_ms"} for r in x[1]])


def check_result(t, qp, floor, stat, channel, outs, res, lo=LO, hi=HI):
    """res against the definition's walk on the composition's table t; the stream is rbt_transcode_gof's at q*; every field of every frame equal, floats bit for bit"""
    D = curve(t, stat, channel)
    q0, qs, qstar, met = walk(D, qp, floor, lo, hi) if floor else (qp, qp, qp, 1)
    r = res[2]
    assert (r["qp_probe"], r["qp_start"], r["qp"], r["met"]) == (q0, qs, qstar, met), (floor, qp, r, (q0, qs, qstar, met))
    assert 1 <= r["n_encodes"] <= abs(qstar - qs) + 5, (floor, qp, r)
    assert outs == t[qstar][0] and r["bytes"] == len(outs[2])
    assert r["frames"] == t[qstar][1], (r["frames"], t[qstar][1])
    for c in range(3):
        p = [float(f["psnr"][c]) for f in r["frames"]]
        assert r["min_psnr"][c] == min(p) and r["mean_psnr"][c] == sum(p) / len(p)
    assert r["n_frames"] == len(r["frames"]) and r["cloud_ms"] >= 0
    assert (res[0]["qp"], res[0]["bytes"], res[0]["n_frames"], res[0]["frames"]) == (8, len(outs[0]), 0, [])
    assert (res[1]["qp"], res[1]["bytes"], res[1]["n_encodes"], res[1]["n_frames"], res[1]["frames"]) == (GEO_QP, len(outs[1]), 1, 0, [])
    return r


def floors_of(D, qps, lo=LO, hi=HI):
    """floors with the margins: one above every D(q) (unreachable), one below every D(q), and midpoints between neighbouring values"""
    vals = sorted(set(D.values()))
    near = [vals[-1] + 0.5, vals[0] - 0.5] + [(D[q] + D[q + 1]) / 2 for q in (lo + 2, hi - 3)]
    return [pick_floor(D, x, qps, lo, hi) for x in near]


def check_job_case(R, ctx, name, table_ctx=None):
    """the walk on one case: floors above, below and between the table's values, from several starting QPs; at least two different q* and one unreachable floor. On the seam
    atlas the floor is on the mean: its first frame carries the atlas' random attribute pictures, whose colour PSNR (12.4 dB) rises with the QP, and it is the worst frame"""
    stat, qps = (MEAN, (32,)) if name == "seam_smooth" else (MIN, (30, 35, 40))
    t = job_table(table_ctx or ctx, name); D = curve(t, stat); c = job_case(name)
    assert len(set(D.values())) > 5, D                                                  # the table varies with q
    if name == "seam_smooth":                                                            # the transfer is under test: points moved and colours changed in some trial
        assert any(s > 0 and ch > 0 for v in t.values() for s, ch in v[2]), [v[2] for v in t.values()]
    ends = set()
    floors = floors_of(D, list(qps))
    for k, floor in enumerate(floors):
        for qp in (qps if k == 2 else qps[:1]):
            check_margins(D, floor, [qp])
            outs, res = ctx.transcode_gof_color(c["src"], job_params(R, qp), job_target(R, name, floor, stat))
            r = check_result(t, qp, floor, stat, 0, outs, res)
            ends.add((r["qp"], r["met"]))
    assert (LO, 0) in ends and len({q for q, m in ends if m}) >= 2, ends
    outs, res = ctx.transcode_gof_color(c["src"], job_params(R, 33), job_target(R, name))         # a floor of 0 reports only
    r = check_result(t, 33, 0, MIN, 0, outs, res)
    assert (r["qp"], r["met"], r["n_encodes"]) == (33, 1, 1)


def check_stats_and_channels(R, ctx, table_ctx=None):
    """both stats on two frames, all three channels"""
    t = job_table(table_ctx or ctx, "seam_smooth"); c = job_case("seam_smooth")
    assert all(v[1][0]["psnr"] != v[1][1]["psnr"] for v in t.values())                   # the two frames differ
    for stat, ch in ((MIN, 1), (MEAN, 0), (MEAN, 2)):
        D = curve(t, stat, ch)
        f = pick_floor(D, (D[34] + D[35]) / 2, [32])
        outs, res = ctx.transcode_gof_color(c["src"], job_params(R, 32), job_target(R, "seam_smooth", f, stat, ch))
        check_result(t, 32, f, stat, ch, outs, res)
    assert curve(t, MIN) != curve(t, MEAN) and curve(t, MIN, 0) != curve(t, MIN, 1) != curve(t, MIN, 2)


def check_reference_handles(R, ctx, table_ctx=None):
    """a handle that is rule 4's own cloud gives the same answer as no handle; another cloud gives its own table's"""
    c = job_case("synth"); tc = table_ctx or ctx
    t = job_table(tc, "synth"); D = curve(t)
    f = pick_floor(D, (D[34] + D[35]) / 2, [32])
    want = ctx.transcode_gof_color(c["src"], job_params(R, 32), job_target(R, "synth", f))
    A, _ = clouds_of(ctx, "synth", c["src"], 2)
    try:
        got = ctx.transcode_gof_color(c["src"], job_params(R, 32), job_target(R, "synth", f, reference=A))
        assert strip(got) == strip(want)
    finally:
        for h in A: h.release()
    ts = job_table(tc, "synth", 0, "source"); Ds = curve(ts)
    assert all(ts[q][1][0]["sse_ab"] != t[q][1][0]["sse_ab"] for q in t)
    fs = pick_floor(Ds, (Ds[34] + Ds[35]) / 2, [32])
    B = [ctx.pcloud_upload(x, rgb) for x, rgb in other_reference(tc, "synth")]
    try:
        outs, res = ctx.transcode_gof_color(c["src"], job_params(R, 32), job_target(R, "synth", fs, reference=B))
        check_result(ts, 32, fs, MIN, 0, outs, res)
    finally:
        for h in B: h.release()


def check_occupancy_rd(R, ctx, table_ctx=None):
    """occupancy_rd 1 on the geometry and the attribute entry"""
    c = job_case("synth"); t = job_table(table_ctx or ctx, "synth", 1); D = curve(t)
    assert any(t[q][0][2] != job_table(table_ctx or ctx, "synth")[q][0][2] for q in t)   # the streams differ from those coded without it
    f = pick_floor(D, (D[33] + D[34]) / 2, [36])
    outs, res = ctx.transcode_gof_color(c["src"], job_params(R, 36, 1), job_target(R, "synth", f))
    check_result(t, 36, f, MIN, 0, outs, res)


def check_against_independent_arithmetic(R, ctx):
    """synth at two QPs: the job's frames == the NumPy restatements of tests/color_cases.py on the oracle's decode of the oracle's streams"""
    c = job_case("synth"); w, h = c["w"], c["h"]
    def cloud(streams, prec):
        om, ow, oh, *_ = O.decode(streams[0]); g, *_ = O.decode(streams[1]); t, *_ = O.decode(streams[2])
        a = pcc_cases._copy_atlas(R, c["atlas"], occupancy_precision=prec)
        geo = (a, c["patches"][0], luma(om[0], ow, oh), luma(g[0], w, h), luma(g[1], w, h), 10)
        pic = CC._luma_picture
        xyz = O.reconstruct(*geo)[0]
        xs = O.reconstruct(*geo, pic(np.tile(np.arange(w), (h, 1))), pic(np.tile(np.arange(w), (h, 1))), 10)[1][:, 0].astype(np.int64)     # every point's pixel and map, from
        ys = O.reconstruct(*geo, pic(np.repeat(np.arange(h), w)), pic(np.repeat(np.arange(h), w)), 10)[1][:, 0].astype(np.int64)           # reconstructions of index pictures
        mp = O.reconstruct(*geo, pic(np.zeros((h, w))), pic(np.ones((h, w))), 10)[1][:, 0].astype(np.int64)
        assert mp.max() == 1
        return xyz, CC.yuv16_to_rgb8(CC.up444(t[:2], w, h, 10)[mp, :, ys, xs])
    ax, argb = cloud(c["src"], 2)
    for q in (31, 38):
        streams = O.transcode_data(c["src"], [QC.OCC_P, (1, GEO_QP, 4, 5, -1, 0, 0, 0), (19, q, 4, 5, -1, 0, 0, 0)])
        bx, brgb = cloud(streams, 4)
        outs, res = ctx.transcode_gof_color(c["src"], job_params(R, q), job_target(R, "synth"))
        assert outs == streams
        check_color_against_brute_force(res[2]["frames"][0], ax, argb, bx, brgb)


def check_jobs_in_flight(R, ctx, table_ctx=None, depth=4, n_jobs=6):
    """colour jobs mixed with plain rbt_submit_gof jobs, depth 4, collected out of order, each equal to the blocking call"""
    c = job_case("synth"); t = job_table(table_ctx or ctx, "synth"); D = curve(t)
    old = ctx.get_depth(); ctx.set_depth(depth)
    try:
        fs = [pick_floor(D, (D[q] + D[q + 1]) / 2, [32]) for q in (31, 34, 37)]
        plain = ctx.transcode_gof(c["src"], job_params(R, 33))
        done = 0
        for batch in (range(0, 4), range(4, n_jobs)):
            jobs = []
            for k in batch:
                jobs.append((k, ctx.submit_gof(c["src"], job_params(R, 33)) if k % 2 else ctx.submit_gof_color(c["src"], job_params(R, 32), job_target(R, "synth", fs[(k // 2) % 3]))))
            if len(jobs) == depth:
                with pytest.raises(R.RbtError) as e:
                    ctx.submit_gof_color(c["src"], job_params(R, 32), job_target(R, "synth", fs[0]))
                assert e.value.code == -7                                                # RBT_ERR_BUSY
            for k, job in jobs[::-1]:
                if k % 2: assert ctx.wait_gof(job) == plain
                else: check_result(t, 32, fs[(k // 2) % 3], MIN, 0, *ctx.wait_gof_color(job))
                done += 1
        assert done == n_jobs
    finally:
        ctx.set_depth(old)


def check_pairing_and_memory(R, ctx, table_ctx=None):
    """wrong pairings of submit and wait calls leave the job collectable; rbt_job_memory is at least the sum DESIGN.md 16 states"""
    c = job_case("seam_smooth"); t = job_table(table_ctx or ctx, "seam_smooth"); w, h, nf = c["w"], c["h"], c["n_frames"]
    job = ctx.submit_gof_color(c["src"], job_params(R, 33), job_target(R, "seam_smooth"))
    vol, pics, ys = (1 << 27) + (1 << 18), 2 * nf, w * h
    # per frame and cloud (B_f and the job's own A_f): a volume and 8 bytes per possible point of distances; the packed geometry planes; per trial the packed attribute
    # planes, their 4:4:4 planes and the two volumes of the transfer
    assert ctx.job_memory(job) >= 2 * nf * (vol + 8 * 2 * ys) + pics * ys * 2 + pics * ys * 3 + pics * ys * 6 + 2 * (1 << 27)
    for other in (ctx.wait_gof, ctx.wait_gof_rate, ctx.wait_gof_quality, ctx.wait_gof_d1):
        with pytest.raises(R.RbtError) as e:
            other(job)
        assert e.value.code == -4
    check_result(t, 33, 0, MIN, 0, *ctx.wait_gof_color(job))
    for submit, args, collect in ((ctx.submit_gof, (), ctx.wait_gof), (ctx.submit_gof_d1, ([R.D1Target()] * 3,), ctx.wait_gof_d1)):
        job = submit(c["src"], job_params(R, 33), *args)
        with pytest.raises(R.RbtError) as e:
            ctx.wait_gof_color(job)
        assert e.value.code == -4
        got = collect(job)
        assert (got[0] if args else got) == t[33][0]


def check_determinism(R, ctx):
    c = job_case("seam_smooth")
    tg = lambda: job_target(R, "seam_smooth", 30000, MEAN, 0)
    a = ctx.transcode_gof_color(c["src"], job_params(R, 34, 1), tg())
    b = ctx.transcode_gof_color(c["src"], job_params(R, 34, 1), tg())
    assert strip(a) == strip(b) and a[1][2]["n_frames"] == 2 and a[1][2]["n_encodes"] > 1


def check_job_arguments(R, ctx, table_ctx=None):
    """every refusal is RBT_ERR_PARAM with its reason, submits nothing and leaves the context usable, shown by a following good call"""
    c = job_case("synth"); src = c["src"]; t = job_table(table_ctx or ctx, "synth")
    old = ctx.get_depth(); ctx.set_depth(1)        # one slot: a refused submit that kept it would make the next call RBT_ERR_BUSY
    try:
        def refused(streams, ps, ts, word):
            for call in (ctx.transcode_gof_color, ctx.submit_gof_color):
                with pytest.raises(R.RbtError) as e:
                    call(streams, ps, ts)
                assert e.value.code == -4 and word in str(e.value), str(e.value)
            outs, res = ctx.transcode_gof_color(src, job_params(R, 33), job_target(R, "synth"))
            assert outs == t[33][0] and res[2]["frames"] == t[33][1]
        tg = lambda **kw: job_target(R, "synth", **kw)
        bad = tg(floor=30000); bad[2].struct_size += 4
        refused(src, job_params(R, 33), bad, "struct_size")
        refused(src, job_params(R, 33), [R.ColorTarget(), tg(floor=30000)[2], R.ColorTarget()], "non-attribute")
        for lo, hi in ((-1, 30), (30, 52), (31, 30), (52, 0)):
            refused(src, job_params(R, 33), tg(floor=30000, lo=lo, hi=hi), "range")
        refused(src, job_params(R, 33), tg(floor=30000, stat=2), "stat")
        refused(src, job_params(R, 33), tg(floor=30000, channel=3), "channel")
        refused(src, job_params(R, 33), tg(floor=30000, filter=5), "upsample_filter")
        refused(src, job_params(R, 33), tg(floor=30000, transfer=2), "attr_transfer")
        refused(src, job_params(R, 33), tg(floor=-1), "negative")
        none = tg(floor=30000); none[2].n_frames = 0
        refused(src, job_params(R, 33), none, "n_frames")
        refused(src[1:], job_params(R, 33)[1:], tg(floor=30000)[1:], "occupancy source")                      # no occupancy entry in front
        refused([src[0], src[2]], [job_params(R, 33)[0], job_params(R, 33)[2]], [R.ColorTarget(), tg(floor=30000)[2]], "geometry source")
        refused([src[0], src[2], src[1]], [job_params(R, 33)[k] for k in (0, 2, 1)], [R.ColorTarget(), tg(floor=30000)[2], R.ColorTarget()], "geometry source")   # ... it is behind
        refused(src, job_params(R, 33), tg(atlas=pcc_cases._copy_atlas(R, c["atlas"], width=256)), "atlas.width")
        refused(src, job_params(R, 33), tg(atlas=pcc_cases._copy_atlas(R, c["atlas"], map_count=1)), "map_count")
        refused(src, job_params(R, 33), tg(atlas=pcc_cases._copy_atlas(R, c["atlas"], occupancy_precision=2)), "occupancy_precision")
        two = R.ColorTarget(c["atlas"], c["patches"] * 2, 30000, 0, MIN, LO, HI)
        refused(src, job_params(R, 33), [R.ColorTarget(), R.ColorTarget(), two], "n_frames")
        bare = ctx.pcloud_upload(other_reference(table_ctx or ctx, "synth")[0][0])
        try:
            refused(src, job_params(R, 33), tg(floor=30000, reference=[bare]), "no colours")
        finally:
            bare.release()
        other = R.Context(lib_path=ctx.lib_path)
        try:
            h = other.pcloud_upload(*other_reference(table_ctx or ctx, "synth")[0])
            refused(src, job_params(R, 33), tg(floor=30000, reference=[h]), "not a cloud of this context")
            h.release()
        finally:
            other.close()
        # an empty cloud is found when the cloud is built: the job fails cleanly in its wait call and the context goes on
        with pytest.raises(R.RbtError) as e:
            ctx.transcode_gof_color(src, job_params(R, 33), [R.ColorTarget(), R.ColorTarget(), R.ColorTarget(c["atlas"], [[]], 30000, 0, MIN, LO, HI)])
        assert e.value.code == -4 and "empty point cloud" in str(e.value)
        assert ctx.transcode_gof(src, job_params(R, 35)) == t[35][0]
        outs, res = ctx.transcode_gof_color(src, job_params(R, 33), job_target(R, "synth"))
        assert outs == t[33][0] and res[2]["frames"] == t[33][1]
    finally:
        ctx.set_depth(old)


@functools.lru_cache(maxsize=None)
def big_cloud():
    """a 129 x 128 x 128 grid with colours: 2 113 536 distinct voxels, more than the 2^21 merged points the colour part allows"""
    g = np.stack(np.meshgrid(np.arange(129), np.arange(128), np.arange(128), indexing="ij"), -1).reshape(-1, 3)
    return (g + 200).astype(np.int16), (g * [1, 2, 3] % 251).astype(np.uint8)


def check_merged_limit(R, ctx, table_ctx=None):
    """rule 7: a cloud of more than 2^21 merged points is RBT_ERR_PARAM from the wait call - the geometry halves exist by then and are released with the job -, and from
    rbt_score_pair_color; the context goes on, the D1 part of the same clouds still works"""
    c = job_case("synth"); src = c["src"]; t = job_table(table_ctx or ctx, "synth")
    xyz, rgb = big_cloud()
    big = ctx.pcloud_upload(xyz, rgb)
    try:
        assert big.points() == (len(xyz), len(xyz)) and len(xyz) > 1 << 21
        tg = lambda: job_target(R, "synth", 30000, reference=[big])
        with pytest.raises(R.RbtError) as e:
            ctx.transcode_gof_color(src, job_params(R, 33), tg())
        assert e.value.code == -4 and "merged points" in str(e.value), str(e.value)
        job = ctx.submit_gof_color(src, job_params(R, 33), tg())                          # nothing at submit knows the cloud of a trial: the job is accepted
        with pytest.raises(R.RbtError) as e:
            ctx.wait_gof_color(job)
        assert e.value.code == -4 and "merged points" in str(e.value), str(e.value)
        outs, res = ctx.transcode_gof_color(src, job_params(R, 33), job_target(R, "synth"))   # ... and the context goes on
        assert outs == t[33][0] and res[2]["frames"] == t[33][1]
        pair = ctx.score_pair(big, big)
        try:
            with pytest.raises(R.RbtError) as e:
                pair.color()
            assert e.value.code == -4 and "2^21 merged points" in str(e.value), str(e.value)
            SC.refused(R, lambda: ctx.score(big, big, parts=SC.COLOR))
            d1 = ctx.score(big, big, parts=SC.D1)["d1"]
            assert (d1["n_a"], d1["n_b"], d1["sse_ab"], d1["sse_ba"]) == (len(xyz), len(xyz), 0, 0)
        finally:
            pair.release()
    finally:
        big.release()
    SC.check_still_works(ctx)
