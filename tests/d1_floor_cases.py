"""Transcoding geometry to a D1 floor (include/rbt.h: rbt_submit_gof_d1 / rbt_wait_gof_d1 / rbt_transcode_gof_d1, rbt_gather_luma): one set of cases for the host emulation
(tests/test_d1_floor.py) and the GPU (tests/test_gpu_d1_floor.py). Every case is held against the oracle: for q = 24..40 O.transcode_data gives the streams, O.decode,
O.reconstruct and O.d1 give D_f(q), and a restatement of the walk gives q0, qs, q*, met. Everything the oracle computes is cached in this module, so the host and the GPU
tests of one run share it."""
import functools
import math
import numpy as np
import pytest
import oracle_lib as O
import rbt_lib
import synth
import pcc_cases
import quality_cases as QC

MIN, MEAN = 0, 1
LO, HI = 24, 40
OCC_P = QC.OCC_P
INT_FIELDS = ("n_a", "n_b", "sse_ab", "sse_ba", "max_ab", "max_ba")


def _R():
    return rbt_lib.module()


def luma(frame, w, h):
    return frame[:w * h].reshape(h, w)


def _yuv(y, bd=10):
    h, w = y.shape
    c = np.full((h // 2) * (w // 2), 1 << (bd - 1), np.uint16)
    return np.concatenate([y.astype(np.uint16).ravel(), c, c])


def _copy_atlas(atlas, **kw):
    return pcc_cases._copy_atlas(_R(), atlas, **kw)


# ------------------------------------------------------------------------------------------------ the cases: streams, output atlas, patches per point-cloud frame
@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: src [occupancy stream, geometry stream], atlas (the OUTPUT atlas, precision 4), patches (one list per frame), w, h, n_frames"""
    R = _R()
    if name == "synth":                                  # 128x128, 1 frame, 2 maps, the patches of synth.atlas_layout, occupancy 64x64 -> 32x32
        w = h = 128
        return dict(src=QC.gof_source(w, h, 21)[:2], atlas=R.AtlasParams(w, h, 16, 4, 2, 1, 1, 0), patches=[synth.atlas_patches(R, w, h, 21)], w=w, h=h, n_frames=1)
    if name in ("seam", "seam_smooth"):                  # 96x96, 2 frames (the second 4 depth levels higher), patches that meet in space: what geometry smoothing is for
        atlas, patches, occ, d0, d1, *_ = pcc_cases.seam_atlas(R, 0, tiles=3, prec=2)
        w = h = atlas.width
        assert (w, atlas.grid_size, atlas.threshold_smoothing, occ.shape) == (96, 8, 64, (48, 48))
        up = lambda d: np.clip(d.astype(np.int64) + 16, 0, 1023).astype(np.uint16)
        geo = np.stack([_yuv(d0), _yuv(d1), _yuv(up(d0)), _yuv(up(d1))])
        occ_frames = np.stack([_yuv(occ, 8), _yuv(occ, 8)])
        src = [O.encode(occ_frames, w // 2, h // 2, 8, 8, gop=1, i_qp_offset=0, lossless=1, log2_ctb=5, rows_per_slice=0)[0], O.encode_hm(geo, w, h, 10, 16)[0]]
        out = _copy_atlas(atlas, occupancy_precision=4, geometry_smoothing=int(name == "seam_smooth"))
        return dict(src=src, atlas=out, patches=[patches, patches], w=w, h=h, n_frames=2)
    if name == "cropped":                                # 72x40 cut out of the 128x128 maps: every picture involved is coded padded (strides differ from widths)
        w, h = 72, 40
        occ = luma(synth.make_maps(128, 128, 21)["occ"][0], 64, 64)[:h // 2, :w // 2]
        src = [O.encode(_yuv(occ, 8)[None, :], w // 2, h // 2, 8, 8, gop=1, i_qp_offset=0, lossless=1, log2_ctb=5, rows_per_slice=0)[0], QC.cropped_stream()]
        return dict(src=src, atlas=R.AtlasParams(w, h, 8, 4, 2, 1, 1, 0), patches=[[R.Patch(0, 0, 9, 5, 100, 200, 50, 2, 0, 1, 0, 0, 1, 1)]], w=w, h=h, n_frames=1)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def input_clouds(name):
    """A_f of rule 4: the reconstruction on the decoded input, the atlas at the input occupancy's precision"""
    c = case(name); w, h = c["w"], c["h"]
    om, ow, oh, *_ = O.decode(c["src"][0]); g, gw, gh, *_ = O.decode(c["src"][1])
    assert (gw, gh) == (w, h) and om.shape[0] == c["n_frames"] and g.shape[0] == 2 * c["n_frames"]
    a = _copy_atlas(c["atlas"], occupancy_precision=w // ow)
    out, moved = [], []
    for f in range(c["n_frames"]):
        out.append(O.reconstruct(a, c["patches"][f], luma(om[f], ow, oh), luma(g[2 * f], w, h), luma(g[2 * f + 1], w, h), 10)[0]); moved.append(O.LAST_SMOOTHED)
    return out, moved


@functools.lru_cache(maxsize=None)
def source_clouds(name="synth"):
    """a deliberately different reference: the source maps of the synthetic atlas reconstructed without any coding"""
    c = case(name); w, h = c["w"], c["h"]
    m = synth.make_maps(w, h, 21)
    a = _copy_atlas(c["atlas"], occupancy_precision=2)
    return [O.reconstruct(a, c["patches"][0], luma(m["occ"][0], w // 2, h // 2), luma(m["geo"][0], w, h), luma(m["geo"][1], w, h), 10)[0]]


@functools.lru_cache(maxsize=None)
def trials(name, rd):
    """q -> (the oracle's [occupancy, geometry] streams at QP q, [B_f(q)], [points the smoothing moved])"""
    c = case(name); w, h = c["w"], c["h"]
    out = {}
    for q in range(LO, HI + 1):
        o = O.transcode_data(c["src"], [OCC_P, (1, q, 4, 5, -1, 0, rd, 0)])
        om, ow, oh, *_ = O.decode(o[0]); g, gw, gh, *_ = O.decode(o[1])
        assert (gw, gh, ow * 4, oh * 4) == (w, h, w, h)
        clouds, moved = [], []
        for f in range(c["n_frames"]):
            clouds.append(O.reconstruct(c["atlas"], c["patches"][f], luma(om[f], ow, oh), luma(g[2 * f], w, h), luma(g[2 * f + 1], w, h), 10)[0]); moved.append(O.LAST_SMOOTHED)
        out[q] = (o, clouds, moved)
    return out


@functools.lru_cache(maxsize=None)
def table(name, rd, ref="input"):
    """q -> [O.d1(A_f, B_f(q)) per frame]"""
    A = input_clouds(name)[0] if ref == "input" else source_clouds(name)
    return {q: [O.d1(A[f], b, 1023) for f, b in enumerate(v[1])] for q, v in trials(name, rd).items()}


def figure(frames, stat):
    p = [float(f["psnr"]) for f in frames]
    return sum(p) / len(p) if stat == MEAN else min(p)


def curve(t, stat=MIN):
    return {q: figure(v, stat) for q, v in t.items()}


# ------------------------------------------------------------------------------------------------ the walk, by the definition
def walk(D, qp, floor_mdb, lo=LO, hi=HI):
    """D: q -> D(q) -> (q0, qs, q*, met)"""
    F = floor_mdb / 1000.0
    ok = lambda q: D[q] >= F
    q0 = min(hi, max(lo, qp))
    qs = q0 if math.isinf(D[q0]) else min(hi, max(lo, q0 + int(D[q0] - F)))
    q = qs
    if ok(q):
        while q < hi and ok(q + 1):
            q += 1
        return q0, qs, q, 1
    while q > lo and not ok(q):
        q -= 1
    return q0, qs, q, int(ok(q))


def check_margins(D, floor_mdb, qp_list, lo=LO, hi=HI):
    """conditions on the inputs: the floor is at least 0.001 dB away from every D(q), and D(q0) - F at least 0.001 away from a whole number - no rounding can change an answer"""
    F = floor_mdb / 1000.0
    assert all(abs(D[q] - F) >= 0.001 for q in D), floor_mdb
    for qp in qp_list:
        x = D[min(hi, max(lo, qp))] - F
        assert abs(x - round(x)) >= 0.001, (floor_mdb, qp)


def pick_floor(D, near_db, qp_list, lo=LO, hi=HI):
    f = int(round(near_db * 1000))
    for _ in range(2000):
        try:
            check_margins(D, f, qp_list, lo, hi)
            return f
        except AssertionError:
            f += 3
    raise AssertionError("no floor with the margins near %r" % near_db)


def params(R, qp, rd=0):
    return [R.StreamParams(*OCC_P, 0), QC.params(R, "geo", qp, rd)]


def target(R, name, floor=0, stat=MIN, lo=LO, hi=HI, reference=None, **kw):
    c = case(name)
    return [R.D1Target(), R.D1Target(kw.get("atlas", c["atlas"]), c["patches"], floor, stat, lo, hi, kw.get("peak", 0), reference)]


def same_frames(got, want):
    """every integer field equals the oracle's; the float fields come from float arithmetic on the same integers on both sides"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert [g[k] for k in INT_FIELDS] == [w[k] for k in INT_FIELDS], (g, w)
        assert g["psnr"] == w["psnr"] or abs(g["psnr"] - w["psnr"]) < 1e-4


def check_result(name, rd, t, qp, floor, stat, outs, res, lo=LO, hi=HI):
    """res against the definition's walk on the oracle's table t; the stream is the oracle's at q*"""
    D = curve(t, stat); s = trials(name, rd)
    q0, qs, qstar, met = walk(D, qp, floor, lo, hi) if floor else (qp, qp, qp, 1)
    r = res[1]
    assert (r["qp_probe"], r["qp_start"], r["qp"], r["met"]) == (q0, qs, qstar, met), (floor, qp, r, (q0, qs, qstar, met))
    assert 1 <= r["n_encodes"] <= abs(qstar - qs) + 5, (floor, qp, r)
    assert outs[1] == s[qstar][0][1] and outs[0] == s[qstar][0][0] and r["bytes"] == len(outs[1])
    same_frames(r["frames"], t[qstar])
    p = [float(f["psnr"]) for f in r["frames"]]
    assert r["n_frames"] == len(p) and r["min_d1"] == min(p) and r["mean_d1"] == sum(p) / len(p) and r["cloud_ms"] >= 0
    assert (res[0]["qp"], res[0]["bytes"], res[0]["n_frames"], res[0]["frames"]) == (8, len(outs[0]), 0, [])
    return r


# ------------------------------------------------------------------------------------------------ 1, 2: the walk on the synthetic atlas
def check_walk(R, ctx, rd):
    t = table("synth", rd); D = curve(t)
    assert len(set(D.values())) > 8                                                      # the table varies with q
    mid = (D[30] + D[31]) / 2
    cases = [(pick_floor(D, max(D.values()) + 0.5, [30]), 30), (pick_floor(D, min(D.values()) - 0.5, [30]), 30)]
    fm = pick_floor(D, mid, [24, 30, 40])
    cases += [(fm, qp) for qp in (24, 30, 40)]
    seen = set()
    for floor, qp in cases:
        check_margins(D, floor, [qp])
        outs, res = ctx.transcode_gof_d1(case("synth")["src"], params(R, qp, rd), target(R, "synth", floor))
        r = check_result("synth", rd, t, qp, floor, MIN, outs, res)
        seen.add((r["qp"], r["met"]))
    assert (LO, 0) in seen and (HI, 1) in seen


def check_not_monotone(R, ctx):
    """D1 rises from QP 24 to 25 and from 26 to 27: a floor between the values is answered differently from two starting QPs"""
    t = table("synth", 0); D = curve(t)
    got = [round(D[q], 3) for q in (24, 25, 26, 27)]
    assert D[24] < D[25] - 0.002 and D[26] < D[25] - 0.002 and D[26] < D[27] - 0.002, "the oracle's streams no longer hold the inversion at QP 24..27: %r" % got
    assert got == [58.545, 59.295, 58.246, 59.135], got
    floor = pick_floor(D, (max(D[24], D[26]) + min(D[25], D[27])) / 2, [25, 27], LO, 27)
    check_margins(D, floor, [25, 27], LO, 27)
    ends = {}
    for qp in (25, 27):
        outs, res = ctx.transcode_gof_d1(case("synth")["src"], params(R, qp), target(R, "synth", floor, MIN, LO, 27))
        ends[qp] = check_result("synth", 0, t, qp, floor, MIN, outs, res, LO, 27)["qp"]
    assert ends[25] != ends[27], ends


# ------------------------------------------------------------------------------------------------ 3: smoothing, several frames, min against mean
def stat_floor(t, qp=30):
    """one floor for which the walk on the minimum and the walk on the mean end at different QPs, on the oracle's table"""
    Dmin, Dmean = curve(t, MIN), curve(t, MEAN)
    for q in range(LO, HI):
        for D in (Dmin, Dmean):
            try:
                f = pick_floor(D, (D[q] + D[q + 1]) / 2, [qp]); check_margins(Dmin, f, [qp]); check_margins(Dmean, f, [qp])
            except AssertionError:
                continue
            if walk(Dmin, qp, f)[2] != walk(Dmean, qp, f)[2]:
                return f
    raise AssertionError("the oracle's table holds no floor that tells the minimum from the mean")


def check_smoothing_frames(R, ctx):
    ts, tu = table("seam_smooth", 0), table("seam", 0)
    moved = [m for v in trials("seam_smooth", 0).values() for m in v[2]]
    assert min(moved) > 0 and min(input_clouds("seam_smooth")[1]) > 0, (moved, input_clouds("seam_smooth")[1])          # n_smoothed > 0 in every trial and in the references
    assert all(not any(v[2]) for v in trials("seam", 0).values())
    assert all([f["sse_ab"] for f in ts[q]] != [f["sse_ab"] for f in tu[q]] for q in ts)                                  # smoothing changes D1 at every QP
    assert all(ts[q][0]["psnr"] != ts[q][1]["psnr"] for q in ts)                                                          # the two frames differ
    src = case("seam")["src"]
    for name, t in (("seam_smooth", ts), ("seam", tu)):
        outs, res = ctx.transcode_gof_d1(src, params(R, 30), target(R, name))                                             # report only
        check_result(name, 0, t, 30, 0, MIN, outs, res)
    f = stat_floor(ts)
    ends = {}
    for stat in (MIN, MEAN):
        outs, res = ctx.transcode_gof_d1(src, params(R, 30), target(R, "seam_smooth", f, stat))
        ends[stat] = check_result("seam_smooth", 0, ts, 30, f, stat, outs, res)["qp"]
    assert ends[MIN] != ends[MEAN]


# ------------------------------------------------------------------------------------------------ 4: strides and windows
def check_cropped(R, ctx):
    t = table("cropped", 0); D = curve(t)
    assert all(v[0]["n_a"] == t[LO][0]["n_a"] and v[0]["n_b"] == t[LO][0]["n_b"] for v in t.values()) and t[LO][0]["n_a"] != t[LO][0]["n_b"]
    assert (len(input_clouds("cropped")[0][0]), len(trials("cropped", 0)[LO][1][0])) == (814, 912)
    assert 61.7 < min(D.values()) and max(D.values()) < 66.9 and max(D.values()) - min(D.values()) > 3
    src = case("cropped")["src"]
    outs, res = ctx.transcode_gof_d1(src, params(R, 30), target(R, "cropped"))
    check_result("cropped", 0, t, 30, 0, MIN, outs, res)
    f = pick_floor(D, (D[31] + D[32]) / 2, [28])
    outs, res = ctx.transcode_gof_d1(src, params(R, 28), target(R, "cropped", f))
    check_result("cropped", 0, t, 28, f, MIN, outs, res)


# ------------------------------------------------------------------------------------------------ 5: reference handles
def check_reference_handles(R, ctx):
    src = case("synth")["src"]; t = table("synth", 0); D = curve(t)
    f = pick_floor(D, (D[30] + D[31]) / 2, [30])
    want = ctx.transcode_gof_d1(src, params(R, 30), target(R, "synth", f))
    a = ctx.pcloud_upload(input_clouds("synth")[0][0])
    try:
        got = ctx.transcode_gof_d1(src, params(R, 30), target(R, "synth", f, reference=[a]))
        strip = lambda x: (x[0], [{k: v for k, v in r.items() if k != "cloud_ms"} for r in x[1]])
        assert strip(got) == strip(want)
    finally:
        a.release()
    ts = table("synth", 0, "source"); Ds = curve(ts)
    assert all(ts[q][0]["sse_ab"] != t[q][0]["sse_ab"] for q in t)
    fs = pick_floor(Ds, (Ds[30] + Ds[31]) / 2, [30])
    b = ctx.pcloud_upload(source_clouds()[0])
    try:
        outs, res = ctx.transcode_gof_d1(src, params(R, 30), target(R, "synth", fs, reference=[b]))
        check_result("synth", 0, ts, 30, fs, MIN, outs, res)
    finally:
        b.release()


# ------------------------------------------------------------------------------------------------ 6: composition through the public calls (no oracle)
def check_composition(R, ctx, name="seam_smooth"):
    c = case(name); w, h = c["w"], c["h"]
    outs, res = ctx.transcode_gof_d1(c["src"], params(R, 30), target(R, name))
    clouds = []
    for streams, prec in ((c["src"], 2), (outs, 4)):
        om, ow, oh, *_ = ctx.decode(streams[0], verify_md5=False); g, *_ = ctx.decode(streams[1], verify_md5=False)
        a = _copy_atlas(c["atlas"], occupancy_precision=prec)
        clouds.append([ctx.reconstruct(a, c["patches"][f], luma(om[f], ow, oh), luma(g[2 * f], w, h), luma(g[2 * f + 1], w, h), 10)[0] for f in range(c["n_frames"])])
    for f in range(c["n_frames"]):
        assert ctx.d1(clouds[0][f], clouds[1][f]) == res[1]["frames"][f]                 # field for field, floats included: the same routine
        pa, pb = ctx.pcloud_upload(clouds[0][f]), ctx.pcloud_upload(clouds[1][f])
        try:
            assert ctx.score(pa, pb, parts=R.RBT_SCORE_D1)["d1"] == res[1]["frames"][f]
        finally:
            pa.release(); pb.release()


# ------------------------------------------------------------------------------------------------ 7: jobs
def check_jobs(R, ctx):
    c = case("synth"); src = c["src"]; t = table("synth", 0); D = curve(t)
    f = pick_floor(D, (D[30] + D[31]) / 2, [30])
    a = ctx.transcode_gof_d1(src, params(R, 30), target(R, "synth", f))
    b = ctx.wait_gof_d1(ctx.submit_gof_d1(src, params(R, 30), target(R, "synth", f)))
    strip = lambda x: (x[0], [{k: v for k, v in r.items() if k != "cloud_ms"} for r in x[1]])
    assert strip(a) == strip(b)
    check_result("synth", 0, t, 30, f, MIN, *a)
    # a job of rbt_submit_gof_d1 is collected by rbt_wait_gof_d1 only; the refused call leaves the job collectable
    job = ctx.submit_gof_d1(src, params(R, 30), target(R, "synth"))
    for other in (ctx.wait_gof, ctx.wait_gof_rate, ctx.wait_gof_quality):
        with pytest.raises(R.RbtError) as e:
            other(job)
        assert e.value.code == -4
    check_result("synth", 0, t, 30, 0, MIN, *ctx.wait_gof_d1(job))
    for submit, args, collect in ((ctx.submit_gof, (), ctx.wait_gof), (ctx.submit_gof_quality, ([R.QualityTarget(), R.QualityTarget()],), ctx.wait_gof_quality)):
        job = submit(src, params(R, 30), *args)
        with pytest.raises(R.RbtError) as e:
            ctx.wait_gof_d1(job)
        assert e.value.code == -4
        got = collect(job)
        assert (got[0] if args else got)[1] == trials("synth", 0)[30][0][1]
    # a geometry entry with a floor beside an attribute entry at constant QP
    src3 = QC.gof_source(128, 128, 21); p3 = QC.gof_params(R, 30, 0)
    outs, res = ctx.transcode_gof_d1(src3, p3, target(R, "synth", f) + [R.D1Target()])
    check_result("synth", 0, t, 30, f, MIN, outs[:2], res[:2])
    assert outs[2] == ctx.transcode_gof(src3, p3)[2] and (res[2]["qp"], res[2]["bytes"], res[2]["n_encodes"], res[2]["n_frames"]) == (30, len(outs[2]), 1, 0)


def check_jobs_in_flight(R, ctx, depth, n_jobs):
    """n_jobs jobs of the synthetic atlas in flight, every one with a floor of its own, collected out of order, each equal to the lone result"""
    src = case("synth")["src"]; t = table("synth", 0); D = curve(t)
    old = ctx.get_depth(); ctx.set_depth(depth)
    try:
        fs = [pick_floor(D, (D[q] + D[q + 1]) / 2, [30]) for q in [LO + 1 + (5 * k) % (HI - LO - 2) for k in range(n_jobs)]]
        jobs = [ctx.submit_gof_d1(src, params(R, 30), target(R, "synth", f)) for f in fs]
        with pytest.raises(R.RbtError) as e:
            ctx.submit_gof_d1(src, params(R, 30), target(R, "synth", fs[0]))
        assert e.value.code == -7                                                       # RBT_ERR_BUSY: the depth holds for these jobs too
        assert ctx.job_memory(jobs[0]) > 2 * ((1 << 27) + (1 << 18))                    # the reference cloud's volume and the trial's are counted
        for k in list(range(1, n_jobs, 2)) + list(range(0, n_jobs, 2))[::-1]:
            outs, res = ctx.wait_gof_d1(jobs[k])
            check_result("synth", 0, t, 30, fs[k], MIN, outs, res)
    finally:
        ctx.set_depth(old)


# ------------------------------------------------------------------------------------------------ 8: arguments
def check_arguments(R, ctx):
    """every refusal is RBT_ERR_PARAM with its reason, submits nothing and leaves the context usable"""
    c = case("synth"); src = c["src"]; t = table("synth", 0)
    attr = QC.gof_source(128, 128, 21)[2]
    old = ctx.get_depth(); ctx.set_depth(1)        # one slot: a refused submit that kept it would make the next call RBT_ERR_BUSY
    try:
        def refused(streams, ps, ts, word):
            for call in (ctx.transcode_gof_d1, ctx.submit_gof_d1):
                with pytest.raises(R.RbtError) as e:
                    call(streams, ps, ts)
                assert e.value.code == -4 and word in str(e.value), str(e.value)
            outs, res = ctx.transcode_gof_d1(src, params(R, 30), target(R, "synth"))      # ... followed by a call that still works on the same context
            assert outs[1] == trials("synth", 0)[30][0][1] and res[1]["frames"][0]["sse_ab"] == t[30][0]["sse_ab"]
        tg = lambda **kw: target(R, "synth", **kw)
        bad = tg(floor=50000); bad[1].struct_size += 4
        refused(src, params(R, 30), bad, "struct_size")
        refused(src + [attr], QC.gof_params(R, 30, 0), [R.D1Target(), R.D1Target(), tg(floor=50000)[1]], "non-geometry")
        refused(src, params(R, 30), [tg(floor=50000)[1], R.D1Target()], "non-geometry")                       # on the occupancy entry
        for lo, hi in ((-1, 30), (30, 52), (31, 30), (52, 0)):
            refused(src, params(R, 30), tg(floor=50000, lo=lo, hi=hi), "range")
        refused(src, params(R, 30), tg(floor=50000, stat=2), "stat")
        refused(src, params(R, 30), tg(floor=-1), "negative")
        none = tg(floor=50000); none[1].n_frames = 0
        refused(src, params(R, 30), none, "n_frames")
        refused(src[1:], params(R, 30)[1:], tg(floor=50000)[1:], "occupancy source")                          # no occupancy entry in front
        refused(src[::-1], params(R, 30)[::-1], tg(floor=50000)[::-1], "occupancy source")                    # ... it is behind
        P2 = R.StreamParams(0, 8, 2, 5, -1, 0, 0, 0, 0)                                                       # passed through, not pooled
        refused(src, [P2, params(R, 30)[1]], tg(floor=50000), "occupancy source")
        refused(src, params(R, 30), tg(atlas=_copy_atlas(c["atlas"], width=256)), "atlas.width")
        refused(src, params(R, 30), tg(atlas=_copy_atlas(c["atlas"], map_count=1)), "map_count")
        refused(src, params(R, 30), tg(atlas=_copy_atlas(c["atlas"], occupancy_precision=2)), "occupancy_precision")
        two = R.D1Target(c["atlas"], c["patches"] * 2, 50000, MIN, LO, HI)
        refused(src, params(R, 30), [R.D1Target(), two], "n_frames")
        refused(src, params(R, 30), tg(atlas=_copy_atlas(c["atlas"], geometry_smoothing=1, grid_size=7, threshold_smoothing=64)), "grid_size")
        other = R.Context(lib_path=ctx.lib_path)
        try:
            h = other.pcloud_upload(input_clouds("synth")[0][0])
            refused(src, params(R, 30), tg(floor=50000, reference=[h]), "not a cloud of this context")
            h.release()
        finally:
            other.close()
        rd = [params(R, 30)[0], QC.params(R, "geo", 30, occupancy_rd=1, verify_md5=1)]
        refused(src, rd, tg(floor=50000), "verify_md5")
        # an empty cloud is found when the cloud is built: the job fails cleanly in its wait call and the context goes on
        empty = R.D1Target(c["atlas"], [[]], 50000, MIN, LO, HI)
        with pytest.raises(R.RbtError) as e:
            ctx.transcode_gof_d1(src, params(R, 30), [R.D1Target(), empty])
        assert e.value.code == -4 and "empty point cloud" in str(e.value)
        far = [R.Patch(*[getattr(p, n) for n, _ in R.Patch._fields_]) for p in c["patches"][0]]
        far[0].u1 = 1000
        with pytest.raises(R.RbtError) as e:
            ctx.transcode_gof_d1(src, params(R, 30), [R.D1Target(), R.D1Target(c["atlas"], [far], 50000, MIN, LO, HI)])
        assert e.value.code == -4 and "outside 0..1023" in str(e.value)
        assert ctx.transcode_gof(src, params(R, 33))[1] == trials("synth", 0)[33][0][1]
    finally:
        ctx.set_depth(old)


# ------------------------------------------------------------------------------------------------ 9: the gather kernel on its own
GATHER_WIDTHS = (2, 8, 14, 72, 264)


def check_gather(ctx, w, n_pics, other=None):
    """GPU == serial host emulation == NumPy slicing: source rows at every misalignment of 0..7 samples against the destination, a window offset in both directions"""
    h, stride, rows = 5, w + 19, 9
    r = np.random.default_rng(w * 31 + n_pics)
    src = r.integers(0, 1 << 16, (n_pics, rows, stride)).astype(np.uint16)
    for mis in range(8):
        for x0, y0 in ((0, 0), (3, 2), (stride - w, rows - h), (8, 1)):
            want = src[:, y0:y0 + h, x0:x0 + w]
            got = ctx.gather_luma(src, x0, y0, w, h, mis)
            assert np.array_equal(got, want), (w, n_pics, mis, x0, y0)
            if other is not None:
                assert np.array_equal(other.gather_luma(src, x0, y0, w, h, mis), got)


def check_gather_arguments(R, ctx):
    src = np.zeros((1, 4, 8), np.uint16)
    for x0, y0, w, h, mis in ((1, 0, 8, 4, 0), (0, 1, 8, 4, 0), (0, 0, 0, 4, 0), (0, 0, 8, 4, 8), (-1, 0, 4, 4, 0)):
        with pytest.raises(R.RbtError) as e:
            ctx.gather_luma(src, x0, y0, w, h, mis)
        assert e.value.code == -4
    assert np.array_equal(ctx.gather_luma(src + 7, 0, 0, 8, 4), src + 7)


# ------------------------------------------------------------------------------------------------ 10: determinism
def check_determinism(R, ctx):
    src = case("seam_smooth")["src"]; D = curve(table("seam_smooth", 0), MEAN)
    f = pick_floor(D, (D[29] + D[30]) / 2, [27])
    strip = lambda x: (x[0], [{k: v for k, v in r.items() if k != "cloud_ms"} for r in x[1]])
    a = ctx.transcode_gof_d1(src, params(R, 27, 1), target(R, "seam_smooth", f, MEAN))
    b = ctx.transcode_gof_d1(src, params(R, 27, 1), target(R, "seam_smooth", f, MEAN))
    assert strip(a) == strip(b) and a[1][1]["n_frames"] == 2
