"""Transcoding to a PSNR floor (include/rbt.h: rbt_picture_sse, rbt_submit_gof_quality / rbt_wait_gof_quality, rbt_transcode_v3c_quality): one set of cases for the host
emulation (tests/test_quality.py) and the GPU (tests/test_gpu_quality.py).
  sums      a NumPy restatement of the definition on synthetic pictures and maps; exact equality of all nine words per picture
  report    floor 0: the oracle's constant-QP stream, and the sums of O.decode(input) against O.decode(output)
  walk      d(q) from the oracle's streams for q = 18..45 (the tables of tests/rate_cases.py, shared); the definition's walk; the stream must be the oracle's at q*
Everything the oracle computes is cached in this module, so the host and the GPU tests of one run share it."""
import functools
import math
import numpy as np
import pytest
import oracle_lib as O
import synth
from rate_cases import source, table, KINDS, STREAMS, Q_LO, Q_HI, v3c_file

ALL, OCCUPIED = 0, 1


# ------------------------------------------------------------------------------------------------ sums
def planes(frame, w, h):
    ys, cs = w * h, (w // 2) * (h // 2)
    return [frame[:ys].reshape(h, w), frame[ys:ys + cs].reshape(h // 2, w // 2), frame[ys + cs:ys + 2 * cs].reshape(h // 2, w // 2)]


def np_sse(a, b, w, h, occ=None):
    """uint64 [n, 3, 3]: per picture and plane sse, sse_occ, n_occ by the definition: one line per rule"""
    a = np.asarray(a).reshape(-1, w * h * 3 // 2); b = np.asarray(b).reshape(-1, w * h * 3 // 2)
    out = np.zeros((a.shape[0], 3, 3), np.uint64)
    for k in range(a.shape[0]):
        luma = None
        if occ is not None:
            oh, ow = occ[k].shape
            s = w // ow
            assert s >= 1 and s * ow == w and s * oh == h
            luma = np.repeat(np.repeat(occ[k] > 0, s, 0), s, 1)                 # luma sample (x, y): O[y / s][x / s] > 0
        for c, (pa, pb) in enumerate(zip(planes(a[k], w, h), planes(b[k], w, h))):
            d2 = (pa.astype(np.int64) - pb.astype(np.int64)) ** 2
            out[k, c, 0] = int(d2.sum())
            if luma is not None:
                m = luma if c == 0 else luma[::2, ::2]                             # chroma sample (x, y): luma sample (2x, 2y)
                out[k, c, 1] = int(d2[m].sum()); out[k, c, 2] = int(m.sum())
    return out


def _pictures(w, h, n, seed, bd=10, noise=12):
    r = np.random.default_rng(seed)
    a = r.integers(0, 1 << bd, (n, w * h * 3 // 2)).astype(np.uint16)
    b = np.clip(a.astype(np.int64) + r.integers(-noise, noise + 1, a.shape), 0, (1 << bd) - 1).astype(np.uint16)
    return a, b


def _map(kind, w, h, s, n=1, seed=0):
    ow, oh = w // s, h // s
    if kind == "zero":
        m = np.zeros((n, oh, ow), np.uint16)
    elif kind == "set":
        m = np.full((n, oh, ow), 1, np.uint16)
    elif kind == "checker":
        yy, xx = np.mgrid[0:oh, 0:ow]
        m = np.broadcast_to(((yy + xx) & 1).astype(np.uint16) * 255, (n, oh, ow)).copy()
    elif kind == "last":
        m = np.zeros((n, oh, ow), np.uint16); m[:, -1, -1] = 1
    else:
        m = (np.random.default_rng(seed).random((n, oh, ow)) < 0.4).astype(np.uint16) * 3
    return m


def _case_sizes(w, h, s, n=1):
    a, b = _pictures(w, h, n, w * 7 + h)
    return a, b, w, h, _map("random", w, h, s, n, seed=w + h + n)


def _case_one_sample(c, last):
    w, h = 130, 66
    a, _ = _pictures(w, h, 1, 77)
    b = a.copy()
    ys, cs = w * h, (w // 2) * (h // 2)
    first = [0, ys, ys + cs][c]; size = [ys, cs, cs][c]
    at = first + (size - 1 if last else 0)
    b[0, at] = a[0, at] ^ 5
    return a, b, w, h, _map("set", w, h, 2)


def _case_extremes(bd):
    w, h = 264, 136
    a = np.zeros((1, w * h * 3 // 2), np.uint16); b = np.full_like(a, (1 << bd) - 1)
    return a, b, w, h, _map("set", w, h, 4)


def _case_map(kind, s):
    a, b = _pictures(72, 40, 1, 5 + s)
    return a, b, 72, 40, _map(kind, 72, 40, s)


SSE_CASES = {
    "8x8": lambda: _case_sizes(8, 8, 1),
    "16x8": lambda: _case_sizes(16, 8, 2),
    "72x40": lambda: _case_sizes(72, 40, 4),
    "130x66": lambda: _case_sizes(130, 66, 2),               # chroma 65x33: rows that are only 2-byte aligned
    "130x66_no_map": lambda: _case_sizes(130, 66, 1)[:4] + (None,),
    "264x136": lambda: _case_sizes(264, 136, 4),             # several workgroups add into one counter
    "72x40_3_frames": lambda: _case_sizes(72, 40, 2, n=3),
    "identical": lambda: (lambda a: (a, a.copy(), 130, 66, _map("checker", 130, 66, 1, n=2)))(_pictures(130, 66, 2, 3)[0]),
    "extremes_10_bits": lambda: _case_extremes(10),
    "extremes_8_bits": lambda: _case_extremes(8),
}
for _c, _n in enumerate(("y", "cb", "cr")):
    SSE_CASES["first_sample_" + _n] = functools.partial(_case_one_sample, _c, False)
    SSE_CASES["last_sample_" + _n] = functools.partial(_case_one_sample, _c, True)
for _s in (1, 2, 4):
    for _k in ("zero", "set", "checker", "last"):
        SSE_CASES["map_%s_scale_%d" % (_k, _s)] = functools.partial(_case_map, _k, _s)


@functools.lru_cache(maxsize=None)
def sse_case(name):
    a, b, w, h, occ = SSE_CASES[name]()
    return (a, b, w, h, occ), np_sse(a, b, w, h, occ)


def check_sse(ctx, name, other=None):
    """the library's nine words per picture equal the definition's (and `other`, a second context's - the host emulation's next to the GPU's)"""
    (a, b, w, h, occ), want = sse_case(name)
    got = ctx.picture_sse(a, b, w, h, occ)
    assert got.dtype == np.uint64 and np.array_equal(got, want), (name, got, want)
    if name == "identical":
        assert not got[:, :, :2].any() and got[:, 0, 2].all()
    if name.startswith(("first_sample", "last_sample")):
        assert int((got[0, :, 0] > 0).sum()) == 1
    if name.startswith("extremes"):
        peak = 1023 if name.endswith("10_bits") else 255
        assert int(got[0, 0, 0]) == 35904 * peak * peak and (peak == 255 or int(got[0, 0, 0]) > 1 << 32)
        assert np.array_equal(got[0, :, 0], got[0, :, 1]) and list(got[0, :, 2]) == [35904, 8976, 8976]
    if name.startswith("map_zero"):
        assert not got[:, :, 1:].any()
    if name.startswith("map_last"):
        s = int(name[-1])
        assert list(got[0, :, 2]) == [s * s, (s // 2) ** 2, (s // 2) ** 2]      # chroma sample (x, y) goes by luma sample (2x, 2y): none at scale 1
    if other is not None:
        assert np.array_equal(other.picture_sse(a, b, w, h, occ), got)


def check_sse_arguments(R, ctx):
    a, b = _pictures(72, 40, 1, 1)
    for w, h, occ in ((72, 40, np.ones((1, 20, 50), np.uint16)), (72, 40, np.ones((1, 20, 18), np.uint16)), (72, 40, np.ones((1, 16, 36), np.uint16))):
        with pytest.raises(R.RbtError) as e:      # 72 / 50 is not whole; 4 across and 2 down; 40 / 16 is not whole
            ctx.picture_sse(a, b, w, h, occ)
        assert e.value.code == -4 and "scale" in str(e.value)
    odd = np.zeros((1, 9 * 8 * 3 // 2), np.uint16)
    with pytest.raises(R.RbtError) as e:
        ctx.picture_sse(odd, odd, 9, 8)
    assert e.value.code == -4
    with pytest.raises(R.RbtError) as e:
        ctx.picture_sse(np.zeros((1, 8194 * 2 * 3 // 2), np.uint16), np.zeros((1, 8194 * 2 * 3 // 2), np.uint16), 8194, 2)
    assert e.value.code == -4
    assert np.array_equal(ctx.picture_sse(a, b, 72, 40), np_sse(a, b, 72, 40))


# ------------------------------------------------------------------------------------------------ PSNR, the floor and the walk, by the definitions
def psnr(sse, samples, bd=10):
    if samples == 0:
        return 0.0
    if sse == 0:
        return math.inf
    peak = float((1 << bd) - 1)
    return 10.0 * math.log10(peak * peak * float(samples) / float(sse))


def meets(sse, samples, floor_mdb, bd=10):
    return samples == 0 or sse == 0 or psnr(sse, samples, bd) >= floor_mdb / 1000.0


def walk(d, qp, floor_mdb, lo, hi, bd=10):
    """d: q -> (sse, samples) of plane 0 of the chosen region -> (q0, qs, q*, met)"""
    F = floor_mdb / 1000.0
    ok = lambda q: meets(d[q][0], d[q][1], floor_mdb, bd)
    q0 = min(hi, max(lo, qp))
    p0 = psnr(d[q0][0], d[q0][1], bd)
    qs = q0 if math.isinf(p0) else min(hi, max(lo, q0 + int(p0 - F)))
    q = qs
    if ok(q):
        while q < hi and ok(q + 1):
            q += 1
        return q0, qs, q, 1
    while q > lo and not ok(q):
        q -= 1
    return q0, qs, q, int(ok(q))


def params(R, kind, qp=30, occupancy_rd=0, verify_md5=0):
    return R.StreamParams(KINDS[kind][0], qp, 4, 5, -1, 0, verify_md5, occupancy_rd, 0)


@functools.lru_cache(maxsize=None)
def decoded(w, h, seed, kind):
    return O.decode(source(w, h, seed, kind))


@functools.lru_cache(maxsize=None)
def dist(w, h, seed, kind):
    """q -> uint64 [3, 3]: the sums of the oracle's stream at q against the decoded input, over the pictures of the stream"""
    a, dw, dh, bd, _, _ = decoded(w, h, seed, kind)
    assert (dw, dh, bd) == (w, h, 10)
    out = {}
    for q, s in table(w, h, seed, kind).items():
        b, bw, bh, _, _, _ = O.decode(s)
        assert (bw, bh) == (w, h)
        out[q] = np_sse(a, b, w, h).sum(axis=0)
    return out


def luma(d, n_samples):
    return {q: (int(v[0, 0]), n_samples) for q, v in d.items()}


def pick_floor(d, near_db, qp_list, lo=Q_LO, hi=Q_HI):
    """a floor in 1/1000 dB at or just above near_db that is at least 0.001 dB away from every d(q) and leaves psnr(q0) - F at least 0.001 away from a whole number for
    every params.qp of qp_list: then no rounding of log10 can change an answer"""
    f = int(round(near_db * 1000))
    for _ in range(1000):
        F = f / 1000.0
        ps = [psnr(*d[q]) for q in d]
        fr = [abs((psnr(*d[min(hi, max(lo, qp))]) - F) - round(psnr(*d[min(hi, max(lo, qp))]) - F)) for qp in qp_list]
        if all(abs(p - F) >= 0.001 for p in ps) and all(x >= 0.001 for x in fr):
            return f
        f += 3
    raise AssertionError("no floor with the margins near %r" % near_db)


def check_margins(d, floor_mdb, qp_list, lo, hi):
    F = floor_mdb / 1000.0
    assert all(abs(psnr(*d[q]) - F) >= 0.001 for q in d), floor_mdb
    for qp in qp_list:
        x = psnr(*d[min(hi, max(lo, qp))]) - F
        assert abs(x - round(x)) >= 0.001, (floor_mdb, qp)


def check_result(R, d, s, qp, floor_mdb, lo, hi, out, res, sums=None, region=ALL):
    """res against the definition's walk on d (plane 0 of the region); s: q -> the oracle's stream; sums: q -> [3, 3] of the whole stream"""
    q0, qs, qstar, met = walk(d, qp, floor_mdb, lo, hi)
    assert (res["qp_probe"], res["qp_start"]) == (q0, qs), (floor_mdb, qp, lo, hi, res)
    assert (res["qp"], res["met"], res["bytes"]) == (qstar, met, len(s[qstar])), (floor_mdb, qp, lo, hi, res, qstar)
    assert 1 <= res["n_encodes"] <= abs(qstar - qs) + 5, (floor_mdb, qp, lo, hi, res)
    assert out == s[qstar], (floor_mdb, qp, lo, hi, res)
    key = "sse_occ" if region == OCCUPIED else "sse"
    assert (res[key][0], res["samples_occ" if region == OCCUPIED else "samples"][0]) == d[qstar]
    assert met == int(meets(d[qstar][0], d[qstar][1], floor_mdb))
    if sums is not None:
        assert res["sse"] == [int(sums[qstar][c, 0]) for c in range(3)]
        got = res["psnr"][0]; want = psnr(res["sse"][0], res["samples"][0])
        assert got == want or abs(got - want) < 1e-9


def check_report(R, ctx, w, h, seed, kind):
    """floor 0 at QP 30: the oracle's stream, and the sums of the displayed pictures against NumPy's for all three planes"""
    src = source(w, h, seed, kind); s = table(w, h, seed, kind); d = dist(w, h, seed, kind)
    outs, res = ctx.transcode_gof_quality([src], [params(R, kind)], [R.QualityTarget()])
    r = res[0]
    assert outs[0] == s[30] and (r["qp"], r["qp_probe"], r["qp_start"], r["met"], r["n_encodes"], r["bytes"]) == (30, 30, 30, 1, 1, len(s[30]))
    assert r["sse"] == [int(d[30][c, 0]) for c in range(3)] and r["samples"] == [2 * w * h, w * h // 2, w * h // 2]
    assert r["sse_occ"] == [0, 0, 0] and r["samples_occ"] == [0, 0, 0] and r["psnr_occ"] == [0.0, 0.0, 0.0]
    for c in range(3):
        want = psnr(r["sse"][c], r["samples"][c])                      # (+inf for the flat chroma planes of a geometry stream that come back exactly)
        assert r["psnr"][c] == want or abs(r["psnr"][c] - want) < 1e-9


@functools.lru_cache(maxsize=None)
def cropped_stream():
    """a 72x40 geometry stream cut out of the 128x128 maps: coded padded (80x48 for the gop-2 output), so the compared area must be the displayed one"""
    w, h = 72, 40
    big = synth.make_maps(128, 128, 21)["geo"]
    fr = np.stack([np.concatenate([p[:hh, :ww].ravel() for p, (ww, hh) in zip(planes(f, 128, 128), ((w, h), (w // 2, h // 2), (w // 2, h // 2)))]) for f in big])
    return O.encode_hm(fr, w, h, 10, 16)[0]


def check_report_cropped(R, ctx):
    w, h = 72, 40
    src = cropped_stream()
    want = O.transcode_substream(src, 1, 30, log2_ctb=5, rows_per_slice=-1, md5_sei=0, preset=0)
    a, aw, ah, _, _, _ = O.decode(src); b, bw, bh, _, _, _ = O.decode(want)
    assert (aw, ah, bw, bh) == (w, h, w, h)
    outs, res = ctx.transcode_gof_quality([src], [params(R, "geo")], [R.QualityTarget()])
    sums = np_sse(a, b, w, h).sum(axis=0)
    assert outs[0] == want and res[0]["sse"] == [int(sums[c, 0]) for c in range(3)] and res[0]["samples"] == [2 * w * h, w * h // 2, w * h // 2]
    assert res[0]["sse"][0] > 0


def walk_cases(d):
    """(floor, params.qp, lo, hi) on the luma table d: a floor above every d(q) (q* = lo, met 0), one below every d(q) (q* = hi), the midpoint between d(30) and d(31)
    started from 20, 30 and 44 - the jump in both directions -, and a narrow range whose lower end misses"""
    p = {q: psnr(*d[q]) for q in d}
    mid = (p[30] + p[31]) / 2
    cases = [(pick_floor(d, max(p.values()) + 0.5, [30]), 30, Q_LO, Q_HI), (pick_floor(d, min(p.values()) - 0.5, [30]), 30, Q_LO, Q_HI)]
    fm = pick_floor(d, mid, [20, 30, 44])
    cases += [(fm, qp, Q_LO, Q_HI) for qp in (20, 30, 44)]
    cases.append((pick_floor(d, max(p[q] for q in range(32, 37)) + 0.25, [30], 32, 36), 30, 32, 36))
    return cases


def check_walk(R, ctx, w, h, seed, kind):
    src = source(w, h, seed, kind); s = table(w, h, seed, kind); sums = dist(w, h, seed, kind); d = luma(sums, 2 * w * h)
    p = [psnr(*d[q]) for q in range(Q_LO, Q_HI + 1)]
    assert min(abs(x - y) for x, y in zip(p, p[1:])) >= 0.001
    seen = set()
    for floor, qp, lo, hi in walk_cases(d):
        check_margins(d, floor, [qp], lo, hi)
        outs, res = ctx.transcode_gof_quality([src], [params(R, kind, qp)], [R.QualityTarget(floor, ALL, lo, hi)])
        check_result(R, d, s, qp, floor, lo, hi, outs[0], res[0], sums)
        seen.add((res[0]["qp"], res[0]["met"]))
    assert (Q_LO, 0) in seen and (Q_HI, 1) in seen and (32, 0) in seen


def check_not_monotone(R, ctx):
    """64x64 geometry: the luma PSNR rises from QP 35 to 36, so the walk's answer depends on where it starts"""
    key = (64, 64, 5, "geo")
    src = source(*key); s = table(*key); sums = dist(*key); d = luma(sums, 2 * 64 * 64)
    p = {q: psnr(*d[q]) for q in d}
    assert p[34] > 41.150 + 0.001 and p[35] < 41.150 - 0.001 and p[36] > 41.150 + 0.001 and p[37] < 41.150 - 0.001, "the oracle's streams no longer hold the inversion at QP 35 / 36: %r" % [p[q] for q in (34, 35, 36, 37)]
    assert [round(p[q], 3) for q in (34, 35, 36, 37)] == [41.737, 41.116, 41.186, 39.719]
    check_margins(d, 41150, [34, 35, 36], Q_LO, Q_HI)
    got = {}
    for qp in (34, 35, 36):
        outs, res = ctx.transcode_gof_quality([src], [params(R, "geo", qp)], [R.QualityTarget(41150, ALL, Q_LO, Q_HI)])
        check_result(R, d, s, qp, 41150, Q_LO, Q_HI, outs[0], res[0], sums)
        got[qp] = res[0]["qp"]
    assert got == {34: 34, 35: 34, 36: 36}


# ------------------------------------------------------------------------------------------------ occupancy
OQ_LO, OQ_HI = 24, 40
OCC_P = (0, 8, 4, 5, -1, 0, 0, 0)


@functools.lru_cache(maxsize=None)
def gof_source(w, h, seed):
    occ = O.encode(synth.make_maps(w, h, seed)["occ"], w // 2, h // 2, 8, 8, gop=1, i_qp_offset=0, lossless=1, log2_ctb=5, rows_per_slice=0)[0]
    return [occ, source(w, h, seed, "geo"), source(w, h, seed, "attr")]


@functools.lru_cache(maxsize=None)
def gof_table(w, h, seed, rd):
    """q -> (the oracle's [occ, geo, attr] at QP q for both, with or without occupancy_rd; uint64 [2, 3, 3]: the sums of geo and attr with the pooled output map)"""
    src = gof_source(w, h, seed)
    dec = [O.decode(x)[0] for x in src[1:]]
    out = {}
    for q in range(OQ_LO, OQ_HI + 1):
        o = O.transcode_data(src, [OCC_P, (1, q, 4, 5, -1, 0, rd, 0), (19, q, 4, 5, -1, 0, rd, 0)])
        om, ow, oh, _, _, _ = O.decode(o[0])
        assert (ow, oh) == (w // 4, h // 4) and om.shape[0] == 1
        m = om[:, :ow * oh].reshape(1, oh, ow)
        sums = []
        for k in (1, 2):
            b = O.decode(o[k])[0]
            sums.append(np_sse(dec[k - 1], b, w, h, np.repeat(m, b.shape[0], 0)).sum(axis=0))
        out[q] = (o, np.stack(sums))
    return out


def region_table(t, k, region):
    """plane 0 of entry k (1 geo, 2 attr) of a gof_table: q -> (sse, samples)"""
    return {q: (int(v[1][k - 1][0, 1]), int(v[1][k - 1][0, 2])) if region == OCCUPIED else (int(v[1][k - 1][0, 0]), None) for q, v in t.items()}


def gof_params(R, qp, rd):
    return [R.StreamParams(*OCC_P, 0), params(R, "geo", qp, rd), params(R, "attr", qp, rd)]


def occupied_floor(t, k, n_all, qp=32):
    """a floor (midpoint between neighbouring occupied PSNRs) for which the occupied walk and the all-samples walk end at different QPs, on the oracle's tables"""
    d_occ = region_table(t, k, OCCUPIED); d_all = {q: (v[0], n_all) for q, v in region_table(t, k, ALL).items()}
    for q in range(OQ_LO + 2, OQ_HI - 2):
        f = pick_floor(d_occ, (psnr(*d_occ[q]) + psnr(*d_occ[q + 1])) / 2, [qp], OQ_LO, OQ_HI)
        try:
            check_margins(d_all, f, [qp], OQ_LO, OQ_HI)
        except AssertionError:
            continue
        if walk(d_occ, qp, f, OQ_LO, OQ_HI)[2] != walk(d_all, qp, f, OQ_LO, OQ_HI)[2]:
            return f, d_occ, d_all
    raise AssertionError("the oracle's tables hold no floor that tells the occupied samples from all samples")


def check_occupancy(R, ctx, rd):
    """[occ, geo, attr] at 128x128 with RBT_QUALITY_OCCUPIED: sse_occ and samples_occ on the pooled output map, q* by the occupied figure - which differs from the
    all-samples answer"""
    w, h, seed = 128, 128, 21
    src = gof_source(w, h, seed); t = gof_table(w, h, seed, rd)
    for k in (1, 2):
        streams = {q: v[0][k] for q, v in t.items()}
        f, d_occ, d_all = occupied_floor(t, k, 2 * w * h)
        assert all(0 < d_occ[q][1] < 2 * w * h for q in d_occ)
        tg = [R.QualityTarget(), R.QualityTarget(), R.QualityTarget()]
        tg[k] = R.QualityTarget(f, OCCUPIED, OQ_LO, OQ_HI)
        calls = (ctx.transcode_gof_quality(src, gof_params(R, 32, rd), tg), ctx.wait_gof_quality(ctx.submit_gof_quality(src, gof_params(R, 32, rd), tg)))
        for outs, res in calls:
            check_result(R, d_occ, streams, 32, f, OQ_LO, OQ_HI, outs[k], res[k], region=OCCUPIED)
            q = res[k]["qp"]
            assert res[k]["sse"] == [int(t[q][1][k - 1][c, 0]) for c in range(3)] and res[k]["sse_occ"] == [int(t[q][1][k - 1][c, 1]) for c in range(3)]
            assert res[k]["samples_occ"] == [int(t[q][1][k - 1][c, 2]) for c in range(3)]
            o = 3 - k                                                               # the other entry: constant QP 32, its occupied sums reported all the same
            assert outs[o] == t[32][0][o] and outs[0] == t[32][0][0]
            assert res[o]["sse_occ"] == [int(t[32][1][o - 1][c, 1]) for c in range(3)] and res[o]["samples_occ"][0] == d_occ[32][1]
            assert (res[0]["qp"], res[0]["bytes"], res[0]["sse"], res[0]["samples"]) == (8, len(outs[0]), [0, 0, 0], [0, 0, 0])
        tg[k] = R.QualityTarget(f, ALL, OQ_LO, OQ_HI)
        outs, res = ctx.transcode_gof_quality(src, gof_params(R, 32, rd), tg)
        check_result(R, d_all, streams, 32, f, OQ_LO, OQ_HI, outs[k], res[k], region=ALL)
        assert res[k]["qp"] != calls[0][1][k]["qp"]


# ------------------------------------------------------------------------------------------------ jobs
def check_jobs(R, ctx):
    """the two halves against the blocking call; one input at two floors and a constant QP; wrong pairings of the halves"""
    key = (64, 64, 5, "geo")
    src = source(*key); s = table(*key); sums = dist(*key); d = luma(sums, 2 * 64 * 64)
    p = {q: psnr(*d[q]) for q in d}
    f1 = pick_floor(d, (p[24] + p[25]) / 2, [30]); f2 = pick_floor(d, (p[38] + p[39]) / 2, [30])
    P = [params(R, "geo"), params(R, "geo", 22), params(R, "geo")]
    T = [R.QualityTarget(f1, ALL, Q_LO, Q_HI), R.QualityTarget(), R.QualityTarget(f2, ALL, Q_LO, Q_HI)]
    a = ctx.transcode_gof_quality([src, src, src], P, T)
    b = ctx.wait_gof_quality(ctx.submit_gof_quality([src, src, src], P, T))
    assert a == b
    outs, res = a
    check_result(R, d, s, 30, f1, Q_LO, Q_HI, outs[0], res[0], sums); check_result(R, d, s, 30, f2, Q_LO, Q_HI, outs[2], res[2], sums)
    assert outs[1] == s[22] and res[1]["sse"] == [int(sums[22][c, 0]) for c in range(3)] and res[1]["n_encodes"] == 1
    # a job of rbt_submit_gof_quality is collected by rbt_wait_gof_quality only; the refused call leaves the job collectable
    job = ctx.submit_gof_quality([src], [params(R, "geo")], [R.QualityTarget()])
    for other in (ctx.wait_gof, ctx.wait_gof_rate):
        with pytest.raises(R.RbtError) as e:
            other(job)
        assert e.value.code == -4
    assert ctx.wait_gof_quality(job)[0][0] == s[30]
    job = ctx.submit_gof([src], [params(R, "geo")])
    with pytest.raises(R.RbtError) as e:
        ctx.wait_gof_quality(job)
    assert e.value.code == -4
    assert ctx.wait_gof(job) == [s[30]]


def check_jobs_in_flight(R, ctx, depth, n_jobs):
    """n_jobs jobs in flight at the given depth, collected out of order; every job has a floor of its own"""
    old = ctx.get_depth()
    ctx.set_depth(depth)
    try:
        key = (64, 64, 5, "geo") if n_jobs > 4 else (128, 128, 21, "attr")
        src = source(*key); s = table(*key); sums = dist(*key); d = luma(sums, 2 * key[0] * key[1])
        p = {q: psnr(*d[q]) for q in d}
        fs = [pick_floor(d, (p[q] + p[q + 1]) / 2, [30]) for q in [Q_LO + 1 + (5 * k) % (Q_HI - Q_LO - 2) for k in range(n_jobs)]]
        jobs = [ctx.submit_gof_quality([src], [params(R, key[3])], [R.QualityTarget(f, ALL, Q_LO, Q_HI)]) for f in fs]
        with pytest.raises(R.RbtError) as e:
            ctx.submit_gof_quality([src], [params(R, key[3])], [R.QualityTarget(fs[0], ALL, Q_LO, Q_HI)])
        assert e.value.code == -7         # RBT_ERR_BUSY: the depth holds for these jobs too
        assert ctx.job_memory(jobs[0]) > 0
        order = list(range(1, n_jobs, 2)) + list(range(0, n_jobs, 2))[::-1]
        for k in order:
            outs, res = ctx.wait_gof_quality(jobs[k])
            check_result(R, d, s, 30, fs[k], Q_LO, Q_HI, outs[0], res[0], sums)
    finally:
        ctx.set_depth(old)


def check_shared_pipelines(R, ctx, depth=1):
    """six streams, two GOFs of different sizes: the pipelines are shared by video type, every entry is coded with and measured on ITS GOF's occupancy map"""
    gofs = [(128, 128, 21), (64, 64, 5)]
    src, P, T, want = [], [], [], []
    for w, h, seed in gofs:
        t = gof_table(w, h, seed, 1)
        src += gof_source(w, h, seed); P += gof_params(R, 32, 1)
        T.append(R.QualityTarget()); want.append(None)
        for k in (1, 2):
            f, d_occ, _ = occupied_floor(t, k, 2 * w * h)
            T.append(R.QualityTarget(f, OCCUPIED, OQ_LO, OQ_HI)); want.append((d_occ, {q: v[0][k] for q, v in t.items()}, f, t))
    old = ctx.get_depth(); ctx.set_depth(depth)
    try:
        jobs = [ctx.submit_gof_quality(src, P, T) for _ in range(depth)]
        for job in jobs[::-1]:
            outs, res = ctx.wait_gof_quality(job)
            for i, wn in enumerate(want):
                if wn is None:
                    assert outs[i] == gof_table(*gofs[i // 3], 1)[32][0][0]
                    continue
                d_occ, streams, f, t = wn
                check_result(R, d_occ, streams, 32, f, OQ_LO, OQ_HI, outs[i], res[i], region=OCCUPIED)
                assert res[i]["sse"] == [int(t[res[i]["qp"]][1][i % 3 - 1][c, 0]) for c in range(3)]
    finally:
        ctx.set_depth(old)


def check_verify_md5(R, ctx):
    """verify_md5 on an entry with a floor: the input's hashes are checked behind the decoder's last filter; a wrong one fails the job, no output"""
    import picture_hash_cases as H
    key = (64, 64, 5, "geo")
    src = source(*key); s = table(*key); sums = dist(*key); d = luma(sums, 2 * 64 * 64)
    frames, w, h, bd, _, _ = decoded(*key)
    f = pick_floor(d, (psnr(*d[27]) + psnr(*d[28])) / 2, [30])
    tg = [R.QualityTarget(f, ALL, Q_LO, Q_HI)]
    outs, res = ctx.transcode_gof_quality([src], [params(R, "geo", verify_md5=1)], tg)
    check_result(R, d, s, 30, f, Q_LO, Q_HI, outs[0], res[0], sums)
    bad = H.rewritten(src, frames, w, h, bd, H.MD5, flip=1)
    with pytest.raises(R.RbtError) as e:
        ctx.transcode_gof_quality([bad], [params(R, "geo", verify_md5=1)], tg)
    assert e.value.code == H.RBT_ERR_MD5 and "input 0" in str(e.value)
    assert ctx.transcode_gof_quality([bad], [params(R, "geo")], tg)[0][0] == outs[0]      # unchecked, the same pictures give the same stream


def check_arguments(R, ctx):
    """every refusal is RBT_ERR_PARAM with its reason, submits nothing and leaves the context usable"""
    geo = source(64, 64, 5, "geo"); s = table(64, 64, 5, "geo")
    occ = gof_source(64, 64, 5)[0]
    PO = R.StreamParams(*OCC_P, 0)
    old = ctx.get_depth(); ctx.set_depth(1)        # one slot: a refused submit that kept it would make the next call RBT_ERR_BUSY
    try:
        def refused(streams, ps, ts, word):
            for call in (ctx.transcode_gof_quality, ctx.submit_gof_quality):
                with pytest.raises(R.RbtError) as e:
                    call(streams, ps, ts)
                assert e.value.code == -4 and word in str(e.value), str(e.value)
        bad = R.QualityTarget(40000); bad.struct_size += 4
        refused([geo], [params(R, "geo")], [bad], "struct_size")
        unset = R.QualityTarget(); unset.struct_size = 0
        refused([geo], [params(R, "geo")], [unset], "struct_size")
        for lo, hi in ((-1, 30), (30, 52), (31, 30), (52, 0)):
            refused([geo], [params(R, "geo")], [R.QualityTarget(40000, ALL, lo, hi)], "range")
        refused([geo], [params(R, "geo")], [R.QualityTarget(40000, 2)], "region")
        refused([geo], [params(R, "geo")], [R.QualityTarget(-1)], "negative")
        refused([occ], [PO], [R.QualityTarget(40000)], "occupancy")
        refused([geo], [params(R, "geo")], [R.QualityTarget(40000, OCCUPIED)], "occupancy source")
        refused([geo, occ], [params(R, "geo"), PO], [R.QualityTarget(40000, OCCUPIED), R.QualityTarget()], "occupancy source")       # the occupancy entry is behind it
        P2 = R.StreamParams(0, 8, 2, 5, -1, 0, 0, 0, 0)                                                                              # passed through, not pooled
        refused([occ, geo], [P2, params(R, "geo")], [R.QualityTarget(), R.QualityTarget(40000, OCCUPIED)], "occupancy source")
        big = source(192, 128, 9, "geo")                                                                                             # 192 / 16 = 12 across, 128 / 16 = 8 down
        refused([occ, big], [PO, params(R, "geo")], [R.QualityTarget(), R.QualityTarget(40000, OCCUPIED)], "does not fit")
        refused([occ, geo], [PO, params(R, "geo", occupancy_rd=1, verify_md5=1)], [R.QualityTarget(), R.QualityTarget(40000)], "verify_md5")
        # the context still transcodes, and an occupancy entry without a floor carries qp, bytes and zeros
        outs, res = ctx.wait_gof_quality(ctx.submit_gof_quality([occ, geo], [PO, params(R, "geo", 40)], [R.QualityTarget(), R.QualityTarget(0, OCCUPIED)]))
        assert outs[1] == s[40] and outs[0] == ctx.transcode_gof([occ], [PO])[0]
        assert (res[0]["qp"], res[0]["bytes"], res[0]["sse"], res[0]["samples_occ"]) == (8, len(outs[0]), [0, 0, 0], [0, 0, 0])
        assert res[1]["samples_occ"][0] > 0
        with pytest.raises(R.RbtError):       # a corrupt input fails in the wait half as it does without a floor, and the context goes on
            ctx.transcode_gof_quality([geo[:len(geo) // 2]], [params(R, "geo")], [R.QualityTarget(40000)])
        assert ctx.transcode_gof([geo], [params(R, "geo", 33)])[0] == s[33]
    finally:
        ctx.set_depth(old)


# ------------------------------------------------------------------------------------------------ container
def check_container(R, ctx):
    import v3c_synth as V
    data, gofs = v3c_file()
    PO = R.StreamParams(*OCC_P, 0)
    # floors 1 dB above what QP 30 / 34 reach in the first GOF: the floors, not the constant QPs, decide
    _, r0 = ctx.transcode_gof_quality(gofs[0], [PO, params(R, "geo", 30), params(R, "attr", 34)], [R.QualityTarget()] * 3)
    gf, af = int(r0[1]["psnr"][0] * 1000) + 1000, int(r0[2]["psnr"][0] * 1000) + 1000
    _, src_units = V.parse(data)
    for rd, region in ((0, ALL), (1, OCCUPIED)):
        out, per = ctx.transcode_v3c_quality(data, 30, 34, gf, af, region, occupancy_rd=rd)
        _, got = V.parse(out)
        assert len(got) == len(src_units) == 10 and len(per) == 2
        for g, st in enumerate(gofs):
            want, res = ctx.transcode_gof_quality(st, [PO, params(R, "geo", 30, rd), params(R, "attr", 34, rd)], [R.QualityTarget(), R.QualityTarget(gf, region), R.QualityTarget(af, region)])
            for k, (t, i) in enumerate(((V.OVD, 2), (V.GVD, 3), (V.AVD, 4))):
                assert got[5 * g + i] == V.unit_header(t) + O.byte_to_sample_stream(want[k]), (g, k)
            assert got[5 * g] == src_units[5 * g] and got[5 * g + 1] == src_units[5 * g + 1]      # V3C_VPS, V3C_AD: carried over
            assert per[g][0] == res[1] and per[g][1] == res[2]
            assert res[1]["qp"] != 30 or res[2]["qp"] != 34
    # a floor for one type only: the other is coded at its QP
    out1, per1 = ctx.transcode_v3c_quality(data, 30, 34, gf, 0)
    _, got1 = V.parse(out1)
    for g, st in enumerate(gofs):
        assert got1[5 * g + 4] == V.unit_header(V.AVD) + O.byte_to_sample_stream(ctx.transcode_gof([st[2]], [params(R, "attr", 34)])[0])
        assert (per1[g][1]["qp"], per1[g][1]["n_encodes"]) == (34, 1) and per1[g][1]["sse"][0] > 0
    # no floor at all: rbt_transcode_v3c's bytes, with and without occupancy_rd, several GOFs a job
    assert ctx.transcode_v3c_quality(data, 30, 34)[0] == ctx.transcode_v3c(data, 30, 34)
    assert ctx.transcode_v3c_quality(data, 30, 34, occupancy_rd=1, gofs_per_job=2)[0] == ctx.transcode_v3c(data, 30, 34, occupancy_rd=1)
    with pytest.raises(R.RbtError) as e:
        ctx.transcode_v3c_quality(data, 30, 34, -5, 0)
    assert e.value.code == -4
