"""Transcoding to a byte budget (include/rbt.h: rbt_level_census, rbt_rate_estimate, rbt_submit_gof_rate / rbt_wait_gof_rate, rbt_transcode_v3c_rate): one set of
cases for the host emulation (tests/test_rate.py) and the GPU (tests/test_gpu_rate.py).
  census    a NumPy restatement of the definition on random arrays; exact equality
  estimate  the table of rbt_rate_estimate against the formula applied to the returned histograms and to B_k from a start-code split made here
  walk      s(q) from the oracle for q = 18..45, tabulated once per stream and variant; the definition's walk from the reported estimate; the stream must be the oracle's
Everything the oracle computes is cached in this module, so the host and the GPU tests of one run share it."""
import functools
import numpy as np
import pytest
import oracle_lib as O
import synth

LS = np.array([40, 45, 51, 57, 64, 72], np.int64)
G = np.array([26214, 23302, 20560, 18396, 16384, 14564], np.int64)
PM_BYPASS = 4


# ------------------------------------------------------------------------------------------------ census
def np_census(y, cb, cr, qp4, pm4):
    """hist[3][53] by the definition: one line per rule"""
    hist = np.zeros((3, 53), np.uint32)
    q = np.arange(52)
    for c, plane in enumerate((y, cb, cr)):
        ys, xs = np.nonzero(plane)
        uy, ux = (ys >> 2, xs >> 2) if c == 0 else ((2 * ys) >> 2, (2 * xs) >> 2)
        keep = (pm4[uy, ux] & PM_BYPASS) == 0
        ys, xs, uy, ux = ys[keep], xs[keep], uy[keep], ux[keep]
        qin = np.clip(qp4[uy, ux].astype(np.int64), 0, 51)
        m = np.abs(plane[ys, xs].astype(np.int64)) * LS[qin % 6] * (1 << (qin // 6))
        survives = 3 * m[:, None] * G[q % 6][None, :] >= (np.int64(1) << (21 + q // 6))[None, :]
        assert (survives[:, 1:] <= survives[:, :-1]).all()      # monotone in q
        hist[c] = np.bincount(survives.sum(axis=1), minlength=53)
    return hist


def _random_picture(w, h, seed, density=0.08, qp=None):
    r = np.random.default_rng(seed)

    def plane(pw, ph):
        mag = np.minimum(r.geometric(0.25, (ph, pw)), 32767) * r.choice([-1, 1], (ph, pw))
        return np.where(r.random((ph, pw)) < density, mag, 0).astype(np.int16)
    qp4 = (r.integers(10, 40, (h // 4, w // 4)) if qp is None else np.full((h // 4, w // 4), qp)).astype(np.int8)
    return [plane(w, h), plane(w // 2, h // 2), plane(w // 2, h // 2), qp4, np.ones((h // 4, w // 4), np.uint8)]   # pm: intra, no bypass


def _case_extremes():
    p = _random_picture(16, 16, 3, density=0.0)
    vals = [1, -1, 32767, -32767, -32768, 2, -2, 255]
    for c in range(3):
        flat = p[c].reshape(-1); flat[:len(vals)] = vals
    p[3][:] = np.random.default_rng(4).integers(0, 52, p[3].shape)
    return p


def _case_every_qp():
    p = _random_picture(64, 64, 5, density=0.3)          # 256 units: 0..51 several times over, and values outside the range to pin the clamp
    qp = (np.arange(256) % 52).astype(np.int64); qp[[3, 60, 117, 200, 255]] = [-3, 60, 127, -128, 52]
    p[3] = qp.reshape(16, 16).astype(np.int8)
    return p


def _case_bypass():
    p = _random_picture(72, 40, 6, density=0.3)
    p[4] = np.where(np.random.default_rng(7).random(p[4].shape) < 0.3, 1 | PM_BYPASS, 1).astype(np.uint8)
    return p


def _case_last_sample(c):
    p = _random_picture(24, 16, 8, density=0.0)
    p[c][-1, -1] = -7
    return p


def _case_padded():
    p = _random_picture(208, 120, 9)                      # a 200x120 picture coded as 208x120: nothing in the padding
    p[0][:, 200:] = 0; p[1][:, 100:] = 0; p[2][:, 100:] = 0
    return p


CENSUS_CASES = {
    "8x8": lambda: _random_picture(8, 8, 1, density=0.5),
    "16x8": lambda: _random_picture(16, 8, 2, density=0.5),
    "72x40": lambda: _random_picture(72, 40, 3),
    "200x120_in_208x120": _case_padded,
    "264x136": lambda: _random_picture(264, 136, 4),       # 13464 words: four workgroups of the kernel, plane boundaries inside them
    "dense_264x136": lambda: _random_picture(264, 136, 10, density=1.0),
    "zero": lambda: _random_picture(40, 24, 5, density=0.0),
    "extremes": _case_extremes,
    "every_qp": _case_every_qp,
    "bypass": _case_bypass,
    "last_sample_y": lambda: _case_last_sample(0),
    "last_sample_cb": lambda: _case_last_sample(1),
    "last_sample_cr": lambda: _case_last_sample(2),
}


@functools.lru_cache(maxsize=None)
def census_case(name):
    p = CENSUS_CASES[name]()
    return p, np_census(*p)


def check_census(ctx, name, other=None):
    """the library's histogram equals the definition's (and `other`, a second context's - the host emulation's next to the GPU's)"""
    p, want = census_case(name)
    got = ctx.level_census(*p)
    assert np.array_equal(got, want), name
    assert got.sum() == sum(int(np.count_nonzero(p[c][np.repeat(np.repeat((p[4] & PM_BYPASS) == 0, 4 >> (c > 0), 0), 4 >> (c > 0), 1)])) for c in range(3))
    if name == "extremes":
        assert want[:, 52].sum() >= 6        # +-32767 and -32768 survive every QP
    if other is not None:
        assert np.array_equal(other.level_census(*p), got)


def check_level_of_one():
    """a level of 1 lands in bin qin + 4 (the definition's own example)"""
    for qin in range(52):
        y = np.zeros((8, 8), np.int16); y[0, 0] = 1
        h = np_census(y, np.zeros((4, 4), np.int16), np.zeros((4, 4), np.int16), np.full((2, 2), qin, np.int8), np.ones((2, 2), np.uint8))
        assert h[0, min(52, qin + 4)] == 1, qin


# ------------------------------------------------------------------------------------------------ streams and their tables
STREAMS = [(64, 64, 5), (128, 128, 21), (192, 128, 9)]
KINDS = {"geo": (1, 16), "attr": (19, 22)}                 # video type, QP of the HM-like input
BASE = dict(log2_ctb=5, rows_per_slice=-1, md5_sei=0, preset=0)
Q_LO, Q_HI = 18, 45


@functools.lru_cache(maxsize=None)
def source(w, h, seed, kind):
    return O.encode_hm(synth.make_maps(w, h, seed)[kind], w, h, 10, KINDS[kind][1])[0]


def _variant(**kw):
    return tuple(sorted({**BASE, **kw}.items()))


@functools.lru_cache(maxsize=None)
def table(w, h, seed, kind, variant=_variant()):
    """q -> the oracle's stream at q, for q = 18..45"""
    src = source(w, h, seed, kind)
    return {q: O.transcode_substream(src, KINDS[kind][0], q, **dict(variant)) for q in range(Q_LO, Q_HI + 1)}


def params(R, kind, variant=_variant(), qp=30):
    v = dict(variant)
    return R.StreamParams(KINDS[kind][0], qp, 4, v["log2_ctb"], v["rows_per_slice"], v["md5_sei"], 0, 0, v["preset"])


def split_annexb(data):
    """NAL units of an Annex-B stream: between start codes, trailing zero bytes dropped"""
    pos, out = [], []
    i = data.find(b"\x00\x00\x01")
    while i >= 0:
        pos.append(i); i = data.find(b"\x00\x00\x01", i + 3)
    for k, p in enumerate(pos):
        out.append(data[p + 3:pos[k + 1] if k + 1 < len(pos) else len(data)].rstrip(b"\x00"))
    return out


def picture_bytes(data):
    """B_k: VCL NAL units (types below 32) per picture; a picture starts at first_slice_segment_in_pic_flag"""
    out = []
    for nal in split_annexb(data):
        if (nal[0] >> 1) & 0x3F < 32:
            if nal[2] & 0x80:
                out.append(0)
            out[-1] += len(nal)
    return out


def estimate_table(hist, bytes_k):
    """E(q), q = 0..51, by section 2"""
    E = []
    for q in range(52):
        e = 0
        for k in range(hist.shape[0]):
            qk = q if k % 2 else max(0, q - 3)
            nz, n0 = int(hist[k][:, qk + 1:].sum()), int(hist[k].sum())
            e += int(bytes_k[k]) * nz // max(1, n0)
        E.append(e)
    return E


def walk(s, E, T, lo, hi):
    """the definition of section 3 on sizes s[q] and estimates E[q] -> (qe, q*, met)"""
    qe = next((q for q in range(lo, hi + 1) if E[q] <= T), hi)
    q = qe
    if s[q] <= T:
        while q > lo and s[q - 1] <= T:
            q -= 1
        return qe, q, 1
    while q < hi and s[q] > T:
        q += 1
    return qe, q, int(s[q] <= T)


@functools.lru_cache(maxsize=None)
def _host_hist(w, h, seed, kind):
    """the host emulation's histograms of a stream, for the GPU to be compared with"""
    import rbt_lib
    c = rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)
    try:
        return c.rate_estimate(source(w, h, seed, kind), KINDS[kind][0])["hist"]
    finally:
        c.close()


def check_estimate(ctx, w, h, seed, kind, against_host=False):
    src = source(w, h, seed, kind)
    t = ctx.rate_estimate(src, KINDS[kind][0])
    want_bytes = picture_bytes(src)
    assert list(t["picture_bytes"]) == want_bytes and len(want_bytes) == 2
    assert t["hist"].shape == (2, 3, 53) and t["hist"].sum() > 0
    assert [int(e) for e in t["estimate"]] == estimate_table(t["hist"], want_bytes)
    assert all(t["estimate"][q] >= t["estimate"][q + 1] for q in range(51))
    if against_host:
        assert np.array_equal(t["hist"], _host_hist(w, h, seed, kind))
    return t


def budgets(s):
    """(T, lo, hi): above s(18) and below s(45) - both range ends, met 1 and 0 -, an exact s(q), s(q) - 1, and a narrow range whose upper end misses"""
    return [(len(s[Q_LO]) + 100, Q_LO, Q_HI), (len(s[Q_HI]) - 1, Q_LO, Q_HI), (len(s[30]), Q_LO, Q_HI), (len(s[30]) - 1, Q_LO, Q_HI), (len(s[26]), 20, 24), (len(s[40]), 38, 0 + Q_HI)]


PLATEAU = [(T, lo, Q_HI) for T in (368, 369) for lo in (Q_LO, 28, 32, 33, 34)]      # estimates below, on and above the plateau at 31..33 of the 192x128 geometry stream


def check_result(s, E, T, lo, hi, out, res):
    sizes = {q: len(v) for q, v in s.items()}
    qe, qs, met = walk(sizes, E, T, lo, hi)
    assert res["qp_estimate"] == qe, (T, lo, hi, res)
    assert (res["qp"], res["met"], res["bytes"]) == (qs, met, sizes[qs]), (T, lo, hi, res, qe, qs)
    assert res["estimate_bytes"] == E[qe]
    assert 1 <= res["n_encodes"] <= abs(qs - qe) + 4, (T, lo, hi, res)
    assert out == s[qs], (T, lo, hi, res)
    assert met == (len(out) <= T)


def check_walk(R, ctx, w, h, seed, kind, variant=_variant(), cases=None):
    src = source(w, h, seed, kind); s = table(w, h, seed, kind, variant)
    E = [int(e) for e in ctx.rate_estimate(src, KINDS[kind][0])["estimate"]]
    for T, lo, hi in cases or budgets(s):
        outs, res = ctx.transcode_gof_rate([src], [params(R, kind, variant)], [R.RateTarget(T, lo, hi)])
        check_result(s, E, T, lo, hi, outs[0], res[0])


def check_plateau(R, ctx):
    """192x128 geometry: 368, 369, 369 bytes at QP 31, 32, 33 - s is not monotone, and the walk's answer depends on where it starts"""
    s = table(192, 128, 9, "geo")
    assert len(s[31]) < len(s[32]) and len(s[32]) <= len(s[33]) and len(s[34]) < len(s[31]), "the oracle's sizes no longer hold the non-monotone case"
    assert (len(s[31]), len(s[32]), len(s[33])) == (368, 369, 369)
    check_walk(R, ctx, 192, 128, 9, "geo", cases=PLATEAU)
    src = source(192, 128, 9, "geo")
    got = {lo: ctx.transcode_gof_rate([src], [params(R, "geo")], [R.RateTarget(368, lo, Q_HI)])[1][0]["qp"] for lo in (Q_LO, 32)}
    assert got == {Q_LO: 31, 32: 34}          # from below the walk stops at 31; from 32 it has to climb over the plateau


VARIANTS = [((64, 64, 5, "geo"), _variant(rows_per_slice=1)), ((128, 128, 21, "attr"), _variant(log2_ctb=4)), ((64, 64, 5, "attr"), _variant(log2_ctb=6)),
            ((64, 64, 5, "geo"), _variant(md5_sei=1)), ((128, 128, 21, "geo"), _variant(preset=1))]


def check_variant(R, ctx, k):
    (w, h, seed, kind), variant = VARIANTS[k]
    s = table(w, h, seed, kind, variant)
    check_walk(R, ctx, w, h, seed, kind, variant, cases=[(len(s[30]), Q_LO, Q_HI), (len(s[33]) - 1, 25, 40)])


def check_mixed_job(R, ctx):
    """a targeted geometry entry, a constant-QP attribute entry and a pooled occupancy entry in one job; the blocking call and the two halves"""
    m = synth.make_maps(128, 128, 21)
    occ = O.encode(m["occ"], 64, 64, 8, 8, gop=1, i_qp_offset=0, lossless=1, log2_ctb=5, rows_per_slice=0)[0]
    geo, attr = source(128, 128, 21, "geo"), source(128, 128, 21, "attr")
    s = table(128, 128, 21, "geo"); E = [int(e) for e in ctx.rate_estimate(geo, 1)["estimate"]]
    P = [R.StreamParams(0, 8, 4, 5, -1, 0, 0, 0, 0), params(R, "geo"), params(R, "attr", qp=27)]
    T = len(s[29])
    tg = [R.RateTarget(), R.RateTarget(T, Q_LO, Q_HI), R.RateTarget()]
    want = ctx.transcode_gof([occ, geo, attr], P)
    assert want[2] == table(128, 128, 21, "attr")[27]
    for outs, res in (ctx.transcode_gof_rate([occ, geo, attr], P, tg), ctx.wait_gof_rate(ctx.submit_gof_rate([occ, geo, attr], P, tg))):
        assert outs[0] == want[0] and outs[2] == want[2]
        check_result(s, E, T, Q_LO, Q_HI, outs[1], res[1])
        assert (res[2]["qp"], res[2]["qp_estimate"], res[2]["met"], res[2]["n_encodes"], res[2]["bytes"]) == (27, 27, 1, 1, len(want[2]))
        assert res[0]["bytes"] == len(want[0])
    # no target anywhere: rbt_transcode_gof's bytes
    outs, res = ctx.transcode_gof_rate([occ, geo, attr], P, [R.RateTarget()] * 3)
    assert outs == want
    # one input at two budgets and a constant QP: decoded once, three entries
    outs, res = ctx.transcode_gof_rate([geo, geo, geo], [params(R, "geo"), params(R, "geo", qp=22), params(R, "geo")], [R.RateTarget(len(s[35]), Q_LO, Q_HI), R.RateTarget(), R.RateTarget(len(s[24]), Q_LO, Q_HI)])
    check_result(s, E, len(s[35]), Q_LO, Q_HI, outs[0], res[0]); check_result(s, E, len(s[24]), Q_LO, Q_HI, outs[2], res[2])
    assert outs[1] == s[22]


def check_jobs_in_flight(R, ctx, depth, n_jobs):
    """n_jobs jobs in flight at the given depth, collected out of order; every job has a budget of its own"""
    old = ctx.get_depth()
    ctx.set_depth(depth)
    try:
        key = (64, 64, 5, "geo") if n_jobs > 4 else (128, 128, 21, "attr")
        src = source(*key); s = table(*key); E = [int(e) for e in ctx.rate_estimate(src, KINDS[key[3]][0])["estimate"]]
        Ts = [len(s[Q_LO + (5 * k) % (Q_HI - Q_LO)]) - (k % 2) for k in range(n_jobs)]
        jobs = [ctx.submit_gof_rate([src], [params(R, key[3])], [R.RateTarget(T, Q_LO, Q_HI)]) for T in Ts]
        with pytest.raises(R.RbtError) as e:
            ctx.submit_gof_rate([src], [params(R, key[3])], [R.RateTarget(Ts[0], Q_LO, Q_HI)])
        assert e.value.code == -7         # RBT_ERR_BUSY: the depth holds for these jobs too
        assert ctx.job_memory(jobs[0]) > 0
        order = list(range(1, n_jobs, 2)) + list(range(0, n_jobs, 2))[::-1]
        for k in order:
            outs, res = ctx.wait_gof_rate(jobs[k])
            check_result(s, E, Ts[k], Q_LO, Q_HI, outs[0], res[0])
    finally:
        ctx.set_depth(old)


def check_arguments(R, ctx):
    """every refusal is RBT_ERR_PARAM with its reason, submits nothing and leaves the context usable"""
    geo = source(64, 64, 5, "geo"); s = table(64, 64, 5, "geo")
    occ = O.encode(synth.make_maps(64, 64, 5)["occ"], 32, 32, 8, 8, gop=1, i_qp_offset=0, lossless=1, log2_ctb=5, rows_per_slice=0)[0]

    def refused(streams, ps, ts, word):
        with pytest.raises(R.RbtError) as e:
            ctx.transcode_gof_rate(streams, ps, ts)
        assert e.value.code == -4 and word in str(e.value), str(e.value)
    refused([occ], [R.StreamParams(0, 8, 4, 5, -1, 0, 0, 0, 0)], [R.RateTarget(1000, Q_LO, Q_HI)], "occupancy")
    rd = params(R, "geo"); rd.occupancy_rd = 1
    refused([occ, geo], [R.StreamParams(0, 8, 4, 5, -1, 0, 0, 0, 0), rd], [R.RateTarget(), R.RateTarget(1000, Q_LO, Q_HI)], "occupancy_rd")
    bad = R.RateTarget(1000, Q_LO, Q_HI); bad.struct_size += 4
    refused([geo], [params(R, "geo")], [bad], "struct_size")
    unset = R.RateTarget(); unset.struct_size = 0
    refused([geo], [params(R, "geo")], [unset], "struct_size")
    for lo, hi in ((-1, 30), (30, 52), (31, 30), (52, 0)):
        refused([geo], [params(R, "geo")], [R.RateTarget(1000, lo, hi)], "range")
    with pytest.raises(R.RbtError) as e:
        ctx.rate_estimate(occ, 0)
    assert e.value.code == -4
    with pytest.raises(R.RbtError) as e:
        ctx.level_census(np.zeros((12, 8), np.int16), np.zeros((6, 4), np.int16), np.zeros((6, 4), np.int16), np.zeros((3, 2), np.int8), np.zeros((3, 2), np.uint8))
    assert e.value.code == -4
    # a refused call took no job slot and left nothing behind: depth 1 still takes a job, and qp_max 0 means 51
    old = ctx.get_depth(); ctx.set_depth(1)
    try:
        outs, res = ctx.wait_gof_rate(ctx.submit_gof_rate([geo], [params(R, "geo")], [R.RateTarget(len(s[40]), 40, 0)]))
    finally:
        ctx.set_depth(old)
    assert outs[0] == s[40] and res[0]["qp"] == 40 and res[0]["met"] == 1
    # a corrupt input fails in the wait half as it does without a target, and the context goes on
    with pytest.raises(R.RbtError):
        ctx.transcode_gof_rate([geo[:len(geo) // 2]], [params(R, "geo")], [R.RateTarget(1000, Q_LO, Q_HI)])
    assert ctx.transcode_gof([geo], [params(R, "geo", qp=33)])[0] == s[33]


def check_verify_md5(R, ctx):
    """verify_md5 on a targeted entry: the input's hashes are checked behind the decoder's last filter as in the constant-QP path; a wrong one fails the job, no output"""
    import picture_hash_cases as H
    src = source(64, 64, 5, "geo"); s = table(64, 64, 5, "geo")
    frames, w, h, bd, _, _ = O.decode(src)
    E = [int(e) for e in ctx.rate_estimate(src, 1)["estimate"]]
    p = params(R, "geo"); p.verify_md5 = 1
    T = len(s[31]) - 1
    outs, res = ctx.transcode_gof_rate([src], [p], [R.RateTarget(T, Q_LO, Q_HI)])
    check_result(s, E, T, Q_LO, Q_HI, outs[0], res[0])
    bad = H.rewritten(src, frames, w, h, bd, H.MD5, flip=1)
    with pytest.raises(R.RbtError) as e:
        ctx.transcode_gof_rate([bad], [p], [R.RateTarget(T, Q_LO, Q_HI)])
    assert e.value.code == H.RBT_ERR_MD5 and "input 0" in str(e.value)
    assert ctx.transcode_gof_rate([bad], [params(R, "geo")], [R.RateTarget(T, Q_LO, Q_HI)])[0][0] == outs[0]      # unchecked, the same pictures give the same stream


# ------------------------------------------------------------------------------------------------ container
@functools.lru_cache(maxsize=None)
def v3c_file():
    import v3c_synth as V
    gofs = [V.gof_streams(64, 64, 1, 40 + g, log2_ctb=5) for g in range(2)]
    units = [u for g, st in enumerate(gofs) for u in V.gof_units(st, 90 + g)]
    return V.sample_stream(units, 2), gofs


def check_container(R, ctx):
    import v3c_synth as V
    data, gofs = v3c_file()
    gbits, abits = 700, 2400
    out, per = ctx.transcode_v3c_rate(data, 30, 34, gbits, abits)
    _, got = V.parse(out); _, src_units = V.parse(data)
    assert len(got) == len(src_units) == 10 and len(per) == 2
    P = [R.StreamParams(0, 8, 4, 5, -1, 0, 0, 0, 0), R.StreamParams(1, 30, 4, 5, -1, 0, 0, 0, 0), R.StreamParams(19, 34, 4, 5, -1, 0, 0, 0, 0)]
    for g, st in enumerate(gofs):
        n_pics = [len(picture_bytes(x)) for x in st]
        tg = [R.RateTarget(), R.RateTarget((gbits * n_pics[1] + 7) // 8), R.RateTarget((abits * n_pics[2] + 7) // 8)]
        want, res = ctx.transcode_gof_rate(st, P, tg)
        for k, (t, i) in enumerate(((V.OVD, 2), (V.GVD, 3), (V.AVD, 4))):
            assert got[5 * g + i] == V.unit_header(t) + O.byte_to_sample_stream(want[k]), (g, k)
        assert got[5 * g] == src_units[5 * g] and got[5 * g + 1] == src_units[5 * g + 1]      # V3C_VPS, V3C_AD: carried over
        assert per[g][0] == res[1] and per[g][1] == res[2]
        assert res[1]["qp"] != 30 or res[2]["qp"] != 34          # the budgets, not the constant QPs, decided
    # a budget for one type only: the other is coded at its QP
    out1, per1 = ctx.transcode_v3c_rate(data, 30, 34, gbits, 0)
    _, got1 = V.parse(out1)
    for g, st in enumerate(gofs):
        assert got1[5 * g + 3] == got[5 * g + 3] and got1[5 * g + 4] == V.unit_header(V.AVD) + O.byte_to_sample_stream(ctx.transcode_gof([st[2]], [P[2]])[0])
        assert (per1[g][1]["qp"], per1[g][1]["n_encodes"]) == (34, 1)
    # no budget at all: rbt_transcode_v3c's bytes
    out0, per0 = ctx.transcode_v3c_rate(data, 30, 34, 0, 0)
    assert out0 == ctx.transcode_v3c(data, 30, 34)
    with pytest.raises(R.RbtError) as e:
        ctx.transcode_v3c_rate(data, 30, 34, gbits, 0, occupancy_rd=1)
    assert e.value.code == -4
