"""Cases and checks of the colour PSNR per patch of the decoded cloud (rbt_score_patches_color, rbt_score_pair_patches_color; csrc/rbt_score.h "col/patch") and of the colour
floors held patch by patch (rbt_submit_gof_color_patches), shared by tests/test_patch_color.py (serial host emulation of the kernel bodies) and
tests/test_gpu_patch_color.py (the GPU build). The definition of include/rbt.h is restated in numpy by brute force - nearest distances on the full matrix, tie sets,
rounded tie means, owners, the BT.709 integer rows - without a call into the library. The jobs are checked against clouds rebuilt independently from the returned
streams: rbt_decode, rbt_pcloud_from_maps, rbt_score_patches_color / rbt_score."""
import functools
import math
import numpy as np
import pytest
import color_cases as CC
import score_cases as SC
import patch_d1_cases as PD
import color_floor_cases as CF

F32 = np.float32
INTS = ("n_ab", "n_ba", "sse_ab", "sse_ba")
FLOATS = ("mse_ab", "mse_ba", "mse", "psnr")
ROWS = np.array([[2126, 7152, 722], [-1146, -3854, 5000], [5000, -4542, -458]], np.int64)      # convertRGBtoYUVBT709 times 10000


# ---- the definition, by brute force ----
def _merged(xyz, rgb):
    """one point per voxel: position, colour sum // count per channel, lowest point index"""
    u, first, inv, cnt = np.unique(np.asarray(xyz, np.int64), axis=0, return_index=True, return_inverse=True, return_counts=True)
    sums = np.zeros((len(u), 3), np.int64); np.add.at(sums, inv.reshape(-1), np.asarray(rgb, np.int64))
    return u, sums // cnt[:, None], first


def _errors(cP, T, cQ):
    """e[0..2] per point of P: its merged colour against the mean over its tie set T (rows: P, columns: Q) rounded half up"""
    n = T.sum(1).astype(np.int64)[:, None]
    s = T.astype(np.int64) @ cQ
    return (cP - (2 * s + n) // (2 * n)) @ ROWS.T


def definition(a, ca, b, cb, labels, n_patches):
    """-> dict n [P, 2] (A -> B, B -> A), sse [P, 2, 3]"""
    A, mA, _ = _merged(a, ca); B, mB, ib = _merged(b, cb)
    lab = np.asarray(labels, np.int64)
    d = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)
    Tab = d == d.min(1, keepdims=True); Tba = (d == d.min(0, keepdims=True)).T
    owner = np.where(Tab, ib[None, :], np.iinfo(np.int64).max).min(1)          # the lowest point index among B's merged points at exactly the distance
    n = np.zeros((n_patches, 2), np.int64); sse = np.zeros((n_patches, 2, 3), np.int64)
    for col, k, e in ((0, lab[owner], _errors(mA, Tab, mB)), (1, lab[ib], _errors(mB, Tba, mA))):
        np.add.at(n[:, col], k, 1)
        for c in range(3): np.add.at(sse[:, col, c], k, e[:, c] ** 2)
    return dict(n=n, sse=sse)


def derived(g):
    """the float fields of a patch from its integers, by color_cases.derived - the routine of rbt_color_metric -; a direction without a point has mse 0 and psnr +inf"""
    out = {k: [] for k in FLOATS}
    for c in range(3):
        mab, pab = CC.derived(g["sse_ab"][c], g["n_ab"]) if g["n_ab"] else (F32(0), F32(np.inf))
        mba, pba = CC.derived(g["sse_ba"][c], g["n_ba"]) if g["n_ba"] else (F32(0), F32(np.inf))
        out["mse_ab"].append(mab); out["mse_ba"].append(mba); out["mse"].append(max(mab, mba)); out["psnr"].append(min(pab, pba))
    return out


def check_floats(g):
    want = derived(g)
    for k in FLOATS:
        assert [F32(x) for x in g[k]] == want[k], (k, g, want)


# ---- clouds: those of score_cases (colours on both sides) with the label patterns of patch_d1_cases ----
def _base(k, length, nb=None):
    a, ca, _, b, cb = SC.base(k)
    if nb: b, cb = b[:nb], cb[:nb]
    lab, n = PD.runs(len(b), length)
    return a, ca, b, cb, lab, n


def _sizes(n, side):
    a, ca, _, b, cb = SC.base(1)
    if side == "a": a, ca = a[:n], ca[:n]
    else: b, cb = b[:n], cb[:n]
    lab, k = PD.runs(len(b), 37)                                              # 37 divides neither 64 nor 256: runs of labels end inside a wave
    return a, ca, b, cb, lab, k


def _shuffled():
    a, ca, _, b, cb = SC.base(0)
    return a, ca, b[:1500], cb[:1500], np.random.default_rng(9).integers(0, 37, 1500).astype(np.uint32), 37


def _tie(first):
    """patch_d1_cases._case_tie with colours: the tie set of A's only point spans voxels of patches 1 and 0, and the lower point index carries label 1 in both orders;
    the tie colour is the rounded mean of two different colours"""
    a, b, lab, n = PD._case_tie(first)
    return a, np.array([[200, 100, 50]], np.uint8), b, np.array([[10, 20, 31], [90, 60, 40], [1, 2, 3]], np.uint8), lab, n


def _gap():
    a, b, lab, n = PD._case_gap()                                             # patches 2 and 6 without a point in either direction
    return a, SC.base(1)[1], b, SC.base(1)[4][:len(b)], lab, n


def _one_way():
    """patch 3: twenty points far from A - representatives of their own (n_ba > 0) that own no point of A (n_ab = 0)"""
    a, ca, _, b, cb = SC.base(1)
    b, cb = b[:300], cb[:300]
    far = (np.arange(60).reshape(20, 3) % 7 + 600).astype(np.int16); far[:, 0] += np.arange(20, dtype=np.int16)
    lab = np.concatenate([np.arange(300) // 100, np.full(20, 3)]).astype(np.uint32)
    return a, ca, np.concatenate([b, far]), np.concatenate([cb, cb[:20]]), lab, 4


def _duplicates():
    """patch 2 holds nothing but copies of points of patch 0, in other colours: it has no representative, and the merged colour of those voxels is no duplicate's"""
    a, ca, _, b, cb = SC.base(1)
    b, cb = b[:300], cb[:300]
    lab = np.concatenate([np.zeros(150), np.ones(150), np.full(40, 2)]).astype(np.uint32)
    return a, ca, np.concatenate([b, b[:40]]), np.concatenate([cb, (255 - cb[:40]).astype(np.uint8)]), lab, 3


def _single_patch():
    a, ca, _, b, cb = SC.base(1)
    return a, ca, b[:1000], cb[:1000], np.zeros(1000, np.uint32), 1


def _wide():
    a, ca, _, b, cb = SC.base(1)
    return a, ca, b[:5], cb[:5], np.array([0, 65535, 40000, 65535, 1], np.uint32), 65536


SUM_CASES = {"runs_97_many_blocks": lambda: _base(0, 97), "runs_211": lambda: _base(2, 211), "shuffled": _shuffled, "tie_lower_index_first": lambda: _tie(0),
             "tie_lower_index_second": lambda: _tie(1), "empty_patches": _gap, "one_direction_only": _one_way, "duplicates_of_an_earlier_patch": _duplicates,
             "single_patch": _single_patch, "p65536": _wide}
SUM_CASES.update({"size_%d_%s" % (n, s): (lambda n=n, s=s: _sizes(n, s)) for n in (1, 63, 64, 65, 255, 256, 257) for s in "ab"})

_REF = {}


def reference(name):
    if name not in _REF:
        case = SUM_CASES[name]()
        _REF[name] = case + (definition(*case),)
    return _REF[name]


def score(ctx, a, ca, b, cb, lab, n, raw=False):
    """uploads, labels, scores per patch -> (patches, whole, rbt_score's colour part, rbt_score_patches' counts)"""
    ha, hb = ctx.pcloud_upload(a, ca), ctx.pcloud_upload(b, cb)
    try:
        hb.set_labels(lab)
        got, whole, ms = ctx.score_patches_color(ha, hb, n, raw=raw)
        assert ms >= 0
        if raw: return got, whole, None, None
        return got, whole, ctx.score(ha, hb, 1023, SC.COLOR)["color"], [(p["n_ab"], p["n_ba"]) for p in ctx.score_patches(ha, hb, n)[0]]
    finally:
        ha.release(); hb.release()


def check_relations(got, whole, color, d1_counts, n):
    """the relations of the definition, all exact: against rbt_score's colour part, rbt_score_patches' counts and the float routine"""
    assert whole == color                                                       # bit for bit: dicts of Python floats made of the same bits
    assert [(g["n_ab"], g["n_ba"]) for g in got] == d1_counts
    assert (sum(g["n_ab"] for g in got), sum(g["n_ba"] for g in got)) == (color["n_a"], color["n_b"])
    for c in range(3):
        assert (sum(g["sse_ab"][c] for g in got), sum(g["sse_ba"][c] for g in got)) == (color["sse_ab"][c], color["sse_ba"][c])
    for k in (range(n) if n <= 700 else (0, 1, 40000, n - 1)):
        g = got[k]
        check_floats(g)
        if g["n_ab"] + g["n_ba"] == 0:
            assert g["sse_ab"] == g["sse_ba"] == [0, 0, 0] and g["mse"] == [0, 0, 0] and g["psnr"] == [np.inf] * 3, (k, g)
    if n == 1:
        assert [got[0][k] for k in INTS] == [color[k] for k in ("n_a", "n_b", "sse_ab", "sse_ba")]
        assert all(got[0][k] == color[k] for k in FLOATS)


def check_sums(ctx, name, other=None):
    a, ca, b, cb, lab, n, want = reference(name)
    got, whole, color, d1_counts = score(ctx, a, ca, b, cb, lab, n)
    assert np.array_equal(np.array([[g["n_ab"], g["n_ba"]] for g in got]), want["n"]), name
    have = np.array([[g["sse_ab"], g["sse_ba"]] for g in got], np.int64)
    bad = np.nonzero((have != want["sse"]).any((1, 2)))[0]
    assert len(bad) == 0, (name, bad[:5], have[bad[:5]], want["sse"][bad[:5]])
    check_relations(got, whole, color, d1_counts, n)
    assert sum(sum(g["sse_ab"]) + sum(g["sse_ba"]) for g in got) > 0, name        # no case passes on zeros
    if name.startswith("tie_"):                                                   # the other owner would move the term: patch 1 holds the lower index in both orders
        assert (got[1]["n_ab"], got[0]["n_ab"]) == (1, 0) and min(got[1]["sse_ab"]) > 0 and got[0]["sse_ab"] == [0, 0, 0]
    if name == "empty_patches": assert all(got[k]["psnr"] == [np.inf] * 3 and got[k]["n_ab"] + got[k]["n_ba"] == 0 for k in (2, 6))
    if name == "one_direction_only": assert (got[3]["n_ab"], got[3]["n_ba"]) == (0, 20) and got[3]["mse_ab"] == [0, 0, 0] and min(got[3]["mse_ba"]) > 0 and all(math.isfinite(x) for x in got[3]["psnr"])
    if name == "duplicates_of_an_earlier_patch": assert (got[2]["n_ab"], got[2]["n_ba"]) == (0, 0) and got[2]["psnr"] == [np.inf] * 3 and got[0]["n_ab"] > 0
    if name == "shuffled": assert all(len(set(lab[w:w + 64].tolist())) > 1 for w in range(0, 1500, 64))      # every wave is mixed
    if name == "runs_97_many_blocks": assert len(a) > 2048 and len(b) > 2048
    if other is not None:
        g2, w2, _, _ = score(other, a, ca, b, cb, lab, n)
        assert g2 == got and w2 == whole


def check_pair(ctx, other=None):
    """the pair's call equals the cloud call and rbt_score_pair_color, before and after either cloud gets new colours; the definition holds after them"""
    a, ca, b, cb, lab, n = _base(1, 211, 1800)
    ha, hb = ctx.pcloud_upload(a, ca), ctx.pcloud_upload(b, cb)
    hb.set_labels(lab)
    pair = ctx.score_pair(ha, hb)
    out = []
    try:
        for step in range(3):
            if step == 1: cb = CF.new_colors(len(b), 41); hb.set_colors(cb)
            if step == 2: ca = CF.new_colors(len(a), 42); ha.set_colors(ca)
            got, whole = pair.patches_color(n)
            g2, w2, _ = ctx.score_patches_color(ha, hb, n)
            assert got == g2 and whole == w2 == pair.color()
            want = definition(a, ca, b, cb, lab, n)
            assert np.array_equal(np.array([[g["sse_ab"], g["sse_ba"]] for g in got], np.int64), want["sse"]) and np.array_equal(np.array([[g["n_ab"], g["n_ba"]] for g in got]), want["n"])
            assert not out or got != out[-1][0]
            out.append((got, whole))
        raw1, raw2 = pair.patches_color(n, raw=True), pair.patches_color(n, raw=True)
        assert bytes(raw1[0]) == bytes(raw2[0]) and bytes(raw1[1]) == bytes(raw2[1])
    finally:
        pair.release(); ha.release(); hb.release()
    if other is not None:
        assert out == check_pair(other)
    return out


def check_determinism(ctx):
    """two calls return the same bits, floats included"""
    case = reference("size_257_b")[:6]
    x, y = score(ctx, *case, raw=True), score(ctx, *case, raw=True)
    assert bytes(x[0]) == bytes(y[0]) and bytes(x[1]) == bytes(y[1]) and x[0][0].sse_ba[0] > 0


def check_still_works(ctx):
    a, ca, b, cb, lab, n, want = reference("tie_lower_index_first")
    got = score(ctx, a, ca, b, cb, lab, n)[0]
    assert [[g["n_ab"], g["n_ba"]] for g in got] == want["n"].tolist() and [[g["sse_ab"], g["sse_ba"]] for g in got] == want["sse"].tolist()


def check_score_arguments(R, ctx, make_ctx):
    """every refusal is RBT_ERR_PARAM with its reason before any sum is written; the context and the handles go on"""
    a, ca, b, cb, lab, n = _tie(0)
    ha, hb, hplain, hgrey_a, hgrey_b = ctx.pcloud_upload(a, ca), ctx.pcloud_upload(b, cb), ctx.pcloud_upload(b, cb), ctx.pcloud_upload(a), ctx.pcloud_upload(b)
    hb.set_labels(lab); hgrey_b.set_labels(lab)
    other_ctx = make_ctx()
    pairs = []
    try:
        foreign = other_ctx.pcloud_upload(b, cb); foreign.set_labels(lab)
        f = ctx.score_patches_color
        def pair_call(x, y, k):
            p = ctx.score_pair(x, y); pairs.append(p)
            return p.patches_color(k)
        bad = [(lambda: f(ha, foreign, n), "not a cloud"), (lambda: f(foreign, hb, n), "not a cloud"), (lambda: f(None, hb, n), "not a cloud"), (lambda: f(ha, None, n), "not a cloud"),
               (lambda: f(ha, hplain, n), "no labels"), (lambda: pair_call(ha, hplain, n), "no labels"),
               (lambda: f(ha, hb, 2), "not below n_patches"), (lambda: f(ha, hb, 1), "not below n_patches"), (lambda: pair_call(ha, hb, 2), "not below n_patches"),
               (lambda: f(hgrey_a, hb, n), "colours"), (lambda: f(ha, hgrey_b, n), "colours"), (lambda: pair_call(hgrey_a, hb, n), "colours"),
               (lambda: f(ha, hb, 0), "n_patches"), (lambda: f(ha, hb, 65537), "n_patches"), (lambda: f(ha, hb, -1), "n_patches"), (lambda: pair_call(ha, hb, 0), "n_patches")]
        for g, word in bad:
            with pytest.raises(R.RbtError) as e: g()
            assert e.value.code == -4 and word in str(e.value), (word, str(e.value))
            check_still_works(ctx)
        # a pair of another context; a pair one of whose clouds has been released
        mine = ctx.score_pair(ha, hb); pairs.append(mine)
        out = (R.PatchColor * n)()
        assert ctx.L.rbt_score_pair_patches_color(other_ctx.h, mine.h, n, out, None) == -4 and b"not a score pair of this context" in other_ctx.L.rbt_last_error(other_ctx.h)
        gone = ctx.pcloud_upload(b, cb); gone.set_labels(lab)
        stale = ctx.score_pair(ha, gone); pairs.append(stale)
        gone.release()
        with pytest.raises(R.RbtError) as e: stale.patches_color(n)
        assert e.value.code == -4 and "released" in str(e.value)
        check_still_works(ctx)
        want = definition(a, ca, b, cb, lab, n)
        for np_ in (n, 65536):                                                # the same handles score as fresh ones do, through either call
            for got in (f(ha, hb, np_)[0], mine.patches_color(np_)[0]):
                assert [[g["sse_ab"], g["sse_ba"]] for g in got[:n]] == want["sse"].tolist()
    finally:
        for p in pairs: p.release()
        other_ctx.close()
    for h in (ha, hb, hplain, hgrey_a, hgrey_b): h.release()


def check_merged_limit(R, ctx):
    """more than 2^21 merged points in a cloud: refused by both calls on either side, and the context goes on"""
    xyz, rgb = CF.big_cloud()
    big = ctx.pcloud_upload(xyz, rgb); big.set_labels(np.zeros(len(xyz), np.uint32))
    a, ca, b, cb, lab, n = _tie(0)
    ha, hb = ctx.pcloud_upload(a, ca), ctx.pcloud_upload(b, cb); hb.set_labels(lab)
    pair = ctx.score_pair(big, big)                                           # (every search ends at distance 0)
    try:
        for g in (lambda: ctx.score_patches_color(ha, big, 1), lambda: ctx.score_patches_color(big, hb, n), lambda: pair.patches_color(1)):
            with pytest.raises(R.RbtError) as e: g()
            assert e.value.code == -4 and "2^21 merged points" in str(e.value), str(e.value)
        check_still_works(ctx)
    finally:
        pair.release(); big.release(); ha.release(); hb.release()


# ------------------------------------------------------------------------------------------------ the job (rbt_submit_gof_color_patches)
import oracle_lib as O
import pcc_cases
import frame_qp_cases as FC
from frame_qp_cases import variant

QP = FC.QP
GEO_QP = CF.GEO_QP       # the geometry source is coded at its own QP, whatever the attribute QPs
NAME = "seam128"         # patch_d1_cases.job_case: 128 x 128, 16 patches of one CTB of 32 each, 2 frames
luma = CF.luma
_plain = PD._plain


@functools.lru_cache(maxsize=None)
def job_case():
    """patch_d1_cases.job_case(NAME) with an attribute entry as color_floor_cases makes it: four smooth pictures behind the occupancy and the geometry stream"""
    c = dict(PD.job_case(NAME)); w, h = c["w"], c["h"]
    r = CF.rng(500)
    attr = O.encode_hm(np.stack([CF.smooth_attr(r, w, h) for _ in range(2 * c["n_frames"])]), w, h, 10, 16)[0]
    c["src"] = list(c["src"]) + [attr]; c["transfer"] = 1
    return c


def params(R, v=variant(), qp=QP):
    return [FC.occ_params(R), FC.params(R, "geo", v, GEO_QP), FC.params(R, "attr", v, qp)]


def maps_cloud(ctx, c, streams, prec, f, host_copy=False):
    """rbt_decode + rbt_pcloud_from_maps of frame f of [occupancy, geometry, attribute] streams, with the atlas at occupancy precision prec"""
    w, h = c["w"], c["h"]
    om, ow, oh, *_ = ctx.decode(streams[0], verify_md5=False); g, *_ = ctx.decode(streams[1], verify_md5=False); t, *_ = ctx.decode(streams[2], verify_md5=False)
    assert ow * prec == w
    a = pcc_cases._copy_atlas(CF._R(), c["atlas"], occupancy_precision=prec)
    return ctx.pcloud_from_maps(a, c["patches"][f], luma(om[f], ow, oh), luma(g[2 * f], w, h), luma(g[2 * f + 1], w, h), 10, t[2 * f], t[2 * f + 1], 10, 0, c["transfer"], host_copy=host_copy)


class References:
    """the references of a job and of its independent rescoring, in one context: handles (the cloud of the decoded input moved by one voxel, its colours reversed, uploaded)
    or None - then the job takes the cloud of the decoded input, and the rescoring makes that cloud through rbt_decode and rbt_pcloud_from_maps"""

    def __init__(self, ctx, handles):
        c = job_case(); self.handles, self.clouds = handles, []
        for f in range(c["n_frames"]):
            if not handles: self.clouds.append(maps_cloud(ctx, c, c["src"], 2, f)); continue
            cl, host = maps_cloud(ctx, c, c["src"], 2, f, host_copy=True)
            cl.release()
            self.clouds.append(ctx.pcloud_upload((host[0] + np.array([1, 0, 0], np.int16)).astype(np.int16), host[4][:, ::-1].copy()))

    def arg(self):
        return self.clouds if self.handles else None

    def release(self):
        for cl in self.clouds: cl.release()


def target(R, refs, **kw):
    c = job_case()
    return [R.PatchColorTarget(), R.PatchColorTarget(), R.PatchColorTarget(kw.pop("atlas", c["atlas"]), kw.pop("patches", c["patches"]), reference=refs.arg() if refs else None, **kw)]


def rescore(ctx, refs, outs):
    """the clouds of the returned streams, rebuilt through rbt_decode and rbt_pcloud_from_maps, against refs -> per frame (patch dicts, the whole frame's colour dict)"""
    c = job_case(); out = []
    for f in range(c["n_frames"]):
        cl = maps_cloud(ctx, c, outs, 4, f)
        try:
            pats, whole, _ = ctx.score_patches_color(refs.clouds[f], cl, len(c["patches"][f]))
            assert whole == ctx.score(refs.clouds[f], cl, 1023, SC.COLOR)["color"]
            out.append((pats, whole))
        finally:
            cl.release()
    return out


def check_picks(R, ctx, refs, outs, res, channel=0, v=variant()):
    """the result of a job against its own streams: the attribute stream is rbt_transcode_gof_qp_map's for the result's map, the geometry stream rbt_transcode_gof's; picks and
    frames equal the independent rescoring"""
    c = job_case(); r = res[2]
    assert outs == ctx.transcode_gof_qp_map(c["src"], params(R, v), [None, None, r["map"]]) and r["bytes"] == len(outs[2])
    assert outs[:2] == ctx.transcode_gof(c["src"], params(R, v))[:2]
    assert [x["bytes"] for x in r["frames"]] == FC.frame_sizes(outs[2])
    again = rescore(ctx, refs, outs)
    for f, (fr, (pats, whole)) in enumerate(zip(r["frames"], again)):
        assert fr["color"] == whole and fr["n_patches"] == len(pats), (f, fr["color"], whole)
        for k, p in enumerate(fr["patches"]):
            assert p["color"] == pats[k] and p["figure"] == float(F32(p["color"]["psnr"][channel])), (f, k, p, pats[k])
    assert r["met_all"] == int(all(fr["met"] for fr in r["frames"])) and r["pictures_encoded"] == 2 * sum(fr["n_trials"] for fr in r["frames"])
    for k in (0, 1):
        assert (res[k]["n_frames"], res[k]["map"], res[k]["frames"], res[k]["bytes"]) == (0, None, [], len(outs[k]))


def _both(R, ctx, other, handles, run):
    """run(ctx, refs) with fresh references; with `other` the same there, and every field equal"""
    refs = References(ctx, handles)
    try:
        got = run(ctx, refs)
    finally:
        refs.release()
    if other is not None:
        r2 = References(other, handles)
        try:
            theirs = other.transcode_gof_color_patches(job_case()["src"], params(R, got[2]), target(R, r2, **got[3]))
        finally:
            r2.release()
        assert theirs[0] == got[0] and _plain(theirs[1]) == _plain(got[1])
    return got


def check_report(R, ctx, handles, other=None, v=variant()):
    """floor 0: one trial at the entry's QP with the uniform map, every patch's rbt_patch_color reported"""
    c = job_case()
    def run(ctx, refs):
        outs, res = ctx.transcode_gof_color_patches(c["src"], params(R, v), target(R, refs))
        r = res[2]
        assert r["n_passes"] == 1 and r["pictures_encoded"] == 2 * c["n_frames"] and r["met_all"] == 1 and r["qp_probe"] == QP and (r["map"] == QP).all()
        assert all(p["met"] == 1 and p["failed"] == 0 and p["qp"] == QP for fr in r["frames"] for p in fr["patches"])
        check_picks(R, ctx, refs, outs, res, 0, v)
        assert all(math.isfinite(p["figure"]) and p["color"]["n_ba"] > 0 for fr in r["frames"] for p in fr["patches"])
        return outs, res, v, {}
    return _both(R, ctx, other, handles, run)


def walk_floors(report, channel):
    """patch_d2_cases.walk_floors on the figures of `channel`: in every frame the patch with the lowest figure gets a floor 1.5 dB above it, the one with the highest a
    floor 2 dB below it, every other patch a floor half a dB below its own figure"""
    out = []
    for fr in report["frames"]:
        fig = [float(F32(p["color"]["psnr"][channel])) for p in fr["patches"]]
        assert all(math.isfinite(x) for x in fig)
        lo, hi = min(range(len(fig)), key=lambda k: fig[k]), max(range(len(fig)), key=lambda k: fig[k])
        assert lo != hi
        fl = [int((x - 0.5) * 1000) for x in fig]; fl[lo] = int((fig[lo] + 1.5) * 1000); fl[hi] = int((fig[hi] - 2.0) * 1000)
        out.append((fl, lo, hi))
    return out


def check_walk(R, ctx, handles, channel=0, other=None, max_trials=0):
    """floors from the report run that make patches move both ways; every patch meets its floor or sits at qp_min; the stream is the qp-map stream for the final map"""
    c = job_case()
    def run(ctx, refs):
        report = ctx.transcode_gof_color_patches(c["src"], params(R), target(R, refs, channel=channel))[1][2]
        plan = walk_floors(report, channel)
        kw = dict(patch_floors=[fl for fl, _, _ in plan], qp_min=20, qp_max=44, channel=channel, max_trials=max_trials)
        outs, res = ctx.transcode_gof_color_patches(c["src"], params(R), target(R, refs, **kw))
        r = res[2]
        print("channel", channel, "trials", [fr["n_trials"] for fr in r["frames"]], "QPs", [[p["qp"] for p in fr["patches"]] for fr in r["frames"]])
        check_picks(R, ctx, refs, outs, res, channel)
        if max_trials:
            assert all(fr["n_trials"] == max_trials for fr in r["frames"]) and r["n_passes"] == max_trials
            return outs, res, variant(), kw
        for fr, (fl, lo, hi) in zip(r["frames"], plan):                  # the premise: at least one patch ends below q0 and one above
            assert fr["patches"][lo]["qp"] < QP < fr["patches"][hi]["qp"], (fr["patches"][lo], fr["patches"][hi])
            assert fr["patches"][lo]["failed"] == 1
            for k, p in enumerate(fr["patches"]):
                assert p["met"] == int(p["figure"] >= fl[k] / 1000.0)
                assert p["met"] or p["qp"] == 20, (k, p)                # every patch meets its floor or sits at qp_min
        assert r["n_passes"] == max(fr["n_trials"] for fr in r["frames"]) >= 2
        return outs, res, variant(), kw
    return _both(R, ctx, other, handles, run)


def check_job_arguments(R, ctx, make_ctx):
    """every refusal of rule 5 with its reason, a wrong wait pairing that leaves the job collectable, an empty target"""
    c = job_case(); src = c["src"]; PS = params(R); T = R.PatchColorTarget
    refs = References(ctx, True)
    old = ctx.get_depth(); ctx.set_depth(1)          # one slot: a refused submit that kept it would make the next call RBT_ERR_BUSY
    try:
        alone = ctx.transcode_gof_color_patches(src, PS, target(R, refs))
        def refused(word, ts, streams=src, ps=PS):
            for call in (ctx.transcode_gof_color_patches, ctx.submit_gof_color_patches):
                with pytest.raises(R.RbtError) as e: call(streams, ps, ts)
                assert e.value.code == -4 and word in str(e.value), (word, str(e.value))
        tg = lambda **kw: target(R, refs, **kw)
        bad = tg(); bad[2].struct_size += 4
        refused("struct_size", bad)
        refused("non-attribute", [T(), tg()[2], T()])
        for lo, hi in ((-1, 30), (30, 52), (31, 30)): refused("range", tg(min_psnr_mdb=30000, qp_min=lo, qp_max=hi))
        refused("channel", tg(channel=3))
        refused("upsample_filter", tg(upsample_filter=5))
        refused("attr_transfer", tg(attr_transfer=2))
        refused("negative", tg(min_psnr_mdb=-1))
        refused("background_qp", tg(background_qp=52))
        refused("max_trials", tg(max_trials=-1))
        refused("is negative", tg(patch_floors=[[-5] * 16, None]))
        refused("log2_ctb", tg(), ps=[PS[0], PS[1], FC.params(R, "attr", variant(log2_ctb=3))])
        none = tg(); none[2].n_frames = 0
        refused("n_frames", none)
        refused("pictures / 2", tg(patches=c["patches"] * 2))
        refused("the atlas is", tg(atlas=pcc_cases._copy_atlas(R, c["atlas"], width=256)))
        refused("map_count 2", tg(atlas=pcc_cases._copy_atlas(R, c["atlas"], map_count=1)))
        refused("occupancy_precision", tg(atlas=pcc_cases._copy_atlas(R, c["atlas"], occupancy_precision=2)))
        refused("occupancy source", tg()[1:], streams=src[1:], ps=PS[1:])
        refused("geometry source", [T(), tg()[2]], streams=[src[0], src[2]], ps=[PS[0], PS[2]])
        bare = ctx.pcloud_upload(PD.input_clouds(NAME)[0])
        other_ctx = make_ctx()
        try:
            refused("no colours", [T(), T(), T(c["atlas"], c["patches"], reference=[bare, None])])
            foreign = other_ctx.pcloud_upload(PD.input_clouds(NAME)[0], np.zeros((len(PD.input_clouds(NAME)[0]), 3), np.uint8))
            refused("not a cloud of this context", [T(), T(), T(c["atlas"], c["patches"], reference=[foreign, None])])
        finally:
            bare.release(); other_ctx.close()
        again = ctx.transcode_gof_color_patches(src, PS, target(R, refs))      # the context goes on, and no refused call kept the slot
        assert again[0] == alone[0] and _plain(again[1]) == _plain(alone[1])
        # an empty target everywhere: coded at the entries' QPs
        outs, res = ctx.transcode_gof_color_patches(src, PS, [T(), T(), T()])
        assert outs == ctx.transcode_gof(src, PS) and all((r["n_frames"], r["map"], r["frames"], r["met_all"]) == (0, None, [], 1) for r in res) and res[2]["qp_probe"] == QP
        # pairing: the job is collected by its own wait call only
        job = ctx.submit_gof_color_patches(src, PS, target(R, refs))
        for wrong in (ctx.wait_gof, ctx.wait_gof_color, ctx.wait_gof_d1_patches, ctx.wait_gof_quality_patches, ctx.wait_gof_d2_patches):
            with pytest.raises(R.RbtError) as e: wrong(job)
            assert e.value.code == -4 and "collect" in str(e.value), str(e.value)
        got = ctx.wait_gof_color_patches(job)
        assert got[0] == alone[0] and _plain(got[1]) == _plain(alone[1])
        for submit, args, collect in ((ctx.submit_gof, (), ctx.wait_gof), (ctx.submit_gof_color, ([R.ColorTarget()] * 3,), ctx.wait_gof_color)):
            job = submit(src, PS, *args)
            with pytest.raises(R.RbtError) as e: ctx.wait_gof_color_patches(job)
            assert e.value.code == -4
            collect(job)
    finally:
        ctx.set_depth(old); refs.release()


def check_jobs_in_flight(R, ctx, depth, n_jobs):
    """depth jobs in flight, report and capped walk alternating, collected out of order: each returns what it returns alone"""
    c = job_case(); PS = params(R); src = c["src"]
    refs = References(ctx, True)
    old = ctx.get_depth(); ctx.set_depth(depth)
    try:
        kinds = [target(R, refs), target(R, refs, min_psnr_mdb=60000, qp_min=26, qp_max=33, max_trials=2), target(R, refs, channel=2)]
        alone = [ctx.transcode_gof_color_patches(src, PS, t) for t in kinds]
        jobs = [ctx.submit_gof_color_patches(src, PS, kinds[i % 3]) for i in range(n_jobs)]
        with pytest.raises(R.RbtError) as e:
            ctx.submit_gof_color_patches(src, PS, kinds[0])
        assert e.value.code == -7         # RBT_ERR_BUSY
        for i in list(range(1, n_jobs, 2)) + list(range(0, n_jobs, 2))[::-1]:
            got = ctx.wait_gof_color_patches(jobs[i])
            assert got[0] == alone[i % 3][0] and _plain(got[1]) == _plain(alone[i % 3][1]), i
        assert alone[1][1][2]["n_passes"] == 2
    finally:
        ctx.set_depth(old); refs.release()


def check_no_leak_between_kinds(R, ctx):
    """colour-patch, colour, D1-patch and constant-QP jobs interleaved in one context: every result equals that of the same job run alone, and rbt_device_memory is back
    where it was after rbt_trim"""
    c = job_case(); PS = params(R); src = c["src"]
    ctx.trim(); before = ctx.device_memory()["in_use"]
    refs = References(ctx, True)
    try:
        calls = [lambda: ctx.transcode_gof_color_patches(src, PS, target(R, refs, min_psnr_mdb=60000, qp_min=26, qp_max=34, max_trials=2)),
                 lambda: ctx.transcode_gof_color(src, PS, [R.ColorTarget(), R.ColorTarget(), R.ColorTarget(c["atlas"], c["patches"], 30000, 0, 0, 26, 34, 0, 1, refs.arg())]),
                 lambda: ctx.transcode_gof_d1_patches(src, PS, [R.PatchD1Target(), R.PatchD1Target(c["atlas"], c["patches"], 60000, max_trials=2), R.PatchD1Target()]),
                 lambda: (ctx.transcode_gof(src, PS), [])]
        plain = lambda x: (x[0], _plain(x[1]))
        alone = [plain(f()) for f in calls]
        for order in ((0, 1, 2, 3), (3, 0, 2, 0, 1), (1, 0)):
            for k in order: assert plain(calls[k]()) == alone[k], k
        assert alone[0][1][2]["n_passes"] == 2 and alone[1][1][2]["n_encodes"] >= 1 and alone[2][1][1]["n_passes"] == 2      # the walks ran
    finally:
        refs.release()
    ctx.trim()
    assert ctx.device_memory()["in_use"] == before
