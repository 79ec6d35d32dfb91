"""Cases and checks of D2 per patch of the decoded cloud (rbt_score_patches_d2; csrc/rbt_score.h "D2/patch") and of the D2 floors on the stream and patch by patch
(rbt_submit_gof_d2, rbt_submit_gof_d2_patches), shared by tests/test_patch_d2.py (serial host emulation of the kernel bodies) and tests/test_gpu_patch_d2.py (the GPU
build). The definition of include/rbt.h is restated in numpy: the per-point values of pcc_cases.d2_brute_force, the owners of patch_d1_cases.definition. The jobs are
checked against clouds rebuilt independently from the returned stream: the oracle's decode, rbt_pcloud_from_maps, rbt_score / rbt_score_patches_d2."""
import ctypes
import functools
import math
import numpy as np
import pytest
import color_cases as CC
import score_cases as SC
import patch_d1_cases as PD

F32, F64 = np.float32, np.float64
PEAK = 1023
COUNTS = ("n_ab", "n_ba")
SUMS = ("sse_ab", "sse_ba")
MAXS = ("max_ab", "max_ba")
REL = 1e-9          # the tolerance score_cases.check_against_definition gives reordered double sums


# ---- the definition ----
def definition(a, na, b, labels, n_patches):
    """-> dict: n [P, 2] (A -> B, B -> A), sse [P, 2], max [P, 2], take (merged points of B that take their normal). Merged points, their normals, the tie sets, the
    give / take rule and the per-point values as pcc_cases.d2_brute_force has them; the owner of a point of A as patch_d1_cases.definition has it"""
    ua, ia = np.unique(np.asarray(a), axis=0, return_index=True); ub, ib = np.unique(np.asarray(b), axis=0, return_index=True)
    nrm = np.asarray(na)[ia].astype(F64)
    A, B = ua.astype(np.int64), ub.astype(np.int64); lab = np.asarray(labels, np.int64)
    d = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)
    tie_ab = d == d.min(1, keepdims=True); tie_ba = d == d.min(0, keepdims=True)
    acc = tie_ab.T.astype(F64) @ nrm; cnt = tie_ab.sum(0).astype(F64)
    take = np.nonzero(cnt == 0)[0]
    for j in take:
        acc[j] = nrm[tie_ba[:, j]].sum(0); cnt[j] = tie_ba[:, j].sum()
    nb = acc / cnt[:, None]
    q = 16384.0 ** 2
    v_ab = np.array([np.mean(((A[i] - B[tie_ab[i]]) * nb[tie_ab[i]]).sum(1) ** 2) for i in range(len(A))]) / q
    v_ba = np.array([np.mean(((B[j] - A[tie_ba[:, j]]) * nrm[tie_ba[:, j]]).sum(1) ** 2) for j in range(len(B))]) / q
    owner = np.where(tie_ab, ib[None, :], np.iinfo(np.int64).max).min(1)
    n = np.zeros((n_patches, 2), np.int64); sse = np.zeros((n_patches, 2)); mx = np.zeros((n_patches, 2))
    for col, k, v in ((0, lab[owner], v_ab), (1, lab[ib], v_ba)):
        np.add.at(n[:, col], k, 1); np.maximum.at(mx[:, col], k, v)
        for p in np.unique(k): sse[p, col] = math.fsum(v[k == p])
    return dict(n=n, sse=sse, max=mx, take=len(take))


def derived(sse_ab, sse_ba, n_ab, n_ba, peak):
    """patch_d1_cases.derived: the float routine with a direction without a point at mse 0"""
    return PD.derived(sse_ab, sse_ba, n_ab, n_ba, peak)


# ---- clouds: those of score_cases and patch_d1_cases, with score_cases' normals on A ----
def _with_normals(case, seed=0):
    a, b, lab, n = case
    return a, SC.normals(seed, len(a)), b, lab, n


def _base(k, length):
    a, _, na, b, _ = SC.base(k)
    lab, n = PD.runs(len(b), length)
    return a, na, b, lab, n


def _own_patch():
    """every point its own patch on about 600 points: 256 distinct labels in the first block of B, and in A's blocks as many as there are owners"""
    a, _, na, b, _ = SC.base(1)
    return a, na, b[:600], np.arange(600, dtype=np.uint32), 600


def _shuffled():
    a, _, na, b, _ = SC.base(0)
    return a, na, b[:1500], np.random.default_rng(9).integers(0, 37, 1500).astype(np.uint32), 37


def _sizes(n, side):
    a, _, na, b, _ = SC.base(1)
    if side == "a": a, na = a[:n], na[:n]
    else: b = b[:n]
    lab, k = PD.runs(len(b), 37)
    return a, na, b, lab, k


def _tie(first):
    a, b, lab, n = PD._case_tie(first)
    return a, np.array([[9459, 9459, 9459]], np.int16), b, lab, n      # a slanted normal: both tie points give a value > 0


SUM_CASES = {"runs_97": lambda: _base(0, 97), "runs_211": lambda: _base(2, 211), "own_patch_600": _own_patch, "shuffled": _shuffled,
             "duplicates_of_an_earlier_patch": lambda: _with_normals(PD._case_duplicates(), 2), "empty_patches": lambda: _with_normals(PD._case_gap(), 1),
             "tie_lower_index_first": lambda: _tie(0), "tie_lower_index_second": lambda: _tie(1), "single_patch": lambda: _with_normals(PD._case_single_patch(), 3)}
SUM_CASES.update({"size_%d_%s" % (n, s): (lambda n=n, s=s: _sizes(n, s)) for n in (1, 63, 64, 65, 255, 256, 257) for s in "ab"})
BASE_CASES = ("runs_97", "runs_211")

_REF = {}


def reference(name):
    if name not in _REF:
        a, na, b, lab, n = SUM_CASES[name]()
        _REF[name] = (a, na, b, lab, n, definition(a, na, b, lab, n))
    return _REF[name]


@functools.lru_cache(maxsize=None)
def large_case():
    """a surface of 257 x 256 points against itself with noise: B holds 65 792 points - 257 blocks, so lane 0 of the column step adds block 256 to block 0 - in runs of 97"""
    r = np.random.default_rng(77)
    y, x = np.mgrid[0:257, 0:256]
    z = np.round(300 + 40 * np.sin(x / 31.0) + 30 * np.cos(y / 23.0)).astype(np.int64)
    a = np.stack([x.ravel() + 100, y.ravel() + 100, z.ravel()], 1).astype(np.int16)
    b = np.clip(a + r.integers(-1, 2, a.shape), 0, 1023).astype(np.int16)
    lab, n = PD.runs(len(b), 97)
    assert len(b) >= 65537 and -(-len(b) // 256) > 256
    return a, SC.normals(0, len(a)), b, lab, n


def score(ctx, a, na, b, lab, n, peak=PEAK, raw=False):
    """uploads, labels, scores per patch and as a whole, releases -> (patches, whole, rbt_score's d2, rbt_score_patches' counts)"""
    ha, hb = ctx.pcloud_upload(a, None, na), ctx.pcloud_upload(b)
    try:
        hb.set_labels(lab)
        got, whole, ms = ctx.score_patches_d2(ha, hb, n, peak, raw=raw)
        assert ms >= 0
        if raw: return got, whole, None, None
        d1 = ctx.score_patches(ha, hb, n, peak)[0]
        return got, whole, ctx.score(ha, hb, peak, SC.D2)["d2"], [(p["n_ab"], p["n_ba"]) for p in d1]
    finally:
        ha.release(); hb.release()


def check_relations(got, whole, d2, d1_counts, n, peak=PEAK):
    """what holds on every case whatever the definition says: against rbt_score's d2, rbt_score_patches' counts and the float routine"""
    assert whole == d2                                                                         # bit for bit: dicts of Python floats made of the same bits
    assert [(g["n_ab"], g["n_ba"]) for g in got] == d1_counts
    assert (sum(g["n_ab"] for g in got), sum(g["n_ba"] for g in got)) == (d2["n_a"], d2["n_b"])
    assert (max(g["max_ab"] for g in got), max(g["max_ba"] for g in got)) == (d2["max_ab"], d2["max_ba"])
    tot = [math.fsum(g[k] for g in got) for k in SUMS]
    print("sum over the patches", tot, "whole", d2["sse_ab"], d2["sse_ba"])
    assert tot[0] == pytest.approx(d2["sse_ab"], rel=REL) and tot[1] == pytest.approx(d2["sse_ba"], rel=REL)
    for k, g in enumerate(got):
        assert g["max_ab"] <= g["sse_ab"] and g["max_ba"] <= g["sse_ba"] and min(g["max_ab"], g["max_ba"]) >= 0
        if g["n_ab"] + g["n_ba"] == 0:
            assert (g["sse_ab"], g["sse_ba"], g["mse_ab"], g["mse_ba"]) == (0, 0, 0, 0) and g["psnr"] == np.inf, (k, g)
    for k in sorted({0, n - 1} | {k for k in range(n) if got[k]["n_ab"] + got[k]["n_ba"]} if n <= 700 else {0, 1, n // 2, n - 1}):
        g = got[k]
        assert (F32(g["mse_ab"]), F32(g["mse_ba"]), F32(g["psnr"])) == derived(g["sse_ab"], g["sse_ba"], g["n_ab"], g["n_ba"], peak), (k, g)
    if n == 1:
        assert [got[0][k] for k in COUNTS + SUMS + MAXS] == [d2[k] for k in ("n_a", "n_b") + SUMS + MAXS]
        assert (F32(got[0]["mse_ab"]), F32(got[0]["mse_ba"]), F32(got[0]["psnr"])) == (F32(d2["mse_ab"]), F32(d2["mse_ba"]), F32(d2["psnr"]))


def check_sums(ctx, name, other=None):
    a, na, b, lab, n, want = reference(name)
    got, whole, d2, d1_counts = score(ctx, a, na, b, lab, n)
    assert np.array_equal(np.array([[g[k] for k in COUNTS] for g in got]), want["n"]), name
    for col, (s, m) in enumerate(zip(SUMS, MAXS)):
        for k in range(n):
            w = want["sse"][k, col]
            if w == 0: assert got[k][s] == 0 and got[k][m] == 0, (name, k, got[k])
            else: assert got[k][s] == pytest.approx(w, rel=REL) and got[k][m] == pytest.approx(want["max"][k, col], rel=REL), (name, k, s, got[k], w)
    check_relations(got, whole, d2, d1_counts, n)
    if name in BASE_CASES: assert want["take"] >= 40, want["take"]                            # score_cases.check_conditions' premise: points of B take their normal
    if name.startswith("tie_"):                                                               # the other owner would move the term: patch 1 holds the lower index in both orders
        assert (got[1]["n_ab"], got[0]["n_ab"]) == (1, 0) and got[1]["sse_ab"] > 0 and got[0]["sse_ab"] == 0
    if name == "duplicates_of_an_earlier_patch": assert (got[2]["n_ab"], got[2]["n_ba"], got[2]["sse_ab"], got[2]["sse_ba"]) == (0, 0, 0, 0) and got[2]["psnr"] == np.inf and got[0]["n_ab"] > 0
    if name == "empty_patches": assert all(got[k]["psnr"] == np.inf and got[k]["sse_ab"] == 0 == got[k]["sse_ba"] for k in (2, 6))
    if name == "own_patch_600": assert len({int(x) for x in lab[:256]}) == 256
    if other is not None:
        g2, w2, _, _ = score(other, a, na, b, lab, n)
        assert g2 == got and w2 == whole


def check_large(ctx, other=None):
    """65 792 points in B: the relations to the whole and, with `other`, every field bit for bit (brute force is too slow here)"""
    a, na, b, lab, n = large_case()
    got, whole, d2, d1_counts = score(ctx, a, na, b, lab, n)
    check_relations(got, whole, d2, d1_counts, n)
    assert whole["sse_ba"] > 0 and sum(1 for g in got if g["n_ba"]) == n
    if other is not None:
        g2, w2, _, _ = score(other, a, na, b, lab, n)
        assert g2 == got and w2 == whole


def check_determinism(ctx):
    """two calls return the same bits, floats included"""
    a, na, b, lab, n, _ = reference("size_257_b")
    x, y = score(ctx, a, na, b, lab, n, raw=True), score(ctx, a, na, b, lab, n, raw=True)
    assert bytes(x[0]) == bytes(y[0]) and bytes(x[1]) == bytes(y[1]) and x[0][0].sse_ba > 0


def check_still_works(ctx):
    a, na, b, lab, n, want = reference("tie_lower_index_first")
    got = score(ctx, a, na, b, lab, n)[0]
    assert [[g[k] for k in COUNTS] for g in got] == want["n"].tolist() and got[1]["sse_ab"] == pytest.approx(want["sse"][1, 0], rel=REL)


def check_score_arguments(R, ctx, make_ctx):
    """every refusal is RBT_ERR_PARAM before any sum is written; the context and the handles go on"""
    a, na, b, lab, n = _tie(0)
    ha, hb, hplain, hbare = ctx.pcloud_upload(a, None, na), ctx.pcloud_upload(b), ctx.pcloud_upload(b), ctx.pcloud_upload(a)
    hb.set_labels(lab)
    other_ctx = make_ctx()
    try:
        foreign = other_ctx.pcloud_upload(b); foreign.set_labels(lab)
        f = ctx.score_patches_d2
        bad = [lambda: f(ha, foreign, n), lambda: f(foreign, hb, n), lambda: f(None, hb, n), lambda: f(ha, None, n),
               lambda: f(ha, hplain, n),                                  # b without labels
               lambda: f(ha, hb, 2), lambda: f(ha, hb, 1),                # a label >= n_patches
               lambda: f(hbare, hb, n),                                   # a without normals
               lambda: f(ha, hb, n, peak=0), lambda: f(ha, hb, n, peak=-3),
               lambda: f(ha, hb, 0), lambda: f(ha, hb, 65537), lambda: f(ha, hb, -1)]
        for g in bad:
            SC.refused(R, g)
            check_still_works(ctx)
        want = definition(a, na, b, lab, n)
        for np_ in (n, 65536):                                            # the same handles score as fresh ones do
            got = f(ha, hb, np_)[0]
            assert [[g[k] for k in COUNTS] for g in got[:n]] == want["n"].tolist() and got[1]["sse_ab"] == pytest.approx(want["sse"][1, 0], rel=REL)
    finally:
        other_ctx.close()
    for h in (ha, hb, hplain, hbare): h.release()


# ------------------------------------------------------------------------------------------------ the jobs (rbt_submit_gof_d2, rbt_submit_gof_d2_patches)
import oracle_lib as O
import frame_qp_cases as FC
import d1_floor_cases as DC
from frame_qp_cases import variant

QP = FC.QP
NAME = "seam128"         # patch_d1_cases.job_case: 128 x 128, 16 patches of one CTB of 32 each, 2 frames
luma = DC.luma


def _plain(x):
    return PD._plain(x)


def cloud_from_maps(ctx, atlas, patches, occ, d0, d1):
    """rbt_pcloud_from_maps with grey attribute pictures, which it asks for: positions, order and labels do not depend on them"""
    grey = np.full(atlas.width * atlas.height * 3 // 2, 512, np.uint16)
    return ctx.pcloud_from_maps(atlas, patches, occ, d0, d1, 10, grey, grey, 10)


def ref_normals(f):
    return SC.normals(f, len(PD.input_clouds(NAME)[f]))


class References:
    """the references of a job and of its independent rescoring, in one context: handles (the decoded input's cloud moved by one voxel, uploaded with normals) or None -
    then the job takes the cloud of the decoded input with estimated normals, and the rescoring makes that cloud through rbt_pcloud_from_maps and
    rbt_pcloud_estimate_normals with the same parameters"""

    def __init__(self, R, ctx, handles, normals=None):
        c = PD.job_case(NAME); self.ctx, self.handles, self.clouds = ctx, handles, []
        if handles:
            for f, xyz in enumerate(PD.input_clouds(NAME)):
                self.clouds.append(ctx.pcloud_upload((xyz + np.array([1, 0, 0], np.int16)).astype(np.int16), None, ref_normals(f)))
            return
        w, h = c["w"], c["h"]
        om, ow, oh, *_ = O.decode(c["src"][0]); g = O.decode(c["src"][1])[0]
        a = PD.P._copy_atlas(R, c["atlas"], occupancy_precision=w // ow)
        for f in range(c["n_frames"]):
            cl = cloud_from_maps(ctx, a, c["patches"][f], luma(om[f], ow, oh), luma(g[2 * f], w, h), luma(g[2 * f + 1], w, h))
            cl.estimate_normals(normals, copy=False)
            self.clouds.append(cl)

    def arg(self):
        return self.clouds if self.handles else None

    def release(self):
        for cl in self.clouds: cl.release()


def rescore(R, ctx, refs, outs, per_patch):
    """the clouds of the returned streams, rebuilt from the oracle's decode through rbt_pcloud_from_maps, against refs -> per frame (patch dicts or None, whole d2)"""
    c = PD.job_case(NAME); w, h = c["w"], c["h"]
    om, ow, oh, *_ = O.decode(outs[0]); g = O.decode(outs[1])[0]
    out = []
    for f in range(c["n_frames"]):
        cl = cloud_from_maps(ctx, c["atlas"], c["patches"][f], luma(om[f], ow, oh), luma(g[2 * f], w, h), luma(g[2 * f + 1], w, h))
        try:
            whole = ctx.score(refs.clouds[f], cl, PEAK, SC.D2)["d2"]
            pats = None
            if per_patch:
                pats, w2, _ = ctx.score_patches_d2(refs.clouds[f], cl, len(c["patches"][f]), PEAK)
                assert w2 == whole
            out.append((pats, whole))
        finally:
            cl.release()
    return out


def params(R, v=variant()):
    return PD.job_params(R, v)


def stream_target(R, refs, normals=None, **kw):
    c = PD.job_case(NAME)
    return [R.D2Target(), R.D2Target(c["atlas"], c["patches"], reference=refs.arg(), normals=normals, **kw)]


def patch_target(R, refs, normals=None, **kw):
    c = PD.job_case(NAME)
    return [R.PatchD2Target(), R.PatchD2Target(c["atlas"], c["patches"], reference=refs.arg(), normals=normals, **kw)]


def d2_stats(frames):
    ps = [float(F32(fr["psnr"])) for fr in frames]
    s = 0.0
    for p in ps: s += p
    return s / len(ps), min(ps)


def check_stream_result(R, ctx, refs, outs, res):
    """the result of a stream-level job against the independent rescoring of its own stream and against rbt_transcode_gof at q*"""
    c = PD.job_case(NAME)
    again = rescore(R, ctx, refs, outs, False)
    assert res["n_frames"] == c["n_frames"] and res["frames"] == [w for _, w in again], (res["frames"], again)
    assert (res["mean_d2"], res["min_d2"]) == d2_stats(res["frames"]) and res["bytes"] == len(outs[1]) and res["cloud_ms"] >= 0
    assert outs == ctx.transcode_gof(c["src"], PD.job_params(R, variant(), res["qp"]))


def check_stream_report(R, ctx, handles, other=None):
    """floor 0 on the stream: coded at the entry's QP, the frames' D2 reported - bit for bit rbt_score's on the rebuilt clouds"""
    c = PD.job_case(NAME)
    refs = References(R, ctx, handles)
    try:
        outs, res = ctx.transcode_gof_d2(c["src"], params(R), stream_target(R, refs))
        assert (res[1]["qp"], res[1]["qp_probe"], res[1]["qp_start"], res[1]["met"], res[1]["n_encodes"]) == (QP, QP, QP, 1, 1)
        assert (res[0]["n_frames"], res[0]["frames"], res[0]["bytes"]) == (0, [], len(outs[0]))
        check_stream_result(R, ctx, refs, outs, res[1])
        assert all(fr["sse_ba"] > 0 and math.isfinite(fr["psnr"]) for fr in res[1]["frames"])
    finally:
        refs.release()
    if other is not None:
        r2 = References(R, other, handles)
        try:
            o_outs, o_res = other.transcode_gof_d2(c["src"], params(R), stream_target(R, r2))
        finally:
            r2.release()
        assert o_outs == outs and _plain(o_res) == _plain(res)
    return outs, res


def check_stream_walk(R, ctx, handles, other=None, stat=0):
    """a floor 1 dB under the reported minimum: the walk runs; the stream is rbt_transcode_gof's at q*, the frames are rbt_score's there, n_encodes <= |q* - qs| + 5"""
    c = PD.job_case(NAME)
    refs = References(R, ctx, handles)
    try:
        _, rep = ctx.transcode_gof_d2(c["src"], params(R), stream_target(R, refs))
        F = int(((rep[1]["mean_d2"] if stat else rep[1]["min_d2"]) - 1.0) * 1000)
        kw = dict(min_d2_mdb=F, stat=stat, qp_min=22, qp_max=40)
        outs, res = ctx.transcode_gof_d2(c["src"], params(R), stream_target(R, refs, **kw))
        r = res[1]
        print("floor", F, "q*", r["qp"], "qs", r["qp_start"], "encodes", r["n_encodes"], "min", r["min_d2"], "met", r["met"])
        check_stream_result(R, ctx, refs, outs, r)
        assert r["qp_probe"] == QP and 22 <= r["qp"] <= 40 and r["n_encodes"] <= abs(r["qp"] - r["qp_start"]) + 5
        fig = r["mean_d2"] if stat else r["min_d2"]
        assert r["met"] == int(fig >= F / 1000.0) and (r["met"] or r["qp"] == 22)
    finally:
        refs.release()
    if other is not None:
        r2 = References(R, other, handles)
        try:
            o_outs, o_res = other.transcode_gof_d2(c["src"], params(R), stream_target(R, r2, **kw))
        finally:
            r2.release()
        assert o_outs == outs and _plain(o_res) == _plain(res)


def check_picks(R, ctx, refs, outs, res):
    """the result of a patch job against its own stream: the stream is rbt_transcode_gof_qp_map's for the result's map; picks and frames equal the independent rescoring"""
    c = PD.job_case(NAME)
    assert outs == PD.run_map(R, ctx, NAME, res["map"], variant()) and res["bytes"] == len(outs[1])
    assert [x["bytes"] for x in res["frames"]] == FC.frame_sizes(outs[1])
    again = rescore(R, ctx, refs, outs, True)
    for f, (fr, (pats, whole)) in enumerate(zip(res["frames"], again)):
        assert fr["d2"] == whole and fr["n_patches"] == len(pats), (f, fr["d2"], whole)
        for k, p in enumerate(fr["patches"]):
            assert p["d2"] == pats[k] and p["figure"] == float(F32(p["d2"]["psnr"])), (f, k, p, pats[k])
    assert res["met_all"] == int(all(fr["met"] for fr in res["frames"])) and res["pictures_encoded"] == 2 * sum(fr["n_trials"] for fr in res["frames"])


def check_patch_report(R, ctx, handles, other=None):
    """floor 0 patch by patch: one trial at the entry's QP with the uniform map, every patch's rbt_patch_d2 reported"""
    c = PD.job_case(NAME)
    refs = References(R, ctx, handles)
    try:
        outs, res = ctx.transcode_gof_d2_patches(c["src"], params(R), patch_target(R, refs))
        r = res[1]
        assert r["n_passes"] == 1 and r["pictures_encoded"] == 2 * c["n_frames"] and r["met_all"] == 1 and r["qp_probe"] == QP and (r["map"] == QP).all()
        assert all(p["met"] == 1 and p["failed"] == 0 and p["qp"] == QP for fr in r["frames"] for p in fr["patches"])
        assert (res[0]["n_frames"], res[0]["map"], res[0]["frames"]) == (0, None, [])
        check_picks(R, ctx, refs, outs, r)
    finally:
        refs.release()
    if other is not None:
        r2 = References(R, other, handles)
        try:
            o_outs, o_res = other.transcode_gof_d2_patches(c["src"], params(R), patch_target(R, r2))
        finally:
            r2.release()
        assert o_outs == outs and _plain(o_res) == _plain(res)
    return r


def walk_floors(report):
    """floors set from a floor-0 report: in every frame the patch with the lowest finite figure gets a floor 1.5 dB above it, the one with the highest a floor 2 dB
    below it, every other patch a floor half a dB below its own figure (it meets, and has no whole dB of room to move on)"""
    out = []
    for fr in report["frames"]:
        fig = [p["figure"] for p in fr["patches"]]
        fin = [k for k, x in enumerate(fig) if math.isfinite(x)]
        lo, hi = min(fin, key=lambda k: fig[k]), max(fin, key=lambda k: fig[k])
        assert lo != hi
        fl = [int((x - 0.5) * 1000) if math.isfinite(x) else 1 for x in fig]; fl[lo] = int((fig[lo] + 1.5) * 1000); fl[hi] = int((fig[hi] - 2.0) * 1000)
        out.append((fl, lo, hi))
    return out


def check_patch_walk(R, ctx, handles, other=None):
    c = PD.job_case(NAME)
    refs = References(R, ctx, handles)
    try:
        report = ctx.transcode_gof_d2_patches(c["src"], params(R), patch_target(R, refs))[1][1]
        plan = walk_floors(report)
        kw = dict(patch_floors=[fl for fl, _, _ in plan], qp_min=20, qp_max=44)
        outs, res = ctx.transcode_gof_d2_patches(c["src"], params(R), patch_target(R, refs, **kw))
        r = res[1]
        print("trials", [fr["n_trials"] for fr in r["frames"]], "QPs", [[p["qp"] for p in fr["patches"]] for fr in r["frames"]])
        for fr, (fl, lo, hi) in zip(r["frames"], plan):                  # the premise: at least one patch moves each way
            assert fr["patches"][lo]["qp"] < QP < fr["patches"][hi]["qp"], (fr["patches"][lo], fr["patches"][hi])
            assert fr["patches"][lo]["failed"] == 1
        check_picks(R, ctx, refs, outs, r)
        for fr, (fl, _, _) in zip(r["frames"], plan):
            for k, p in enumerate(fr["patches"]):
                assert p["met"] == int(p["figure"] >= fl[k] / 1000.0)
                assert p["met"] or p["qp"] == 20, (k, p)                # every patch meets its floor or sits at lo
        assert r["n_passes"] == max(fr["n_trials"] for fr in r["frames"]) >= 2
    finally:
        refs.release()
    if other is not None:
        r2 = References(R, other, handles)
        try:
            o_outs, o_res = other.transcode_gof_d2_patches(c["src"], params(R), patch_target(R, r2, **kw))
        finally:
            r2.release()
        assert o_outs == outs and _plain(o_res) == _plain(res)


def check_normals_params(R, ctx):
    """target.normals reaches the estimation: k = 8 without orientation gives the rescoring's figures with those parameters, and not the defaults'"""
    c = PD.job_case(NAME); N = R.NormalsParams(8, 0)
    refs = References(R, ctx, False, N)
    try:
        outs, res = ctx.transcode_gof_d2(c["src"], params(R), stream_target(R, refs, normals=N))
        check_stream_result(R, ctx, refs, outs, res[1])
        dflt = ctx.transcode_gof_d2(c["src"], params(R), stream_target(R, refs))[1][1]
        assert dflt["frames"] != res[1]["frames"]
    finally:
        refs.release()


def check_job_arguments(R, ctx, make_ctx):
    """the refusals the D2 kinds add, and the pairing of submit and wait"""
    c = PD.job_case(NAME); PS = params(R); src = c["src"]
    refs = References(R, ctx, True)
    bare = [ctx.pcloud_upload(x) for x in PD.input_clouds(NAME)]          # handles without normals
    try:
        def refused(word, f):
            with pytest.raises(R.RbtError) as e: f()
            assert e.value.code == -4 and word in str(e.value), str(e.value)
        D, Pt = R.D2Target, R.PatchD2Target
        refused("no normals", lambda: ctx.submit_gof_d2(src, PS, [D(), D(c["atlas"], c["patches"], reference=bare)]))
        refused("no normals", lambda: ctx.submit_gof_d2_patches(src, PS, [Pt(), Pt(c["atlas"], c["patches"], reference=[refs.clouds[0], bare[1]])]))
        t = D(c["atlas"], c["patches"]); t.struct_size += 8
        refused("struct_size", lambda: ctx.submit_gof_d2(src, PS, [D(), t]))
        t = Pt(c["atlas"], c["patches"]); t.struct_size -= 4
        refused("struct_size", lambda: ctx.submit_gof_d2_patches(src, PS, [Pt(), t]))
        refused("k is", lambda: ctx.submit_gof_d2(src, PS, [D(), D(c["atlas"], c["patches"], normals=R.NormalsParams(2))]))
        refused("negative", lambda: ctx.submit_gof_d2(src, PS, [D(), D(c["atlas"], c["patches"], min_d2_mdb=-1)]))
        refused("stat", lambda: ctx.submit_gof_d2(src, PS, [D(), D(c["atlas"], c["patches"], stat=2)]))
        refused("non-geometry", lambda: ctx.submit_gof_d2(src, PS, [D(c["atlas"], c["patches"]), D()]))
        refused("occupancy source", lambda: ctx.submit_gof_d2(src[1:], PS[1:], [D(c["atlas"], c["patches"])]))
        other_ctx = make_ctx()
        try:
            foreign = other_ctx.pcloud_upload(PD.input_clouds(NAME)[0], None, ref_normals(0))
            refused("not a cloud of this context", lambda: ctx.submit_gof_d2(src, PS, [D(), D(c["atlas"], c["patches"], reference=[foreign, None])]))
        finally:
            other_ctx.close()
        alone_s = ctx.transcode_gof_d2(src, PS, stream_target(R, refs)); alone_p = ctx.transcode_gof_d2_patches(src, PS, patch_target(R, refs))
        old = ctx.get_depth(); ctx.set_depth(2)
        try:                                                              # a refused call took no job slot; a wrong wait leaves the job collectable
            js, jp = ctx.submit_gof_d2(src, PS, stream_target(R, refs)), ctx.submit_gof_d2_patches(src, PS, patch_target(R, refs))
            for job, wrongs in ((js, (ctx.wait_gof, ctx.wait_gof_d1, ctx.wait_gof_d2_patches, ctx.wait_gof_d1_patches)), (jp, (ctx.wait_gof, ctx.wait_gof_d2, ctx.wait_gof_d1_patches, ctx.wait_gof_quality_patches))):
                for wrong in wrongs:
                    with pytest.raises(R.RbtError) as e: wrong(job)
                    assert e.value.code == -4 and "collect" in str(e.value), str(e.value)
            got_p, got_s = ctx.wait_gof_d2_patches(jp), ctx.wait_gof_d2(js)
            jd = ctx.submit_gof_d1(src, PS, [R.D1Target(), R.D1Target(c["atlas"], c["patches"])])
            for wrong in (ctx.wait_gof_d2, ctx.wait_gof_d2_patches):     # ... and the D2 waits collect no other kind's job
                with pytest.raises(R.RbtError) as e: wrong(jd)
                assert e.value.code == -4
            ctx.wait_gof_d1(jd)
        finally:
            ctx.set_depth(old)
        assert got_s[0] == alone_s[0] and _plain(got_s[1]) == _plain(alone_s[1]) and got_p[0] == alone_p[0] and _plain(got_p[1]) == _plain(alone_p[1])
    finally:
        refs.release()
        for h in bare: h.release()


def check_jobs_in_flight(R, ctx, depth, n_jobs):
    """depth jobs in flight, the two kinds alternating, collected out of order: each returns what it returns alone"""
    c = PD.job_case(NAME); PS = params(R); src = c["src"]
    refs = References(R, ctx, True)
    old = ctx.get_depth(); ctx.set_depth(depth)
    try:
        rep = ctx.transcode_gof_d2(src, PS, stream_target(R, refs))[1][1]
        F = int((rep["min_d2"] - 0.5) * 1000)
        kinds = [("d2", stream_target(R, refs, min_d2_mdb=F, qp_min=28, qp_max=33)), ("d2_patches", patch_target(R, refs, min_d2_mdb=F, qp_min=28, qp_max=33, max_trials=2)),
                 ("d2", stream_target(R, refs))]
        alone = [getattr(ctx, "transcode_gof_" + k)(src, PS, t) for k, t in kinds]
        jobs = [getattr(ctx, "submit_gof_" + kinds[i % 3][0])(src, PS, kinds[i % 3][1]) for i in range(n_jobs)]
        with pytest.raises(R.RbtError) as e:
            ctx.submit_gof_d2(src, PS, kinds[0][1])
        assert e.value.code == -7         # RBT_ERR_BUSY
        for i in list(range(1, n_jobs, 2)) + list(range(0, n_jobs, 2))[::-1]:
            got = getattr(ctx, "wait_gof_" + kinds[i % 3][0])(jobs[i])
            assert got[0] == alone[i % 3][0] and _plain(got[1]) == _plain(alone[i % 3][1]), i
    finally:
        ctx.set_depth(old); refs.release()


def check_no_leak_between_kinds(R, ctx):
    """a D2 job beside a D1 job: D1 jobs before, between and after the D2 kinds return what they returned, and so do the D2 kinds"""
    c = PD.job_case(NAME); PS = params(R); src = c["src"]
    refs = References(R, ctx, True)
    try:
        d1 = lambda: (_plain(ctx.transcode_gof_d1(src, PS, [R.D1Target(), R.D1Target(c["atlas"], c["patches"], 60000, 0, 26, 34, 0, refs.arg())])),
                      _plain(ctx.transcode_gof_d1_patches(src, PS, [R.PatchD1Target(), R.PatchD1Target(c["atlas"], c["patches"], 60000, max_trials=2, reference=refs.arg())])))
        before = d1()
        s1 = ctx.transcode_gof_d2(src, PS, stream_target(R, refs, min_d2_mdb=60000, qp_min=26, qp_max=34))
        between = d1()
        p1 = ctx.transcode_gof_d2_patches(src, PS, patch_target(R, refs, min_d2_mdb=60000, max_trials=2))
        after = d1()
        assert before == between == after
        s2 = ctx.transcode_gof_d2(src, PS, stream_target(R, refs, min_d2_mdb=60000, qp_min=26, qp_max=34))
        p2 = ctx.transcode_gof_d2_patches(src, PS, patch_target(R, refs, min_d2_mdb=60000, max_trials=2))
        assert s1[0] == s2[0] and _plain(s1[1]) == _plain(s2[1]) and p1[0] == p2[0] and _plain(p1[1]) == _plain(p2[1])
        # the two kinds disagree where the figures do: a D2 frame is no D1 frame under another name
        assert s1[1][1]["frames"][0]["sse_ba"] != before[0][1][1]["frames"][0]["sse_ba"]
    finally:
        refs.release()
