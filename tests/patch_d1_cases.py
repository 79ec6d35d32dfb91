"""Cases and checks of D1 per patch of the decoded cloud (rbt_pcloud_set_labels, rbt_pcloud_labels, rbt_score_patches; csrc/rbt_score.h "patches"), shared by
tests/test_patch_d1.py (serial host emulation of the kernel bodies) and tests/test_gpu_patch_d1.py (the GPU build). The definition of include/rbt.h is restated by
brute force on a chunked distance matrix; the labels of a cloud made from maps are restated with the oracle's reconstruction, patch by patch."""
import ctypes
import numpy as np
import color_cases as CC
import pcc_cases as P
import score_cases as SC

F32, F64 = np.float32, np.float64
INTS = ("n_ab", "n_ba", "sse_ab", "sse_ba", "max_ab", "max_ba")
PEAK = 1023


# ---- the definition, by brute force ----
def definition(a, b, labels, n_patches, chunk=512):
    """-> int64 [n_patches, 6] in the order of INTS. Representative of a voxel: its lowest point index (np.unique returns the first occurrence)"""
    A = np.unique(np.asarray(a, np.int64), axis=0)
    B, ib = np.unique(np.asarray(b, np.int64), axis=0, return_index=True)
    lab = np.asarray(labels, np.int64)
    out = np.zeros((n_patches, 6), np.int64)
    mba = np.full(len(B), np.iinfo(np.int64).max, np.int64)
    for s in range(0, len(A), chunk):
        d = ((A[s:s + chunk, None, :] - B[None, :, :]) ** 2).sum(-1)
        mab = d.min(1)
        owner = np.where(d == mab[:, None], ib[None, :], np.iinfo(np.int64).max).min(1)      # the lowest point index among B's merged points at exactly the distance
        k = lab[owner]
        np.add.at(out[:, 0], k, 1); np.add.at(out[:, 2], k, mab); np.maximum.at(out[:, 4], k, mab)
        mba = np.minimum(mba, d.min(0))
    k = lab[ib]
    np.add.at(out[:, 1], k, 1); np.add.at(out[:, 3], k, mba); np.maximum.at(out[:, 5], k, mba)
    return out


_OFFSETS = {}


def _shells(rmax):
    """the offsets of the ball of radius rmax, grouped by squared length in ascending order"""
    if rmax not in _OFFSETS:
        g = np.mgrid[-rmax:rmax + 1, -rmax:rmax + 1, -rmax:rmax + 1].reshape(3, -1).T
        d2 = (g ** 2).sum(1); keep = d2 <= rmax * rmax
        g, d2 = g[keep], d2[keep]
        _OFFSETS[rmax] = [(int(v), g[d2 == v]) for v in np.unique(d2)]
    return _OFFSETS[rmax]


def _nearest_in_volume(Pts, vol, lo, rmax):
    """per point the least squared distance to a set voxel of vol (int64: the voxel's lowest point index, BIG where empty) and the lowest index among the voxels at
    exactly that distance; -1 where no voxel lies within rmax"""
    BIG = np.iinfo(np.int64).max
    best = np.full(len(Pts), -1, np.int64); owner = np.full(len(Pts), BIG, np.int64)
    for d2, offs in _shells(rmax):
        pend = np.nonzero(best < 0)[0]
        if len(pend) == 0: break
        base = Pts[pend] - lo
        o = np.full(len(pend), BIG, np.int64)
        for off in offs:
            q = base + off
            o = np.minimum(o, vol[q[:, 0], q[:, 1], q[:, 2]])
        hit = o < BIG
        best[pend[hit]] = d2; owner[pend[hit]] = o[hit]
    return best, owner


def definition_near(a, b, labels, n_patches, rmax=6):
    """`definition` for clouds that lie near each other: the same words from two dense volumes walked shell by shell (all offsets of one squared length at a time, so the
    first shell that hits holds the whole tie set); a point without a neighbour within rmax falls back to the distance matrix"""
    BIG = np.iinfo(np.int64).max
    A, ia = np.unique(np.asarray(a, np.int64), axis=0, return_index=True)
    B, ib = np.unique(np.asarray(b, np.int64), axis=0, return_index=True)
    lab = np.asarray(labels, np.int64)
    lo = np.minimum(A.min(0), B.min(0)) - rmax; shape = tuple(np.maximum(A.max(0), B.max(0)) - lo + rmax + 1)
    if np.prod(shape) > (1 << 27): return definition(a, b, labels, n_patches)
    va = np.full(shape, BIG, np.int64); va[tuple((A - lo).T)] = ia
    vb = np.full(shape, BIG, np.int64); vb[tuple((B - lo).T)] = ib
    mab, owner = _nearest_in_volume(A, vb, lo, rmax); mba, _ = _nearest_in_volume(B, va, lo, rmax)
    for i in np.nonzero(mab < 0)[0]:
        d = ((A[i] - B) ** 2).sum(1); mab[i] = d.min(); owner[i] = ib[d == d.min()].min()
    for j in np.nonzero(mba < 0)[0]:
        mba[j] = ((B[j] - A) ** 2).sum(1).min()
    out = np.zeros((n_patches, 6), np.int64)
    k = lab[owner]
    np.add.at(out[:, 0], k, 1); np.add.at(out[:, 2], k, mab); np.maximum.at(out[:, 4], k, mab)
    k = lab[ib]
    np.add.at(out[:, 1], k, 1); np.add.at(out[:, 3], k, mba); np.maximum.at(out[:, 5], k, mba)
    return out


def derived(sse_ab, sse_ba, n_ab, n_ba, peak):
    """the figures of one patch with the float routine of score_cases.geometry_derived: a direction without a point has mse 0, 3 peak^2 / 0 is +inf"""
    mab = F32(F64(sse_ab) / F64(n_ab)) if n_ab else F32(0)
    mba = F32(F64(sse_ba) / F64(n_ba)) if n_ba else F32(0)
    m = max(mab, mba)
    q = F32(3) * F32(peak) * F32(peak) / m if m > 0 else None
    return mab, mba, (F32(10) * F32(CC.LIBM.log10f(ctypes.c_float(float(q)))) if m > 0 else F32(np.inf))


# ---- clouds ----
def runs(n, length, n_patches=None):
    """labels in patch order, a new patch every `length` points"""
    lab = np.arange(n) // length
    return lab.astype(np.uint32), int(n_patches or lab.max() + 1)


def _base_b(n):
    a, _, _, b, _ = SC.base(1)
    return a, b[:n]


def _case_tie(first):
    """one reference point at distance 1 from two points of B that belong to two patches. pc_for_ties meets (5, 6, 5) before (5, 5, 6); the owner is the lower INDEX, so
    putting either first moves the A -> B term from one patch to the other"""
    pts = [[5, 5, 6], [5, 6, 5]] if first == 0 else [[5, 6, 5], [5, 5, 6]]
    return np.array([[5, 5, 5]], np.int16), np.array(pts + [[40, 40, 40]], np.int16), np.array([1, 0, 2], np.uint32), 3


def _case_duplicates():
    """patch 2 holds nothing but copies of points of patch 0: it has no representative, and the reference points next to its points go to patch 0"""
    a, b = _base_b(300)
    lab = np.concatenate([np.zeros(150), np.ones(150), np.full(40, 2)]).astype(np.uint32)
    return a, np.concatenate([b, b[:40]]), lab, 3


def _case_far(name):
    a, _, _, b, _ = SC.far_case(name)
    lab, n = runs(len(b), 97)
    return a, b, lab, n


def _case_boundary(name):
    a, _, _, b, _ = SC.boundary_cases()[name]
    lab, n = runs(len(b), 211)
    return a, b, lab, n


def _case_sizes(n, side):
    a, b = SC.base(1)[0], SC.base(1)[3]
    if side == "a": a = a[:n]
    else: b = b[:n]
    lab, k = runs(len(b), 37)                                              # 37 divides neither 64 nor 256: labels change in mid-wave
    return a, b, lab, k


def _case_mixed():
    """every lane another label, in no order: P = 64 with one point per patch ..."""
    a, b = _base_b(64)
    return a, b, np.random.default_rng(5).permutation(64).astype(np.uint32), 64


def _case_interleaved():
    """... and labels that alternate point by point over several waves"""
    a, b = _base_b(700)
    return a, b, (np.arange(700) % 3).astype(np.uint32), 3


def _case_gap():
    a, b = _base_b(500)
    lab = (np.arange(500) // 100).astype(np.uint32); lab[lab >= 2] += 1     # patch 2 has no point
    return a, b, lab, 7                                                     # ... and neither has patch 6, behind the last label


def _case_wide():
    a, b = _base_b(5)
    return a, b, np.array([0, 65535, 40000, 65535, 1], np.uint32), 65536


def _case_same():
    a = SC.base(0)[0]
    lab, n = runs(len(a), 500)
    return a, a.copy(), lab, n


def _case_one():
    return np.array([[7, 8, 9]], np.int16), np.array([[7, 8, 12]], np.int16), np.zeros(1, np.uint32), 1


def _case_single_patch():
    a, b = _base_b(1000)
    return a, b, np.zeros(1000, np.uint32), 1


SUM_CASES = {"one_point": _case_one, "single_patch": _case_single_patch, "one_point_per_patch": _case_mixed, "interleaved": _case_interleaved, "empty_patches": _case_gap,
             "duplicates_of_an_earlier_patch": _case_duplicates, "tie_lower_index_first": lambda: _case_tie(0), "tie_lower_index_second": lambda: _case_tie(1),
             "a_is_b": _case_same, "p65536": _case_wide}
SUM_CASES.update({"size_%d_%s" % (n, s): (lambda n=n, s=s: _case_sizes(n, s)) for n in (63, 64, 65, 255, 256, 257) for s in "ab"})
SUM_CASES.update({name: (lambda name=name: _case_far(name)) for name in SC.FAR})
SUM_CASES.update({name: (lambda name=name: _case_boundary(name)) for name in ("word_x23", "faces_x1023_y0")})

_REF = {}


def reference(name):
    if name not in _REF:
        a, b, lab, n = SUM_CASES[name]()
        _REF[name] = (a, b, lab, n, definition(a, b, lab, n))
    return _REF[name]


def score(ctx, a, b, lab, n, peak=PEAK, raw=False):
    """uploads, labels, scores per patch and as a whole, releases -> (patches, whole, rbt_score's d1)"""
    ha, hb = ctx.pcloud_upload(a), ctx.pcloud_upload(b)
    try:
        hb.set_labels(lab)
        assert np.array_equal(hb.labels(), lab)
        got, whole, ms = ctx.score_patches(ha, hb, n, peak, raw=raw)
        assert ms >= 0
        return got, whole, (None if raw else ctx.score(ha, hb, peak, SC.D1)["d1"])
    finally:
        ha.release(); hb.release()


def check_sums(ctx, name, other=None):
    a, b, lab, n, want = reference(name)
    got, whole, d1 = score(ctx, a, b, lab, n)
    ints = np.array([[g[k] for k in INTS] for g in got], np.int64)
    bad = np.nonzero((ints != want).any(1))[0]
    assert len(bad) == 0, (name, bad[:5], ints[bad[:5]], want[bad[:5]])
    for k in np.nonzero(want[:, :2].sum(1) > 0)[0].tolist() + [n - 1]:     # the floats of every patch with a point (and of the last one)
        g = got[k]
        assert (F32(g["mse_ab"]), F32(g["mse_ba"]), F32(g["psnr"])) == derived(g["sse_ab"], g["sse_ba"], g["n_ab"], g["n_ba"], PEAK), (name, k, g)
    empty = np.nonzero(want[:, :2].sum(1) == 0)[0]
    assert all(got[k]["psnr"] == np.inf and got[k]["mse_ab"] == 0 and got[k]["mse_ba"] == 0 for k in empty)
    # the invariants of the definition, against rbt_score
    assert whole == d1
    assert (ints[:, 2].sum(), ints[:, 3].sum(), ints[:, 0].sum(), ints[:, 1].sum()) == (d1["sse_ab"], d1["sse_ba"], d1["n_a"], d1["n_b"])
    assert (ints[:, 4].max(), ints[:, 5].max()) == (d1["max_ab"], d1["max_ba"])
    if len(a) * len(b) < 4e6 or name in SC.FAR: assert np.array_equal(definition_near(a, b, lab, n), want), name      # the replays' restatement agrees with the brute force
    if name.startswith("tie_"):                                             # the other owner would move the term: patch 1 holds the lower index in both orders
        assert (got[1]["n_ab"], got[1]["sse_ab"], got[0]["n_ab"]) == (1, 1, 0)
    if name == "duplicates_of_an_earlier_patch": assert got[2]["n_ba"] == 0 and got[2]["n_ab"] == 0 and got[0]["n_ab"] > 0
    if name == "a_is_b": assert ints[:, 2:].sum() == 0 and all(g["psnr"] == np.inf for g in got)
    if name in SC.FAR_SHIFTS: assert ints[:, 4:].max() > 32 * 32
    if other is not None:
        g2, w2, _ = score(other, a, b, lab, n)
        assert g2 == got and w2 == whole


def check_determinism(ctx):
    """two calls return the same words, floats included"""
    a, b, lab, n, _ = reference("size_257_b")
    x, y = score(ctx, a, b, lab, n, raw=True), score(ctx, a, b, lab, n, raw=True)
    assert bytes(x[0]) == bytes(y[0]) and bytes(x[1]) == bytes(y[1]) and x[0][0].n_ba > 0


def check_still_works(ctx):
    a, b, lab, n, want = reference("tie_lower_index_first")
    got = score(ctx, a, b, lab, n)[0]
    assert [[g[k] for k in INTS] for g in got] == want.tolist()


def check_score_arguments(R, ctx, make_ctx):
    a, b, lab, n = _case_tie(0)
    ha, hb, hplain = ctx.pcloud_upload(a), ctx.pcloud_upload(b), ctx.pcloud_upload(b)
    hb.set_labels(lab)
    other_ctx = make_ctx()
    try:
        foreign = other_ctx.pcloud_upload(b); foreign.set_labels(lab)
        bad = [lambda: ctx.score_patches(ha, foreign, n), lambda: ctx.score_patches(foreign, hb, n), lambda: ctx.score_patches(None, hb, n), lambda: ctx.score_patches(ha, None, n),
               lambda: ctx.score_patches(ha, hplain, n),                                        # b without labels
               lambda: ctx.score_patches(ha, hb, 2), lambda: ctx.score_patches(ha, hb, 1),      # a label >= n_patches
               lambda: ctx.score_patches(ha, hb, 0), lambda: ctx.score_patches(ha, hb, 65537), lambda: ctx.score_patches(ha, hb, -1),
               lambda: ctx.score_patches(ha, hb, n, peak=0),
               lambda: hplain.labels(),                                                        # a cloud without labels
               lambda: hplain.set_labels(np.array([0, 65536, 0], np.uint32))]                   # a label that is no patch index
        for f in bad:
            SC.refused(R, f)
            check_still_works(ctx)
        SC.refused(R, lambda: hplain.labels())                                                 # the refused labels were not kept
        # a refused call has written nothing the next one sees: the same handles score as fresh ones do
        want = definition(a, b, lab, n)
        assert [[g[k] for k in INTS] for g in ctx.score_patches(ha, hb, n)[0]] == want.tolist()
        assert [[g[k] for k in INTS] for g in ctx.score_patches(ha, hb, 65536)[0]][:3] == want.tolist()
        hb.set_labels(lab[::-1].copy())                                                        # new labels replace the old ones
        assert [[g[k] for k in INTS] for g in ctx.score_patches(ha, hb, n)[0]] == definition(a, b, lab[::-1], n).tolist()
    finally:
        other_ctx.close()
    for h in (ha, hb, hplain): h.release()


# ---- the labels of a cloud made from maps ----
def label_cases(R):
    """(name, case): seam and random atlases of 64 x 64 and 128 x 128, occupancy precision 1, 2 and 4, overlapping patch rectangles in the random ones"""
    out = [("seam64_p1", P.seam_atlas(R, 0, tiles=2, prec=1)), ("seam128_p2", P.seam_atlas(R, 1, tiles=4, prec=2)), ("seam128_p4_two_axes", P.seam_atlas(R, 5, tiles=4, prec=4, two_axes=True))]
    for seed, side in ((21, 64), (22, 64), (4, 128), (1, 128), (2, 128), (7, 128)):              # precision 2, 4, 1, 2, 4; 7: lossy occupancy. (Seeds whose clouds stay inside 0..1023)
        case = list(P.random_atlas(R, seed, side, side))
        case[0] = P._copy_atlas(R, case[0], geometry_smoothing=1, grid_size=8, threshold_smoothing=64)
        out.append(("random%d_%d" % (side, seed), tuple(case)))
    return out


LABEL_CASES = ["seam64_p1", "seam128_p2", "seam128_p4_two_axes", "random64_21", "random64_22", "random128_4", "random128_1", "random128_2", "random128_7"]


def overlapping(patches):
    def rect(p):
        sw, sh = (p.size_v0, p.size_u0) if p.orientation in (1, 5, 6, 7) else (p.size_u0, p.size_v0)
        return p.u0, p.v0, p.u0 + sw, p.v0 + sh
    r = [rect(p) for p in patches]
    return any(a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3] for i, a in enumerate(r) for b in r[i + 1:])


def check_labels(R, ctx, name, other=None):
    import oracle_lib as O
    case = dict(label_cases(R))[name]
    atlas, patches, occ, d0, d1 = case[:5]
    plain = (P._copy_atlas(R, atlas, geometry_smoothing=0),) + tuple(case[1:])
    h, host = ctx.pcloud_from_maps(*plain, host_copy=True)
    hs, moved = ctx.pcloud_from_maps(*case, host_copy=True)
    try:
        lab, smoothed = h.labels(), hs.labels()
    finally:
        h.release(); hs.release()
    xyz, b2p = host[0], host[3]
    res, prec = atlas.occupancy_resolution, atlas.occupancy_precision
    assert len(lab) == len(xyz) > 0 and lab.max() < len(patches)
    parts = []
    for k in range(len(patches)):
        own = np.kron(b2p == k + 1, np.ones((res // prec, res // prec), bool))                   # ownership as the host copy states it; every other block's occupancy cleared
        want = O.reconstruct(plain[0], patches, np.where(own, occ, 0).astype(np.uint16), d0, d1, *case[5:])[0]
        assert np.array_equal(xyz[lab == k], want), (name, k)
        parts.append(want)
    assert np.array_equal(np.concatenate(parts), xyz)
    assert name.startswith("random") or (ctx.n_smoothed > 0 and not np.array_equal(moved[0], xyz))     # the seams are there to be smoothed
    assert np.array_equal(smoothed, lab)                                                        # smoothing moves points; order and patch stay
    if name.startswith("random128"): assert overlapping(patches)
    if other is not None:
        ho = other.pcloud_from_maps(*case)
        try: assert np.array_equal(ho.labels(), lab)
        finally: ho.release()


def check_labels_score(R, ctx, other=None):
    """a cloud made from maps scores per patch with the labels it carries: against the definition, with the decoded cloud's own positions and labels read back"""
    case = P.seam_atlas(R, 3, tiles=2)
    src = (P._copy_atlas(R, case[0], geometry_smoothing=0),) + tuple(case[1:])
    hb, host = ctx.pcloud_from_maps(*case, host_copy=True)
    ha, hsrc = ctx.pcloud_from_maps(*src, host_copy=True)
    try:
        lab = hb.labels(); n = len(case[1])
        got, whole, _ = ctx.score_patches(ha, hb, n)
        assert [[g[k] for k in INTS] for g in got] == definition(hsrc[0], host[0], lab, n).tolist() and whole == ctx.score(ha, hb, PEAK, SC.D1)["d1"] and whole["sse_ba"] > 0
    finally:
        ha.release(); hb.release()
    if other is not None:
        hb2, ha2 = other.pcloud_from_maps(*case), other.pcloud_from_maps(*src)
        try: assert other.score_patches(ha2, hb2, n)[:2] == (got, whole)
        finally: ha2.release(); hb2.release()


def check_no_patches(R, ctx):
    case = list(P.seam_atlas(R, 0, tiles=2)); case[1] = []
    SC.refused(R, lambda: ctx.pcloud_from_maps(*case))
    check_still_works(ctx)


# ------------------------------------------------------------------------------------------------ D1 floors held patch by patch (rbt_submit_gof_d1_patches)
# Every trial of the replay is a transcode_gof_qp_map of the whole GOF with the frame's trial map, decoded by the oracle, reconstructed by the oracle through the output
# atlas, labelled patch by patch with the oracle (one reconstruction per patch, the other blocks' occupancy cleared) and summed by `definition`.
import functools
import math
import pytest
import oracle_lib as O
import frame_qp_cases as FC
import d1_floor_cases as DC
from frame_qp_cases import variant

QP = FC.QP
luma = DC.luma


@functools.lru_cache(maxsize=None)
def job_case(name):
    """-> dict as d1_floor_cases.case: src [occupancy stream, geometry stream], atlas (the OUTPUT atlas, precision 4), patches per frame, w, h, n_frames
    seam128 / seam128_smooth: 128 x 128, 16 patches of one CTB of 32 each, 2 frames (the second 4 depth levels higher); seam96 / seam96_smooth: d1_floor_cases' 96 x 96;
    seam96x80: the upper 96 x 80 of it with the six patches that lie inside - CTBs of 64 are partial on both edges; hole: seam96 with a patch whose blocks hold no occupied sample"""
    import rbt_lib
    R = rbt_lib.module()
    if name.startswith("seam128"):
        atlas, patches, occ, d0, d1, *_ = P.seam_atlas(R, 0, tiles=4, prec=2, noise=3)
        w = h = 128
        up = lambda d: np.clip(d.astype(np.int64) + 16, 0, 1023).astype(np.uint16)
        geo = np.stack([DC._yuv(d0), DC._yuv(d1), DC._yuv(up(d0)), DC._yuv(up(d1))])
        occ_frames = np.stack([DC._yuv(occ, 8), DC._yuv(occ, 8)])
        src = [O.encode(occ_frames, w // 2, h // 2, 8, 8, gop=1, i_qp_offset=0, lossless=1, log2_ctb=5, rows_per_slice=0)[0], O.encode_hm(geo, w, h, 10, 16)[0]]
        out = P._copy_atlas(R, atlas, occupancy_precision=4, geometry_smoothing=int(name.endswith("smooth")))
        return dict(src=src, atlas=out, patches=[patches, patches], w=w, h=h, n_frames=2)
    if name in ("seam96", "seam96_smooth"):
        return DC.case("seam" if name == "seam96" else "seam_smooth")
    if name in ("seam96x80", "hole"):
        atlas, patches, occ, d0, d1, *_ = P.seam_atlas(R, 0, tiles=3, prec=2)
        w, h = (96, 80) if name == "seam96x80" else (96, 96)
        patches = [p for p in patches if (p.v0 + p.size_v0) * 16 <= h]
        occ, d0, d1 = occ[:h // 2, :w // 2].copy(), d0[:h, :w], d1[:h, :w]
        if name == "hole": occ[0:16, 16:32] = 0                           # patch 1 contributes no point
        geo = np.stack([DC._yuv(d0), DC._yuv(d1), DC._yuv(d0 + 8), DC._yuv(d1 + 8)])
        occ_frames = np.stack([DC._yuv(occ, 8), DC._yuv(occ, 8)])
        src = [O.encode(occ_frames, w // 2, h // 2, 8, 8, gop=1, i_qp_offset=0, lossless=1, log2_ctb=5, rows_per_slice=0)[0], O.encode_hm(geo, w, h, 10, 16)[0]]
        out = P._copy_atlas(R, atlas, width=w, height=h, occupancy_precision=4, geometry_smoothing=0)
        return dict(src=src, atlas=out, patches=[patches, patches], w=w, h=h, n_frames=2)
    raise KeyError(name)


def job_params(R, v, qp=QP):
    return [FC.occ_params(R), FC.params(R, "geo", v, qp)]


def oracle_cloud(atlas, patches, occ, d0, d1):
    """the oracle's cloud with the patch of every point: per patch the points of a reconstruction in which only the blocks it owns keep their occupancy, by count"""
    import rbt_lib
    R = rbt_lib.module()
    xyz, _, _, b2p = O.reconstruct(atlas, patches, occ, d0, d1, 10)
    plain = P._copy_atlas(R, atlas, geometry_smoothing=0)
    s = atlas.occupancy_resolution // atlas.occupancy_precision
    counts = [len(O.reconstruct(plain, patches, np.where(np.kron(b2p == k + 1, np.ones((s, s), bool)), occ, 0).astype(np.uint16), d0, d1, 10)[0]) for k in range(len(patches))]
    assert sum(counts) == len(xyz)
    return xyz, np.repeat(np.arange(len(patches)), counts).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def input_clouds(name):
    c = job_case(name); w, h = c["w"], c["h"]
    om, ow, oh, *_ = O.decode(c["src"][0]); g = O.decode(c["src"][1])[0]
    a = P._copy_atlas(__import__("rbt_lib").module(), c["atlas"], occupancy_precision=w // ow)
    return [O.reconstruct(a, c["patches"][f], luma(om[f], ow, oh), luma(g[2 * f], w, h), luma(g[2 * f + 1], w, h), 10)[0] for f in range(c["n_frames"])]


def trial_figures(name, occ_stream, geo_stream, refs, frames=None):
    """per frame (rows of `definition`, the figures as Python floats, the whole frame's O.d1) of the decoded pair of streams against refs"""
    c = job_case(name); w, h = c["w"], c["h"]
    om, ow, oh, *_ = O.decode(occ_stream); g = O.decode(geo_stream)[0]
    out = {}
    for f in (range(c["n_frames"]) if frames is None else frames):
        xyz, lab = oracle_cloud(c["atlas"], c["patches"][f], luma(om[f], ow, oh), luma(g[2 * f], w, h), luma(g[2 * f + 1], w, h))
        rows = definition_near(refs[f], xyz, lab, len(c["patches"][f]))
        out[f] = (rows, [float(derived(r[2], r[3], r[0], r[1], PEAK)[2]) for r in rows], O.d1(refs[f], xyz, PEAK))
    return out


@functools.lru_cache(maxsize=None)
def premise(name="seam128", rd=0):
    """on the oracle alone: the figure of every patch of every frame in the oracle's constant-QP transcode at QP"""
    c = job_case(name)
    o = O.transcode_data(c["src"], [DC.OCC_P, (1, QP, 4, 5, -1, 0, rd, 0)])
    t = trial_figures(name, o[0], o[1], input_clouds(name))
    return [t[f][1] for f in range(c["n_frames"])]


def main_floor():
    """a floor, in 1/1000 dB, that every frame's figures at q0 straddle - a patch below it and one at least 1 dB above -, 0.05 dB or more from each of them"""
    figs = premise()
    for f in range(int(min(map(min, figs)) * 1000), int(max(map(max, figs)) * 1000), 7):
        F = f / 1000.0
        if all(min(fr) < F and max(x for x in fr if math.isfinite(x)) >= F + 1 for fr in figs) and all(abs(x - F) >= 0.05 for fr in figs for x in fr):
            return f
    raise AssertionError("the atlas gives no floor with a patch below and a patch 1 dB above it in every frame: %r" % (figs,))


def check_main_premise():
    figs = premise(); F = main_floor() / 1000.0
    print("figures at q0", [[round(x, 2) for x in fr] for fr in figs], "floor", F)
    for fr in figs:
        assert min(fr) < F and max(x for x in fr if math.isfinite(x)) >= F + 1


def d1_target(R, name, refs=None, **kw):
    c = job_case(name)
    return R.PatchD1Target(kw.pop("atlas", c["atlas"]), kw.pop("patches", c["patches"]), reference=refs, **kw)


def run_job(R, ctx, name, v, refs=None, **kw):
    outs, res = ctx.transcode_gof_d1_patches(job_case(name)["src"], job_params(R, v), [R.PatchD1Target(), d1_target(R, name, refs, **kw)])
    return outs, res[1]


def run_map(R, ctx, name, M, v):
    return ctx.transcode_gof_qp_map(job_case(name)["src"], job_params(R, v), [None, M])


def replay(R, ctx, name, v, ref_clouds, min_d1_mdb=0, qp_min=0, qp_max=0, background_qp=-1, max_trials=0, patch_floors=None):
    """rules 4 - 6 of the PSNR floors held patch by patch with the D1 figure, frame by frame and trial by trial -> per frame a dict, the final map, q0"""
    c = job_case(name); w, h, n = c["w"], c["h"], c["n_frames"]; l2 = dict(v)["log2_ctb"]; ctb = 1 << l2; hc, wc = -(-h // ctb), -(-w // ctb)
    any_floor = min_d1_mdb != 0 or any(x for fl in (patch_floors or []) if fl is not None for x in fl)
    lo, hi = (qp_min, qp_max or 51) if any_floor else (QP, QP)
    q0 = min(hi, max(lo, QP)); bg = q0 if background_qp < 0 else background_qp
    lib = __import__("qp_map_cases")._lib(R)
    frames, final = [], np.full((n, hc, wc), q0, np.int8)
    for f in range(n):
        pats = c["patches"][f]
        floors = list(patch_floors[f]) if patch_floors is not None and patch_floors[f] is not None else [min_d1_mdb] * len(pats)
        q, failed, trials = [q0] * len(pats), [0] * len(pats), 0
        while True:
            m = R.qp_map_from_patches(c["atlas"], pats, q, bg, l2, lib=lib)
            M = final.copy(); M[f] = m
            o = run_map(R, ctx, name, M, v)
            rows, fig, whole = trial_figures(name, o[0], o[1], ref_clouds, [f])[f]
            ok = [x >= F / 1000.0 for x, F in zip(fig, floors)]
            trials += 1
            for k in range(len(pats)): failed[k] |= int(not ok[k])
            if max_trials and trials >= max_trials: break
            new = list(q)
            for k in range(len(pats)):
                F = floors[k] / 1000.0
                if not ok[k]:
                    if q[k] > lo: new[k] = max(lo, q[k] - max(1, int(min(64.0, F - fig[k]))))
                elif not failed[k] and q[k] < hi and math.isfinite(fig[k]) and int(min(64.0, fig[k] - F)) >= 1:
                    new[k] = min(hi, q[k] + int(min(64.0, fig[k] - F)))
            if new == q: break
            q = new
        final[f] = m
        frames.append(dict(n_trials=trials, q=q, failed=failed, rows=rows, fig=fig, ok=ok, whole=whole, met=int(all(ok))))
    return frames, final, q0


def _plain(x):
    if isinstance(x, dict): return {k: (0.0 if k == "cloud_ms" else _plain(v)) for k, v in x.items()}
    if isinstance(x, (list, tuple)): return [_plain(v) for v in x]
    return x.tolist() if hasattr(x, "tolist") else x


def check_against_replay(R, ctx, name, v, other=None, uploaded=(), **kw):
    """the library's result is the replay's; the stream is transcode_gof_qp_map's for the final map. uploaded: the frames whose reference is an uploaded handle (a cloud
    moved by one voxel, so that it is not the decoded input's)"""
    c = job_case(name); n = c["n_frames"]
    ref_clouds = [(a + np.array([1, 0, 0], np.int16)).astype(np.int16) if f in uploaded else a for f, a in enumerate(input_clouds(name))]

    def run_with(cx):
        hs = [cx.pcloud_upload(ref_clouds[f]) if f in uploaded else None for f in range(n)]
        try: return run_job(R, cx, name, v, hs if uploaded else None, **kw)
        finally:
            for hh in hs:
                if hh is not None: hh.release()
    outs, res = run_with(ctx)
    frames, final, q0 = replay(R, ctx, name, v, ref_clouds, **kw)
    assert res["n_frames"] == n == len(res["frames"]) and res["qp_probe"] == q0 and res["cloud_ms"] >= 0
    assert np.array_equal(res["map"], final), (res["map"], final)
    for f, (want, got) in enumerate(zip(frames, res["frames"])):
        assert (got["n_trials"], got["met"], got["n_patches"]) == (want["n_trials"], want["met"], len(want["q"])), (f, got, want)
        for k, p in enumerate(got["patches"]):
            assert (p["qp"], p["failed"], p["met"]) == (want["q"][k], want["failed"][k], int(want["ok"][k])), (f, k, p, want)
            assert [p["d1"][x] for x in INTS] == want["rows"][k].tolist(), (f, k, p["d1"], want["rows"][k])
            assert p["figure"] == want["fig"][k] == float(F32(p["d1"]["psnr"])), (f, k, p, want["fig"][k])
        assert [got["d1"][x] for x in DC.INT_FIELDS] == [want["whole"][x] for x in DC.INT_FIELDS], (f, got["d1"], want["whole"])
    assert res["n_passes"] == max(x["n_trials"] for x in frames) and res["pictures_encoded"] == 2 * sum(x["n_trials"] for x in frames)
    want_streams = run_map(R, ctx, name, final, v)
    assert outs == want_streams and res["bytes"] == len(outs[1]) and res["met_all"] == int(all(x["met"] for x in frames))
    assert [x["bytes"] for x in res["frames"]] == FC.frame_sizes(outs[1])
    if dict(v)["md5_sei"]:
        got = O.decode(outs[1])
        assert (got[4], got[5]) == (2 * n, 0)                            # the oracle's decoder accepted every picture's MD5
    if other is not None:
        o_outs, o_res = run_with(other)
        assert o_outs == outs and _plain(o_res) == _plain(res)
    return outs, res, frames


REPORT_CASES = [("seam128", variant(), 0), ("seam96_smooth", variant(md5_sei=1), 0), ("seam96", variant(occupancy_rd=1), 1)]


def check_report(R, ctx, k, other=None):
    """floor 0: one trial at the entry's QP with the uniform map; every patch's words are the definition's on the oracle's decode and reconstruction; the frame's D1 is
    rbt_transcode_gof_d1's at the same QP"""
    name, v, rd = REPORT_CASES[k]
    outs, res, frames = check_against_replay(R, ctx, name, v, other=other)
    c = job_case(name)
    assert res["n_passes"] == 1 and res["pictures_encoded"] == 2 * c["n_frames"] and res["met_all"] == 1 and res["qp_probe"] == QP and (res["map"] == QP).all()
    assert all(p["met"] == 1 and p["failed"] == 0 and p["qp"] == QP for fr in res["frames"] for p in fr["patches"])
    d_outs, d_res = ctx.transcode_gof_d1(c["src"], job_params(R, v), [R.D1Target(), R.D1Target(c["atlas"], c["patches"], 0, 0, 0, 0, 0, None)])
    assert [fr["d1"] for fr in res["frames"]] == d_res[1]["frames"]
    assert O.decode(d_outs[1])[0].tobytes() == O.decode(outs[1])[0].tobytes()      # (the stream of a uniform map carries cu_qp_delta_enabled_flag: the pictures are the same)


def check_main_walk(R, ctx, other=None):
    F = main_floor()
    outs, res, frames = check_against_replay(R, ctx, "seam128", variant(md5_sei=1), other=other, min_d1_mdb=F)
    for fr in res["frames"]:
        qs = [p["qp"] for p in fr["patches"]]
        assert min(qs) < QP < max(qs), qs
    print("trials", [fr["n_trials"] for fr in res["frames"]], "met", res["met_all"], "QPs", [[p["qp"] for p in fr["patches"]] for fr in res["frames"]])


def _mixed(name, lo_f, hi_f):
    c = job_case(name)
    return [None if f == c["n_frames"] - 1 else [(hi_f, lo_f)[(k + f) % 2] for k in range(len(c["patches"][f]))] for f in range(c["n_frames"])]


def replay_cases():
    F = main_floor()
    return [
        ("seam96", variant(md5_sei=1), dict(min_d1_mdb=F), dict(uploaded=(1,))),                                      # an uploaded reference handle beside a NULL one
        ("seam96_smooth", variant(md5_sei=1), dict(min_d1_mdb=F, max_trials=3), {}),                                   # geometry smoothing on
        ("seam96", variant(occupancy_rd=1, md5_sei=1), dict(min_d1_mdb=F, max_trials=3), {}),                          # occupancy_rd
        ("seam96", variant(), dict(min_d1_mdb=F - 2000, patch_floors=_mixed("seam96", F - 3000, F + 1500), max_trials=4), {}),   # floors that differ within a frame
        ("seam96", variant(md5_sei=1), dict(min_d1_mdb=F, background_qp=51, max_trials=3), {}),
        ("seam96", variant(md5_sei=1, log2_ctb=4, rows_per_slice=1), dict(min_d1_mdb=F, max_trials=3), {}),            # CTBs of 16, one-row slices
        ("seam96x80", variant(md5_sei=1, log2_ctb=6, rows_per_slice=0), dict(min_d1_mdb=F, max_trials=3), {}),         # CTBs of 64 on 96 x 80
    ]


N_REPLAY = 7


def check_replay(R, ctx, k, other=None):
    name, v, kw, extra = replay_cases()[k]
    outs, res, frames = check_against_replay(R, ctx, name, v, other=other, **kw, **extra)
    assert max(x["n_trials"] for x in frames) >= 2                      # the case walks
    if kw.get("background_qp") == 51: assert (res["map"] == 51).any() or dict(v)["log2_ctb"] == 5


def check_edges(R, ctx, other=None):
    v = variant(); F = main_floor()
    # a floor nothing reaches: every patch with a point ends at lo with met 0, the call returns RBT_OK, the stream is the map's
    outs, res, frames = check_against_replay(R, ctx, "seam96", v, other=other, min_d1_mdb=150000, qp_min=27, qp_max=33)
    assert res["met_all"] == 0 and all(p["qp"] == 27 and p["met"] == 0 and p["failed"] == 1 for fr in res["frames"] for p in fr["patches"])
    # a QP range of one: one trial
    outs, res, frames = check_against_replay(R, ctx, "seam96", v, min_d1_mdb=F, qp_min=QP, qp_max=QP)
    assert res["n_passes"] == 1 and all(fr["n_trials"] == 1 for fr in res["frames"])
    # max_trials 1 and 2: the result is the last trial's, met as measured
    for cap in (1, 2):
        outs, res, frames = check_against_replay(R, ctx, "seam128", v, other=other if cap == 2 else None, min_d1_mdb=F, max_trials=cap)
        assert res["n_passes"] == cap and all(fr["n_trials"] <= cap for fr in res["frames"])
        if cap == 1: assert res["met_all"] == 0 and (res["map"] == QP).all()
    # a patch that contributes no point and owns no reference point: +inf, it meets and stays
    outs, res, frames = check_against_replay(R, ctx, "hole", v, other=other, min_d1_mdb=F, max_trials=3)
    for fr in res["frames"]:
        p = fr["patches"][1]
        assert (p["d1"]["n_ab"], p["d1"]["n_ba"], p["met"], p["qp"]) == (0, 0, 1, QP) and p["figure"] == float("inf")


def check_job_arguments(R, ctx, make_ctx):
    """every refusal is RBT_ERR_PARAM with its reason, submits nothing and leaves the context usable; the pairing of submit and wait"""
    c = job_case("seam96"); occ, geo = c["src"]; v = variant(); PS = job_params(R, v); E = R.PatchD1Target

    def refused(word, streams, ps, ts):
        with pytest.raises(R.RbtError) as e:
            ctx.transcode_gof_d1_patches(streams, ps, ts)
        assert e.value.code == -4 and word in str(e.value), str(e.value)

    def tgt(**kw):
        return d1_target(R, "seam96", kw.pop("refs", None), **kw)
    bad = tgt(); bad.struct_size += 8
    refused("struct_size", [occ, geo], PS, [E(), bad])
    refused("occupancy source", [geo], PS[1:], [tgt()])                                   # the D1 section's: no pooled occupancy entry in front
    refused("n_frames", [occ, geo], PS, [E(), tgt(patches=c["patches"][:1])])            # not pictures / 2
    a = P._copy_atlas(R, c["atlas"], width=128)
    refused("atlas", [occ, geo], PS, [E(), tgt(atlas=a)])
    a = P._copy_atlas(R, c["atlas"], occupancy_precision=2)
    refused("occupancy_precision", [occ, geo], PS, [E(), tgt(atlas=a)])
    a = P._copy_atlas(R, c["atlas"], map_count=1)
    refused("map_count", [occ, geo], PS, [E(), tgt(atlas=a)])
    for bq in (-2, 52): refused("background_qp", [occ, geo], PS, [E(), tgt(background_qp=bq)])
    refused("max_trials", [occ, geo], PS, [E(), tgt(max_trials=-1)])
    refused("negative", [occ, geo], PS, [E(), tgt(min_d1_mdb=-1)])
    refused("negative", [occ, geo], PS, [E(), tgt(patch_floors=[None, [-5] * len(c["patches"][1])])])
    refused("peak", [occ, geo], PS, [E(), tgt(peak=-1)])
    refused("QP range", [occ, geo], PS, [E(), tgt(qp_min=40, qp_max=30)])
    refused("non-geometry", [occ, geo], PS, [tgt(), E()])                                  # a target on an occupancy entry
    refused("non-geometry", [occ, geo], [PS[0], FC.params(R, "attr", v)], [E(), tgt()])    # ... and on an attribute entry
    t = tgt(); t.n_patches = None
    refused("patch list", [occ, geo], PS, [E(), t])
    other_ctx = make_ctx()
    try:
        foreign = other_ctx.pcloud_upload(input_clouds("seam96")[0])
        refused("not a cloud of this context", [occ, geo], PS, [E(), tgt(refs=[foreign, None])])
    finally:
        other_ctx.close()
    rd = [FC.occ_params(R), R.StreamParams(1, QP, 4, 5, -1, 0, 1, 1, 0)]                   # occupancy_rd together with verify_md5
    refused("verify_md5", [occ, geo], rd, [E(), tgt()])
    F = main_floor(); alone = run_job(R, ctx, "seam96", v, min_d1_mdb=F, max_trials=2)
    old = ctx.get_depth(); ctx.set_depth(1)
    try:                                                                   # a refused call took no job slot; the wrong wait leaves the job collectable
        job = ctx.submit_gof_d1_patches([occ, geo], PS, [E(), tgt(min_d1_mdb=F, max_trials=2)])
        for wrong in (ctx.wait_gof, ctx.wait_gof_d1, ctx.wait_gof_d1_frames, ctx.wait_gof_quality_patches):
            with pytest.raises(R.RbtError) as e:
                wrong(job)
            assert e.value.code == -4 and "collect" in str(e.value)
        assert ctx.job_memory(job) > 0
        outs, res = ctx.wait_gof_d1_patches(job)
        other_job = ctx.submit_gof([occ, geo], PS)
        with pytest.raises(R.RbtError) as e:
            ctx.wait_gof_d1_patches(other_job)
        assert e.value.code == -4
        plain = ctx.wait_gof(other_job)
    finally:
        ctx.set_depth(old)
    assert outs == alone[0] and _plain(res[1]) == _plain(alone[1]) and plain == ctx.transcode_gof([occ, geo], PS)
    assert (res[0]["n_frames"], res[0]["map"], res[0]["frames"], res[0]["bytes"]) == (0, None, [], len(outs[0]))      # an entry without a target
    with pytest.raises(R.RbtError):                                        # a corrupt input fails in the wait half, and the context goes on
        ctx.transcode_gof_d1_patches([occ, geo[:len(geo) // 2]], PS, [E(), tgt()])
    assert ctx.transcode_gof([occ, geo], PS) == plain


def check_jobs_in_flight(R, ctx, depth, n_jobs):
    old = ctx.get_depth(); ctx.set_depth(depth)
    try:
        c = job_case("seam96"); v = variant(); PS = job_params(R, v); F = main_floor()
        floors = [F - 1500 + 500 * (k % 6) for k in range(n_jobs)]
        mk = lambda f: [R.PatchD1Target(), d1_target(R, "seam96", min_d1_mdb=f, max_trials=2)]
        jobs = [ctx.submit_gof_d1_patches(c["src"], PS, mk(floors[k])) for k in range(n_jobs)]
        with pytest.raises(R.RbtError) as e:
            ctx.submit_gof_d1_patches(c["src"], PS, mk(F))
        assert e.value.code == -7         # RBT_ERR_BUSY
        got = {}
        for k in list(range(1, n_jobs, 2)) + list(range(0, n_jobs, 2))[::-1]:
            got[k] = ctx.wait_gof_d1_patches(jobs[k])
        alone = {}
        for k in range(n_jobs):
            f = floors[k]
            if f not in alone: alone[f] = ctx.transcode_gof_d1_patches(c["src"], PS, mk(f))
            assert got[k][0] == alone[f][0] and _plain(got[k][1]) == _plain(alone[f][1]), k
        assert len({o[0][1] for o in got.values()}) >= 2
    finally:
        ctx.set_depth(old)


def check_two_gofs(R, ctx, other=None):
    """two GOFs in one job: the entries share pipelines by video type; two carry targets. An entry in company gives what it gives alone"""
    v = variant(md5_sei=1); F = main_floor(); a, b = job_case("seam96"), job_case("seam128")
    streams = a["src"] + b["src"]; ps = job_params(R, v) + job_params(R, v); E = R.PatchD1Target
    kws = {1: dict(min_d1_mdb=F, max_trials=2), 3: dict(min_d1_mdb=F - 1000, max_trials=3, background_qp=45)}
    ts = [E(), d1_target(R, "seam96", **kws[1]), E(), d1_target(R, "seam128", **kws[3])]
    outs, res = ctx.transcode_gof_d1_patches(streams, ps, ts)
    for i, name in ((1, "seam96"), (3, "seam128")):
        a_outs, a_res = run_job(R, ctx, name, v, **kws[i])
        assert outs[i - 1:i + 1] == a_outs and _plain(res[i]) == _plain(a_res), i
        got = O.decode(outs[i])
        assert (got[4], got[5]) == (4, 0)
    if other is not None:
        o_outs, o_res = other.transcode_gof_d1_patches(streams, ps, ts)
        assert o_outs == outs and _plain(o_res) == _plain(res)


def check_no_leak_between_kinds(R, ctx):
    """a job of every older kind before and after in the same context: each returns what it returned before"""
    c = job_case("seam96"); v = variant(); PS = job_params(R, v); F = main_floor()
    d1t = lambda f: [R.D1Target(), R.D1Target(c["atlas"], c["patches"], f, 0, 24, 40, 0, None)]
    pft = [R.PatchFloorTarget(), R.PatchFloorTarget(c["atlas"], c["patches"], 46000, max_trials=2)]

    def older():
        return [ctx.transcode_gof(c["src"], PS), _plain(ctx.transcode_gof_rate(c["src"], PS, [R.RateTarget(), R.RateTarget(len(c["src"][1]) // 2)])),
                _plain(ctx.transcode_gof_quality(c["src"], PS, [R.QualityTarget(), R.QualityTarget(45000)])), _plain(ctx.transcode_gof_d1(c["src"], PS, d1t(F))),
                _plain(ctx.transcode_gof_d1_frames(c["src"], PS, d1t(F))), _plain(ctx.transcode_gof_quality_patches(c["src"], PS, pft)),
                ctx.transcode_gof_qp_map(c["src"], PS, [None, np.full((2, 3, 3), 33, np.int8)])]
    before = older()
    mine = run_job(R, ctx, "seam96", v, min_d1_mdb=F, max_trials=2)
    after = older()
    assert before == after
    again = run_job(R, ctx, "seam96", v, min_d1_mdb=F, max_trials=2)
    assert again[0] == mine[0] and _plain(again[1]) == _plain(mine[1])
