"""Cases and checks of the frame scoring on device clouds (rbt_pcloud_*, rbt_score, rbt_score_summary; csrc/rbt_score.h), shared by tests/test_score.py (serial host
emulation of the kernel bodies) and tests/test_gpu_score.py (the GPU build). The definitions are restated by brute force: color_cases.merge / one_way / derived for the
colour part, pcc_cases.d2_brute_force for D2, a distance matrix for D1. A case's reference is computed once per process and shared."""
import ctypes
import numpy as np
import pytest
import color_cases as CC
import pcc_cases as P

F32, F64 = np.float32, np.float64
D1, D2, COLOR = 1, 2, 4
OUTLIERS = np.array([[900, 40, 300], [0, 0, 0], [1023, 1023, 1023]], np.int16)
OUTLIER_RGB = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
OUTLIER_NRM = np.array([[16384, 0, 0], [0, -16384, 0], [9459, 9459, 9459]], np.int16)


def normals(seed, n):
    """as pcc_cases.d2_cases makes them: even seeds slanted unit vectors, odd seeds axis normals (Q14)"""
    r = np.random.default_rng(40 + seed)
    if seed % 2:
        out = np.zeros((n, 3), np.int16); out[np.arange(n), r.integers(0, 3, n)] = 16384 * r.choice([-1, 1], n)
        return out
    v = r.normal(size=(n, 3))
    return np.round(16384 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.int16)


_BASE = []


def base(k):
    """base cloud k: (a, rgb_a, normals_a, b, rgb_b) - color_cases.metric_cases() with seeded normals"""
    if not _BASE:
        for seed, (a, ca, b, cb) in enumerate(CC.metric_cases()):
            _BASE.append((a, ca, normals(seed, len(a)), b, cb))
    return _BASE[k]


def moved(case, da, db):
    a, ca, na, b, cb = case
    return (a + np.array(da, np.int16)).astype(np.int16), ca, na, (b + np.array(db, np.int16)).astype(np.int16), cb


def boundary_cases():
    """base cloud 0 translated so that x starts at 23 (the cloud then crosses the 32-voxel word at x = 31 | 32), and so that x ends at 1023 while y starts at 0"""
    a, _, _, b, _ = base(0)
    lo = np.minimum(a.min(0), b.min(0)).astype(int); hi = np.maximum(a.max(0), b.max(0)).astype(int)
    one = moved(base(0), (23 - lo[0], 0, 0), (23 - lo[0], 0, 0))
    two = moved(base(0), (1023 - hi[0], -lo[1], 0), (1023 - hi[0], -lo[1], 0))
    assert min(one[0][:, 0].min(), one[3][:, 0].min()) == 23 and max(one[0][:, 0].max(), one[3][:, 0].max()) >= 32
    assert max(two[0][:, 0].max(), two[3][:, 0].max()) == 1023 and min(two[0][:, 1].min(), two[3][:, 1].min()) == 0
    return {"word_x23": one, "faces_x1023_y0": two}


FAR_SHIFTS = {"far_x40": (40, 0, 0), "far_y100": (0, 100, 0), "far_z-90": (0, 0, -90), "far_33_33_33": (33, 33, 33)}


def far_case(name):
    if name in FAR_SHIFTS: return moved(base(0), (0, 0, 0), FAR_SHIFTS[name])
    a, ca, na, b, cb = base(0)
    if name == "outliers_in_a": return np.concatenate([a, OUTLIERS]), np.concatenate([ca, OUTLIER_RGB]), np.concatenate([na, OUTLIER_NRM]), b, cb
    assert name == "outliers_in_b"
    return a, ca, na, np.concatenate([b, OUTLIERS]), np.concatenate([cb, OUTLIER_RGB])


FAR = list(FAR_SHIFTS) + ["outliers_in_a", "outliers_in_b"]
SIZES = [(n, side) for n in (1, 63, 64, 65, 257) for side in "ab"]


def size_case(n, side):
    a, ca, na, b, cb = base(1)
    return (a[:n], ca[:n], na[:n], b, cb) if side == "a" else (a, ca, na, b[:n], cb[:n])


# ---- the definition, by brute force ----
_REF = {}


def reference(key, case):
    """-> dict: d1 / color (exact integers), d2 sums, and what the conditions on the cases need (tie shares, merged points of B that take their normal, mixed duplicates)"""
    if key in _REF: return _REF[key]
    a, ca, na, b, cb = case
    A, mA, mix_a = CC.merge(a, ca); B, mB, mix_b = CC.merge(b, cb)
    col_ab, tie_ab, _, _ = CC.one_way(A, mA, B, mB); col_ba, tie_ba, _, _ = CC.one_way(B, mB, A, mA)
    d = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)
    mab, mba = d.min(1), d.min(0)
    take = int(((d == mab[:, None]).sum(0) == 0).sum())
    s_ab, s_ba, n_a, n_b = P.d2_brute_force(a, na, b)
    assert (n_a, n_b) == (len(A), len(B))
    _REF[key] = {"n": (len(A), len(B)), "d1": (int(mab.sum()), int(mba.sum()), int(mab.max()), int(mba.max())), "color": (col_ab, col_ba), "d2": (s_ab, s_ba),
                 "ties": (tie_ab, tie_ba), "take": take, "mixed": (mix_a, mix_b)}
    return _REF[key]


def check_conditions(ref):
    """no case may pass empty (measured on the six base clouds: tie shares 0.16 to 0.44, 47 to 246 merged points of B take their normal)"""
    assert ref["mixed"] == (True, True), "no voxel with >= 3 duplicates of different colours"
    assert ref["ties"][0] >= 0.15 and ref["ties"][1] >= 0.15, ref["ties"]
    assert ref["take"] >= 40, ref["take"]


def geometry_derived(sse_ab, sse_ba, n_a, n_b, peak):
    """mse = (float)(sse / n); psnr = 10 log10f(3 peak^2 / mse) in float; symmetric: against the larger mse"""
    def psnr(m):
        with np.errstate(divide="ignore"):
            q = F32(3) * F32(peak) * F32(peak) / m
        return F32(10) * F32(CC.LIBM.log10f(ctypes.c_float(float(q)))) if m > 0 else F32(np.inf)
    mab, mba = F32(F64(sse_ab) / F64(n_a)), F32(F64(sse_ba) / F64(n_b))
    return mab, mba, psnr(mab), psnr(mba), psnr(max(mab, mba))


def check_geometry_derived(g, peak):
    want = geometry_derived(g["sse_ab"], g["sse_ba"], g["n_a"], g["n_b"], peak)
    got = tuple(F32(g[k]) for k in ("mse_ab", "mse_ba", "psnr_ab", "psnr_ba", "psnr"))
    assert got == want, (got, want)


def score_case(ctx, case, peak=1023):
    """uploads both clouds, scores with everything they allow, releases -> the result as dicts"""
    a, ca, na, b, cb = case
    ha, hb = ctx.pcloud_upload(a, ca, na), ctx.pcloud_upload(b, cb)
    try:
        assert ha.points()[0] == len(a) and hb.points()[0] == len(b)
        return ctx.score(ha, hb, peak)
    finally:
        ha.release(); hb.release()


def same_result(x, y):
    """two results equal field for field, bit for bit (device_ms aside)"""
    return all(x[k] == y[k] for k in x if k != "device_ms")


def check_against_definition(got, ref, peak=1023):
    """D1 and colour exact; D2 sums within rel 1e-9 (the tolerance tests/pcc_cases.py gives reordered double sums); every derived field by its formula"""
    assert got["parts"] == D1 | D2 | COLOR
    n_a, n_b = ref["n"]
    assert (got["n_merged_a"], got["n_merged_b"]) == (n_a, n_b)
    d1, d2, col = got["d1"], got["d2"], got["color"]
    assert (d1["n_a"], d1["n_b"], d2["n_a"], d2["n_b"], col["n_a"], col["n_b"]) == (n_a, n_b) * 3
    assert (d1["sse_ab"], d1["sse_ba"], d1["max_ab"], d1["max_ba"]) == ref["d1"], (d1, ref["d1"])
    check_geometry_derived(d1, peak)
    assert (col["sse_ab"], col["sse_ba"]) == ref["color"], (col["sse_ab"], col["sse_ba"], ref["color"])
    CC.check_derived(col)
    print("d2 sse", d2["sse_ab"], d2["sse_ba"], "brute force", ref["d2"])
    assert d2["sse_ab"] == pytest.approx(ref["d2"][0], rel=1e-9) and d2["sse_ba"] == pytest.approx(ref["d2"][1], rel=1e-9)
    check_geometry_derived(d2, peak)
    assert 0 <= d2["max_ab"] <= d2["sse_ab"] and 0 <= d2["max_ba"] <= d2["sse_ba"]


def check_against_host_array_calls(ctx, got, case, peak=1023, colour=True):
    """out->d1 == rbt_d1, out->color == rbt_color_metric and out->d2 == rbt_d2 field for field: the D2 sums are the same additions in the same order"""
    a, ca, na, b, cb = case
    assert got["d1"] == ctx.d1(a, b, peak)
    if colour: assert got["color"] == ctx.color_metric(a, ca, b, cb)
    old = ctx.d2(a, na, b, peak)
    print("d2 max", got["d2"]["max_ab"], got["d2"]["max_ba"], "rbt_d2", old["max_ab"], old["max_ba"], "sse", got["d2"]["sse_ab"], old["sse_ab"], got["d2"]["sse_ba"], old["sse_ba"])
    for k in ("n_a", "n_b", "max_ab", "max_ba"): assert got["d2"][k] == old[k], (k, got["d2"][k], old[k])
    for k in ("sse_ab", "sse_ba"): assert got["d2"][k] == old[k], (k, got["d2"][k], old[k])


def check_swap(ctx, case, got):
    """swapping a and b swaps the directions of D1 and colour (the swapped source has no normals: D1 and colour are what the clouds allow)"""
    a, ca, na, b, cb = case
    hb, ha = ctx.pcloud_upload(b, cb), ctx.pcloud_upload(a, ca)
    try:
        sw = ctx.score(hb, ha)
    finally:
        ha.release(); hb.release()
    assert sw["parts"] == D1 | COLOR and sw["d2"] is None
    for part in ("d1", "color"):
        for k in ("sse", "mse", "psnr"):
            assert sw[part][k + "_ab"] == got[part][k + "_ba"] and sw[part][k + "_ba"] == got[part][k + "_ab"], (part, k)
        assert (sw[part]["n_a"], sw[part]["n_b"]) == (got[part]["n_b"], got[part]["n_a"]) and sw[part]["psnr"] == got[part]["psnr"]
    assert (sw["d1"]["max_ab"], sw["d1"]["max_ba"]) == (got["d1"]["max_ba"], got["d1"]["max_ab"])


# ---- the cases, each a function of a context (and of a second one to compare with, bit for bit) ----
def check_base(ctx, k, other=None):
    case = base(k); ref = reference(("base", k), case)
    check_conditions(ref)
    got = score_case(ctx, case)
    check_against_definition(got, ref)
    check_against_host_array_calls(ctx, got, case)
    check_swap(ctx, case, got)
    if other is not None: assert same_result(got, score_case(other, case))


def check_boundary(ctx, name, other=None):
    case = boundary_cases()[name]; ref = reference(("boundary", name), case)
    check_conditions(ref)
    got = score_case(ctx, case)
    check_against_definition(got, ref)
    check_against_host_array_calls(ctx, got, case)
    if other is not None: assert same_result(got, score_case(other, case))


def check_far(ctx, name, other=None):
    case = far_case(name); ref = reference(("far", name), case)
    got = score_case(ctx, case)
    check_against_definition(got, ref)
    if name in FAR_SHIFTS: assert max(ref["d1"][2], ref["d1"][3]) > 32 * 32           # nearest distances span more than one word and several coarse blocks
    else: assert max(ref["d1"][2], ref["d1"][3]) > 600 * 600
    if other is not None: assert same_result(got, score_case(other, case))


def check_size(ctx, n, side, other=None):
    case = size_case(n, side)
    got = score_case(ctx, case)
    check_against_definition(got, reference(("size", n, side), case))
    if other is not None: assert same_result(got, score_case(other, case))


def check_degenerate(ctx, other=None):
    a, ca, na, b, cb = base(1)
    one = (a[:1], ca[:1], na[:1], b[:1], cb[:1])
    got = score_case(ctx, one)
    check_against_definition(got, reference(("one",), one))
    same = score_case(ctx, (a, ca, na, a, ca))
    perm = np.random.default_rng(1).permutation(len(a))
    shuffled = score_case(ctx, (a, ca, na, a[perm], ca[perm]))
    for s in (same, shuffled):
        assert s["d1"]["sse_ab"] == s["d1"]["sse_ba"] == 0 and s["d2"]["sse_ab"] == s["d2"]["sse_ba"] == 0.0 and s["color"]["sse_ab"] == s["color"]["sse_ba"] == [0, 0, 0]
        for x in [s["d1"][k] for k in ("psnr", "psnr_ab", "psnr_ba")] + [s["d2"][k] for k in ("psnr", "psnr_ab", "psnr_ba")] + s["color"]["psnr"] + s["color"]["psnr_ab"] + s["color"]["psnr_ba"]:
            assert np.isinf(x) and x > 0
    assert same_result(same, shuffled)
    if other is not None:
        assert same_result(got, score_case(other, one)) and same_result(same, score_case(other, (a, ca, na, a, ca)))


def check_determinism(ctx):
    """two calls on the same handles: the three results byte for byte, d2.sse_* included"""
    a, ca, na, b, cb = base(3)
    ha, hb = ctx.pcloud_upload(a, ca, na), ctx.pcloud_upload(b, cb)
    try:
        x, y = ctx.score(ha, hb, raw=True), ctx.score(ha, hb, raw=True)
    finally:
        ha.release(); hb.release()
    assert x.parts == y.parts == D1 | D2 | COLOR and x.d2.sse_ab > 0
    for part in ("d1", "d2", "color"):
        assert bytes(getattr(x, part)) == bytes(getattr(y, part)), part


def check_handles(R, make_ctx):
    """handles outlive scores and each other; the normals given to the decoded cloud are per call; a recycled volume is clean; rbt_trim hands the cached volumes back"""
    ctx = make_ctx()
    fresh = {}

    def fresh_score(key, case):
        if key not in fresh:
            c = make_ctx()
            try: fresh[key] = score_case(c, case)
            finally: c.close()
        return fresh[key]
    try:
        a, ca, na = base(0)[:3]
        decoded = [base(0)[3:], base(5)[3:], moved(base(0), (0, 0, 0), (3, 0, -2))[3:]]
        ha = ctx.pcloud_upload(a, ca, na)
        hb = [ctx.pcloud_upload(b, cb) for b, cb in decoded]
        for k in (0, 1, 2, 0):                                           # one source against three decoded clouds, then the first again
            assert same_result(ctx.score(ha, hb[k]), fresh_score(("a0", k), (a, ca, na) + tuple(decoded[k])))
        a2, ca2, na2 = base(5)[:3]                                       # one decoded cloud against two sources
        ha2 = ctx.pcloud_upload(a2, ca2, na2)
        assert same_result(ctx.score(ha2, hb[0]), fresh_score(("a5", 0), (a2, ca2, na2) + tuple(decoded[0])))
        assert same_result(ctx.score(ha, hb[0]), fresh[("a0", 0)])
        for h in [ha, ha2] + hb: h.release()
        before = ctx.device_memory()["cached"]
        assert before >= 5 * (1 << 27)                                   # the five volumes are kept
        other = moved(base(2), (700, 500, 300), (700, 500, 300))         # clouds in other voxels: a stale bit of the released clouds would be a nearer neighbour or a tie
        assert same_result(score_case(ctx, other), fresh_score("other", other))
        far = moved(base(0), (0, 0, 0), (0, 100, 0))                     # and across the gap where the released clouds' points lay
        assert same_result(score_case(ctx, far), fresh_score("far", far))
        ctx.trim()
        after = ctx.device_memory()["cached"]
        assert after < before and after + 5 * (1 << 27) <= before, (before, after)
        assert same_result(score_case(ctx, other), fresh["other"])
    finally:
        ctx.close()


def small_pair():
    """one point against two: D1 sums 1 and 2, colour as in color_cases (mean of 4 and 7 = 5.5 -> 6)"""
    return (np.array([[5, 5, 5]], np.int16), np.array([[1, 2, 3]], np.uint8), np.array([[0, 0, 16384]], np.int16),
            np.array([[5, 5, 6], [5, 6, 5]], np.int16), np.array([[1, 2, 4], [1, 2, 7]], np.uint8))


def check_still_works(ctx):
    got = score_case(ctx, small_pair())
    assert (got["d1"]["sse_ab"], got["d1"]["sse_ba"]) == (1, 2) and got["color"]["sse_ab"] == [(722 * -3) ** 2, (5000 * -3) ** 2, (-458 * -3) ** 2]
    assert got["d2"]["sse_ab"] == 0.5 and got["d2"]["sse_ba"] == 1.0      # the plane z = 5 of the source: (1 + 0) / 2 from the source, 1 + 0 from the decoded cloud


def refused(R, f):
    try:
        f()
    except R.RbtError as e:
        assert e.code == -4, str(e)                                     # RBT_ERR_PARAM
        return
    raise AssertionError("accepted")


def check_arguments(R, ctx, make_ctx):
    a, ca, na, b, cb = small_pair()
    check_still_works(ctx)
    ha, hb, hplain = ctx.pcloud_upload(a, ca, na), ctx.pcloud_upload(b, cb), ctx.pcloud_upload(b)
    other_ctx = make_ctx()
    try:
        foreign = other_ctx.pcloud_upload(b, cb)
        bad = [lambda: ctx.score(None, hb), lambda: ctx.score(ha, None), lambda: ctx.score(ha, foreign), lambda: ctx.score(foreign, hb),
               lambda: ctx.score(hb, ha, parts=D2),                      # D2 without normals on the source
               lambda: ctx.score(ha, hplain, parts=COLOR), lambda: ctx.score(ha, hplain, parts=D1 | D2 | COLOR),      # colour without colours
               lambda: ctx.score(ha, hb, parts=8), lambda: ctx.score(ha, hb, peak=0),
               lambda: ctx.pcloud_upload(np.zeros((0, 3), np.int16)),
               lambda: ctx.pcloud_upload(np.array([[5, 5, 5], [0, -1, 0]], np.int16)), lambda: ctx.pcloud_upload(np.array([[5, 5, 5], [0, 0, 1024]], np.int16), np.zeros((2, 3), np.uint8))]
        for f in bad:
            refused(R, f)
            check_still_works(ctx)
        assert ctx.score(ha, hplain)["parts"] == D1 | D2 and same_result(ctx.score(ha, hb), score_case(ctx, small_pair()))
    finally:
        other_ctx.close()                                               # rbt_destroy releases the handle still outstanding
    # by maps: a patch whose tangent offset puts points at -1, or at 1024 and beyond (smoothing off, so that the check of the index is the one that refuses)
    for u1 in (-3, 1000):                                               # the occupied area of a patch starts 2 pixels in: -3 + 2 = -1
        case = list(P.seam_atlas(R, 0, tiles=3)); case[0] = P._copy_atlas(R, case[0], geometry_smoothing=0)
        case[1][0].u1 = u1
        xyz = ctx.reconstruct_rgb(*case)[0]
        assert (xyz.min() == -1) if u1 < 0 else (xyz.max() >= 1024)
        refused(R, lambda: ctx.pcloud_from_maps(*case))
        check_still_works(ctx)
    for h in (ha, hb, hplain): h.release()


def seam_source(R, ctx, case, tiles):
    """the source side of a seam atlas: the same maps reconstructed without smoothing, RGB as the decoder leaves it, normals = the projection axis of each point's patch
    (the patch of a point read back through an index picture, as synth.source_normals does)"""
    plain = list(case); plain[0] = P._copy_atlas(R, case[0], geometry_smoothing=0)
    xyz, _, _, _, rgb = ctx.reconstruct_rgb(*plain)
    w = case[0].width
    yy, xx = np.mgrid[0:w, 0:w]
    idx = np.concatenate([((yy // 32) * tiles + xx // 32).astype(np.uint16).ravel(), np.zeros(w * w // 2, np.uint16)])
    pi = ctx.reconstruct(plain[0], plain[1], plain[2], plain[3], plain[4], plain[5], idx, idx, 10)[1][:, 0].astype(np.int64)
    axes = np.array([p.normal_axis for p in case[1]])
    n = np.zeros((len(xyz), 3), np.int16); n[np.arange(len(xyz)), axes[pi]] = 16384
    return xyz, rgb, n


def check_from_maps(R, ctx, case, tiles=3, other=None):
    want = ctx.reconstruct_decoded(*case); n_sm, n_ch = ctx.n_smoothed, ctx.n_changed
    h, host = ctx.pcloud_from_maps(*case, host_copy=True)
    assert all(np.array_equal(g, x) for g, x in zip(host, want[:5])) and (ctx.n_smoothed, ctx.n_changed) == (n_sm, n_ch) and n_sm > 0
    assert h.points()[0] == len(want[0])
    sx, srgb, sn = seam_source(R, ctx, case, tiles)
    hs, h2, h3 = ctx.pcloud_upload(sx, srgb, sn), ctx.pcloud_upload(host[0], host[4]), ctx.pcloud_from_maps(*case)
    try:
        got = ctx.score(hs, h)
        assert got["parts"] == D1 | D2 | COLOR and same_result(got, ctx.score(hs, h2)) and same_result(got, ctx.score(hs, h3))
        assert got["d1"] == ctx.d1(sx, host[0]) and got["color"] == ctx.color_metric(sx, srgb, host[0], host[4]) and got["d1"]["sse_ab"] > 0
    finally:
        for x in (h, hs, h2, h3): x.release()
    if other is not None:
        assert same_result(got, score_case(other, (sx, srgb, sn, host[0], host[4])))
    return got


def check_summary(R):
    def frame(parts, d1=0.0, d2=0.0, yuv=(0.0, 0.0, 0.0), pts=(0, 0, 0, 0)):
        s = R.FrameScore(); s.parts = parts; s.d1.psnr = d1; s.d2.psnr = d2
        for c in range(3): s.color.psnr[c] = yuv[c]
        s.n_points_a, s.n_points_b, s.n_merged_a, s.n_merged_b = pts
        return s
    frames = [frame(7, 70.5, 75.25, (40.0, 45.0, 50.0), (10, 9, 8, 7)), frame(1, 60.0, 99.0, (1.0, 1.0, 1.0), (20, 19, 18, 17)), frame(5, 65.0, 99.0, (30.0, 47.0, 44.0), (1, 1, 1, 1)),
              frame(3, 71.0, 70.0, (1.0, 1.0, 1.0), (2, 2, 2, 2))]
    s = R.score_summary(frames)
    assert (s["n_frames"], s["n_d1"], s["n_d2"], s["n_color"]) == (4, 4, 2, 2)
    assert s["mean_d1"] == (70.5 + 60.0 + 65.0 + 71.0) / 4 and s["min_d1"] == 60.0
    assert s["mean_d2"] == (75.25 + 70.0) / 2 and s["min_d2"] == 70.0                # frames lacking D2 are left out, whatever their d2 fields hold
    assert s["mean_color"] == [35.0, 46.0, 47.0] and s["min_color"] == [30.0, 45.0, 44.0]
    assert (s["points_a"], s["points_b"], s["merged_a"], s["merged_b"]) == (33, 31, 29, 27)
    inf = R.score_summary(frames + [frame(7, float("inf"), 80.0, (float("inf"), 41.0, 42.0))])
    assert inf["mean_d1"] == float("inf") and inf["min_d1"] == 60.0 and inf["mean_color"][0] == float("inf") and inf["min_color"][0] == 30.0 and inf["mean_d2"] == (75.25 + 70.0 + 80.0) / 3
    # float PSNRs are widened, not re-rounded: the mean is formed in double
    third = R.score_summary([frame(1, 0.1), frame(1, 0.2), frame(1, 0.4)])
    assert third["mean_d1"] == (float(F32(0.1)) + float(F32(0.2)) + float(F32(0.4))) / 3
    empty = R.score_summary([])
    assert empty["n_frames"] == 0 and empty["n_d1"] == 0 and empty["mean_d1"] == 0.0
