"""Cases and checks of the host-array metrics rbt_d1, rbt_d2 and rbt_color_metric as what they are now: upload + score + release of two temporary clouds
(host/rbt_pcc.cpp). Shared by tests/test_metric_fold.py (serial host emulation of the kernel bodies) and tests/test_gpu_metric_fold.py (the GPU build). The clouds are
a few thousand points at most; references are NumPy brute force (tests/score_cases.py reference: D1 and colour exact) and the oracle's D2 (rel 1e-9: it adds the
doubles in another order, as tests/pcc_cases.py check_d2 says)."""
import numpy as np
import pytest
import oracle_lib as O
import pcc_cases as P
import score_cases as SC

EMPTY = {"d1": "empty point cloud", "d2": "empty point cloud or no normals", "color": "empty point cloud or no colours"}
RANGE = "coordinate outside 0..1023"
MERGED = "more than 2^21 merged points"
CALLS = ("d1", "d2", "color")


def call(ctx, which, case, peak=1023):
    a, ca, na, b, cb = case
    if which == "d1": return ctx.d1(a, b, peak)
    if which == "d2": return ctx.d2(a, na, b, peak)
    return ctx.color_metric(a, ca, b, cb)


def refused_with(R, ctx, f, text):
    """RBT_ERR_PARAM and exactly this text from rbt_last_error"""
    try:
        f()
    except R.RbtError as e:
        assert e.code == -4, str(e)
        assert ctx.L.rbt_last_error(ctx.h).decode() == text, str(e)
        return
    raise AssertionError("accepted")


def check_good_pair(ctx):
    """score_cases.small_pair through the three calls: D1 sums 1 and 2, D2 sums 0.5 and 1.0, the colour terms of a tie mean of 5.5 -> 6"""
    case = SC.small_pair()
    d1, d2, col = (call(ctx, w, case) for w in CALLS)
    assert (d1["sse_ab"], d1["sse_ba"], d1["n_a"], d1["n_b"]) == (1, 2, 1, 2) and (d2["sse_ab"], d2["sse_ba"]) == (0.5, 1.0)
    assert col["sse_ab"] == [(722 * -3) ** 2, (5000 * -3) ** 2, (-458 * -3) ** 2] and col["n_b"] == 2


def refusal_cases(which):
    """(name, case, peak, text): every refusal the call can give on small input, the bad cloud in position A and in position B. Left out: more than 2^26 points in a cloud
    (pcloud_index refuses it on the count alone, before any kernel runs) - it takes 400 MB of input, and the cases here are a few thousand points at most"""
    a, ca, na, b, cb = SC.small_pair()
    none = (np.zeros((0, 3), np.int16), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int16))
    low = (np.array([[5, 5, 5], [0, -1, 0]], np.int16), np.zeros((2, 3), np.uint8), np.array([[0, 0, 16384]] * 2, np.int16))
    high = (np.array([[5, 5, 5], [0, 0, 1024]], np.int16), np.zeros((2, 3), np.uint8), np.array([[0, 0, 16384]] * 2, np.int16))
    out = [("empty_a", none + (b, cb), 1023, EMPTY[which]), ("empty_b", (a, ca, na) + none[:2], 1023, EMPTY[which]),
           ("low_a", low + (b, cb), 1023, RANGE), ("high_a", high + (b, cb), 1023, RANGE), ("low_b", (a, ca, na) + low[:2], 1023, RANGE), ("high_b", (a, ca, na) + high[:2], 1023, RANGE),
           ("both_out", high + low[:2], 1023, RANGE)]
    if which != "color":
        out += [("peak_0", (a, ca, na, b, cb), 0, EMPTY[which]), ("peak_negative", (a, ca, na, b, cb), -5, EMPTY[which]),
                ("peak_before_range", low + (b, cb), 0, EMPTY[which])]          # the call's own checks come first, as they did
    else:
        out += [("no_colours_a", (a, None, na, b, cb), 1023, EMPTY[which]), ("no_colours_b", (a, ca, na, b, None), 1023, EMPTY[which]),
                ("no_colours_before_range", (a, ca, na, high[0], None), 1023, EMPTY[which])]
    return out


def check_refusals(R, ctx, which):
    """code and exact text; the device holds what it held before; the context holds no handle (a good pair scores, and the memory figure says so)"""
    check_good_pair(ctx)                                                   # whatever a first call sets up once is set up
    for name, case, peak, text in refusal_cases(which):
        before = ctx.device_memory()["in_use"]
        refused_with(R, ctx, lambda: call(ctx, which, case, peak), text)
        assert ctx.device_memory()["in_use"] == before, name
        check_good_pair(ctx)
        assert ctx.device_memory()["in_use"] == before, name


# ---- edge clouds ----
def _colours(seed, n):
    return np.random.default_rng(900 + seed).integers(0, 256, (n, 3)).astype(np.uint8)


def _distinct(seed, n, lo=200, span=4):
    """n distinct voxels of a span^3 cube: neighbours tie"""
    r = np.random.default_rng(800 + seed)
    ids = r.permutation(span ** 3)[:n]
    return (lo + np.stack([ids % span, ids // span % span, ids // (span * span)], 1)).astype(np.int16)


def edge_cases():
    """name -> (a, rgb_a, normals_a, b, rgb_b)"""
    out = {}
    out["one_point_each"] = (np.array([[7, 9, 11]], np.int16), _colours(0, 1), SC.normals(0, 1), np.array([[9, 9, 12]], np.int16), _colours(1, 1))
    cloud = _distinct(2, 60, lo=300, span=5)
    out["a_in_one_voxel"] = (np.repeat(np.array([[301, 302, 303]], np.int16), 50, 0), _colours(2, 50), SC.normals(1, 50), cloud, _colours(3, 60))
    out["b_in_one_voxel"] = (cloud, _colours(4, 60), SC.normals(2, 60), np.repeat(np.array([[310, 300, 305]], np.int16), 50, 0), _colours(5, 50))
    for n in (8, 9):                                                      # 2 n = 16 fills the smallest map, 2 n = 18 doubles the slot count - in both clouds
        out["n%d" % n] = (_distinct(10 + n, n), _colours(10 + n, n), SC.normals(n, n), _distinct(20 + n, n), _colours(20 + n, n))
    return out


def check_edge(ctx, name, other=None):
    case = edge_cases()[name]
    a, ca, na, b, cb = case
    ref = SC.reference(("fold_edge", name), case)
    d1, d2, col = (call(ctx, w, case) for w in CALLS)
    assert (d1["n_a"], d1["n_b"], d2["n_a"], d2["n_b"], col["n_a"], col["n_b"]) == ref["n"] * 3
    assert (d1["sse_ab"], d1["sse_ba"], d1["max_ab"], d1["max_ba"]) == ref["d1"], (d1, ref["d1"])
    SC.check_geometry_derived(d1, 1023)
    assert (col["sse_ab"], col["sse_ba"]) == ref["color"], (col, ref["color"])
    SC.CC.check_derived(col)
    want = O.d2(a, na, b)
    print("d2", d2, "oracle", want)
    assert (d2["n_a"], d2["n_b"]) == (want["n_a"], want["n_b"])
    for k in ("sse_ab", "sse_ba", "max_ab", "max_ba"):
        assert d2[k] == pytest.approx(want[k], rel=1e-9), k
    SC.check_geometry_derived(d2, 1023)
    if other is not None:
        assert (d1, d2, col) == tuple(call(other, w, case) for w in CALLS)


def check_same_array(ctx):
    """the same array as A and as B: every sum 0, every psnr +inf"""
    a, ca, na, _, _ = SC.base(1)
    case = (a, ca, na, a, ca)
    d1, d2, col = (call(ctx, w, case) for w in CALLS)
    n = len(np.unique(a, axis=0))
    assert (d1["n_a"], d1["n_b"], d2["n_a"], d2["n_b"], col["n_a"], col["n_b"]) == (n,) * 6
    assert d1["sse_ab"] == d1["sse_ba"] == d1["max_ab"] == d1["max_ba"] == 0 and d2["sse_ab"] == d2["sse_ba"] == d2["max_ab"] == d2["max_ba"] == 0.0
    assert col["sse_ab"] == col["sse_ba"] == [0, 0, 0]
    for x in [g[k] for g in (d1, d2) for k in ("psnr", "psnr_ab", "psnr_ba")] + col["psnr"] + col["psnr_ab"] + col["psnr_ba"]:
        assert np.isinf(x) and x > 0


# ---- rbt_d2 is the score's D2: the same additions, the same bits from every call ----
def _bits(r):
    return {k: (float(v).hex() if isinstance(v, float) else v) for k, v in r.items()}


def check_d2_determinism(ctx, k):
    a, n, b = P.d2_cases()[k]
    assert len(np.unique(a, axis=0)) < len(a) and (k == 3 or len(np.unique(b, axis=0)) < len(b))      # duplicates (case 3: the sparse reconstruction, 300 points, has none)
    x, y = ctx.d2(a, n, b), ctx.d2(a, n, b)
    assert x["sse_ab"] > 0 and x["sse_ba"] > 0 and _bits(x) == _bits(y)
    ha, hb = ctx.pcloud_upload(a, None, n), ctx.pcloud_upload(b)
    try:
        s = ctx.score(ha, hb)
    finally:
        ha.release(); hb.release()
    assert _bits(s["d2"]) == _bits(x)


# ---- memory ----
def check_memory_after_success(ctx, which):
    """the two temporary clouds and their volumes are gone when the call returns: nothing in use, nothing more in the context's caches"""
    case = SC.base(0)
    call(ctx, which, case)                                                 # whatever a first call sets up once is set up
    ctx.trim()
    m0 = ctx.device_memory()
    call(ctx, which, case)
    assert ctx.device_memory()["in_use"] == m0["in_use"]
    ctx.trim()
    assert ctx.device_memory()["cached"] == m0["cached"]
