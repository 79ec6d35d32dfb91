"""Cases and NumPy restatements for the colour stages (rbt_yuv420_to_yuv444, rbt_yuv16_to_rgb8, rbt_reconstruct_rgb, rbt_color_metric), shared by the host-emulation
test (tests/test_color.py) and the GPU test (tests/test_gpu_color.py). The restatements are written from the reference's text, not from the product code:
  up-conversion  PCCInternalColorConverter::convertYUV420ToYUV444 (PCCInternalColorConverter.cpp:466-485): YUVtoFloatYUV (:596-610), upsampling (:669-695) with the float
                 loops of PCCInternalColorConverter.h:187-249 and g_filter420to444[0] (:297-302), floatYUVToYUV with nbyte = 2 (:580-593) - float32 / float64 step for step
  RGB            PCCPointSet3::convertYUV16ToRGB8 (PCCPointSet.h:133-166) in float64
  metric         removeDuplicate with averaged colours (PCCPointSet.cpp:190-203), QualityMetrics::compute's colour part (PCCMetrics.cpp:127-179, :221-225), by brute force"""
import ctypes
import ctypes.util
import numpy as np

F32, F64 = np.float32, np.float64
# g_filter420to444[0], PCCInternalColorConverter.cpp:297-302; struct Filter420to444 is {horizontal0_, vertical0_, horizontal1_, vertical1_}
H0, V0, H1, V1 = [0, 256], [-8, 64, 216, -16], [-16, 144, 144, -16], [-16, 216, 64, -8]


def round_away(x):
    """std::round on float64 values: half away from zero (x - trunc(x) is exact)"""
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0.0)


def to_float(p, chroma, bd):
    """YUVtoFloatYUV"""
    weight = F64(1.0) / F64(255.0 if bd == 8 else 1023.0)
    off = (128 if bd == 8 else 512) if chroma else 0
    v = (weight * (p.astype(np.int64) - off).astype(F64)).astype(F32)
    return np.minimum(np.maximum(v, F32(-0.5 if chroma else 0.0)), F32(0.5 if chroma else 1.0))


def to_16(v, chroma):
    """floatYUVToYUV, nbyte = 2"""
    x = (F64(65535.0) * v.astype(F64) + F64(32768.0 if chroma else 0.0)).astype(F32)
    r = round_away(x.astype(F64)).astype(F32)
    return np.minimum(np.maximum(r, F32(0)), F32(65535)).astype(np.uint16)


def taps_sum(taps, sample):
    """the float inner loop: value += tap * sample, tap by tap, each product and each sum rounded to float32; then (value + 0) * (1 / 256)"""
    value = None
    for k, t in enumerate(taps):
        prod = F32(t) * sample(k)
        assert prod.dtype == F32
        value = (F32(0) + prod) if value is None else value + prod
        assert value.dtype == F32
    return (value + F32(0)) * (F32(1.0) / F32(256))


def upsampling(c):
    """upsampling (:669-695): vertical pass into a widthIn x 2 heightIn plane, then horizontal; indices clamped to the plane; position = (taps + 1) >> 1"""
    ch, cw = c.shape
    rows, cols = np.arange(ch), np.arange(cw)
    temp = np.zeros((2 * ch, cw), F32)
    temp[0::2] = taps_sum(V0, lambda k: c[np.clip(rows + 0 + k - ((len(V0) + 1) >> 1), 0, ch - 1)])
    temp[1::2] = taps_sum(V1, lambda k: c[np.clip(rows + 1 + k - ((len(V1) + 1) >> 1), 0, ch - 1)])
    out = np.zeros((2 * ch, 2 * cw), F32)
    out[:, 0::2] = taps_sum(H0, lambda k: temp[:, np.clip(cols + 0 + k - ((len(H0) + 1) >> 1), 0, cw - 1)])
    out[:, 1::2] = taps_sum(H1, lambda k: temp[:, np.clip(cols + 1 + k - ((len(H1) + 1) >> 1), 0, cw - 1)])
    return out


def split420(frame, w, h):
    ys, cs = w * h, (w // 2) * (h // 2)
    return frame[:ys].reshape(h, w), frame[ys:ys + cs].reshape(h // 2, w // 2), frame[ys + cs:ys + 2 * cs].reshape(h // 2, w // 2)


def up444(frames, w, h, bd):
    """convertYUV420ToYUV444 with filter 0 on [n, w*h*3/2] pictures -> uint16 [n, 3, h, w]"""
    frames = np.asarray(frames, np.uint16).reshape(-1, w * h * 3 // 2)
    out = np.zeros((frames.shape[0], 3, h, w), np.uint16)
    for i, f in enumerate(frames):
        y, u, v = split420(f, w, h)
        out[i, 0] = to_16(to_float(y, False, bd), False)
        out[i, 1] = to_16(upsampling(to_float(u, True, bd)), True)
        out[i, 2] = to_16(upsampling(to_float(v, True, bd)), True)
    return out


def replicate444(frames, w, h):
    """PCCImage::convertYUV420ToYUV444 (PCCImage.cpp:111-135)"""
    frames = np.asarray(frames, np.uint16).reshape(-1, w * h * 3 // 2)
    out = np.zeros((frames.shape[0], 3, h, w), np.uint16)
    for i, f in enumerate(frames):
        y, u, v = split420(f, w, h)
        out[i, 0] = y; out[i, 1] = np.repeat(np.repeat(u, 2, 0), 2, 1); out[i, 2] = np.repeat(np.repeat(v, 2, 0), 2, 1)
    return out


def yuv16_to_rgb8(yuv):
    """convertYUV16ToRGB8 in float64, operation for operation"""
    yuv = np.asarray(yuv, np.uint16).reshape(-1, 3).astype(F64)
    offset, weight = F64(32768.0), F64(1.0) / F64(65535.0)
    y1 = weight * yuv[:, 0]; u1 = weight * (yuv[:, 1] - offset); v1 = weight * (yuv[:, 2] - offset)
    y1 = np.minimum(np.maximum(y1, 0.0), 1.0); u1 = np.minimum(np.maximum(u1, -0.5), 0.5); v1 = np.minimum(np.maximum(v1, -0.5), 0.5)
    r = y1 + 1.57480 * v1
    g = y1 - 0.18733 * u1 - 0.46813 * v1
    b = y1 + 1.85563 * u1
    return np.stack([np.clip(round_away(c * 255), 0.0, 255.0) for c in (r, g, b)], axis=1).astype(np.uint8)


# ---- up-conversion cases ----
UP_SIZES = [(2, 2), (4, 6), (64, 48), (130, 70)]


def up_pictures(w, h, bd, seed, n=2):
    """noise, steps at the borders and full-range extremes: n pictures; samples use all 16 bits' worth of the range the depth allows plus values ABOVE it (a 10-bit
    sample of 1023 + k in a uint16 makes YUVtoFloatYUV's clamp act, and filter overshoot next to extremes makes the final clip act)"""
    r = np.random.default_rng(500 + seed)
    top = (1 << bd) - 1
    out = []
    for k in range(n):
        f = r.integers(0, top + 1, w * h * 3 // 2).astype(np.uint16)
        if k % 2 == 1:
            y, u, v = (a.copy() for a in split420(f, w, h))
            for p in (y, u, v):        # steps at the borders, extremes in blocks and as single samples
                p[:, : max(1, p.shape[1] // 4)] = top; p[: max(1, p.shape[0] // 4), :] = 0; p[-1, :] = top; p[:, -1] = 0
                m = r.random(p.shape) < 0.1; p[m] = r.choice([0, top, top + 1, min(65535, 4 * top)], int(m.sum()))
            f = np.concatenate([y.ravel(), u.ravel(), v.ravel()]).astype(np.uint16)
        out.append(f)
    return np.stack(out)


def check_up(ctx, R):
    for bd in (8, 10):
        for i, (w, h) in enumerate(UP_SIZES):
            f = up_pictures(w, h, bd, 10 * i + bd)
            got, want = ctx.yuv420_to_yuv444(f, w, h, bd), up444(f, w, h, bd)
            assert got.shape == want.shape and np.array_equal(got, want), (bd, w, h, int((got != want).sum()))
            assert want.min() == 0 and want.max() == 65535 or w * h < 64       # the clip acts
            assert np.array_equal(ctx.yuv420_to_yuv444(f, w, h, bd, R.RBT_UPSAMPLE_REPLICATE), replicate444(f, w, h))


def check_up_large(ctx, bd=10):
    f = up_pictures(1280, 1280, bd, 99)
    got = ctx.yuv420_to_yuv444(f, 1280, 1280, bd)
    assert np.array_equal(got, up444(f, 1280, 1280, bd))
    return f, got


def check_up_known_answers(ctx, R):
    w, h = 16, 12
    # a constant picture stays constant: chroma 512 -> 32768, luma k -> round((float)(65535 * (double)(float)(k / 1023))) for every k. The product is rounded to float before
    # std::round, as floatYUVToYUV writes it: for k = 820 it is 52530.4992..., the float nearest to it is 52530.5, and the sample is 52531 (52530 without that cast).
    for k in range(0, 1024):
        f = np.concatenate([np.full(w * h, k, np.uint16), np.full(w * h // 2, 512, np.uint16)])[None]
        got = ctx.yuv420_to_yuv444(f, w, h, 10)
        assert np.all(got[0, 1:] == 32768) and np.all(got[0, 0] == got[0, 0, 0, 0])
        assert int(got[0, 0, 0, 0]) == int(round_away(F64(F32(F64(65535.0) * F64(F32(F64(k) / F64(1023.0))))))), k
    assert int(ctx.yuv420_to_yuv444(np.concatenate([np.full(w * h, 820, np.uint16), np.full(w * h // 2, 512, np.uint16)])[None], w, h, 10)[0, 0, 0, 0]) == 52531
    f8 = np.concatenate([np.full(w * h, 77, np.uint16), np.full(w * h // 4, 128, np.uint16), np.full(w * h // 4, 90, np.uint16)])[None]
    g8 = ctx.yuv420_to_yuv444(f8, w, h, 8)
    assert np.all(g8[0, 1] == 32768) and np.all(g8[0, 2] == g8[0, 2, 0, 0]) and np.all(g8[0, 0] == g8[0, 0, 0, 0])
    # a single bright chroma sample in a flat field: the 4x4 outer product of the tap rows around it. Field 512 -> 0.0f, sample s -> a = (float)((s - 512) / 1023): the
    # vertical pass leaves a * tv / 256 in rows 2i-2 .. 2i+1 for tv = (-16 [v1 at i-1... see below]), the horizontal pass multiplies by th / 256.
    cw, ch, ci, cj, s = w // 2, h // 2, 3, 4, 700
    u = np.full((ch, cw), 512, np.uint16); u[ci, cj] = s
    f = np.concatenate([np.full(w * h, 300, np.uint16), u.ravel(), np.full(cw * ch, 512, np.uint16)])[None]
    got = ctx.yuv420_to_yuv444(f, w, h, 10)[0, 1]
    a = F32(F64(1.0) / F64(1023.0) * F64(s - 512))
    # output row 2i' (even) = V0 at i': taps k over rows i'-2+k; row 2i'+1 = V1 at i'+1: rows i'-1+k. The sample at row ci is seen with tap V0[ci-i'+2] / V1[ci-i'+1].
    tv = {}
    for ip in range(ch):
        if 0 <= ci - ip + 2 < 4: tv[2 * ip] = V0[ci - ip + 2]
        if 0 <= ci - ip + 1 < 4: tv[2 * ip + 1] = V1[ci - ip + 1]
    th = {}
    for jp in range(cw):       # column 2j' = H0 at j': columns j'-1+k; column 2j'+1 = H1 at j'+1: columns j'-1+k
        if 0 <= cj - jp + 1 < 2: th[2 * jp] = H0[cj - jp + 1]
        if 0 <= cj - jp + 1 < 4: th[2 * jp + 1] = H1[cj - jp + 1]
    tv = {k: v for k, v in tv.items() if v}; th = {k: v for k, v in th.items() if v}
    # each output phase has a four-tap row (H0's first tap is 0): the sample spreads over 8 rows (4 even by V0, 4 odd by V1) and 5 columns (1 even by H0, 4 odd by H1)
    assert sorted(tv) == list(range(2 * ci - 3, 2 * ci + 5)) and sorted(th) == [2 * cj - 3, 2 * cj - 1, 2 * cj, 2 * cj + 1, 2 * cj + 3]
    want = np.full((h, w), 32768, np.int64)
    for y_, a_ in tv.items():
        t = F32(F32(a_) * a) * (F32(1) / F32(256))                 # all other taps see 0.0f: adding +-0 changes nothing
        for x_, b_ in th.items():
            o = F32(F32(b_) * t) * (F32(1) / F32(256))
            want[y_, x_] = int(to_16(np.array([o], F32), True)[0])
    assert np.array_equal(got.astype(np.int64), want) and (want != 32768).sum() == 40
    assert np.array_equal(ctx.yuv420_to_yuv444(f, w, h, 10, R.RBT_UPSAMPLE_REPLICATE)[0, 1], np.repeat(np.repeat(u, 2, 0), 2, 1))


def check_up_bad_arguments(ctx, R):
    for w, h, bd, filt in ((3, 4, 10, 0), (4, 3, 10, 0), (4, 4, 12, 0), (4, 4, 10, 5)):      # odd sizes, a depth other than 8 / 10, an unknown filter
        try:
            ctx.yuv420_to_yuv444(np.zeros((1, w * h * 3 // 2), np.uint16), w, h, bd, filt)
            raise AssertionError("accepted %r" % ((w, h, bd, filt),))
        except R.RbtError as e:
            assert e.code == -4
    assert ctx.yuv420_to_yuv444(np.zeros((1, 24), np.uint16), 4, 4, 10).shape == (1, 3, 4, 4)


# ---- RGB cases ----
def rgb_inputs():
    e = np.array([0, 1, 32767, 32768, 65534, 65535], np.uint16)
    grid = np.stack(np.meshgrid(e, e, e, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([grid, np.random.default_rng(3).integers(0, 65536, (100000, 3)).astype(np.uint16)])


def check_rgb(ctx):
    x = rgb_inputs()
    got = ctx.yuv16_to_rgb8(x)
    assert np.array_equal(got, yuv16_to_rgb8(x))
    assert ctx.yuv16_to_rgb8(np.array([[65535, 32768, 32768], [0, 32768, 32768]], np.uint16)).tolist() == [[255, 255, 255], [0, 0, 0]]
    assert got.min() == 0 and got.max() == 255


# ---- reconstruct_rgb ----
def _luma_picture(plane):
    return np.concatenate([plane.ravel().astype(np.uint16), np.zeros(plane.size // 2, np.uint16)])


def check_reconstruct_rgb(ctx, R, case, oracle_reconstruct=None):
    """xyz / occupancy_map / block_to_patch as reconstruct's; yuv = the restated 4:4:4 planes at every point's pixel (pixel and map of a point from reconstructions of
    index pictures through the 4:2:0 path); rgb = the restated conversion of yuv; the 4:2:0 path itself unchanged (== the oracle)"""
    atlas, patches, occ, d0, d1, gbd, t0, t1, abd = case
    w, h = atlas.width, atlas.height
    plain = ctx.reconstruct(*case)
    if oracle_reconstruct is not None:
        for g, x in zip(plain, oracle_reconstruct(*case)): assert np.array_equal(g, x)
    xs = ctx.reconstruct(atlas, patches, occ, d0, d1, gbd, _luma_picture(np.tile(np.arange(w), (h, 1))), _luma_picture(np.tile(np.arange(w), (h, 1))), 10)[1][:, 0].astype(np.int64)
    ys = ctx.reconstruct(atlas, patches, occ, d0, d1, gbd, _luma_picture(np.repeat(np.arange(h), w)), _luma_picture(np.repeat(np.arange(h), w)), 10)[1][:, 0].astype(np.int64)
    mp = ctx.reconstruct(atlas, patches, occ, d0, d1, gbd, _luma_picture(np.zeros((h, w))), _luma_picture(np.ones((h, w))), 10)[1][:, 0].astype(np.int64)
    assert plain[0].shape[0] > 0 and (atlas.map_count < 2 or mp.max() == 1)
    for filt, planes in ((R.RBT_UPSAMPLE_F0, up444(np.stack([t0, t1]), w, h, abd)), (R.RBT_UPSAMPLE_REPLICATE, replicate444(np.stack([t0, t1]), w, h))):
        xyz, yuv, om, b2p, rgb = ctx.reconstruct_rgb(atlas, patches, occ, d0, d1, gbd, t0, t1, abd, filt)
        assert np.array_equal(xyz, plain[0]) and np.array_equal(om, plain[2]) and np.array_equal(b2p, plain[3])
        assert np.array_equal(yuv, planes[mp, :, ys, xs])
        assert np.array_equal(rgb, yuv16_to_rgb8(yuv))
    return xyz, rgb


def check_reconstruct_rgb_known_answer(ctx, R):
    """the single 16x16 patch of tests/test_pcc_recon.py: occupied pixels x = 0..2, y = 16..19 in raster order, pixel (1, 17) also gives a point of the far map"""
    atlas = R.AtlasParams(32, 32, 16, 1, 2, 1, 1, 0)
    occ = np.zeros((32, 32), np.uint16); occ[16:20, 0:3] = 1
    d0 = np.full((32, 32), 40, np.uint16); d1 = d0.copy(); d1[17, 1] = 44
    p = R.Patch(0, 1, 1, 1, 100, 200, 7, 2, 0, 1, 0, 0, 1, 1)
    r = np.random.default_rng(9)
    t = r.integers(0, 1024, (2, 32 * 32 * 3 // 2)).astype(np.uint16)
    xyz, yuv, om, b2p, rgb = ctx.reconstruct_rgb(atlas, [p], occ, d0, d1, 10, t[0], t[1], 10)
    planes = up444(t, 32, 32, 10)
    want = []
    for v in range(4):
        for u in range(3):
            want.append(planes[0, :, 16 + v, u])
            if (u, v) == (1, 1): want.append(planes[1, :, 17, 1])
    assert xyz.shape[0] == 13 and np.array_equal(yuv, np.array(want)) and np.array_equal(rgb, yuv16_to_rgb8(yuv))
    for bad in (dict(t0=None, t1=None), dict(t0=t[0], t1=t[1], attr_bd=12), dict(t0=t[0], t1=t[1], upsample_filter=3)):
        try:
            ctx.reconstruct_rgb(atlas, [p], occ, d0, d1, 10, **bad)
            raise AssertionError("accepted %r" % (sorted(bad),))
        except R.RbtError as e:
            assert e.code == -4
    assert ctx.reconstruct_rgb(atlas, [p], occ, d0, d1, 10, t[0], t[1], 10)[0].shape[0] == 13


# ---- colour metric ----
def metric_cases():
    """(xyz_a, rgb_a, xyz_b, rgb_b), up to 3000 points per cloud, coordinates from a narrow range so that voxels hold several points and nearest neighbours tie"""
    out = []
    for seed, lo in enumerate((100, 300, 0, 1012, 512, 40)):
        r = np.random.default_rng(70 + seed)
        span = 12
        a = r.integers(lo, lo + span, (3000, 3)).astype(np.int16)
        ca = r.integers(0, 256, (3000, 3)).astype(np.uint8)
        if seed == 4:                                                                           # a sparse source against an independent cloud
            a[1200:] = a[:1800]; ca[1200:] = r.integers(0, 256, (1800, 3))
        if seed == 5: ca = (ca // 64 * 64 + 40).astype(np.uint8)                                # few colour levels
        k = 2500 if seed != 2 else 1200
        pick = r.permutation(3000)[:k]
        b = np.clip(a[pick] + r.integers(-1, 2, (k, 3)), max(lo - 1, 0), min(lo + span, 1023)).astype(np.int16)
        cb = np.clip(ca[pick].astype(int) + r.integers(-20, 21, (k, 3)), 0, 255).astype(np.uint8)
        if seed == 4: b = r.integers(lo, lo + span, (k, 3)).astype(np.int16)
        out.append((a, ca, b, cb))
    return out


def merge(xyz, rgb):
    """removeDuplicate, dropDuplicates = 2: one point per voxel, channels sum / count in integer division -> (points, colours, a voxel with >= 3 points of different colours exists)"""
    u, inv, cnt = np.unique(np.asarray(xyz, np.int64), axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    sums = np.zeros((len(u), 3), np.int64); np.add.at(sums, inv, np.asarray(rgb, np.int64))
    mixed = False
    for v in np.nonzero(cnt >= 3)[0][:200]:
        if len(np.unique(np.asarray(rgb)[inv == v], axis=0)) >= 2: mixed = True; break
    return u, sums // cnt[:, None], mixed


def one_way(P, cP, Q, cQ):
    """brute force P -> Q: integer sums of squared error terms [Y, U, V], and the share of queries with ties / whether a tie mean landed on .5, and the float form's mse"""
    d = ((P[:, None, :] - Q[None, :, :]) ** 2).sum(-1)
    T = d == d.min(1, keepdims=True)
    n = T.sum(1).astype(np.int64)
    s = T.astype(np.int64) @ cQ
    mean = (2 * s + n[:, None]) // (2 * n[:, None])                       # round half up of s / n
    half = bool(((n[:, None] > 1) & ((2 * s) % (2 * n[:, None]) == n[:, None])).any())
    dr, dg, db = (cP - mean).T
    e = np.stack([2126 * dr + 7152 * dg + 722 * db, -1146 * dr - 3854 * dg + 5000 * db, 5000 * dr - 4542 * dg - 458 * db])
    sse = [int(x) for x in (e * e).sum(1)]
    # the reference's text: convertRGBtoYUVBT709 in double, rounded to float (:50-55); pow(yuvA - yuvB, 2.F) on floats (:178); summed in double, / num, cast to float (:223)
    def yuv709(c):
        c = c.astype(F64)
        return np.stack([((0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]) / 255.0).astype(F32),
                         ((-0.1146 * c[:, 0] - 0.3854 * c[:, 1] + 0.5000 * c[:, 2]) / 255.0 + 0.5000).astype(F32),
                         ((0.5000 * c[:, 0] - 0.4542 * c[:, 1] - 0.0458 * c[:, 2]) / 255.0 + 0.5000).astype(F32)])
    df = yuv709(cP) - yuv709(mean)
    assert df.dtype == F32
    sq = df * df                                                           # float square (the worse of the two readings of pow(float, 2.F) for the bound below)
    mse_float = [F32(x.astype(F64).sum() / len(P)) for x in sq]
    return sse, float((n > 1).mean()), half, mse_float


LIBM = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
LIBM.log10f.restype = ctypes.c_float
LIBM.log10f.argtypes = [ctypes.c_float]


def derived(sse, n):
    """mse = (float)(sse / (2550000^2 n)), psnr = 10 log10f(1 / mse)"""
    mse = F32(F64(sse) / (F64(2550000.0) * F64(2550000.0) * F64(n)))
    with np.errstate(divide="ignore"):
        inv = F32(1.0) / mse
    psnr = F32(10) * F32(LIBM.log10f(ctypes.c_float(float(inv)))) if mse > 0 else F32(np.inf)
    return mse, psnr


def check_derived(got):
    for d, n in (("ab", got["n_a"]), ("ba", got["n_b"])):
        for c in range(3):
            mse, psnr = derived(got["sse_" + d][c], n)
            assert F32(got["mse_" + d][c]) == mse and F32(got["psnr_" + d][c]) == psnr, (d, c, got["mse_" + d][c], mse, got["psnr_" + d][c], psnr)
    for c in range(3):
        assert got["mse"][c] == max(got["mse_ab"][c], got["mse_ba"][c]) and got["psnr"][c] == min(got["psnr_ab"][c], got["psnr_ba"][c])


def check_metric_case(ctx, case):
    a, ca, b, cb = case
    assert len(a) <= 3000 and len(b) <= 3000
    A, mA, mixA = merge(a, ca); B, mB, mixB = merge(b, cb)
    ab, tie_ab, half_ab, f_ab = one_way(A, mA, B, mB)
    ba, tie_ba, half_ba, f_ba = one_way(B, mB, A, mA)
    # conditions on the cases: no case can pass empty
    assert mixA and mixB, "no voxel with >= 3 duplicates of different colours"
    assert tie_ab >= 0.05 and tie_ba >= 0.05, (tie_ab, tie_ba)
    assert half_ab and half_ba, "no tie mean lands on .5"
    got = ctx.color_metric(a, ca, b, cb)
    assert (got["n_a"], got["n_b"]) == (len(A), len(B))
    assert got["sse_ab"] == ab and got["sse_ba"] == ba, (got["sse_ab"], ab, got["sse_ba"], ba)
    check_derived(got)
    # the float form lies within 2 sqrt(mse) eps + eps^2 of the integer form, eps = 2^-22: every yuv value is one rounding to float of a number below 1 (<= 2^-25 each),
    # the float subtraction one more (<= 2^-25), so a point's difference is off by at most 3 * 2^-25; Cauchy-Schwarz carries that to the mean of the squares; eps is
    # doubled for the float cast of the mean
    eps = 2.0 ** -22
    for d, fl in (("ab", f_ab), ("ba", f_ba)):
        for c in range(3):
            m = float(got["mse_" + d][c])
            assert abs(float(fl[c]) - m) <= 2 * np.sqrt(m) * eps + eps * eps, (d, c, float(fl[c]), m)
    sw = ctx.color_metric(b, cb, a, ca)                                    # swapping a and b swaps the directions
    assert sw["sse_ab"] == got["sse_ba"] and sw["sse_ba"] == got["sse_ab"] and (sw["n_a"], sw["n_b"]) == (got["n_b"], got["n_a"]) and sw["psnr"] == got["psnr"]
    return got


def check_metric_identity_and_bad_arguments(ctx, R):
    a, ca, b, cb = metric_cases()[0]
    same = ctx.color_metric(a, ca, a, ca)
    assert same["sse_ab"] == [0, 0, 0] and same["sse_ba"] == [0, 0, 0] and all(np.isinf(x) and x > 0 for x in same["psnr"] + same["psnr_ab"] + same["psnr_ba"]) and same["mse"] == [0, 0, 0]
    check_derived(same)
    # a shuffled copy with its duplicates is the same merged cloud
    perm = np.random.default_rng(1).permutation(len(a))
    assert ctx.color_metric(a, ca, a[perm], ca[perm])["sse_ab"] == [0, 0, 0]
    one = np.array([[5, 5, 5]], np.int16); col = np.array([[1, 2, 3]], np.uint8)
    bad = [(np.array([[0, 0, 1024]], np.int16), col, one, col), (one, col, np.array([[-1, 0, 0]], np.int16), col), (np.zeros((0, 3), np.int16), np.zeros((0, 3), np.uint8), one, col),
           (one, col, np.zeros((0, 3), np.int16), np.zeros((0, 3), np.uint8)), (one, None, one, col), (one, col, one, None)]
    for args in bad:
        try:
            ctx.color_metric(*args)
            raise AssertionError("accepted")
        except R.RbtError as e:
            assert e.code == -4
    got = ctx.color_metric(one, col, np.array([[5, 5, 6], [5, 6, 5]], np.int16), np.array([[1, 2, 4], [1, 2, 7]], np.uint8))   # the context still works: mean of (4, 7) = 5.5 -> 6
    assert got["sse_ab"] == [(722 * -3) ** 2, (5000 * -3) ** 2, (-458 * -3) ** 2] and got["n_b"] == 2


def large_clouds(n=120000, seed=5):
    """two clouds of >= 100 000 points each with duplicates, ties and a few outliers, for GPU == host emulation"""
    r = np.random.default_rng(seed)
    a = r.integers(200, 260, (n, 3)).astype(np.int16)
    ca = r.integers(0, 256, (n, 3)).astype(np.uint8)
    pick = r.permutation(n)[: n * 9 // 10]
    b = np.clip(a[pick] + r.integers(-2, 3, (len(pick), 3)), 0, 1023).astype(np.int16)
    cb = np.clip(ca[pick].astype(int) + r.integers(-30, 31, (len(pick), 3)), 0, 255).astype(np.uint8)
    b = np.concatenate([b, np.array([[900, 40, 300], [0, 0, 0], [1023, 1023, 1023]], np.int16)]); cb = np.concatenate([cb, np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)])
    return a, ca, b, cb
