"""One transform block reconstructed the way the TEXT of Rec. ITU-T H.265 (v1 tools, 4:2:0) says, in exact integers: NumPy int64 / Python ints only, nothing is ever stored
in 16 bits. Written from the clauses; it imports nothing of the product, of the oracle or of their tables - the transform matrices come from
tests/golden/hevc_rom_tables.json (compiled from the reference's ROM), the angle tables are Tables 8-5 / 8-6 typed in.

    8.4.4.2.2  substitution of reference samples that are not available        substitute()
    8.4.4.2.3  filtering of the reference samples (filterFlag, both filters)     filter_refs()
    8.4.4.2.4  planar   8.4.4.2.5  DC   8.4.4.2.6  angular 2..34                   predict()
    8.6.2      residual of a block: bypass, scaling, transformation, bdShift     residual()
    8.6.3      scaling with flat lists (m = 16)                                  scale()
    8.6.4.2    transform skip (<< 7), DST 4x4 intra luma, DCT 4..32               transform()
    8.6.7      picture construction Clip1(pred + res)                            reconstruct()

Reference samples are held in ONE array of 4N+1 entries in the order the kernels and the oracle use too (it is the order 8.4.4.2.2 searches in):
index 0 = p[-1][2N-1] ... 2N-1 = p[-1][0], 2N = p[-1][-1], 2N+1+x = p[x][-1].  p[x][y]: x to the right, y downwards, as in the text."""
import json
import os
import numpy as np

_G = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hevc_rom_tables.json")))
DCT = {n: np.array(_G["T%d" % n], dtype=np.int64).reshape(n, n) for n in (4, 8, 16, 32)}      # transMatrix rows 0, 32/n, 2*32/n, ... and columns 0..n-1 (8.6.4.2)
DST = np.array(_G["DST4"], dtype=np.int64).reshape(4, 4)
LEVEL_SCALE = (40, 45, 51, 57, 64, 72)                                                         # 8.6.3
COEFF_MIN, COEFF_MAX = -32768, 32767                                                           # CoeffMinY / CoeffMaxY without extended_precision_processing
# Table 8-5: intraPredAngle for predModeIntra 2..34
INTRA_PRED_ANGLE = dict(zip(range(2, 35), (32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26, -32, -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32)))
# Table 8-6: invAngle for predModeIntra 11..25
INV_ANGLE = dict(zip(range(11, 26), (-4096, -1638, -910, -630, -482, -390, -315, -256, -315, -390, -482, -630, -910, -1638, -4096)))


def clip3(lo, hi, v):
    return np.minimum(hi, np.maximum(lo, v))


# ------------------------------------------------------------------------------------------------------------------ 8.4.4.2.2
def substitute(samples, avail, bit_depth):
    """samples, avail: 4N+1 entries in search order -> the 4N+1 reference samples p (int64)"""
    n = len(samples)
    av = [bool(a) for a in avail]
    if not any(av):
        return np.full(n, 1 << (bit_depth - 1), dtype=np.int64)
    p = [int(v) for v in samples]
    if not av[0]:                                     # search from p[-1][2N-1] up to p[-1][-1], then p[0][-1] .. p[2N-1][-1]; the first available one is taken
        p[0] = p[av.index(True)]
    for i in range(1, n):                             # then, in the same order, one that is not available takes the one before it
        if not av[i]:
            p[i] = p[i - 1]
    return np.array(p, dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------------ 8.4.4.2.3
def filter_flag(c_idx, n, mode):
    if c_idx != 0 or mode == 1 or n == 4:
        return False
    min_dist_ver_hor = min(abs(mode - 26), abs(mode - 10))
    return min_dist_ver_hor > {8: 7, 16: 1, 32: 0}[n]


def filter_refs(p, n, bit_depth, strong_intra_smoothing):
    """p -> pF"""
    c = 2 * n                                          # index of p[-1][-1]
    pf = p.copy()
    bi_int = (strong_intra_smoothing and n == 32 and
              abs(int(p[c]) + int(p[c + 2 * n]) - 2 * int(p[c + n])) < (1 << (bit_depth - 5)) and          # p[-1][-1] + p[2N-1][-1] - 2 p[N-1][-1]
              abs(int(p[c]) + int(p[c - 2 * n]) - 2 * int(p[c - n])) < (1 << (bit_depth - 5)))             # p[-1][-1] + p[-1][2N-1] - 2 p[-1][N-1]
    if bi_int:
        k = np.arange(63, dtype=np.int64)
        pf[c - 1 - k] = ((63 - k) * p[c] + (k + 1) * p[c - 64] + 32) >> 6                                 # pF[-1][y], y = 0..62
        pf[c + 1 + k] = ((63 - k) * p[c] + (k + 1) * p[c + 64] + 32) >> 6                                 # pF[x][-1], x = 0..62
    else:
        pf[1:-1] = (p[:-2] + 2 * p[1:-1] + p[2:] + 2) >> 2                                                # every sample but the two ends, its two neighbours in the array
    return pf


# ------------------------------------------------------------------------------------------------------------------ 8.4.4.2.4 - 8.4.4.2.6
def predict(p, c_idx, log2, mode, bit_depth):
    """the final reference samples p (4N+1) -> predSamples as [y][x] (int64)"""
    n = 1 << log2
    c = 2 * n
    left = lambda y: p[c - 1 - np.asarray(y)]          # p[-1][y], y = -1 .. 2N-1
    top = lambda x: p[c + 1 + np.asarray(x)]           # p[x][-1], x = -1 .. 2N-1
    y, x = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
    edge = c_idx == 0 and n < 32
    max_v = (1 << bit_depth) - 1
    if mode == 0:                                                                                         # (8-29)
        return ((n - 1 - x) * left(y) + (x + 1) * top(n) + (n - 1 - y) * top(x) + (y + 1) * left(n) + n) >> (log2 + 1)
    if mode == 1:
        k = np.arange(n)
        dc = (int(top(k).sum()) + int(left(k).sum()) + n) >> (log2 + 1)
        pred = np.full((n, n), dc, dtype=np.int64)
        if edge:
            pred[0, 0] = (left(0) + 2 * dc + top(0) + 2) >> 2
            pred[0, 1:] = (top(k[1:]) + 3 * dc + 2) >> 2
            pred[1:, 0] = (left(k[1:]) + 3 * dc + 2) >> 2
        return pred
    ang = INTRA_PRED_ANGLE[mode]
    ref = {}                                                                                              # ref[x], x = -N .. 2N
    main, side = (top, left) if mode >= 18 else (left, top)
    for i in range(0, n + 1):
        ref[i] = int(main(i - 1))
    if ang < 0:
        if (n * ang) >> 5 < -1:
            for i in range((n * ang) >> 5, 0):
                ref[i] = int(side(-1 + ((i * INV_ANGLE[mode] + 128) >> 8)))
    else:
        for i in range(n + 1, 2 * n + 1):
            ref[i] = int(main(i - 1))
    lo = min(ref)
    r = np.array([ref[i] for i in range(lo, max(ref) + 1)], dtype=np.int64)
    a, b = (y, x) if mode >= 18 else (x, y)            # a: the coordinate the angle advances along
    i_idx, i_fact = ((a + 1) * ang) >> 5, ((a + 1) * ang) & 31
    whole = r[b + i_idx + 1 - lo]
    frac = ((32 - i_fact) * whole + i_fact * r[np.minimum(b + i_idx + 2 - lo, len(r) - 1)] + 16) >> 5      # the second sample is not read when iFact is 0
    pred = np.where(i_fact != 0, frac, whole)
    if mode == 26 and edge:
        pred[:, 0] = clip3(0, max_v, top(0) + ((left(np.arange(n)) - left(-1)) >> 1))
    if mode == 10 and edge:
        pred[0, :] = clip3(0, max_v, left(0) + ((top(np.arange(n)) - top(-1)) >> 1))
    return pred


def intra(samples, avail, c_idx, log2, mode, bit_depth, strong_intra_smoothing):
    p = substitute(samples, avail, bit_depth)
    if filter_flag(c_idx, 1 << log2, mode):
        p = filter_refs(p, 1 << log2, bit_depth, strong_intra_smoothing)
    return predict(p, c_idx, log2, mode, bit_depth)


# ------------------------------------------------------------------------------------------------------------------ 8.6.2 - 8.6.4
def scale(levels, log2, qp, bit_depth):
    """TransCoeffLevel [y][x] -> d (8-309), m = 16"""
    bd_shift = bit_depth + log2 - 5
    lv = np.asarray(levels, dtype=np.int64)
    return clip3(COEFF_MIN, COEFF_MAX, ((lv * 16 * LEVEL_SCALE[qp % 6] << (qp // 6)) + (1 << (bd_shift - 1))) >> bd_shift)


def transform(d, log2, use_dst, transform_skip):
    """d [y][x] -> r before the bdShift of 8.6.2"""
    if transform_skip:
        return d << 7                                                                                    # rotation and extended shifts are range-extension tools
    m = DST if use_dst else DCT[1 << log2]              # y[i] = sum_j transMatrix[j][i] * x[j]
    e = m.T @ d                                          # each column: e[y][x] = sum_j m[j][y] d[j][x]
    g = clip3(COEFF_MIN, COEFF_MAX, (e + 64) >> 7)
    return g @ m                                         # each row:    r[y][x] = sum_j g[y][j] m[j][x]


def residual(levels, c_idx, log2, qp, bit_depth, is_intra, transform_skip, cu_transquant_bypass):
    """the residual r [y][x] of a coded block, exact (no storage width)"""
    lv = np.asarray(levels, dtype=np.int64).reshape(1 << log2, 1 << log2)
    if cu_transquant_bypass:
        return lv
    r = transform(scale(lv, log2, qp, bit_depth), log2, bool(is_intra) and c_idx == 0 and log2 == 2, transform_skip)
    bd_shift = 20 - bit_depth
    return (r + (1 << (bd_shift - 1))) >> bd_shift


def reconstruct(pred, res, bit_depth):
    return clip3(0, (1 << bit_depth) - 1, np.asarray(pred, dtype=np.int64) + res)                        # 8.6.7


def block(c_idx, log2, bit_depth, strong_intra_smoothing, is_intra, mode, cbf, transform_skip, cu_transquant_bypass, qp, samples, avail, levels):
    """-> (pred or None, res or None): the prediction of an intra block [y][x] and the exact residual of a coded one"""
    pred = intra(samples, avail, c_idx, log2, mode, bit_depth, strong_intra_smoothing) if is_intra else None
    res = residual(levels, c_idx, log2, qp, bit_depth, is_intra, transform_skip, cu_transquant_bypass) if cbf else None
    return pred, res
