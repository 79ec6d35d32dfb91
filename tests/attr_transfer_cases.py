"""Cases and a brute-force restatement for the attribute transfer after geometry smoothing (rbt_transfer_colors, rbt_reconstruct_decoded), shared by the host-emulation
test (tests/test_attr_transfer.py) and the GPU test (tests/test_gpu_attr_transfer.py).

The restatement is written from the definition in include/rbt.h (what PCCPointSet3::transferColors16bitBP, PCCPointSet.cpp:1126-1485, reduces to with the arguments of
PCCDecoder.cpp:434-494), not from the product code: O(moved x points), doubles are Python floats added in the stated order, round is libm's (half away from zero; np.round
is half-to-even and would be wrong here), sqrt and / are IEEE double operations."""
import ctypes
import ctypes.util
import math
import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.round.restype = ctypes.c_double
_libm.round.argtypes = [ctypes.c_double]


def clip16(v):
    return int(min(max(_libm.round(v), 0.0), 65535.0))


def transfer_reference(sxyz, syuv, txyz, tyuv, moved):
    """-> (colours after, n_changed, {"identical", "forward", "single", "multi"}: moved points per branch of the definition)"""
    S, T = np.asarray(sxyz, np.int64).reshape(-1, 3), np.asarray(txyz, np.int64).reshape(-1, 3)
    sc = [[int(v) for v in row] for row in np.asarray(syuv).reshape(-1, 3)]
    tc = [[int(v) for v in row] for row in np.asarray(tyuv).reshape(-1, 3)]
    sidx = np.arange(len(S))
    mv = [int(u) for u in np.nonzero(np.asarray(moved).reshape(-1))[0]]
    color1, E, identical = {}, [], set()
    for u in mv:                                                     # forward
        d = ((S - T[u]) ** 2).sum(1)
        nn = np.lexsort((sidx, d))[:8]                               # ascending by (distance, source index)
        assert len(nn) == 8
        if d[nn[0]] == 0:
            color1[u] = list(sc[nn[0]]); identical.add(u)
        else:
            acc, sw = [0.0, 0.0, 0.0], 0.0
            for i in nn:
                w = 1.0 / (float(d[i]) + 4.0)
                for k in range(3): acc[k] += float(sc[i][k]) * w
                sw += w
            color1[u] = [clip16(acc[k] / sw) for k in range(3)]
        E.extend(int(i) for i in nn)
    L, nearest = {}, {}
    for pos, i in enumerate(E):                                      # backward; the nearest target point of a source point does not depend on the entry
        if i not in nearest:
            d = ((T - S[i]) ** 2).sum(1)
            v = int(np.argmin(d))                                    # the first, i.e. lowest-index, minimum
            nearest[i] = (v, int(d[v]))
        v, dist = nearest[i]
        if all(abs(sc[i][k] - tc[v][k]) < 40 for k in range(3)):
            L.setdefault(v, []).append((dist, pos, sc[i]))
    out = [list(c) for c in tc]
    br = {"identical": 0, "forward": 0, "single": 0, "multi": 0}
    for u in mv:
        lst = sorted(L.get(u, []), key=lambda t: (t[0], t[1]))
        if not lst:
            out[u] = color1[u]; br["identical" if u in identical else "forward"] += 1
        elif len(lst) == 1:
            out[u] = list(lst[0][2]); br["single"] += 1
        else:
            acc, sw = [0.0, 0.0, 0.0], 0.0
            for dist, _, c in lst:
                w = 1.0 / (math.sqrt(float(dist)) + 4.0)
                for k in range(3): acc[k] += float(c[k]) * w
                sw += w
            out[u] = [clip16(acc[k] / sw) for k in range(3)]; br["multi"] += 1
    n_changed = sum(1 for u in mv if out[u] != tc[u])
    return np.array(out, np.uint16).reshape(-1, 3), n_changed, br


def _smooth_colours(r, p):
    x, y, z = p[:, 0].astype(int), p[:, 1].astype(int), p[:, 2].astype(int)
    n = len(p)
    return np.stack([2 * (x + y + z) + r.integers(0, 4, n), 30000 + 2 * x + r.integers(0, 4, n), 20000 + 2 * y + r.integers(0, 4, n)], 1).astype(np.uint16)


def surface_case(seed, colours="smooth", n=3000, doubled=False, side=40):
    """n source points on a wavy sheet three layers thick over a side x side square; the target is the same cloud with 15 % of the points flagged and displaced by up to 2 per
    axis. smooth colours: neighbours pass the |difference| < 40 test and the backward lists fill; random colours (10-bit x 64): almost every list is empty.
    doubled: every point twice, the twin with another colour - all candidates coincide in pairs and the lower index wins the ties."""
    r = np.random.default_rng(seed)
    xy = r.integers(8, 8 + side, (n, 2))
    z = 20 + np.round(6 * np.sin(xy[:, 0] / 7.0)).astype(int) + r.integers(0, 3, n)
    s = np.concatenate([xy, z[:, None]], 1).astype(np.int16)
    sc = _smooth_colours(r, s) if colours == "smooth" else (r.integers(0, 1024, (n, 3)) * 64).astype(np.uint16)
    if doubled:
        s = np.repeat(s, 2, axis=0); sc = np.repeat(sc, 2, axis=0)
        sc[1::2] = sc[1::2] + r.integers(1, 30, (n, 3)).astype(np.uint16)
    moved = r.random(len(s)) < 0.15
    t = s.copy()
    t[moved] = np.clip(t[moved].astype(int) + r.integers(-2, 3, (int(moved.sum()), 3)), 0, 1023).astype(np.int16)
    return s, sc, t, sc.copy(), moved.astype(np.uint8)


def tie_case():
    """one moved point at the centre of a full 3 x 3 x 3 block (source order shuffled): six neighbours at squared distance 1, twelve at 2 - the 7th to the 18th tie, the two
    lowest indices among them are the 7th and 8th; and the block's own centre is absent, so the forward average runs. A second moved point sits on a source position."""
    r = np.random.default_rng(77)
    g = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]) + 100
    far = r.integers(110, 130, (40, 3))
    s = np.concatenate([g, far])[r.permutation(26 + 40)].astype(np.int16)
    sc = _smooth_colours(r, s)
    t = np.concatenate([s, np.array([[100, 100, 100], [101, 100, 100]], np.int16)])
    tc = np.concatenate([sc, np.array([[600, 30200, 20200], [602, 30202, 20200]], np.uint16)])
    moved = np.zeros(len(t), np.uint8); moved[-2:] = 1
    return s, sc, t, tc, moved


def faces_case():
    """clusters in the corners (0, 0, 0), (1023, 1023, 1023) and (0, 1023, 0) of the volume with moved points on its faces: the shell walk is cut by the volume's bounds"""
    r = np.random.default_rng(78)
    parts = []
    for c in ((0, 0, 0), (1020, 1020, 1020), (0, 1020, 0)):
        parts.append(np.array(c) + r.integers(0, 4, (45, 3)))
    s = np.concatenate(parts).astype(np.int16)
    s[0] = (0, 0, 0); s[45] = (1023, 1023, 1023); s[90] = (0, 1023, 0)
    sc = _smooth_colours(r, s)
    moved = r.random(len(s)) < 0.4; moved[[0, 45, 90]] = True
    t = s.copy()
    t[moved] = np.clip(t[moved].astype(int) + r.integers(-2, 3, (int(moved.sum()), 3)), 0, 1023).astype(np.int16)
    t[0] = (0, 0, 1); t[45] = (1023, 1022, 1023)
    return s, sc, t, sc.copy(), moved.astype(np.uint8)


# eight neighbours of P = (50, 50, 50) at squared distances 2, 3, 5, 6, 8, 10, 11, 12 - none of them a square
KNOWN_OFFSETS = [(1, 1, 0), (1, 1, 1), (2, 1, 0), (2, 1, 1), (2, 2, 0), (3, 1, 0), (3, 1, 1), (2, 2, 2)]
KNOWN_D2 = [2, 3, 5, 6, 8, 10, 11, 12]
KNOWN_Y = [1000, 1010, 1020, 1005, 1031, 1013, 1002, 1037]
KNOWN_U = [30000, 30011, 30023, 30002, 30017, 30035, 30008, 30029]
KNOWN_V = [20000, 20003, 20038, 20021, 20009, 20030, 20014, 20026]
# Worked out from the definition with 60-digit decimals (python's decimal module), then rounded half away from zero. The quotients lie at least 0.06 from a rounding
# boundary, so these two cases pin the formula (which weights, which order of sqrt and + 4.0, which rounding), not the last bit of a double: that is the business of the
# surface cases, which must equal the restatement exactly over hundreds of non-square distances.
#   forward:  sum(c_i / (d_i + 4)) / sum(1 / (d_i + 4))             Y 1012.563995..., U 30013.161775..., V 20015.165967...
#   backward: sum(c_i / (sqrt(d_i) + 4)) / sum(1 / (sqrt(d_i) + 4))  Y 1014.060388..., U 30014.840085..., V 20016.873837...
KNOWN_FORWARD = (1013, 30013, 20015)
KNOWN_BACKWARD = (1014, 30015, 20017)


def known_forward_case():
    """the moved point's old colour is far from every neighbour's, so no list fills and the result is the forward average"""
    s = (np.array(KNOWN_OFFSETS) + 50).astype(np.int16)
    sc = np.stack([KNOWN_Y, KNOWN_U, KNOWN_V], 1).astype(np.uint16)
    t = np.array([[50, 50, 50]], np.int16); tc = np.array([[5000, 40000, 10000]], np.uint16)
    return s, sc, t, tc, np.array([1], np.uint8)


def known_backward_case():
    """the moved point is the only target point and its old colour is within 40 of all eight: the list holds all eight at distances sqrt(2) .. sqrt(12)"""
    s, sc, t, _, moved = known_forward_case()
    return s, sc, t, np.array([[1018, 30018, 20019]], np.uint16), moved


def check_known_answers(ctx):
    for case, want in ((known_forward_case(), KNOWN_FORWARD), (known_backward_case(), KNOWN_BACKWARD)):
        got, n_changed = ctx.transfer_colors(*case)
        ref, ref_changed, _ = transfer_reference(*case)
        assert tuple(int(v) for v in got[0]) == want == tuple(int(v) for v in ref[0]) and n_changed == ref_changed == 1


def check_case(ctx, case):
    got, n_changed = ctx.transfer_colors(*case)
    want, want_changed, br = transfer_reference(*case)
    print("moved %d, branches %s, changed %d" % (int(np.count_nonzero(case[4])), br, want_changed))
    assert np.array_equal(got, want) and n_changed == want_changed
    assert np.array_equal(got[case[4] == 0], np.asarray(case[3])[case[4] == 0])
    return br


def check_surface(ctx, seed):
    """smooth colours: every one of the four branches is taken by at least 20 points (on the restatement's own bookkeeping); random colours: the forward-only path"""
    # 3000 points over 40 x 40 give 13 to 20 single-entry lists (426-479 moved, 71-82 lists, 54-66 of them longer): the same density over 57 x 57 gives every branch its 20
    br = check_case(ctx, surface_case(seed, n=6000, side=57))
    assert all(v >= 20 for v in br.values()), br
    br = check_case(ctx, surface_case(seed, "random"))
    assert br["forward"] >= 100 and br["identical"] >= 20, br


def check_tie_rules(ctx):
    br = check_case(ctx, surface_case(5, doubled=True))
    assert br["identical"] >= 20 and br["multi"] >= 20, br
    s, sc, t, tc, moved = tie_case()
    d = ((s.astype(int) - t[-2].astype(int)) ** 2).sum(1)
    assert sorted(int(v) for v in d)[:19][:18] == [1] * 6 + [2] * 12 and sorted(int(v) for v in d)[18] > 2           # the 8th and the 9th neighbour tie
    check_case(ctx, (s, sc, t, tc, moved))
    check_case(ctx, faces_case())


def check_arguments(ctx, R):
    s, sc, t, tc, moved = surface_case(0, n=200)
    for args in ((s[:7], sc[:7], t, tc, moved), (np.where(np.arange(600).reshape(200, 3) == 31, 1024, s), sc, t, tc, moved), (s, sc, np.where(np.arange(600).reshape(200, 3) == 5, -1, t), tc, moved)):
        try:
            ctx.transfer_colors(*args)
            raise AssertionError("accepted")
        except R.RbtError as e:
            assert e.code == -4                                       # RBT_ERR_PARAM
    ctx.transfer_colors(s, sc, t, tc, moved)
    assert ctx.color_stage_ms()["transfer"] > 0
    got, n_changed = ctx.transfer_colors(s, sc, t, tc, np.zeros(len(t), np.uint8))
    assert np.array_equal(got, tc) and n_changed == 0
    assert ctx.color_stage_ms()["transfer"] == 0                     # a call with nothing to transfer reports no stage time, not the last call's
    got, n_changed = ctx.transfer_colors(s, sc, t[:0], tc[:0], moved[:0])
    assert got.shape == (0, 3) and n_changed == 0
    # flagged although it did not move: the colour of its source twin (lowest index at distance 0), whatever colour it had
    tc2 = tc.copy(); tc2[3] = (9, 9, 9); flag = np.zeros(len(s), np.uint8); flag[3] = 1
    twin = int(np.nonzero((s == s[3]).all(1))[0][0])
    got, n_changed = ctx.transfer_colors(s, sc, s, tc2, flag)
    want = tc2.copy(); want[3] = sc[twin]
    assert np.array_equal(got, want) and n_changed == 1 and np.array_equal(got, transfer_reference(s, sc, s, tc2, flag)[0])
    # a moved point out of the search's reach is refused, and the context works afterwards
    far = t.copy(); far[0] = (900, 900, 900); flag[:] = 0; flag[0] = 1
    try:
        ctx.transfer_colors(s, sc, far, tc, flag)
        raise AssertionError("accepted")
    except R.RbtError as e:
        assert e.code == -3                                           # RBT_ERR_UNSUPPORTED
    # more than 256 source points at one position, or more than 1024 entries in one list (130 moved points on a line whose 8 nearest source points are one cluster, which
    # all choose the moved point in its middle): refused, the single-lane sorts stay short
    for args in (crowded_case(), long_list_case()):
        try:
            ctx.transfer_colors(*args)
            raise AssertionError("accepted")
        except R.RbtError as e:
            assert e.code == -3
    check_case(ctx, (s, sc, t, tc, moved))


def crowded_case():
    s, sc, t, tc, moved = surface_case(0, n=200)
    s = np.concatenate([s, np.repeat(s[:1], 300, axis=0)]); sc = np.concatenate([sc, np.repeat(sc[:1], 300, axis=0)])
    return s, sc, t, tc, moved


def long_list_case():
    cluster = np.array([[100 + dx, 100 + dy, 100 + dz] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)], np.int16)
    line = np.array([[104 + k // 3, 100 + k % 3, 100] for k in range(130)], np.int16)
    t = np.concatenate([np.array([[100, 100, 100]], np.int16), line])
    sc = np.full((8, 3), 1000, np.uint16); tc = np.full((len(t), 3), 1000, np.uint16)
    return cluster, sc, t, tc, np.ones(len(t), np.uint8)


def ramp_atlas(R, seed, tiles=3):
    """seam_atlas whose attribute pictures are plateaus of one 10-bit level 16 luma samples wide (one level is 64 in 16 bits, more than the test's 40): neighbours on a
    plateau pass the colour test, so the backward lists fill"""
    import pcc_cases
    case = list(pcc_cases.seam_atlas(R, seed, tiles=tiles))
    w = case[0].width
    yy, xx = np.mgrid[0:w, 0:w]
    luma = (400 + xx // 16 + yy // 32).astype(np.uint16)
    cb = (500 + (xx[::2, ::2] // 32)).astype(np.uint16); cr = np.full((w // 2, w // 2), 520, np.uint16)
    frame = np.concatenate([luma.reshape(-1), cb.reshape(-1), cr.reshape(-1)])
    case[6] = frame; case[7] = frame.copy()
    return tuple(case)


def check_chained(ctx, R, case, lists=False):
    """rbt_reconstruct_decoded against rbt_reconstruct_rgb and the restatement -> (its six arrays, n_changed)"""
    import color_cases as CC
    import pcc_cases
    plain = list(case); plain[0] = pcc_cases._copy_atlas(R, case[0], geometry_smoothing=0)
    base = ctx.reconstruct_rgb(*case); n_sm = ctx.n_smoothed
    pre = ctx.reconstruct_rgb(*plain)
    assert n_sm > 0 and np.array_equal(base[1], pre[1])
    got = ctx.reconstruct_decoded(*case)
    moved = got[5]
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[2], base[2]) and np.array_equal(got[3], base[3])
    assert int(moved.sum()) == n_sm == ctx.n_smoothed and set(np.unique(moved)) <= {0, 1}
    assert not (pre[0][moved == 0] != base[0][moved == 0]).any()                  # what is not flagged did not move
    want, n_changed, br = transfer_reference(pre[0], pre[1], base[0], base[1], moved)
    print("points %d, moved %d, branches %s, changed %d" % (len(moved), n_sm, br, n_changed))
    assert np.array_equal(got[1], want) and ctx.n_changed == n_changed
    assert np.array_equal(got[4], CC.yuv16_to_rgb8(got[1]))
    assert np.array_equal(got[1][moved == 0], base[1][moved == 0])
    if lists: assert br["single"] + br["multi"] > 0, br
    else: assert br["forward"] > 0 or n_sm < 100, br
    off = ctx.reconstruct_decoded(*case, attr_transfer=0)
    assert all(np.array_equal(a, b) for a, b in zip(off[:5], base)) and np.array_equal(off[5], moved) and ctx.n_smoothed == n_sm and ctx.n_changed == 0
    off = ctx.reconstruct_decoded(*plain)
    assert all(np.array_equal(a, b) for a, b in zip(off[:5], pre)) and not off[5].any() and ctx.n_smoothed == 0
    return got, n_changed


def check_chained_unsupported(ctx, R):
    import pcc_cases
    case = pcc_cases.seam_atlas(R, 0, tiles=3)
    for ft in (2, 3, 5, 7, 9, -1):
        try:
            ctx.reconstruct_decoded(*case, attr_transfer=ft)
            raise AssertionError("accepted")
        except R.RbtError as e:
            assert e.code == -3


# the chained cases: grids 8, 4 and 16 (seam_atlas picks the grid by seed), one of them with patches along two axes. Grid 4 moves points only with a low threshold (as
# pcc_cases.edge_atlas sets it), and then a handful
CHAINED = [(0, False), (2, False), (3, True)]


def chained_case(R, seed, two_axes, tiles=3):
    import pcc_cases
    case = list(pcc_cases.seam_atlas(R, seed, tiles=tiles, two_axes=two_axes))
    if case[0].grid_size == 4: case[0] = pcc_cases._copy_atlas(R, case[0], threshold_smoothing=1)
    return tuple(case)
