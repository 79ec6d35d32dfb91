"""Seeded random atlases for the verification-stage tests (shared by the CPU and the GPU test)."""
import numpy as np
import pytest


def random_atlas(R, seed, w=None, h=None):
    r = np.random.default_rng(1000 + seed)
    res = 16
    prec = [1, 2, 4, 2][seed % 4]
    w = w or int(r.integers(4, 9)) * res
    h = h or int(r.integers(4, 9)) * res
    bw, bh = w // res, h // res
    used = np.zeros((bh, bw), bool)
    patches = []
    for _ in range(40):
        su, sv = int(r.integers(1, 4)), int(r.integers(1, 4))
        orient = int(r.integers(0, 8))
        sw, sh = (sv, su) if orient in (1, 5, 6, 7) else (su, sv)       # SWAP, ROT270, MROT90, ROT90 exchange the axes on the canvas
        if sw > bw or sh > bh: continue
        u0, v0 = int(r.integers(0, bw - sw + 1)), int(r.integers(0, bh - sh + 1))
        overlap = used[v0:v0 + sh, u0:u0 + sw].any()
        if overlap and r.random() < 0.8: continue                       # a few overlapping patches: the later one owns the shared blocks
        used[v0:v0 + sh, u0:u0 + sw] = True
        axes = [int(x) for x in r.permutation(3)]
        pm = int(r.integers(0, 2))
        patches.append(R.Patch(u0, v0, su, sv, int(r.integers(0, 300)), int(r.integers(0, 300)), int(r.integers(0, 200)) + (300 if pm else 0), axes[0], axes[1], axes[2], pm, orient,
                               1 if r.random() < 0.8 else 2, 1))
    occ_full = (r.random((h // prec, w // prec)) < 0.7)
    occ_full &= np.kron(used, np.ones((res // prec, res // prec), bool))
    thr = 0
    if seed % 3 == 0: occ = occ_full.astype(np.uint16) * int(r.integers(1, 255))
    else: occ = occ_full.astype(np.uint16)
    if seed % 8 == 7:
        # lossy occupancy (thresholdLossyOM = 2): samples in 1..2 are NOT occupied and must not make a patch own a block (PCCCodec.cpp:1599-1600 binarises the frame
        # before generateBlockToPatchFromOccupancyMapVideo :1754 reads it); some blocks hold nothing but such samples
        thr = 2
        low = np.kron(r.random((bh, bw)) < 0.4, np.ones((res // prec, res // prec), bool))
        occ = np.where(occ_full, np.where(low, r.integers(1, 3, occ_full.shape), r.integers(3, 200, occ_full.shape)), 0).astype(np.uint16)
    d0 = r.integers(0, 1024, (h, w)).astype(np.uint16)
    d1 = np.clip(d0.astype(int) + r.integers(0, 12, (h, w)) * (r.random((h, w)) < 0.5), 0, 1023).astype(np.uint16)
    t0 = r.integers(0, 1024, w * h * 3 // 2).astype(np.uint16)
    t1 = r.integers(0, 1024, w * h * 3 // 2).astype(np.uint16)
    atlas = R.AtlasParams(w, h, res, prec, 2, 1 if seed % 5 else 0, 1 if seed % 7 != 6 else 0, thr)
    return atlas, patches, occ, d0, d1, 10, t0, t1, 10


def seam_atlas(R, seed, tiles=4, prec=1, two_axes=False, noise=1):
    """A dense surface cut into patches that MEET in 3-D, the situation geometry smoothing exists for (PCCCodec::smoothPointCloudPostprocess): tiles x tiles patches of
    2 x 2 blocks, each occupied but for a margin of 2 pixels (so its border points are boundary points, identifyBoundaryPoints), placed 28 apart in space so that the occupied
    areas of neighbours abut; depth = a smooth surface + an offset per patch (the seam a lossy geometry codec leaves) + noise; the far map a few levels behind.
    two_axes: every other patch projects along another axis (points of different patches then share cells away from the seams too); noise: amplitude of the depth noise."""
    r = np.random.default_rng(7000 + seed)
    res, w = 16, tiles * 32
    patches, occ_full = [], np.zeros((w, w), bool)
    yy, xx = np.mgrid[0:w, 0:w]
    surf = 60 + 25 * np.sin(xx / 37.0 + seed) + 20 * np.cos(yy / 29.0)
    d0 = np.zeros((w, w))
    for j in range(tiles):
        for i in range(tiles):
            k = j * tiles + i
            flip = two_axes and (k % 2 == 1)
            axes = (1, 2, 0) if flip else (2, 0, 1)               # normal, tangent, bitangent
            patches.append(R.Patch(2 * i, 2 * j, 2, 2, 40 + 28 * i, 40 + 28 * j, 30, axes[0], axes[1], axes[2], 0, 0, 1, 1))
            sl = (slice(32 * j, 32 * j + 32), slice(32 * i, 32 * i + 32))
            occ_full[32 * j + 2:32 * j + 30, 32 * i + 2:32 * i + 30] = True
            d0[sl] = surf[sl] + int(r.integers(-6, 7)) + r.integers(-noise, noise + 1, (32, 32))
    holes = r.random((w, w)) < 0.01
    occ_full &= ~holes
    if prec > 1: occ_full = np.kron(occ_full[::prec, ::prec], np.ones((prec, prec), bool))
    d0 = np.clip(d0, 0, 255).astype(np.uint16) * 4                 # 10-bit video samples of 8-bit depths
    d1 = np.clip(d0 + 4 * r.integers(0, 4, (w, w)), 0, 1023).astype(np.uint16)
    occ = occ_full[::prec, ::prec].astype(np.uint16)
    t0 = r.integers(0, 1024, w * w * 3 // 2).astype(np.uint16)
    t1 = r.integers(0, 1024, w * w * 3 // 2).astype(np.uint16)
    atlas = R.AtlasParams(w, w, res, prec, 2, 1, 1, 0, 1, [8, 8, 4, 16, 6][seed % 5], [64, 64, 16, 64, 1][seed % 5])
    return atlas, patches, occ, d0, d1, 10, t0, t1, 10


def _copy_atlas(R, atlas, **kw):
    a = R.AtlasParams(*[getattr(atlas, n) for n, _ in R.AtlasParams._fields_])
    for k, v in kw.items(): setattr(a, k, v)
    return a


EDGE_GRIDS = (2, 4, 6, 8, 16, 254)


def edge_residues(g):
    return range(g) if g <= 16 else (0, 1, g // 2 - 1, g // 2, g // 2 + 1, g - 1)


def edge_atlas(R, g, axis, residue, seed=0):
    """seam_atlas moved so that the cloud's largest coordinate lies on `axis` (0 x, 1 y, 2 z) and is `residue` modulo the grid size g: the grid of the smoothing spans that
    coordinate (w = ceil(max / g) cells a side), so the residue decides where in the last cell the outermost points sit and which of them pc_sm_skip lets through.
    -> (case, largest coordinate)"""
    import oracle_lib as O
    case = seam_atlas(R, seed, tiles=3)
    atlas = _copy_atlas(R, case[0], grid_size=g, threshold_smoothing=1 if g <= 4 else 64)
    field = ("u1", "v1", "d1")[axis]                              # the patches project along z: tangent = x (u1), bitangent = y (v1), normal = z (d1)
    low = max(0, g // 2 - 30)                                     # (the cloud starts near 40: keep it clear of the lower skip margin of a large grid)
    for p in case[1]: p.u1 += low; p.v1 += low; p.d1 += low
    mx = O.reconstruct(_copy_atlas(R, atlas, geometry_smoothing=0), *case[1:])[0].max(axis=0).astype(int)
    t = max(int(mx.max()) + 1, int(mx[axis]))
    t += (residue - t) % g
    for p in case[1]: setattr(p, field, getattr(p, field) + t - int(mx[axis]))
    return (atlas,) + tuple(case[1:]), t


def check_grid_edge(ctx, g, axis):
    """even grid sizes with the cloud's largest coordinate at every residue modulo g along one axis: points, their order, colours and the count of moved points == oracle,
    and the smoothing moves points in at least one of the clouds (the edge is not passed over by the skip rule alone)"""
    import oracle_lib as O
    R = __import__("rbt_lib").module()
    most = 0
    for residue in edge_residues(g):
        case, t = edge_atlas(R, g, axis, residue)
        plain = O.reconstruct(_copy_atlas(R, case[0], geometry_smoothing=0), *case[1:])[0]
        assert int(plain.max()) == t and int(plain[:, axis].max()) == t and t % g == residue and plain.shape[0] > 5000
        got, want = ctx.reconstruct(*case), O.reconstruct(*case)
        assert got[0].shape == want[0].shape
        for a, b in zip(got, want):
            assert np.array_equal(a, b), (g, axis, residue)
        assert ctx.n_smoothed == O.LAST_SMOOTHED, (g, axis, residue)
        most = max(most, ctx.n_smoothed)
    # Grid size 2 is the one grid that cannot move a point, whatever the cloud: a point moves when cnt * |P - c|^2 + 0.5 >= 2 * max(threshold, cnt), c the trilinear blend of
    # the eight cell centres (an empty cell counts as P). Along each axis the four cells on P's side of the blend hold coordinates P - 1 .. P (or P .. P + 1) and weigh 3/4
    # together, the four on the other side lie 1 .. 2 away and weigh 1/4, and the two pull in opposite directions: |P - c| <= 0.75 per axis, |P - c|^2 < 1.6875. That leaves
    # cnt = 1 (needs 1.5), i.e. fewer than five points in P's own cell (weight 27/64 each), and with so few - P itself among them - the own cell's centre cannot lie far
    # enough towards one corner on all three axes at once (best case 1.25). 3000 random sparse clouds through smooth_reference moved none either. So 2 is held to the oracle.
    assert most > 0 or g == 2, "no cloud of grid size %d had a point moved" % g


def check_odd_grid_refused(ctx):
    """rbt.h: grid_size 2..255, even. An odd grid would index one cell past the w^3 cell arrays (rbt_pcc.cpp); it is refused and the context works afterwards"""
    import oracle_lib as O
    R = __import__("rbt_lib").module()
    case = seam_atlas(R, 0, tiles=3)
    for g in (3, 5, 7, 255):
        try:
            ctx.reconstruct(_copy_atlas(R, case[0], grid_size=g), *case[1:])
            raise AssertionError("grid_size %d accepted" % g)
        except R.RbtError as e:
            assert e.code == -4, (g, str(e))                       # RBT_ERR_PARAM
    got, want = ctx.reconstruct(*case), O.reconstruct(*case)
    assert got[0].shape[0] > 5000 and all(np.array_equal(a, b) for a, b in zip(got, want)) and ctx.n_smoothed == O.LAST_SMOOTHED > 0


def d2_cases():
    """(a, normals_a, b) clouds for the point-to-plane metric: axis normals and slanted ones, duplicates on both sides, a sparse
    reconstruction (points of B that no source point is nearest to take their normal from the source) and an outlier"""
    out = []
    for seed in range(4):
        r = np.random.default_rng(40 + seed)
        a = r.integers(100, 140, (3000, 3)).astype(np.int16)
        if seed % 2:
            n = np.zeros((3000, 3), np.int16); n[np.arange(3000), r.integers(0, 3, 3000)] = 16384 * r.choice([-1, 1], 3000)
        else:
            v = r.normal(size=(3000, 3)); n = np.round(16384 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.int16)
        b = np.clip(a[r.permutation(3000)[:2500 if seed < 3 else 300]] + r.integers(-2, 3, (2500 if seed < 3 else 300, 3)), 0, 1023).astype(np.int16)
        if seed == 2: b = np.concatenate([b, np.array([[230, 40, 300]], np.int16)])
        out.append((a, n, b))
    return out


def d2_brute_force(a, n, b):
    """the definition, by brute force on the merged points: (sum A -> B, sum B -> A, unique A, unique B)"""
    ua, ia = np.unique(a, axis=0, return_index=True); ub = np.unique(b, axis=0)
    na = n[ia].astype(np.float64)          # np.unique returns the FIRST occurrence: the lowest original index
    A, B = ua.astype(np.int64), ub.astype(np.int64)
    d = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)
    tie_ab = d == d.min(1, keepdims=True); tie_ba = d == d.min(0, keepdims=True)
    acc = tie_ab.T.astype(np.float64) @ na; cnt = tie_ab.sum(0).astype(np.float64)
    for j in np.nonzero(cnt == 0)[0]:
        acc[j] = na[tie_ba[:, j]].sum(0); cnt[j] = tie_ba[:, j].sum()
    nb = acc / cnt[:, None]
    s_ab = s_ba = 0.0
    for i in range(len(A)):
        js = np.nonzero(tie_ab[i])[0]
        s_ab += np.mean(((A[i] - B[js]) * nb[js]).sum(1) ** 2)
    for j in range(len(B)):
        ii = np.nonzero(tie_ba[:, j])[0]
        s_ba += np.mean(((B[j] - A[ii]) * na[ii]).sum(1) ** 2)
    q = 16384.0 ** 2
    return s_ab / q, s_ba / q, len(A), len(B)


def check_d2(ctx):
    import oracle_lib as O
    for a, n, b in d2_cases():
        got, want = ctx.d2(a, n, b), O.d2(a, n, b)
        assert (got["n_a"], got["n_b"]) == (want["n_a"], want["n_b"])
        for k in ("sse_ab", "sse_ba", "max_ab", "max_ba"):
            assert got[k] == pytest.approx(want[k], rel=1e-9), k          # sums of doubles in another order
        assert got["psnr"] == pytest.approx(want["psnr"], abs=1e-4) and got["psnr_ab"] == pytest.approx(want["psnr_ab"], abs=1e-4)
        s_ab, s_ba, n_a, n_b = d2_brute_force(a, n, b)
        assert (n_a, n_b) == (want["n_a"], want["n_b"]) and want["sse_ab"] == pytest.approx(s_ab, rel=1e-9) and want["sse_ba"] == pytest.approx(s_ba, rel=1e-9)
        # planes cannot be further away than points: D2 <= D1 per direction
        d1 = ctx.d1(a, b)
        assert got["sse_ab"] <= d1["sse_ab"] * (1 + 1e-9) and got["sse_ba"] <= d1["sse_ba"] * (1 + 1e-9)
    a, n, _ = d2_cases()[0]
    assert ctx.d2(a, n, a)["sse_ab"] == 0


def smooth_reference(xyz, boundary, partition, g, threshold):
    """Geometry smoothing once more, in numpy / Python straight from the reference's text (PCCCodec.cpp:52-145, :980-1104) with its types (float32 cell centres, float64
    filter): a second, independent writing of what oracle/pcc_recon.c smooth_grid restates, for the tests. xyz int16 [n, 3]; boundary bool [n]; partition [n] -> new xyz."""
    xyz = xyz.astype(np.int64); out = xyz.copy()
    if len(xyz) == 0: return out.astype(np.int16)
    w = (int(xyz.max()) + g - 1) // g
    disth, th = max(g // 2, 1), g * w
    inside = ~((xyz < disth).any(axis=1) | (th <= xyz + disth).any(axis=1))
    cells = {}
    lo = np.where(xyz % g < g // 2, -1, 0) + xyz // g
    for i in np.nonzero(boundary & inside)[0]:
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    cells.setdefault((lo[i, 0] + dx, lo[i, 1] + dy, lo[i, 2] + dz), [np.zeros(3, np.float32), 0, None, False])
    for j in np.nonzero(inside)[0]:
        c = cells.get(tuple(xyz[j] // g))
        if c is None: continue
        if c[1] == 0: c[2], c[3] = partition[j] + 1, False
        elif not c[3] and c[2] != partition[j] + 1: c[3] = True
        c[0] = (c[0] + xyz[j].astype(np.float32)).astype(np.float32); c[1] += 1
    for c in cells.values():
        if c[1]: c[0] = (c[0] / np.float32(c[1])).astype(np.float32)
    g2 = 2 * g
    for i in np.nonzero(boundary & inside)[0]:
        P = xyz[i]; S = lo[i]
        nb = [[[cells[(S[0] + dx, S[1] + dy, S[2] + dz)] for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
        if not any(c[3] and c[1] for pl in nb for ro in pl for c in ro): continue
        W = (P - S * g - g // 2) * 2 + 1; Q = g2 - W
        c4 = np.zeros(3, np.float64); cnt = 0
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    c = nb[dz][dy][dx]; abc = int((W[0] if dx else Q[0]) * (W[1] if dy else Q[1]) * (W[2] if dz else Q[2]))
                    c4 = c4 + (c[0].astype(np.float64) if c[1] > 0 else P.astype(np.float64)) * np.float64(abc)
                    cnt += abc * c[1]
        c4 = c4 / np.float64(g2 ** 3); cnt //= g2 ** 3
        if cnt == 0: continue
        centroid = c4 * np.float64(cnt)
        d = P.astype(np.float64) * np.float64(cnt) - centroid
        dist2 = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / np.float64(cnt) + 0.5
        if dist2 >= max(int(threshold), cnt) * 2:
            out[i] = np.floor(centroid / np.float64(cnt) + 0.5).astype(np.int64)
    return out.astype(np.int16)


def boundary_reference(om, x, y):
    """PCCCodec::identifyBoundaryPoints (:266-325) for an occupied pixel, from the text, in Python"""
    H, W = om.shape; t = False
    if 0 < y < H - 1 and (om[y - 1, x] == 0 or om[y + 1, x] == 0): t = True
    if 0 < x < W - 1 and not t and (om[y, x + 1] == 0 or om[y, x - 1] == 0): t = True
    if 0 < y < H - 1 and x > 0 and not t and (om[y - 1, x - 1] == 0 or om[y + 1, x - 1] == 0): t = True
    if 0 < y < H - 1 and x < W - 1 and not t and (om[y - 1, x + 1] == 0 or om[y + 1, x + 1] == 0): t = True
    if y in (0, H - 1) or x in (0, W - 1): t = True
    if not t:
        for ix in range(-2, 3):
            for iy in range(-2, 3):
                if (abs(ix) > 1 or abs(iy) > 1) and 0 <= y + iy < H and 0 <= x + ix < W and om[y + iy, x + ix] == 0: t = True
        if y in (1, H - 2) or x in (1, W - 2): t = True
    return t
