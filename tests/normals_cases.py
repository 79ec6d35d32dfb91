"""Cases and checks of the normal estimation (rbt_pcloud_estimate_normals, rbt_estimate_normals; csrc/rbt_normals.h), shared by tests/test_normals.py (serial host emulation
of the kernel bodies) and tests/test_gpu_normals.py (the GPU build). The definition in include/rbt.h is restated by brute force in NumPy: all pairwise distances, the
neighbours sorted by (squared distance, voxel id), the integer scatter matrix, and the eigenvector from numpy.linalg.eigh - another solver than the library's Jacobi
iteration. A case's reference is computed once per process and shared.

The comparison with eigh is up to sign and covers the points whose relative eigen-gap (l1 - l0) / max(l2, 1) is at least GAP: there the eigenvector's double-precision
error is about 1e-9 against a Q14 LSB of 6e-5, and the Q14 rounding moves either side by at most half an LSB, hence a margin of 1 LSB per component. At most 1 % of a
case's points may fall under the gap (asserted from the restatement alone; measured: none on the sphere, the slab and the plane), except where the cloud itself is
degenerate: a prefix of fewer than 4 points lies in a plane or on a line, S is singular by construction and the case says what then holds instead."""
import numpy as np
import score_cases as SC

GAP = 1e-6
D1, D2, COLOR = 1, 2, 4
NONE, SPANNING_TREE, VIEW_POINT, CUBEMAP = range(4)
PREFIXES = (1, 2, 3, 15, 16, 17, 63, 64, 65)


def voxel_id(p):
    p = np.asarray(p, np.int64)
    return p[..., 2] << 20 | p[..., 1] << 10 | p[..., 0]


# ---- the clouds ----
def sphere():
    """voxelised sphere shell: radius 30, centre (200, 200, 200), voxels with |d - R| < 0.5"""
    g = np.mgrid[-31:32, -31:32, -31:32].reshape(3, -1).T
    p = g[np.abs(np.sqrt((g * g).sum(1)) - 30.0) < 0.5] + 200
    assert len(p) == 11226
    return p.astype(np.int16)


def slab(at=(100, 900, 500)):
    """slanted wavy slab, 48 x 48: z = round(0.37 u + 0.21 v + 3 sin(u / 7) + {0, 1}), the last term seeded"""
    u, v = np.mgrid[0:48, 0:48]
    z = np.round(0.37 * u + 0.21 * v + 3 * np.sin(u / 7) + np.random.default_rng(7).integers(0, 2, u.shape)).astype(int)
    return (np.stack([u.ravel(), v.ravel(), z.ravel()], 1) + np.array(at)).astype(np.int16)


def plane():
    """axis-aligned plane, 20 x 20, z = 333"""
    u, v = np.mgrid[0:20, 0:20]
    return np.stack([300 + u.ravel(), 310 + v.ravel(), np.full(400, 333)], 1).astype(np.int16)


def cube():
    return (np.mgrid[0:3, 0:3, 0:3].reshape(3, -1).T + np.array([40, 50, 60])).astype(np.int16)


def doubled_sphere():
    """every point of the sphere twice, the order shuffled"""
    p = np.concatenate([sphere(), sphere()])
    return p[np.random.default_rng(11).permutation(len(p))]


def _slab_word():
    p = slab((15, 900, 500))                                            # x = 15 .. 62: crosses the word boundary 31 | 32
    assert p[:, 0].min() < 31 and p[:, 0].max() > 32
    return p


def _slab_faces():
    s = slab((0, 0, 0)); hi = s.max(0)
    p = (s + np.array([0, 1023 - hi[1], 1023 - hi[2]])).astype(np.int16)    # touches x = 0, y = 1023 and z = 1023
    assert p[:, 0].min() == 0 and p[:, 1].max() == 1023 and p[:, 2].max() == 1023
    return p


CLOUDS = {"sphere": sphere, "slab": slab, "plane": plane, "slab_word_31_32": _slab_word, "slab_faces_0_1023": _slab_faces,
          "slab_outliers": lambda: np.concatenate([slab(), SC.OUTLIERS]), "sphere_doubled": doubled_sphere}
CLOUDS.update({"slab_prefix_%d" % n: (lambda n=n: slab()[:n]) for n in PREFIXES})
_CLOUD = {}


def cloud(name):
    if name not in _CLOUD: _CLOUD[name] = CLOUDS[name]()
    return _CLOUD[name]


# ---- the definition, by brute force ----
def restatement(pts, k=16, queries=None):
    """pts: int [n, 3], duplicates allowed. -> dict over the unique voxels (ascending voxel id), or over `queries` (voxels of pts): v (unit eigenvector of the smallest
    eigenvalue, double, sign arbitrary), gap, m, kth (squared distance of the last neighbour), tie (another voxel at exactly that distance was left out)"""
    ids, first = np.unique(voxel_id(pts), return_index=True)
    vox = np.asarray(pts, np.int64)[first]                             # ascending voxel id
    q = vox if queries is None else np.asarray(queries, np.int64)
    n, m = len(vox), min(k, len(vox))
    v = np.zeros((len(q), 3)); gap = np.zeros(len(q)); kth = np.zeros(len(q), np.int64); tie = np.zeros(len(q), bool)
    for lo in range(0, len(q), 512):
        c = q[lo:lo + 512]
        d = ((c[:, None, :] - vox[None, :, :]) ** 2).sum(-1)
        key = d << 32 | ids[None, :]
        part = np.sort(np.partition(key, m - 1, axis=1)[:, :m], axis=1) if m < n else np.sort(key, axis=1)
        nb = vox[np.searchsorted(ids, part & 0xFFFFFFFF)]               # [c, m, 3]
        kth[lo:lo + 512] = part[:, -1] >> 32
        tie[lo:lo + 512] = (d == kth[lo:lo + 512, None]).sum(1) + (d < kth[lo:lo + 512, None]).sum(1) > m
        s1 = nb.sum(1); s2 = np.einsum("cmi,cmj->cij", nb, nb)
        S = m * s2 - s1[:, :, None] * s1[:, None, :]                    # exact integers, |entry| < 2^31
        assert np.abs(S).max() < 1 << 31
        if m <= 1: continue
        w, e = np.linalg.eigh(S.astype(np.float64))
        v[lo:lo + 512] = e[:, :, 0]; gap[lo:lo + 512] = (w[:, 1] - w[:, 0]) / np.maximum(w[:, 2], 1.0)
    return {"vox": q, "ids": voxel_id(q), "v": v, "gap": gap, "m": m, "kth": kth, "tie": tie}


_REF = {}


def reference(name, k=16):
    if (name, k) not in _REF: _REF[(name, k)] = restatement(cloud(name), k)
    return _REF[(name, k)]


# ---- the rules every result obeys ----
def check_length(q):
    """|q|^2 between 16383.13^2 and 16384.87^2 (a unit vector whose components are rounded: sqrt(3) / 2), or q is zero"""
    l2 = (q.astype(np.int64) ** 2).sum(1)
    assert np.all((l2 == 0) | ((l2 >= 16383.13 ** 2) & (l2 <= 16384.87 ** 2))), (l2.min(), l2.max())


def check_sign(pts, q, view_point=(0, 0, 0)):
    """the integer dot of the Q14 normal with (view_point - p) is >= -1/2 sum |view_point - p|_i, the rounding bound of a non-negative double dot"""
    e = np.array(view_point, np.int64) - np.asarray(pts, np.int64)
    dot = (q.astype(np.int64) * e).sum(1)
    assert np.all(2 * dot >= -np.abs(e).sum(1)), (2 * dot + np.abs(e).sum(1)).min()
    return dot


def check_same_in_a_voxel(pts, q):
    order = np.argsort(voxel_id(pts), kind="stable"); ids = voxel_id(pts)[order]; qq = q[order]
    same = ids[1:] == ids[:-1]
    assert np.array_equal(qq[1:][same], qq[:-1][same])


def check_against_restatement(pts, q, ref, degenerate=False):
    """every component of a compared point within 1 LSB of round(16384 v_eigh), up to the sign of the whole vector"""
    at = np.searchsorted(ref["ids"], voxel_id(pts))
    assert np.array_equal(ref["ids"][at], voxel_id(pts))
    use = ref["gap"][at] >= GAP
    print("points %d, compared %d, under the gap %d, tie at the k-th place %.0f %%" % (len(pts), use.sum(), (~use).sum(), 100 * ref["tie"][at].mean()))
    if not degenerate: assert (~use).sum() <= 0.01 * len(pts), ((~use).sum(), len(pts))
    want = np.round(16384 * ref["v"][at]).astype(np.int64)              # |component| <= 16384: no half-way case differs between the two rounding rules by more than the margin
    s = np.sign((q.astype(np.int64) * want).sum(1))[:, None]
    err = np.abs(q.astype(np.int64) * s - want).max(1)
    print("largest difference to eigh in LSB:", err[use].max() if use.any() else None)
    assert np.all(err[use] <= 1), err[use].max()


def estimate(ctx, pts, params=None):
    """the handle route -> normals"""
    h = ctx.pcloud_upload(pts)
    try:
        return h.estimate_normals(params)[0]
    finally:
        h.release()


def params_of(R, **kw):
    return R.NormalsParams(**kw)


# ---- the cases, each a function of a context (and of a second one to compare with, bit for bit) ----
def check_cloud(R, ctx, name, other=None):
    pts = cloud(name); ref = reference(name)
    q = estimate(ctx, pts)
    check_length(q); check_sign(pts, q); check_same_in_a_voxel(pts, q)
    n_vox = len(ref["ids"])
    if n_vox == 1:
        assert not q.any()                                              # m <= 1: the zero vector
    elif n_vox <= 3 and not np.cross(ref["vox"][1] - ref["vox"][0], ref["vox"][-1] - ref["vox"][0]).any():
        # two voxels, or three on a line (the first three of the slab are): S = a multiple of the outer product of their direction e, of rank 1; the gap is 0 and any
        # vector across e is an eigenvector of 0. What the definition fixes is q . e = 0 before rounding, so |q . e| <= 1/2 sum |e_i| after it (+ 1 for the
        # double-precision error of the vector itself, 1e-12 of that)
        e = ref["vox"][-1] - ref["vox"][0]
        assert np.all(2 * np.abs((q.astype(np.int64) * e).sum(1)) <= np.abs(e).sum() + 1)
    else:
        check_against_restatement(pts, q, ref, degenerate=n_vox < 4)
    if name == "plane":
        assert np.array_equal(np.abs(q), np.tile([0, 0, 16384], (len(pts), 1)))       # all neighbours in z = 333: the z row of S is exactly zero
    if name in ("sphere", "slab", "plane"): assert ref["tie"].mean() > 0.5            # the tie rule is exercised everywhere
    if name == "slab_outliers": assert ref["kth"].max() > 600 * 600                   # the coarse-shell walk: the outliers' neighbours are hundreds of voxels away
    if other is not None: assert np.array_equal(q, estimate(other, pts))
    return q


def check_isotropic_cube(R, ctx, other=None):
    """a full 3 x 3 x 3 cube with k = 27: S is isotropic for every point, the expected normal exactly (0, 0, 16384) before orientation"""
    p = params_of(R, k=27, orientation=NONE)
    q = estimate(ctx, cube(), p)
    assert np.array_equal(q, np.tile([0, 0, 16384], (27, 1))), q
    q = estimate(ctx, cube(), params_of(R, k=27))                       # seen from the origin the same vector points away: it is flipped
    assert np.array_equal(q, np.tile([0, 0, -16384], (27, 1))), q
    if other is not None: assert np.array_equal(estimate(other, cube(), p), np.tile([0, 0, 16384], (27, 1)))


def check_view_point_inside(R, ctx, other=None):
    """a view point at the centre of the sphere: every normal points inwards; without orientation the same vectors up to sign"""
    pts = cloud("sphere"); vp = (200, 200, 200)
    q = estimate(ctx, pts, params_of(R, view_point=vp))
    dot = check_sign(pts, q, vp)
    assert np.all(dot > 0)                                              # a shell of radius 30: the fitted plane is nowhere near containing the centre
    check_length(q); check_against_restatement(pts, q, reference("sphere"))
    raw = estimate(ctx, pts, params_of(R, orientation=NONE))
    out = estimate(ctx, pts)                                            # seen from the origin, outside: the near side points outwards, the far side inwards
    for x in (raw, out): assert np.all((x == q).all(1) | (x == -q).all(1))
    assert 0.3 < (out == -q).all(1).mean() < 0.7
    if other is not None: assert np.array_equal(q, estimate(other, pts, params_of(R, view_point=vp)))


def check_other_k(R, ctx, other=None):
    """k = 3, 10, 17 and 32 on the slab with outliers: both instantiations of the search below and at their sizes"""
    pts = cloud("slab_outliers")
    for k in (3, 10, 17, 32):
        q = estimate(ctx, pts, params_of(R, k=k))
        check_length(q); check_sign(pts, q)
        check_against_restatement(pts, q, reference("slab_outliers", k), degenerate=k == 3)     # three neighbours span a plane at most: l0 = 0, and collinear triples have no gap
        if other is not None: assert np.array_equal(q, estimate(other, pts, params_of(R, k=k)))


def check_order_and_duplicates(R, ctx):
    """shuffling the points permutes the normals and changes no value; all points of a voxel carry the same triple"""
    for name in ("slab_outliers", "sphere"):
        pts = cloud(name); q = estimate(ctx, pts)
        perm = np.random.default_rng(5).permutation(len(pts))
        assert np.array_equal(estimate(ctx, pts[perm]), q[perm])
    pts = cloud("sphere_doubled"); q = estimate(ctx, pts)
    check_same_in_a_voxel(pts, q)
    one = cloud("sphere"); q1 = estimate(ctx, one)
    order = np.argsort(voxel_id(one))
    assert np.array_equal(q, q1[order][np.searchsorted(voxel_id(one)[order], voxel_id(pts))])


def score_with(ctx, hs, dec):
    hd = ctx.pcloud_upload(*dec)
    try:
        return ctx.score(hs, hd)
    finally:
        hd.release()


def check_scoring(R, ctx, other=None):
    """a cloud uploaded without normals refuses D2 as a source; after the estimation the same handle allows it, and scores bit for bit as a fresh upload of the same points
    with the returned normals; rbt_estimate_normals on host arrays returns the same triples"""
    a, ca, _, b, cb = SC.base(0)
    ha, hb = ctx.pcloud_upload(a, ca), ctx.pcloud_upload(b, cb)
    try:
        SC.refused(R, lambda: ctx.score(ha, hb, parts=D2))
        assert ctx.score(ha, hb)["parts"] == D1 | COLOR
        nrm, ms = ha.estimate_normals()
        assert nrm.shape == a.shape and nrm.any() and ms >= 0
        got = ctx.score(ha, hb)
        assert got["parts"] == D1 | D2 | COLOR and got["d2"]["sse_ab"] > 0 and ctx.score(ha, hb, parts=D2)["parts"] == D1 | D2
        quiet, _ = ha.estimate_normals(copy=False)                     # the normals stay on the device: nothing is copied unless asked for
        assert quiet is None and SC.same_result(got, ctx.score(ha, hb))
    finally:
        ha.release(); hb.release()
    assert SC.same_result(got, SC.score_case(ctx, (a, ca, nrm, b, cb)))
    assert np.array_equal(ctx.estimate_normals(a), nrm)
    if other is not None:
        assert np.array_equal(other.estimate_normals(a), nrm)
    return got


def check_scoring_from_maps(R, ctx, case, other=None):
    """the same for a handle from rbt_pcloud_from_maps (no normals) used as the source"""
    h, host = ctx.pcloud_from_maps(*case, host_copy=True)
    sx, srgb, _ = SC.seam_source(R, ctx, case, 3)
    hd = ctx.pcloud_upload(sx, srgb)
    try:
        SC.refused(R, lambda: ctx.score(h, hd, parts=D2))
        nrm, _ = h.estimate_normals()
        got = ctx.score(h, hd)
        assert got["parts"] == D1 | D2 | COLOR
    finally:
        h.release(); hd.release()
    check_length(nrm); check_sign(host[0], nrm); check_same_in_a_voxel(host[0], nrm)
    assert SC.same_result(got, SC.score_case(ctx, (host[0], host[4], nrm, sx, srgb)))
    assert np.array_equal(ctx.estimate_normals(host[0]), nrm)
    if other is not None: assert np.array_equal(other.estimate_normals(host[0]), nrm)


def unsupported(R, f):
    try:
        f()
    except R.RbtError as e:
        assert e.code == -3, str(e)                                     # RBT_ERR_UNSUPPORTED
        return
    raise AssertionError("accepted")


def check_arguments(R, ctx, make_ctx):
    """every refusal of include/rbt.h; after each the context still works, and the normals the cloud held before are still there: the score is unchanged"""
    a, ca, na, b, cb = SC.base(1)
    SC.check_still_works(ctx)
    ha, hb = ctx.pcloud_upload(a, ca, na), ctx.pcloud_upload(b, cb)
    other_ctx = make_ctx()
    try:
        before = ctx.score(ha, hb)
        foreign = other_ctx.pcloud_upload(b, cb)
        short = params_of(R); short.struct_size -= 4
        long_ = params_of(R); long_.struct_size += 4
        zero = params_of(R); zero.struct_size = 0
        bad = [lambda k=k: ha.estimate_normals(params_of(R, k=k)) for k in (-1, 1, 2, 33, 1 << 20)] + \
              [lambda o=o: ha.estimate_normals(params_of(R, orientation=o)) for o in (-1, 4, 100)] + \
              [lambda p=p: ha.estimate_normals(p) for p in (short, long_, zero)] + \
              [lambda: R.PCloud(ctx, foreign.h).estimate_normals(), lambda: R.PCloud(ctx, None).estimate_normals(copy=False),
               lambda: ctx.estimate_normals(a, params_of(R, k=2)), lambda: ctx.estimate_normals(a, short),
               lambda: ctx.estimate_normals(np.zeros((0, 3), np.int16)), lambda: ctx.estimate_normals(np.array([[5, 5, 5], [0, -1, 0]], np.int16)),
               lambda: ctx.estimate_normals(np.array([[5, 5, 5], [0, 0, 1024]], np.int16))]
        for f in bad:
            SC.refused(R, f)
            SC.check_still_works(ctx)
            assert SC.same_result(before, ctx.score(ha, hb))
        for o in (SPANNING_TREE, CUBEMAP):
            unsupported(R, lambda: ha.estimate_normals(params_of(R, orientation=o)))
            unsupported(R, lambda: ctx.estimate_normals(a, params_of(R, orientation=o)))
            SC.check_still_works(ctx)
            assert SC.same_result(before, ctx.score(ha, hb))
        # an accepted call replaces the normals the cloud was uploaded with
        nrm, _ = ha.estimate_normals(params_of(R, k=3, orientation=NONE))
        after = ctx.score(ha, hb)
        assert not SC.same_result(before, after) and SC.same_result(after, SC.score_case(ctx, (a, ca, nrm, b, cb)))
    finally:
        other_ctx.close()
        ha.release(); hb.release()
