"""PSNR floors held patch by patch (include/rbt.h: rbt_ctb_sse, rbt_submit_gof_quality_patches / rbt_wait_gof_quality_patches / rbt_transcode_gof_quality_patches): one set of
cases for the host emulation (tests/test_patch_floor.py) and the GPU (tests/test_gpu_patch_floor.py).
  sums      rbt_ctb_sse against a NumPy restatement of the definition, exact equality of every word; the words of a picture add up to rbt_picture_sse's luma words
  report    floor 0: the map is uniform, so the output decodes to the oracle's C(q0) (rule 8 of the QP map); every patch's sums against NumPy sums over R_k
  replay    a Python restatement of the walk that drives transcode_gof_qp_map, O.decode and the NumPy sums trial by trial; the library's result must be the replay's, and
            the returned stream transcode_gof_qp_map's for the final map, byte for byte
  edges     floors nothing reaches, a range of one QP, max_trials, a frame without patches, a patch outside the atlas, background_qp 51 behind occupancy_rd
  refusals  every RBT_ERR_PARAM of rule 9; the wrong wait call; jobs at depth 4 and 16; two GOFs in shared pipelines
The GOFs are frame_qp_cases' (64x64 with 3 frames, 128x128 with 4) and qp_map_cases' atlas of 96x80. Everything the oracle computes is cached, so the host and the GPU
tests of one run share it."""
import functools
import math
import numpy as np
import pytest
import oracle_lib as O
import synth
import frame_qp_cases as FC
import quality_cases as QC
import qp_map_cases as MC
from frame_qp_cases import variant, source, occupancy, constant, constant_decoded, params, occ_params, pooled_map, QP

ALL, OCCUPIED = 0, 1


# ------------------------------------------------------------------------------------------------ 1. sums
def np_ctb(a, b, w, h, log2_ctb, occ=None):
    """uint64 [n, h_ctb, w_ctb, 3]: per picture and CTB the luma sse, sse_occ, n_occ by the definition"""
    ctb = 1 << log2_ctb; hc, wc = -(-h // ctb), -(-w // ctb)
    a = np.asarray(a).reshape(-1, w * h * 3 // 2)[:, :w * h].reshape(-1, h, w).astype(np.int64)
    b = np.asarray(b).reshape(-1, w * h * 3 // 2)[:, :w * h].reshape(-1, h, w).astype(np.int64)
    d2 = (a - b) ** 2
    out = np.zeros((a.shape[0], hc, wc, 3), np.uint64)
    for k in range(a.shape[0]):
        m = None
        if occ is not None:
            s = w // occ[k].shape[1]
            m = np.repeat(np.repeat(occ[k] > 0, s, 0), s, 1)
        for r in range(hc):
            for c in range(wc):
                e = d2[k, r * ctb:(r + 1) * ctb, c * ctb:(c + 1) * ctb]
                out[k, r, c, 0] = int(e.sum())
                if m is not None:
                    mm = m[r * ctb:(r + 1) * ctb, c * ctb:(c + 1) * ctb]
                    out[k, r, c, 1] = int(e[mm].sum()); out[k, r, c, 2] = int(mm.sum())
    return out


def np_fold(words, rects):
    """uint64 [n / 2, len(rects) + 2, 3]: per pair of pictures the words summed over each rectangle (c0, r0, c1, r1, half-open), over the CTBs no rectangle meets, over all"""
    n, hc, wc, _ = words.shape
    pair = words.reshape(n // 2, 2, hc, wc, 3).sum(axis=1)
    out = np.zeros((n // 2, len(rects) + 2, 3), np.uint64)
    hit = np.zeros((hc, wc), bool)
    for k, (c0, r0, c1, r1) in enumerate(rects):
        out[:, k] = pair[:, r0:r1, c0:c1].sum(axis=(1, 2)); hit[r0:r1, c0:c1] = True
    out[:, len(rects)] = pair[:, ~hit].sum(axis=1)
    out[:, len(rects) + 1] = pair.sum(axis=(1, 2))
    return out


def _one_sample(last):
    w, h = 130, 66
    a, _ = QC._pictures(w, h, 2, 77)
    b = a.copy()
    at = w * h - 1 if last else 0
    b[:, at] = a[:, at] ^ 5
    return a, b, w, h, QC._map("set", w, h, 2, 2)


def _extremes(bd):
    w, h = 264, 136
    a = np.zeros((2, w * h * 3 // 2), np.uint16); b = np.full_like(a, (1 << bd) - 1)
    return a, b, w, h, QC._map("set", w, h, 4, 2)


def _with_map(kind, s):
    a, b = QC._pictures(96, 80, 2, 5 + s)
    return a, b, 96, 80, QC._map(kind, 96, 80, s, 2, seed=s)


def _sized(w, h, n, s):
    a, b = QC._pictures(w, h, n, w * 7 + h)
    return a, b, w, h, (QC._map("random", w, h, s, n, seed=w + h + n) if s else None)


# name -> (pictures a, b, width, height, maps), and the CTB sizes the case runs at
SUM_CASES = {
    "96x80": (lambda: _sized(96, 80, 2, 4), (4, 5, 6)),          # partial CTBs on both edges at 64, half a row at 32
    "96x80_no_map": (lambda: _sized(96, 80, 2, 0), (5,)),
    "130x66": (lambda: _sized(130, 66, 2, 2), (4, 5, 6)),        # rows whose pointers are not 16-byte aligned
    "264x136_4_frames": (lambda: _sized(264, 136, 4, 4), (5, 6)),
    "extremes_10_bits": (lambda: _extremes(10), (6,)),           # the largest sums at 10 bits: a CTB of 64x64 is 8.4 million short of 2^32, two of them are beyond it
    "extremes_16_bits": (lambda: _extremes(16), (6, 4)),          # one CTB of 16x16 is beyond 2^32
    "first_sample": (lambda: _one_sample(False), (4, 6)),
    "last_sample": (lambda: _one_sample(True), (4, 6)),
}
for _s in (1, 2, 4):
    for _k in ("zero", "set", "checker", "last", "random"):
        SUM_CASES["map_%s_scale_%d" % (_k, _s)] = (functools.partial(_with_map, _k, _s), (5,))


def rect_lists(wc, hc):
    """none, one CTB, the whole grid, overlapping ones with an empty one among them"""
    return [[], [(wc - 1, hc - 1, wc, hc)], [(0, 0, wc, hc)], [(0, 0, max(1, wc - 1), max(1, hc - 1)), (wc // 2, 0, wc, hc), (1, 1, 1, 1), (0, hc - 1, 1, hc)]]


@functools.lru_cache(maxsize=None)
def sum_case(name):
    make, l2s = SUM_CASES[name]
    a, b, w, h, occ = make()
    return (a, b, w, h, occ), {l2: np_ctb(a, b, w, h, l2, occ) for l2 in l2s}


def check_sums(ctx, name, other=None):
    (a, b, w, h, occ), want = sum_case(name)
    for l2, words in want.items():
        hc, wc = words.shape[1:3]
        got = ctx.ctb_sse(a, b, w, h, l2, occ)
        assert got.dtype == np.uint64 and np.array_equal(got, words), (name, l2)
        # the CTB words of a picture add up to rbt_picture_sse's luma words
        assert np.array_equal(got.sum(axis=(1, 2)), ctx.picture_sse(a, b, w, h, occ)[:, 0, :]), (name, l2)
        for rects in rect_lists(wc, hc):
            g2, folded = ctx.ctb_sse(a, b, w, h, l2, occ, rects)
            assert np.array_equal(g2, words) and np.array_equal(folded, np_fold(words, rects)), (name, l2, rects)
            if other is not None:
                o2, of = other.ctb_sse(a, b, w, h, l2, occ, rects)
                assert np.array_equal(o2, g2) and np.array_equal(of, folded)
    if name.startswith("extremes"):
        peak = 1023 if name.endswith("10_bits") else 65535
        g = ctx.ctb_sse(a, b, w, h, 6, occ)
        assert int(g[0, 0, 0, 0]) == 4096 * peak * peak and int(g[0, 0, 0, 2]) == 4096 and (peak == 1023 or int(g[0, 0, 0, 0]) > 1 << 32)
        assert int(g[0].sum(axis=(0, 1))[0]) == 264 * 136 * peak * peak
    if name in ("first_sample", "last_sample"):
        g = ctx.ctb_sse(a, b, w, h, 4, occ)
        nz = np.argwhere(g[0, :, :, 0] > 0).tolist()
        assert nz == ([[g.shape[1] - 1, g.shape[2] - 1]] if name == "last_sample" else [[0, 0]])
    if name.startswith("map_zero"):
        assert not ctx.ctb_sse(a, b, w, h, 5, occ)[..., 1:].any()
    if name.startswith("map_last"):
        s = int(name[-1]); g = ctx.ctb_sse(a, b, w, h, 5, occ)
        assert int(g[..., 2].sum()) == 2 * s * s and int(g[0, -1, -1, 2]) == s * s


def check_sums_arguments(R, ctx):
    a, b = QC._pictures(96, 80, 2, 1)

    def refused(word, *args):
        with pytest.raises(R.RbtError) as e:
            ctx.ctb_sse(*args)
        assert e.value.code == -4 and word in str(e.value), str(e.value)
    refused("log2_ctb", a, b, 96, 80, 3)
    refused("log2_ctb", a, b, 96, 80, 7)
    refused("scale", a, b, 96, 80, 5, np.ones((2, 20, 50), np.uint16))
    for r in ((0, 0, 4, 1), (0, 0, 1, 4), (-1, 0, 1, 1), (2, 0, 1, 1), (0, -1, 1, 1)):       # the grid is 3 x 3
        refused("rectangle", a, b, 96, 80, 5, None, [r])
    refused("even", a[:1], b[:1], 96, 80, 5, None, [])                                         # sums per rectangle are taken over pairs
    odd = np.zeros((2, 9 * 8 * 3 // 2), np.uint16)
    refused("even", odd, odd, 9, 8, 4)
    assert np.array_equal(ctx.ctb_sse(a[:1], b[:1], 96, 80, 5), np_ctb(a[:1], b[:1], 96, 80, 5))   # an odd count is fine without rectangles


# ------------------------------------------------------------------------------------------------ the definition, restated
def frame_patches(R, gof, f):
    w, h, n_pc, seed = FC.GOFS[gof]
    return synth.atlas_patches(R, w, h, seed + f % min(4, n_pc))


def region(p, w, h, res, log2_ctb):
    """R_k in CTB units (c0, r0, c1, r1), half-open: the CTBs the patch's rectangle meets, clipped to the atlas; None for a patch without one"""
    x0, y0 = max(0, p.u0 * res), max(0, p.v0 * res)
    x1, y1 = min(w, (p.u0 + p.size_u0) * res), min(h, (p.v0 + p.size_v0) * res)
    if x0 >= x1 or y0 >= y1:
        return None
    return (x0 >> log2_ctb, y0 >> log2_ctb, ((x1 - 1) >> log2_ctb) + 1, ((y1 - 1) >> log2_ctb) + 1)


def np_patch_sums(a, b, occ, w, h, log2_ctb, rect):
    """(sse, samples, sse_occ, n_occ) of the luma of pictures a, b ([2, h, w] each, int64) over the displayed samples of the CTBs of rect"""
    if rect is None:
        return (0, 0, 0, 0)
    c0, r0, c1, r1 = rect
    ys, xs = slice(r0 << log2_ctb, min(h, r1 << log2_ctb)), slice(c0 << log2_ctb, min(w, c1 << log2_ctb))
    d2 = (a[:, ys, xs] - b[:, ys, xs]) ** 2
    m = np.broadcast_to(occ[ys, xs], d2.shape) if occ is not None else np.zeros(d2.shape, bool)
    return (int(d2.sum()), int(d2.size), int(d2[m].sum()), int(m.sum()))


def luma(pics, w, h):
    return np.asarray(pics)[:, :w * h].reshape(-1, h, w).astype(np.int64)


def occ_mask(gof, f):
    w, h, _, _ = FC.GOFS[gof]
    m = pooled_map(gof)[f] > 0
    return np.repeat(np.repeat(m, w // m.shape[1], 0), h // m.shape[0], 1)


def figures(sums, reg, floors):
    """per patch (sse, samples, figure, meets) in the chosen region"""
    out = []
    for (sse, n, sse_o, n_o), F in zip(sums, floors):
        s, k = (sse_o, n_o) if reg == OCCUPIED else (sse, n)
        out.append((s, k, QC.psnr(s, k), QC.meets(s, k, F)))
    return out


def run_map(R, ctx, gof, kind, M, v):
    return MC.run(R, ctx, gof, kind, M, v)


def replay(R, ctx, gof, kind, v, floor_mdb=0, reg=ALL, qp_min=0, qp_max=0, background_qp=-1, max_trials=0, patch_floors=None, patches=None):
    """the walk of include/rbt.h rule 5, frame by frame and trial by trial: every trial is a transcode_gof_qp_map of the whole stream with the frame's trial map (the other
    frames at q0: frames are closed pairs), decoded by the oracle and summed by NumPy. -> per frame a dict, and the final map"""
    w, h, n_pc, _ = FC.GOFS[gof]; l2 = dict(v)["log2_ctb"]; ctb = 1 << l2; hc, wc = -(-h // ctb), -(-w // ctb)
    inp = luma(O.decode(source(gof, kind))[0], w, h)
    any_floor = floor_mdb != 0 or any(x for fl in (patch_floors or []) if fl is not None for x in fl)
    qp = min(51, max(0, QP))
    lo, hi = (qp_min, qp_max or 51) if any_floor else (qp, qp)
    q0 = min(hi, max(lo, qp))
    bg = q0 if background_qp < 0 else background_qp
    frames, final = [], np.full((n_pc, hc, wc), q0, np.int8)
    for f in range(n_pc):
        pats = patches[f] if patches is not None else frame_patches(R, gof, f)
        floors = list(patch_floors[f]) if patch_floors is not None and patch_floors[f] is not None else [floor_mdb] * len(pats)
        rects = [region(p, w, h, 16, l2) for p in pats]
        occ = occ_mask(gof, f) if reg == OCCUPIED else None
        q, failed, trials = [q0] * len(pats), [0] * len(pats), 0
        while True:
            m = R.qp_map_from_patches(MC.atlas(R, w, h), pats, q, bg, l2, lib=MC._lib(R))
            M = final.copy(); M[f] = m
            dec = luma(O.decode(run_map(R, ctx, gof, kind, M, v))[0], w, h)
            sums = [np_patch_sums(inp[2 * f:2 * f + 2], dec[2 * f:2 * f + 2], occ, w, h, l2, r) for r in rects]
            fg = figures(sums, reg, floors)
            trials += 1
            for k, (_, _, _, ok) in enumerate(fg):
                failed[k] |= int(not ok)
            if max_trials and trials >= max_trials:
                break
            new = list(q)
            for k, (_, _, fig, ok) in enumerate(fg):
                F = floors[k] / 1000.0
                if not ok:
                    if q[k] > lo:
                        new[k] = max(lo, q[k] - max(1, int(F - fig)))
                elif not failed[k] and q[k] < hi and math.isfinite(fig) and int(fig - F) >= 1:
                    new[k] = min(hi, q[k] + int(fig - F))
            if new == q:
                break
            q = new
        final[f] = m
        frames.append(dict(n_trials=trials, q=q, failed=failed, fig=fg, met=int(all(x[3] for x in fg))))
    return frames, final, q0


def target(R, gof, v, **kw):
    w, h, n_pc, _ = FC.GOFS[gof]
    pats = kw.pop("patches", None) or [frame_patches(R, gof, f) for f in range(n_pc)]
    return R.PatchFloorTarget(MC.atlas(R, w, h), pats, **kw)


def run(R, ctx, gof, kind, v, **kw):
    """the entry through rbt_transcode_gof_quality_patches; with occupancy_rd, or for the occupied region, behind its pooled occupancy entry -> (stream, result)"""
    t = target(R, gof, v, **kw)
    if dict(v)["occupancy_rd"] or kw.get("region") == OCCUPIED:
        outs, res = ctx.transcode_gof_quality_patches([occupancy(gof), source(gof, kind)], [occ_params(R), params(R, kind, v)], [R.PatchFloorTarget(), t])
        return outs[1], res[1]
    outs, res = ctx.transcode_gof_quality_patches([source(gof, kind)], [params(R, kind, v)], [t])
    return outs[0], res[0]


def check_against_replay(R, ctx, gof, kind, v, other=None, **kw):
    """the library's result is the replay's; the stream is transcode_gof_qp_map's for the final map"""
    out, res = run(R, ctx, gof, kind, v, **kw)
    rk = dict(kw); rk["reg"] = rk.pop("region", ALL); rk["floor_mdb"] = rk.pop("min_psnr_mdb", 0)
    frames, final, q0 = replay(R, ctx, gof, kind, v, **rk)
    n_pc = FC.GOFS[gof][2]
    assert res["n_frames"] == n_pc == len(res["frames"]) and res["qp_probe"] == q0
    assert np.array_equal(res["map"], final), (res["map"], final)
    for f, (want, got) in enumerate(zip(frames, res["frames"])):
        assert got["n_trials"] == want["n_trials"] and got["met"] == want["met"] and got["n_patches"] == len(want["q"]), (f, got, want)
        for k, p in enumerate(got["patches"]):
            s, n, fig, ok = want["fig"][k]
            assert (p["qp"], p["failed"], p["met"], p["sse"], p["samples"]) == (want["q"][k], want["failed"][k], int(ok), s, n), (f, k, p, want)
            assert p["figure"] == fig or abs(p["figure"] - fig) < 1e-9
    assert res["n_passes"] == max(x["n_trials"] for x in frames) and res["pictures_encoded"] == 2 * sum(x["n_trials"] for x in frames)
    assert res["met_all"] == int(all(x["met"] for x in frames)) and res["bytes"] == len(out)
    assert out == run_map(R, ctx, gof, kind, final, v)
    assert [x["bytes"] for x in res["frames"]] == FC.frame_sizes(out)
    if dict(v)["md5_sei"]:
        got = O.decode(out)
        assert (got[4], got[5]) == (2 * n_pc, 0)                       # the oracle's decoder accepted every picture's MD5
    if other is not None:
        o_out, o_res = run(R, other, gof, kind, v, **kw)
        assert o_out == out and _plain(o_res) == _plain(res)
    return out, res, frames


def _plain(x):
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x.tolist() if hasattr(x, "tolist") else x


# ------------------------------------------------------------------------------------------------ 2. report
REPORT_CASES = [("128", "geo", variant(), ALL), ("64", "attr", variant(occupancy_rd=1), OCCUPIED), ("96", "geo", variant(log2_ctb=6), ALL)]


def check_report(R, ctx, k, other=None):
    """floor 0, background_qp -1: one trial with a uniform map, which decodes to the samples of the oracle's C(q0); every patch's sums are NumPy's over O.decode(C(q0))
    against O.decode(input) on R_k; sums are rbt_transcode_gof_quality's at floor 0"""
    gof, kind, v, reg = REPORT_CASES[k]
    w, h, n_pc, _ = FC.GOFS[gof]; l2 = dict(v)["log2_ctb"]
    out, res = run(R, ctx, gof, kind, v, region=reg)
    assert res["n_passes"] == 1 and res["pictures_encoded"] == 2 * n_pc and res["met_all"] == 1 and res["qp_probe"] == QP and (res["map"] == QP).all()
    inp, ref = luma(O.decode(source(gof, kind))[0], w, h), luma(constant_decoded(gof, kind, QP, v), w, h)
    assert np.array_equal(luma(O.decode(out)[0], w, h), ref)
    for f, fr in enumerate(res["frames"]):
        pats = frame_patches(R, gof, f)
        assert fr["n_trials"] == 1 and fr["met"] == 1 and fr["n_patches"] == len(pats) >= 1
        occ = occ_mask(gof, f) if reg == OCCUPIED else None
        for p, pick in zip(pats, fr["patches"]):
            sse, n, sse_o, n_o = np_patch_sums(inp[2 * f:2 * f + 2], ref[2 * f:2 * f + 2], occ, w, h, l2, region(p, w, h, 16, l2))
            s, cnt = (sse_o, n_o) if reg == OCCUPIED else (sse, n)
            assert (pick["qp"], pick["met"], pick["failed"], pick["sse"], pick["samples"]) == (QP, 1, 0, s, cnt), (f, pick)
            assert cnt > 0 and abs(pick["figure"] - QC.psnr(s, cnt)) < 1e-9
    QT = R.QualityTarget(0, reg)
    if dict(v)["occupancy_rd"] or reg == OCCUPIED:
        q_out, q_res = ctx.transcode_gof_quality([occupancy(gof), source(gof, kind)], [occ_params(R), params(R, kind, v)], [R.QualityTarget(), QT])
        q_out, q_res = q_out[1], q_res[1]
    else:
        q_out, q_res = ctx.transcode_gof_quality([source(gof, kind)], [params(R, kind, v)], [QT])
        q_out, q_res = q_out[0], q_res[0]
    for name in ("sse", "samples", "sse_occ", "samples_occ", "psnr", "psnr_occ"):
        assert res["sums"][name] == q_res[name], name
    assert res["sums"]["qp"] == -1 and O.decode(q_out)[0].shape == O.decode(out)[0].shape
    if other is not None:
        o_out, o_res = run(R, other, gof, kind, v, region=reg)
        assert o_out == out and _plain(o_res) == _plain(res)


# ------------------------------------------------------------------------------------------------ 3. walk replay
MAIN_FLOOR = 46500


@functools.lru_cache(maxsize=None)
def main_premise():
    """from the oracle's C(30) alone: the PSNR of every patch of the four frames of ("128", geo) at log2_ctb 5, all samples"""
    import rbt_lib
    R = rbt_lib.module()
    w, h, n_pc, _ = FC.GOFS["128"]; v = variant()
    inp, ref = luma(O.decode(source("128", "geo"))[0], w, h), luma(constant_decoded("128", "geo", QP, v), w, h)
    out = []
    for f in range(n_pc):
        sums = [np_patch_sums(inp[2 * f:2 * f + 2], ref[2 * f:2 * f + 2], None, w, h, 5, region(p, w, h, 16, 5)) for p in frame_patches(R, "128", f)]
        out.append([QC.psnr(s[0], s[1]) for s in sums])
    return out


def check_main_premise():
    """every frame has a patch below 46.5 dB and one at least 1.5 dB above it, so the walk has to move patches both ways"""
    want = [[44.11, 52.56, 45.93], [44.53, 48.04, 48.16], [44.57, 44.80, 49.73], [53.77, 45.13, 44.59]]
    got = main_premise()
    assert [[round(x, 2) for x in fr] for fr in got] == want, got
    for fr in got:
        assert min(fr) < MAIN_FLOOR / 1000.0 and max(fr) >= MAIN_FLOOR / 1000.0 + 1.5


def check_main_walk(R, ctx, other=None):
    v = variant(md5_sei=1)
    out, res, frames = check_against_replay(R, ctx, "128", "geo", v, other=other, min_psnr_mdb=MAIN_FLOOR)
    assert res["met_all"] == 1
    for fr in res["frames"]:
        qs = [p["qp"] for p in fr["patches"]]
        assert min(qs) < QP < max(qs), qs


REPLAY_CASES = [
    ("128", "attr", variant(md5_sei=1), dict(min_psnr_mdb=42000)),                                    # the spread is under 1 dB: steps of one
    ("64", "geo", variant(occupancy_rd=1, md5_sei=1), dict(min_psnr_mdb=47000, region=OCCUPIED)),     # frame 1 has one patch
    ("128", "geo", variant(md5_sei=1), dict(min_psnr_mdb=45000, patch_floors="mixed")),               # per-patch floors that differ within a frame
    ("64", "attr", variant(md5_sei=1, rows_per_slice=1, log2_ctb=4), dict(min_psnr_mdb=41000)),       # one-row slices, CTBs of 16
    ("96", "geo", variant(md5_sei=1, log2_ctb=6, rows_per_slice=0), dict(min_psnr_mdb=46000, qp_min=24, qp_max=36)),
]


def _mixed_floors(R, gof):
    """49 / 43 / 46 dB in turn, None (the target's floor) for the last frame"""
    n_pc = FC.GOFS[gof][2]
    return [None if f == n_pc - 1 else [(49000, 43000, 46000)[(k + f) % 3] for k in range(len(frame_patches(R, gof, f)))] for f in range(n_pc)]


def check_replay(R, ctx, k, other=None):
    gof, kind, v, kw = REPLAY_CASES[k]
    kw = dict(kw)
    if kw.get("patch_floors") == "mixed":
        kw["patch_floors"] = _mixed_floors(R, gof)
    out, res, frames = check_against_replay(R, ctx, gof, kind, v, other=other, **kw)
    assert max(x["n_trials"] for x in frames) >= 2                      # the case walks


# ------------------------------------------------------------------------------------------------ 4. edges of the walk
def check_edges(R, ctx, other=None):
    v = variant()
    P = lambda u0, v0, su, sv: R.Patch(u0, v0, su, sv, 0, 0, 0, 0, 1, 2, 0, 0, 1, 1)
    # a floor nothing reaches: every patch ends at lo with met 0, the call returns RBT_OK, the stream is the map's
    out, res, frames = check_against_replay(R, ctx, "64", "geo", v, other=other, min_psnr_mdb=90000, qp_min=26, qp_max=34)
    assert res["met_all"] == 0 and all(p["qp"] == 26 and p["met"] == 0 and p["failed"] == 1 for fr in res["frames"] for p in fr["patches"])
    # lo = hi = q0: one trial
    out, res, frames = check_against_replay(R, ctx, "64", "geo", v, min_psnr_mdb=46000, qp_min=QP, qp_max=QP)
    assert res["n_passes"] == 1 and all(fr["n_trials"] == 1 for fr in res["frames"])
    # max_trials 1 and 2: the result is the last trial's, met as measured
    for cap in (1, 2):
        out, res, frames = check_against_replay(R, ctx, "128", "geo", v, other=other if cap == 2 else None, min_psnr_mdb=MAIN_FLOOR, max_trials=cap)
        assert res["n_passes"] == cap and all(fr["n_trials"] <= cap for fr in res["frames"])
        if cap == 1:
            assert res["met_all"] == 0 and (res["map"] == QP).all()
    # a frame without patches (one trial, background only), a patch wholly outside the atlas (it meets, without a sample), one that reaches beyond it (clipped)
    pats = [frame_patches(R, "64", 0), [], [P(9, 9, 2, 2), P(3, 2, 4, 1)]]
    out, res, frames = check_against_replay(R, ctx, "64", "geo", v, other=other, min_psnr_mdb=46000, patches=pats, background_qp=40)
    assert res["frames"][1]["n_trials"] == 1 and res["frames"][1]["n_patches"] == 0 and res["frames"][1]["met"] == 1 and (res["map"][1] == 40).all()
    assert res["frames"][1]["background"][0] > 0
    outside = res["frames"][2]["patches"][0]
    assert (outside["samples"], outside["sse"], outside["met"], outside["figure"]) == (0, 0, 1, 0.0)
    assert res["frames"][2]["patches"][1]["samples"] == 2 * 32 * 32          # columns 48..63 of rows 32..47 meet one CTB of 32
    # background_qp 51 behind occupancy_rd
    out, res, frames = check_against_replay(R, ctx, "128", "attr", variant(occupancy_rd=1, md5_sei=1), other=other, min_psnr_mdb=41000, background_qp=51)
    assert (res["map"] == 51).any()


# ------------------------------------------------------------------------------------------------ 5. refusals and jobs
def check_arguments(R, ctx):
    """rule 9: every refusal is RBT_ERR_PARAM with its reason, submits nothing and leaves the context usable"""
    geo, occ = source("64", "geo"), occupancy("64")
    v = variant()
    P = [params(R, "geo")]

    def refused(word, streams, ps, ts):
        with pytest.raises(R.RbtError) as e:
            ctx.transcode_gof_quality_patches(streams, ps, ts)
        assert e.value.code == -4 and word in str(e.value), str(e.value)

    def tgt(**kw):
        return target(R, "64", v, **kw)
    bad = tgt(); bad.struct_size += 8
    refused("struct_size", [geo], P, [bad])
    odd = O.encode_hm(synth.make_gof_maps(64, 64, 3, 5)[0][:5], 64, 64, 10, 16)[0]      # a stream with an odd picture count
    refused("n_frames", [odd], P, [tgt()])
    refused("n_frames", [geo], P, [tgt(patches=[frame_patches(R, "64", 0)] * 2)])       # not pictures / 2
    refused("n_frames", [geo], P, [tgt(patches=[frame_patches(R, "64", 0)] * 4)])
    t = tgt(); t.atlas.width = 128
    refused("atlas", [geo], P, [t])
    t = tgt(); t.atlas.height = 48
    refused("atlas", [geo], P, [t])
    t = tgt(); t.atlas.occupancy_resolution = 0
    refused("occupancy_resolution", [geo], P, [t])
    for bq in (-2, 52):
        refused("background_qp", [geo], P, [tgt(background_qp=bq)])
    refused("max_trials", [geo], P, [tgt(max_trials=-1)])
    refused("negative", [geo], P, [tgt(min_psnr_mdb=-1)])
    refused("negative", [geo], P, [tgt(patch_floors=[None, [-5] * len(frame_patches(R, "64", 1)), None])])
    refused("QP range", [geo], P, [tgt(qp_min=40, qp_max=30)])
    refused("region", [geo], P, [tgt(region=2)])
    refused("occupancy", [occ, geo], [occ_params(R), params(R, "geo")], [target(R, "64", v, patches=[[]] * 3), tgt()])   # a target on an occupancy entry
    refused("occupancy source", [geo], P, [tgt(region=OCCUPIED)])                      # the PSNR floor's own refusal
    t = tgt(); t.n_patches = None
    refused("patch list", [geo], P, [t])
    # the wrong count is found once the pictures are known, behind the other entries' decoders: the job is refused whole
    refused("entry 2", [occ, geo, source("64", "attr")], [occ_params(R), params(R, "geo"), params(R, "attr")], [R.PatchFloorTarget(), tgt(), tgt(patches=[[]] * 2)])
    # a refused call took no job slot: depth 1 still takes a job; collecting with the wrong wait call leaves the job collectable
    old = ctx.get_depth(); ctx.set_depth(1)
    try:
        job = ctx.submit_gof_quality_patches([geo], P, [tgt(min_psnr_mdb=46000)])
        for wrong in (ctx.wait_gof, ctx.wait_gof_quality, ctx.wait_gof_quality_frames):
            with pytest.raises(R.RbtError) as e:
                wrong(job)
            assert e.value.code == -4 and "collect" in str(e.value)      # (of the two kinds the one that comes first in the library's order is named)
        outs, res = ctx.wait_gof_quality_patches(job)
        other_job = ctx.submit_gof([geo], P)
        with pytest.raises(R.RbtError) as e:
            ctx.wait_gof_quality_patches(other_job)
        assert e.value.code == -4
        assert ctx.wait_gof(other_job)[0] == constant("64", "geo", QP)
    finally:
        ctx.set_depth(old)
    assert outs[0] == run(R, ctx, "64", "geo", v, min_psnr_mdb=46000)[0]
    # an entry without a target beside one with: coded at its own QP, n_frames 0, sums filled
    outs, res = ctx.transcode_gof_quality_patches([geo, source("64", "attr")], [params(R, "geo"), params(R, "attr")], [R.PatchFloorTarget(), target(R, "64", v, min_psnr_mdb=41000)])
    assert outs[0] == constant("64", "geo", QP) and res[0]["n_frames"] == 0 and res[0]["map"] is None and res[0]["frames"] == [] and res[0]["sums"]["samples"][0] == 6 * 64 * 64
    assert outs[1] == run(R, ctx, "64", "attr", v, min_psnr_mdb=41000)[0]
    # a corrupt input fails in the wait half, and the context goes on
    with pytest.raises(R.RbtError):
        ctx.transcode_gof_quality_patches([geo[:len(geo) // 2]], P, [tgt()])
    assert ctx.transcode_gof([geo], P)[0] == constant("64", "geo", QP)


def check_jobs_in_flight(R, ctx, depth, n_jobs):
    """n_jobs jobs in flight at the given depth, every one with a floor of its own, collected out of order"""
    old = ctx.get_depth()
    ctx.set_depth(depth)
    try:
        v = variant(); src = source("64", "geo")
        floors = [44000 + 500 * (k % 8) for k in range(n_jobs)]
        jobs = [ctx.submit_gof_quality_patches([src], [params(R, "geo", v)], [target(R, "64", v, min_psnr_mdb=floors[k], max_trials=3)]) for k in range(n_jobs)]
        with pytest.raises(R.RbtError) as e:
            ctx.submit_gof_quality_patches([src], [params(R, "geo", v)], [target(R, "64", v)])
        assert e.value.code == -7         # RBT_ERR_BUSY
        assert ctx.job_memory(jobs[0]) > 0
        got = {}
        for k in list(range(1, n_jobs, 2)) + list(range(0, n_jobs, 2))[::-1]:
            got[k] = ctx.wait_gof_quality_patches(jobs[k])
        alone = {}
        for k in range(n_jobs):
            f = floors[k]
            if f not in alone:
                alone[f] = ctx.transcode_gof_quality_patches([src], [params(R, "geo", v)], [target(R, "64", v, min_psnr_mdb=f, max_trials=3)])
            assert got[k][0] == alone[f][0] and _plain(got[k][1]) == _plain(alone[f][1]), k
        assert len({o[0][0] for o in got.values()}) >= 2
    finally:
        ctx.set_depth(old)


def check_two_gofs(R, ctx, other=None):
    """two GOFs in one job: six entries share three pipelines; three carry targets, one nothing. An entry in company gives what it gives alone"""
    v = variant(occupancy_rd=1, md5_sei=1)
    streams = [occupancy("64"), source("64", "geo"), source("64", "attr"), occupancy("128"), source("128", "geo"), source("128", "attr")]
    ps = [occ_params(R), params(R, "geo", v), params(R, "attr", v), occ_params(R), params(R, "geo", v), params(R, "attr", v)]
    E = R.PatchFloorTarget
    kws = {1: dict(min_psnr_mdb=47000, region=OCCUPIED), 4: dict(min_psnr_mdb=MAIN_FLOOR, max_trials=3), 5: dict(min_psnr_mdb=42000, background_qp=45)}
    ts = [E(), target(R, "64", v, **kws[1]), E(), E(), target(R, "128", v, **kws[4]), target(R, "128", v, **kws[5])]
    outs, res = ctx.transcode_gof_quality_patches(streams, ps, ts)
    want = ctx.transcode_gof(streams, ps)
    assert outs[0] == want[0] and outs[3] == want[3] and outs[2] == want[2] and res[2]["n_frames"] == 0 and res[0]["n_frames"] == 0
    for i, (gof, kind) in ((1, ("64", "geo")), (4, ("128", "geo")), (5, ("128", "attr"))):
        a_out, a_res = run(R, ctx, gof, kind, v, **kws[i])
        assert outs[i] == a_out and _plain(res[i]) == _plain(a_res), i
        got = O.decode(outs[i])
        assert (got[4], got[5]) == (2 * FC.GOFS[gof][2], 0)
    if other is not None:
        o_outs, o_res = other.transcode_gof_quality_patches(streams, ps, ts)
        assert o_outs == outs and _plain(o_res) == _plain(res)
