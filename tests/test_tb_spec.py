"""Single transform blocks held against the TEXT of H.265 (tests/tb_spec.py: 8.4.4.2.2-6, 8.6.2-8.6.4.2, 8.6.7 in exact integers) instead of against the oracle:
the decoder's own rc_tile_tb / rc_tile_tb_cpair, run as serial host code through rbt_selftest_tb (tests/hostemu), and the oracle's hevc_dequant / hevc_inv_transform /
hevc_inv_transform_skip / hevc_intra_pred_buf, called through ctypes, both over the whole list of tests/tb_cases.py. Every comparison is of exact integers.
The device build of the same is tests/test_gpu_tb_spec.py."""
import ctypes as C
import os
import re
import subprocess
import tempfile
import numpy as np
import pytest
import rbt_lib
import tb_cases as TC
import tb_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def host_out():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "hostemu")])
    c = rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)
    out = TC.run_hook(c)
    c.close()
    return out


# ---------------------------------------------------------------------------------------------------------------------- the list itself
def test_the_list_covers_what_it_says():
    cs = TC.build(); h = cs.hdr
    assert 2500 <= len(cs.ids) <= 3500
    luma = h[:, TC.H_KIND] == TC.LUMA; pair = h[:, TC.H_KIND] == TC.PAIR; intra = h[:, TC.H_INTRA] == 1
    for bd in (8, 10):
        at = h[:, TC.H_BD] == bd
        for log2 in (2, 3, 4, 5):
            assert set(h[at & luma & intra & (h[:, TC.H_LOG2] == log2), TC.H_MODE]) == set(range(35))
            assert {0, 5, 6, 51, 51 + 6 * (bd - 8)} <= set(h[at & luma & (h[:, TC.H_LOG2] == log2) & (h[:, TC.H_CBF0] == 1), TC.H_QP0])
        for log2 in (2, 3, 4):
            assert set(h[at & pair & intra & (h[:, TC.H_LOG2] == log2), TC.H_MODE]) == set(range(35))
            coded = {(int(a), int(b)) for a, b in h[at & pair & (h[:, TC.H_LOG2] == log2)][:, [TC.H_CBF0, TC.H_CBF1]]}
            assert {(1, 0), (0, 1), (1, 1), (0, 0)} <= coded
    assert {4, 5, 6} == set(h[:, TC.H_CTB]) and h[:, TC.H_TS].any() and h[:, TC.H_BYP].any()
    # availability: none, several runs (the find-last-set path), first available unit not unit 0 - after the positional mask
    runs = lambda u: int(np.count_nonzero(np.diff(np.concatenate(([0], u.astype(np.int8)))) == 1))
    n_runs = np.array([runs(cs.uav[i]) for i in range(len(cs.ids))])
    assert (n_runs[intra] == 0).sum() >= 14 and (n_runs[intra] >= 3).sum() >= 50 and ((cs.uav[:, 0] == 0) & (n_runs >= 1))[intra].sum() >= 50
    # the blocks the known defect needs: exact residuals beyond int16 exist in the list, and only at 32x32 10 bit
    over = [(int(h[i, TC.H_LOG2]), int(h[i, TC.H_BD])) for i, per in enumerate(TC.expected()) for _, res in per if res is not None and not h[i, TC.H_BYP] and np.abs(res).max() > 32767]
    assert len(over) >= 30 and set(over) == {(5, 10)}
    for i in np.flatnonzero(intra):                                          # nothing that cannot be available is marked available
        assert not (cs.uav[i, :len(TC.legal_units(*h[i, [TC.H_KIND, TC.H_LOG2, TC.H_CTB, TC.H_X0, TC.H_Y0]]))].astype(bool) & ~TC.legal_units(*h[i, [TC.H_KIND, TC.H_LOG2, TC.H_CTB, TC.H_X0, TC.H_Y0]])).any()


def test_the_reference_stands_alone():
    """tests/tb_spec.py imports neither the oracle's binding nor the product, and stores nothing in 16 bits"""
    src = open(os.path.join(HERE, "tb_spec.py")).read()
    code = src.split('"""', 2)[2]                                             # after the module's docstring
    assert set(re.findall(r"^\s*(?:import|from)\s+(\w+)", code, re.M)) == {"json", "os", "numpy"}
    assert not re.search(r"int16|int32|oracle_lib|rbt_lib|csrc", code)


# ---------------------------------------------------------------------------------------------------------------------- self-checks of the reference
@pytest.mark.parametrize("n", [4, 8, 16, 32])
def test_golden_matrices_are_the_scaled_dct(n):
    """The text's matrix is the orthonormal DCT-II basis times 64 sqrt(n), in integers (every entry within 2 of it; the first row is exactly 64). What follows from that and
    only that: row norms within n * (2 * 90.5 * 2 + 4) of 4096 n, and rows orthogonal within the same bound - tight enough to catch a swapped, negated or shifted row or entry
    of any size that matters (a single entry changed by d moves a norm by about 2 * |entry| * d)."""
    t = S.DCT[n]
    k, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    real = 64 * np.sqrt(n) * np.where(k == 0, np.sqrt(1 / n), np.sqrt(2 / n) * np.cos(np.pi * (2 * i + 1) * k / (2 * n)))
    assert np.abs(t - real).max() < 2 and (t[0] == 64).all() and np.abs(t).max() <= 90
    g = t @ t.T
    bound = n * (2 * 90.5 * 2 + 4)
    assert np.abs(g - 4096 * n * np.eye(n, dtype=np.int64)).max() <= bound
    assert (S.DCT[32][::32 // n, :n] == t).all()                              # 8.6.4.2: the smaller ones are rows 0, 32/n, ... and columns 0..n-1 of the 32-point matrix


def test_golden_dst_is_the_scaled_dst7():
    i, k = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    real = 128 * (2 / 3) * np.sin(np.pi * (2 * i + 1) * (k + 1) / 9)        # DST-VII basis times 128 (every entry within 1 of it), transMatrix[i][k]
    assert np.abs(S.DST - real).max() < 1
    assert np.abs(S.DST @ S.DST.T - 16384 * np.eye(4, dtype=np.int64)).max() <= 4 * (2 * 84.5 + 1)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("log2", [2, 3, 4, 5])
def test_dc_only_block_is_flat(log2, bd):
    """a single DC level: the residual is one value everywhere (the first basis function is constant), of the level's sign, and grows with qP"""
    n = 1 << log2; last = None
    for qp in (0, 6, 12, 30, 51):
        for level in (1, -1, 37, -900):
            lv = np.zeros((n, n), np.int64); lv[0, 0] = level
            r = S.residual(lv, 1, log2, qp, bd, 0, 0, 0)
            assert (r == r[0, 0]).all() and (r[0, 0] == 0 or np.sign(r[0, 0]) == np.sign(level))
        r37 = int(S.residual(np.pad([[37]], ((0, n - 1), (0, n - 1))), 1, log2, qp, bd, 0, 0, 0)[0, 0])
        assert last is None or r37 >= last
        last = r37
    assert last > 0


# ---------------------------------------------------------------------------------------------------------------------- the decoder's routine, as host code
@pytest.mark.parametrize("group", TC.groups())
def test_the_text_equals_the_decoders_routine(host_out, group):
    bad = TC.compare(host_out, group, "host emulation")
    assert not bad, "\n".join(bad[:20])


def test_arguments():
    """a case the hook could not stage inside the CTB tile is refused before anything runs"""
    R = rbt_lib.module(); cs = TC.build()
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "hostemu")])
    c = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
    try:
        pair = int(np.flatnonzero(cs.hdr[:, TC.H_KIND] == TC.PAIR)[0])
        for at, field, value in ((0, TC.H_KIND, 4), (0, TC.H_LOG2, 6), (pair, TC.H_LOG2, 5), (0, TC.H_BD, 7), (0, TC.H_CTB, 7), (0, TC.H_X0, 64), (0, TC.H_Y0, 2), (0, TC.H_MODE, 35),
                                 (0, TC.H_QP0, 64), (pair, TC.H_TS, 1)):
            h = cs.hdr[at:at + 1].copy(); h[0, field] = value
            with pytest.raises(R.RbtError) as e:
                c.selftest_tb(h, cs.nb[at:at + 1], cs.uav[at:at + 1], cs.lev[at:at + 1])
            assert e.value.code == -4                                        # RBT_ERR_PARAM
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------- the oracle's functions
class _Frame(C.Structure):
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("cw", C.c_int), ("ch", C.c_int), ("bit_depth", C.c_int), ("p", C.c_void_p * 3)]


class _SliceMeta(C.Structure):
    _fields_ = [("flags", C.c_uint8 * 4), ("offs", C.c_int8 * 2), ("slice_type", C.c_int8), ("ref_poc", C.c_int32 * 16)]


class _Meta(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("w", "h", "w4", "h4", "log2_ctb", "w_ctb", "h_ctb")] + \
               [(n, C.c_void_p) for n in ("pred_mode", "done", "intra_mode", "cu_depth", "qp", "tq_bypass", "nz", "edge_v", "edge_h", "mv", "ref_idx", "ctb_slice", "sao")] + \
               [("slices", _SliceMeta * 1024), ("n_slices", C.c_int), ("constrained_intra_pred", C.c_int), ("pcm_loop_filter_disabled", C.c_int), ("cb_qp_offset", C.c_int),
                ("cr_qp_offset", C.c_int), ("strong_intra_smoothing", C.c_int)]


PIC = 192                                                                      # 3 x 3 CTBs of 64: the case's CTB is the middle one, whatever its size


@pytest.fixture(scope="module")
def oracle():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(HERE), "oracle"), "liboracle.so"])
    L = C.CDLL(os.path.join(os.path.dirname(HERE), "oracle", "liboracle.so"))
    L.hevc_meta_alloc.restype = C.POINTER(_Meta); L.hevc_meta_alloc.argtypes = [C.c_int] * 3
    L.hevc_meta_free.argtypes = [C.POINTER(_Meta)]
    L.hevc_dequant.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.hevc_inv_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.hevc_inv_transform_skip.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.hevc_intra_pred_buf.argtypes = [C.POINTER(_Frame), C.POINTER(_Meta), C.c_int] * 1 + [C.c_int] * 4 + [C.c_void_p]
    m = L.hevc_meta_alloc(PIC, PIC, 6)
    assert (m.contents.w4, m.contents.h4, m.contents.w_ctb, m.contents.h_ctb, m.contents.n_slices, m.contents.strong_intra_smoothing) == (PIC // 4, PIC // 4, 3, 3, 0, 0)   # the layout above is the C one
    yield L, m
    L.hevc_meta_free(m)


def _oracle_block(L, m, cs, ci, b):
    """(pred or None, res or None) of plane b of case ci by the oracle's functions"""
    h = cs.hdr[ci]; kind, log2, bd = int(h[TC.H_KIND]), int(h[TC.H_LOG2]), int(h[TC.H_BD]); n = 1 << log2
    c_idx = 0 if kind == TC.LUMA else (b + 1 if kind == TC.PAIR else kind); sh = 1 if c_idx else 0
    pred = res = None
    if h[TC.H_CBF0 + b]:
        lev = np.ascontiguousarray(cs.lev[ci, b, :n * n])
        if h[TC.H_BYP]:
            res = lev.copy()
        else:
            d = np.zeros(n * n, np.int16); res = np.zeros(n * n, np.int16)
            L.hevc_dequant(lev.ctypes.data, d.ctypes.data, log2, int(h[TC.H_QP0 + b]), bd)
            if h[TC.H_TS]: L.hevc_inv_transform_skip(d.ctypes.data, res.ctypes.data, log2, bd)
            else: L.hevc_inv_transform(d.ctypes.data, res.ctypes.data, log2, int(c_idx == 0 and log2 == 2 and h[TC.H_INTRA]), bd)
        res = res.reshape(n, n).astype(np.int64)
    if h[TC.H_INTRA]:
        planes = [np.full((PIC >> s, PIC >> s), 0xA5A5, np.uint16) for s in (0, 1, 1)]
        f = _Frame(PIC, PIC, PIC // 2, PIC // 2, bd); f.p[:] = [p.ctypes.data for p in planes]
        done = np.zeros((PIC // 4, PIC // 4), np.uint8)
        # the CTB of the case: the one that holds luma (64, 64); a smaller CTB is the top-left part of that 64x64 area, whose surroundings count as other CTBs
        ox = 64 >> sh; x0, y0 = ox + int(h[TC.H_X0]), ox + int(h[TC.H_Y0]); unit = TC.unit_of_sample(kind, log2)
        for i in range(4 * n + 1):
            xn, yn = (x0 - 1, y0 + 2 * n - 1 - i) if i < 2 * n else (x0 - 1 + (i - 2 * n), y0 - 1)
            planes[c_idx][yn, xn] = cs.nb[ci, b, i]
            if cs.uav[ci, unit[i]]: done[(yn << sh) >> 2, (xn << sh) >> 2] = 1
        mm = m.contents; mm.done = done.ctypes.data; mm.strong_intra_smoothing = int(h[TC.H_STRONG])
        out = np.zeros(n * n, np.uint16)
        L.hevc_intra_pred_buf(C.byref(f), m, c_idx, x0, y0, log2, int(h[TC.H_MODE]), out.ctypes.data)
        pred = out.reshape(n, n).astype(np.int64)
    return pred, res


@pytest.mark.parametrize("group", TC.groups())
def test_the_text_equals_the_oracle(oracle, group):
    """the oracle's prediction is the text's; its residual, which it keeps in int16, gives the text's picture: Clip1(pred + res) for an intra block, Clip1(p + res) for
    p = 0, 2^(bd-1), 2^bd - 1 for an inter block"""
    L, m = oracle; cs = TC.build(); E = TC.expected(); bad = []
    keep = m.contents.done
    try:
        for ci in range(len(cs.ids)):
            if cs.groups[ci] != group:
                continue
            bd = int(cs.hdr[ci, TC.H_BD])
            for b, (pred, res) in enumerate(E[ci]):
                o_pred, o_res = _oracle_block(L, m, cs, ci, b)
                assert (pred is None) == (o_pred is None) and (res is None) == (o_res is None)
                if pred is not None and not np.array_equal(pred, o_pred):
                    bad.append("%s plane %d: prediction differs in %d samples" % (cs.ids[ci], b, int((pred != o_pred).sum())))
                if res is not None:
                    ps = [pred] if pred is not None else [0, 1 << (bd - 1), (1 << bd) - 1]
                    diff = sum((S.reconstruct(p, res, bd) != S.reconstruct(p, o_res, bd)) for p in ps).astype(bool)
                    if diff.any():
                        y, x = np.argwhere(diff)[0]
                        bad.append("oracle %s plane %d: %d samples differ; at (x %d, y %d) exact residual %d, the oracle's %d, the text's sample %d" % (
                            cs.ids[ci], b, int(diff.sum()), x, y, int(res[y, x]), int(o_res[y, x]), int(np.broadcast_to(S.reconstruct(ps[-1], res, bd), res.shape)[y, x])))
    finally:
        m.contents.done = keep                           # hevc_meta_free frees what hevc_meta_alloc allocated
    assert not bad, "\n".join(bad[:20])


# ---------------------------------------------------------------------------------------------------------------------- the bodies under the sanitizers
def test_bodies_under_the_sanitizers():
    """the hook's bodies - staging, rc_tile_tb / rc_tile_tb_cpair, copy back - as a stand-alone host program (tests/tb_check.cpp) built with the address and
    undefined-behaviour sanitizers: a program of its own, nothing of it is loaded into this process"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "tb_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-Wno-unused-variable", "-Wno-unused-but-set-variable", "-o", exe, os.path.join(HERE, "tb_check.cpp")], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
