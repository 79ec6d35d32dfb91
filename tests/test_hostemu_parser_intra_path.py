"""The cases of tests/test_gpu_parser_intra_path.py over the host emulation (the same csrc/rbt_parse.h as serial host code), plus what only this build can show: the
emulation counts the slices each instantiation of the parser took (rbt_hostemu_parse_paths: [general, intra-only]), so every case also proves WHICH one it ran."""
import ctypes
import os
import subprocess
import pytest
import rbt_lib
import parser_intra_path_cases as K


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    R = rbt_lib.module()
    c = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


def paths():
    v = (ctypes.c_uint32 * 2).in_dll(ctypes.CDLL(rbt_lib.HOSTEMU_LIB), "rbt_hostemu_parse_paths")
    return v[0], v[1]


@pytest.mark.parametrize("gop", [1, 2])
@pytest.mark.parametrize("w,h,log2_ctb,rows", K.GRID)
def test_i_and_p_pictures(ctx, w, h, log2_ctb, rows, gop):
    g0, i0 = paths()
    K.check_grid(ctx, w, h, log2_ctb, rows, gop)
    g1, i1 = paths()
    assert i1 > i0                                   # the I pictures went through the intra-only instantiation ...
    assert (g1 > g0) == (gop == 2)                   # ... and only a P picture through the general one
    if gop == 2: assert i1 - i0 == 2 * (g1 - g0)     # I P I, cut into the same slices and row tasks


@pytest.mark.parametrize("seed", K.STRESS_SEEDS)
def test_p_slices_with_intra_cus(ctx, seed):
    g0, i0 = paths()
    K.check_stress(ctx, seed)
    g1, i1 = paths()
    assert g1 > g0 and i1 > i0


def test_lossless_8bit(ctx):
    g0, i0 = paths()
    K.check_lossless(ctx)
    g1, i1 = paths()
    assert g1 == g0 and i1 > i0


def test_banded_parse(ctx):
    K.run_banded(rbt_lib.HOSTEMU_LIB)
