"""GPU parity of the slice parser's two instantiations (csrc/rbt_parse.h): I slices take the intra-only one, P slices the general one; the streams are in
tests/parser_intra_path_cases.py. Which instantiation a slice type takes is decided by one branch on the slice record (rbt_parse_slice); its host-emulation twin
(tests/test_hostemu_parser_intra_path.py) counts the slices each one parsed."""
import pytest
import rbt_lib
import parser_intra_path_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    R = rbt_lib.module()
    c = R.Context(device=0)
    yield c
    c.close()


@pytest.mark.parametrize("gop", [1, 2])
@pytest.mark.parametrize("w,h,log2_ctb,rows", K.GRID)
def test_i_and_p_pictures(ctx, w, h, log2_ctb, rows, gop):
    K.check_grid(ctx, w, h, log2_ctb, rows, gop)


@pytest.mark.parametrize("seed", K.STRESS_SEEDS)
def test_p_slices_with_intra_cus(ctx, seed):
    K.check_stress(ctx, seed)


def test_lossless_8bit(ctx):
    K.check_lossless(ctx)


def test_banded_parse():
    K.run_banded(None)
