"""Flat chroma on the GPU: the cases of tests/flat_chroma_cases.py through the HIP build, and the committed 1280x1280 geometry fixture, whose 64
pictures must all be taken as flat - what the rule is for."""
import os
import numpy as np
import pytest
import rbt_lib
import flat_chroma_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    return rbt_lib.module()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(device=0)
    yield c
    c.close()


@pytest.mark.parametrize("log2_ctb", [4, 5, 6])
@pytest.mark.parametrize("rows", [-1, 0, 1])
def test_geometry_gof_is_flat(ctx, R, log2_ctb, rows):
    F.check_geometry(ctx, R, log2_ctb, rows)


def test_geometry_with_partial_ctbs_and_a_window(ctx, R):
    F.check_geometry_partial_ctbs(ctx, R)


def test_attribute_gof_is_not_flat(ctx, R):
    F.check_attribute(ctx, R)


@pytest.mark.parametrize("which", sorted(F.NEAR))
def test_one_sample_off_is_not_flat(ctx, R, which):
    F.check_near_flat(ctx, R, which)


@pytest.mark.parametrize("cb,cr", [(500, 500), (512, 500)])
def test_constant_at_another_value_is_not_flat(ctx, R, cb, cr):
    F.check_other_constant(ctx, R, cb, cr)


@pytest.mark.parametrize("w,h", [(64, 64), (72, 40)])
def test_lossless_8_bit_occupancy(ctx, R, w, h):
    F.check_occupancy(ctx, R, w, h)


@pytest.mark.parametrize("rows", [1, -1])
def test_row_slices_and_wavefront_input(ctx, R, rows):
    F.check_row_slices(ctx, R, rows)


def test_occupancy_rd_over_flat_geometry(ctx, R):
    F.check_occupancy_rd(ctx, R)


def test_banded_parse_takes_no_picture_as_flat():
    F.run_worker("gpu", "banded", {"RBT_PARSE_BANDS": "2"})


def test_sixteen_jobs_out_of_order(ctx, R):
    F.check_sixteen_jobs(ctx, R)


def test_fan_out_from_one_decode(ctx, R):
    F.check_fan_out(ctx, R)


def test_walks_over_a_flat_entry(ctx, R):
    F.check_walks(ctx, R)


@pytest.mark.parametrize("share", ["0", "1"])
def test_arena_sharing_on_and_off(share):
    F.run_worker("gpu", "arena", {"RBT_ARENA_SHARE": share})


def test_committed_geometry_fixture_is_flat_throughout(ctx):
    """64 pictures of 1280x1280 as the CTC's encoder wrote them: every hash SEI of the stream checks (the encoder's own reconstruction, an independent reference),
    both chroma planes are 512 everywhere, and all 64 pictures were taken as flat. A count below 64 means the rule is too coarse for real input."""
    s = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hm_r5_1280x1280_f32_geo.annexb"), "rb").read()
    dec, w, h, bd, chk, fail = ctx.decode(s)
    assert (w, h, bd, dec.shape[0]) == (1280, 1280, 10, 64) and (chk, fail) == (64, 0)
    assert (dec[:, w * h:] == 512).all()
    assert ctx.flat_pictures() == 64
