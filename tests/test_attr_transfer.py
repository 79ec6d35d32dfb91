"""Attribute transfer after geometry smoothing (csrc/rbt_color.h: rbt_transfer_colors, rbt_reconstruct_decoded) - the kernel BODIES run as serial host code
(tests/hostemu, no GPU here) against a brute-force restatement of the definition in include/rbt.h (tests/attr_transfer_cases.py). The GPU build of the same is
tests/test_gpu_attr_transfer.py."""
import os
import subprocess
import pytest
import rbt_lib
import attr_transfer_cases as AT


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    R = rbt_lib.module()
    c = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


@pytest.mark.parametrize("seed", range(3))
def test_stage_equals_the_restatement(ctx, seed):
    """3000 points on a wavy sheet, 15 % moved by up to 2 per axis: all triples and n_changed == brute force; with smooth colours each of the four branches (identical
    source point, forward average kept, single-entry list, multi-entry list) is taken by at least 20 points, with random colours the forward path alone"""
    AT.check_surface(ctx, seed)


def test_tie_rules_and_volume_faces(ctx):
    """every point doubled with another colour (coincident candidates: the lower index first); 8th and 9th neighbour at the same distance; clusters in the corners of the
    1024^3 volume with moved points at coordinates 0 and 1023"""
    AT.check_tie_rules(ctx)


def test_known_answers(ctx):
    """one moved point, eight hand-placed neighbours at squared distances 2, 3, 5, 6, 8, 10, 11, 12: forward average (13, 30013, 20015 above 1000, 0, 0) and the
    eight-entry backward list with w = 1 / (sqrt(d) + 4), both written out in attr_transfer_cases.py"""
    AT.check_known_answers(ctx)


def test_arguments(ctx):
    """7 source points, a coordinate of 1024 or -1: RBT_ERR_PARAM; no moved point or no target point: nothing changes; a flagged point that did not move takes its source
    twin's colour; a moved point without 8 source points within the search bound: RBT_ERR_UNSUPPORTED, and the context works afterwards"""
    AT.check_arguments(ctx, rbt_lib.module())


@pytest.mark.parametrize("seed,two_axes", AT.CHAINED)
def test_reconstruct_decoded_on_seam_atlases(ctx, seed, two_axes):
    """grids 8, 4 and 16: positions == reconstruct_rgb's, moved.sum() == n_smoothed > 0, yuv == the restatement on (cloud without smoothing, smoothed cloud, moved),
    rgb == yuv16_to_rgb8 of it, unmoved points keep their colour; attr_transfer = 0 and smoothing off == reconstruct_rgb"""
    R = rbt_lib.module()
    AT.check_chained(ctx, R, AT.chained_case(R, seed, two_axes))


def test_reconstruct_decoded_with_smooth_attributes(ctx):
    """attribute pictures of wide plateaus instead of noise: the backward lists fill"""
    R = rbt_lib.module()
    AT.check_chained(ctx, R, AT.ramp_atlas(R, 0), lists=True)


def test_other_filter_types_are_refused(ctx):
    AT.check_chained_unsupported(ctx, rbt_lib.module())
