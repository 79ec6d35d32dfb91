"""Colour half of the metric (csrc/rbt_color.h): 4:2:0 -> 4:4:4 up-conversion, YUV16 -> RGB8, reconstruction with decoder-side colours and the colour PSNR - the kernel
BODIES run as serial host code (tests/hostemu, no GPU here) against NumPy restatements written from the reference's text (tests/color_cases.py). The GPU build of the
same is tests/test_gpu_color.py."""
import os
import subprocess
import numpy as np
import pytest
import oracle_lib as O
import rbt_lib
import color_cases as CC
import pcc_cases


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    R = rbt_lib.module()
    c = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


def test_up_conversion_equals_the_restatement(ctx):
    """8 and 10 bit; 2x2, 4x6, 64x48, 130x70; noise, steps at the borders, full-range extremes and samples above the depth's range (clamps and final clip act):
    array equality with the float32 / float64 restatement; RBT_UPSAMPLE_REPLICATE == np.repeat in both axes"""
    CC.check_up(ctx, rbt_lib.module())


def test_up_conversion_of_a_full_size_pair(ctx):
    CC.check_up_large(ctx)


def test_up_conversion_known_answers(ctx):
    """constant pictures stay constant (chroma 512 -> 32768, luma k -> round(65535 (float)(k / 1023)) for every k); a single bright chroma sample in a flat field gives the
    outer product of the tap rows, worked out from the taps"""
    CC.check_up_known_answers(ctx, rbt_lib.module())


def test_up_conversion_bad_arguments(ctx):
    CC.check_up_bad_arguments(ctx, rbt_lib.module())


def test_rgb_equals_the_restatement(ctx):
    """{0, 1, 32767, 32768, 65534, 65535}^3 and 100 000 random triples == convertYUV16ToRGB8 in float64; white and black"""
    CC.check_rgb(ctx)


@pytest.mark.parametrize("seed", range(8))
def test_reconstruct_rgb_on_random_atlases(ctx, seed):
    """xyz / occupancy_map / block_to_patch == reconstruct's; yuv == the restated 4:4:4 planes at each point's pixel; rgb == the restated conversion; and reconstruct with
    4:2:0 attributes still gives the oracle's bytes"""
    R = rbt_lib.module()
    CC.check_reconstruct_rgb(ctx, R, pcc_cases.random_atlas(R, seed), O.reconstruct)


def test_reconstruct_rgb_known_answer(ctx):
    CC.check_reconstruct_rgb_known_answer(ctx, rbt_lib.module())


def test_geometry_smoothing_moves_points_not_colours(ctx):
    R = rbt_lib.module()
    case = pcc_cases.seam_atlas(R, 0, tiles=3)
    plain = list(case); plain[0] = pcc_cases._copy_atlas(R, case[0], geometry_smoothing=0)
    a, b = ctx.reconstruct_rgb(*case), ctx.reconstruct_rgb(*plain)
    assert (a[0] != b[0]).any() and np.array_equal(a[0], ctx.reconstruct(*case)[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4])


@pytest.mark.parametrize("k", range(6))
def test_colour_metric_equals_brute_force(ctx, k):
    """n_a, n_b and the six sse integers == brute force (voxels merged with floor means, ALL points at the minimum squared distance, rounded mean, integer error terms);
    mse / psnr == recomputed from the integers; the reference's float form within the derived bound; swapping a and b swaps the directions"""
    CC.check_metric_case(ctx, CC.metric_cases()[k])


def test_colour_metric_identity_and_bad_arguments(ctx):
    CC.check_metric_identity_and_bad_arguments(ctx, rbt_lib.module())
