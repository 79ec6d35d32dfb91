"""The recolouring route (csrc/rbt_score.h: recolour, colour walks on stored distances; csrc/rbt_cloudmaps.h: the gather on 4:2:0 pictures; rbt_pcloud_set_colors,
rbt_score_pair_*, rbt_gather_420) - the kernel bodies run as serial host code (tests/hostemu, no GPU here) against fresh uploads, the colour part of rbt_score, the brute
force of tests/color_cases.py and NumPy slicing. The GPU build of the same is tests/test_gpu_color_floor.py."""
import os
import subprocess
import tempfile
import pytest
import rbt_lib
import color_floor_cases as FC


def make_ctx():
    return rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = make_ctx()
    yield c
    c.close()


def test_recoloured_cloud_scores_as_a_fresh_upload(ctx):
    """voxels of 1, 2 and 300 points, duplicates of different colours"""
    FC.check_set_colors(ctx, *FC.crowded_cloud())


@pytest.mark.parametrize("n", FC.SET_SIZES)
def test_recolour_sizes(ctx, n):
    FC.check_set_colors(ctx, *FC.sized_cloud(n))


@pytest.mark.parametrize("k", (0, 4))
def test_pair_equals_the_colour_part_of_the_score(ctx, k):
    FC.check_pair(ctx, k)


def test_pair_single_point_clouds(ctx):
    FC.check_pair_single_points(ctx)


def test_arguments(ctx):
    FC.check_arguments(rbt_lib.module(), ctx, make_ctx)


@pytest.mark.parametrize("n_pics", [1, 3])
@pytest.mark.parametrize("w", FC.GATHER_WIDTHS)
def test_gather_420_equals_slicing(ctx, w, n_pics):
    FC.check_gather(ctx, w, n_pics)


def test_gather_420_feeds_the_upconversion(ctx):
    FC.check_gather_feeds_upconversion(ctx)


def test_gather_420_arguments(ctx):
    FC.check_gather_arguments(rbt_lib.module(), ctx)


@pytest.mark.parametrize("name", ("synth", "seam_smooth", "cropped"))
def test_job_equals_the_composition(ctx, name):
    """floors above, below and between the values of D(q) = rbt_transcode_gof -> rbt_decode -> rbt_pcloud_from_maps -> rbt_score: q0, qs, q*, met, the bound on the encodes,
    the stream at q*, every field of every frame"""
    FC.check_job_case(rbt_lib.module(), ctx, name)


def test_job_stats_and_channels(ctx):
    FC.check_stats_and_channels(rbt_lib.module(), ctx)


def test_job_reference_handles(ctx):
    FC.check_reference_handles(rbt_lib.module(), ctx)


def test_job_occupancy_rd(ctx):
    FC.check_occupancy_rd(rbt_lib.module(), ctx)


def test_job_against_independent_arithmetic(ctx):
    FC.check_against_independent_arithmetic(rbt_lib.module(), ctx)


def test_jobs_in_flight(ctx):
    FC.check_jobs_in_flight(rbt_lib.module(), ctx)


def test_job_pairing_and_memory(ctx):
    FC.check_pairing_and_memory(rbt_lib.module(), ctx)


def test_job_determinism(ctx):
    FC.check_determinism(rbt_lib.module(), ctx)


def test_job_arguments(ctx):
    FC.check_job_arguments(rbt_lib.module(), ctx)


def test_more_than_2_21_merged_points(ctx):
    FC.check_merged_limit(rbt_lib.module(), ctx)


def test_bodies_under_the_sanitizers():
    """the recolour bodies, the colour walks on stored distances and the 4:2:0 gather descriptors as a stand-alone host program (tests/color_floor_check.cpp) built with the
    address and undefined-behaviour sanitizers: a program of its own, nothing of it is loaded into this process"""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "color_floor_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-o", exe, os.path.join(here, "color_floor_check.cpp")], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
