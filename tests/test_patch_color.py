"""Colour PSNR per patch of the decoded cloud (csrc/rbt_score.h "col/patch"; host/rbt_pcc.cpp: rbt_score_patches_color, rbt_score_pair_patches_color) and the colour floors
held patch by patch (rbt_submit_gof_color_patches) - the kernel BODIES run as serial host code (tests/hostemu, no GPU here) against the definition restated in
tests/patch_color_cases.py and against clouds rebuilt independently from the returned streams. The GPU build of the same is tests/test_gpu_patch_color.py."""
import os
import subprocess
import tempfile
import pytest
import rbt_lib
import patch_color_cases as PC


def make_ctx():
    return rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = make_ctx()
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(PC.SUM_CASES))
def test_sums_equal_the_definition(ctx, name):
    PC.check_sums(ctx, name)


def test_pair_equals_the_cloud_call_before_and_after_new_colours(ctx):
    PC.check_pair(ctx)


def test_two_calls_return_the_same_bits(ctx):
    PC.check_determinism(ctx)


def test_arguments(ctx):
    PC.check_score_arguments(rbt_lib.module(), ctx, make_ctx)


def test_merged_limit(ctx):
    PC.check_merged_limit(rbt_lib.module(), ctx)


# ---- the job ----
@pytest.mark.parametrize("handles", [True, False])
def test_report(ctx, handles):
    PC.check_report(rbt_lib.module(), ctx, handles)


@pytest.mark.parametrize("handles,channel", [(True, 0), (False, 1), (True, 2)])
def test_walk_moves_patches_both_ways(ctx, handles, channel):
    PC.check_walk(rbt_lib.module(), ctx, handles, channel)


def test_max_trials_caps_the_walk(ctx):
    PC.check_walk(rbt_lib.module(), ctx, False, 0, max_trials=2)


def test_job_arguments(ctx):
    PC.check_job_arguments(rbt_lib.module(), ctx, make_ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
def test_jobs_in_flight(ctx, depth, n_jobs):
    PC.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


def test_nothing_leaks_between_job_kinds(ctx):
    PC.check_no_leak_between_kinds(rbt_lib.module(), ctx)


def test_bodies_under_the_sanitizers():
    """the serial body of the per-patch colour kernel and the host-only figure / trial source as a stand-alone host program (tests/patch_color_check.cpp) built with the
    address and undefined-behaviour sanitizers: a program of its own, nothing of it is loaded into this process"""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "patch_color_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-o", exe, os.path.join(here, "patch_color_check.cpp")], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
