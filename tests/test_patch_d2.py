"""D2 per patch of the decoded cloud (csrc/rbt_score.h "D2/patch"; host/rbt_pcc.cpp: rbt_score_patches_d2) and the D2 floors on the stream and patch by patch
(rbt_submit_gof_d2, rbt_submit_gof_d2_patches) - the kernel BODIES run as serial host code (tests/hostemu, no GPU here) against the definition restated in
tests/patch_d2_cases.py and against clouds rebuilt independently from the returned streams. The GPU build of the same is tests/test_gpu_patch_d2.py."""
import os
import subprocess
import tempfile
import pytest
import rbt_lib
import patch_d2_cases as P2


def make_ctx():
    return rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = make_ctx()
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(P2.SUM_CASES))
def test_sums_equal_the_definition(ctx, name):
    P2.check_sums(ctx, name)


def test_a_second_block_in_a_column(ctx):
    P2.check_large(ctx)


def test_two_calls_return_the_same_bits(ctx):
    P2.check_determinism(ctx)


def test_arguments(ctx):
    P2.check_score_arguments(rbt_lib.module(), ctx, make_ctx)


# ---- the jobs ----
@pytest.mark.parametrize("handles", [True, False])
def test_stream_report(ctx, handles):
    P2.check_stream_report(rbt_lib.module(), ctx, handles)


@pytest.mark.parametrize("handles,stat", [(True, 0), (False, 1)])
def test_stream_walk(ctx, handles, stat):
    P2.check_stream_walk(rbt_lib.module(), ctx, handles, stat=stat)


@pytest.mark.parametrize("handles", [True, False])
def test_patch_report(ctx, handles):
    P2.check_patch_report(rbt_lib.module(), ctx, handles)


@pytest.mark.parametrize("handles", [True, False])
def test_patch_walk_moves_patches_both_ways(ctx, handles):
    P2.check_patch_walk(rbt_lib.module(), ctx, handles)


def test_normals_parameters_reach_the_estimation(ctx):
    P2.check_normals_params(rbt_lib.module(), ctx)


def test_job_arguments(ctx):
    P2.check_job_arguments(rbt_lib.module(), ctx, make_ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
def test_jobs_in_flight(ctx, depth, n_jobs):
    P2.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


def test_nothing_leaks_between_d1_and_d2_jobs(ctx):
    P2.check_no_leak_between_kinds(rbt_lib.module(), ctx)


def test_bodies_under_the_sanitizers():
    """the serial bodies of the per-patch D2 kernels and the host-only figure / trial source as a stand-alone host program (tests/patch_d2_check.cpp) built with the
    address and undefined-behaviour sanitizers: a program of its own, nothing of it is loaded into this process"""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "patch_d2_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-o", exe, os.path.join(here, "patch_d2_check.cpp")], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
