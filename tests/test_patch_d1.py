"""D1 per patch of the decoded cloud (csrc/rbt_score.h "patches"; host/rbt_pcc.cpp: rbt_pcloud_set_labels, rbt_pcloud_labels, rbt_score_patches) - the kernel BODIES run as
serial host code (tests/hostemu, no GPU here) against the definition restated in tests/patch_d1_cases.py and the oracle's reconstruction. The GPU build of the same is
tests/test_gpu_patch_d1.py."""
import os
import subprocess
import tempfile
import pytest
import rbt_lib
import patch_d1_cases as PD


def make_ctx():
    return rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = make_ctx()
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(PD.SUM_CASES))
def test_sums_equal_the_definition(ctx, name):
    PD.check_sums(ctx, name)


def test_two_calls_return_the_same_words(ctx):
    PD.check_determinism(ctx)


def test_arguments(ctx):
    PD.check_score_arguments(rbt_lib.module(), ctx, make_ctx)


@pytest.mark.parametrize("name", PD.LABEL_CASES)
def test_labels_of_a_cloud_made_from_maps(ctx, name):
    PD.check_labels(rbt_lib.module(), ctx, name)


def test_a_cloud_made_from_maps_scores_with_its_labels(ctx):
    PD.check_labels_score(rbt_lib.module(), ctx)


def test_frame_without_patches(ctx):
    PD.check_no_patches(rbt_lib.module(), ctx)


# ---- D1 floors held patch by patch (rbt_submit_gof_d1_patches) ----
@pytest.mark.parametrize("k", range(len(PD.REPORT_CASES)))
def test_report_only(ctx, k):
    PD.check_report(rbt_lib.module(), ctx, k)


def test_walk_moves_patches_both_ways(ctx):
    """(seam128, QP 30, CTBs of 32): the premise on the oracle alone, then the replay, then a patch below and one above q0 in every frame"""
    PD.check_main_premise()
    PD.check_main_walk(rbt_lib.module(), ctx)


@pytest.mark.parametrize("k", range(PD.N_REPLAY))
def test_walk_is_the_replay(ctx, k):
    PD.check_replay(rbt_lib.module(), ctx, k)


def test_edges_of_the_walk(ctx):
    PD.check_edges(rbt_lib.module(), ctx)


def test_job_arguments(ctx):
    PD.check_job_arguments(rbt_lib.module(), ctx, make_ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
def test_jobs_in_flight(ctx, depth, n_jobs):
    PD.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


def test_two_gofs_in_shared_pipelines(ctx):
    PD.check_two_gofs(rbt_lib.module(), ctx)


def test_nothing_leaks_between_kinds_of_job(ctx):
    PD.check_no_leak_between_kinds(rbt_lib.module(), ctx)


def test_bodies_under_the_sanitizers():
    """the serial bodies of the label, check and sum kernels as a stand-alone host program (tests/patch_d1_check.cpp) built with the address and undefined-behaviour
    sanitizers: a program of its own, nothing of it is loaded into this process"""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "patch_d1_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-o", exe, os.path.join(here, "patch_d1_check.cpp")], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
