"""PSNR floors held patch by patch (csrc/rbt_ctbsse.h, host/rbt_patch_walk.h, host/rbt_transcode.cpp: rbt_ctb_sse, rbt_submit_gof_quality_patches / rbt_wait_gof_quality_patches) -
the kernel BODIES and the host's walk run as serial host code (tests/hostemu, no GPU here) against the definitions restated in tests/patch_floor_cases.py, the oracle's
constant-QP streams and its decoder. The GPU build of the same is tests/test_gpu_patch_floor.py."""
import os
import subprocess
import tempfile
import pytest
import rbt_lib
import patch_floor_cases as PC


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(PC.SUM_CASES))
def test_sums_equal_the_definition(ctx, name):
    PC.check_sums(ctx, name)


def test_ctb_sse_arguments(ctx):
    PC.check_sums_arguments(rbt_lib.module(), ctx)


@pytest.mark.parametrize("k", range(len(PC.REPORT_CASES)))
def test_report_only(ctx, k):
    PC.check_report(rbt_lib.module(), ctx, k)


def test_walk_moves_patches_both_ways(ctx):
    """("128", geo, QP 30, log2_ctb 5, all samples, F = 46.5 dB): the premise on the oracle alone, then the replay, then a patch below and one above q0 in every frame"""
    PC.check_main_premise()
    PC.check_main_walk(rbt_lib.module(), ctx)


@pytest.mark.parametrize("k", range(len(PC.REPLAY_CASES)))
def test_walk_is_the_replay(ctx, k):
    PC.check_replay(rbt_lib.module(), ctx, k)


def test_edges_of_the_walk(ctx):
    PC.check_edges(rbt_lib.module(), ctx)


def test_arguments(ctx):
    PC.check_arguments(rbt_lib.module(), ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
def test_jobs_in_flight(ctx, depth, n_jobs):
    PC.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


def test_two_gofs_in_shared_pipelines(ctx):
    PC.check_two_gofs(rbt_lib.module(), ctx)


def test_bodies_under_the_sanitizers():
    """the walk of host/rbt_patch_walk.h and the two kernel bodies as a stand-alone host program (tests/patch_floor_check.cpp) built with the address and undefined-behaviour
    sanitizers: a program of its own, nothing of it is loaded into this process"""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "patch_floor_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-o", exe, os.path.join(here, "patch_floor_check.cpp")], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
