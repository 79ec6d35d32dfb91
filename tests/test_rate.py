"""Transcoding to a byte budget (csrc/rbt_rate.h, host/rbt_transcode.cpp: rbt_level_census, rbt_rate_estimate, rbt_submit_gof_rate / rbt_wait_gof_rate,
rbt_transcode_v3c_rate) - the kernel BODY and the host's walk run as serial host code (tests/hostemu, no GPU here) against the definitions restated in
tests/rate_cases.py and the oracle's constant-QP streams. The GPU build of the same is tests/test_gpu_rate.py."""
import os
import subprocess
import tempfile
import pytest
import rbt_lib
import rate_cases as RC


def make_ctx():
    return rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = make_ctx()
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(RC.CENSUS_CASES))
def test_census_equals_the_definition(ctx, name):
    RC.check_census(ctx, name)


def test_a_level_of_one_lands_in_bin_qin_plus_4():
    RC.check_level_of_one()


@pytest.mark.parametrize("w,h,seed", RC.STREAMS)
@pytest.mark.parametrize("kind", sorted(RC.KINDS))
def test_estimate_is_the_formula(ctx, w, h, seed, kind):
    RC.check_estimate(ctx, w, h, seed, kind)


@pytest.mark.parametrize("w,h,seed", RC.STREAMS)
@pytest.mark.parametrize("kind", sorted(RC.KINDS))
def test_walk(ctx, w, h, seed, kind):
    """budgets above s(18) and below s(45), an exact s(q), s(q) - 1, ranges that end before the budget is met: q*, met, bytes, the bound on the encodes, and the oracle's stream at q*"""
    RC.check_walk(rbt_lib.module(), ctx, w, h, seed, kind)


def test_walk_across_the_plateau(ctx):
    RC.check_plateau(rbt_lib.module(), ctx)


@pytest.mark.parametrize("k", range(len(RC.VARIANTS)))
def test_walk_variants(ctx, k):
    """rows 1, log2_ctb 4 and 6, hash SEIs, RBT_PRESET_FAST"""
    RC.check_variant(rbt_lib.module(), ctx, k)


def test_mixed_job(ctx):
    RC.check_mixed_job(rbt_lib.module(), ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
def test_jobs_in_flight(ctx, depth, n_jobs):
    RC.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


def test_verify_md5(ctx):
    RC.check_verify_md5(rbt_lib.module(), ctx)


def test_arguments(ctx):
    RC.check_arguments(rbt_lib.module(), ctx)


def test_container(ctx):
    RC.check_container(rbt_lib.module(), ctx)


def test_bodies_under_the_sanitizers():
    """the census body, the estimate and the walk as a stand-alone host program (tests/rate_check.cpp) built with the address and undefined-behaviour sanitizers: a
    program of its own, nothing of it is loaded into this process"""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "rate_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-o", exe, os.path.join(here, "rate_check.cpp")], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
