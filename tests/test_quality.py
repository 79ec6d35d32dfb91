"""Transcoding to a PSNR floor (csrc/rbt_quality.h, host/rbt_quality_walk.h, host/rbt_transcode.cpp: rbt_picture_sse, rbt_submit_gof_quality / rbt_wait_gof_quality,
rbt_transcode_v3c_quality) - the kernel BODY and the host's walk run as serial host code (tests/hostemu, no GPU here) against the definitions restated in
tests/quality_cases.py and the oracle's constant-QP streams. The GPU build of the same is tests/test_gpu_quality.py."""
import os
import subprocess
import tempfile
import pytest
import rbt_lib
import quality_cases as QC


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(QC.SSE_CASES))
def test_sums_equal_the_definition(ctx, name):
    QC.check_sse(ctx, name)


def test_picture_sse_arguments(ctx):
    QC.check_sse_arguments(rbt_lib.module(), ctx)


@pytest.mark.parametrize("w,h,seed", QC.STREAMS)
@pytest.mark.parametrize("kind", sorted(QC.KINDS))
def test_report_only(ctx, w, h, seed, kind):
    """floor 0 at QP 30: the oracle's stream; sse and samples of all three planes against O.decode(input) and O.decode(output)"""
    QC.check_report(rbt_lib.module(), ctx, w, h, seed, kind)


def test_report_only_compares_the_displayed_area(ctx):
    QC.check_report_cropped(rbt_lib.module(), ctx)


@pytest.mark.parametrize("w,h,seed", QC.STREAMS)
@pytest.mark.parametrize("kind", sorted(QC.KINDS))
def test_walk(ctx, w, h, seed, kind):
    """floors above d(18) and below d(45), a midpoint around QP 30 started from 20, 30 and 44, a narrow range whose lower end misses: q*, q0, qs, met, bytes, sse, the bound
    on the encodes, and the oracle's stream at q*"""
    QC.check_walk(rbt_lib.module(), ctx, w, h, seed, kind)


def test_walk_where_the_distortion_is_not_monotone(ctx):
    QC.check_not_monotone(rbt_lib.module(), ctx)


@pytest.mark.parametrize("rd", [0, 1])
def test_occupied_floor(ctx, rd):
    QC.check_occupancy(rbt_lib.module(), ctx, rd)


def test_jobs(ctx):
    QC.check_jobs(rbt_lib.module(), ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
def test_jobs_in_flight(ctx, depth, n_jobs):
    QC.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


@pytest.mark.parametrize("depth", [1, 3])
def test_two_gofs_in_shared_pipelines(ctx, depth):
    QC.check_shared_pipelines(rbt_lib.module(), ctx, depth)


def test_verify_md5(ctx):
    QC.check_verify_md5(rbt_lib.module(), ctx)


def test_arguments(ctx):
    QC.check_arguments(rbt_lib.module(), ctx)


def test_container(ctx):
    QC.check_container(rbt_lib.module(), ctx)


def test_bodies_under_the_sanitizers():
    """the kernel body, PSNR, the floor and the walk as a stand-alone host program (tests/quality_check.cpp) built with the address and undefined-behaviour sanitizers: a
    program of its own, nothing of it is loaded into this process"""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "quality_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-o", exe, os.path.join(here, "quality_check.cpp")], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
