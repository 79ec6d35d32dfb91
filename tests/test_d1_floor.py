"""Transcoding geometry to a D1 floor (csrc/rbt_cloudmaps.h, host/rbt_d1_walk.h, host/rbt_pcc.cpp, host/rbt_transcode.cpp: rbt_submit_gof_d1 / rbt_wait_gof_d1 /
rbt_transcode_gof_d1, rbt_gather_luma) - the kernel bodies and the host's walk run as serial host code (tests/hostemu, no GPU here) against the oracle's streams, clouds and
D1 figures and the walk restated in tests/d1_floor_cases.py. The GPU build of the same is tests/test_gpu_d1_floor.py."""
import os
import subprocess
import tempfile
import pytest
import rbt_lib
import d1_floor_cases as DC


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


@pytest.mark.parametrize("rd", [0, 1])
def test_walk(ctx, rd):
    """floors above and below every D(q), a midpoint around QP 30 started from 24, 30 and 40: q*, q0, qs, met, the bound on the encodes, every integer field of the
    frame's D1 result, and the oracle's stream at q*"""
    DC.check_walk(rbt_lib.module(), ctx, rd)


def test_walk_where_d1_is_not_monotone(ctx):
    DC.check_not_monotone(rbt_lib.module(), ctx)


def test_smoothing_and_several_frames(ctx):
    DC.check_smoothing_frames(rbt_lib.module(), ctx)


def test_strides_and_windows(ctx):
    DC.check_cropped(rbt_lib.module(), ctx)


def test_reference_handles(ctx):
    DC.check_reference_handles(rbt_lib.module(), ctx)


def test_composition_through_the_public_calls(ctx):
    DC.check_composition(rbt_lib.module(), ctx)


def test_jobs(ctx):
    DC.check_jobs(rbt_lib.module(), ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
def test_jobs_in_flight(ctx, depth, n_jobs):
    DC.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


def test_arguments(ctx):
    DC.check_arguments(rbt_lib.module(), ctx)


@pytest.mark.parametrize("n_pics", [1, 3])
@pytest.mark.parametrize("w", DC.GATHER_WIDTHS)
def test_gather_equals_slicing(ctx, w, n_pics):
    DC.check_gather(ctx, w, n_pics)


def test_gather_arguments(ctx):
    DC.check_gather_arguments(rbt_lib.module(), ctx)


def test_determinism(ctx):
    DC.check_determinism(rbt_lib.module(), ctx)


def test_bodies_under_the_sanitizers():
    """the gather kernel's body and the D1 walk as a stand-alone host program (tests/d1_check.cpp) built with the address and undefined-behaviour sanitizers: a program of
    its own, nothing of it is loaded into this process"""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "d1_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-o", exe, os.path.join(here, "d1_check.cpp")], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
