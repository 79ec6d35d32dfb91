"""A QP per point-cloud frame (include/rbt.h: rbt_submit_gof_frame_qp, rbt_transcode_gof_frame_qp; host/rbt_transcode.cpp encode_plan) - the kernel BODIES run as serial
host code (tests/hostemu, no GPU here) against the oracle's constant-QP streams, frame by frame (tests/frame_qp_cases.py). The GPU build of the same is
tests/test_gpu_frame_qp.py."""
import os
import subprocess
import pytest
import rbt_lib
import frame_qp_cases as FC


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


@pytest.mark.parametrize("gof", FC.LIST_GOFS)
@pytest.mark.parametrize("kind", sorted(FC.KINDS))
def test_identity(ctx, gof, kind):
    """every Q[f] equal to the entry's QP: rbt_transcode_gof's bytes"""
    FC.check_identity(rbt_lib.module(), ctx, gof, kind)


@pytest.mark.parametrize("gof", FC.LIST_GOFS)
@pytest.mark.parametrize("kind", sorted(FC.KINDS))
def test_lists_compose_frame_by_frame(ctx, gof, kind):
    """ascending, descending and Q[f] < 3: every frame decodes to the constant-QP stream's frame at its QP, SEIs equal, slice NALs within 2 bytes"""
    FC.check_lists(rbt_lib.module(), ctx, gof, kind)


@pytest.mark.parametrize("k", range(len(FC.VARIANTS)))
def test_variants(ctx, k):
    """rows 1 / 0 / 2, log2_ctb 4, RBT_PRESET_FAST, hash SEIs (rbt_decode verifies them), occupancy_rd"""
    FC.check_variant(rbt_lib.module(), ctx, k)


def test_verify_md5(ctx):
    FC.check_verify_md5(rbt_lib.module(), ctx)


def test_arguments(ctx):
    FC.check_arguments(rbt_lib.module(), ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
def test_jobs_in_flight(ctx, depth, n_jobs):
    FC.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


def test_two_gofs_in_shared_pipelines(ctx):
    FC.check_two_gofs(rbt_lib.module(), ctx)


# ---- floors held frame by frame (rbt_submit_gof_quality_frames)
@pytest.mark.parametrize("gof", FC.LIST_GOFS)
@pytest.mark.parametrize("kind", sorted(FC.KINDS))
def test_frame_floors(ctx, gof, kind):
    """q*_f, qs_f, met_f, n_encodes_f, n_passes, pictures_encoded and the frames' bytes by the Python walk on the oracle's per-frame tables; the stream is the QP list's"""
    FC.check_frame_floors(rbt_lib.module(), ctx, gof, kind)


@pytest.mark.parametrize("rd,region", [(0, FC.ALL), (1, FC.ALL), (0, FC.OCCUPIED), (1, FC.OCCUPIED)])
def test_passes_over_a_subset_of_the_frames(ctx, rd, region):
    FC.check_subset_passes(rbt_lib.module(), ctx, rd, region)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16), (5, 3)])
def test_floor_jobs_in_flight(ctx, depth, n_jobs):
    FC.check_floor_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


def test_floor_two_gofs_in_shared_pipelines(ctx):
    FC.check_floor_two_gofs(rbt_lib.module(), ctx)


def test_floor_arguments(ctx):
    FC.check_floor_arguments(rbt_lib.module(), ctx)


def test_frame_walk_under_the_sanitizers():
    """the per-frame walk, the round and pass formation, the cut and the stream assembly as a stand-alone host program (tests/frame_qp_check.cpp) built with the address
    and undefined-behaviour sanitizers: a program of its own, nothing of it is loaded into this process"""
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "frame_qp_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-o", exe, os.path.join(here, "frame_qp_check.cpp")], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


def test_floor_container(ctx):
    FC.check_floor_container(rbt_lib.module(), ctx)


@pytest.mark.parametrize("k", range(len(FC.FLOOR_VARIANTS)))
def test_floor_variants(ctx, k):
    FC.check_floor_variant(rbt_lib.module(), ctx, k)


# ---- D1 floors frame by frame (rbt_submit_gof_d1_frames)
@pytest.mark.parametrize("rd", [0, 1])
def test_d1_frame_floors(ctx, rd):
    FC.check_d1_frames(rbt_lib.module(), ctx, rd)


def test_d1_frame_arguments(ctx):
    FC.check_d1_arguments(rbt_lib.module(), ctx)
