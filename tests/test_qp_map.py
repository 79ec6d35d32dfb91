"""A QP per CTB (include/rbt.h: rbt_submit_gof_qp_map, rbt_transcode_gof_qp_map, rbt_qp_map_from_patches; csrc/rbt_qpmap.h) - the kernel BODIES run as serial host code
(tests/hostemu, no GPU here) against the oracle's constant-QP streams and the oracle's decoder (tests/qp_map_cases.py). The GPU build of the same is
tests/test_gpu_qp_map.py."""
import os
import subprocess
import pytest
import rbt_lib
import qp_map_cases as MC


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


@pytest.mark.parametrize("gof,kind", [("128", "geo"), ("64", "attr"), ("96", "geo")])
def test_identity(ctx, gof, kind):
    """no map: rbt_transcode_gof's bytes, which are the oracle's"""
    MC.check_identity(rbt_lib.module(), ctx, gof, kind)


@pytest.mark.parametrize("k", range(len(MC.UNIFORM_CASES)))
def test_uniform_maps(ctx, k):
    """every M == q, every M[f] == Q[f]: the decoded pictures and hash SEIs of the constant-QP streams, frame by frame; the slice QPs of rule 3"""
    MC.check_uniform(rbt_lib.module(), ctx, k)


@pytest.mark.parametrize("k", range(len(MC.DECODE_CASES)))
def test_maps_decode_to_the_reconstruction(ctx, k):
    """checkerboard, ramp, per-frame patterns, 0 next to 51, values below 3, single CTBs, row starts, patch-derived maps behind occupancy_rd; every slice structure,
    log2_ctb 4..6, RBT_PRESET_FAST: the oracle's decoder and rbt_decode find every picture's MD5 right"""
    MC.check_decodes(rbt_lib.module(), ctx, k)


@pytest.mark.parametrize("gof,kind", MC.PLACEMENT_CASES)
def test_placement_premise(gof, kind):
    """the oracle's C(22) and C(40) differ by more than 4x on both sets of CTBs"""
    MC.check_placement_premise(gof, kind)


@pytest.mark.parametrize("gof,kind", MC.PLACEMENT_CASES)
def test_map_is_applied_where_it_says(ctx, gof, kind):
    MC.check_placement(rbt_lib.module(), ctx, gof, kind)


def test_arguments(ctx):
    MC.check_arguments(rbt_lib.module(), ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
def test_jobs_in_flight(ctx, depth, n_jobs):
    MC.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


def test_two_gofs_in_shared_pipelines(ctx):
    MC.check_two_gofs(rbt_lib.module(), ctx)


def test_map_from_patches(ctx):
    MC.check_from_patches(rbt_lib.module())


def test_qp_map_arithmetic_under_the_sanitizers():
    """the delta's range and wrap, the closed form of the predictor with the QpY rewrite, and the patch helper as a stand-alone host program (tests/qp_map_check.cpp) built
    with the address and undefined-behaviour sanitizers: a program of its own, nothing of it is loaded into this process"""
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "qp_map_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-o", exe, os.path.join(here, "qp_map_check.cpp")], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
