"""Normal estimation (csrc/rbt_normals.h: rbt_pcloud_estimate_normals, rbt_estimate_normals) - the kernel BODIES run as serial host code (tests/hostemu, no GPU here)
against a brute-force restatement of the definition in include/rbt.h (tests/normals_cases.py). The GPU build of the same is tests/test_gpu_normals.py."""
import os
import subprocess
import tempfile
import pytest
import rbt_lib
import attr_transfer_cases as AT
import normals_cases as NC


def make_ctx():
    return rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = make_ctx()
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(NC.CLOUDS))
def test_equals_the_definition(ctx, name):
    """sphere, slab, plane, the slab across a word boundary, at the faces of the volume, with outliers and cut to 1 .. 65 points, the sphere with duplicates: within 1 LSB
    of eigh where the eigen-gap allows the comparison; length, sign and one triple per voxel everywhere; the plane exactly (0, 0, +-16384); one point (0, 0, 0)"""
    NC.check_cloud(rbt_lib.module(), ctx, name)


def test_isotropic_cube(ctx):
    NC.check_isotropic_cube(rbt_lib.module(), ctx)


def test_view_point_inside_the_sphere(ctx):
    NC.check_view_point_inside(rbt_lib.module(), ctx)


def test_other_k(ctx):
    NC.check_other_k(rbt_lib.module(), ctx)


def test_order_and_duplicates(ctx):
    NC.check_order_and_duplicates(rbt_lib.module(), ctx)


def test_estimated_normals_allow_d2(ctx):
    NC.check_scoring(rbt_lib.module(), ctx)


@pytest.mark.parametrize("seed,two_axes", AT.CHAINED[:1])
def test_estimated_normals_on_a_cloud_from_maps(ctx, seed, two_axes):
    R = rbt_lib.module()
    NC.check_scoring_from_maps(R, ctx, AT.chained_case(R, seed, two_axes))


def test_arguments(ctx):
    NC.check_arguments(rbt_lib.module(), ctx, make_ctx)


def test_bodies_under_the_sanitizers():
    """search, integer sums, Jacobi iteration and Q14 rounding as a stand-alone host program (tests/normals_check.cpp) built with the address and undefined-behaviour
    sanitizers: a program of its own, nothing of it is loaded into this process"""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "normals_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-o", exe, os.path.join(here, "normals_check.cpp")], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
