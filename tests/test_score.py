"""Frame scoring on device clouds (csrc/rbt_score.h: rbt_pcloud_upload, rbt_pcloud_from_maps, rbt_score, rbt_score_summary) - the kernel BODIES run as serial host code
(tests/hostemu, no GPU here) against brute-force restatements of the definitions and against rbt_d1 / rbt_d2 / rbt_color_metric (tests/score_cases.py). The GPU build of
the same is tests/test_gpu_score.py."""
import os
import subprocess
import pytest
import rbt_lib
import attr_transfer_cases as AT
import score_cases as SC


def make_ctx():
    return rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = make_ctx()
    yield c
    c.close()


@pytest.mark.parametrize("k", range(6))
def test_equals_the_definition(ctx, k):
    """the six clouds of color_cases.metric_cases() with seeded normals: D1 and colour == brute force and == rbt_d1 / rbt_color_metric field for field; D2 counts and
    maxima == rbt_d2, sums within rel 1e-9 of rbt_d2 and of brute force; swapped clouds swap the directions"""
    SC.check_base(ctx, k)


@pytest.mark.parametrize("name", sorted(SC.boundary_cases()))
def test_word_boundaries_and_faces(ctx, name):
    SC.check_boundary(ctx, name)


@pytest.mark.parametrize("name", SC.FAR)
def test_far_neighbours(ctx, name):
    """the decoded cloud 40 to 100 voxels away along each axis and along the diagonal, and three outliers up to 1500 voxels away on either side"""
    SC.check_far(ctx, name)


@pytest.mark.parametrize("n,side", SC.SIZES)
def test_sizes(ctx, n, side):
    SC.check_size(ctx, n, side)


def test_degenerate_clouds(ctx):
    """one point against one; identical clouds and a shuffled copy: every sse 0, every psnr +inf"""
    SC.check_degenerate(ctx)


def test_two_calls_give_the_same_bytes(ctx):
    SC.check_determinism(ctx)


def test_handles(ctx):
    SC.check_handles(rbt_lib.module(), make_ctx)


def test_arguments(ctx):
    SC.check_arguments(rbt_lib.module(), ctx, make_ctx)


@pytest.mark.parametrize("seed,two_axes", AT.CHAINED)
def test_from_maps_on_seam_atlases(ctx, seed, two_axes):
    """host copy == rbt_reconstruct_decoded; the handle scores as a handle uploaded from those arrays, against the same atlas without smoothing"""
    R = rbt_lib.module()
    SC.check_from_maps(R, ctx, AT.chained_case(R, seed, two_axes))


def test_from_maps_with_smooth_attributes(ctx):
    R = rbt_lib.module()
    SC.check_from_maps(R, ctx, AT.ramp_atlas(R, 0))


def test_summary():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    R = rbt_lib.module()
    SC.check_summary(type("M", (), {"FrameScore": R.FrameScore, "score_summary": staticmethod(lambda f: R.score_summary(f, R.load(rbt_lib.HOSTEMU_LIB)))}))
