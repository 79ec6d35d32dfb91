"""Flat chroma on the host build of the kernel bodies: the cases of tests/flat_chroma_cases.py, each against the oracle and against the number of
pictures the stream's syntax makes flat. The GPU run of the same cases: tests/test_gpu_flat_chroma.py."""
import ctypes
import os
import subprocess
import pytest
import rbt_lib
import flat_chroma_cases as F


@pytest.fixture(scope="module")
def hostemu():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])


@pytest.fixture(scope="module")
def R():
    return rbt_lib.module()


@pytest.fixture(scope="module")
def ctx(hostemu, R):
    c = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


def flat_ctbs():
    """CTBs that took the flat path of the encoder's intra stage, inter stage and SAO stage so far (a counter of the host build: rbt_hostemu_flat_ctbs)"""
    return list((ctypes.c_uint32 * 3).in_dll(ctypes.CDLL(rbt_lib.HOSTEMU_LIB), "rbt_hostemu_flat_ctbs"))


def test_encoder_takes_the_flat_path_where_the_source_is_flat(ctx, R):
    """The output bytes are the oracle's with or without the encoder's fast path, so the flat count of the decoder says nothing about it: the host build counts the
    CTBs that took it. 128x128 re-encoded with 32x32 CTBs is 16 CTBs per picture: two I and two P pictures of a flat geometry stream take it everywhere, SAO
    included; the pooled occupancy pictures (32x32: one CTB each, lossless: no SAO) take it by construction; an attribute stream never does."""
    def delta(fn):
        a = flat_ctbs(); fn(); b = flat_ctbs()
        return [y - x for x, y in zip(a, b)]
    assert delta(lambda: F.transcode_is(ctx, F.geo_stream()[0], R.RBT_VIDEO_GEOMETRY, 24, 4, log2_ctb=5, rows_per_slice=-1)) == [32, 32, 64]
    assert delta(lambda: F.transcode_is(ctx, F.occ_stream()[0], R.RBT_VIDEO_OCCUPANCY, 8, 2, occupancy_precision=4, log2_ctb=5, rows_per_slice=-1)) == [2, 0, 0]
    assert delta(lambda: F.transcode_is(ctx, F.occ_stream()[0], R.RBT_VIDEO_OCCUPANCY, 8, 2, occupancy_precision=2, log2_ctb=5, rows_per_slice=-1)) == [8, 0, 0]
    assert delta(lambda: F.transcode_is(ctx, F.attr_stream()[0], R.RBT_VIDEO_ATTRIBUTE, 32, 0, log2_ctb=5, rows_per_slice=-1)) == [0, 0, 0]
    assert delta(lambda: F.check_near_flat(ctx, R, "cr_only")) == [16, 16, 32]          # pictures 2 and 3 only


@pytest.mark.parametrize("log2_ctb", [4, 5, 6])
@pytest.mark.parametrize("rows", [-1, 0, 1])
def test_geometry_gof_is_flat(ctx, R, log2_ctb, rows):
    F.check_geometry(ctx, R, log2_ctb, rows)


def test_geometry_with_partial_ctbs_and_a_window(ctx, R):
    F.check_geometry_partial_ctbs(ctx, R)


def test_attribute_gof_is_not_flat(ctx, R):
    F.check_attribute(ctx, R)


@pytest.mark.parametrize("which", sorted(F.NEAR))
def test_one_sample_off_is_not_flat(ctx, R, which):
    F.check_near_flat(ctx, R, which)


@pytest.mark.parametrize("cb,cr", [(500, 500), (512, 500)])
def test_constant_at_another_value_is_not_flat(ctx, R, cb, cr):
    F.check_other_constant(ctx, R, cb, cr)


@pytest.mark.parametrize("w,h", [(64, 64), (72, 40)])
def test_lossless_8_bit_occupancy(ctx, R, w, h):
    F.check_occupancy(ctx, R, w, h)


@pytest.mark.parametrize("rows", [1, -1])
def test_row_slices_and_wavefront_input(ctx, R, rows):
    F.check_row_slices(ctx, R, rows)


def test_occupancy_rd_over_flat_geometry(ctx, R):
    F.check_occupancy_rd(ctx, R)


def test_banded_parse_takes_no_picture_as_flat(hostemu):
    F.run_worker("hostemu", "banded", {"RBT_PARSE_BANDS": "2"})


def test_sixteen_jobs_out_of_order(ctx, R):
    F.check_sixteen_jobs(ctx, R)


def test_fan_out_from_one_decode(ctx, R):
    F.check_fan_out(ctx, R)


def test_walks_over_a_flat_entry(ctx, R):
    F.check_walks(ctx, R)


@pytest.mark.parametrize("share", ["0", "1"])
def test_arena_sharing_on_and_off(hostemu, share):
    F.run_worker("hostemu", "arena", {"RBT_ARENA_SHARE": share})
