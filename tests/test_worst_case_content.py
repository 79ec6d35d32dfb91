"""Worst-case content (noise in all three planes, checkerboards) through the encoder, the decoder and the transcoder on the host emulation (tests/hostemu: the product's
host code, the kernels' bodies as serial host code): the table of tests/worst_case_cases.py - slice QPs on both sides of every band of the output sizing, lossless, 8 and
10 bit, every slice structure - must encode to the oracle's bytes and decode to its pictures. tests/test_gpu_worst_case_content.py runs the same table on the GPU."""
import os
import subprocess
import pytest
import rbt_lib
import worst_case_cases as WC


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    R = rbt_lib.module()
    c = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


def test_the_table_covers_what_it_claims(ctx):
    """both sides of each band edge (slice QP 15 | 16 and 33 | 34) for I and for P slices, the ends of the QP range, lossless, both bit depths, every content and structure"""
    i_qps = {WC.slice_qps(c)[0] for c in WC.CASES if not c.lossless}
    p_qps = {WC.slice_qps(c)[1] for c in WC.CASES if not c.lossless}
    assert {0, 15, 16, 33, 34} <= i_qps and {0, 15, 16, 33, 34, 51} <= p_qps
    for kind in WC.KINDS:
        assert {8, 10} <= {c.bd for c in WC.CASES if c.kind == kind} and any(c.lossless for c in WC.CASES if c.kind == kind)
    assert {(c.log2_ctb, c.rows) for c in WC.CASES} >= {(l, r) for l in (4, 5, 6) for r in (-1, 0, 1)}
    assert all(c.w * c.h * c.n >= 1280 * 256 * 2 for c in WC.CASES)
    R = rbt_lib.module()
    assert (R.RBT_ERR_NOMEM, R.RBT_ERR_OUTPUT) == (-5, WC.RBT_ERR_OUTPUT)
    assert ctx.L.rbt_strerror(WC.RBT_ERR_OUTPUT) not in (ctx.L.rbt_strerror(-5), ctx.L.rbt_strerror(-99))      # a text of its own, not "out of memory" / "unknown error"


@pytest.mark.parametrize("case", WC.CASES, ids=WC.case_id)
def test_encode_and_decode_equal_the_oracle(ctx, case):
    WC.check_case(ctx, case)


@pytest.mark.parametrize("kind,video_type,qp", WC.TRANSCODES)
def test_transcode_of_noise_equals_the_oracle(ctx, kind, video_type, qp):
    """the oracle's stream of the content at QP 16 -> QP 24 / 32 as geometry and as attribute video"""
    WC.check_transcode(ctx, kind, video_type, qp)


def test_transcode_gof_of_three_noise_streams(ctx):
    WC.check_transcode_gof(ctx)


def test_noise_gof_between_two_ordinary_gofs_in_flight(ctx):
    WC.check_noise_between_ordinary_gofs(ctx)
