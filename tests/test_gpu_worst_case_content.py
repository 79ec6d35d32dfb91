"""The table of tests/worst_case_cases.py on the GPU: noise and checkerboards at slice QPs around every band of the encoder's output sizing, lossless, 8 and 10 bit, every
slice structure. Encoder == oracle byte for byte, and the parser and the reconstruction read every oracle stream back to the oracle's pictures (dense coefficients, long
escape codes, clipping at QP 0). Plus one I/P pair of noise at the benchmark's picture size per band edge, and the transcodes of tests/test_worst_case_content.py."""
import pytest
import rbt_lib
import worst_case_cases as WC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    R = rbt_lib.module()
    c = R.Context(device=0)
    yield c
    c.close()


@pytest.mark.parametrize("case", WC.CASES + WC.FULL_SIZE, ids=WC.case_id)
def test_encode_and_decode_equal_the_oracle(ctx, case):
    WC.check_case(ctx, case)


@pytest.mark.parametrize("kind,video_type,qp", WC.TRANSCODES)
def test_transcode_of_noise_equals_the_oracle(ctx, kind, video_type, qp):
    WC.check_transcode(ctx, kind, video_type, qp)


def test_transcode_gof_of_three_noise_streams(ctx):
    WC.check_transcode_gof(ctx)


def test_noise_gof_between_two_ordinary_gofs_in_flight(ctx):
    WC.check_noise_between_ordinary_gofs(ctx)
