"""How one intra transform block is coded on the GPU: the cases of tests/intra_tb_cases.py through the HIP build, each against the oracle. On the GPU the
passes of a block run on the 64 lanes of a wave, so what the host build cannot show - a lane reading what another lane has not written yet - shows here as bytes that
differ. The host run of the same cases, with the counters that say what they reach: tests/test_intra_tb.py."""
import pytest
import rbt_lib
import intra_tb_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    return rbt_lib.module()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(device=0)
    yield c
    c.close()


@pytest.mark.parametrize("log2_ctb", [4, 5, 6])
@pytest.mark.parametrize("rows", [-1, 0, 1])
def test_ten_bit_geometry_and_attribute(ctx, log2_ctb, rows):
    T.check_ten_bit(ctx, log2_ctb, rows)


@pytest.mark.parametrize("log2_ctb", [4, 5, 6])
def test_eight_bit_lossless(ctx, log2_ctb):
    T.check_lossless(ctx, log2_ctb)


@pytest.mark.parametrize("bd,log2_ctb,rows", [(10, 5, -1), (10, 4, 1), (10, 6, 0), (8, 5, -1)])
def test_transform_skip(ctx, bd, log2_ctb, rows):
    T.check_transform_skip(ctx, bd, log2_ctb, rows)


@pytest.mark.parametrize("w,h", T.SIZES)
@pytest.mark.parametrize("log2_ctb", [5, 6])
def test_occupancy_aware_coding(ctx, R, w, h, log2_ctb):
    T.check_occupancy_aware(ctx, R, w, h, log2_ctb)


@pytest.mark.parametrize("w,h", T.SIZES)
@pytest.mark.parametrize("log2_ctb,rows", [(5, -1), (4, 1), (6, 0)])
def test_transcode_with_the_inputs_modes_as_hints(ctx, R, w, h, log2_ctb, rows):
    T.check_transcode_hints(ctx, R, w, h, log2_ctb, rows)


@pytest.mark.parametrize("k", T.QP_MAP_DECODES)
def test_qp_map_decodes_to_the_encoders_reconstruction(ctx, R, k):
    T.check_qp_map_decodes(ctx, R, k)


@pytest.mark.parametrize("k", T.QP_MAP_UNIFORM)
def test_uniform_qp_map_is_the_constant_qp_stream(ctx, R, k):
    T.check_qp_map_uniform(ctx, R, k)
