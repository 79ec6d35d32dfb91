"""Device build of tests/test_tb_spec.py: every case of tests/tb_cases.py through rbt_selftest_tb on the GPU (csrc/rbt_kernels.hip k_selftest_tb: one wave per case calls
the decoder's rc_tile_tb / rc_tile_tb_cpair) against the text of H.265 restated in tests/tb_spec.py, bit for bit. What only the device has - the ballot over the units'
availability, the DPP wave sum of DC, the packed 16+16-bit sum of the Cb/Cr pair, the matrix-core stages of the 32-point transform - gets its ground truth here.

One launch serves all tests. A device error ends the run: nothing more is started on a device that has faulted."""
import faulthandler
import pytest
import rbt_lib
import tb_cases as TC

pytestmark = pytest.mark.gpu
TIMEOUT_S = 120


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(TIMEOUT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def device_out():
    R = rbt_lib.module()
    c = R.Context(device=0)
    try:
        out = TC.run_hook(c)
    except R.RbtError as e:
        if e.code == -1:                                                      # RBT_ERR_NO_DEVICE: a HIP error
            pytest.exit("device error in rbt_selftest_tb: %s" % e, returncode=3)
        raise
    c.close()
    return out


@pytest.mark.parametrize("group", TC.groups())
def test_the_text_equals_the_decoders_routine_on_the_device(device_out, group):
    bad = TC.compare(device_out, group, "device")
    assert not bad, "\n".join(bad[:20])

