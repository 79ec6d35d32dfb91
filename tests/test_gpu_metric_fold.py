"""GPU build of rbt_d1, rbt_d2 and rbt_color_metric as upload + score + release of two temporary clouds (host/rbt_pcc.cpp) through the C ABI: every case of
tests/test_metric_fold.py on the device, the edge clouds identical to the host emulation's field for field.

Every test runs under a watchdog of its own (faulthandler ends the process when a call does not come back), and a device error ends the run: nothing more is started on a
device that has faulted."""
import faulthandler
import os
import subprocess
import pytest
import rbt_lib
import metric_fold_cases as MF
import pcc_cases
from test_gpu_frame_qp import device_guard

pytestmark = pytest.mark.gpu
TIMEOUT_S = 120


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(TIMEOUT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    c = rbt_lib.module().Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


@pytest.mark.parametrize("which", MF.CALLS)
@device_guard
def test_refusals_keep_code_and_text(ctx, which):
    MF.check_refusals(rbt_lib.module(), ctx, which)


@pytest.mark.parametrize("name", sorted(MF.edge_cases()))
@device_guard
def test_edge_clouds(ctx, host, name):
    MF.check_edge(ctx, name, other=host)


@device_guard
def test_the_same_array_twice(ctx):
    MF.check_same_array(ctx)


@pytest.mark.parametrize("k", range(len(pcc_cases.d2_cases())))
@device_guard
def test_d2_is_the_score_bit_for_bit(ctx, k):
    MF.check_d2_determinism(ctx, k)


@pytest.mark.parametrize("which", MF.CALLS)
@device_guard
def test_memory_after_a_call(ctx, which):
    MF.check_memory_after_success(ctx, which)
