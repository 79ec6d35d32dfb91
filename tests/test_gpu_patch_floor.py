"""GPU build of the PSNR floors held patch by patch (csrc/rbt_quality.hip: k_ctb_sse, k_patch_fold; host/rbt_transcode.cpp: rbt_ctb_sse, rbt_submit_gof_quality_patches) through
the C ABI: every case of tests/test_patch_floor.py on the device, and every word, stream and result identical to the host emulation's; the checks with many calls run on
both contexts at once (Both, tests/test_gpu_frame_qp.py).

Every test runs under a watchdog of its own (faulthandler ends the process when a call does not come back), and a device error ends the run: nothing more is started on a
device that has faulted."""
import faulthandler
import os
import subprocess
import pytest
import rbt_lib
import patch_floor_cases as PC
from test_gpu_frame_qp import Both, device_guard

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


@pytest.fixture(scope="module")
def both(ctx, host):
    return Both(ctx, host)


@pytest.mark.parametrize("name", sorted(PC.SUM_CASES))
@device_guard
def test_sums_equal_the_definition(ctx, host, name):
    PC.check_sums(ctx, name, other=host)


@device_guard
def test_ctb_sse_arguments(both):
    PC.check_sums_arguments(rbt_lib.module(), both)


@pytest.mark.parametrize("k", range(len(PC.REPORT_CASES)))
@device_guard
def test_report_only(ctx, host, k):
    PC.check_report(rbt_lib.module(), ctx, k, other=host)


@device_guard
def test_walk_moves_patches_both_ways(ctx, host):
    PC.check_main_premise()
    PC.check_main_walk(rbt_lib.module(), ctx, other=host)


@pytest.mark.parametrize("k", range(len(PC.REPLAY_CASES)))
@device_guard
def test_walk_is_the_replay(ctx, host, k):
    PC.check_replay(rbt_lib.module(), ctx, k, other=host)


@device_guard
def test_edges_of_the_walk(ctx, host):
    PC.check_edges(rbt_lib.module(), ctx, other=host)


@device_guard
def test_arguments(both):
    PC.check_arguments(rbt_lib.module(), both)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
@device_guard
def test_jobs_in_flight(both, depth, n_jobs):
    PC.check_jobs_in_flight(rbt_lib.module(), both, depth, n_jobs)


@device_guard
def test_two_gofs_in_shared_pipelines(ctx, host):
    PC.check_two_gofs(rbt_lib.module(), ctx, other=host)
