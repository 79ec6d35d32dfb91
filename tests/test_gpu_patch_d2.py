"""GPU build of D2 per patch of the decoded cloud (csrc/rbt_color.hip: k_p2_block, k_p2_cols, k_p2_fold; host/rbt_pcc.cpp: rbt_score_patches_d2) and of the D2 floors on
the stream and patch by patch, through the C ABI: every case of tests/test_patch_d2.py on the device, and every field identical to the host emulation's, bit for bit.

Every test runs under a watchdog of its own (faulthandler ends the process when a call does not come back), and a device error ends the run: nothing more is started on a
device that has faulted."""
import faulthandler
import os
import subprocess
import pytest
import rbt_lib
import patch_d2_cases as P2
from test_gpu_frame_qp import device_guard

pytestmark = pytest.mark.gpu
TIMEOUT_S = 120


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(TIMEOUT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def make_ctx():
    return rbt_lib.module().Context(device=0)


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(P2.SUM_CASES))
@device_guard
def test_sums_equal_the_definition(ctx, host, name):
    P2.check_sums(ctx, name, other=host)


@device_guard
def test_a_second_block_in_a_column(ctx, host):
    P2.check_large(ctx, other=host)


@device_guard
def test_two_calls_return_the_same_bits(ctx):
    P2.check_determinism(ctx)


@device_guard
def test_arguments(ctx):
    P2.check_score_arguments(rbt_lib.module(), ctx, make_ctx)


# ---- the jobs ----
@pytest.mark.parametrize("handles", [True, False])
@device_guard
def test_stream_report(ctx, host, handles):
    P2.check_stream_report(rbt_lib.module(), ctx, handles, other=host)


@pytest.mark.parametrize("handles,stat", [(True, 0), (False, 1)])
@device_guard
def test_stream_walk(ctx, host, handles, stat):
    P2.check_stream_walk(rbt_lib.module(), ctx, handles, other=host, stat=stat)


@pytest.mark.parametrize("handles", [True, False])
@device_guard
def test_patch_report(ctx, host, handles):
    P2.check_patch_report(rbt_lib.module(), ctx, handles, other=host)


@pytest.mark.parametrize("handles", [True, False])
@device_guard
def test_patch_walk_moves_patches_both_ways(ctx, host, handles):
    P2.check_patch_walk(rbt_lib.module(), ctx, handles, other=host)


@device_guard
def test_normals_parameters_reach_the_estimation(ctx):
    P2.check_normals_params(rbt_lib.module(), ctx)


@device_guard
def test_job_arguments(ctx):
    P2.check_job_arguments(rbt_lib.module(), ctx, make_ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
@device_guard
def test_jobs_in_flight(ctx, depth, n_jobs):
    P2.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


@device_guard
def test_nothing_leaks_between_d1_and_d2_jobs(ctx):
    P2.check_no_leak_between_kinds(rbt_lib.module(), ctx)
