"""GPU build of the colour PSNR per patch of the decoded cloud (csrc/rbt_color.hip: k_pc_sums; host/rbt_pcc.cpp: rbt_score_patches_color,
rbt_score_pair_patches_color) and of the colour floors held patch by patch, through the C ABI: every case of tests/test_patch_color.py on the device, and every field
identical to the host emulation's, bit for bit.

Every test runs under a watchdog of its own (faulthandler ends the process when a call does not come back), and a device error ends the run: nothing more is started on a
device that has faulted."""
import faulthandler
import os
import subprocess
import pytest
import rbt_lib
import patch_color_cases as PC
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


@pytest.mark.parametrize("name", sorted(PC.SUM_CASES))
@device_guard
def test_sums_equal_the_definition(ctx, host, name):
    PC.check_sums(ctx, name, other=host)


@device_guard
def test_pair_equals_the_cloud_call_before_and_after_new_colours(ctx, host):
    PC.check_pair(ctx, other=host)


@device_guard
def test_two_calls_return_the_same_bits(ctx):
    PC.check_determinism(ctx)


@device_guard
def test_arguments(ctx):
    PC.check_score_arguments(rbt_lib.module(), ctx, make_ctx)


@device_guard
def test_merged_limit(ctx):
    PC.check_merged_limit(rbt_lib.module(), ctx)


# ---- the job ----
@pytest.mark.parametrize("handles", [True, False])
@device_guard
def test_report(ctx, host, handles):
    PC.check_report(rbt_lib.module(), ctx, handles, other=host)


@pytest.mark.parametrize("handles,channel", [(True, 0), (False, 1), (True, 2)])
@device_guard
def test_walk_moves_patches_both_ways(ctx, host, handles, channel):
    PC.check_walk(rbt_lib.module(), ctx, handles, channel, other=host)


@device_guard
def test_max_trials_caps_the_walk(ctx, host):
    PC.check_walk(rbt_lib.module(), ctx, False, 0, other=host, max_trials=2)


@device_guard
def test_job_arguments(ctx):
    PC.check_job_arguments(rbt_lib.module(), ctx, make_ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
@device_guard
def test_jobs_in_flight(ctx, depth, n_jobs):
    PC.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


@device_guard
def test_nothing_leaks_between_job_kinds(ctx):
    PC.check_no_leak_between_kinds(rbt_lib.module(), ctx)
