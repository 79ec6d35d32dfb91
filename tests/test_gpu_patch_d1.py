"""GPU build of D1 per patch of the decoded cloud (csrc/rbt_color.hip: k_pd_labels, k_pd_check, k_pd_sums; host/rbt_pcc.cpp: rbt_pcloud_set_labels, rbt_pcloud_labels,
rbt_score_patches) through the C ABI: every case of tests/test_patch_d1.py on the device, and every word and label identical to the host emulation's.

Every test runs under a watchdog of its own (faulthandler ends the process when a call does not come back), and a device error ends the run: nothing more is started on a
device that has faulted."""
import faulthandler
import os
import subprocess
import pytest
import rbt_lib
import patch_d1_cases as PD
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


@pytest.mark.parametrize("name", sorted(PD.SUM_CASES))
@device_guard
def test_sums_equal_the_definition(ctx, host, name):
    PD.check_sums(ctx, name, other=host)


@device_guard
def test_two_calls_return_the_same_words(ctx):
    PD.check_determinism(ctx)


@device_guard
def test_arguments(ctx):
    PD.check_score_arguments(rbt_lib.module(), ctx, make_ctx)


@pytest.mark.parametrize("name", PD.LABEL_CASES)
@device_guard
def test_labels_of_a_cloud_made_from_maps(ctx, host, name):
    PD.check_labels(rbt_lib.module(), ctx, name, other=host)


@device_guard
def test_a_cloud_made_from_maps_scores_with_its_labels(ctx, host):
    PD.check_labels_score(rbt_lib.module(), ctx, other=host)


@device_guard
def test_frame_without_patches(ctx):
    PD.check_no_patches(rbt_lib.module(), ctx)


# ---- D1 floors held patch by patch (rbt_submit_gof_d1_patches) ----
@pytest.mark.parametrize("k", range(len(PD.REPORT_CASES)))
@device_guard
def test_report_only(ctx, host, k):
    PD.check_report(rbt_lib.module(), ctx, k, other=host)


@device_guard
def test_walk_moves_patches_both_ways(ctx, host):
    """(seam128, QP 30, CTBs of 32): the premise on the oracle alone, then the replay, then a patch below and one above q0 in every frame"""
    PD.check_main_premise()
    PD.check_main_walk(rbt_lib.module(), ctx, other=host)


@pytest.mark.parametrize("k", range(PD.N_REPLAY))
@device_guard
def test_walk_is_the_replay(ctx, host, k):
    PD.check_replay(rbt_lib.module(), ctx, k, other=host)


@device_guard
def test_edges_of_the_walk(ctx, host):
    PD.check_edges(rbt_lib.module(), ctx, other=host)


@device_guard
def test_job_arguments(ctx):
    PD.check_job_arguments(rbt_lib.module(), ctx, make_ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
@device_guard
def test_jobs_in_flight(ctx, depth, n_jobs):
    PD.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


@device_guard
def test_two_gofs_in_shared_pipelines(ctx, host):
    PD.check_two_gofs(rbt_lib.module(), ctx, other=host)


@device_guard
def test_nothing_leaks_between_kinds_of_job(ctx):
    PD.check_no_leak_between_kinds(rbt_lib.module(), ctx)
