"""GPU build of the recolouring route (csrc/rbt_color.hip: k_sc_recolor_zero, k_sc_recolor_add, k_sc_color_walk; k_gather_luma on 4:2:0 descriptors) through the C ABI:
every case of tests/test_color_floor.py on the device, and GPU == serial host emulation of the same bodies bit for bit.

Every test runs under a watchdog of its own (faulthandler ends the process when a call does not come back), and a device error ends the run: nothing more is started on a
device that has faulted."""
import faulthandler
import functools
import os
import subprocess
import pytest
import rbt_lib
import color_floor_cases as FC

pytestmark = pytest.mark.gpu
TIMEOUT_S = 120


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(TIMEOUT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def device_guard(f):
    @functools.wraps(f)
    def run(*a, **kw):
        try:
            return f(*a, **kw)
        except rbt_lib.module().RbtError as e:
            if e.code == -1:                                          # RBT_ERR_NO_DEVICE: a HIP error
                pytest.exit("device error in %s: %s" % (f.__name__, e), returncode=3)
            raise
    return run


def make_ctx():
    return rbt_lib.module().Context(device=0)


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


@device_guard
def test_recoloured_cloud_scores_as_a_fresh_upload(ctx, emu):
    FC.check_set_colors(ctx, *FC.crowded_cloud(), other=emu)


@pytest.mark.parametrize("n", FC.SET_SIZES)
@device_guard
def test_recolour_sizes(ctx, emu, n):
    FC.check_set_colors(ctx, *FC.sized_cloud(n), other=emu)


@pytest.mark.parametrize("k", (0, 4))
@device_guard
def test_pair_equals_the_colour_part_of_the_score(ctx, emu, k):
    FC.check_pair(ctx, k, other=emu)


@device_guard
def test_pair_single_point_clouds(ctx, emu):
    FC.check_pair_single_points(ctx, other=emu)


@device_guard
def test_arguments(ctx):
    FC.check_arguments(rbt_lib.module(), ctx, make_ctx)


@pytest.mark.parametrize("n_pics", [1, 3])
@pytest.mark.parametrize("w", FC.GATHER_WIDTHS)
@device_guard
def test_gather_420_equals_slicing(ctx, w, n_pics):
    FC.check_gather(ctx, w, n_pics)


@device_guard
def test_gather_420_feeds_the_upconversion(ctx):
    FC.check_gather_feeds_upconversion(ctx)


@device_guard
def test_gather_420_arguments(ctx):
    FC.check_gather_arguments(rbt_lib.module(), ctx)


# ---- the job. The composition's tables come from the serial host emulation of the same bodies (the parity tests hold the two builds together stream for stream and cloud
# for cloud), so the device runs the jobs only; one case runs the composition itself on the device.
@pytest.mark.parametrize("name", ("synth", "seam_smooth", "cropped"))
@device_guard
def test_job_equals_the_composition(ctx, emu, name):
    FC.check_job_case(rbt_lib.module(), ctx, name, table_ctx=emu)


@device_guard
def test_job_composition_on_the_device(ctx):
    FC.check_job_case(rbt_lib.module(), ctx, "cropped")


@device_guard
def test_job_stats_and_channels(ctx, emu):
    FC.check_stats_and_channels(rbt_lib.module(), ctx, table_ctx=emu)


@device_guard
def test_job_reference_handles(ctx, emu):
    FC.check_reference_handles(rbt_lib.module(), ctx, table_ctx=emu)


@device_guard
def test_job_occupancy_rd(ctx, emu):
    FC.check_occupancy_rd(rbt_lib.module(), ctx, table_ctx=emu)


@device_guard
def test_job_against_independent_arithmetic(ctx):
    FC.check_against_independent_arithmetic(rbt_lib.module(), ctx)


@device_guard
def test_jobs_in_flight(ctx, emu):
    FC.check_jobs_in_flight(rbt_lib.module(), ctx, table_ctx=emu)


@device_guard
def test_job_pairing_and_memory(ctx, emu):
    FC.check_pairing_and_memory(rbt_lib.module(), ctx, table_ctx=emu)


@device_guard
def test_job_determinism(ctx):
    FC.check_determinism(rbt_lib.module(), ctx)


@device_guard
def test_job_arguments(ctx, emu):
    FC.check_job_arguments(rbt_lib.module(), ctx, table_ctx=emu)


@device_guard
def test_more_than_2_21_merged_points(ctx, emu):
    FC.check_merged_limit(rbt_lib.module(), ctx, table_ctx=emu)
