"""GPU build of the luma gather and of the job with D1 floors (csrc/rbt_cloudmaps.hip: k_gather_luma; host/rbt_pcc.cpp, host/rbt_transcode.cpp) through the C ABI: every
case of tests/test_d1_floor.py on the device - the gather GPU == serial host emulation of the same body == NumPy slicing, the walk against the oracle's streams, clouds and
D1 figures, smoothing and several frames, padded pictures, reference handles, composition through the public calls, jobs in flight at depth 4 and 16, the refusals.

Every test runs under a watchdog of its own (faulthandler ends the process when a call does not come back), and a device error ends the run: nothing more is started on a
device that has faulted."""
import faulthandler
import functools
import os
import subprocess
import pytest
import rbt_lib
import d1_floor_cases as DC

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


@pytest.mark.parametrize("n_pics", [1, 3])
@pytest.mark.parametrize("w", DC.GATHER_WIDTHS)
@device_guard
def test_gather_equals_slicing_and_the_host_emulation(ctx, host, w, n_pics):
    DC.check_gather(ctx, w, n_pics, other=host)


@device_guard
def test_gather_arguments(ctx):
    DC.check_gather_arguments(rbt_lib.module(), ctx)


@pytest.mark.parametrize("rd", [0, 1])
@device_guard
def test_walk(ctx, rd):
    DC.check_walk(rbt_lib.module(), ctx, rd)


@device_guard
def test_walk_where_d1_is_not_monotone(ctx):
    DC.check_not_monotone(rbt_lib.module(), ctx)


@device_guard
def test_smoothing_and_several_frames(ctx):
    DC.check_smoothing_frames(rbt_lib.module(), ctx)


@device_guard
def test_strides_and_windows(ctx):
    DC.check_cropped(rbt_lib.module(), ctx)


@device_guard
def test_reference_handles(ctx):
    DC.check_reference_handles(rbt_lib.module(), ctx)


@device_guard
def test_composition_through_the_public_calls(ctx):
    DC.check_composition(rbt_lib.module(), ctx)


@device_guard
def test_jobs(ctx):
    DC.check_jobs(rbt_lib.module(), ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
@device_guard
def test_jobs_in_flight(ctx, depth, n_jobs):
    DC.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


@device_guard
def test_arguments(ctx):
    DC.check_arguments(rbt_lib.module(), ctx)


@device_guard
def test_determinism(ctx):
    DC.check_determinism(rbt_lib.module(), ctx)
