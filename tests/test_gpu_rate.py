"""GPU build of the level census and the rate-targeted job (csrc/rbt_rate.hip: k_level_census; host/rbt_transcode.cpp) through the C ABI: every case of
tests/test_rate.py on the device - census GPU == serial host emulation of the same body == the NumPy restatement, histograms of decoded streams identical between the two
builds, the walk against the oracle's streams, jobs in flight at depth 4 and 16.

Every test runs under a watchdog of its own (faulthandler ends the process when a call does not come back), and a device error ends the run: nothing more is started on a
device that has faulted."""
import faulthandler
import functools
import os
import subprocess
import pytest
import rbt_lib
import rate_cases as RC

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


@pytest.mark.parametrize("name", sorted(RC.CENSUS_CASES))
@device_guard
def test_census_equals_the_definition_and_the_host_emulation(ctx, host, name):
    RC.check_census(ctx, name, other=host)


@pytest.mark.parametrize("w,h,seed", RC.STREAMS)
@pytest.mark.parametrize("kind", sorted(RC.KINDS))
@device_guard
def test_estimate_is_the_formula_and_the_host_emulations_histograms(ctx, w, h, seed, kind):
    RC.check_estimate(ctx, w, h, seed, kind, against_host=True)


@pytest.mark.parametrize("w,h,seed", RC.STREAMS)
@pytest.mark.parametrize("kind", sorted(RC.KINDS))
@device_guard
def test_walk(ctx, w, h, seed, kind):
    RC.check_walk(rbt_lib.module(), ctx, w, h, seed, kind)


@device_guard
def test_walk_across_the_plateau(ctx):
    RC.check_plateau(rbt_lib.module(), ctx)


@pytest.mark.parametrize("k", range(len(RC.VARIANTS)))
@device_guard
def test_walk_variants(ctx, k):
    RC.check_variant(rbt_lib.module(), ctx, k)


@device_guard
def test_mixed_job(ctx):
    RC.check_mixed_job(rbt_lib.module(), ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
@device_guard
def test_jobs_in_flight(ctx, depth, n_jobs):
    RC.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


@device_guard
def test_verify_md5(ctx):
    RC.check_verify_md5(rbt_lib.module(), ctx)


@device_guard
def test_arguments(ctx):
    RC.check_arguments(rbt_lib.module(), ctx)


@device_guard
def test_container(ctx):
    RC.check_container(rbt_lib.module(), ctx)
