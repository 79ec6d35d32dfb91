"""GPU build of the distortion sums and the job with PSNR floors (csrc/rbt_quality.hip: k_picture_sse; host/rbt_transcode.cpp) through the C ABI: every case of
tests/test_quality.py on the device - sums GPU == serial host emulation of the same body == the NumPy restatement, report-only jobs against the oracle's decoded pictures,
the walk against the oracle's streams, occupied floors with and without occupancy_rd, jobs in flight at depth 4 and 16, two GOFs in shared pipelines, the container.

Every test runs under a watchdog of its own (faulthandler ends the process when a call does not come back), and a device error ends the run: nothing more is started on a
device that has faulted."""
import faulthandler
import functools
import os
import subprocess
import pytest
import rbt_lib
import quality_cases as QC

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


@pytest.mark.parametrize("name", sorted(QC.SSE_CASES))
@device_guard
def test_sums_equal_the_definition_and_the_host_emulation(ctx, host, name):
    QC.check_sse(ctx, name, other=host)


@device_guard
def test_picture_sse_arguments(ctx):
    QC.check_sse_arguments(rbt_lib.module(), ctx)


@pytest.mark.parametrize("w,h,seed", QC.STREAMS)
@pytest.mark.parametrize("kind", sorted(QC.KINDS))
@device_guard
def test_report_only(ctx, w, h, seed, kind):
    QC.check_report(rbt_lib.module(), ctx, w, h, seed, kind)


@device_guard
def test_report_only_compares_the_displayed_area(ctx):
    QC.check_report_cropped(rbt_lib.module(), ctx)


@pytest.mark.parametrize("w,h,seed", QC.STREAMS)
@pytest.mark.parametrize("kind", sorted(QC.KINDS))
@device_guard
def test_walk(ctx, w, h, seed, kind):
    QC.check_walk(rbt_lib.module(), ctx, w, h, seed, kind)


@device_guard
def test_walk_where_the_distortion_is_not_monotone(ctx):
    QC.check_not_monotone(rbt_lib.module(), ctx)


@pytest.mark.parametrize("rd", [0, 1])
@device_guard
def test_occupied_floor(ctx, rd):
    QC.check_occupancy(rbt_lib.module(), ctx, rd)


@device_guard
def test_jobs(ctx):
    QC.check_jobs(rbt_lib.module(), ctx)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
@device_guard
def test_jobs_in_flight(ctx, depth, n_jobs):
    QC.check_jobs_in_flight(rbt_lib.module(), ctx, depth, n_jobs)


@pytest.mark.parametrize("depth", [1, 3])
@device_guard
def test_two_gofs_in_shared_pipelines(ctx, depth):
    QC.check_shared_pipelines(rbt_lib.module(), ctx, depth)


@device_guard
def test_verify_md5(ctx):
    QC.check_verify_md5(rbt_lib.module(), ctx)


@device_guard
def test_arguments(ctx):
    QC.check_arguments(rbt_lib.module(), ctx)


@device_guard
def test_container(ctx):
    QC.check_container(rbt_lib.module(), ctx)
