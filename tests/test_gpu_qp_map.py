"""GPU build of the QP per CTB (rbt_submit_gof_qp_map, rbt_transcode_gof_qp_map; csrc/rbt_qpmap.h k_enc_qp_fix and the map instantiations of the encoder kernels) through
the C ABI: every case of tests/test_qp_map.py on the device, and every stream identical to the host emulation's - for every map of the decode cases byte for byte; the checks
with many calls run on both contexts at once (Both, tests/test_gpu_frame_qp.py).

Every test runs under a watchdog of its own (faulthandler ends the process when a call does not come back), and a device error ends the run: nothing more is started on a
device that has faulted."""
import faulthandler
import os
import subprocess
import pytest
import rbt_lib
import qp_map_cases as MC
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


@pytest.mark.parametrize("gof,kind", [("128", "geo"), ("64", "attr"), ("96", "geo")])
@device_guard
def test_identity(ctx, host, gof, kind):
    MC.check_identity(rbt_lib.module(), ctx, gof, kind, other=host)


@pytest.mark.parametrize("k", range(len(MC.UNIFORM_CASES)))
@device_guard
def test_uniform_maps(ctx, host, k):
    MC.check_uniform(rbt_lib.module(), ctx, k, other=host)


@pytest.mark.parametrize("k", range(len(MC.DECODE_CASES)))
@device_guard
def test_maps_decode_to_the_reconstruction(ctx, host, k):
    """... and the GPU's bytes are the host emulation's for every map"""
    MC.check_decodes(rbt_lib.module(), ctx, k, same_as=host)


@pytest.mark.parametrize("gof,kind", MC.PLACEMENT_CASES)
@device_guard
def test_map_is_applied_where_it_says(ctx, gof, kind):
    MC.check_placement_premise(gof, kind)
    MC.check_placement(rbt_lib.module(), ctx, gof, kind)


@device_guard
def test_arguments(both):
    MC.check_arguments(rbt_lib.module(), both)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
@device_guard
def test_jobs_in_flight(both, depth, n_jobs):
    MC.check_jobs_in_flight(rbt_lib.module(), both, depth, n_jobs)


@device_guard
def test_two_gofs_in_shared_pipelines(ctx, host):
    MC.check_two_gofs(rbt_lib.module(), ctx, other=host)


@device_guard
def test_map_from_patches(host):
    MC.check_from_patches(rbt_lib.module())
