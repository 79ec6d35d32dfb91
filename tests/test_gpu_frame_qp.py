"""GPU build of the QP list per point-cloud frame (rbt_submit_gof_frame_qp, rbt_transcode_gof_frame_qp) through the C ABI: every case of tests/test_frame_qp.py on the
device, and every stream and result identical to the host emulation's: the checks with many calls run on both contexts at once (Both).

Every test runs under a watchdog of its own (faulthandler ends the process when a call does not come back), and a device error ends the run: nothing more is started on a
device that has faulted."""
import faulthandler
import functools
import os
import subprocess
import pytest
import rbt_lib
import frame_qp_cases as FC

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


class Both:
    """the GPU context and the host emulation behind one face: every call goes to both, and both must answer alike - the same streams and results, or the same error code.
    What a check does with the answers is then done with the GPU's. (Times, and the bytes a job holds, are each context's own.)"""
    OWN = ("get_depth", "set_depth", "job_memory", "close")

    def __init__(self, gpu, host):
        self.gpu, self.host = gpu, host

    @staticmethod
    def _plain(x):
        if isinstance(x, dict):
            return {k: (0.0 if k == "cloud_ms" else Both._plain(v)) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return [Both._plain(v) for v in x]
        return x.tolist() if hasattr(x, "tolist") else x

    def __getattr__(self, name):
        fg, fh = getattr(self.gpu, name), getattr(self.host, name)
        E = rbt_lib.module().RbtError

        def call(*a, **kw):
            ag = [x[1] if isinstance(x, tuple) and x and x[0] == "both" else x for x in a]
            ah = [x[2] if isinstance(x, tuple) and x and x[0] == "both" else x for x in a]
            try:
                rg = fg(*ag, **kw)
            except E as e:
                with pytest.raises(E) as eh:
                    fh(*ah, **kw)
                assert eh.value.code == e.code, (name, e, eh.value)
                raise
            rh = fh(*ah, **kw)
            if name.startswith("submit_"):
                return ("both", rg, rh)
            if name not in Both.OWN:
                assert Both._plain(rg) == Both._plain(rh), name
            return rg
        return call


@pytest.fixture(scope="module")
def both(ctx, host):
    return Both(ctx, host)


@pytest.mark.parametrize("gof", FC.LIST_GOFS)
@pytest.mark.parametrize("kind", sorted(FC.KINDS))
@device_guard
def test_identity(ctx, host, gof, kind):
    FC.check_identity(rbt_lib.module(), ctx, gof, kind, other=host)


@pytest.mark.parametrize("gof", FC.LIST_GOFS)
@pytest.mark.parametrize("kind", sorted(FC.KINDS))
@device_guard
def test_lists_compose_frame_by_frame(ctx, host, gof, kind):
    FC.check_lists(rbt_lib.module(), ctx, gof, kind, other=host)


@pytest.mark.parametrize("k", range(len(FC.VARIANTS)))
@device_guard
def test_variants(ctx, host, k):
    FC.check_variant(rbt_lib.module(), ctx, k, other=host)


@device_guard
def test_verify_md5(both):
    FC.check_verify_md5(rbt_lib.module(), both)


@device_guard
def test_arguments(both):
    FC.check_arguments(rbt_lib.module(), both)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16)])
@device_guard
def test_jobs_in_flight(both, depth, n_jobs):
    FC.check_jobs_in_flight(rbt_lib.module(), both, depth, n_jobs)


@device_guard
def test_two_gofs_in_shared_pipelines(ctx, host):
    FC.check_two_gofs(rbt_lib.module(), ctx, other=host)


# ---- floors held frame by frame (rbt_submit_gof_quality_frames)
@pytest.mark.parametrize("gof", FC.LIST_GOFS)
@pytest.mark.parametrize("kind", sorted(FC.KINDS))
@device_guard
def test_frame_floors(ctx, host, gof, kind):
    FC.check_frame_floors(rbt_lib.module(), ctx, gof, kind, other=host)


@pytest.mark.parametrize("rd,region", [(0, FC.ALL), (1, FC.ALL), (0, FC.OCCUPIED), (1, FC.OCCUPIED)])
@device_guard
def test_passes_over_a_subset_of_the_frames(ctx, host, rd, region):
    FC.check_subset_passes(rbt_lib.module(), ctx, rd, region, other=host)


@pytest.mark.parametrize("depth,n_jobs", [(4, 4), (16, 16), (5, 3)])
@device_guard
def test_floor_jobs_in_flight(both, depth, n_jobs):
    FC.check_floor_jobs_in_flight(rbt_lib.module(), both, depth, n_jobs)


@device_guard
def test_floor_two_gofs_in_shared_pipelines(ctx, host):
    FC.check_floor_two_gofs(rbt_lib.module(), ctx, other=host)


@device_guard
def test_floor_arguments(both):
    FC.check_floor_arguments(rbt_lib.module(), both)


@device_guard
def test_floor_container(both):
    FC.check_floor_container(rbt_lib.module(), both)


@pytest.mark.parametrize("k", range(len(FC.FLOOR_VARIANTS)))
@device_guard
def test_floor_variants(ctx, host, k):
    FC.check_floor_variant(rbt_lib.module(), ctx, k, other=host)


# ---- D1 floors frame by frame (rbt_submit_gof_d1_frames)
@pytest.mark.parametrize("rd", [0, 1])
@device_guard
def test_d1_frame_floors(ctx, host, rd):
    FC.check_d1_frames(rbt_lib.module(), ctx, rd, other=host)


@device_guard
def test_d1_frame_arguments(both):
    FC.check_d1_arguments(rbt_lib.module(), both)
