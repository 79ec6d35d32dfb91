"""GPU build of the normal estimation (csrc/rbt_normals.hip: k_nm_*) through the C ABI: every case of tests/test_normals.py on the device against the brute-force
restatement (tests/normals_cases.py), GPU == serial host emulation of the same bodies on every case bit for bit, and one full-size frame.

Every test runs under a watchdog of its own (faulthandler ends the process when a call does not come back), and a device error ends the run: nothing more is started on a
device that has faulted."""
import faulthandler
import functools
import os
import subprocess
import numpy as np
import pytest
import rbt_lib
import attr_transfer_cases as AT
import normals_cases as NC
import pcc_cases
import score_cases as SC

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


@pytest.mark.parametrize("name", sorted(NC.CLOUDS))
@device_guard
def test_equals_the_definition(ctx, emu, name):
    NC.check_cloud(rbt_lib.module(), ctx, name, emu)


@device_guard
def test_isotropic_cube(ctx, emu):
    NC.check_isotropic_cube(rbt_lib.module(), ctx, emu)


@device_guard
def test_view_point_inside_the_sphere(ctx, emu):
    NC.check_view_point_inside(rbt_lib.module(), ctx, emu)


@device_guard
def test_other_k(ctx, emu):
    NC.check_other_k(rbt_lib.module(), ctx, emu)


@device_guard
def test_order_and_duplicates(ctx):
    NC.check_order_and_duplicates(rbt_lib.module(), ctx)


@device_guard
def test_estimated_normals_allow_d2(ctx, emu):
    NC.check_scoring(rbt_lib.module(), ctx, emu)


@pytest.mark.parametrize("seed,two_axes", AT.CHAINED)
@device_guard
def test_estimated_normals_on_a_cloud_from_maps(ctx, emu, seed, two_axes):
    R = rbt_lib.module()
    NC.check_scoring_from_maps(R, ctx, AT.chained_case(R, seed, two_axes), emu)


@device_guard
def test_arguments(ctx):
    NC.check_arguments(rbt_lib.module(), ctx, make_ctx)


@device_guard
def test_full_size_frame(ctx):
    """the 36-tile seam atlas of test_gpu_score.py::test_full_size_frame through rbt_pcloud_from_maps, more than a million points: device_ms printed, with the device time
    of rbt_score (all three parts) on the same frame beside it; the length and sign rules on all points; 200 seeded sample points against the restatement restricted to the
    box +-8 around each, which is exact as long as the sample's k-th squared distance is <= 64 (asserted); at most 1 % of the samples under the eigen-gap."""
    R = rbt_lib.module()
    case = list(pcc_cases.seam_atlas(R, 9, tiles=36, two_axes=True))
    for k, p in enumerate(case[1]): p.u1 = 40 + 28 * (k % 30); p.v1 = 40 + 28 * ((k // 30) % 30); p.d1 = 30 + 200 * (k // 900)
    h, host = ctx.pcloud_from_maps(*case, host_copy=True)
    hs = ctx.pcloud_upload(*SC.seam_source(R, ctx, case, 36))
    try:
        q, ms = h.estimate_normals()
        n, merged = h.points()
        score_ms = ctx.score(hs, h)["device_ms"]
    finally:
        h.release(); hs.release()
    xyz = host[0]
    print("points %d, merged %d, estimate device_ms %.3f, rbt_score device_ms %.3f" % (n, merged, ms, score_ms))
    assert n == len(xyz) > 1000000 and ms > 0
    NC.check_length(q); NC.check_sign(xyz, q)
    pick = np.random.default_rng(3).choice(len(xyz), 200, replace=False)
    p64 = xyz.astype(np.int64)
    order = np.argsort(p64[:, 0], kind="stable"); xs = p64[order, 0]
    worst = skipped = 0
    for i in pick:
        c = p64[i]
        cand = order[np.searchsorted(xs, c[0] - 8):np.searchsorted(xs, c[0] + 8, side="right")]
        box = p64[cand][(np.abs(p64[cand] - c) <= 8).all(1)]
        ref = NC.restatement(box, 16, queries=c[None])
        assert ref["m"] == 16 and ref["kth"][0] <= 64, ref["kth"]
        if ref["gap"][0] < NC.GAP: skipped += 1; continue
        want = np.round(16384 * ref["v"][0]).astype(np.int64); got = q[i].astype(np.int64)
        err = min(np.abs(got - want).max(), np.abs(got + want).max()); worst = max(worst, err)
        assert err <= 1, (i, got, want)
    print("largest difference to eigh over the samples in LSB:", worst, "- samples under the gap:", skipped)
    assert skipped <= 2
