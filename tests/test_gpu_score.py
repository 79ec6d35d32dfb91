"""GPU build of the frame scoring on device clouds (csrc/rbt_color.hip: k_sc_*) through the C ABI: every case of tests/test_score.py on the device against the brute-force
restatements (tests/score_cases.py), GPU == serial host emulation of the same bodies on every case bit for bit (the D2 sums included), and one full-size frame.

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
import metric_fold_cases as MF
import oracle_lib as O
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


@pytest.mark.parametrize("k", range(6))
@device_guard
def test_equals_the_definition(ctx, emu, k):
    SC.check_base(ctx, k, emu)


@pytest.mark.parametrize("name", sorted(SC.boundary_cases()))
@device_guard
def test_word_boundaries_and_faces(ctx, emu, name):
    SC.check_boundary(ctx, name, emu)


@pytest.mark.parametrize("name", SC.FAR)
@device_guard
def test_far_neighbours(ctx, emu, name):
    SC.check_far(ctx, name, emu)


@pytest.mark.parametrize("n,side", SC.SIZES)
@device_guard
def test_sizes(ctx, emu, n, side):
    SC.check_size(ctx, n, side, emu)


@device_guard
def test_degenerate_clouds(ctx, emu):
    SC.check_degenerate(ctx, emu)


@device_guard
def test_two_calls_give_the_same_bytes(ctx):
    SC.check_determinism(ctx)


@device_guard
def test_handles(ctx):
    SC.check_handles(rbt_lib.module(), make_ctx)


@device_guard
def test_arguments(ctx):
    SC.check_arguments(rbt_lib.module(), ctx, make_ctx)


@pytest.mark.parametrize("seed,two_axes", AT.CHAINED)
@device_guard
def test_from_maps_on_seam_atlases(ctx, emu, seed, two_axes):
    R = rbt_lib.module()
    SC.check_from_maps(R, ctx, AT.chained_case(R, seed, two_axes), other=emu)


@device_guard
def test_from_maps_with_smooth_attributes(ctx, emu):
    R = rbt_lib.module()
    SC.check_from_maps(R, ctx, AT.ramp_atlas(R, 0), other=emu)


@pytest.mark.parametrize("tiles", (40, 36))
@device_guard
def test_full_size_frame(ctx, tiles):
    """the 1280 x 1280 seam atlas of tests/test_gpu_attr_transfer.py (40 x 40 tiles, 2 173 375 points) through rbt_pcloud_from_maps, scored against the same atlas without
    smoothing: D1 == rbt_d1 on the host copies and == the oracle's D1 exactly, D2 == rbt_d2 field for field; device time printed. That cloud has more than 2^21 merged
    points, where rbt_color_metric refuses (its 64-bit sums are exact up to there): the clouds then do not allow the colour part, and asking for it is refused alike. The
    colour part at size runs on the same atlas cut to 36 x 36 tiles (1152 x 1152, more than a million points, below the limit): all three parts, colour == rbt_color_metric
    exactly."""
    R = rbt_lib.module()
    case = list(pcc_cases.seam_atlas(R, 9, tiles=tiles, two_axes=True))
    for k, p in enumerate(case[1]): p.u1 = 40 + 28 * (k % 30); p.v1 = 40 + 28 * ((k // 30) % 30); p.d1 = 30 + 200 * (k // 900)
    h, host = ctx.pcloud_from_maps(*case, host_copy=True)
    sx, srgb, sn = SC.seam_source(R, ctx, case, tiles)
    hs = ctx.pcloud_upload(sx, srgb, sn)
    try:
        got = ctx.score(hs, h)
        if tiles == 40: SC.refused(R, lambda: ctx.score(hs, h, parts=SC.COLOR))
    finally:
        h.release(); hs.release()
    print("points %d / %d, merged %d / %d, parts %d, device_ms %.3f" % (got["n_points_a"], got["n_points_b"], got["n_merged_a"], got["n_merged_b"], got["parts"], got["device_ms"]))
    assert got["n_points_b"] == len(host[0]) > 1000000 and got["device_ms"] > 0 and got["d1"]["sse_ab"] > 0
    want = O.d1(sx, host[0])                                           # a third party: rbt_d1 and rbt_score are two routes through the same kernels (the oracle takes 1.3 s here)
    for k in ("n_a", "n_b", "sse_ab", "sse_ba", "max_ab", "max_ba"): assert got["d1"][k] == want[k], (k, got["d1"][k], want[k])
    if tiles == 40:
        assert got["parts"] == SC.D1 | SC.D2 and got["n_merged_b"] > 1 << 21
        MF.refused_with(R, ctx, lambda: ctx.color_metric(sx, srgb, host[0], host[4]), MF.MERGED)      # RBT_ERR_PARAM as before, in rbt_color_metric's own words, not the score's
        SC.check_against_host_array_calls(ctx, got, (sx, srgb, sn, host[0], host[4]), colour=False)
    else:
        assert got["parts"] == 7
        SC.check_against_host_array_calls(ctx, got, (sx, srgb, sn, host[0], host[4]))
