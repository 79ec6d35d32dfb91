"""GPU build of the attribute transfer after geometry smoothing (csrc/rbt_color.hip: k_tc_*) through the C ABI: every case of tests/test_attr_transfer.py on the
device against the brute-force restatement (tests/attr_transfer_cases.py), GPU == serial host emulation of the same bodies on every case, and one full-size frame.

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
import pcc_cases

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
    R = rbt_lib.module()
    c = R.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    R = rbt_lib.module()
    c = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


@pytest.mark.parametrize("seed", range(3))
@device_guard
def test_stage_equals_the_restatement(ctx, seed):
    AT.check_surface(ctx, seed)


@device_guard
def test_tie_rules_and_volume_faces(ctx):
    AT.check_tie_rules(ctx)


@device_guard
def test_known_answers(ctx):
    AT.check_known_answers(ctx)


@device_guard
def test_arguments(ctx):
    AT.check_arguments(ctx, rbt_lib.module())


@device_guard
def test_stage_equals_host_emulation(ctx, emu):
    """every stand-alone case: colours and n_changed of the GPU == the host emulation's"""
    cases = [AT.surface_case(0, n=6000, side=57), AT.surface_case(1, "random"), AT.surface_case(5, doubled=True), AT.tie_case(), AT.faces_case(), AT.known_forward_case(),
             AT.known_backward_case()]
    for case in cases:
        got, want = ctx.transfer_colors(*case), emu.transfer_colors(*case)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]


@pytest.mark.parametrize("seed,two_axes", AT.CHAINED)
@device_guard
def test_reconstruct_decoded_on_seam_atlases(ctx, emu, seed, two_axes):
    R = rbt_lib.module()
    case = AT.chained_case(R, seed, two_axes)
    got, n_changed = AT.check_chained(ctx, R, case)
    assert all(np.array_equal(a, b) for a, b in zip(got, emu.reconstruct_decoded(*case))) and n_changed == emu.n_changed


@device_guard
def test_reconstruct_decoded_with_smooth_attributes(ctx, emu):
    R = rbt_lib.module()
    case = AT.ramp_atlas(R, 0)
    got, n_changed = AT.check_chained(ctx, R, case, lists=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, emu.reconstruct_decoded(*case))) and n_changed == emu.n_changed


@device_guard
def test_other_filter_types_are_refused(ctx):
    AT.check_chained_unsupported(ctx, rbt_lib.module())


@device_guard
def test_full_size_frame_equals_host_emulation(ctx, emu):
    """40 x 40 tiles at 1280 x 1280 (the patches folded back into the 1024^3 volume as tests/test_gpu_pcc.py does), with plateau attributes in one half so that both the
    forward path and the lists are exercised at size: all six arrays and n_changed == the host emulation's; stage time printed"""
    R = rbt_lib.module()
    case = list(pcc_cases.seam_atlas(R, 9, tiles=40, two_axes=True))
    for k, p in enumerate(case[1]): p.u1 = 40 + 28 * (k % 30); p.v1 = 40 + 28 * ((k // 30) % 30); p.d1 = 30 + 200 * (k // 900)
    w = case[0].width
    ramp = AT.ramp_atlas(R, 0)[6]                                    # a 96 x 96 plateau picture: tile it over the upper half of the luma plane and of both chroma planes
    for f in (6, 7):
        pic = case[f].copy()
        y = pic[: w * w].reshape(w, w); y[: w // 2] = np.tile(ramp[: 96 * 96].reshape(96, 96), (w // 96 + 1, w // 96 + 1))[: w // 2, :w]
        c = pic[w * w:].reshape(2, w // 2, w // 2); c[0, : w // 4] = 500; c[1, : w // 4] = 520
        case[f] = pic
    got = ctx.reconstruct_decoded(*case)
    n_sm, n_ch, ms = ctx.n_smoothed, ctx.n_changed, ctx.color_stage_ms()["transfer"]
    print("points %d, moved %d, changed %d, transfer stage %.3f ms" % (len(got[0]), n_sm, n_ch, ms))
    assert len(got[0]) > 1000000 and n_sm > 1000 and int(got[5].sum()) == n_sm and 0 < n_ch <= n_sm and ms > 0
    want = emu.reconstruct_decoded(*case)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and n_ch == emu.n_changed
    base = ctx.reconstruct_rgb(*case)
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1][got[5] == 0], base[1][got[5] == 0]) and (got[1][got[5] == 1] != base[1][got[5] == 1]).any()
