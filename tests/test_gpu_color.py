"""GPU build of the colour stages (csrc/rbt_color.hip: k_up444, k_yuv16_rgb8, and the k_sc_* kernels behind rbt_color_metric) through the C ABI: every case of
tests/test_color.py on the device, full-size inputs against the serial host emulation of the same bodies (arrays and integers equal), and point-cloud frame 0 of the
benchmark fixture after a real R5 -> R3 transcode."""
import json
import os
import subprocess
import numpy as np
import pytest
import oracle_lib as O
import rbt_lib
import color_cases as CC
import pcc_cases
import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


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


def test_up_conversion_equals_the_restatement(ctx):
    CC.check_up(ctx, rbt_lib.module())


def test_up_conversion_known_answers(ctx):
    CC.check_up_known_answers(ctx, rbt_lib.module())


def test_up_conversion_bad_arguments(ctx):
    CC.check_up_bad_arguments(ctx, rbt_lib.module())


def test_up_conversion_of_a_full_size_pair_equals_restatement_and_host_emulation(ctx, emu):
    """one 1280x1280 frame pair: GPU == float32 / float64 restatement == host emulation, for the filter and for the replication"""
    R = rbt_lib.module()
    f, got = CC.check_up_large(ctx)
    assert np.array_equal(got, emu.yuv420_to_yuv444(f, 1280, 1280, 10))
    f8 = CC.up_pictures(1280, 1280, 8, 98)
    assert np.array_equal(ctx.yuv420_to_yuv444(f8, 1280, 1280, 8), emu.yuv420_to_yuv444(f8, 1280, 1280, 8))
    assert np.array_equal(ctx.yuv420_to_yuv444(f, 1280, 1280, 10, R.RBT_UPSAMPLE_REPLICATE), emu.yuv420_to_yuv444(f, 1280, 1280, 10, R.RBT_UPSAMPLE_REPLICATE))


def test_rgb_equals_the_restatement(ctx, emu):
    CC.check_rgb(ctx)
    x = CC.rgb_inputs()
    assert np.array_equal(ctx.yuv16_to_rgb8(x), emu.yuv16_to_rgb8(x))


@pytest.mark.parametrize("seed", range(8))
def test_reconstruct_rgb_on_random_atlases(ctx, seed):
    R = rbt_lib.module()
    CC.check_reconstruct_rgb(ctx, R, pcc_cases.random_atlas(R, seed, *((1280, 1280) if seed == 7 else (None, None))), O.reconstruct)


def test_reconstruct_rgb_known_answer(ctx):
    CC.check_reconstruct_rgb_known_answer(ctx, rbt_lib.module())


def test_geometry_smoothing_moves_points_not_colours(ctx):
    R = rbt_lib.module()
    case = pcc_cases.seam_atlas(R, 0, tiles=3)
    plain = list(case); plain[0] = pcc_cases._copy_atlas(R, case[0], geometry_smoothing=0)
    a, b = ctx.reconstruct_rgb(*case), ctx.reconstruct_rgb(*plain)
    assert (a[0] != b[0]).any() and np.array_equal(a[0], ctx.reconstruct(*case)[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4])


@pytest.mark.parametrize("k", range(6))
def test_colour_metric_equals_brute_force(ctx, k):
    CC.check_metric_case(ctx, CC.metric_cases()[k])


def test_colour_metric_identity_and_bad_arguments(ctx):
    CC.check_metric_identity_and_bad_arguments(ctx, rbt_lib.module())


INT_FIELDS = ("n_a", "n_b", "sse_ab", "sse_ba")


def test_colour_metric_of_large_clouds_equals_host_emulation(ctx, emu):
    """a cloud pair of >= 100 000 points each: merged counts and all six integer sums == the host emulation's; derived fields recomputed from the integers"""
    a, ca, b, cb = CC.large_clouds()
    assert len(a) >= 100000 and len(b) >= 100000
    got, want = ctx.color_metric(a, ca, b, cb), emu.color_metric(a, ca, b, cb)
    for k in INT_FIELDS:
        assert got[k] == want[k], k
    assert min(got["n_a"], got["n_b"]) > 50000 and all(x > 0 for x in got["sse_ab"] + got["sse_ba"])
    CC.check_derived(got)
    assert got == want or all(np.array_equal(np.float32(got[k]), np.float32(want[k])) for k in got)


def test_full_size_frame_after_transcode(ctx, emu):
    """point-cloud frame 0 of the benchmark fixture (the flow of tests/test_gpu_pcc.py::test_full_size_frame_after_transcode): the source cloud with colours is
    reconstruct_rgb of the synthetic maps; the decoded R5 input and the R3 output of the whole path are rebuilt with decoder-side colours. R5 against itself: +inf; R5 and
    R3 against the source: finite Y / U / V PSNR between 10 and 100 dB; all integers == the host emulation's"""
    R = rbt_lib.module(); gs = rbt_lib.module_file("gof_shard")
    man = json.load(open(os.path.join(GOLD, "hm_r5_manifest.json")))["1280x1280_f32"]
    gof = [gs.split_pairs(open(os.path.join(GOLD, man["streams"][k]["file"]), "rb").read())[0] for k in ("occ", "geo", "attr")]
    out = ctx.transcode_gof(gof, gs.rate_params(R, 3))
    w = h = 1280
    patches = synth.atlas_patches(R, w, h, 1051)
    src = synth.make_maps(w, h, 1051)
    s = ctx.reconstruct_rgb(R.AtlasParams(w, h, 16, 1, 2, 1, 1, 0), patches, src["occ_full"].astype(np.uint16), src["geo"][0][: w * h].reshape(h, w), src["geo"][1][: w * h].reshape(h, w), 10,
                            src["attr"][0], src["attr"][1], 10)
    assert s[0].shape[0] > 100000
    clouds = []
    for streams, prec in ((gof, 2), (out, 4)):
        occ = ctx.decode(streams[0])[0][0][: (w // prec) * (h // prec)].reshape(h // prec, w // prec)
        geo = ctx.decode(streams[1])[0]; att = ctx.decode(streams[2])[0]
        c = ctx.reconstruct_rgb(R.AtlasParams(w, h, 16, prec, 2, 1, 1, 0), patches, occ, geo[0][: w * h].reshape(h, w), geo[1][: w * h].reshape(h, w), 10, att[0], att[1], 10)
        plain = ctx.reconstruct(R.AtlasParams(w, h, 16, prec, 2, 1, 1, 0), patches, occ, geo[0][: w * h].reshape(h, w), geo[1][: w * h].reshape(h, w), 10, att[0], att[1], 10)
        assert np.array_equal(c[0], plain[0]) and c[0].shape[0] > 100000
        assert np.array_equal(c[1][:, 0], CC.to_16(CC.to_float(plain[1][:, 0], False, 10), False))          # luma: the point's own sample through the float round trip
        assert np.array_equal(c[4], CC.yuv16_to_rgb8(c[1]))
        clouds.append((c[0], c[4]))
    same = ctx.color_metric(*clouds[0], *clouds[0])
    assert same["sse_ab"] == [0, 0, 0] and all(np.isinf(x) and x > 0 for x in same["psnr"])
    for xyz, rgb in clouds:
        got = ctx.color_metric(s[0], s[4], xyz, rgb)
        print("colour PSNR vs source [Y, U, V]:", got["psnr"])
        assert all(np.isfinite(x) and 10 < x < 100 for x in got["psnr"] + got["psnr_ab"] + got["psnr_ba"])
        want = emu.color_metric(s[0], s[4], xyz, rgb)
        for k in INT_FIELDS:
            assert got[k] == want[k], k
        CC.check_derived(got)
