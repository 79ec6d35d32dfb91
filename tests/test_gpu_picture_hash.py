"""Decoded picture hashes on the MI355X: the checks of tests/test_picture_hash.py against the HIP kernels, and the full-size fixture with
its hash SEIs rewritten in each kind, verified and re-hashed inside the transcoder at depth 1 and with 16 jobs in flight."""
import json
import os
import numpy as np
import pytest
import picture_hash_cases as H
import rbt_lib

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def ctx():
    R = rbt_lib.module()
    c = R.Context(device=0)
    yield c
    c.close()


@pytest.mark.parametrize("bit_depth", [8, 10, 12])
@pytest.mark.parametrize("w,h,n", [(6, 10, 1), (18, 14, 2), (34, 22, 3), (130, 66, 1), (1282, 70, 2)])
def test_picture_hash_matches_annex_d(ctx, bit_depth, w, h, n):
    H.check_picture_hash(ctx, bit_depth, w, h, n, seed=w * 1000 + h * 10 + bit_depth)


def test_verify_every_kind(ctx):
    H.check_verify_kinds(ctx)


def test_output_every_kind(ctx):
    H.check_output_kinds(ctx)


def test_kind_out_of_range_refused(ctx):
    H.check_refused(ctx)


@pytest.fixture(scope="module")
def fixture_gof(ctx):
    """the 1280x1280 32-frame GOF [occ, geo, attr] and, per kind, the same streams with every hash SEI rewritten in that kind"""
    man = json.load(open(os.path.join(GOLDEN, "hm_r5_manifest.json")))["1280x1280_f32"]
    src = [open(os.path.join(GOLDEN, man["streams"][k]["file"]), "rb").read() for k in ("occ", "geo", "attr")]
    kinds = {}
    for s in src:
        dec, w, h, bd, chk, fail = ctx.decode(s, verify_md5=True)     # the fixture's MD5 SEIs (geometry, attribute), checked by the device MD5
        assert chk in (0, len(dec)) and fail == 0
        assert np.array_equal(ctx.picture_hash(dec[:1], w, h, bd, H.MD5)[0], H.picture_hash(dec[0], w, h, bd, H.MD5))
        for kind in (H.MD5, H.CRC, H.CHECKSUM):
            kinds.setdefault(kind, []).append(H.rewrite_hashes(s, ctx.picture_hash(dec, w, h, bd, kind), kind) if chk else s)
    return src, kinds


def _params(R, md5_sei, verify):
    P = R.StreamParams
    return [P(R.RBT_VIDEO_OCCUPANCY, 8, 4, 5, -1, md5_sei, verify), P(R.RBT_VIDEO_GEOMETRY, 24, 4, 5, -1, md5_sei, verify), P(R.RBT_VIDEO_ATTRIBUTE, 32, 4, 5, -1, md5_sei, verify)]


def _same_pictures(out, ref, kind):
    for o, r in zip(out, ref):
        assert H.vcl(o) == H.vcl(r), "outputs differ apart from the SEIs"
        assert [k for k, _ in H.read_hash_seis(o)] == [kind] * len(H.read_hash_seis(o)) and len(H.read_hash_seis(o)) > 0


def test_fixture_every_kind_blocking(ctx, fixture_gof):
    R = rbt_lib.module()
    src, kinds = fixture_gof
    ref = ctx.transcode_gof(src, _params(R, 0, 0))
    for kind, streams in kinds.items():
        out = ctx.transcode_gof(streams, _params(R, kind, 1))
        _same_pictures(out, ref, kind)
        for o in out:                                              # the SEIs written are what the decoder's check finds
            _, _, _, _, chk, fail = ctx.decode(o, verify_md5=True)
            assert chk > 0 and fail == 0


def test_fixture_every_kind_16_jobs(ctx, fixture_gof):
    R = rbt_lib.module()
    src, kinds = fixture_gof
    ref = ctx.transcode_gof(src, _params(R, 0, 0))
    depth = ctx.get_depth()
    ctx.set_depth(16)
    try:
        jobs = [(1 + k % 3, ctx.submit_gof(kinds[1 + k % 3], _params(R, 1 + k % 3, 1))) for k in range(16)]
        for kind, j in jobs:
            _same_pictures(ctx.wait_gof(j), ref, kind)
    finally:
        ctx.set_depth(depth)


def test_fixture_one_bad_picture_fails_its_job_only(ctx, fixture_gof):
    R = rbt_lib.module()
    src, kinds = fixture_gof
    ref = ctx.transcode_gof(src, _params(R, 0, 0))
    dec, w, h, bd, _, _ = ctx.decode(src[2], verify_md5=False)
    bad_attr = H.rewrite_hashes(src[2], ctx.picture_hash(dec, w, h, bd, H.CRC), H.CRC, flip=37)
    depth = ctx.get_depth()
    ctx.set_depth(8)
    try:
        jobs = [ctx.submit_gof([src[0], src[1], bad_attr if k == 3 else kinds[H.CRC][2]], _params(R, 0, 1)) for k in range(6)]
        for k, j in enumerate(jobs):
            if k == 3:
                with pytest.raises(R.RbtError) as e:
                    ctx.wait_gof(j)
                assert e.value.code == H.RBT_ERR_MD5 and "input 2" in str(e.value)
            else:
                assert ctx.wait_gof(j) == ref
    finally:
        ctx.set_depth(depth)
