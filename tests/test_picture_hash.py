"""Decoded picture hashes of all three kinds (MD5, CRC, checksum; H.265 D.3.19): rbt_picture_hash against the restatement of Annex D,
verify_md5 on streams whose SEIs carry each kind, md5_sei = 1..3 on the output. Runs the hash kernels' bodies through the host emulation
(tests/hostemu); tests/test_gpu_picture_hash.py runs the same checks on the GPU."""
import os
import subprocess
import pytest
import picture_hash_cases as H
import rbt_lib


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    R = rbt_lib.module()
    c = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


def test_crc_restatements_agree():
    rng = __import__("numpy").random.default_rng(1)
    for n in (0, 1, 2, 3, 17, 64, 200):
        data = rng.integers(0, 256, n, dtype="uint8").tobytes()
        assert H.crc_annex_d(data) == H.crc_bytewise(data)
    assert H.crc_annex_d(b"123456789") == 0xE5CC      # the register of D.3.19 is CRC-16/AUG-CCITT


@pytest.mark.parametrize("bit_depth", [8, 10, 12])
@pytest.mark.parametrize("w,h,n", [(6, 10, 1), (18, 14, 2), (34, 22, 3), (2, 6, 2), (130, 66, 1)])
def test_picture_hash_matches_annex_d(ctx, bit_depth, w, h, n):
    H.check_picture_hash(ctx, bit_depth, w, h, n, seed=w * 1000 + h * 10 + bit_depth)


def test_verify_every_kind(ctx):
    H.check_verify_kinds(ctx)


def test_output_every_kind(ctx):
    H.check_output_kinds(ctx)


def test_kind_out_of_range_refused(ctx):
    H.check_refused(ctx)
