"""Runs the kernel BODIES (rabbit-transcoding_amd/csrc/*.h) as serial host code (tests/hostemu, a test-only build) and
checks them bit-exactly against the oracle. This catches logic regressions in this GPU-less container; the real parity
tests of the HIP build are tests/test_gpu_*.py (-m gpu), which run the cases of tests/parity_cases.py on the GPU."""
import os
import subprocess
import numpy as np
import pytest
import oracle_lib as O
import rbt_lib
import synth
import parity_cases


@pytest.fixture(scope="module")
def hostemu():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])


@pytest.fixture(scope="module")
def ctx(hostemu):
    R = rbt_lib.module()
    c = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


@pytest.mark.parametrize("seed", range(1, 31))
def test_decode_stress_streams(ctx, seed):
    parity_cases.check_stress_decode(ctx, seed)


@pytest.mark.parametrize("log2_ctb,rows", [(5, 1), (6, 0), (4, 2), (5, -1), (6, -1), (4, -1)])   # rows -1: wavefront mode (one dependent slice segment per CTB row)
def test_encoder_and_transcode_bitstreams(ctx, log2_ctb, rows):
    R = rbt_lib.module()
    geo, attr, occ = synth.make_gof(128, 128, 2, 21)
    for fr, qp in ((geo, 24), (attr, 32)):
        assert ctx.encode(fr, 128, 128, 10, qp, gop=2, log2_ctb=log2_ctb, rows_per_slice=rows) == O.encode(fr, 128, 128, 10, qp, gop=2, log2_ctb=log2_ctb, rows_per_slice=rows)[0]
    sg, _ = O.encode(geo, 128, 128, 10, 16, gop=2, log2_ctb=6, rows_per_slice=0)
    so, _ = O.encode(occ, 64, 64, 8, 8, gop=1, lossless=1, i_qp_offset=0, log2_ctb=6, rows_per_slice=0)
    assert ctx.transcode_substream(sg, R.RBT_VIDEO_GEOMETRY, 24, log2_ctb=log2_ctb, rows_per_slice=rows) == O.transcode_substream(sg, 1, 24, log2_ctb=log2_ctb, rows_per_slice=rows)
    assert ctx.transcode_substream(so, R.RBT_VIDEO_OCCUPANCY, 8, log2_ctb=log2_ctb, rows_per_slice=rows) == O.transcode_substream(so, 0, 8, log2_ctb=log2_ctb, rows_per_slice=rows)


@pytest.mark.parametrize("w,h,log2_ctb,n,bd,lossless", [(32, 96, 5, 2, 10, 0), (16, 64, 4, 3, 10, 0), (200, 120, 5, 4, 10, 0), (96, 80, 4, 3, 10, 0), (256, 192, 6, 2, 10, 0), (64, 64, 5, 2, 8, 1), (72, 40, 5, 2, 8, 1)])
def test_wavefront_mode_edge_sizes(ctx, w, h, log2_ctb, n, bd, lossless):
    parity_cases.check_wavefront_edge_sizes(ctx, w, h, log2_ctb, n, bd, lossless)


def test_transcode_of_hm_like_input_uses_its_intra_modes(ctx):
    """a transcode hands the input stream's intra modes to the re-encoder's analysis (planar, DC + the input's modes at a block's four quarters): on
    HM-like input (NxN, 35 modes: up to six distinct candidates per block) the re-encode differs from the encoder run on the decoded pictures alone,
    and equals the oracle's"""
    R = rbt_lib.module()
    m = synth.make_maps(192, 128, 9)
    for key, vt, q0, q1 in (("geo", R.RBT_VIDEO_GEOMETRY, 16, 24), ("attr", R.RBT_VIDEO_ATTRIBUTE, 22, 32)):
        bs, _ = O.encode_hm(m[key], 192, 128, 10, q0)
        out = ctx.transcode_substream(bs, vt, q1, log2_ctb=5, rows_per_slice=-1, md5_sei=0)
        assert out == O.transcode_substream(bs, int(vt), q1, 4, 5, -1, 0)
        dec, *_ = O.decode(bs)
        assert out != O.encode(dec, 192, 128, 10, q1, gop=2, log2_ctb=5, rows_per_slice=-1, md5_sei=0)[0]


def test_transcode_rejects_damaged_input(ctx):
    parity_cases.check_damaged_input(ctx, rbt_lib.module())


def test_banded_parse_is_bit_identical(monkeypatch, hostemu):
    """RBT_PARSE_BANDS: the resumable parser (suspend in front of a CTB row, resume in a later launch) gives the same streams"""
    import subprocess, sys, os
    code = ("import sys; sys.path.insert(0, 'tests'); import rbt_lib, synth, oracle_lib as O\n"
            "R = rbt_lib.module(); c = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)\n"
            "geo, attr, occ = synth.make_gof(128, 192, 2, 21)\n"
            "sa, _ = O.encode(attr, 128, 192, 10, 22, gop=2, log2_ctb=5, rows_per_slice=0)\n"
            "assert c.transcode_substream(sa, R.RBT_VIDEO_ATTRIBUTE, 32) == O.transcode_substream(sa, 19, 32)\n")
    env = dict(os.environ, RBT_PARSE_BANDS="3")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_transcode_gof_more_streams_than_pipelines(ctx):
    parity_cases.check_more_streams_than_pipelines(ctx, rbt_lib.module(), 64, 64, log2_ctb=5)


def test_two_gofs_in_one_call_equal_single_gof_calls(ctx):
    parity_cases.check_two_gofs_in_one_call(ctx, rbt_lib.module(), (64, 64, 2, 101), (128, 64, 1, 202))


def test_two_jobs_in_flight_equal_blocking_calls(ctx):
    """one round, then a damaged job next to a good one; depth 8: two streams per job, 16: one"""
    parity_cases.check_jobs_in_flight(ctx, rbt_lib.module(), (64, 64, 2, 303), (128, 64, 2, 404), rounds=1, submit_ahead=False, depths=(8, 16), damaged_job=True)


@pytest.mark.parametrize("w", [1536, 1552, 4096, 4112])
def test_wide_pictures_use_the_larger_parser_variants(ctx, w):
    parity_cases.check_wide_pictures(ctx, w)


def test_destroy_with_jobs_in_flight_drains_them(ctx):
    """the module's context takes the sixteen jobs afterwards"""
    R = rbt_lib.module()
    parity_cases.check_destroy_with_jobs_in_flight(R, lambda: R.Context(lib_path=rbt_lib.HOSTEMU_LIB), (64, 64, 1, 909), ctx=ctx)


def test_job_api_argument_checks(ctx):
    """bad arguments are refused with RBT_ERR_PARAM before anything is enqueued; a job belongs to the context that submitted it"""
    import ctypes as C
    R = rbt_lib.module(); L = ctx.L
    job = C.c_void_p()
    assert L.rbt_submit_gof(ctx.h, 0, None, None, None, C.byref(job)) == -4
    assert L.rbt_submit_gof(None, 1, None, None, None, C.byref(job)) == -4
    assert L.rbt_set_depth(ctx.h, 0) == -4 and L.rbt_set_depth(ctx.h, 17) == -4
    outs = (C.c_void_p * 1)(); ns = (C.c_size_t * 1)()
    assert L.rbt_wait_gof(ctx.h, None, outs, ns) == -4
    geo, attr, occ = synth.make_gof(64, 64, 1, 5)
    s1 = O.encode(geo, 64, 64, 10, 16, gop=2, log2_ctb=6, rows_per_slice=0)[0]
    other = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
    j = ctx.submit_gof([s1], [R.StreamParams(1, 24, 4, 5, 1, 1, 0)])
    with pytest.raises(R.RbtError) as e:
        other.wait_gof(j)                        # not its job
    assert e.value.code == -4
    assert ctx.wait_gof(j) == [O.transcode_substream(s1, 1, 24)]
    other.close()



def test_last_error_text_and_trim(ctx):
    """rbt_last_error names what a failing call objected to; rbt_trim hands the cached device memory back (refused while jobs are in flight)"""
    R = rbt_lib.module()
    geo, attr, occ = synth.make_gof(64, 64, 1, 5)
    src, _ = O.encode(geo, 64, 64, 10, 16, gop=2, log2_ctb=5, rows_per_slice=1)
    bad = bytearray(src); i = bad.find(b"\x00\x00\x01\x42"); bad[i + 5:i + 20] = b"\xff" * 15   # an SPS that does not parse
    with pytest.raises(R.RbtError) as ei:
        ctx.decode(bytes(bad))
    assert len(str(ei.value)) > len("rbt error")            # code text plus the library's own sentence
    job = ctx.submit_gof([src], [R.StreamParams(R.RBT_VIDEO_GEOMETRY, 24, 4, 5, -1, 0, 0)])
    with pytest.raises(R.RbtError):
        ctx.trim()                                           # RBT_ERR_BUSY: a job is in flight
    out = ctx.wait_gof(job)
    ctx.trim()
    assert ctx.transcode_gof([src], [R.StreamParams(R.RBT_VIDEO_GEOMETRY, 24, 4, 5, -1, 0, 0)]) == out   # works the same from an empty cache


@pytest.mark.parametrize("log2_ctb", [4, 5, 6])
def test_wavefront_rows_behind_entry_points(ctx, log2_ctb):
    """x265's form of a wavefront stream: one slice segment per picture, its CTB rows behind entry point offsets (the oracle writes it with rows_per_slice=-2).
    The decoder cuts the segment into one parse task per row; result == the oracle's decode, and a transcode of it == the oracle's."""
    R = rbt_lib.module()
    m = synth.make_maps(256, 192, 31)
    for key, vt, q0, q1 in (("geo", R.RBT_VIDEO_GEOMETRY, 16, 24), ("attr", R.RBT_VIDEO_ATTRIBUTE, 22, 32)):
        bs, rec = O.encode(m[key], 256, 192, 10, q0, gop=2, log2_ctb=log2_ctb, rows_per_slice=-2)
        assert len(O.slice_headers(bs)) == 2                                      # two pictures, one segment each
        dec, w, h, bd, chk, fail = ctx.decode(bs)
        assert (chk, fail) == (2, 0) and np.array_equal(dec, rec)
        assert ctx.transcode_substream(bs, vt, q1, log2_ctb=5, rows_per_slice=-1, md5_sei=0) == O.transcode_substream(bs, int(vt), q1, 4, 5, -1, 0)


def test_transform_skip_blocks_are_chosen_and_mirrored(ctx, monkeypatch):
    """RBT-E1 codes a 4x4 luma block with the DST or with transform skip, whichever is cheaper (oracle hm_tb_finish, csrc en_tile_intra_tb). A depth map made of
    small steps is where skipping wins: the stream must differ from the one coded with RBT_ENC_TS=0 (the oracle reads the switch per call), equal the oracle's
    with it, carry transform_skip_enabled_flag, and decode to the encoder's reconstruction."""
    w, h = 128, 96
    y = parity_cases.step_map(np.random.default_rng(5), w, h)
    fr = np.concatenate([y.ravel(), np.full(w * h // 2, 512)]).astype(np.uint16)[None, :].repeat(2, 0)
    bs = ctx.encode(fr, w, h, 10, 24, gop=2, log2_ctb=5, rows_per_slice=-1)
    on, rec = O.encode(fr, w, h, 10, 24, gop=2, log2_ctb=5, rows_per_slice=-1)
    assert bs == on
    monkeypatch.setenv("RBT_ENC_TS", "0")
    off, _ = O.encode(fr, w, h, 10, 24, gop=2, log2_ctb=5, rows_per_slice=-1)
    monkeypatch.delenv("RBT_ENC_TS")
    assert off != on          # transform skip blocks were chosen (the choice is by distortion + lambda * rate per block: a few bytes either way on this clip)
    dec, _, _, _, chk, fail = ctx.decode(bs)
    assert (chk, fail) == (2, 0) and np.array_equal(dec, rec)
    # lossless streams have no transform to skip: the flag stays off
    lo = ctx.encode(fr[:1], w, h, 10, 8, gop=1, lossless=1, log2_ctb=5, rows_per_slice=0)
    assert lo == O.encode(fr[:1], w, h, 10, 8, gop=1, lossless=1, i_qp_offset=0, log2_ctb=5, rows_per_slice=0)[0]


@pytest.mark.parametrize("w,h,log2_ctb,rows", [(128, 96, 5, -1), (64, 64, 4, 1), (192, 128, 6, 0)])
def test_transform_skip_8_bit_streams(ctx, w, h, log2_ctb, rows):
    """the same choice in 8-bit streams (the residual is scaled by 2^5 instead of 2^3 before the quantiser): encoder == oracle, decoder reads it back"""
    r = np.random.default_rng(w)
    y = (r.integers(0, 6, (h // 4, w // 4)) * 9 + 60).repeat(4, 0).repeat(4, 1) + r.integers(0, 3, (h, w))
    fr = np.concatenate([y.ravel(), r.integers(100, 140, w * h // 2)]).astype(np.uint16)[None, :].repeat(2, 0)
    for qp in (18, 27, 36):
        bs = ctx.encode(fr, w, h, 8, qp, gop=2, log2_ctb=log2_ctb, rows_per_slice=rows)
        on, rec = O.encode(fr, w, h, 8, qp, gop=2, log2_ctb=log2_ctb, rows_per_slice=rows)
        assert bs == on
        dec, _, _, bd, chk, fail = ctx.decode(bs)
        assert (bd, chk, fail) == (8, 2, 0) and np.array_equal(dec, rec)


def test_occupancy_aware_coding_matches_oracle(ctx):
    parity_cases.check_occupancy_rd(ctx, rbt_lib.module())


def test_preset_matches_oracle(ctx):
    parity_cases.check_preset(ctx, rbt_lib.module())


def test_slice_segments_must_tile_the_picture(ctx):
    parity_cases.slice_segment_damage(ctx, rbt_lib.module())


@pytest.mark.parametrize("mode", ["RBT_RECON_QUEUE", "RBT_RECON_LEVEL", "RBT_RECON_DIAG"])
def test_every_reconstruction_mode_gives_the_same_pictures(mode, hostemu):
    """the three ways a dependency level is launched (one launch per anti-diagonal; one per level with neighbour flags; one per level with a ready queue, round 4): the host
    build walks each one's order serially - the ready queue by the kernel's own rules (rc_ctb_successors / rc_ctb_need, first in first out) - and all must reproduce the
    oracle. The mode is read once per process, hence the child process (tests/recon_mode_worker.py); the GPU run of the same cases: tests/test_gpu_decode.py"""
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "recon_mode_worker.py"), "hostemu"], env=dict(os.environ, **{mode: "1"}), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK 12"), (r.stdout[-500:], r.stderr[-3000:])
