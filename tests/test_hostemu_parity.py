"""Runs the kernel BODIES (rabbit-transcoding_amd/csrc/*.h) as serial host code (tests/hostemu, a test-only build) and
checks them bit-exactly against the oracle. This catches logic regressions in this GPU-less container; the real parity
tests of the HIP build are tests/test_gpu_*.py (-m gpu)."""
import os
import subprocess
import numpy as np
import pytest
import oracle_lib as O
import rbt_lib
import synth


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
    w = [64, 96, 128, 80][seed % 4]; h = [64, 80, 48, 128][(seed // 4) % 4]
    bd = 10 if seed % 3 else 8
    fr = np.zeros((5, w * h * 3 // 2), np.uint16)
    bs, rec = O.encode(fr, w, h, bd, qp=30, gop=2, stress_seed=seed, log2_ctb=0)
    dec, dw, dh, dbd, chk, fail = ctx.decode(bs)
    assert (dw, dh, dbd, chk, fail) == (w, h, bd, 5, 0) and np.array_equal(dec, rec)


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
    """wavefront mode (one dependent slice segment per CTB row, context variables from the CTB above-right) where its rules bend: pictures one CTB wide
    (no above-right CTB: every row starts from the initial variables), sizes that need a conformance window, 64x64 CTBs, lossless; noise content, so that
    every row carries bins and the one-or-four transform-unit decision goes both ways. Encoder == oracle, and both decoders read the result back."""
    fr = np.random.default_rng(w * 131 + h).integers(0, 1 << bd, size=(n, w * h * 3 // 2), dtype=np.uint16)
    for qp in (22, 34):
        a, ra = O.encode(fr, w, h, bd, qp, gop=1 if lossless else 2, i_qp_offset=0 if lossless else -3, lossless=lossless, log2_ctb=log2_ctb, rows_per_slice=-1)
        b = ctx.encode(fr, w, h, bd, qp, gop=1 if lossless else 2, lossless=lossless, log2_ctb=log2_ctb, rows_per_slice=-1)
        assert a == b
        dec, dw, dh, dbd, chk, fail = ctx.decode(b)
        assert (dw, dh, dbd, chk, fail) == (w, h, bd, n, 0) and np.array_equal(dec, ra)
        if lossless: assert np.array_equal(dec, fr)


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
    R = rbt_lib.module()
    geo, attr, occ = synth.make_gof(128, 128, 2, 11)
    sa, _ = O.encode(attr, 128, 128, 10, 22, gop=2, log2_ctb=6, rows_per_slice=0)
    # CABAC data has no redundancy of its own: a damaged slice may decode to garbage without a syntax error. Eight damage patterns:
    # none may crash or hang, most must be caught (overrun of the slice data, impossible syntax), and the context stays usable.
    caught = 0
    for seed in range(8):
        bad = bytearray(sa)
        r = np.random.default_rng(seed)
        for k in r.integers(len(bad) // 4, len(bad) - 8, 200): bad[int(k)] = int(r.integers(1, 255))
        try:
            ctx.transcode_substream(bytes(bad[: len(bad) // 2 + len(bad) // 3]), R.RBT_VIDEO_ATTRIBUTE, 32)
        except R.RbtError:
            caught += 1
    assert caught >= 4


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
    """more sub-bitstreams than HIP streams (4): pipelines share streams, results must not change"""
    R = rbt_lib.module()
    geo, attr, occ = synth.make_gof(64, 64, 1, 33)
    sg, _ = O.encode(geo, 64, 64, 10, 16, gop=2, log2_ctb=5, rows_per_slice=0)
    sa, _ = O.encode(attr, 64, 64, 10, 22, gop=2, log2_ctb=5, rows_per_slice=0)
    P = R.StreamParams
    streams = [sg, sa, sg, sa, sg]
    params = [P(1, 24, 4, 5, 1, 1, 0), P(19, 32, 4, 5, 1, 1, 0), P(1, 32, 4, 4, 1, 1, 0), P(19, 42, 4, 5, 0, 1, 0), P(1, 28, 4, 5, 1, 1, 1)]
    outs = ctx.transcode_gof(streams, params)
    assert outs[0] == O.transcode_substream(sg, 1, 24)
    assert outs[1] == O.transcode_substream(sa, 19, 32)
    assert outs[2] == O.transcode_substream(sg, 1, 32, log2_ctb=4)
    assert outs[3] == O.transcode_substream(sa, 19, 42, rows_per_slice=0)
    assert outs[4] == ctx.transcode_substream(sg, 1, 28, verify_md5=1)


def test_two_gofs_in_one_call_equal_single_gof_calls(ctx):
    R = rbt_lib.module()
    def gof(w, h, n, seed):
        geo, attr, occ = synth.make_gof(w, h, n, seed)
        return [O.encode(occ, w // 2, h // 2, 8, 8, gop=1, lossless=1, i_qp_offset=0, log2_ctb=6, rows_per_slice=0)[0],
                O.encode(geo, w, h, 10, 16, gop=2, log2_ctb=6, rows_per_slice=0)[0], O.encode(attr, w, h, 10, 22, gop=2, log2_ctb=6, rows_per_slice=0)[0]]
    a, b = gof(64, 64, 2, 101), gof(128, 64, 1, 202)
    P = R.StreamParams
    ps = [P(0, 8, 4, 5, 1, 1, 0), P(1, 24, 4, 5, 1, 1, 0), P(19, 32, 4, 5, 1, 1, 0)]
    outs = ctx.transcode_gof(a + b, ps + ps)
    assert outs[:3] == ctx.transcode_gof(a, ps) and outs[3:] == ctx.transcode_gof(b, ps)
    assert outs[1] == O.transcode_substream(a[1], 1, 24) and outs[5] == O.transcode_substream(b[2], 19, 32)


def test_two_jobs_in_flight_equal_blocking_calls(ctx):
    """rbt_submit_gof / rbt_wait_gof: four GOFs in flight, waited for out of order, give the blocking call's outputs;
    a fifth submit is refused (RBT_ERR_BUSY) and the slots are free again afterwards"""
    R = rbt_lib.module()
    def gof(w, h, n, seed):
        geo, attr, occ = synth.make_gof(w, h, n, seed)
        return [O.encode(occ, w // 2, h // 2, 8, 8, gop=1, lossless=1, i_qp_offset=0, log2_ctb=6, rows_per_slice=0)[0],
                O.encode(geo, w, h, 10, 16, gop=2, log2_ctb=6, rows_per_slice=0)[0], O.encode(attr, w, h, 10, 22, gop=2, log2_ctb=6, rows_per_slice=0)[0]]
    a, b = gof(64, 64, 2, 303), gof(128, 64, 2, 404)
    P = R.StreamParams
    ps = [P(0, 8, 4, 5, 1, 1, 0), P(1, 24, 4, 5, 1, 1, 0), P(19, 32, 4, 5, 1, 1, 0)]
    want_a, want_b = ctx.transcode_gof(a, ps), ctx.transcode_gof(b, ps)
    ctx.set_depth(4)
    ja = ctx.submit_gof(a, ps); jb = ctx.submit_gof(b, ps); jc = ctx.submit_gof(b, ps); jd = ctx.submit_gof(a, ps)
    with pytest.raises(R.RbtError) as e:
        ctx.submit_gof(a, ps)
    assert e.value.code == -7
    assert ctx.wait_gof(jb) == want_b and ctx.wait_gof(jd) == want_a and ctx.wait_gof(ja) == want_a and ctx.wait_gof(jc) == want_b
    with pytest.raises(R.RbtError):          # a job can be waited for once
        ctx.wait_gof(ja)
    dmg = bytearray(a[2]); r = np.random.default_rng(3)
    for k in r.integers(len(dmg) // 2, len(dmg) - 8, 200): dmg[int(k)] = int(r.integers(1, 255))
    i = bytes(dmg).find(b"\x00\x00\x01\x42")           # the SPS: a parameter set that does not parse is an error whatever the slice data decodes to
    dmg[i + 5:i + 20] = b"\xff" * 15
    bad = [a[0], a[1], bytes(dmg[: len(dmg) // 2 + len(dmg) // 3])]
    jc = ctx.submit_gof(bad, ps); jd = ctx.submit_gof(b, ps)
    with pytest.raises(R.RbtError):
        ctx.wait_gof(jc)
    assert ctx.wait_gof(jd) == want_b        # a failed job leaves its neighbour alone
    for depth in (8, 16):                    # 8: two streams per job, 16: one (the parsers of pipelines sharing a stream go into one launch)
        ctx.set_depth(depth)
        jobs = [ctx.submit_gof(a if i % 2 == 0 else b, ps) for i in range(depth)]
        with pytest.raises(R.RbtError):
            ctx.set_depth(2)                 # refused while jobs are in flight
        for i, jb in enumerate(jobs):
            assert ctx.wait_gof(jb) == (want_a if i % 2 == 0 else want_b)
    ctx.set_depth(4)

@pytest.mark.parametrize("w", [1536, 1552, 4096, 4112])
def test_wide_pictures_use_the_larger_parser_variants(ctx, w):
    """the slice parser's LDS line buffers come in three sizes (pictures up to 1536 / 4096 / 8192 samples wide): widths on
    both sides of each boundary, several CTB rows so that every above-neighbour path reads the line buffers"""
    h = 48
    r = np.random.default_rng(w)
    fr = r.integers(0, 1024, (2, w * h * 3 // 2)).astype(np.uint16)
    fr[1] = np.clip(fr[0].astype(int) + r.integers(-2, 3, fr[0].shape), 0, 1023)
    for log2_ctb, seed in ((4, 0), (6, 7)):
        bs, rec = O.encode(fr, w, h, 10, qp=34, gop=2, stress_seed=seed, log2_ctb=log2_ctb)
        dec, dw, dh, dbd, chk, fail = ctx.decode(bs)
        assert (dw, dh, fail) == (w, h, 0) and np.array_equal(dec, rec)


def test_destroy_with_jobs_in_flight_drains_them(ctx):
    """rbt_destroy on a context that still owns submitted jobs waits for their streams and frees them; the slots are free again"""
    R = rbt_lib.module()
    geo, attr, occ = synth.make_gof(64, 64, 1, 909)
    a = [O.encode(occ, 32, 32, 8, 8, gop=1, lossless=1, i_qp_offset=0, log2_ctb=6, rows_per_slice=0)[0],
         O.encode(geo, 64, 64, 10, 16, gop=2, log2_ctb=6, rows_per_slice=0)[0], O.encode(attr, 64, 64, 10, 22, gop=2, log2_ctb=6, rows_per_slice=0)[0]]
    P = R.StreamParams
    ps = [P(0, 8, 4, 5, 1, 1, 0), P(1, 24, 4, 5, 1, 1, 0), P(19, 32, 4, 5, 1, 1, 0)]
    want = ctx.transcode_gof(a, ps)
    c1 = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
    c1.set_depth(3)
    for _ in range(3): c1.submit_gof(a, ps)
    c1.close()                                   # three jobs never waited for
    ctx.set_depth(16)
    jobs = [ctx.submit_gof(a, ps) for _ in range(16)]    # every slot is free again
    assert all(ctx.wait_gof(j) == want for j in jobs)
    ctx.set_depth(4)


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
    r = np.random.default_rng(5)
    y = (r.integers(0, 6, (h // 4, w // 4)) * 37 + 300).repeat(4, 0).repeat(4, 1)            # 4x4 plateaus with steps between them
    y[:, w // 2:] += r.integers(0, 2, (h, w // 2)) * 9                                        # and a noisy half
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


def occupancy_rd_cases(R):
    """(streams, params) lists for occupancy-aware coding (rbt_stream_params.occupancy_rd), shared with tests/test_gpu_transcode.py"""
    P = R.StreamParams

    def gof(w, h, n, seed, l2=6):
        geo, attr, occ = synth.make_gof(w, h, n, seed)
        return [O.encode(occ, w // 2, h // 2, 8, 8, gop=1, lossless=1, i_qp_offset=0, log2_ctb=l2, rows_per_slice=0)[0],
                O.encode(geo, w, h, 10, 16, gop=2, log2_ctb=l2, rows_per_slice=0)[0], O.encode(attr, w, h, 10, 22, gop=2, log2_ctb=l2, rows_per_slice=0)[0]]
    a, b = gof(128, 128, 2, 101), gof(192, 128, 1, 202)
    return [
        (a, [P(0, 8, 4, 5, -1, 0, 0, 0), P(1, 24, 4, 5, -1, 0, 0, 1), P(19, 32, 4, 5, -1, 0, 0, 1)]),                    # the rate points' form: wavefront rows
        (b, [P(0, 8, 4, 5, 1, 1, 0, 0), P(1, 32, 4, 5, 1, 1, 0, 1), P(19, 42, 4, 6, 0, 1, 0, 0)]),                       # row slices; 64x64 CTBs without it on the attribute stream
        (a + b, [P(0, 8, 4, 5, -1, 0, 0, 0), P(1, 24, 4, 5, -1, 0, 0, 1), P(19, 32, 4, 5, -1, 0, 0, 1)] * 2),            # two GOFs in one call: each with its own occupancy map
        (a, [P(0, 8, 2, 5, -1, 0, 0, 0), P(1, 24, 2, 5, -1, 0, 0, 1), P(19, 32, 2, 5, -1, 0, 0, 1)]),                    # occupancy passed through (precision 2): every sample counts
        ([a[1], a[0], a[2]], [P(1, 24, 4, 5, -1, 0, 0, 1), P(0, 8, 4, 5, -1, 0, 0, 0), P(19, 32, 4, 5, -1, 0, 0, 1)]),   # geometry in front of the occupancy stream: coded without it
    ]


def check_occupancy_rd(ctx, R):
    for streams, params in occupancy_rd_cases(R):
        got = ctx.transcode_gof(streams, params)
        want = O.transcode_data(streams, [(p.video_type, p.qp, p.occupancy_precision, p.log2_ctb, p.ctb_rows_per_slice, p.md5_sei, p.occupancy_rd) for p in params])
        assert got == want
    # what it is for: fewer bytes at (about) the same quality of the samples the decoder makes points of
    streams, params = occupancy_rd_cases(R)[0]
    off = ctx.transcode_gof(streams, [R.StreamParams(p.video_type, p.qp, p.occupancy_precision, p.log2_ctb, p.ctb_rows_per_slice, 0, 0, 0) for p in params])
    on = ctx.transcode_gof(streams, params)
    assert on[0] == off[0] and len(on[1]) < 0.9 * len(off[1]) and len(on[2]) < 0.9 * len(off[2])
    w = h = 128
    occ4 = ctx.decode(on[0])[0][:, : (w // 4) * (h // 4)].reshape(-1, h // 4, w // 4) > 0
    m = occ4.repeat(4, 1).repeat(4, 2).repeat(2, 0)                                   # two maps per point-cloud frame
    src = ctx.decode(streams[1])[0][:, : w * h].reshape(-1, h, w).astype(np.float64)
    for s in (1, 2):
        src = ctx.decode(streams[s])[0][:, : w * h].reshape(-1, h, w).astype(np.float64)
        e_on = ((ctx.decode(on[s])[0][:, : w * h].reshape(-1, h, w) - src) ** 2)[m].mean()
        e_off = ((ctx.decode(off[s])[0][:, : w * h].reshape(-1, h, w) - src) ** 2)[m].mean()
        assert e_on < 1.25 * e_off, (s, e_on, e_off)
    with pytest.raises(R.RbtError):
        ctx.transcode_gof(streams, [params[0], R.StreamParams(1, 24, 4, 5, -1, 0, 1, 1), params[2]])      # not together with verify_md5


def test_occupancy_aware_coding_matches_oracle(ctx):
    check_occupancy_rd(ctx, rbt_lib.module())


def check_preset(ctx, R):
    """rbt_stream_params.preset (the reference's x265 preset string, PCCTranscoderParameters.h:58): RBT_PRESET_FAST leaves the round-3 decision tools out, in the library and in
    the oracle alike; HM-like input (the input's modes as candidates), every slice structure, one GOF call with both presets side by side. Shared with tests/test_gpu_transcode.py."""
    assert [R.preset_from_name(n) for n in ("ultrafast", "superfast", "veryfast", "faster", "fast", "medium", "slow", "slower", "veryslow", "placebo", "", None)] == [1] * 2 + [0] * 10
    with pytest.raises(R.RbtError):
        R.preset_from_name("quick")
    m = synth.make_maps(192, 128, 9)
    for key, vt, q0, q1 in (("geo", R.RBT_VIDEO_GEOMETRY, 16, 24), ("attr", R.RBT_VIDEO_ATTRIBUTE, 22, 32)):
        bs, _ = O.encode_hm(m[key], 192, 128, 10, q0)
        for ctb, rows in ((5, -1), (6, 0), (4, 1)):
            fast = ctx.transcode_substream(bs, vt, q1, log2_ctb=ctb, rows_per_slice=rows, md5_sei=0, preset=R.RBT_PRESET_FAST)
            full = ctx.transcode_substream(bs, vt, q1, log2_ctb=ctb, rows_per_slice=rows, md5_sei=0)
            assert fast == O.transcode_substream(bs, int(vt), q1, 4, ctb, rows, 0, preset=1) and full == O.transcode_substream(bs, int(vt), q1, 4, ctb, rows, 0) and fast != full
            assert ctx.decode(fast)[5] == 0
        both = ctx.transcode_gof([bs, bs], [R.StreamParams(vt, q1, 4, 5, -1, 0, 0, 0, 1), R.StreamParams(vt, q1, 4, 5, -1, 0, 0, 0, 0)])     # one decode, two encoders
        assert both[0] == O.transcode_substream(bs, int(vt), q1, 4, 5, -1, 0, preset=1) and both[1] == O.transcode_substream(bs, int(vt), q1, 4, 5, -1, 0)
    with pytest.raises(R.RbtError):
        ctx.transcode_substream(bs, R.RBT_VIDEO_GEOMETRY, 24, preset=2)


def test_preset_matches_oracle(ctx):
    check_preset(ctx, rbt_lib.module())


def split_nals(bs):
    """Annex-B stream -> list of NAL units with their start codes"""
    pos, i = [], bs.find(b"\x00\x00\x01")
    while i >= 0:
        pos.append(i - 1 if i > 0 and bs[i - 1] == 0 else i)
        i = bs.find(b"\x00\x00\x01", i + 3)
    return [bs[a:b] for a, b in zip(pos, pos[1:] + [len(bs)])]


def slice_segment_damage(ctx, R):
    """Slice segments that do not tile their picture (round-2 advisor findings): the host knows where segments start, only the parser finds where they end. A missing
    segment (a hole: in a wavefront stream the row task below would wait for a row nobody parses), a repeated one and two in the wrong order must all be refused -
    quickly, by the first wave that sees it, not after a poll bound - and the context stays usable. Shared with tests/test_gpu_decode.py."""
    geo, attr, occ = synth.make_gof(128, 128, 1, 17)
    for rows in (1, -1):                                   # independent row slices; wavefront rows (dependent segments, one row task per row)
        bs, _ = O.encode(geo, 128, 128, 10, 24, gop=2, log2_ctb=5, rows_per_slice=rows)
        nals = split_nals(bs)
        vcl = [k for k, n in enumerate(nals) if (n[4 if n[:4] == b"\x00\x00\x00\x01" else 3] >> 1) & 63 < 32]
        assert len(vcl) == 8 and ctx.decode(bs)[5] == 0     # two pictures of four CTB rows
        hole = b"".join(n for k, n in enumerate(nals) if k != vcl[2])
        twice = b"".join(n + (n if k == vcl[1] else b"") for k, n in enumerate(nals))
        order = list(range(len(nals))); order[vcl[1]], order[vcl[2]] = order[vcl[2]], order[vcl[1]]
        swapped = b"".join(nals[k] for k in order)
        early = b"".join(n for k, n in enumerate(nals) if k != vcl[3])            # the last row of the first picture is missing
        for bad in (hole, twice, swapped, early):
            with pytest.raises(R.RbtError):
                ctx.decode(bad)
        assert ctx.decode(bs)[5] == 0


def test_slice_segments_must_tile_the_picture(ctx):
    slice_segment_damage(ctx, rbt_lib.module())


@pytest.mark.parametrize("mode", ["RBT_RECON_QUEUE", "RBT_RECON_LEVEL", "RBT_RECON_DIAG"])
def test_every_reconstruction_mode_gives_the_same_pictures(mode, hostemu):
    """the three ways a dependency level is launched (one launch per anti-diagonal; one per level with neighbour flags; one per level with a ready queue, round 4): the host
    build walks each one's order serially - the ready queue by the kernel's own rules (rc_ctb_successors / rc_ctb_need, first in first out) - and all must reproduce the
    oracle. The mode is read once per process, hence the child process (tests/recon_mode_worker.py); the GPU run of the same cases: tests/test_gpu_decode.py"""
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "recon_mode_worker.py"), "hostemu"], env=dict(os.environ, **{mode: "1"}), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK 12"), (r.stdout[-500:], r.stderr[-3000:])
