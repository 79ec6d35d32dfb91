"""GPU parity of the encode half and of the whole transcode path (through the C ABI) vs the CPU oracle: bit-exact
bitstreams, plus size-independent properties at BASELINE.json frame size. The cases shared with the host build are in tests/parity_cases.py."""
import numpy as np
import pytest
import oracle_lib as O
import rbt_lib
import synth
import parity_cases
from parity_cases import r5_gof, r3_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    R = rbt_lib.module()
    c = R.Context(device=0)
    yield c
    c.close()


@pytest.mark.parametrize("w,h,log2_ctb,n,bd,lossless", [(32, 96, 5, 2, 10, 0), (16, 64, 4, 3, 10, 0), (200, 120, 5, 4, 10, 0), (256, 192, 6, 2, 10, 0), (72, 40, 5, 2, 8, 1), (640, 352, 5, 2, 10, 0)])
def test_wavefront_mode_edge_sizes(ctx, w, h, log2_ctb, n, bd, lossless):
    parity_cases.check_wavefront_edge_sizes(ctx, w, h, log2_ctb, n, bd, lossless)


@pytest.mark.parametrize("log2_ctb,rows", [(5, 1), (6, 0), (4, 2), (5, 0), (6, 1), (5, -1), (6, -1), (4, -1)])   # rows -1: wavefront mode
def test_encoder_bitstream_identical(ctx, log2_ctb, rows):
    m = synth.make_maps(256, 192, 41)
    for key, qp in (("geo", 24), ("attr", 32), ("geo", 40), ("attr", 12)):
        a = ctx.encode(m[key], 256, 192, 10, qp, gop=2, log2_ctb=log2_ctb, rows_per_slice=rows)
        b, _ = O.encode(m[key], 256, 192, 10, qp, gop=2, log2_ctb=log2_ctb, rows_per_slice=rows)
        assert a == b
    a = ctx.encode(m["occ"], 128, 96, 8, 8, gop=1, lossless=1, log2_ctb=log2_ctb, rows_per_slice=rows)
    b, _ = O.encode(m["occ"], 128, 96, 8, 8, gop=1, lossless=1, i_qp_offset=0, log2_ctb=log2_ctb, rows_per_slice=rows)
    assert a == b


def test_encoder_edge_sizes(ctx):
    """picture sizes that are not multiples of the CTB: implicit quadtree splits at the right / bottom edge"""
    for (w, h) in ((80, 48), (144, 112), (48, 208)):
        r = np.random.default_rng(w * h)
        fr = r.integers(0, 1024, (4, w * h * 3 // 2)).astype(np.uint16)
        fr[1] = np.clip(fr[0].astype(int) + r.integers(-3, 4, fr[0].shape), 0, 1023)
        fr[3] = fr[2]
        for log2_ctb in (4, 5, 6):
            a = ctx.encode(fr, w, h, 10, 30, gop=2, log2_ctb=log2_ctb, rows_per_slice=1)
            b, _ = O.encode(fr, w, h, 10, 30, gop=2, log2_ctb=log2_ctb, rows_per_slice=1)
            assert a == b


def test_or_pool(ctx):
    r = np.random.default_rng(9)
    p = (r.integers(0, 256, (128, 192)) * (r.random((128, 192)) < 0.2)).astype(np.uint16)
    assert np.array_equal(ctx.or_pool(p, 2), O.or_pool(p, 2))
    assert np.array_equal(ctx.or_pool(np.zeros((64, 64), np.uint16), 2), np.zeros((32, 32), np.uint16))


@pytest.mark.parametrize("target", [(24, 32), (32, 42)])   # R3 and R1 QPs (cfg/rate/ctc-r3.cfg, ctc-r1.cfg)
def test_transcode_substreams_identical_to_oracle(ctx, target):
    R = rbt_lib.module()
    (so, sg, sa), _ = r5_gof(192, 128, 2, 77)
    for s, vt, qp in ((sg, R.RBT_VIDEO_GEOMETRY, target[0]), (sa, R.RBT_VIDEO_ATTRIBUTE, target[1]), (so, R.RBT_VIDEO_OCCUPANCY, 8)):
        assert ctx.transcode_substream(s, vt, qp, verify_md5=1) == O.transcode_substream(s, vt, qp)
    # occupancy precision 2: no pooling, lossless re-encode at the same size
    assert ctx.transcode_substream(so, R.RBT_VIDEO_OCCUPANCY, 8, occupancy_precision=2) == O.transcode_substream(so, 0, 8, occupancy_precision=2)


def test_transcode_gof_equals_per_stream_calls(ctx):
    (so, sg, sa), _ = r5_gof(192, 128, 3, 5)
    outs = ctx.transcode_gof([so, sg, sa], r3_params(rbt_lib.module()))
    assert outs[0] == ctx.transcode_substream(so, 0, 8)
    assert outs[1] == ctx.transcode_substream(sg, 1, 24)
    assert outs[2] == ctx.transcode_substream(sa, 19, 32)


def test_full_size_point_cloud_frame(ctx):
    """BASELINE.json frame size (1280x1280 maps, 640x640 occupancy), one point-cloud frame, R5 -> R3, bit-exact vs oracle;
    then the size-independent properties: output decodes with every MD5 SEI matching, occupancy == OR-pool of the input."""
    R = rbt_lib.module()
    (so, sg, sa), occ = r5_gof(1280, 1280, 1, 1051)
    P = R.StreamParams
    outs = ctx.transcode_gof([so, sg, sa], [P(0, 8, 4, 5, 1, 1, 1), P(1, 24, 4, 5, 1, 1, 1), P(19, 32, 4, 5, 1, 1, 1)])
    assert outs[1] == O.transcode_substream(sg, 1, 24)
    assert outs[2] == O.transcode_substream(sa, 19, 32)
    assert outs[0] == O.transcode_substream(so, 0, 8)
    dec, w, h, bd, chk, fail = ctx.decode(outs[0])
    assert (w, h, bd, fail) == (320, 320, 8, 0) and chk == 1
    want = (occ[:, :640 * 640].reshape(1, 320, 2, 320, 2).max(axis=(2, 4)) > 0).astype(np.uint16)
    assert np.array_equal(dec[:, :320 * 320].reshape(1, 320, 320), want)
    for o in outs[1:]:
        dec, w, h, bd, chk, fail = ctx.decode(o)
        assert (w, h, bd, chk, fail) == (1280, 1280, 10, 2, 0)


def test_transcode_is_idempotent_in_structure(ctx):
    """transcoding the transcoder's own output (per-row slices, CTB 32) works and keeps sizes / frame counts"""
    R = rbt_lib.module()
    (so, sg, sa), _ = r5_gof(128, 128, 2, 3)
    once = ctx.transcode_substream(sg, R.RBT_VIDEO_GEOMETRY, 24)
    twice = ctx.transcode_substream(once, R.RBT_VIDEO_GEOMETRY, 32, verify_md5=1)
    assert twice == O.transcode_substream(once, 1, 32)
    dec, w, h, bd, chk, fail = ctx.decode(twice)
    assert (w, h, dec.shape[0], fail) == (128, 128, 4, 0)


def test_transcode_rejects_damaged_input(ctx):
    parity_cases.check_damaged_input(ctx, rbt_lib.module())


def test_transcode_gof_more_streams_than_pipelines(ctx):
    parity_cases.check_more_streams_than_pipelines(ctx, rbt_lib.module(), 128, 128, log2_ctb=6)


def test_two_gofs_in_one_call_equal_single_gof_calls(ctx):
    parity_cases.check_two_gofs_in_one_call(ctx, rbt_lib.module(), (128, 128, 2, 101), (192, 128, 1, 202))


def test_two_jobs_in_flight_equal_blocking_calls(ctx):
    """three rounds, the steady-state pipeline, depths on both sides of every change in the HIP streams per job; no damaged job"""
    parity_cases.check_jobs_in_flight(ctx, rbt_lib.module(), (192, 128, 4, 303), (128, 192, 4, 404), rounds=3, submit_ahead=True, depths=(5, 8, 16, 1), damaged_job=False)


def test_destroy_with_jobs_in_flight_drains_them():
    """a new context takes the sixteen jobs afterwards"""
    R = rbt_lib.module()
    parity_cases.check_destroy_with_jobs_in_flight(R, lambda: R.Context(device=0), (128, 128, 2, 909))



def test_matrix_core_transforms_equal_vector_alu(ctx):
    """32-point transform stages on v_mfma_i32_32x32x32_i8 (csrc/rbt_mfma.h) vs the vector-ALU stages, on the device: random, sparse and extreme blocks"""
    r = np.random.default_rng(5)
    blocks = [r.integers(-32768, 32768, 1024), r.integers(-600, 600, 1024), np.full(1024, 32767), np.full(1024, -32768), np.zeros(1024)]
    sp = np.zeros(1024, np.int64); sp[[0, 1, 32, 33, 5 * 32 + 7]] = [4000, -3000, 2500, -32768, 32767]; blocks.append(sp)
    for k in range(26): blocks.append(r.integers(-32768, 32768, 1024) * (r.random(1024) < 0.05))
    alt = np.where((np.arange(1024) // 32 + np.arange(1024)) % 2 == 0, 32767, -32768); blocks.append(alt)
    for bd in (8, 10):
        assert ctx.selftest_transform32(np.stack(blocks).astype(np.int16), bd) == 0


def test_stream_conversions_in_the_gpu_run(ctx):
    """rbt_sample_to_byte_stream / rbt_byte_to_sample_stream (PCCVideoBitstream.cpp:85-172) need no device, but they are part of the path the GPU box
    runs: a re-encoded sub-bitstream framed the way transcodeVideo leaves it (byteStreamToSampleStream, :517) and back, vs the oracle restatement"""
    import ctypes
    R = rbt_lib.module()
    (so, sg, sa), _ = r5_gof(128, 128, 2, 19)
    out = ctx.transcode_substream(sg, R.RBT_VIDEO_GEOMETRY, 24)
    L = ctx.L
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert L.rbt_byte_to_sample_stream(out, len(out), ctypes.byref(p), ctypes.byref(n)) == 0
    ss = ctypes.string_at(p, n.value); L.rbt_free(p)
    assert ss == O.byte_to_sample_stream(out)
    assert L.rbt_sample_to_byte_stream(ss, len(ss), ctypes.byref(p), ctypes.byref(n)) == 0
    bs = ctypes.string_at(p, n.value); L.rbt_free(p)
    assert bs == O.sample_to_byte_stream(ss)
    # the reference's start-code rule re-frames the stream (4-byte codes only for the first NAL, parameter sets / SEI and after a VCL NAL);
    # the NAL payloads must survive the round trip, and the result must still transcode to the same output
    assert ctx.transcode_substream(bs, R.RBT_VIDEO_GEOMETRY, 24) == ctx.transcode_substream(out, R.RBT_VIDEO_GEOMETRY, 24)


@pytest.mark.parametrize("w,h,log2_ctb,rows", [(128, 96, 5, -1), (320, 256, 5, -1), (192, 128, 4, 1), (256, 256, 6, 0)])
def test_transform_skip_blocks(ctx, monkeypatch, w, h, log2_ctb, rows):
    """4x4 luma blocks with the DST or with transform skip, whichever is cheaper (csrc en_tile_intra_tb == oracle hm_tb_finish): step-shaped depth maps, where skipping
    wins often. GPU encoder == oracle, the stream differs from the oracle's without transform skip, and the GPU decoder reads it back to the encoder's reconstruction."""
    y = parity_cases.step_map(np.random.default_rng(w + h), w, h)
    fr = np.concatenate([y.ravel(), np.full(w * h // 2, 512)]).astype(np.uint16)[None, :].repeat(4, 0)
    fr[2:, : w * h] = np.roll(y, 3, axis=1).ravel()
    ratios = []
    for qp in (20, 30):
        bs = ctx.encode(fr, w, h, 10, qp, gop=2, log2_ctb=log2_ctb, rows_per_slice=rows)
        on, rec = O.encode(fr, w, h, 10, qp, gop=2, log2_ctb=log2_ctb, rows_per_slice=rows)
        assert bs == on
        monkeypatch.setenv("RBT_ENC_TS", "0")
        off, rec_off = O.encode(fr, w, h, 10, qp, gop=2, log2_ctb=log2_ctb, rows_per_slice=rows)
        monkeypatch.delenv("RBT_ENC_TS")
        assert on != off                                                      # transform skip blocks were chosen (per block by distortion + lambda * rate)
        # ... and the choice pays: the rate-distortion cost of the whole stream (squared error of the reconstruction + lambda * bits, lambda of the I slices' QP as HM
        # defines it, 0.57 * 2^((QP - 12) / 3)) is no greater with the tool than without it - neither bytes nor distortion alone need to go down
        lam = 0.57 * 2.0 ** ((qp - 3 - 12) / 3.0)
        cost = lambda stream, r_: float(((r_.astype(np.int64) - fr.astype(np.int64)) ** 2).sum()) + lam * 8 * len(stream)
        ratios.append(cost(on, rec) / cost(off, rec_off))
        assert ratios[-1] <= 1.001, (qp, len(on), len(off), ratios)            # the choice is made block by block on the block's own cost: one case of the eight here ends 0.03 % above
        dec, _, _, _, chk, fail = ctx.decode(bs)
        assert (chk, fail) == (4, 0) and np.array_equal(dec, rec)
    assert sum(ratios) / len(ratios) < 1.0005, ratios                           # ... over the two QPs: a gain of 0.1 - 1 % in three of the four cases here, a wash (+0.01 %) in the 320x256 one


def test_occupancy_aware_coding_matches_oracle(ctx):
    """rbt_stream_params.occupancy_rd on the GPU: geometry / attribute streams coded with the occupancy map the output carries (made on the
    occupancy pipeline's stream, waited for by the others) == oracle_transcode_data for every case of tests/parity_cases.py occupancy_rd_cases, fewer bytes,
    the occupied samples as good as without; then with two jobs in flight (the maps of one job must not be read by another)."""
    R = rbt_lib.module()
    parity_cases.check_occupancy_rd(ctx, R)
    cases = parity_cases.occupancy_rd_cases(R)[:3]
    want = [ctx.transcode_gof(s, p) for s, p in cases]
    jobs = [ctx.submit_gof(s, p) for s, p in cases[:2]]
    assert [ctx.wait_gof(j) for j in jobs] == want[:2]


def test_preset_matches_oracle(ctx):
    """rbt_stream_params.preset on the GPU: RBT_PRESET_FAST == the oracle without the round-3 decision tools, the default == the oracle with them, both in one call"""
    parity_cases.check_preset(ctx, rbt_lib.module())


def test_preset_fast_full_size_frame(ctx):
    """one point-cloud frame of the committed 1280x1280 fixture, R5 -> R3 at RBT_PRESET_FAST: == oracle; more bytes than the default (which the other full-size tests pin)"""
    import os
    gs = rbt_lib.module_file("gof_shard")
    R = rbt_lib.module()
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    first = [gs.split_pairs(open(os.path.join(gold, f"hm_r5_1280x1280_f32_{k}.annexb"), "rb").read())[0] for k in ("occ", "geo", "attr")]
    fast_p = gs.rate_params(R, 3, preset=R.RBT_PRESET_FAST)
    fast = ctx.transcode_gof(first, fast_p)
    assert fast == O.transcode_data(first, [(p.video_type, p.qp, p.occupancy_precision, p.log2_ctb, p.ctb_rows_per_slice, p.md5_sei, 0, p.preset) for p in fast_p])
    full = ctx.transcode_gof(first, gs.rate_params(R, 3))
    assert fast[0] == full[0] and len(fast[1]) > len(full[1]) and len(fast[2]) > 1.05 * len(full[2])


def test_occupancy_aware_coding_full_size_frame(ctx):
    """the committed 1280x1280 fixture, R5 -> R3 with occupancy_rd. Frame 0: == oracle, and what the option is for - at least 40 % fewer geometry bytes. Quality where the
    claim of include/rbt.h and DESIGN.md stands - on the MEAN over the GOF's four base atlases (frames 0..3), because one frame's D1 scatters by +-0.3 dB between any
    two encoder variants (a depth error of 1 on a few thousand of 600 000 points; round 3 saw 0.34 dB on frame 0 alone): mean D1 within 0.1 dB of the plain transcode's,
    luma PSNR of the samples the decoder makes points of within 0.1 dB (geometry and attribute, all eight pictures)."""
    import os
    gs = rbt_lib.module_file("gof_shard")
    R = rbt_lib.module()
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    fixture = [open(os.path.join(gold, f"hm_r5_1280x1280_f32_{k}.annexb"), "rb").read() for k in ("occ", "geo", "attr")]
    first = [gs.split_pairs(s)[0] for s in fixture]
    P = R.StreamParams
    on_p = [P(0, 8, 4, 5, -1, 0, 0, 0), P(1, 24, 4, 5, -1, 0, 0, 1), P(19, 32, 4, 5, -1, 0, 0, 1)]
    off_p = [P(p.video_type, p.qp, 4, 5, -1, 0, 0, 0) for p in on_p]
    on = ctx.transcode_gof(first, on_p)
    assert on == O.transcode_data(first, [(p.video_type, p.qp, p.occupancy_precision, p.log2_ctb, p.ctb_rows_per_slice, p.md5_sei, p.occupancy_rd) for p in on_p])
    off = ctx.transcode_gof(first, off_p)
    assert len(on[1]) < 0.6 * len(off[1]) and len(on[2]) < 0.85 * len(off[2])
    w = h = 1280; nfr = 4
    four = [b"".join(gs.split_pairs(s)[:nfr]) for s in fixture]
    on4, off4 = ctx.transcode_gof(four, on_p), ctx.transcode_gof(four, off_p)
    d1 = {"off": [], "on": []}
    for key, outs in (("off", off4), ("on", on4)):
        occ_d, geo_d = ctx.decode(outs[0])[0], ctx.decode(outs[1])[0]
        for k in range(nfr):
            src = synth.make_maps(w, h, 1051 + k)
            pats = synth.atlas_patches(R, w, h, 1051 + k)
            cloud = lambda occ_plane, prec, g0, g1: ctx.reconstruct(R.AtlasParams(w, h, 16, prec, 2, 1, 1, 0), pats, occ_plane, g0[: w * h].reshape(h, w), g1[: w * h].reshape(h, w), 10)[0]
            c_src = cloud(src["occ_full"].astype(np.uint16), 1, src["geo"][0], src["geo"][1])
            d1[key].append(ctx.d1(c_src, cloud(occ_d[k][: (w // 4) * (h // 4)].reshape(h // 4, w // 4), 4, geo_d[2 * k], geo_d[2 * k + 1]))["psnr"])
    mean = lambda v: sum(v) / len(v)
    assert abs(mean(d1["on"]) - mean(d1["off"])) <= 0.1, d1
    m = (ctx.decode(on4[0])[0][:, : (w // 4) * (h // 4)].reshape(-1, h // 4, w // 4) > 0).repeat(4, 1).repeat(4, 2).repeat(2, 0)      # two maps per point-cloud frame
    for k in (1, 2):
        ref = ctx.decode(four[k])[0][:, : w * h].reshape(-1, h, w).astype(np.float64)
        e = [float(np.mean(((ctx.decode(o[k])[0][:, : w * h].reshape(-1, h, w) - ref) ** 2)[m])) for o in (off4, on4)]
        assert abs(10 * np.log10(e[1] / e[0])) <= 0.1, (k, e)
