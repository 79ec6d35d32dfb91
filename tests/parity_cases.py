"""Decode and transcode parity cases, shared by the host build of the kernel bodies (test_hostemu_parity.py) and the HIP build (test_gpu_transcode.py, test_gpu_decode.py):
a case means the same on both. The test files pick the context and the sizes; what differs between the backends (picture sizes, rounds, depth lists, steps that feed
damaged streams) comes in as arguments."""
import numpy as np
import pytest
import oracle_lib as O
import synth


def r5_gof(w, h, n_pc, seed, log2_ctb=6):
    """-> ([occupancy, geometry, attribute] sub-bitstreams of one GOF of n_pc point-cloud frames at R5-like settings, the occupancy source frames)"""
    geo, attr, occ = synth.make_gof(w, h, n_pc, seed)
    sg, _ = O.encode(geo, w, h, 10, 16, gop=2, log2_ctb=log2_ctb, rows_per_slice=0)
    sa, _ = O.encode(attr, w, h, 10, 22, gop=2, log2_ctb=log2_ctb, rows_per_slice=0)
    so, _ = O.encode(occ, w // 2, h // 2, 8, 8, gop=1, lossless=1, i_qp_offset=0, log2_ctb=log2_ctb, rows_per_slice=0)
    return [so, sg, sa], occ


def r3_params(R):
    """the R3 target of an [occupancy, geometry, attribute] GOF: 32x32 CTBs, one slice per CTB row, MD5 SEIs written, the input's not checked"""
    P = R.StreamParams
    return [P(0, 8, 4, 5, 1, 1, 0), P(1, 24, 4, 5, 1, 1, 0), P(19, 32, 4, 5, 1, 1, 0)]


def step_map(r, w, h):
    """luma of a depth map made of small steps, where transform skip wins: 4x4 plateaus with steps between them, and a noisy half"""
    y = (r.integers(0, 6, (h // 4, w // 4)) * 37 + 300).repeat(4, 0).repeat(4, 1)
    y[:, w // 2:] += r.integers(0, 2, (h, w // 2)) * 9
    return y


def damage(bs, seed, first):
    """200 bytes of bs[first:] overwritten, the last sixth cut off"""
    bad = bytearray(bs); r = np.random.default_rng(seed)
    for k in r.integers(first, len(bad) - 8, 200): bad[int(k)] = int(r.integers(1, 255))
    return bad[: len(bad) // 2 + len(bad) // 3]


def check_stress_decode(ctx, seed):
    """random-syntax streams: all intra modes, NxN, TU trees, TS, bypass, AMP, AMVP/merge, TMVP, SAO, dQP, SDH, slices"""
    w = [64, 96, 128, 80][seed % 4]; h = [64, 80, 48, 128][(seed // 4) % 4]
    bd = 10 if seed % 3 else 8
    fr = np.zeros((5, w * h * 3 // 2), np.uint16)
    bs, rec = O.encode(fr, w, h, bd, qp=30, gop=2, stress_seed=seed, log2_ctb=0)
    dec, dw, dh, dbd, chk, fail = ctx.decode(bs)
    assert (dw, dh, dbd, chk, fail) == (w, h, bd, 5, 0) and np.array_equal(dec, rec)


def check_wavefront_edge_sizes(ctx, w, h, log2_ctb, n, bd, lossless):
    """wavefront mode (one dependent slice segment per CTB row, context variables from the CTB above-right; on the GPU rows of a picture on different waves, progress
    counters between them) where its rules bend: pictures one CTB wide (no above-right CTB: every row starts from the initial variables), sizes that need a conformance
    window, 64x64 CTBs, lossless, a picture wide enough for several waves; noise content, so that every row carries bins and the one-or-four transform-unit decision
    goes both ways. Encoder == oracle, the decoder reads the result back, and a lossless stream decodes to the source."""
    fr = np.random.default_rng(w * 131 + h).integers(0, 1 << bd, size=(n, w * h * 3 // 2), dtype=np.uint16)
    for qp in (22, 34):
        a, ra = O.encode(fr, w, h, bd, qp, gop=1 if lossless else 2, i_qp_offset=0 if lossless else -3, lossless=lossless, log2_ctb=log2_ctb, rows_per_slice=-1)
        b = ctx.encode(fr, w, h, bd, qp, gop=1 if lossless else 2, lossless=lossless, log2_ctb=log2_ctb, rows_per_slice=-1)
        assert a == b
        dec, dw, dh, dbd, chk, fail = ctx.decode(b)
        assert (dw, dh, dbd, chk, fail) == (w, h, bd, n, 0) and np.array_equal(dec, ra)
        if lossless: assert np.array_equal(dec, fr)


def check_wide_pictures(ctx, w):
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


def check_damaged_input(ctx, R):
    """a slice whose data is damaged must surface as an error from the chained decode -> re-encode pipeline (on the GPU the
    encoder is enqueued behind the decoder without a host round trip, so it runs on whatever the decoder left)"""
    (so, sg, sa), _ = r5_gof(128, 128, 2, 11)
    # CABAC data has no redundancy of its own: a damaged slice may decode to garbage without a syntax error. Eight damage patterns:
    # none may crash or hang, most must be caught (overrun of the slice data, impossible syntax), and the context stays usable.
    caught = 0
    for seed in range(8):
        try:
            ctx.transcode_substream(bytes(damage(sa, seed, len(sa) // 4)), R.RBT_VIDEO_ATTRIBUTE, 32)
        except R.RbtError:
            caught += 1
    assert caught >= 4
    assert ctx.transcode_substream(sg, R.RBT_VIDEO_GEOMETRY, 24) == O.transcode_substream(sg, 1, 24)


def check_more_streams_than_pipelines(ctx, R, w, h, log2_ctb):
    """more sub-bitstreams than HIP streams (4): pipelines share streams, results must not change"""
    (so, sg, sa), _ = r5_gof(w, h, 1, 33, log2_ctb)
    P = R.StreamParams
    streams = [sg, sa, sg, sa, sg, so]
    params = [P(1, 24, 4, 5, 1, 1, 0), P(19, 32, 4, 5, 1, 1, 0), P(1, 32, 4, 4, 1, 1, 0), P(19, 42, 4, 5, 0, 1, 0), P(1, 28, 4, 5, 1, 1, 1), r3_params(R)[0]]
    outs = ctx.transcode_gof(streams, params)
    assert outs[0] == O.transcode_substream(sg, 1, 24)
    assert outs[1] == O.transcode_substream(sa, 19, 32)
    assert outs[2] == O.transcode_substream(sg, 1, 32, log2_ctb=4)
    assert outs[3] == O.transcode_substream(sa, 19, 42, rows_per_slice=0)
    assert outs[4] == ctx.transcode_substream(sg, 1, 28, verify_md5=1)
    assert outs[5] == O.transcode_substream(so, 0, 8)


def check_two_gofs_in_one_call(ctx, R, gof_a, gof_b):
    """sub-bitstreams of several GOFs in one call (grouped by video type into three pipelines) give the single-GOF outputs, and those are the oracle's"""
    a, b = r5_gof(*gof_a)[0], r5_gof(*gof_b)[0]
    ps = r3_params(R)
    outs = ctx.transcode_gof(a + b, ps + ps)
    assert outs[:3] == ctx.transcode_gof(a, ps) and outs[3:] == ctx.transcode_gof(b, ps)
    assert outs[1] == O.transcode_substream(a[1], 1, 24) and outs[5] == O.transcode_substream(b[2], 19, 32)


def check_jobs_in_flight(ctx, R, gof_a, gof_b, rounds, submit_ahead, depths, damaged_job):
    """rbt_submit_gof / rbt_wait_gof: four GOFs in flight (on the GPU on disjoint HIP streams), waited for out of order, give the blocking call's outputs;
    a fifth submit is refused (RBT_ERR_BUSY) and the slots are free again afterwards; a job can be waited for once.
    submit_ahead: the steady-state walk, job i + 1 submitted before job i is waited for. damaged_job: a job that fails next to a good one.
    depths: deeper pipelines give each job fewer HIP streams (5: three, 6..8: two, 9..16: one, the parsers of pipelines that share a stream in one merged launch)."""
    a, b = r5_gof(*gof_a)[0], r5_gof(*gof_b)[0]
    ps = r3_params(R)
    want_a, want_b = ctx.transcode_gof(a, ps), ctx.transcode_gof(b, ps)
    ctx.set_depth(4)
    for _ in range(rounds):
        ja = ctx.submit_gof(a, ps); jb = ctx.submit_gof(b, ps); jc = ctx.submit_gof(b, ps); jd = ctx.submit_gof(a, ps)
        with pytest.raises(R.RbtError) as e:
            ctx.submit_gof(a, ps)
        assert e.value.code == -7
        assert ctx.wait_gof(jb) == want_b and ctx.wait_gof(jd) == want_a and ctx.wait_gof(ja) == want_a and ctx.wait_gof(jc) == want_b
    with pytest.raises(R.RbtError):          # a job can be waited for once
        ctx.wait_gof(ja)
    if submit_ahead:
        seq = [a, b, a, b, a]
        outs = []; prev = ctx.submit_gof(seq[0], ps)
        for g in seq[1:]:
            nxt = ctx.submit_gof(g, ps); outs.append(ctx.wait_gof(prev)); prev = nxt
        outs.append(ctx.wait_gof(prev))
        assert outs == [want_a, want_b, want_a, want_b, want_a]
    if damaged_job:
        dmg = damage(a[2], 3, len(a[2]) // 2)
        i = bytes(dmg).find(b"\x00\x00\x01\x42")           # the SPS: a parameter set that does not parse is an error whatever the slice data decodes to
        dmg[i + 5:i + 20] = b"\xff" * 15
        jc = ctx.submit_gof([a[0], a[1], bytes(dmg)], ps); jd = ctx.submit_gof(b, ps)
        with pytest.raises(R.RbtError):
            ctx.wait_gof(jc)
        assert ctx.wait_gof(jd) == want_b        # a failed job leaves its neighbour alone
    for depth in depths:
        ctx.set_depth(depth)
        jobs = [ctx.submit_gof(a if i % 2 == 0 else b, ps) for i in range(depth)]
        with pytest.raises(R.RbtError):
            ctx.set_depth(2)                 # refused while jobs are in flight
        for i, jb in enumerate(jobs):
            assert ctx.wait_gof(jb) == (want_a if i % 2 == 0 else want_b)
    ctx.set_depth(4)


def check_destroy_with_jobs_in_flight(R, new_ctx, gof_a, ctx=None):
    """rbt_destroy on a context that still owns submitted jobs waits for their streams and frees them; the slots are free again and the library stays usable.
    ctx: the context that takes sixteen jobs afterwards (None: a new one)"""
    a = r5_gof(*gof_a)[0]
    ps = r3_params(R)
    c1 = new_ctx()
    want = c1.transcode_gof(a, ps)
    c1.set_depth(3)
    for _ in range(3): c1.submit_gof(a, ps)
    c1.close()                                   # three jobs never waited for
    c2 = new_ctx() if ctx is None else ctx
    c2.set_depth(16)
    jobs = [c2.submit_gof(a, ps) for _ in range(16)]     # every slot is free again
    assert all(c2.wait_gof(j) == want for j in jobs)
    if ctx is None: c2.close()
    else: ctx.set_depth(4)


def occupancy_rd_cases(R):
    """(streams, params) lists for occupancy-aware coding (rbt_stream_params.occupancy_rd)"""
    P = R.StreamParams
    a, b = r5_gof(128, 128, 2, 101)[0], r5_gof(192, 128, 1, 202)[0]
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


def check_preset(ctx, R):
    """rbt_stream_params.preset (the reference's x265 preset string, PCCTranscoderParameters.h:58): RBT_PRESET_FAST leaves the round-3 decision tools out, in the library and in
    the oracle alike; HM-like input (the input's modes as candidates), every slice structure, one GOF call with both presets side by side."""
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
    quickly, by the first wave that sees it, not after a poll bound - and the context stays usable."""
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
