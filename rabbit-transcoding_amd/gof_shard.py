"""Multi-GPU host side of the transcoder: GOF sharding, rate fan-out and the gather of the re-encoded NAL units.

A V3C group of frames is self-contained (it starts with a VPS, PCCBitstreamReader.cpp:78-96, and every video sub-bitstream
restarts with an IDR), so GOFs shard across ranks with no data-path collective; the only exchange is the gather of the
re-encoded sub-bitstreams (<= ~3 MB per GOF) onto rank 0, which writes the output file (PccAppTranscoder.cpp:345-348).
One process per GPU, torch.distributed (backend "nccl" = RCCL over xGMI on ROCm, "gloo" in the CPU tests).

  transcode_sequence  BASELINE.json configs[3]: a sequence of GOFs (300 frames = 9 x 32 + 12) sharded over the ranks; mirrors the
                      per-GOF loop of PccAppTranscoder.cpp:307-341 with several GOFs in flight per GPU (rbt_submit_gof / rbt_wait_gof)
  transcode_fanout    BASELINE.json configs[4]: every rate point R1..R5 from one R5 input, one target rate per GPU (decode replicated,
                      no broadcast of decoded pictures); a rank that holds several rates decodes once and re-encodes once per rate
"""
from typing import Dict, List, Sequence

# cfg/rate/ctc-r{1..5}.cfg:5-11: geometryQP, attributeQP, occupancyPrecision
RATE_POINTS = {1: (32, 42, 4), 2: (28, 37, 4), 3: (24, 32, 4), 4: (20, 27, 4), 5: (16, 22, 2)}
VIDEO_OCCUPANCY, VIDEO_GEOMETRY, VIDEO_ATTRIBUTE = 0, 1, 19    # PCCVideoType (PCCBitstreamCommon.h:79-118)
# encoder slice structure (rbt_stream_params.ctb_rows_per_slice): wavefront mode, one slice per picture coded as one dependent slice segment per CTB row
# with entropy_coding_sync (libx265, which the reference encodes with, has wavefront rows on by default as well)
DEFAULT_ROWS = -1


def gof_lengths(n_frames: int, gof: int = 32) -> List[int]:
    """Point-cloud frames per GOF of a sequence (groupOfFramesSize, cfg/sequence/longdress_vox10.cfg:10): 300 -> 9 x 32 + 12."""
    return [min(gof, n_frames - s) for s in range(0, n_frames, gof)]


def gofs_of_rank(n_gofs: int, rank: int, world: int) -> List[int]:
    """GOF g is processed by rank g mod world (round-robin keeps ranks balanced when n_gofs is not a multiple). Same rule as
    rbt_owns_gof (include/rbt.h)."""
    return [g for g in range(n_gofs) if g % world == rank]


def rates_of_rank(rates: Sequence[int], rank: int, world: int) -> List[int]:
    """Rate fan-out: target rate i of the list goes to rank i mod world (8 GPUs, 5 rates: ranks 0..4 one rate each, 5..7 idle)."""
    return [r for i, r in enumerate(rates) if i % world == rank]


def rate_params(R, rate: int, log2_ctb: int = 5, rows_per_slice: int = DEFAULT_ROWS, md5_sei: int = 0, occupancy_rd: int = 0, preset: int = 0):
    """rbt_stream_params of the [occupancy, geometry, attribute] sub-bitstreams for CTC rate point `rate` (1..5).
    R = the rabbit_transcoding_amd module (StreamParams). md5_sei: RBT_HASH_* kind of the decoded picture hash SEI of every output picture (0 = none);
    occupancy_rd: occupancy-aware coding of the geometry and attribute maps; preset: RBT_PRESET_* (include/rbt.h)."""
    gq, aq, prec = RATE_POINTS[rate]
    P = R.StreamParams
    return [P(VIDEO_OCCUPANCY, 8, prec, log2_ctb, rows_per_slice, md5_sei, 0, 0), P(VIDEO_GEOMETRY, gq, prec, log2_ctb, rows_per_slice, md5_sei, 0, occupancy_rd, preset),
            P(VIDEO_ATTRIBUTE, aq, prec, log2_ctb, rows_per_slice, md5_sei, 0, occupancy_rd, preset)]


def gather_streams(local: Sequence[bytes], group=None, device="cpu") -> List[List[bytes]]:
    """All ranks call this with their list of byte strings (one per locally transcoded sub-bitstream, in GOF order).
    Returns on rank 0 a list indexed by rank of those lists; on other ranks an empty list.
    Two collectives per call: an all_gather of the sizes, then an all_gather of the padded payloads (RCCL has no
    gatherv; the payloads are a few MB, far below what xGMI moves in a millisecond)."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    sizes = torch.tensor([len(b) for b in local], dtype=torch.int64, device=device)
    n_local = torch.tensor([len(local)], dtype=torch.int64, device=device)
    counts = [torch.zeros(1, dtype=torch.int64, device=device) for _ in range(world)]
    dist.all_gather(counts, n_local, group=group)
    max_n = int(max(int(c.item()) for c in counts))
    sizes_p = torch.zeros(max(1, max_n), dtype=torch.int64, device=device)
    sizes_p[: len(local)] = sizes
    all_sizes = [torch.zeros(max(1, max_n), dtype=torch.int64, device=device) for _ in range(world)]
    dist.all_gather(all_sizes, sizes_p, group=group)
    totals = [int(s.sum().item()) for s in all_sizes]
    cap = max(1, max(totals))
    payload = torch.zeros(cap, dtype=torch.uint8, device=device)
    blob = b"".join(local)
    if blob:
        payload[: len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(device)
    gathered = [torch.zeros(cap, dtype=torch.uint8, device=device) for _ in range(world)]
    dist.all_gather(gathered, payload, group=group)
    if rank != 0:
        return []
    out = []
    for r in range(world):
        raw = gathered[r][: totals[r]].cpu().numpy().tobytes()
        n = int(counts[r].item())
        items, pos = [], 0
        for k in range(n):
            sz = int(all_sizes[r][k].item())
            items.append(raw[pos:pos + sz])
            pos += sz
        out.append(items)
    return out


def stitch(gathered: List[List[bytes]], n_gofs: int, streams_per_gof: int) -> List[List[bytes]]:
    """Re-orders what gather_streams returned into GOF order: result[g][s] = sub-bitstream s of GOF g."""
    world = len(gathered)
    res = [[b""] * streams_per_gof for _ in range(n_gofs)]
    for r in range(world):
        mine = gofs_of_rank(n_gofs, r, world)
        for i, g in enumerate(mine):
            for s in range(streams_per_gof):
                res[g][s] = gathered[r][i * streams_per_gof + s]
    return res


def _walk(ctx, jobs, depth):
    """Runs (streams, params) jobs through rbt_submit_gof / rbt_wait_gof with `depth` of them in flight, in order - fewer when the device memory does not hold that many:
    like rbt_transcode_v3c, a job is submitted only while free + cached - reserve holds another one of the size the largest so far took (rbt_job_memory / rbt_device_memory)."""
    depth = max(1, min(depth, 16, len(jobs) or 1))
    ctx.set_depth(depth)
    q, outs, job_bytes = [], [], 0

    def room():
        if not job_bytes: return True
        m = ctx.device_memory()
        return m["free"] + m["cached"] - m["reserve"] >= job_bytes + job_bytes // 8
    for streams, params in jobs:
        while q and (len(q) == depth or not room()):
            outs.append(ctx.wait_gof(q.pop(0)))
        q.append(ctx.submit_gof(streams, params))
        job_bytes = max(job_bytes, ctx.job_memory(q[-1]))
    while q:
        outs.append(ctx.wait_gof(q.pop(0)))
    return outs


def job_shape(n_gofs: int, max_depth: int = 16):
    """(GOFs per job, jobs in flight) for a walk of n_gofs GOFs on one GPU. A long walk keeps 16 jobs of 3 GOFs in flight (2 GOFs below 96: every job owns one hardware queue,
    several GOFs per launch fill the GPU: DESIGN.md 5); a walk shorter than 48 GOFs is all ramp-up and drain and does better as at most 7 jobs (2 up to 12 GOFs), which then own two
    or more queues each (rbt_set_depth), so that a job's geometry and attribute pipelines run side by side. Measured with tools/short_run_sweep.sh."""
    import os
    if os.environ.get("RBT_WALK_SHAPE"):                         # experiments: "G,D"
        g, d = (int(x) for x in os.environ["RBT_WALK_SHAPE"].split(","))
        return g, d
    if n_gofs >= 96:                                             # round 3: 16 x 3 GOFs 905-909 fps, 16 x 2 874-882, 12 x 4 897 (192-GOF walks); 48 GOFs of arenas are 216 GB at 1280x1280
        return 3, max(1, min(max_depth, 16))
    if n_gofs >= 48:
        return 2, max(1, min(max_depth, 16))
    jobs = 2 if n_gofs <= 12 else 7                              # measured on one MI355X: 10 GOFs 470 / 544 / 573 / 601 / 563 fps as 10 / 5 / 3 / 2 / 1 jobs; 20 GOFs 484 / 650 / 798 / 784 / 731
    g = max(1, (n_gofs + jobs - 1) // jobs)                      # as 16 / 10 / 7 / 5 / 4 jobs; 40 GOFs 769 / 843 / 848 / 843 / 831 as 20 / 14 / 10 / 7 / 5 jobs
    return g, max(1, min(max_depth, 16, (n_gofs + g - 1) // g))


def spread(n: int, g: int) -> List[int]:
    """n GOFs over ceil(n / g) jobs, as evenly as possible: 20, 3 -> 3 3 3 3 3 3 2"""
    nj = (n + g - 1) // g
    return [n // nj + (1 if i < n % nj else 0) for i in range(nj)] if nj else []


def transcode_sequence(ctx, gofs: Sequence[Sequence[bytes]], params, rank: int = 0, world: int = 1, depth: int = 16, group=None, device="cpu", gofs_per_job: int = 1):
    """configs[3]. gofs[g] = [occupancy, geometry, attribute] Annex-B sub-bitstreams of GOF g; every rank holds the whole compressed
    input (PccAppTranscoder loads the file first, PccAppTranscoder.cpp:289). Each rank transcodes the GOFs its context owns
    (rbt_owns_gof) with up to `depth` jobs in flight, `gofs_per_job` consecutive GOFs of its share per job (0: both by job_shape); the outputs
    are gathered on rank 0. Returns on rank 0 the output in GOF order (result[g][s]), None elsewhere. world == 1 needs no process group."""
    n = len(gofs)
    mine = [g for g in range(n) if ctx.owns_gof(g)]
    assert mine == gofs_of_rank(n, rank, world)
    if gofs_per_job <= 0:
        gofs_per_job, depth = job_shape(len(mine), depth)
    jobs, pos = [], 0
    for sz in spread(len(mine), max(1, gofs_per_job)):
        jobs.append(([s for g in mine[pos:pos + sz] for s in gofs[g]], list(params) * sz)); pos += sz
    outs = _walk(ctx, jobs, depth)
    local = [s for o in outs for s in o]
    if world == 1:
        return stitch([local], n, len(params))
    gathered = gather_streams(local, group=group, device=device)
    return stitch(gathered, n, len(params)) if rank == 0 else None


def transcode_fanout(ctx, R, gofs: Sequence[Sequence[bytes]], rates: Sequence[int] = (1, 2, 3, 4, 5), rank: int = 0, world: int = 1, depth: int = 16,
                     group=None, device="cpu", **enc) -> Dict[int, List[List[bytes]]]:
    """configs[4]. Every GOF of the sequence is transcoded to every rate point of `rates`; rate i belongs to rank i mod world
    (rates_of_rank). A rank with several rates hands each GOF over once with all its rates (the library decodes identical inputs once).
    Returns on rank 0 {rate: result[g][s]}, None elsewhere."""
    mine = rates_of_rank(rates, rank, world)
    jobs = []
    for g in gofs:
        streams, params = [], []
        for r in mine:
            streams += list(g)
            params += rate_params(R, r, **enc)
        if streams:
            jobs.append((streams, params))
    outs = _walk(ctx, jobs, depth) if jobs else []
    local = [s for o in outs for s in o]             # per GOF: rate-major, then [occ, geo, attr]
    gathered = [local] if world == 1 else gather_streams(local, group=group, device=device)
    if rank != 0:
        return None
    res = {}
    for rk in range(world):
        rs = rates_of_rank(rates, rk, world)
        for gi in range(len(gofs)):
            for ri, r in enumerate(rs):
                base = (gi * len(rs) + ri) * 3
                res.setdefault(r, []).append(gathered[rk][base:base + 3])
    return res


def wrap_v3c(R, gofs: Sequence[Sequence[bytes]], precision_bytes: int = 0, lib=None) -> bytes:
    """A V3C sample stream around a sequence of [occupancy, geometry, attribute] Annex-B GOFs: per GOF the units PCCBitstreamWriter::encode emits for a
    single-atlas, single-stream sequence (:96-237) - V3C_VPS, V3C_AD, V3C_OVD, V3C_GVD, V3C_AVD with the unit headers of :309-333. The parameter set and
    atlas payloads are placeholders (the transcoder carries those units over unread); used where a container is wanted around synthetic video."""
    import struct
    units = []
    for g, s in enumerate(gofs):
        units.append(struct.pack(">I", 0 << 27) + bytes([g & 255]) * 32)
        units.append(struct.pack(">I", 1 << 27) + bytes([(g + 1) & 255]) * 2048)
        for t, b in zip((2, 3, 4), s):
            units.append(struct.pack(">I", t << 27) + R.byte_to_sample_stream(b, lib))
    return R.v3c_write(units, precision_bytes, lib)


def unwrap_v3c(R, data: bytes, lib=None, annexb: bool = True) -> List[List[bytes]]:
    """The video units of a V3C sample stream: result[g] = the [occupancy, geometry, attribute] sub-bitstreams of GOF g, as Annex-B byte streams
    (sampleStreamToByteStream, which chooses start code lengths by its own rule: not the inverse of byteStreamToSampleStream byte for byte) or, with
    annexb=False, in the sample stream form they are stored in."""
    out = {}
    for u in R.v3c_index(data, lib):
        if u["video_type"] >= 0:
            payload = data[u["offset"] + 4:u["offset"] + u["size"]]
            out.setdefault(u["gof"], []).append(R.sample_to_byte_stream(payload, lib) if annexb else payload)
    return [out[g] for g in sorted(out)]


def merge_v3c(R, parts: Sequence[bytes], forced_precision_bytes: int = 0, lib=None) -> bytes:
    """Merges the V3C sample streams the ranks made of one input (rbt_transcode_v3c with world_size = len(parts): part r holds the GOFs r, r + world, ...
    in order) into the stream one rank would have written: units in GOF order, unit size precision by the writer's rule over ALL units
    (PCCBitstreamWriter::write is called once, after the last GOF: PccAppTranscoder.cpp:343-348)."""
    world = len(parts)
    per_rank = []
    for p in parts:
        gofs = {}
        for u in R.v3c_index(p, lib):
            gofs.setdefault(u["gof"], []).append(p[u["offset"]:u["offset"] + u["size"]])
        per_rank.append([gofs[k] for k in sorted(gofs)])
    units, g = [], 0
    while any(g // world < len(per_rank[r]) for r in range(world) if g % world == r):
        units += per_rank[g % world][g // world]
        g += 1
    assert g == sum(len(x) for x in per_rank), "ranks do not hold a round-robin split of one stream"
    return R.v3c_write(units, forced_precision_bytes, lib)


def transcode_v3c(ctx, R, data: bytes, geometry_qp: int, attribute_qp: int, rank: int = 0, world: int = 1, depth: int = 16, group=None, device="cpu", **kw):
    """The container form of transcode_sequence: every rank holds the input file (PccAppTranscoder.cpp:289), transcodes the GOFs its context owns
    (rbt_transcode_v3c; gofs_per_job=0 lets the library cut them into jobs by rbt_job_shape, with `depth` as the cap), rank 0 gathers the partial streams and
    writes the output. Returns the output on rank 0, None elsewhere."""
    ctx.set_depth(max(1, min(depth, 16)))
    part = ctx.transcode_v3c(data, geometry_qp, attribute_qp, **kw)
    if world == 1:
        return part
    gathered = gather_streams([part], group=group, device=device)
    return merge_v3c(R, [g[0] for g in gathered], kw.get("forced_precision_bytes", 0), lib=ctx.L) if rank == 0 else None


def split_pairs(stream: bytes) -> List[bytes]:
    """Splits an Annex-B sub-bitstream made of closed GOPs, each starting with its own VPS (parameter sets repeated with every IDR,
    as libx265 does behind PCCTranscoder.cpp:706 and as the CTC streams do), into one byte string per closed GOP. Used to cut the
    12-frame tail GOF of a 300-frame sequence out of a 32-frame one and to make the GOFs of a synthetic sequence differ."""
    cuts, i = [], stream.find(b"\x00\x00\x01")
    while i >= 0:
        if (stream[i + 3] >> 1) & 63 == 32:          # VPS
            cuts.append(i - 1 if i > 0 and stream[i - 1] == 0 else i)
        i = stream.find(b"\x00\x00\x01", i + 3)
    if not cuts or cuts[0] != 0: raise ValueError("stream does not start with a VPS")
    cuts.append(len(stream))
    return [stream[a:b] for a, b in zip(cuts, cuts[1:])]


def access_units(stream: bytes) -> List[bytes]:
    """An Annex-B sub-bitstream cut into access units (7.4.2.4.4): a unit starts at the first parameter set / AUD / prefix SEI after the last slice segment of the
    picture before it, or at a slice segment with first_slice_segment_in_pic_flag; suffix SEI (the hash of the CTC streams) stay with their picture."""
    starts, i = [], stream.find(b"\x00\x00\x01")
    while i >= 0:
        starts.append(i)
        i = stream.find(b"\x00\x00\x01", i + 3)
    cuts, have_vcl = [], False
    for i in starts:
        t = (stream[i + 3] >> 1) & 63
        at = i - 1 if i > 0 and stream[i - 1] == 0 else i            # a four-byte start code belongs to its NAL unit
        if t < 32:
            if i + 5 < len(stream) and stream[i + 5] & 0x80 and (have_vcl or not cuts): cuts.append(at)
            have_vcl = True
        elif t in (32, 33, 34, 35, 39) or 41 <= t <= 44 or 48 <= t <= 55:
            if have_vcl or not cuts: cuts.append(at); have_vcl = False
    cuts = sorted(set(cuts)) + [len(stream)]
    return [stream[a:b] for a, b in zip(cuts, cuts[1:])]


def parameter_sets(stream: bytes) -> bytes:
    """The VPS / SPS / PPS NAL units in front of the first picture."""
    i, end = stream.find(b"\x00\x00\x01"), 0
    while i >= 0:
        if not 32 <= ((stream[i + 3] >> 1) & 63) <= 34: break
        nxt = stream.find(b"\x00\x00\x01", i + 3)
        end = len(stream) if nxt < 0 else (nxt - 1 if stream[nxt - 1] == 0 else nxt)
        i = nxt
    return stream[:end]


def is_closed_pairs(stream: bytes) -> bool:
    """True for a stream of closed groups that each bring their parameter sets (what split_pairs cuts); False for the structure of the CTC's HM encoder - ONE IDR
    with the parameter sets, then trailing pictures with POC running on (cfg/hm/ctc-hm-geometry-ai.cfg:21-30): such a stream has no cut points."""
    return stream.count(b"\x00\x00\x01\x40\x01") > 1


def first_pictures(stream: bytes, n: int) -> bytes:
    """The first n pictures of a sub-bitstream (whole access units). A prefix of a stream is a stream in either structure."""
    return b"".join(access_units(stream)[:n])


def frame_pieces(stream: bytes, pictures_per_frame: int) -> List[bytes]:
    """One byte string per point-cloud frame (pictures_per_frame pictures: 2 maps, 1 occupancy picture), each handed to a decoder on its own: the closed groups of a
    closed stream as they are; for the CTC structure (pictures reference nothing outside their frame, but only the first frame carries parameter sets and an IRAP
    picture) the parameter sets are put in front of every later frame - a decoder that does not insist on an IRAP start (this library, the oracle) reads them alike."""
    if is_closed_pairs(stream):
        return split_pairs(stream)
    aus, ps = access_units(stream), parameter_sets(stream)
    return [(b"" if k == 0 else ps) + b"".join(aus[k:k + pictures_per_frame]) for k in range(0, len(aus), pictures_per_frame)]


def make_sequence(gof: Sequence[bytes], n_frames: int, gof_size: int = 32) -> List[List[bytes]]:
    """A synthetic sequence of ceil(n_frames / gof_size) GOFs from ONE [occupancy, geometry, attribute] GOF of gof_size frames:
    GOF g holds the point-cloud frames (7 g + i) mod gof_size, i < its length - every GOF differs and the last one is shorter
    (300 frames -> 9 x 32 + 12). Valid because every point-cloud frame is a closed GOP in all three sub-bitstreams.
    A GOF in the structure of the CTC's HM encoder (one IDR per sub-bitstream, is_closed_pairs false) cannot be re-ordered: there GOF g is the first
    min(gof_size, frames left) frames of the given one (the GOFs only differ in length)."""
    if not any(is_closed_pairs(s) for s in gof):
        pics = [len(access_units(s)) for s in gof]
        if any(p % gof_size for p in pics): raise ValueError(f"sub-bitstreams of {pics} pictures do not hold {gof_size} point-cloud frames")
        return [[first_pictures(s, n * (p // gof_size)) for s, p in zip(gof, pics)] for n in gof_lengths(n_frames, gof_size)]
    if not all(is_closed_pairs(s) for s in gof): raise ValueError("sub-bitstreams of one GOF in different structures (closed groups and the CTC encoder's)")
    parts = [split_pairs(s) for s in gof]
    assert all(len(p) == gof_size for p in parts), [len(p) for p in parts]
    seq = []
    for g, n in enumerate(gof_lengths(n_frames, gof_size)):
        idx = [(7 * g + i) % gof_size for i in range(n)]
        seq.append([b"".join(p[k] for k in idx) for p in parts])
    return seq
