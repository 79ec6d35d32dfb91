"""rabbit-transcoding_amd: ctypes binding of librbt.so (include/rbt.h), the MI355X-native V-PCC transcoding hot path.

The package directory name contains a hyphen (mandated layout), so load it with
    importlib.util.spec_from_file_location("rabbit_transcoding_amd", ".../rabbit-transcoding_amd/__init__.py")
or through tests/rbt_lib.py. There is no CPU fallback: creating a Context without a HIP device raises RbtError.
"""
import ctypes as C
import os
import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RBT_LIB_PATH") or os.path.join(_DIR, "librbt.so")   # RBT_LIB_PATH: another build of the same library (experiments)

RBT_VIDEO_OCCUPANCY, RBT_VIDEO_GEOMETRY, RBT_VIDEO_ATTRIBUTE = 0, 1, 19
RBT_ERR_NOMEM, RBT_ERR_OUTPUT = -5, -8   # device (or host) memory ran out / a slice's coded data is larger than the output buffer sized for it
RBT_HASH_NONE, RBT_HASH_MD5, RBT_HASH_CRC, RBT_HASH_CHECKSUM = 0, 1, 2, 3   # md5_sei: kind of decoded picture hash SEI (HM / x265 numbering)


class RbtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rbt error {code}: {msg}")
        self.code = code


class Memory(C.Structure):
    """rbt_memory (include/rbt.h)"""
    _fields_ = [(n, C.c_size_t) for n in ("total_bytes", "free_bytes", "cached_bytes", "in_use_bytes", "reserve_bytes")]


class StreamParams(C.Structure):
    _fields_ = [("video_type", C.c_int), ("qp", C.c_int), ("occupancy_precision", C.c_int), ("log2_ctb", C.c_int),
                ("ctb_rows_per_slice", C.c_int), ("md5_sei", C.c_int), ("verify_md5", C.c_int), ("occupancy_rd", C.c_int), ("preset", C.c_int)]


class Video(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bit_depth", C.c_int), ("n_frames", C.c_int),
                ("data", C.POINTER(C.c_uint16)), ("md5_checked", C.c_int), ("md5_failed", C.c_int)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("host_parse_ms", "h2d_ms", "gpu_ms", "d2h_ms", "host_pack_ms", "total_ms", "k_parse_ms",
                                          "k_recon_ms", "k_filter_ms", "k_analyse_ms", "k_encode_ms", "k_entropy_ms")] + [("algorithmic_bytes", C.c_uint64)]


class Patch(C.Structure):
    """rbt_patch: the fields of PCCPatch the reconstruction reads"""
    _fields_ = [(n, C.c_int32) for n in ("u0", "v0", "size_u0", "size_v0", "u1", "v1", "d1", "normal_axis", "tangent_axis", "bitangent_axis", "projection_mode", "orientation", "lod_x", "lod_y")]


class AtlasParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "occupancy_resolution", "occupancy_precision", "map_count", "absolute_d1", "remove_duplicate_points", "threshold_lossy_om",
                                            "geometry_smoothing", "grid_size", "threshold_smoothing")]      # the last three default to 0 = no smoothing; CTC: 1, 8, 64


def ctc_smoothing(atlas):
    """the same atlas with the geometry smoothing of the CTC switched on (cfg/common/ctc-common.cfg:57-60: gridSmoothing, gridSize 8, thresholdSmoothing 64)"""
    a = AtlasParams(*[getattr(atlas, n) for n, _ in AtlasParams._fields_])
    a.geometry_smoothing, a.grid_size, a.threshold_smoothing = 1, 8, 64
    return a


class Cloud(C.Structure):
    _fields_ = [("n_points", C.c_int), ("xyz", C.POINTER(C.c_int16)), ("yuv", C.POINTER(C.c_uint16)), ("occupancy_map", C.POINTER(C.c_uint8)), ("block_to_patch", C.POINTER(C.c_uint32)), ("n_smoothed", C.c_int)]


class D1Result(C.Structure):
    _fields_ = [("n_a", C.c_int), ("n_b", C.c_int), ("sse_ab", C.c_uint64), ("sse_ba", C.c_uint64), ("max_ab", C.c_uint64), ("max_ba", C.c_uint64),
                ("mse_ab", C.c_float), ("mse_ba", C.c_float), ("psnr_ab", C.c_float), ("psnr_ba", C.c_float), ("psnr", C.c_float)]


class D2Result(C.Structure):
    _fields_ = [("n_a", C.c_int), ("n_b", C.c_int), ("sse_ab", C.c_double), ("sse_ba", C.c_double), ("max_ab", C.c_double), ("max_ba", C.c_double),
                ("mse_ab", C.c_float), ("mse_ba", C.c_float), ("psnr_ab", C.c_float), ("psnr_ba", C.c_float), ("psnr", C.c_float)]


class ColorResult(C.Structure):
    """rbt_color_result: [Y, U, V] per field"""
    _fields_ = [("n_a", C.c_int), ("n_b", C.c_int), ("sse_ab", C.c_uint64 * 3), ("sse_ba", C.c_uint64 * 3)] + \
               [(n, C.c_float * 3) for n in ("mse_ab", "mse_ba", "psnr_ab", "psnr_ba", "mse", "psnr")]


RBT_SCORE_D1, RBT_SCORE_D2, RBT_SCORE_COLOR = 1, 2, 4


class PatchD1(C.Structure):
    """rbt_patch_d1: the D1 sums and figures of one patch of the decoded cloud (rbt_score_patches)"""
    _fields_ = [("n_ab", C.c_uint32), ("n_ba", C.c_uint32), ("sse_ab", C.c_uint64), ("sse_ba", C.c_uint64), ("max_ab", C.c_uint64), ("max_ba", C.c_uint64),
                ("mse_ab", C.c_float), ("mse_ba", C.c_float), ("psnr", C.c_float)]


def patch_d1_dict(p):
    return {k: getattr(p, k) for k, _ in PatchD1._fields_}


class PatchD2(C.Structure):
    """rbt_patch_d2: the D2 sums and figures of one patch of the decoded cloud (rbt_score_patches_d2)"""
    _fields_ = [("n_ab", C.c_uint32), ("n_ba", C.c_uint32), ("sse_ab", C.c_double), ("sse_ba", C.c_double), ("max_ab", C.c_double), ("max_ba", C.c_double),
                ("mse_ab", C.c_float), ("mse_ba", C.c_float), ("psnr", C.c_float)]


def patch_d2_dict(p):
    return {k: getattr(p, k) for k, _ in PatchD2._fields_}


class PatchColor(C.Structure):
    """rbt_patch_color: the colour sums and figures of one patch of the decoded cloud (rbt_score_patches_color), [Y, U, V] per array field"""
    _fields_ = [("n_ab", C.c_uint32), ("n_ba", C.c_uint32), ("sse_ab", C.c_uint64 * 3), ("sse_ba", C.c_uint64 * 3)] + [(n, C.c_float * 3) for n in ("mse_ab", "mse_ba", "mse", "psnr")]


def patch_color_dict(p):
    return {k: (list(getattr(p, k)) if isinstance(getattr(p, k), C.Array) else getattr(p, k)) for k, _ in PatchColor._fields_}


class FrameScore(C.Structure):
    """rbt_frame_score: what rbt_score returns for one pair of clouds"""
    _fields_ = [("parts", C.c_int), ("d1", D1Result), ("d2", D2Result), ("color", ColorResult), ("device_ms", C.c_double)] + \
               [(n, C.c_int) for n in ("n_points_a", "n_points_b", "n_merged_a", "n_merged_b")]


class SequenceScore(C.Structure):
    """rbt_sequence_score: mean and minimum of the per-frame symmetric PSNRs"""
    _fields_ = [(n, C.c_int) for n in ("n_frames", "n_d1", "n_d2", "n_color")] + [(n, C.c_double) for n in ("mean_d1", "min_d1", "mean_d2", "min_d2")] + \
               [("mean_color", C.c_double * 3), ("min_color", C.c_double * 3)] + [(n, C.c_int64) for n in ("points_a", "points_b", "merged_a", "merged_b")]


RBT_UPSAMPLE_REPLICATE, RBT_UPSAMPLE_F0 = -1, 0   # rbt_yuv420_to_yuv444 / rbt_reconstruct_rgb: sample replication / g_filter420to444[0], the decoder's default


class V3CUnit(C.Structure):
    """rbt_v3c_unit: one unit of a V3C sample stream"""
    _fields_ = [(n, C.c_int) for n in ("type", "gof", "parameter_set_id", "atlas_id", "attribute_index", "attribute_dimension_index", "map_index", "auxiliary_video", "video_type")] + \
               [("offset", C.c_size_t), ("size", C.c_size_t)]


class V3CParams(C.Structure):
    """rbt_v3c_params: PCCTranscoderParameters as the container walk needs them"""
    _fields_ = [(n, C.c_int) for n in ("occupancy_precision", "geometry_qp", "attribute_qp", "forced_unit_size_precision_bytes", "log2_ctb", "ctb_rows_per_slice", "md5_sei", "verify_md5", "gofs_per_job", "occupancy_rd", "preset")]


class V3CStat(C.Structure):
    """rbt_v3c_stat: PCCBitstreamStat of a V3C sample stream"""
    _fields_ = [("n_units", C.c_int), ("n_gofs", C.c_int), ("unit_size_precision_bytes", C.c_int), ("header", C.c_uint64), ("unit_size", C.c_uint64 * 5)] + \
               [(n, C.c_uint64) for n in ("occupancy_video", "geometry_video", "geometry_aux_video", "attribute_video", "attribute_aux_video", "total_metadata", "total_geometry", "total_attribute", "total")]


class RateTarget(C.Structure):
    """rbt_rate_target; struct_size is filled in. target_bytes 0 = constant QP, qp_max 0 = 51"""
    _fields_ = [("struct_size", C.c_uint32), ("target_bytes", C.c_uint64), ("qp_min", C.c_int), ("qp_max", C.c_int)]

    def __init__(self, target_bytes=0, qp_min=0, qp_max=0):
        super().__init__(C.sizeof(RateTarget), target_bytes, qp_min, qp_max)


class RateResult(C.Structure):
    """rbt_rate_result: q*, the estimate it started from, met, trial encodes, s(q*), E(estimate)"""
    _fields_ = [("qp", C.c_int), ("qp_estimate", C.c_int), ("met", C.c_int), ("n_encodes", C.c_int), ("bytes", C.c_uint64), ("estimate_bytes", C.c_uint64)]


class FrameQp(C.Structure):
    """rbt_frame_qp: one QP per point-cloud frame of an entry; struct_size is filled in. No argument (or an empty list) = no list: the entry is coded at its own QP"""
    _fields_ = [("struct_size", C.c_uint32), ("n_frames", C.c_int), ("qp", C.POINTER(C.c_int8))]

    def __init__(self, qps=None):
        qps = list(qps or [])
        self._keep = (C.c_int8 * max(1, len(qps)))(*qps)
        super().__init__(C.sizeof(FrameQp), len(qps), self._keep if qps else None)


class QpMap(C.Structure):
    """rbt_qp_map: one QP per CTB and point-cloud frame of an entry, from an integer array M[f][r][c] (n_frames x h_ctb x w_ctb); struct_size is filled in. No argument = no
    map: the entry is coded at its own QP"""
    _fields_ = [("struct_size", C.c_uint32), ("n_frames", C.c_int), ("w_ctb", C.c_int), ("h_ctb", C.c_int), ("qp", C.POINTER(C.c_int8))]

    def __init__(self, m=None):
        if m is None:
            self._keep = None
            super().__init__(C.sizeof(QpMap), 0, 0, 0, None)
            return
        m = np.ascontiguousarray(np.asarray(m), dtype=np.int8)
        if m.ndim != 3:
            raise ValueError("a QP map is M[f][r][c]: three dimensions")
        self._keep = m
        super().__init__(C.sizeof(QpMap), m.shape[0], m.shape[2], m.shape[1], m.ctypes.data_as(C.POINTER(C.c_int8)))


RBT_QUALITY_ALL, RBT_QUALITY_OCCUPIED = 0, 1


class QualityTarget(C.Structure):
    """rbt_quality_target; struct_size is filled in. min_psnr_mdb 0 = no floor (coded at the entry's QP, distortion reported), qp_max 0 = 51"""
    _fields_ = [("struct_size", C.c_uint32), ("min_psnr_mdb", C.c_int32), ("region", C.c_int), ("qp_min", C.c_int), ("qp_max", C.c_int)]

    def __init__(self, min_psnr_mdb=0, region=RBT_QUALITY_ALL, qp_min=0, qp_max=0):
        super().__init__(C.sizeof(QualityTarget), min_psnr_mdb, region, qp_min, qp_max)


class QualityResult(C.Structure):
    """rbt_quality_result: q*, the probe q0, the walk's start qs, met, distinct QPs encoded, the stream's size, its sums and PSNRs (Y, Cb, Cr; all samples and occupied)"""
    _fields_ = [("qp", C.c_int), ("qp_probe", C.c_int), ("qp_start", C.c_int), ("met", C.c_int), ("n_encodes", C.c_int), ("bytes", C.c_uint64),
                ("sse", C.c_uint64 * 3), ("samples", C.c_uint64 * 3), ("sse_occ", C.c_uint64 * 3), ("samples_occ", C.c_uint64 * 3), ("psnr", C.c_double * 3), ("psnr_occ", C.c_double * 3)]


class FramePick(C.Structure):
    """rbt_frame_pick: q*_f, qs_f, met_f, distinct QPs encoded for the frame, the frame's bytes in the returned stream, its figure at q*_f"""
    _fields_ = [("qp", C.c_int), ("qp_start", C.c_int), ("met", C.c_int), ("n_encodes", C.c_int), ("bytes", C.c_uint64), ("figure", C.c_double)]


class FrameFloorResult(C.Structure):
    """rbt_frame_floor_result: the picks per frame, the probe q0, met_all, the passes, the stream's size, the pictures encoded, the stream's sums"""
    _fields_ = [("n_frames", C.c_int), ("qp_probe", C.c_int), ("met_all", C.c_int), ("n_passes", C.c_int), ("bytes", C.c_uint64), ("pictures_encoded", C.c_uint64),
                ("frames", C.POINTER(FramePick)), ("sums", QualityResult), ("d1", C.POINTER(D1Result)), ("cloud_ms", C.c_double)]


class PatchFloorTarget(C.Structure):
    """rbt_patch_floor_target; struct_size is filled in. PatchFloorTarget() is the empty target of an entry without one. patches: one list of Patch per point-cloud frame;
    patch_floors: None, or per frame None / one floor in 1/1000 dB per patch (F_k; else min_psnr_mdb). The object keeps the arrays it points to alive."""
    _fields_ = [("struct_size", C.c_uint32), ("min_psnr_mdb", C.c_int32), ("region", C.c_int), ("qp_min", C.c_int), ("qp_max", C.c_int), ("background_qp", C.c_int), ("max_trials", C.c_int),
                ("atlas", AtlasParams), ("n_frames", C.c_int), ("patches", C.POINTER(C.POINTER(Patch))), ("n_patches", C.POINTER(C.c_int)), ("patch_min_psnr_mdb", C.POINTER(C.POINTER(C.c_int32)))]

    def __init__(self, atlas=None, patches=None, min_psnr_mdb=0, region=RBT_QUALITY_ALL, qp_min=0, qp_max=0, background_qp=-1, max_trials=0, patch_floors=None):
        super().__init__(C.sizeof(PatchFloorTarget))
        self._keep = []
        if atlas is None:
            return
        self.min_psnr_mdb, self.region, self.qp_min, self.qp_max, self.background_qp, self.max_trials = min_psnr_mdb, region, qp_min, qp_max, background_qp, max_trials
        self.atlas = AtlasParams(*[getattr(atlas, n) for n, _ in AtlasParams._fields_])
        self.n_frames = len(patches)
        lists = [(Patch * max(1, len(p)))(*p) for p in patches]
        ptrs = (C.POINTER(Patch) * max(1, len(lists)))(*[C.cast(a, C.POINTER(Patch)) for a in lists])
        counts = (C.c_int * max(1, len(lists)))(*[len(p) for p in patches])
        self.patches, self.n_patches = ptrs, counts
        self._keep += [lists, ptrs, counts]
        if patch_floors is not None:
            fl = [None if f is None else (C.c_int32 * max(1, len(f)))(*f) for f in patch_floors]
            fp = (C.POINTER(C.c_int32) * max(1, len(fl)))(*[None if a is None else C.cast(a, C.POINTER(C.c_int32)) for a in fl])
            self.patch_min_psnr_mdb = fp
            self._keep += [fl, fp]


class PatchPick(C.Structure):
    """rbt_patch_pick: of a frame's settling trial, per patch: its QP, met, failed, the sums of its region in the chosen region of samples, its figure"""
    _fields_ = [("qp", C.c_int), ("met", C.c_int), ("failed", C.c_int), ("sse", C.c_uint64), ("samples", C.c_uint64), ("figure", C.c_double)]


class PatchFrame(C.Structure):
    """rbt_patch_frame: trials, met, the patch count, the frame's bytes, the background's {sse, sse_occ, n_occ}, the picks"""
    _fields_ = [("n_trials", C.c_int), ("met", C.c_int), ("n_patches", C.c_int), ("bytes", C.c_uint64), ("background", C.c_uint64 * 3), ("patches", C.POINTER(PatchPick))]


class PatchFloorResult(C.Structure):
    """rbt_patch_floor_result: frames, the probe q0, met_all, the passes, the stream's size, the pictures encoded, the grid, the final map, the frames, the stream's sums"""
    _fields_ = [("n_frames", C.c_int), ("qp_probe", C.c_int), ("met_all", C.c_int), ("n_passes", C.c_int), ("bytes", C.c_uint64), ("pictures_encoded", C.c_uint64), ("w_ctb", C.c_int), ("h_ctb", C.c_int),
                ("map", C.POINTER(C.c_int8)), ("frames", C.POINTER(PatchFrame)), ("picks", C.POINTER(PatchPick)), ("sums", QualityResult)]


RBT_D1_MIN, RBT_D1_MEAN = 0, 1


class D1Target(C.Structure):
    """rbt_d1_target; struct_size is filled in. D1Target() is the empty target of an entry without one. patches: one list of Patch per point-cloud frame; reference: None,
    or one PCloud (or None = the cloud of the decoded input) per frame. The object keeps the arrays it points to alive."""
    _fields_ = [("struct_size", C.c_uint32), ("min_d1_mdb", C.c_int32), ("stat", C.c_int), ("peak", C.c_int), ("qp_min", C.c_int), ("qp_max", C.c_int), ("n_frames", C.c_int),
                ("atlas", AtlasParams), ("patches", C.POINTER(C.POINTER(Patch))), ("n_patches", C.POINTER(C.c_int)), ("reference", C.POINTER(C.c_void_p))]

    def __init__(self, atlas=None, patches=None, min_d1_mdb=0, stat=RBT_D1_MIN, qp_min=0, qp_max=0, peak=0, reference=None):
        super().__init__(C.sizeof(D1Target), min_d1_mdb, stat, peak, qp_min, qp_max)
        self._keep = []
        if atlas is None:
            return
        self.atlas = AtlasParams(*[getattr(atlas, n) for n, _ in AtlasParams._fields_])
        self.n_frames = len(patches)
        lists = [(Patch * max(1, len(p)))(*p) for p in patches]
        ptrs = (C.POINTER(Patch) * max(1, len(lists)))(*[C.cast(a, C.POINTER(Patch)) for a in lists])
        counts = (C.c_int * max(1, len(lists)))(*[len(p) for p in patches])
        self.patches, self.n_patches = ptrs, counts
        self._keep += [lists, ptrs, counts]
        if reference is not None:
            refs = (C.c_void_p * max(1, len(reference)))(*[None if r is None else (r.h.value if isinstance(r, PCloud) else r) for r in reference])
            self.reference = refs
            self._keep += [refs, list(reference)]


class PatchD1Target(C.Structure):
    """rbt_patch_d1_target; struct_size is filled in. PatchD1Target() is the empty target of an entry without one. patches: one list of Patch per point-cloud frame;
    patch_floors: None, or per frame None / one floor in 1/1000 dB per patch (F_k; else min_d1_mdb); reference: None, or one PCloud (or None = the cloud of the decoded
    input) per frame. The object keeps the arrays it points to alive."""
    _fields_ = [("struct_size", C.c_uint32), ("min_d1_mdb", C.c_int32), ("peak", C.c_int), ("qp_min", C.c_int), ("qp_max", C.c_int), ("background_qp", C.c_int), ("max_trials", C.c_int),
                ("atlas", AtlasParams), ("n_frames", C.c_int), ("patches", C.POINTER(C.POINTER(Patch))), ("n_patches", C.POINTER(C.c_int)), ("patch_min_d1_mdb", C.POINTER(C.POINTER(C.c_int32))),
                ("reference", C.POINTER(C.c_void_p))]

    def __init__(self, atlas=None, patches=None, min_d1_mdb=0, peak=0, qp_min=0, qp_max=0, background_qp=-1, max_trials=0, patch_floors=None, reference=None):
        super().__init__(C.sizeof(PatchD1Target))
        self._keep = []
        if atlas is None:
            return
        self.min_d1_mdb, self.peak, self.qp_min, self.qp_max, self.background_qp, self.max_trials = min_d1_mdb, peak, qp_min, qp_max, background_qp, max_trials
        self.atlas = AtlasParams(*[getattr(atlas, n) for n, _ in AtlasParams._fields_])
        self.n_frames = len(patches)
        lists = [(Patch * max(1, len(p)))(*p) for p in patches]
        ptrs = (C.POINTER(Patch) * max(1, len(lists)))(*[C.cast(a, C.POINTER(Patch)) for a in lists])
        counts = (C.c_int * max(1, len(lists)))(*[len(p) for p in patches])
        self.patches, self.n_patches = ptrs, counts
        self._keep += [lists, ptrs, counts]
        if patch_floors is not None:
            fl = [None if f is None else (C.c_int32 * max(1, len(f)))(*f) for f in patch_floors]
            fp = (C.POINTER(C.c_int32) * max(1, len(fl)))(*[None if a is None else C.cast(a, C.POINTER(C.c_int32)) for a in fl])
            self.patch_min_d1_mdb = fp
            self._keep += [fl, fp]
        if reference is not None:
            refs = (C.c_void_p * max(1, len(reference)))(*[None if r is None else (r.h.value if isinstance(r, PCloud) else r) for r in reference])
            self.reference = refs
            self._keep += [refs, list(reference)]


class PatchD1Pick(C.Structure):
    """rbt_patch_d1_pick: of a frame's settling trial, per patch: its QP, met, failed, its PatchD1, its figure"""
    _fields_ = [("qp", C.c_int), ("met", C.c_int), ("failed", C.c_int), ("d1", PatchD1), ("figure", C.c_double)]


class PatchD1Frame(C.Structure):
    """rbt_patch_d1_frame: trials, met, the patch count, the frame's bytes, the whole frame's D1Result in the settling trial, the picks"""
    _fields_ = [("n_trials", C.c_int), ("met", C.c_int), ("n_patches", C.c_int), ("bytes", C.c_uint64), ("d1", D1Result), ("patches", C.POINTER(PatchD1Pick))]


class PatchD1Result(C.Structure):
    """rbt_patch_d1_result: frames, the probe q0, met_all, the passes, the stream's size, the pictures encoded, the grid, the final map, the frames, the picks, device
    milliseconds of the clouds"""
    _fields_ = [("n_frames", C.c_int), ("qp_probe", C.c_int), ("met_all", C.c_int), ("n_passes", C.c_int), ("bytes", C.c_uint64), ("pictures_encoded", C.c_uint64), ("w_ctb", C.c_int), ("h_ctb", C.c_int),
                ("map", C.POINTER(C.c_int8)), ("frames", C.POINTER(PatchD1Frame)), ("picks", C.POINTER(PatchD1Pick)), ("cloud_ms", C.c_double)]


class D1FloorResult(C.Structure):
    """rbt_d1_floor_result: q*, the probe q0, the walk's start qs, met, distinct QPs encoded, the stream's size, mean and minimum D1 over the frames, the frames' D1Result
    (freed by the binding), device milliseconds of the clouds"""
    _fields_ = [("qp", C.c_int), ("qp_probe", C.c_int), ("qp_start", C.c_int), ("met", C.c_int), ("n_encodes", C.c_int), ("bytes", C.c_uint64), ("mean_d1", C.c_double), ("min_d1", C.c_double),
                ("n_frames", C.c_int), ("frames", C.POINTER(D1Result)), ("cloud_ms", C.c_double)]


class ColorTarget(C.Structure):
    """rbt_color_target; struct_size is filled in. ColorTarget() is the empty target of an entry without one. patches: one list of Patch per point-cloud frame; reference:
    None, or one PCloud with colours (or None = the cloud of the decoded input) per frame. The object keeps the arrays it points to alive."""
    _fields_ = [("struct_size", C.c_uint32), ("min_psnr_mdb", C.c_int32), ("channel", C.c_int), ("stat", C.c_int), ("qp_min", C.c_int), ("qp_max", C.c_int), ("n_frames", C.c_int),
                ("atlas", AtlasParams), ("patches", C.POINTER(C.POINTER(Patch))), ("n_patches", C.POINTER(C.c_int)), ("upsample_filter", C.c_int), ("attr_transfer", C.c_int),
                ("reference", C.POINTER(C.c_void_p))]

    def __init__(self, atlas=None, patches=None, min_psnr_mdb=0, channel=0, stat=RBT_D1_MIN, qp_min=0, qp_max=0, upsample_filter=0, attr_transfer=1, reference=None):
        super().__init__(C.sizeof(ColorTarget))
        self._keep = []
        if atlas is None:
            return
        self.min_psnr_mdb, self.channel, self.stat, self.qp_min, self.qp_max, self.upsample_filter, self.attr_transfer = min_psnr_mdb, channel, stat, qp_min, qp_max, upsample_filter, attr_transfer
        self.atlas = AtlasParams(*[getattr(atlas, n) for n, _ in AtlasParams._fields_])
        self.n_frames = len(patches)
        lists = [(Patch * max(1, len(p)))(*p) for p in patches]
        ptrs = (C.POINTER(Patch) * max(1, len(lists)))(*[C.cast(a, C.POINTER(Patch)) for a in lists])
        counts = (C.c_int * max(1, len(lists)))(*[len(p) for p in patches])
        self.patches, self.n_patches = ptrs, counts
        self._keep += [lists, ptrs, counts]
        if reference is not None:
            refs = (C.c_void_p * max(1, len(reference)))(*[None if r is None else (r.h.value if isinstance(r, PCloud) else r) for r in reference])
            self.reference = refs
            self._keep += [refs, list(reference)]


class ColorFloorResult(C.Structure):
    """rbt_color_floor_result: q*, the probe q0, the walk's start qs, met, distinct QPs encoded, the stream's size, mean and minimum colour PSNR (Y, U, V) over the frames,
    the frames' ColorResult (freed by the binding), device milliseconds of the clouds"""
    _fields_ = [("qp", C.c_int), ("qp_probe", C.c_int), ("qp_start", C.c_int), ("met", C.c_int), ("n_encodes", C.c_int), ("bytes", C.c_uint64), ("mean_psnr", C.c_double * 3),
                ("min_psnr", C.c_double * 3), ("n_frames", C.c_int), ("frames", C.POINTER(ColorResult)), ("cloud_ms", C.c_double)]


class RateTable(C.Structure):
    """rbt_rate_table"""
    _fields_ = [("n_pictures", C.c_int), ("hist", C.POINTER(C.c_uint32)), ("picture_bytes", C.POINTER(C.c_uint64)), ("estimate", C.c_uint64 * 52), ("census_ms", C.c_double)]


V3C_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t))   # rbt_v3c_sink
RBT_V3C_VPS, RBT_V3C_AD, RBT_V3C_OVD, RBT_V3C_GVD, RBT_V3C_AVD = range(5)


def load(path=None):
    """Loads the shared library and declares the C ABI. Raises OSError if the HIP extension has not been built."""
    # 16 HIP streams shared by the jobs in flight: the ROCm runtime multiplexes streams onto 4 hardware queues unless told otherwise, and
    # it reads this when it initialises (librbt also sets it in rbt_create, which is too late if torch touched the GPU first)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    L = C.CDLL(path or LIB_PATH)
    L.rbt_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]
    L.rbt_destroy.argtypes = [C.c_void_p]
    L.rbt_owns_gof.argtypes = [C.c_void_p, C.c_int]
    L.rbt_world.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rbt_strerror.restype = C.c_char_p
    L.rbt_strerror.argtypes = [C.c_int]
    L.rbt_last_error.restype = C.c_char_p
    L.rbt_last_error.argtypes = [C.c_void_p]
    L.rbt_version.restype = C.c_char_p
    L.rbt_free.argtypes = [C.c_void_p]
    L.rbt_decode.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(Video)]
    L.rbt_encode.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 10 + [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.rbt_transcode_substream.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(StreamParams), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.rbt_transcode_gof.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.rbt_submit_gof.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(C.c_void_p)]
    L.rbt_set_depth.argtypes = [C.c_void_p, C.c_int]
    L.rbt_trim.argtypes = [C.c_void_p]
    L.rbt_get_depth.argtypes = [C.c_void_p]
    L.rbt_job_shape.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rbt_preset_from_name.argtypes = [C.c_char_p]
    L.rbt_wait_gof.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.rbt_or_pool.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.rbt_picture_hash.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    L.rbt_sample_to_byte_stream.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.rbt_byte_to_sample_stream.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.rbt_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.rbt_selftest_transform32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint32)]
    L.rbt_selftest_tb.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rbt_reconstruct.argtypes = [C.c_void_p, C.POINTER(AtlasParams), C.POINTER(Patch), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Cloud)]
    L.rbt_cloud_free.argtypes = [C.POINTER(Cloud)]
    L.rbt_d1.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(D1Result)]
    L.rbt_d2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(D2Result)]
    L.rbt_yuv420_to_yuv444.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    L.rbt_yuv16_to_rgb8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.rbt_reconstruct_rgb.argtypes = [C.c_void_p, C.POINTER(AtlasParams), C.POINTER(Patch), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.POINTER(Cloud), C.POINTER(C.c_void_p)]
    L.rbt_color_metric.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(ColorResult)]
    L.rbt_color_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.rbt_transfer_colors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.rbt_reconstruct_decoded.argtypes = [C.c_void_p, C.POINTER(AtlasParams), C.POINTER(Patch), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(Cloud), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.rbt_transfer_stage.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.rbt_pcloud_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.rbt_pcloud_from_maps.argtypes = [C.c_void_p, C.POINTER(AtlasParams), C.POINTER(Patch), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(C.c_void_p), C.POINTER(Cloud), C.POINTER(C.c_void_p)]
    L.rbt_pcloud_points.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rbt_pcloud_release.argtypes = [C.c_void_p, C.c_void_p]
    L.rbt_pcloud_release.restype = None
    L.rbt_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(FrameScore)]
    L.rbt_pcloud_estimate_normals.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(NormalsParams), C.c_void_p, C.POINTER(C.c_double)]
    L.rbt_estimate_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(NormalsParams), C.c_void_p]
    L.rbt_score_summary.argtypes = [C.POINTER(FrameScore), C.c_int, C.POINTER(SequenceScore)]
    L.rbt_v3c_index.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(V3CUnit)), C.POINTER(C.c_int)]
    L.rbt_v3c_write.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.rbt_v3c_stats.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(V3CStat)]
    L.rbt_device_memory.argtypes = [C.c_void_p, C.POINTER(Memory)]
    L.rbt_job_memory.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    L.rbt_transcode_v3c_stream.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(V3CParams), V3C_SINK, C.c_void_p]
    L.rbt_transcode_v3c.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(V3CParams), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.rbt_submit_gof_frame_qp.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(FrameQp), C.POINTER(C.c_void_p)]
    L.rbt_transcode_gof_frame_qp.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(FrameQp), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.rbt_submit_gof_qp_map.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(QpMap), C.POINTER(C.c_void_p)]
    L.rbt_transcode_gof_qp_map.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(QpMap), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    gof_patch = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(PatchFloorTarget)]
    L.rbt_submit_gof_quality_patches.argtypes = gof_patch + [C.POINTER(C.c_void_p)]
    L.rbt_wait_gof_quality_patches.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(PatchFloorResult)]
    L.rbt_transcode_gof_quality_patches.argtypes = gof_patch + [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(PatchFloorResult)]
    gof_pd1 = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(PatchD1Target)]
    L.rbt_submit_gof_d1_patches.argtypes = gof_pd1 + [C.POINTER(C.c_void_p)]
    L.rbt_wait_gof_d1_patches.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(PatchD1Result)]
    L.rbt_transcode_gof_d1_patches.argtypes = gof_pd1 + [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(PatchD1Result)]
    L.rbt_ctb_sse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.rbt_qp_map_from_patches.argtypes = [C.POINTER(AtlasParams), C.POINTER(Patch), C.c_int, C.POINTER(C.c_int8), C.c_int, C.c_int, C.POINTER(C.c_int8), C.c_int, C.c_int]
    L.rbt_submit_gof_rate.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(RateTarget), C.POINTER(C.c_void_p)]
    L.rbt_wait_gof_rate.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(RateResult)]
    L.rbt_transcode_gof_rate.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(RateTarget), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                         C.POINTER(RateResult)]
    L.rbt_submit_gof_quality.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(QualityTarget), C.POINTER(C.c_void_p)]
    L.rbt_wait_gof_quality.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(QualityResult)]
    L.rbt_transcode_gof_quality.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(QualityTarget), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                            C.POINTER(QualityResult)]
    L.rbt_submit_gof_quality_frames.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(QualityTarget), C.POINTER(C.c_void_p)]
    L.rbt_wait_gof_quality_frames.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(FrameFloorResult)]
    L.rbt_transcode_gof_quality_frames.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(QualityTarget), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                   C.POINTER(FrameFloorResult)]
    L.rbt_submit_gof_d1_frames.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(D1Target), C.POINTER(C.c_void_p)]
    L.rbt_wait_gof_d1_frames.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(FrameFloorResult)]
    L.rbt_transcode_gof_d1_frames.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(D1Target), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                              C.POINTER(FrameFloorResult)]
    for name, tt, rt in (("d2", D2Target, D2FloorResult), ("d2_patches", PatchD2Target, PatchD2Result), ("color_patches", PatchColorTarget, PatchColorResult)):
        args = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(tt)]
        getattr(L, "rbt_submit_gof_" + name).argtypes = args + [C.POINTER(C.c_void_p)]
        getattr(L, "rbt_wait_gof_" + name).argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(rt)]
        getattr(L, "rbt_transcode_gof_" + name).argtypes = args + [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(rt)]
    L.rbt_submit_gof_d1.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(D1Target), C.POINTER(C.c_void_p)]
    L.rbt_wait_gof_d1.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(D1FloorResult)]
    L.rbt_transcode_gof_d1.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(D1Target), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                       C.POINTER(D1FloorResult)]
    L.rbt_gather_luma.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 8 + [C.c_void_p]
    L.rbt_submit_gof_color.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(ColorTarget), C.POINTER(C.c_void_p)]
    L.rbt_wait_gof_color.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(ColorFloorResult)]
    L.rbt_transcode_gof_color.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(StreamParams), C.POINTER(ColorTarget), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                          C.POINTER(ColorFloorResult)]
    L.rbt_gather_420.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 10 + [C.c_void_p]
    L.rbt_pcloud_set_colors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rbt_pcloud_set_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rbt_pcloud_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rbt_score_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(PatchD1), C.POINTER(D1Result), C.POINTER(C.c_double)]
    L.rbt_score_patches_d2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(PatchD2), C.POINTER(D2Result), C.POINTER(C.c_double)]
    L.rbt_score_pair_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    L.rbt_score_pair_color.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ColorResult)]
    L.rbt_score_patches_color.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(PatchColor), C.POINTER(ColorResult), C.POINTER(C.c_double)]
    L.rbt_score_pair_patches_color.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(PatchColor), C.POINTER(ColorResult)]
    L.rbt_score_pair_release.argtypes = [C.c_void_p, C.c_void_p]
    L.rbt_score_pair_release.restype = None
    L.rbt_picture_sse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.rbt_transcode_v3c_quality.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(V3CParams), C.c_int32, C.c_int32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.POINTER(QualityResult))]
    L.rbt_transcode_v3c_quality_frames.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(V3CParams), C.c_int32, C.c_int32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                   C.POINTER(C.POINTER(FrameFloorResult))]
    L.rbt_level_census.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rbt_rate_estimate.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(RateTable)]
    L.rbt_transcode_v3c_rate.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(V3CParams), C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.POINTER(RateResult))]
    return L


def _convert(fn, data, L):
    out, n = C.c_void_p(), C.c_size_t()
    rc = fn(data, len(data), C.byref(out), C.byref(n))
    if rc != 0:
        raise RbtError(rc, L.rbt_strerror(rc).decode())
    res = C.string_at(out, n.value)
    L.rbt_free(out)
    return res


RBT_PRESET_DEFAULT, RBT_PRESET_FAST = 0, 1


def preset_from_name(name, lib=None):
    """rbt_preset_from_name: the reference's `preset` string (an x265 preset name) as RBT_PRESET_*"""
    L = lib or load()
    rc = L.rbt_preset_from_name(name.encode() if name is not None else None)
    if rc < 0:
        raise RbtError(rc, L.rbt_strerror(rc).decode())
    return rc


def job_shape(n_gofs, max_jobs=16, lib=None):
    """rbt_job_shape: (GOFs per job, jobs in flight) for a walk of n_gofs GOFs on one GPU"""
    L = lib or load()
    g, d = C.c_int(), C.c_int()
    rc = L.rbt_job_shape(n_gofs, max_jobs, C.byref(g), C.byref(d))
    if rc != 0:
        raise RbtError(rc, L.rbt_strerror(rc).decode())
    return g.value, d.value


def qp_map_from_patches(atlas, patches, patch_qp, background_qp, log2_ctb=5, lib=None):
    """rbt_qp_map_from_patches (host only): the QP map of one frame, int8 [h_ctb, w_ctb] - per CTB the lowest patch_qp of the patches that meet it, background_qp where none does"""
    L = lib or load()
    ctb = 1 << log2_ctb
    wc, hc = (atlas.width + ctb - 1) // ctb, (atlas.height + ctb - 1) // ctb
    n = len(patches)
    out = np.zeros((max(hc, 0), max(wc, 0)), np.int8)
    rc = L.rbt_qp_map_from_patches(C.byref(atlas), (Patch * max(1, n))(*patches), n, (C.c_int8 * max(1, n))(*patch_qp), background_qp, log2_ctb,
                                   out.ctypes.data_as(C.POINTER(C.c_int8)), wc, hc)
    if rc != 0:
        raise RbtError(rc, L.rbt_strerror(rc).decode())
    return out


def byte_to_sample_stream(data: bytes, lib=None):
    """rbt_byte_to_sample_stream (PCCVideoBitstream::byteStreamToSampleStream): Annex-B -> 4-byte sizes (host only)"""
    L = lib or load()
    return _convert(L.rbt_byte_to_sample_stream, data, L)


def sample_to_byte_stream(data: bytes, lib=None):
    """rbt_sample_to_byte_stream (PCCVideoBitstream::sampleStreamToByteStream): 4-byte sizes -> Annex-B (host only)"""
    L = lib or load()
    return _convert(L.rbt_sample_to_byte_stream, data, L)


def v3c_index(data: bytes, lib=None):
    """rbt_v3c_index: the units of a V3C sample stream as a list of dicts (host only: works without a GPU)"""
    L = lib or load()
    u, n = C.POINTER(V3CUnit)(), C.c_int()
    rc = L.rbt_v3c_index(data, len(data), C.byref(u), C.byref(n))
    if rc != 0:
        raise RbtError(rc, L.rbt_strerror(rc).decode())
    out = [{f: getattr(u[i], f) for f, _ in V3CUnit._fields_} for i in range(n.value)]
    L.rbt_free(u)
    return out


def v3c_stats(data: bytes, lib=None):
    """rbt_v3c_stats: the PCCBitstreamStat figures of a V3C sample stream as a dict (host only)"""
    L = lib or load()
    st = V3CStat()
    rc = L.rbt_v3c_stats(data, len(data), C.byref(st))
    if rc != 0:
        raise RbtError(rc, L.rbt_strerror(rc).decode())
    return {n: (list(getattr(st, n)) if n == "unit_size" else getattr(st, n)) for n, _ in V3CStat._fields_}


def v3c_write(units, forced_precision_bytes=0, lib=None):
    """rbt_v3c_write: a V3C sample stream from a list of units (bytes, each with its 4-byte header; host only)"""
    L = lib or load()
    k = len(units)
    arr = (C.c_char_p * max(1, k))(*units)
    sizes = (C.c_size_t * max(1, k))(*[len(x) for x in units])
    out, n = C.c_void_p(), C.c_size_t()
    rc = L.rbt_v3c_write(arr, sizes, k, forced_precision_bytes, C.byref(out), C.byref(n))
    if rc != 0:
        raise RbtError(rc, L.rbt_strerror(rc).decode())
    res = C.string_at(out, n.value)
    L.rbt_free(out)
    return res


def _result_dict(r):
    return {n: (list(v) if isinstance(v, C.Array) else v) for n, v in ((n, getattr(r, n)) for n, _ in r._fields_)}


def frame_score_dict(s):
    """a FrameScore as nested dicts: parts, device_ms, the point counts, and d1 / d2 / color as Context.d1 / d2 / color_metric return them (None for a part not computed)"""
    out = {n: getattr(s, n) for n in ("parts", "device_ms", "n_points_a", "n_points_b", "n_merged_a", "n_merged_b")}
    for name, bit in (("d1", RBT_SCORE_D1), ("d2", RBT_SCORE_D2), ("color", RBT_SCORE_COLOR)):
        out[name] = _result_dict(getattr(s, name)) if s.parts & bit else None
    return out


def score_summary(frames, lib=None):
    """rbt_score_summary: a list of FrameScore (Context.score(..., raw=True)) -> dict of the sequence's means, minima and counts (host only)"""
    L = lib or load()
    arr = (FrameScore * max(1, len(frames)))(*frames)
    out = SequenceScore()
    rc = L.rbt_score_summary(arr, len(frames), C.byref(out))
    if rc != 0:
        raise RbtError(rc, L.rbt_strerror(rc).decode())
    return _result_dict(out)


RBT_NORMALS_ORIENT_NONE, RBT_NORMALS_ORIENT_SPANNING_TREE, RBT_NORMALS_ORIENT_VIEW_POINT, RBT_NORMALS_ORIENT_CUBEMAP = range(4)


class NormalsParams(C.Structure):
    """rbt_normals_params; struct_size is filled in"""
    _fields_ = [("struct_size", C.c_uint32), ("k", C.c_int), ("orientation", C.c_int), ("view_point", C.c_int32 * 3)]

    def __init__(self, k=0, orientation=RBT_NORMALS_ORIENT_VIEW_POINT, view_point=(0, 0, 0)):
        super().__init__(C.sizeof(NormalsParams), k, orientation, (C.c_int32 * 3)(*view_point))


RBT_D2_MIN, RBT_D2_MEAN = RBT_D1_MIN, RBT_D1_MEAN


def _set_normals(target, normals):
    """the normals field of a D2 target: None leaves struct_size 0 (all defaults)"""
    if normals is not None:
        target.normals = NormalsParams(normals.k, normals.orientation, tuple(normals.view_point))


class D2Target(C.Structure):
    """rbt_d2_target: D1Target with min_d2_mdb, references that carry normals (None = the cloud of the decoded input with estimated normals) and normals, the
    NormalsParams of that estimation (None = all defaults)"""
    _fields_ = [("struct_size", C.c_uint32), ("min_d2_mdb", C.c_int32), ("stat", C.c_int), ("peak", C.c_int), ("qp_min", C.c_int), ("qp_max", C.c_int), ("n_frames", C.c_int),
                ("atlas", AtlasParams), ("patches", C.POINTER(C.POINTER(Patch))), ("n_patches", C.POINTER(C.c_int)), ("reference", C.POINTER(C.c_void_p)), ("normals", NormalsParams)]

    def __init__(self, atlas=None, patches=None, min_d2_mdb=0, stat=RBT_D2_MIN, qp_min=0, qp_max=0, peak=0, reference=None, normals=None):
        C.Structure.__init__(self)
        self.struct_size = C.sizeof(D2Target)
        self._keep = []
        if atlas is None:
            return
        d = D1Target(atlas, patches, min_d2_mdb, stat, qp_min, qp_max, peak, reference)      # the arrays are D1Target's, kept alive with it
        for name, _ in D1Target._fields_[2:]:
            setattr(self, name, getattr(d, name))
        self.min_d2_mdb = min_d2_mdb
        self._keep.append(d)
        _set_normals(self, normals)


class D2FloorResult(C.Structure):
    """rbt_d2_floor_result: D1FloorResult with mean_d2, min_d2 and the frames' D2Result"""
    _fields_ = [("qp", C.c_int), ("qp_probe", C.c_int), ("qp_start", C.c_int), ("met", C.c_int), ("n_encodes", C.c_int), ("bytes", C.c_uint64), ("mean_d2", C.c_double), ("min_d2", C.c_double),
                ("n_frames", C.c_int), ("frames", C.POINTER(D2Result)), ("cloud_ms", C.c_double)]


class PatchD2Target(C.Structure):
    """rbt_patch_d2_target: PatchD1Target with min_d2_mdb, patch_floors as patch_min_d2_mdb, references that carry normals and normals (None = all defaults)"""
    _fields_ = [("struct_size", C.c_uint32), ("min_d2_mdb", C.c_int32), ("peak", C.c_int), ("qp_min", C.c_int), ("qp_max", C.c_int), ("background_qp", C.c_int), ("max_trials", C.c_int),
                ("atlas", AtlasParams), ("n_frames", C.c_int), ("patches", C.POINTER(C.POINTER(Patch))), ("n_patches", C.POINTER(C.c_int)), ("patch_min_d2_mdb", C.POINTER(C.POINTER(C.c_int32))),
                ("reference", C.POINTER(C.c_void_p)), ("normals", NormalsParams)]

    def __init__(self, atlas=None, patches=None, min_d2_mdb=0, peak=0, qp_min=0, qp_max=0, background_qp=-1, max_trials=0, patch_floors=None, reference=None, normals=None):
        C.Structure.__init__(self)
        self.struct_size = C.sizeof(PatchD2Target)
        self._keep = []
        if atlas is None:
            return
        d = PatchD1Target(atlas, patches, min_d2_mdb, peak, qp_min, qp_max, background_qp, max_trials, patch_floors, reference)      # the arrays are PatchD1Target's
        for (name, _), (src, _) in zip(PatchD2Target._fields_[1:13], PatchD1Target._fields_[1:13]):
            setattr(self, name, getattr(d, src))
        self._keep.append(d)
        _set_normals(self, normals)


class PatchD2Pick(C.Structure):
    """rbt_patch_d2_pick: of a frame's settling trial, per patch: its QP, met, failed, its PatchD2, its figure"""
    _fields_ = [("qp", C.c_int), ("met", C.c_int), ("failed", C.c_int), ("d2", PatchD2), ("figure", C.c_double)]


class PatchD2Frame(C.Structure):
    """rbt_patch_d2_frame: trials, met, the patch count, the frame's bytes, the whole frame's D2Result in the settling trial, the picks"""
    _fields_ = [("n_trials", C.c_int), ("met", C.c_int), ("n_patches", C.c_int), ("bytes", C.c_uint64), ("d2", D2Result), ("patches", C.POINTER(PatchD2Pick))]


class PatchD2Result(C.Structure):
    """rbt_patch_d2_result: as PatchD1Result"""
    _fields_ = [("n_frames", C.c_int), ("qp_probe", C.c_int), ("met_all", C.c_int), ("n_passes", C.c_int), ("bytes", C.c_uint64), ("pictures_encoded", C.c_uint64), ("w_ctb", C.c_int), ("h_ctb", C.c_int),
                ("map", C.POINTER(C.c_int8)), ("frames", C.POINTER(PatchD2Frame)), ("picks", C.POINTER(PatchD2Pick)), ("cloud_ms", C.c_double)]


class PatchColorTarget(C.Structure):
    """rbt_patch_color_target: PatchD1Target's walk side (min_psnr_mdb, qp_min, qp_max, background_qp, max_trials, patch_floors as patch_min_psnr_mdb) with ColorTarget's
    cloud side (channel, upsample_filter, attr_transfer, references with colours)"""
    _fields_ = [("struct_size", C.c_uint32), ("min_psnr_mdb", C.c_int32), ("channel", C.c_int), ("qp_min", C.c_int), ("qp_max", C.c_int), ("background_qp", C.c_int), ("max_trials", C.c_int),
                ("atlas", AtlasParams), ("n_frames", C.c_int), ("patches", C.POINTER(C.POINTER(Patch))), ("n_patches", C.POINTER(C.c_int)), ("patch_min_psnr_mdb", C.POINTER(C.POINTER(C.c_int32))),
                ("upsample_filter", C.c_int), ("attr_transfer", C.c_int), ("reference", C.POINTER(C.c_void_p))]

    def __init__(self, atlas=None, patches=None, min_psnr_mdb=0, channel=0, qp_min=0, qp_max=0, background_qp=-1, max_trials=0, patch_floors=None, upsample_filter=0, attr_transfer=1, reference=None):
        C.Structure.__init__(self)
        self.struct_size = C.sizeof(PatchColorTarget)
        self._keep = []
        if atlas is None:
            return
        d = PatchD1Target(atlas, patches, min_psnr_mdb, 0, qp_min, qp_max, background_qp, max_trials, patch_floors, reference)      # the arrays are PatchD1Target's, kept alive with it
        for name, src in (("min_psnr_mdb", "min_d1_mdb"), ("patch_min_psnr_mdb", "patch_min_d1_mdb")) + tuple((n, n) for n in ("qp_min", "qp_max", "background_qp", "max_trials", "atlas", "n_frames", "patches", "n_patches", "reference")):
            setattr(self, name, getattr(d, src))
        self.channel, self.upsample_filter, self.attr_transfer = channel, upsample_filter, attr_transfer
        self._keep.append(d)


class PatchColorPick(C.Structure):
    """rbt_patch_color_pick: of a frame's settling trial, per patch: its QP, met, failed, its PatchColor, its figure"""
    _fields_ = [("qp", C.c_int), ("met", C.c_int), ("failed", C.c_int), ("color", PatchColor), ("figure", C.c_double)]


class PatchColorFrame(C.Structure):
    """rbt_patch_color_frame: trials, met, the patch count, the frame's bytes, the whole frame's ColorResult in the settling trial, the picks"""
    _fields_ = [("n_trials", C.c_int), ("met", C.c_int), ("n_patches", C.c_int), ("bytes", C.c_uint64), ("color", ColorResult), ("patches", C.POINTER(PatchColorPick))]


class PatchColorResult(C.Structure):
    """rbt_patch_color_result: as PatchD1Result"""
    _fields_ = [("n_frames", C.c_int), ("qp_probe", C.c_int), ("met_all", C.c_int), ("n_passes", C.c_int), ("bytes", C.c_uint64), ("pictures_encoded", C.c_uint64), ("w_ctb", C.c_int), ("h_ctb", C.c_int),
                ("map", C.POINTER(C.c_int8)), ("frames", C.POINTER(PatchColorFrame)), ("picks", C.POINTER(PatchColorPick)), ("cloud_ms", C.c_double)]


class PCloud:
    """rbt_pcloud: a point cloud on the device with its index; belongs to the context that made it. release() hands it back (its clean volume stays cached in the context)."""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def points(self):
        """(points, merged points)"""
        n, m = C.c_int(), C.c_int()
        self.ctx._chk(self.ctx.L.rbt_pcloud_points(self.h, C.byref(n), C.byref(m)))
        return n.value, m.value

    def estimate_normals(self, params=None, copy=True):
        """rbt_pcloud_estimate_normals: the cloud gets normals of its own (params: NormalsParams or None = defaults) -> (normals int16 [n,3] in Q14, or None without
        copy; device_ms)"""
        out = np.empty((self.points()[0], 3), np.int16) if copy else None
        ms = C.c_double()
        self.ctx._chk(self.ctx.L.rbt_pcloud_estimate_normals(self.ctx.h, self.h, None if params is None else C.byref(params), None if out is None else out.ctypes.data, C.byref(ms)))
        return out, ms.value

    def set_colors(self, rgb):
        """rbt_pcloud_set_colors: new colours (uint8 [n,3], one per point in point order) for the indexed cloud; positions and the index's keys stay"""
        c = np.ascontiguousarray(rgb, dtype=np.uint8)
        if c.shape != (self.points()[0], 3):
            raise ValueError("one colour per point")
        self.ctx._chk(self.ctx.L.rbt_pcloud_set_colors(self.ctx.h, self.h, c.ctypes.data))

    def set_labels(self, labels):
        """rbt_pcloud_set_labels: a label per point (uint32 [n], each below 65536), in point order - the patch of the point for rbt_score_patches"""
        a = np.ascontiguousarray(labels, dtype=np.uint32)
        if a.shape != (self.points()[0],):
            raise ValueError("one label per point")
        self.ctx._chk(self.ctx.L.rbt_pcloud_set_labels(self.ctx.h, self.h, a.ctypes.data))

    def labels(self):
        """rbt_pcloud_labels: the label of every point (uint32 [n]); of a cloud made from maps, the index of the patch that emitted the point"""
        out = np.empty(self.points()[0], np.uint32)
        self.ctx._chk(self.ctx.L.rbt_pcloud_labels(self.ctx.h, self.h, out.ctypes.data))
        return out

    def release(self):
        if self.h:
            self.ctx.L.rbt_pcloud_release(self.ctx.h, self.h)
            self.h = C.c_void_p()


class ScorePair:
    """rbt_score_pair: the nearest squared distances between two PClouds, both directions, kept on the device; color() is the colour part of Context.score for the
    colours the clouds have at that moment. The clouds must outlive the pair."""

    def __init__(self, ctx, a, b):
        self.ctx, self.h = ctx, C.c_void_p()
        ctx._chk(ctx.L.rbt_score_pair_create(ctx.h, a.h if a is not None else None, b.h if b is not None else None, C.byref(self.h)))

    def color(self):
        """rbt_score_pair_color -> dict as Context.color_metric returns it"""
        r = ColorResult()
        self.ctx._chk(self.ctx.L.rbt_score_pair_color(self.ctx.h, self.h, C.byref(r)))
        return {n: (getattr(r, n) if n in ("n_a", "n_b") else list(getattr(r, n))) for n, _ in ColorResult._fields_}

    def patches_color(self, n_patches, raw=False):
        """rbt_score_pair_patches_color -> (one dict per patch - or the PatchColor array itself (raw) -, the whole frame's colour result as color() returns it)"""
        out = (PatchColor * max(1, n_patches))(); whole = ColorResult()
        self.ctx._chk(self.ctx.L.rbt_score_pair_patches_color(self.ctx.h, self.h, n_patches, out, C.byref(whole)))
        return (out if raw else [patch_color_dict(out[k]) for k in range(n_patches)]), (whole if raw else _result_dict(whole))

    def release(self):
        if self.h:
            self.ctx.L.rbt_score_pair_release(self.ctx.h, self.h)
            self.h = C.c_void_p()


class Context:
    """One transcoder context (rbt_create). Mirrors how PCCTranscoder is used: construct, then transcode per GOF."""

    def __init__(self, device=0, rank=0, world=1, lib_path=None):
        self.L = load(lib_path)
        self.lib_path = lib_path      # (a second context on the same build: Context(lib_path=ctx.lib_path))
        self.h = C.c_void_p()
        rc = self.L.rbt_create(C.byref(self.h), device, rank, world)
        if rc != 0:
            raise RbtError(rc, self.L.rbt_strerror(rc).decode())

    def owns_gof(self, g):
        """rbt_owns_gof: GOF g of a sequence belongs to rank g mod world"""
        return bool(self.L.rbt_owns_gof(self.h, g))

    def close(self):
        if self.h:
            self.L.rbt_destroy(self.h)
            self.h = C.c_void_p()

    def _chk(self, rc):
        if rc != 0:
            detail = self.L.rbt_last_error(self.h).decode()
            raise RbtError(rc, self.L.rbt_strerror(rc).decode() + (": " + detail if detail else ""))

    def _take(self, ptr, n):
        out = C.string_at(ptr, n.value) if ptr.value else b""
        self.L.rbt_free(ptr)
        return out

    def decode(self, stream: bytes, verify_md5=True):
        v = Video()
        self._chk(self.L.rbt_decode(self.h, stream, len(stream), int(verify_md5), C.byref(v)))
        fs = v.width * v.height * 3 // 2
        arr = np.ctypeslib.as_array(v.data, shape=(v.n_frames, fs)).copy()
        self.L.rbt_free(v.data)
        return arr, v.width, v.height, v.bit_depth, v.md5_checked, v.md5_failed

    def encode(self, frames, w, h, bit_depth, qp, gop=2, lossless=0, log2_ctb=5, rows_per_slice=1, md5_sei=1):
        frames = np.ascontiguousarray(frames, dtype=np.uint16)
        out, n = C.c_void_p(), C.c_size_t()
        self._chk(self.L.rbt_encode(self.h, frames.ctypes.data, w, h, bit_depth, frames.shape[0], qp, gop, lossless, log2_ctb, rows_per_slice, md5_sei, C.byref(out), C.byref(n)))
        return self._take(out, n)

    def transcode_substream(self, stream: bytes, video_type, qp, occupancy_precision=4, log2_ctb=5, rows_per_slice=1, md5_sei=1, verify_md5=0, preset=0):
        p = StreamParams(video_type, qp, occupancy_precision, log2_ctb, rows_per_slice, md5_sei, verify_md5, 0, preset)
        out, n = C.c_void_p(), C.c_size_t()
        self._chk(self.L.rbt_transcode_substream(self.h, stream, len(stream), C.byref(p), C.byref(out), C.byref(n)))
        return self._take(out, n)

    def transcode_gof(self, streams, params):
        return self._transcode(self.L.rbt_transcode_gof, streams, params)

    def transcode_v3c(self, data: bytes, geometry_qp, attribute_qp, occupancy_precision=4, forced_precision_bytes=0, log2_ctb=5, rows_per_slice=-1, md5_sei=0,
                      verify_md5=0, gofs_per_job=1, occupancy_rd=0, preset=0):
        """rbt_transcode_v3c: a whole V3C sample stream (every GOF this context owns) -> transcoded sample stream; gofs_per_job=0: job shape by rbt_job_shape"""
        p = V3CParams(occupancy_precision, geometry_qp, attribute_qp, forced_precision_bytes, log2_ctb, rows_per_slice, md5_sei, verify_md5, gofs_per_job, occupancy_rd, preset)
        out, n = C.c_void_p(), C.c_size_t()
        self._chk(self.L.rbt_transcode_v3c(self.h, data, len(data), C.byref(p), C.byref(out), C.byref(n)))
        return self._take(out, n)

    def transcode_v3c_stream(self, data: bytes, sink, geometry_qp, attribute_qp, occupancy_precision=4, log2_ctb=5, rows_per_slice=-1, md5_sei=0, verify_md5=0, gofs_per_job=0):
        """rbt_transcode_v3c_stream: sink(gof, [unit bytes, ...]) is called once per GOF this context owns, in GOF order, while later GOFs are still on the GPU; a truthy
        return of the sink ends the walk"""
        p = V3CParams(occupancy_precision, geometry_qp, attribute_qp, 0, log2_ctb, rows_per_slice, md5_sei, verify_md5, gofs_per_job)

        def cb(_user, gof, n_units, unit, unit_size):
            return 1 if sink(gof, [C.string_at(unit[i], unit_size[i]) for i in range(n_units)]) else 0
        self._chk(self.L.rbt_transcode_v3c_stream(self.h, data, len(data), C.byref(p), V3C_SINK(cb), None))

    def device_memory(self):
        """rbt_device_memory: {total, free, cached, in_use, reserve} bytes as the library sees the device"""
        m = Memory()
        self._chk(self.L.rbt_device_memory(self.h, C.byref(m)))
        return {"total": m.total_bytes, "free": m.free_bytes, "cached": m.cached_bytes, "in_use": m.in_use_bytes, "reserve": m.reserve_bytes}

    def job_memory(self, job):
        """rbt_job_memory: device bytes a submitted job holds"""
        b = C.c_size_t()
        self._chk(self.L.rbt_job_memory(self.h, job[0] if isinstance(job, tuple) else job, C.byref(b)))
        return b.value

    def set_depth(self, n):
        """rbt_set_depth: how many GOFs the caller will keep in flight (1..16 = RBT_MAX_JOBS, default 4)"""
        self._chk(self.L.rbt_set_depth(self.h, n))

    def get_depth(self):
        """rbt_get_depth: the depth announced with set_depth"""
        return self.L.rbt_get_depth(self.h)

    def trim(self):
        """rbt_trim: hand the cached device memory of earlier jobs back to the driver (call when the workload changes shape)"""
        self._chk(self.L.rbt_trim(self.h))

    @staticmethod
    def _gof_args(streams, params, targets=None, target_type=None):
        """the entries of a GOF call as ctypes arguments: count, streams, sizes, params and, for a call with targets, one target_type per entry"""
        k = len(streams)
        args = [k, (C.c_char_p * k)(*streams), (C.c_size_t * k)(*[len(s) for s in streams]), (StreamParams * k)(*params)]
        return args if target_type is None else args + [(target_type * k)(*targets)]

    def _submit(self, fn, streams, params, targets=None, target_type=None):
        job = C.c_void_p()
        self._chk(fn(self.h, *self._gof_args(streams, params, targets, target_type), C.byref(job)))
        return (job, len(streams))

    def _collect(self, fn, k, args, result_type=None):
        """fn(handle, *args, outs, sizes[, results]) -> [stream bytes, ...], with a result_type: ([stream bytes, ...], [result dict, ...])"""
        outs = (C.c_void_p * k)()
        ns = (C.c_size_t * k)()
        rs = [(result_type * k)()] if result_type is not None else []
        self._chk(fn(self.h, *args, outs, ns, *rs))
        res = []
        for i in range(k):
            res.append(C.string_at(outs[i], ns[i]) if outs[i] else b"")
            self.L.rbt_free(outs[i])
        return (res, [_result_dict(r) for r in rs[0]]) if rs else res

    def _transcode(self, fn, streams, params, targets=None, target_type=None, result_type=None):
        args = self._gof_args(streams, params, targets, target_type)
        return self._collect(fn, args[0], args, result_type)

    def submit_gof(self, streams, params):
        """rbt_submit_gof: enqueue one GOF; returns a job for wait_gof. Up to set_depth() jobs may be in flight."""
        return self._submit(self.L.rbt_submit_gof, streams, params)

    def wait_gof(self, job):
        return self._collect(self.L.rbt_wait_gof, job[1], [job[0]])

    @staticmethod
    def _frame_qp(lists):
        return [l if isinstance(l, FrameQp) else FrameQp(l) for l in lists]

    def submit_gof_frame_qp(self, streams, params, lists):
        """rbt_submit_gof_frame_qp: submit_gof with, per entry, a list of one QP per point-cloud frame (None / empty = the entry's own QP) or a FrameQp; returns a job for wait_gof"""
        lists = self._frame_qp(lists)      # (alive until the call returns: the library copies the lists)
        return self._submit(self.L.rbt_submit_gof_frame_qp, streams, params, lists, FrameQp)

    def transcode_gof_frame_qp(self, streams, params, lists):
        """rbt_transcode_gof_frame_qp: submit + wait"""
        lists = self._frame_qp(lists)
        return self._transcode(self.L.rbt_transcode_gof_frame_qp, streams, params, lists, FrameQp)

    @staticmethod
    def _qp_maps(maps):
        return [m if isinstance(m, QpMap) else QpMap(m) for m in maps]

    def submit_gof_qp_map(self, streams, params, maps):
        """rbt_submit_gof_qp_map: submit_gof with, per entry, a map M[f][r][c] of one QP per CTB and point-cloud frame (None = the entry's own QP) or a QpMap; maps=None hands
        the library a null pointer (rbt_submit_gof). Returns a job for wait_gof"""
        if maps is None:
            job = C.c_void_p()
            self._chk(self.L.rbt_submit_gof_qp_map(self.h, *self._gof_args(streams, params), None, C.byref(job)))
            return (job, len(streams))
        maps = self._qp_maps(maps)      # (alive until the call returns: the library copies the maps)
        return self._submit(self.L.rbt_submit_gof_qp_map, streams, params, maps, QpMap)

    def transcode_gof_qp_map(self, streams, params, maps):
        """rbt_transcode_gof_qp_map: submit + wait"""
        return self.wait_gof(self.submit_gof_qp_map(streams, params, maps))

    def _frame_results(self, res):
        """([stream bytes, ...], [FrameFloorResult, ...] as dicts): frames becomes a list of pick dicts, sums a dict, and the library's array is released"""
        outs, rs = res
        for r in rs:
            ptr = r["frames"]
            r["frames"] = [_result_dict(ptr[f]) for f in range(r["n_frames"])] if ptr else []
            self.L.rbt_free(ptr)
            r["sums"] = _result_dict(r["sums"])
            d1 = r["d1"]
            r["d1"] = [{n: getattr(d1[f], n) for n, _ in D1Result._fields_} for f in range(r["n_frames"])] if d1 else None
            self.L.rbt_free(d1)
        return outs, rs

    def _patch_results(self, res, frame_dict=_result_dict, pick_dict=_result_dict):
        """([stream bytes, ...], [PatchFloorResult or PatchD1Result, ...] as dicts): map becomes an int8 array [n_frames, h_ctb, w_ctb] (None without a target), frames a list
        of dicts (frame_dict of the frame) whose patches are pick dicts (pick_dict of the pick), sums (the PSNR kind's) a dict, and the library's arrays are released"""
        outs, rs = res
        for r in rs:
            fr, mp = r["frames"], r["map"]
            r["frames"] = [dict(frame_dict(fr[f]), patches=[pick_dict(fr[f].patches[k]) for k in range(fr[f].n_patches)]) for f in range(r["n_frames"])] if fr else []
            r["map"] = np.ctypeslib.as_array(mp, (r["n_frames"], r["h_ctb"], r["w_ctb"])).copy() if mp else None
            for ptr in (fr, mp, r.pop("picks")):
                self.L.rbt_free(ptr)
            if "sums" in r:
                r["sums"] = _result_dict(r["sums"])
        return outs, rs

    def ctb_sse(self, a, b, w, h, log2_ctb=5, occ=None, rects=None):
        """rbt_ctb_sse: planar 4:2:0 pictures a, b ([n, w*h*3/2] uint16), or None one occupancy plane per picture ([n, oh, ow] uint16), or None rectangles [[c0, r0, c1, r1],
        ...] in CTB units -> uint64 [n, h_ctb, w_ctb, 3]: per picture and CTB the luma sums sse, sse_occ, n_occ; with rects (a list, may be empty) also uint64
        [n / 2, n_rects + 2, 3]: per pair of pictures the sums over each rectangle, the background and the whole frame. stats()["gpu_ms"]: the device time of the launches"""
        a = np.ascontiguousarray(a, dtype=np.uint16).reshape(-1, w * h * 3 // 2)
        b = np.ascontiguousarray(b, dtype=np.uint16).reshape(-1, w * h * 3 // 2)
        if a.shape != b.shape:
            raise ValueError("a and b must hold the same number of pictures")
        ow = oh = 0
        if occ is not None:
            occ = np.ascontiguousarray(occ, dtype=np.uint16)
            if occ.ndim != 3 or occ.shape[0] != a.shape[0]:
                raise ValueError("occ must be [n, oh, ow]")
            oh, ow = occ.shape[1:]
        ctb = 1 << max(0, min(log2_ctb, 12))
        out = np.zeros((a.shape[0], (h + ctb - 1) // ctb, (w + ctb - 1) // ctb, 3), np.uint64)
        rc = out_r = None
        if rects is not None:
            rc = np.ascontiguousarray(np.asarray(rects, dtype=np.int32).reshape(-1, 4))
            out_r = np.zeros((a.shape[0] // 2, rc.shape[0] + 2, 3), np.uint64)
        self._chk(self.L.rbt_ctb_sse(self.h, a.ctypes.data, b.ctypes.data, w, h, a.shape[0], log2_ctb, occ.ctypes.data if occ is not None else None, ow, oh,
                                     rc.ctypes.data if rc is not None and rc.size else None, rc.shape[0] if rc is not None else 0, out.ctypes.data, out_r.ctypes.data if out_r is not None else None))
        return out if rects is None else (out, out_r)

    def _d1_results(self, res):
        """([stream bytes, ...], [D1FloorResult, ...] as dicts): frames becomes a list of D1 dicts and the library's array is released"""
        outs, rs = res
        for r in rs:
            ptr = r["frames"]
            r["frames"] = [{n: getattr(ptr[f], n) for n, _ in D1Result._fields_} for f in range(r["n_frames"])]
            self.L.rbt_free(ptr)
        return outs, rs

    def _d2_results(self, res):
        """as _d1_results, with D2 dicts"""
        outs, rs = res
        for r in rs:
            ptr = r["frames"]
            r["frames"] = [{n: getattr(ptr[f], n) for n, _ in D2Result._fields_} for f in range(r["n_frames"])]
            self.L.rbt_free(ptr)
        return outs, rs

    def _color_results(self, res):
        """([stream bytes, ...], [ColorFloorResult, ...] as dicts): frames becomes a list of colour dicts (Context.color_metric's) and the library's array is released"""
        outs, rs = res
        for r in rs:
            ptr = r["frames"]
            r["frames"] = [{n: (getattr(ptr[f], n) if n in ("n_a", "n_b") else list(getattr(ptr[f], n))) for n, _ in ColorResult._fields_} for f in range(r["n_frames"])]
            r["mean_psnr"], r["min_psnr"] = list(r["mean_psnr"]), list(r["min_psnr"])
            self.L.rbt_free(ptr)
        return outs, rs

    def gather_luma(self, src, x0, y0, w, h, src_misalign=0):
        """rbt_gather_luma: planes src ([n, rows, stride] uint16) -> the w x h window at (x0, y0) of each, packed ([n, h, w]); the planes lie src_misalign samples behind
        a 256-byte boundary on the device"""
        src = np.ascontiguousarray(src, dtype=np.uint16)
        n, rows, stride = src.shape
        out = np.zeros((n, h, w), np.uint16)
        self._chk(self.L.rbt_gather_luma(self.h, src.ctypes.data, n, stride, rows, x0, y0, w, h, src_misalign, out.ctypes.data))
        return out

    def picture_sse(self, a, b, w, h, occ=None):
        """rbt_picture_sse: planar 4:2:0 pictures a, b ([n, w*h*3/2] uint16) and, or None, one occupancy plane per picture ([n, oh, ow] uint16) -> uint64 [n, 3, 3]:
        per picture and plane (Y, Cb, Cr) the sums sse, sse_occ, n_occ; stats()["gpu_ms"] afterwards: the device time of the kernel's launches"""
        a = np.ascontiguousarray(a, dtype=np.uint16).reshape(-1, w * h * 3 // 2)
        b = np.ascontiguousarray(b, dtype=np.uint16).reshape(-1, w * h * 3 // 2)
        if a.shape != b.shape:
            raise ValueError("a and b must hold the same number of pictures")
        ow = oh = 0
        if occ is not None:
            occ = np.ascontiguousarray(occ, dtype=np.uint16)
            if occ.ndim != 3 or occ.shape[0] != a.shape[0]:
                raise ValueError("occ must be [n, oh, ow]")
            oh, ow = occ.shape[1:]
        out = np.zeros((a.shape[0], 3, 3), np.uint64)
        self._chk(self.L.rbt_picture_sse(self.h, a.ctypes.data, b.ctypes.data, w, h, a.shape[0], occ.ctypes.data if occ is not None else None, ow, oh, out.ctypes.data))
        return out

    def transcode_v3c_quality(self, data: bytes, geometry_qp, attribute_qp, geometry_min_psnr_mdb=0, attribute_min_psnr_mdb=0, region=RBT_QUALITY_ALL, occupancy_precision=4, forced_precision_bytes=0,
                              log2_ctb=5, rows_per_slice=-1, md5_sei=0, verify_md5=0, gofs_per_job=1, occupancy_rd=0, preset=0):
        """rbt_transcode_v3c_quality -> (sample stream, [(geometry result, attribute result) per GOF of the input])"""
        p = V3CParams(occupancy_precision, geometry_qp, attribute_qp, forced_precision_bytes, log2_ctb, rows_per_slice, md5_sei, verify_md5, gofs_per_job, occupancy_rd, preset)
        out, n, rs = C.c_void_p(), C.c_size_t(), C.POINTER(QualityResult)()
        self._chk(self.L.rbt_transcode_v3c_quality(self.h, data, len(data), C.byref(p), geometry_min_psnr_mdb, attribute_min_psnr_mdb, region, C.byref(out), C.byref(n), C.byref(rs)))
        n_gofs = v3c_stats(data, self.L)["n_gofs"]
        per = [(_result_dict(rs[2 * g]), _result_dict(rs[2 * g + 1])) for g in range(n_gofs)]
        self.L.rbt_free(rs)
        return self._take(out, n), per

    def transcode_v3c_quality_frames(self, data: bytes, geometry_qp, attribute_qp, geometry_min_psnr_mdb=0, attribute_min_psnr_mdb=0, region=RBT_QUALITY_ALL, occupancy_precision=4,
                                     forced_precision_bytes=0, log2_ctb=5, rows_per_slice=-1, md5_sei=0, verify_md5=0, gofs_per_job=1, occupancy_rd=0, preset=0):
        """rbt_transcode_v3c_quality_frames -> (sample stream, [(geometry result, attribute result) per GOF of the input]), the results as wait_gof_quality_frames gives them"""
        p = V3CParams(occupancy_precision, geometry_qp, attribute_qp, forced_precision_bytes, log2_ctb, rows_per_slice, md5_sei, verify_md5, gofs_per_job, occupancy_rd, preset)
        out, n, rs = C.c_void_p(), C.c_size_t(), C.POINTER(FrameFloorResult)()
        self._chk(self.L.rbt_transcode_v3c_quality_frames(self.h, data, len(data), C.byref(p), geometry_min_psnr_mdb, attribute_min_psnr_mdb, region, C.byref(out), C.byref(n), C.byref(rs)))
        n_gofs = v3c_stats(data, self.L)["n_gofs"]
        flat = self._frame_results(([], [_result_dict(rs[i]) for i in range(2 * n_gofs)]))[1]
        self.L.rbt_free(rs)
        return self._take(out, n), [(flat[2 * g], flat[2 * g + 1]) for g in range(n_gofs)]

    def level_census(self, y, cb, cr, qp4, pm4):
        """rbt_level_census: int16 planes y [h, w], cb / cr [h/2, w/2], int8 qp4 and uint8 pm4 [h/4, w/4] -> uint32 [3, 53]"""
        y = np.ascontiguousarray(y, dtype=np.int16); cb = np.ascontiguousarray(cb, dtype=np.int16); cr = np.ascontiguousarray(cr, dtype=np.int16)
        qp4 = np.ascontiguousarray(qp4, dtype=np.int8); pm4 = np.ascontiguousarray(pm4, dtype=np.uint8)
        h, w = y.shape
        if cb.shape != (h // 2, w // 2) or cr.shape != cb.shape or qp4.shape != (h // 4, w // 4) or pm4.shape != qp4.shape:
            raise ValueError("plane and map shapes do not belong to one picture")
        out = np.zeros((3, 53), np.uint32)
        self._chk(self.L.rbt_level_census(self.h, y.ctypes.data, cb.ctypes.data, cr.ctypes.data, w, h, qp4.ctypes.data, pm4.ctypes.data, out.ctypes.data))
        return out

    def rate_estimate(self, stream: bytes, video_type=RBT_VIDEO_GEOMETRY):
        """rbt_rate_estimate -> {"hist": uint32 [n, 3, 53], "picture_bytes": uint64 [n], "estimate": uint64 [52], "census_ms": float}"""
        t = RateTable()
        self._chk(self.L.rbt_rate_estimate(self.h, stream, len(stream), video_type, C.byref(t)))
        n = t.n_pictures
        out = {"hist": np.ctypeslib.as_array(t.hist, shape=(n, 3, 53)).copy(), "picture_bytes": np.ctypeslib.as_array(t.picture_bytes, shape=(n,)).copy(),
               "estimate": np.array(list(t.estimate), np.uint64), "census_ms": t.census_ms}
        self.L.rbt_free(t.hist); self.L.rbt_free(t.picture_bytes)
        return out

    def transcode_v3c_rate(self, data: bytes, geometry_qp, attribute_qp, geometry_bits_per_picture=0, attribute_bits_per_picture=0, occupancy_precision=4, forced_precision_bytes=0, log2_ctb=5,
                           rows_per_slice=-1, md5_sei=0, verify_md5=0, gofs_per_job=1, occupancy_rd=0, preset=0):
        """rbt_transcode_v3c_rate -> (sample stream, [(geometry result, attribute result) per GOF of the input])"""
        p = V3CParams(occupancy_precision, geometry_qp, attribute_qp, forced_precision_bytes, log2_ctb, rows_per_slice, md5_sei, verify_md5, gofs_per_job, occupancy_rd, preset)
        out, n, rs = C.c_void_p(), C.c_size_t(), C.POINTER(RateResult)()
        self._chk(self.L.rbt_transcode_v3c_rate(self.h, data, len(data), C.byref(p), geometry_bits_per_picture, attribute_bits_per_picture, C.byref(out), C.byref(n), C.byref(rs)))
        n_gofs = v3c_stats(data, self.L)["n_gofs"]
        per = [(_result_dict(rs[2 * g]), _result_dict(rs[2 * g + 1])) for g in range(n_gofs)]
        self.L.rbt_free(rs)
        return self._take(out, n), per

    def or_pool(self, plane, factor=2):
        plane = np.ascontiguousarray(plane, dtype=np.uint16)
        h, w = plane.shape
        out = np.zeros((h // factor, w // factor), np.uint16)
        self._chk(self.L.rbt_or_pool(self.h, plane.ctypes.data, w, h, factor, out.ctypes.data))
        return out

    def picture_hash(self, frames, w, h, bit_depth, kind=RBT_HASH_MD5):
        """rbt_picture_hash: decoded picture hash of planar 4:2:0 pictures ([n, w*h*3/2] uint16) -> uint8 [n, 3, 16], per component in SEI byte order
        (MD5: 16 bytes; CRC: 2, checksum: 4, most significant first; zero-padded)"""
        frames = np.ascontiguousarray(frames, dtype=np.uint16).reshape(-1, w * h * 3 // 2)
        out = np.zeros((frames.shape[0], 3, 16), np.uint8)
        self._chk(self.L.rbt_picture_hash(self.h, frames.ctypes.data, w, h, bit_depth, frames.shape[0], kind, out.ctypes.data))
        return out

    def reconstruct(self, atlas, patches, occ, d0, d1, geo_bd=10, t0=None, t1=None, attr_bd=10):
        """rbt_reconstruct: (xyz int16 [n,3], yuv uint16 [n,3], occupancy_map uint8 [h,w], block_to_patch uint32 [h/res, w/res])
        atlas: AtlasParams; patches: list of Patch; occ / d0 / d1: luma planes (2-D arrays); t0 / t1: planar 4:2:0 frames (1-D) or None"""
        ps = (Patch * max(1, len(patches)))(*patches)
        arr = [np.ascontiguousarray(x, dtype=np.uint16) if x is not None else None for x in (occ, d0, d1, t0, t1)]
        ptr = [x.ctypes.data if x is not None else None for x in arr]
        c = Cloud()
        self._chk(self.L.rbt_reconstruct(self.h, C.byref(atlas), ps, len(patches), ptr[0], ptr[1], ptr[2], geo_bd, ptr[3], ptr[4], attr_bd, C.byref(c)))
        n, w, h, res = c.n_points, atlas.width, atlas.height, atlas.occupancy_resolution
        xyz = np.ctypeslib.as_array(c.xyz, shape=(max(n, 1), 3))[:n].copy(); yuv = np.ctypeslib.as_array(c.yuv, shape=(max(n, 1), 3))[:n].copy()
        om = np.ctypeslib.as_array(c.occupancy_map, shape=(h, w)).copy(); b2p = np.ctypeslib.as_array(c.block_to_patch, shape=(h // res, w // res)).copy()
        self.n_smoothed = c.n_points and c.n_smoothed      # points the geometry smoothing moved in this call
        self.L.rbt_cloud_free(C.byref(c))
        return xyz, yuv, om, b2p

    def d1(self, a, b, peak=1023):
        """rbt_d1: point-to-point metric between two clouds (int16 [n,3]) -> dict"""
        a = np.ascontiguousarray(a, dtype=np.int16); b = np.ascontiguousarray(b, dtype=np.int16)
        r = D1Result()
        self._chk(self.L.rbt_d1(self.h, a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], peak, C.byref(r)))
        return {n: getattr(r, n) for n, _ in D1Result._fields_}

    def d2(self, a, normals_a, b, peak=1023):
        """rbt_d2: point-to-plane metric; a, b int16 [n,3]; normals_a int16 [n_a,3] in Q14 (16384 = 1.0) -> dict"""
        a = np.ascontiguousarray(a, dtype=np.int16); b = np.ascontiguousarray(b, dtype=np.int16); na = np.ascontiguousarray(normals_a, dtype=np.int16)
        if na.shape != a.shape:
            raise ValueError("one normal per point of a")
        r = D2Result()
        self._chk(self.L.rbt_d2(self.h, a.ctypes.data, na.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], peak, C.byref(r)))
        return {n: getattr(r, n) for n, _ in D2Result._fields_}

    def yuv420_to_yuv444(self, frames, w, h, bit_depth=10, upsample_filter=RBT_UPSAMPLE_F0):
        """rbt_yuv420_to_yuv444: planar 4:2:0 pictures ([n, w*h*3/2] uint16, 8 or 10 bits) -> uint16 [n, 3, h, w], 16-bit 4:4:4 as the decoder converts an attribute video
        (upsample_filter RBT_UPSAMPLE_F0), or the samples replicated with their values unchanged (RBT_UPSAMPLE_REPLICATE)"""
        frames = np.ascontiguousarray(frames, dtype=np.uint16).reshape(-1, w * h * 3 // 2)
        out = np.zeros((frames.shape[0], 3, h, w), np.uint16)
        self._chk(self.L.rbt_yuv420_to_yuv444(self.h, frames.ctypes.data, w, h, bit_depth, frames.shape[0], upsample_filter, out.ctypes.data))
        return out

    def yuv16_to_rgb8(self, yuv):
        """rbt_yuv16_to_rgb8: 16-bit 4:4:4 triples (uint16 [n, 3]) -> uint8 [n, 3], PCCPointSet3::convertYUV16ToRGB8"""
        yuv = np.ascontiguousarray(yuv, dtype=np.uint16).reshape(-1, 3)
        out = np.zeros((yuv.shape[0], 3), np.uint8)
        self._chk(self.L.rbt_yuv16_to_rgb8(self.h, yuv.ctypes.data, yuv.shape[0], out.ctypes.data))
        return out

    def reconstruct_rgb(self, atlas, patches, occ, d0, d1, geo_bd=10, t0=None, t1=None, attr_bd=10, upsample_filter=RBT_UPSAMPLE_F0):
        """rbt_reconstruct_rgb: reconstruct with the colours as the decoder leaves them -> (xyz, yuv uint16 [n,3] = the 16-bit 4:4:4 samples at each point's pixel,
        occupancy_map, block_to_patch, rgb uint8 [n,3])"""
        ps = (Patch * max(1, len(patches)))(*patches)
        arr = [np.ascontiguousarray(x, dtype=np.uint16) if x is not None else None for x in (occ, d0, d1, t0, t1)]
        ptr = [x.ctypes.data if x is not None else None for x in arr]
        c, rgb_p = Cloud(), C.c_void_p()
        self._chk(self.L.rbt_reconstruct_rgb(self.h, C.byref(atlas), ps, len(patches), ptr[0], ptr[1], ptr[2], geo_bd, ptr[3], ptr[4], attr_bd, upsample_filter, C.byref(c), C.byref(rgb_p)))
        n, w, h, res = c.n_points, atlas.width, atlas.height, atlas.occupancy_resolution
        xyz = np.ctypeslib.as_array(c.xyz, shape=(max(n, 1), 3))[:n].copy(); yuv = np.ctypeslib.as_array(c.yuv, shape=(max(n, 1), 3))[:n].copy()
        om = np.ctypeslib.as_array(c.occupancy_map, shape=(h, w)).copy(); b2p = np.ctypeslib.as_array(c.block_to_patch, shape=(h // res, w // res)).copy()
        rgb = np.frombuffer(C.string_at(rgb_p, 3 * n), np.uint8).reshape(n, 3).copy()
        self.n_smoothed = c.n_points and c.n_smoothed
        self.L.rbt_free(rgb_p); self.L.rbt_cloud_free(C.byref(c))
        return xyz, yuv, om, b2p, rgb

    def color_metric(self, a, rgb_a, b, rgb_b):
        """rbt_color_metric: colour PSNR between two clouds (xyz int16 [n,3], rgb uint8 [n,3]) -> dict; every field but n_a / n_b is a list [Y, U, V]"""
        a = np.ascontiguousarray(a, dtype=np.int16); b = np.ascontiguousarray(b, dtype=np.int16)
        ca = None if rgb_a is None else np.ascontiguousarray(rgb_a, dtype=np.uint8); cb = None if rgb_b is None else np.ascontiguousarray(rgb_b, dtype=np.uint8)
        if (ca is not None and ca.shape != a.shape) or (cb is not None and cb.shape != b.shape):
            raise ValueError("one colour per point")
        r = ColorResult()
        self._chk(self.L.rbt_color_metric(self.h, a.ctypes.data, None if ca is None else ca.ctypes.data, a.shape[0], b.ctypes.data, None if cb is None else cb.ctypes.data, b.shape[0], C.byref(r)))
        return {n: (getattr(r, n) if n in ("n_a", "n_b") else list(getattr(r, n))) for n, _ in ColorResult._fields_}

    def color_stage_ms(self):
        """rbt_color_stage_ms + rbt_transfer_stage: device milliseconds of the last up-conversion, RGB conversion, colour metric (the device_ms of its
        score: search, walks and sums, the index building outside) and attribute transfer of this context"""
        ms = (C.c_double * 3)(); t = C.c_double()
        self._chk(self.L.rbt_color_stage_ms(self.h, ms))
        self._chk(self.L.rbt_transfer_stage(self.h, C.byref(t), None))
        return {"upconvert": ms[0], "rgb": ms[1], "metric": ms[2], "transfer": t.value}

    def transfer_colors(self, src_xyz, src_yuv, tgt_xyz, tgt_yuv, moved):
        """rbt_transfer_colors: the attribute transfer after geometry smoothing on its own. src_* : the cloud before smoothing (int16 [n,3], uint16 [n,3]); tgt_xyz: the
        cloud after it, tgt_yuv its colours before the transfer, moved: one flag per target point -> (yuv uint16 [n_tgt,3] after the transfer, n_changed)"""
        sx = np.ascontiguousarray(src_xyz, dtype=np.int16).reshape(-1, 3); sc = np.ascontiguousarray(src_yuv, dtype=np.uint16).reshape(-1, 3)
        tx = np.ascontiguousarray(tgt_xyz, dtype=np.int16).reshape(-1, 3); out = np.array(tgt_yuv, dtype=np.uint16).reshape(-1, 3)
        mv = np.ascontiguousarray(np.asarray(moved) != 0, dtype=np.uint8).reshape(-1)
        if sc.shape != sx.shape or out.shape != tx.shape or mv.shape[0] != tx.shape[0]:
            raise ValueError("one colour per point and one flag per target point")
        n = C.c_int()
        self._chk(self.L.rbt_transfer_colors(self.h, sx.ctypes.data, sc.ctypes.data, sx.shape[0], tx.ctypes.data, out.ctypes.data, mv.ctypes.data, tx.shape[0], C.byref(n)))
        return out, n.value

    def reconstruct_decoded(self, atlas, patches, occ, d0, d1, geo_bd=10, t0=None, t1=None, attr_bd=10, upsample_filter=RBT_UPSAMPLE_F0, attr_transfer=1):
        """rbt_reconstruct_decoded: reconstruct_rgb, then the colours of the points the geometry smoothing moved are transferred from the unsmoothed cloud as the reference
        decoder does (attr_transfer=1; 0 = off) -> (xyz, yuv, occupancy_map, block_to_patch, rgb, moved uint8 [n]); self.n_changed = colours the transfer changed"""
        ps = (Patch * max(1, len(patches)))(*patches)
        arr = [np.ascontiguousarray(x, dtype=np.uint16) if x is not None else None for x in (occ, d0, d1, t0, t1)]
        ptr = [x.ctypes.data if x is not None else None for x in arr]
        c, rgb_p, mv_p = Cloud(), C.c_void_p(), C.c_void_p()
        self._chk(self.L.rbt_reconstruct_decoded(self.h, C.byref(atlas), ps, len(patches), ptr[0], ptr[1], ptr[2], geo_bd, ptr[3], ptr[4], attr_bd, upsample_filter, attr_transfer,
                                                 C.byref(c), C.byref(rgb_p), C.byref(mv_p)))
        n, w, h, res = c.n_points, atlas.width, atlas.height, atlas.occupancy_resolution
        xyz = np.ctypeslib.as_array(c.xyz, shape=(max(n, 1), 3))[:n].copy(); yuv = np.ctypeslib.as_array(c.yuv, shape=(max(n, 1), 3))[:n].copy()
        om = np.ctypeslib.as_array(c.occupancy_map, shape=(h, w)).copy(); b2p = np.ctypeslib.as_array(c.block_to_patch, shape=(h // res, w // res)).copy()
        rgb = np.frombuffer(C.string_at(rgb_p, 3 * n), np.uint8).reshape(n, 3).copy()
        moved = np.frombuffer(C.string_at(mv_p, n), np.uint8).copy()
        self.n_smoothed = c.n_points and c.n_smoothed
        ch = C.c_int(); self._chk(self.L.rbt_transfer_stage(self.h, None, C.byref(ch))); self.n_changed = ch.value
        self.L.rbt_free(rgb_p); self.L.rbt_free(mv_p); self.L.rbt_cloud_free(C.byref(c))
        return xyz, yuv, om, b2p, rgb, moved

    def pcloud_upload(self, xyz, rgb=None, normals=None):
        """rbt_pcloud_upload: xyz int16 [n,3], rgb uint8 [n,3] or None, normals int16 [n,3] in Q14 or None -> PCloud"""
        a = np.ascontiguousarray(xyz, dtype=np.int16).reshape(-1, 3)
        c = None if rgb is None else np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1, 3); nr = None if normals is None else np.ascontiguousarray(normals, dtype=np.int16).reshape(-1, 3)
        if (c is not None and c.shape != a.shape) or (nr is not None and nr.shape != a.shape):
            raise ValueError("one colour and one normal per point")
        h = C.c_void_p()
        self._chk(self.L.rbt_pcloud_upload(self.h, a.ctypes.data, None if c is None else c.ctypes.data, None if nr is None else nr.ctypes.data, a.shape[0], C.byref(h)))
        return PCloud(self, h)

    def pcloud_from_maps(self, atlas, patches, occ, d0, d1, geo_bd=10, t0=None, t1=None, attr_bd=10, upsample_filter=RBT_UPSAMPLE_F0, attr_transfer=1, host_copy=False):
        """rbt_pcloud_from_maps: reconstruct_decoded whose cloud stays on the device -> PCloud, or with host_copy (PCloud, (xyz, yuv, occupancy_map, block_to_patch, rgb));
        self.n_smoothed / self.n_changed as after reconstruct_decoded"""
        ps = (Patch * max(1, len(patches)))(*patches)
        arr = [np.ascontiguousarray(x, dtype=np.uint16) if x is not None else None for x in (occ, d0, d1, t0, t1)]
        ptr = [x.ctypes.data if x is not None else None for x in arr]
        h, c, rgb_p = C.c_void_p(), Cloud(), C.c_void_p()
        self._chk(self.L.rbt_pcloud_from_maps(self.h, C.byref(atlas), ps, len(patches), ptr[0], ptr[1], ptr[2], geo_bd, ptr[3], ptr[4], attr_bd, upsample_filter, attr_transfer, C.byref(h),
                                              C.byref(c) if host_copy else None, C.byref(rgb_p) if host_copy else None))
        ch = C.c_int(); self._chk(self.L.rbt_transfer_stage(self.h, None, C.byref(ch))); self.n_changed = ch.value
        cloud = PCloud(self, h)
        if not host_copy:
            return cloud
        n, w, hh, res = c.n_points, atlas.width, atlas.height, atlas.occupancy_resolution
        xyz = np.ctypeslib.as_array(c.xyz, shape=(max(n, 1), 3))[:n].copy(); yuv = np.ctypeslib.as_array(c.yuv, shape=(max(n, 1), 3))[:n].copy()
        om = np.ctypeslib.as_array(c.occupancy_map, shape=(hh, w)).copy(); b2p = np.ctypeslib.as_array(c.block_to_patch, shape=(hh // res, w // res)).copy()
        rgb = np.frombuffer(C.string_at(rgb_p, 3 * n), np.uint8).reshape(n, 3).copy()
        self.n_smoothed = c.n_points and c.n_smoothed
        self.L.rbt_free(rgb_p); self.L.rbt_cloud_free(C.byref(c))
        return cloud, (xyz, yuv, om, b2p, rgb)

    def estimate_normals(self, xyz, params=None):
        """rbt_estimate_normals: xyz int16 [n,3] -> normals int16 [n,3] in Q14 (params: NormalsParams or None = defaults)"""
        a = np.ascontiguousarray(xyz, dtype=np.int16).reshape(-1, 3)
        out = np.empty(a.shape, np.int16)
        self._chk(self.L.rbt_estimate_normals(self.h, a.ctypes.data, a.shape[0], None if params is None else C.byref(params), out.ctypes.data))
        return out

    def score(self, a, b, peak=1023, parts=0, raw=False):
        """rbt_score: a = the source PCloud, b = the decoded one; parts = RBT_SCORE_* wanted, 0 = all the clouds allow -> frame_score_dict, or the FrameScore itself (raw)"""
        s = FrameScore()
        self._chk(self.L.rbt_score(self.h, a.h if a is not None else None, b.h if b is not None else None, peak, parts, C.byref(s)))
        return s if raw else frame_score_dict(s)

    def score_patches(self, a, b, n_patches, peak=1023, raw=False):
        """rbt_score_patches: a = the reference PCloud, b = the decoded one with its labels -> (one dict per patch - or the PatchD1 array itself (raw) -, the whole
        frame's D1 as rbt_score returns it, device_ms)"""
        out = (PatchD1 * max(1, n_patches))(); whole = D1Result(); ms = C.c_double()
        self._chk(self.L.rbt_score_patches(self.h, a.h if a is not None else None, b.h if b is not None else None, peak, n_patches, out, C.byref(whole), C.byref(ms)))
        return (out if raw else [patch_d1_dict(out[k]) for k in range(n_patches)]), (whole if raw else _result_dict(whole)), ms.value

    def score_patches_d2(self, a, b, n_patches, peak=1023, raw=False):
        """rbt_score_patches_d2: a = the source PCloud with normals, b = the decoded one with its labels -> (one dict per patch - or the PatchD2 array itself (raw) -, the
        whole frame's D2 as rbt_score returns it, device_ms)"""
        out = (PatchD2 * max(1, n_patches))(); whole = D2Result(); ms = C.c_double()
        self._chk(self.L.rbt_score_patches_d2(self.h, a.h if a is not None else None, b.h if b is not None else None, peak, n_patches, out, C.byref(whole), C.byref(ms)))
        return (out if raw else [patch_d2_dict(out[k]) for k in range(n_patches)]), (whole if raw else _result_dict(whole)), ms.value

    def score_patches_color(self, a, b, n_patches, raw=False):
        """rbt_score_patches_color: a = the source PCloud, b = the decoded one with its labels, both with colours -> (one dict per patch - or the PatchColor array itself
        (raw) -, the whole frame's colour result as rbt_score returns it, device_ms)"""
        out = (PatchColor * max(1, n_patches))(); whole = ColorResult(); ms = C.c_double()
        self._chk(self.L.rbt_score_patches_color(self.h, a.h if a is not None else None, b.h if b is not None else None, n_patches, out, C.byref(whole), C.byref(ms)))
        return (out if raw else [patch_color_dict(out[k]) for k in range(n_patches)]), (whole if raw else _result_dict(whole)), ms.value

    def score_pair(self, a, b):
        """rbt_score_pair_create: a = the source PCloud, b = the decoded one -> ScorePair"""
        return ScorePair(self, a, b)

    def gather_420(self, src, stride, rows, chroma_stride, chroma_rows, x0, y0, w, h, src_misalign=0):
        """rbt_gather_420: coded 4:2:0 pictures src ([n, stride*rows + 2*chroma_stride*chroma_rows] uint16: luma plane, Cb, Cr) -> the even w x h window at (x0, y0) of
        each as packed planar 4:2:0 ([n, w*h*3/2]); the pictures lie src_misalign samples behind a 256-byte boundary on the device"""
        src = np.ascontiguousarray(src, dtype=np.uint16)
        n = src.shape[0]
        if src.ndim != 2 or src.shape[1] != stride * rows + 2 * chroma_stride * chroma_rows:
            raise ValueError("a picture is its luma plane followed by the two chroma planes")
        out = np.zeros((n, max(0, w * h * 3 // 2)), np.uint16)
        self._chk(self.L.rbt_gather_420(self.h, src.ctypes.data, n, stride, rows, chroma_stride, chroma_rows, x0, y0, w, h, src_misalign, out.ctypes.data))
        return out

    def selftest_transform32(self, blocks, bit_depth=10):
        """rbt_selftest_transform32: matrix-core vs vector-ALU 32-point transforms on int16 blocks [n, 1024]; returns the number of differing samples"""
        blocks = np.ascontiguousarray(blocks, dtype=np.int16)
        bad = C.c_uint32()
        self._chk(self.L.rbt_selftest_transform32(self.h, blocks.ctypes.data, blocks.shape[0], bit_depth, C.byref(bad)))
        return bad.value

    def selftest_tb(self, cases, nb, unit_av, levels):
        """rbt_selftest_tb: transform blocks through the decoder's own routine. cases int32 [n, 16] (the fields of rbt_tb_case in order), nb uint16 [n, 2, 129],
        unit_av uint8 [n, 33], levels int16 [n, 2, 1024] -> uint16 [n, 2, 1024]"""
        cases = np.ascontiguousarray(cases, dtype=np.int32); n = cases.shape[0]
        nb = np.ascontiguousarray(nb, dtype=np.uint16); unit_av = np.ascontiguousarray(unit_av, dtype=np.uint8); levels = np.ascontiguousarray(levels, dtype=np.int16)
        if cases.shape != (n, 16) or nb.shape != (n, 2, 129) or unit_av.shape != (n, 33) or levels.shape != (n, 2, 1024):
            raise ValueError("selftest_tb: array shapes")
        out = np.zeros((n, 2, 1024), np.uint16)
        self._chk(self.L.rbt_selftest_tb(self.h, cases.ctypes.data, n, nb.ctypes.data, unit_av.ctypes.data, levels.ctypes.data, out.ctypes.data))
        return out

    def flat_pictures(self):
        """rbt_flat_pictures: decoded pictures of the last collected job or decode that were reconstructed with flat chroma"""
        self.L.rbt_flat_pictures.argtypes = [C.c_void_p]      # (declared here: load() also serves builds from before the function, which comparisons of two libraries put side by side)
        return int(self.L.rbt_flat_pictures(self.h))

    def stats(self):
        s = Stats()
        self._chk(self.L.rbt_get_stats(self.h, C.byref(s)))
        return {n: getattr(s, n) for n, _ in Stats._fields_}


# The jobs with targets and results: Context.submit_gof_<name>, .wait_gof_<name> and .transcode_gof_<name> over rbt_submit_gof_<name>, rbt_wait_gof_<name> and
# rbt_transcode_gof_<name>. Per name: the target type, the result type, how ([stream bytes, ...], [result dict, ...]) is finished (None: as it is), what the targets are
# (submit's docstring) and what wait's docstring adds
_GOF_KINDS = {
    "rate": (RateTarget, RateResult, None, "submit_gof with one RateTarget per entry (target_bytes 0 = constant QP)", ""),
    "quality": (QualityTarget, QualityResult, None, "submit_gof with one QualityTarget per entry (min_psnr_mdb 0 = constant QP, distortion reported)", ""),
    "d1_frames": (D1Target, FrameFloorResult, Context._frame_results, "submit_gof_d1 with the floor held by every point-cloud frame on its own (stat must be RBT_D1_MIN)",
                  "; d1: the D1 dict of every frame at its pick"),
    "quality_frames": (QualityTarget, FrameFloorResult, Context._frame_results, "submit_gof_quality with the floor held by every point-cloud frame on its own", ""),
    "quality_patches": (PatchFloorTarget, PatchFloorResult, Context._patch_results,
                        "submit_gof with one PatchFloorTarget per entry (PatchFloorTarget() = none): every patch of every frame holds its floor", ""),
    # a frame with the whole frame's d1 as a dict, a pick with its d1 as a patch_d1_dict
    "d1_patches": (PatchD1Target, PatchD1Result,
                   lambda self, res: self._patch_results(res, lambda f: dict(_result_dict(f), d1=_result_dict(f.d1)), lambda p: dict(_result_dict(p), d1=patch_d1_dict(p.d1))),
                   "submit_gof with one PatchD1Target per entry (PatchD1Target() = none): every patch of every frame of a geometry entry holds its D1 floor", ""),
    "d1": (D1Target, D1FloorResult, Context._d1_results, "submit_gof with one D1Target per entry (D1Target() = none; min_d1_mdb 0 = constant QP, D1 reported)", ""),
    "d2": (D2Target, D2FloorResult, Context._d2_results, "submit_gof with one D2Target per entry (D2Target() = none; min_d2_mdb 0 = constant QP, D2 reported)", ""),
    "d2_patches": (PatchD2Target, PatchD2Result,
                   lambda self, res: self._patch_results(res, lambda f: dict(_result_dict(f), d2=_result_dict(f.d2)), lambda p: dict(_result_dict(p), d2=patch_d2_dict(p.d2))),
                   "submit_gof with one PatchD2Target per entry (PatchD2Target() = none): every patch of every frame of a geometry entry holds its D2 floor", ""),
    "color_patches": (PatchColorTarget, PatchColorResult,
                      lambda self, res: self._patch_results(res, lambda f: dict(_result_dict(f), color=_result_dict(f.color)), lambda p: dict(_result_dict(p), color=patch_color_dict(p.color))),
                      "submit_gof with one PatchColorTarget per entry (PatchColorTarget() = none): every patch of every frame of an attribute entry holds its colour PSNR floor", ""),
    "color": (ColorTarget, ColorFloorResult, Context._color_results,
              "submit_gof with one ColorTarget per entry (ColorTarget() = none; min_psnr_mdb 0 = constant QP, colour results reported)", ""),
}


def _gof_kind(name, target_type, result_type, finish, what, wait_adds):
    finish = finish or (lambda self, res: res)

    def submit(self, streams, params, targets):
        return self._submit(getattr(self.L, "rbt_submit_gof_" + name), streams, params, targets, target_type)

    def wait(self, job):
        return finish(self, self._collect(getattr(self.L, "rbt_wait_gof_" + name), job[1], [job[0]], result_type))

    def transcode(self, streams, params, targets):
        args = self._gof_args(streams, params, targets, target_type)
        return finish(self, self._collect(getattr(self.L, "rbt_transcode_gof_" + name), args[0], args, result_type))

    submit.__doc__ = "rbt_submit_gof_%s: %s; returns a job for wait_gof_%s" % (name, what, name)
    wait.__doc__ = "rbt_wait_gof_%s -> ([stream bytes, ...], [result dict, ...])%s" % (name, wait_adds)
    transcode.__doc__ = "rbt_transcode_gof_%s: submit + wait" % name
    for f, part in ((submit, "submit"), (wait, "wait"), (transcode, "transcode")):
        f.__name__ = "%s_gof_%s" % (part, name)
        f.__qualname__ = "Context." + f.__name__
        setattr(Context, f.__name__, f)


for _name, _kind in _GOF_KINDS.items():
    _gof_kind(_name, *_kind)
