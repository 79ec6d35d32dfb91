/* rbt.h — C ABI of librbt.so, the MI355X-native replacement of the V-PCC transcoding hot path.
 *
 * Drop-in boundary: the reference's
 *     void PCCTranscoder::transcodeVideo(PCCVideoBitstream& videoBitstream, PCCVideoType type)
 *     (source/lib/PccLibTranscoder/include/PCCTranscoder.h:105, source/PCCTranscoder.cpp:374-546)
 * which decodes one HEVC sub-bitstream of a GOF with libavcodec, OR-pools the occupancy luma plane when
 * occupancyPrecision == 4 (resize_frame2, PCCTranscoder.cpp:594-646) and re-encodes it with libx265
 * (setEncoderOptions :825-904, encodeVideo :548-592). rbt_transcode_substream() has the same contract on plain
 * pointers: Annex-B in, Annex-B out, parameters from PCCTranscoderParameters (PCCTranscoderParameters.h:58-80).
 * INTEGRATION.md shows the ten-line patch of transcodeVideo that calls it.
 *
 * Everything runs on the GPU selected at rbt_create(); there is no CPU fallback: every entry point returns
 * RBT_ERR_NO_DEVICE if no HIP device is usable.
 */
#ifndef RBT_H
#define RBT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rbt_ctx rbt_ctx;

enum {
  RBT_OK = 0,
  RBT_ERR_NO_DEVICE = -1,     /* no usable HIP device / HIP runtime error */
  RBT_ERR_BITSTREAM = -2,     /* corrupt or truncated input */
  RBT_ERR_UNSUPPORTED = -3,   /* stream uses a tool outside the V-PCC CTC toolset (B slices, tiles, PCM, ...) */
  RBT_ERR_PARAM = -4,
  RBT_ERR_NOMEM = -5,
  RBT_ERR_MD5 = -6,           /* decoded picture hash SEI mismatch on the input stream */
  RBT_ERR_BUSY = -7,          /* rbt_submit_gof: the announced number of transcodes is already in flight */
  RBT_ERR_OUTPUT = -8         /* a slice's coded data is larger than the output buffer sized for it; not a shortage of device memory: running the job
                               * again, alone or later, gives the same result */
};

/* PCCVideoType values the reference passes (PCCBitstreamCommon.h:79-118) */
enum { RBT_VIDEO_OCCUPANCY = 0, RBT_VIDEO_GEOMETRY = 1, RBT_VIDEO_ATTRIBUTE = 19 };

typedef struct {
  int video_type;            /* RBT_VIDEO_* (transcodeVideo's `type`) */
  int qp;                    /* geometryQP_ / attributeQP_ / occupancyMapQP_ (PCCTranscoderParameters.h:58-80) */
  int occupancy_precision;   /* occupancyPrecision_: 4 => 2x2 OR-pool of the occupancy map (PCCTranscoder.cpp:466) */
  int log2_ctb;              /* encoder CTB size, 0 = default (5) */
  int ctb_rows_per_slice;    /* encoder slice structure: n > 0 = independent slices of n CTB rows; 0 = one slice per picture; -1 = wavefront mode, one slice per
                              * picture coded as one dependent slice segment per CTB row with entropy_coding_sync (rows predict from each other and inherit
                              * context variables: ~11 % fewer bytes than 1 at the same PSNR; what the CTC rate points use, gof_shard.DEFAULT_ROWS).
                              * All streams of one call must agree on wavefront mode or not. */
  int md5_sei;               /* RBT_HASH_*: kind of decoded picture hash SEI written behind every output picture (0 = none; 1 = MD5, as before). Hashed on the GPU from the
                              * encoder's reconstruction; values above RBT_HASH_CHECKSUM: RBT_ERR_PARAM */
  int verify_md5;            /* check the input stream's decoded picture hash SEIs, whichever kind each picture carries (MD5, CRC or checksum), on the GPU after the
                              * decoder's last filter: a mismatch fails the call with RBT_ERR_MD5 (rbt_last_error names the input) and no output */
  int occupancy_rd;          /* geometry / attribute streams handed to rbt_transcode_gof / rbt_submit_gof behind an occupancy stream that is transcoded in the same call
                              * (occupancy_precision 4): occupancy-aware coding (what dependencies/hm-modification/HM-16.20+SCM-8.8_with_RDO.patch does to
                              * HM's distortion, TComRdCost.cpp xGetSSE*). The occupancy map the output carries tells which 4x4 units the decoder makes points of; with one unit
                              * of margin around them, transform blocks outside carry no residual, partly occupied blocks code what their occupied samples ask for, and the
                              * unoccupied samples stay out of the encoder's distortion terms. Measured on the benchmark GOF at R3: 67 % fewer geometry and 30 % fewer
                              * attribute bytes, mean D1 over the GOF's four base atlases -0.08 dB (67.14 -> 67.06 dB; a single frame scatters by +-0.3 dB either way, frame 0: -0.05 dB), PSNR of the occupied samples -0.04 / -0.02 dB (tests/test_gpu_transcode.py holds both within 0.1 dB). The pictures outside the occupied area are then whatever
                              * prediction leaves there. Entries come GOF by GOF, occupancy first; ignored where the call holds no such occupancy stream, by
                              * rbt_transcode_substream (one stream) and for lossless streams; not together with verify_md5 (RBT_ERR_PARAM). 0 = off: every sample counts. */
  int preset;                /* RBT_PRESET_*: what the reference's `preset` (PCCTranscoderParameters.h:58, handed to libx265 at PCCTranscoder.cpp:877,883) selects here.
                              * RBT_PRESET_DEFAULT (0, x265 "veryfast" and slower): every decision tool of RBT-E1. RBT_PRESET_FAST (1, "ultrafast", "superfast"):
                              * the open-loop decisions only - no SATD block costs, no closed-loop mode choice, no coded mode trial, fixed rounding: 16 % more bytes at the same
                              * QP (benchmark GOF: out / in 0.382 instead of 0.329, D1 67.80 instead of 67.94 dB), 2-3 % faster (805 against 779 point-cloud frames/s for a
                              * 20-GOF run).
                              * rbt_preset_from_name maps the reference's strings. */
} rbt_stream_params;
enum { RBT_PRESET_DEFAULT = 0, RBT_PRESET_FAST = 1 };

/* Kinds of decoded picture hash (H.265 D.3.19), numbered as HM's SEIDecodedPictureHash and x265's --hash: the SEI's hash_type is kind - 1 */
enum { RBT_HASH_NONE = 0, RBT_HASH_MD5 = 1, RBT_HASH_CRC = 2, RBT_HASH_CHECKSUM = 3 };

typedef struct {             /* decoded video returned by rbt_decode (host memory, rbt_free) */
  int width, height, bit_depth, n_frames;
  uint16_t* data;            /* n_frames x planar 4:2:0: Y (w*h), Cb, Cr */
  int md5_checked, md5_failed;   /* with verify_md5: pictures whose decoded picture hash SEI was checked / did not match, of any kind (MD5, CRC, checksum) */
} rbt_video;

typedef struct {             /* timings of the last call, milliseconds */
  double host_parse_ms, h2d_ms, gpu_ms, d2h_ms, host_pack_ms, total_ms;
  double k_parse_ms, k_recon_ms, k_filter_ms, k_analyse_ms, k_encode_ms, k_entropy_ms;
  uint64_t algorithmic_bytes; /* SURVEY.md 8(d) accounting of the call */
} rbt_stats;

/* One context per host thread and GPU. `device` is the HIP device the context's work runs on; streams, timers, job slots and the
 * recycling pool of device memory are per device, so contexts on different devices may be used concurrently from different threads
 * (contexts on the same device share its 16 HIP streams and job slots and are serialised by the library).
 * world_rank / world_size describe the multi-GPU job the context is part of (one process per GPU): the library owns
 * the GOF sharding rule (rbt_owns_gof), the NAL gather itself runs in the host program over RCCL. 0 <= world_rank < world_size. */
int rbt_create(rbt_ctx** ctx, int device, int world_rank, int world_size);
/* GOF g of a sequence is transcoded by rank g mod world_size; a host that walks the sequence GOF by GOF (PccAppTranscoder.cpp:307-341)
 * on every rank skips what its context does not own. Returns 1 / 0. */
int rbt_owns_gof(const rbt_ctx* ctx, int gof_index);
int rbt_world(const rbt_ctx* ctx, int* world_rank, int* world_size);
void rbt_destroy(rbt_ctx* ctx);
const char* rbt_strerror(int code);
const char* rbt_last_error(rbt_ctx* ctx);   /* what the LAST call on this context had to say if it failed (e.g. which syntax element it rejected); "" if it succeeded or gave no
                                              * detail: every entry point that takes the context starts by clearing the text. The pointer is valid until the next call on the context. */
void rbt_free(void* p);
const char* rbt_version(void);

/* transcodeVideo: one Annex-B HEVC sub-bitstream of a GOF -> re-encoded Annex-B stream (malloc'd, rbt_free). */
int rbt_transcode_substream(rbt_ctx* ctx, const uint8_t* annexb_in, size_t n_in, const rbt_stream_params* p, uint8_t** annexb_out, size_t* n_out);

/* transcodeData (PCCTranscoder.cpp:145-168): the sub-bitstreams of one GOF in one call, each as its own pipeline on its own
 * HIP stream. As in the reference (:150), an occupancy stream is only transcoded when occupancy_precision == 4; with any other
 * precision it is returned unchanged (rbt_transcode_substream, like transcodeVideo, re-encodes whatever it is handed).
 * Entries that name the same input buffer (same pointer and size) with different parameters are decoded once and re-encoded once
 * per entry: the rate fan-out of BASELINE.json configs[4] (R1..R5 from one R5 input) on one GPU. More than three streams (the sub-bitstreams of several GOFs: one GOF leaves most of an MI355X idle) are grouped
 * by video type into three pipelines. Outputs come back in input order. */
#define RBT_MAX_STREAMS 96
int rbt_transcode_gof(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, uint8_t** annexb_out, size_t* n_out);

/* rbt_transcode_gof in two halves, for the caller that walks a sequence GOF by GOF (PccAppTranscoder.cpp:307-341 calls
 * transcode -> transcodeData, PCCTranscoder.cpp:66-70 / :145-168, once per GOF): submit builds the batch and enqueues every
 * kernel of the GOF, wait collects the streams.
 * Several transcodes may be in flight; they use disjoint HIP streams, so the entropy decoding of GOF i+1 (a few hundred lone
 * waves) runs underneath the entropy decoding, reconstruction and re-encode of GOF i. The input buffers may be released as soon
 * as submit returns. Jobs may be waited for in any order; every submitted job must be waited for (rbt_destroy drains what is
 * left). Results are identical to rbt_transcode_gof's. Calls on one device are serialised by the library (a wait blocks a
 * concurrent submit from another thread on the same GPU).
 * rbt_set_depth announces how many jobs the caller keeps in flight (1..RBT_MAX_JOBS, default 4; per device; refused with
 * RBT_ERR_BUSY while jobs are in flight): the library has 16 HIP streams (more hardware queues slow every queue down on
 * MI355X), so up to 4 jobs get four streams each, 5 get three, up to 8 two, up to 16 one (pipelines that share a stream run
 * their entropy decoding and their reconstruction in merged launches). rbt_submit_gof returns RBT_ERR_BUSY when that many
 * jobs are already in flight.
 * Every shape above assumes that each of the 16 streams has a hardware queue of its own (streams that share a queue serialise). The HIP
 * runtime has 4 unless GPU_MAX_HW_QUEUES says otherwise, and reads that once, when it initialises. The first rbt_create of a process
 * therefore sets GPU_MAX_HW_QUEUES=16 before its first HIP call, over a value that is already there (RBT_HW_QUEUES=<1..32> chooses
 * another count and, since GPU_MAX_HW_QUEUES is overwritten, is the only way to choose it for such a process; RBT_HW_QUEUES=4 gives the
 * runtime's default back, fewer than 4 is accepted and untested). The library cannot change the count in a process that has used
 * HIP before - a host application with HIP code of its own, a framework that selected its device first: such a process sets
 * GPU_MAX_HW_QUEUES=16 in its own environment, or creates the context before its first HIP call. */
#define RBT_MAX_JOBS 16
typedef struct rbt_job rbt_job;
int rbt_set_depth(rbt_ctx* ctx, int max_in_flight);
int rbt_get_depth(rbt_ctx* ctx);   /* the announced depth (> 0) or RBT_ERR_PARAM */
/* How to cut a walk of n_gofs GOFs into jobs on one GPU, as measured on 1280x1280 maps: 16 jobs of 3 GOFs for a long walk (96 GOFs and more; 2 GOFs from 48: the
 * arenas of 48 GOFs in flight are 209 GB at that size (4.35 GB per GOF, rbt_job_memory; 4.12 GB when the shapes were measured: 64 in flight fit too and run no faster). The shape looks at the length of the walk only; rbt_transcode_v3c bounds the jobs it keeps in flight by the memory the
 * first job took (rbt_job_memory against rbt_device_memory) and falls back to one GOF per job, one job at a time, when a job still fails with RBT_ERR_NOMEM; a caller
 * that drives rbt_submit_gof itself does the same or passes its own shape); a walk shorter than 48 GOFs is all ramp-up and
 * drain and does better as at most 7 jobs (2 jobs up to 12 GOFs) of ceil(n / jobs) GOFs, which then own several hardware queues each. max_jobs caps the jobs in flight. */
int rbt_job_shape(int n_gofs, int max_jobs, int* gofs_per_job, int* jobs_in_flight);
/* The reference's `preset` string (an x265 preset name, PCCTranscoderParameters.h:58) as RBT_PRESET_*: "ultrafast", "superfast" -> RBT_PRESET_FAST; "veryfast"
 * (what the reference's scripts pass, transcode.sh:18), "faster", "fast", "medium", "slow", "slower", "veryslow", "placebo" and NULL / "" -> RBT_PRESET_DEFAULT (even x265's
 * "veryfast" decides by rate-distortion cost, which RBT_PRESET_FAST does not); anything else -> RBT_ERR_PARAM. */
int rbt_preset_from_name(const char* name);
int rbt_submit_gof(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, rbt_job** job);
/* Device memory as the library sees it, for callers that size their own pipelines (rbt_transcode_v3c does: jobs in flight are bounded by it). free_bytes / total_bytes: the
 * driver's figures; cached_bytes: arenas of collected jobs kept for the next job of the same shape (handed back before an allocation fails; rbt_trim); in_use_bytes: arenas
 * of jobs in flight; reserve_bytes: what a new arena leaves free for the HIP runtime's own allocations (scratch memory of the hardware queues: 3 GB unless the environment
 * variable RBT_HBM_RESERVE_MB says otherwise) - an arena that would cut into it fails with RBT_ERR_NOMEM and the context stays usable. */
typedef struct { size_t total_bytes, free_bytes, cached_bytes, in_use_bytes, reserve_bytes; } rbt_memory;
int rbt_device_memory(rbt_ctx* ctx, rbt_memory* out);
/* Device memory a submitted job holds (its decoder and encoder arenas); what the next job of the same shape will take. */
int rbt_job_memory(rbt_ctx* ctx, const rbt_job* job, size_t* bytes);
int rbt_wait_gof(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out);
/* The library keeps the device memory of collected jobs for the next job of the same shape (hipMalloc / hipFree of GOF-sized arenas cost milliseconds
 * and hipFree drains the device). rbt_trim hands that cache back to the driver: worth calling when the workload changes shape (other picture sizes, other
 * numbers of streams per job), so that the old shapes do not crowd the 288 GB. RBT_ERR_BUSY while jobs are in flight on the device. */
int rbt_trim(rbt_ctx* ctx);

/* ---- a QP per point-cloud frame (host/rbt_transcode.cpp encode_plan) ----
 * rbt_submit_gof codes every picture of an entry from one QP. Here an entry may carry a list with one QP per point-cloud frame: the constant-quality building block beside
 * constant QP (the frames of a GOF scatter by several dB of D1 at one QP). The encoder kernels read the QP from the slice descriptor, so nothing on the device
 * changes: the list reaches the slices of each picture, and the slice headers carry the difference to the picture parameter set.
 *
 * 1. Frames. A geometry / attribute entry has 2 output pictures per point-cloud frame: frame f is output pictures 2f and 2f + 1, an I picture and a zero-motion P picture
 *    that refers to it; nothing crosses a frame. n_frames must equal pictures / 2.
 * 2. QPs. With Q = the list, picture 2f is coded at max(0, Q[f] - 3) and picture 2f + 1 at Q[f], exactly as the constant-QP path derives them from qp. 0 <= Q[f] <= 51.
 * 3. Parameter sets. They are those of rbt_transcode_gof at params[i].qp - init_qp_minus26 comes from params[i].qp -; only slice_qp_delta differs from picture to picture.
 * 4. Identity. If every Q[f] == params[i].qp the output is byte for byte rbt_transcode_gof's.
 * 5. Composition. With C(q) = rbt_transcode_gof's stream at qp = q and everything else equal: decoded pictures 2f and 2f + 1 of the output equal those of C(Q[f]) sample
 *    for sample; the picture hash SEI NAL units behind them (md5_sei) are byte for byte those of C(Q[f]); each slice NAL differs in length from its counterpart in C(Q[f])
 *    by at most 2 bytes - the width of slice_qp_delta (se(v) of a difference of up to 51: 1 to 13 bits against 1 to 13 bits) and one emulation prevention byte at the
 *    seam. The encoder holds no state that crosses a frame: every decision of a picture reads its own source, its own slice QP and, for the P picture, the I picture of
 *    the same frame.
 * 6. occupancy_rd, the input-mode hints, the flat-chroma fill, verify_md5, preset, log2_ctb, every slice structure (wavefront included) and every job depth behave as in
 *    the constant-QP path. The slice buffers are sized per slice from the slice's own QP.
 * 7. RBT_ERR_PARAM (reason in rbt_last_error; nothing is submitted and the context stays usable): struct_size that is not sizeof(rbt_frame_qp); a list on an occupancy
 *    entry (coded losslessly); n_frames that is not pictures / 2 (n_frames without a list, a list without n_frames); a QP outside 0..51.
 * An entry with n_frames 0 and qp NULL is coded at params[i].qp. The lists are copied at submit. The job is collected by rbt_wait_gof like a job of rbt_submit_gof.
 * Floors that choose the list: "floors held frame by frame" (rbt_submit_gof_quality_frames), further down. */
typedef struct {
  uint32_t struct_size;      /* sizeof(rbt_frame_qp): checked */
  int n_frames;              /* pictures / 2; 0 with qp NULL = no list */
  const int8_t* qp;          /* Q[0 .. n_frames - 1] */
} rbt_frame_qp;
int rbt_submit_gof_frame_qp(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_frame_qp* lists, rbt_job** job);   /* collected by rbt_wait_gof */
int rbt_transcode_gof_frame_qp(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_frame_qp* lists,
                               uint8_t** annexb_out, size_t* n_out);   /* submit + wait */

/* ---- transcoding to a byte budget (csrc/rbt_rate.h) ----
 * rbt_submit_gof codes every entry at the QP the caller names. Here an entry may name a budget instead: the library decodes the input once, counts on the GPU what the
 * decoder left in device memory (the level census), forms a first guess of the QP on the host and closes the loop on the true sizes of trial encodes of the still-resident
 * decoded pictures. Nothing is decoded twice.
 *
 * 1. Level census. Per decoded picture uint32 hist[3][53], one histogram per plane (Y, Cb, Cr). A coefficient level l != 0 of plane c at sample (x, y) has the input QP
 *    qin = QpY of the 4x4 luma unit that covers it (chroma: the unit that covers luma sample (2x, 2y); QpY for all three planes, on both sides - a model), clamped to 0..51.
 *    Units coded with cu_transquant_bypass hold residual samples, not levels, and are left out. With LS = {40, 45, 51, 57, 64, 72}, G = {26214, 23302, 20560, 18396, 16384, 14564}
 *    and m = |l| * LS[qin % 6] * 2^(qin / 6) (|-32768| = 32768), l SURVIVES output QP q when 3 * m * G[q % 6] >= 2^(21 + q / 6): the requantised level is at least 2 / 3.
 *    64-bit integers (46 bits at most); monotone in q. The bin of l is the number of q in 0..51 it survives (0..52; a level of 1 lands in bin qin + 4), and hist[c][b]
 *    counts the levels of plane c with bin b.
 * 2. Estimate. Output picture k of a geometry / attribute stream is an I picture coded at max(0, q - 3) for even k and a P picture coded at q for odd k; q_k is that QP.
 *    nz_k(q') = sum over the planes of the bins b > q'; N0_k = the sum of all bins; B_k = the bytes of the VCL NAL units of input picture k as they stand in the Annex-B
 *    input (start codes and trailing zero bytes excluded, emulation prevention bytes included; a picture starts at first_slice_segment_in_pic_flag).
 *    E(q) = sum over k of floor(B_k * nz_k(q_k) / max(1, N0_k)), in 64 bits: the input calibrates itself through its own bytes per non-zero level, there is no tuned constant.
 * 3. Walk. s(q) = the size of the entry's output from rbt_transcode_gof with qp = q and everything else equal; T = target_bytes, the budget of the WHOLE output stream
 *    (parameter sets, SEIs and start codes included); lo = qp_min, hi = qp_max (0 = 51), 0 <= lo <= hi <= 51.
 *      qe = the lowest q in [lo, hi] with E(q) <= T, or hi if there is none.
 *      s(qe) <= T:  q* starts at qe and goes down while q* > lo and s(q* - 1) <= T; met = 1.
 *      otherwise:   q* starts at qe and goes up while q* < hi and s(q*) > T; met = (s(q*) <= T).
 *    s is NOT monotone in q - the 192x128 geometry maps of the tests give 368, 369, 369 bytes at QP 31, 32, 33 - so "the lowest QP that fits" is not defined by bisection; the
 *    walk is the definition, and it says where it starts. A budget that even hi misses is no error: the stream at hi comes back with met = 0 and RBT_OK. The returned stream is
 *    byte for byte rbt_transcode_gof's at qp = q*. The result depends on s and E alone, not on how the library batches its trial encodes (qe - 1, qe, qe + 1 first, then two at a
 *    time in the walk's direction): n_encodes <= |q* - qe| + 4.
 * target_bytes 0: the entry is coded at params[i].qp exactly as rbt_submit_gof codes it. RBT_ERR_PARAM (reason in rbt_last_error; nothing is submitted and the context stays
 * usable): a target on an occupancy entry; a target on an entry with occupancy_rd (left out on purpose: the census would have to know the occupancy map); struct_size that is
 * not sizeof(rbt_rate_target); a bad range. verify_md5, md5_sei, preset, log2_ctb, the slice structure and any job depth work as in the constant-QP path.
 * Submit enqueues the decoders and, behind each targeted stream's last filter, the census; the wait half reads the histograms back (3 x 53 words a picture), forms qe and runs
 * the trial encodes in rounds on the job's streams, one entry's rounds after the other's, while the decoders of the other jobs in flight keep the GPU busy.
 * rbt_job_memory counts the arenas of the first round (three trial encodes per targeted entry). */
typedef struct {
  uint32_t struct_size;      /* sizeof(rbt_rate_target): checked */
  uint64_t target_bytes;     /* 0 = constant QP (params[i].qp) */
  int qp_min, qp_max;        /* the walk's range; qp_max 0 = 51 */
} rbt_rate_target;
typedef struct {
  int qp, qp_estimate, met, n_encodes;   /* q*, qe, met, trial encodes run for the entry (constant-QP entries: params[i].qp twice, 1, 1) */
  uint64_t bytes, estimate_bytes;        /* s(q*), E(qe) (constant-QP entries: the output size, 0) */
} rbt_rate_result;
int rbt_submit_gof_rate(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_rate_target* targets, rbt_job** job);
int rbt_wait_gof_rate(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_rate_result* results);   /* results: n entries; a job of rbt_submit_gof may be collected here too */
int rbt_transcode_gof_rate(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_rate_target* targets,
                           uint8_t** annexb_out, size_t* n_out, rbt_rate_result* results);   /* submit + wait */
/* The census kernel on host arrays (tests): three planes of int16 levels (w x h, then two of w/2 x h/2; w, h multiples of 8, at most 8192), QpY and the pm byte
 * (bit 2 = cu_transquant_bypass) per 4x4 luma unit, (w / 4) x (h / 4) each -> hist[3][53]. */
int rbt_level_census(rbt_ctx* ctx, const int16_t* y, const int16_t* cb, const int16_t* cr, int w, int h, const int8_t* qp4, const uint8_t* pm4, uint32_t* hist);
/* Decodes a geometry / attribute stream, runs the census and returns what the walk starts from: per picture the histogram (hist: n_pictures x 3 x 53) and B_k
 * (picture_bytes), and E(q) for q = 0..51. The arrays are malloc'd (rbt_free). census_ms: device time between events around the census kernel. */
typedef struct { int n_pictures; uint32_t* hist; uint64_t* picture_bytes; uint64_t estimate[52]; double census_ms; } rbt_rate_table;
int rbt_rate_estimate(rbt_ctx* ctx, const uint8_t* annexb, size_t n, int video_type, rbt_rate_table* out);

/* ---- transcoding to a PSNR floor (csrc/rbt_quality.h) ----
 * "Keep the output within X dB of the input and spend as few bytes as possible." When a re-encode finishes both pictures are in device memory - the decoded input is the
 * encoder's source, and the encoder's reconstruction after its last filter is bit for bit what a decoder makes of the output - so the distortion costs one streaming kernel
 * (k_picture_sse) behind the trial encode's last filter and nine words of read-back per picture.
 *
 * 1. Sums. Per picture and plane c (Y, Cb, Cr), unsigned 64-bit integers: sse[c] = the sum of (A - B)^2 over the plane (w x h for luma, w/2 x h/2 for chroma), A the decoded
 *    input seen through its conformance window, B the reconstruction of the displayed w x h area (the coding padding is excluded); sse_occ[c] the same sum over the occupied
 *    samples and n_occ[c] their number. Occupied, with an occupancy luma plane O of ow x oh samples: s = w / ow must equal h / oh, both divisions whole, s >= 1; luma sample
 *    (x, y) is occupied iff O[y / s][x / s] > 0, chroma sample (x, y) iff luma sample (2x, 2y) is. Without a map sse_occ and n_occ are 0. Integer sums: exact, and
 *    independent of the order of arrival.
 * 2. PSNR. psnr = 10.0 * log10((double)peak * peak * (double)samples / (double)sse) with peak = 2^bit_depth - 1; +inf for sse == 0 with samples > 0, 0 for samples == 0.
 * 3. Occupancy source of an entry: the nearest occupancy entry in front of it that this call pools (the rule of occupancy_rd), if the entry's picture count is a multiple of
 *    the occupancy frame count and there is one whole scale in both directions. Picture k uses occupancy frame k * n_occ / cnt; O is the pooled luma plane, the one the output
 *    occupancy stream carries. When an entry has a source, sse_occ is reported whatever `region` says.
 * 4. meets(q), on plane 0 of the chosen region: true when samples == 0 (nothing to protect); true when sse == 0; otherwise psnr >= min_psnr_mdb / 1000.0, in double as written.
 * 5. Walk. lo = qp_min, hi = qp_max (0 = 51), 0 <= lo <= hi <= 51. q0 = clamp(params[i].qp, lo, hi) is encoded first. qs = q0 when its psnr is +inf, otherwise
 *    qs = clamp(q0 + (int)(psnr(q0) - F), lo, hi) with F = min_psnr_mdb / 1000.0 and a cast that truncates toward zero: one QP step is 2^(1/6) of the quantiser's step size,
 *    about 1 dB - no tuned constant.
 *      meets(qs):  q* starts at qs and goes up while q* < hi and meets(q* + 1); met = 1.
 *      otherwise:  q* starts at qs and goes down while q* > lo and !meets(q*); met = meets(q*).
 *    The distortion is NOT monotone in q - the 64x64 geometry maps of the tests give 41.737, 41.116, 41.186, 39.719 dB at QP 34..37 - so the walk is the definition, and it
 *    says where it starts. A floor that even lo misses is no error: the stream at lo comes back with met = 0 and RBT_OK. The returned stream is byte for byte
 *    rbt_transcode_gof's at qp = q* with the same parameters, occupancy_rd included. Rounds: q0; then qs - 1, qs, qs + 1; then two at a time in the walk's direction; a QP
 *    already tried is never encoded again: n_encodes <= |q* - qs| + 5.
 * min_psnr_mdb 0: the entry is coded at params[i].qp and its distortion is reported (qp = qp_probe = qp_start = params[i].qp, met = 1, n_encodes = 1). Occupancy entries
 * are coded as rbt_submit_gof codes them; their result carries qp, bytes and zeros.
 * RBT_ERR_PARAM (reason in rbt_last_error; nothing is submitted and the context stays usable): struct_size that is not sizeof(rbt_quality_target); a bad range; an unknown
 * region; a negative min_psnr_mdb; a floor on an occupancy entry; RBT_QUALITY_OCCUPIED on an entry without an occupancy source (or with a shape rule 3 refuses);
 * occupancy_rd together with verify_md5, as in rbt_submit_gof.
 * Submit enqueues the decoders and the occupancy pipelines; the geometry / attribute pipelines are encoded in the wait half, in rounds on the job's streams. The pooled
 * occupancy planes and the per-unit maps of occupancy_rd stay alive until the job is collected, and the first trial encode starts only after the occupancy pipeline has made
 * them. A job of rbt_submit_gof_quality is collected by rbt_wait_gof_quality only, and rbt_wait_gof_quality collects no other job: any other pairing is RBT_ERR_PARAM and the
 * job stays collectable. rbt_job_memory counts the arenas of the first round (one trial encode per geometry / attribute entry).
 * Not built: a floor and a byte budget in one call. (A floor per point-cloud frame: rbt_submit_gof_quality_frames below.) (A floor on the point-to-point distortion D1: rbt_submit_gof_d1 below.) */
enum { RBT_QUALITY_ALL = 0, RBT_QUALITY_OCCUPIED = 1 };
typedef struct {
  uint32_t struct_size;    /* sizeof(rbt_quality_target): checked */
  int32_t  min_psnr_mdb;   /* floor on the luma PSNR of the entry's output against its decoded input, 1/1000 dB; 0 = none: coded at params[i].qp, distortion reported */
  int      region;         /* RBT_QUALITY_*: which samples the floor looks at */
  int      qp_min, qp_max; /* the walk's range; qp_max 0 = 51 */
} rbt_quality_target;
typedef struct {
  int qp, qp_probe, qp_start, met, n_encodes;   /* q*, q0, qs, met, distinct QPs encoded */
  uint64_t bytes;                               /* size of the returned stream */
  uint64_t sse[3], samples[3];                  /* of the returned stream, summed over its pictures; Y, Cb, Cr */
  uint64_t sse_occ[3], samples_occ[3];          /* occupied samples; zeros when the entry has no occupancy source */
  double psnr[3], psnr_occ[3];
} rbt_quality_result;
int rbt_submit_gof_quality(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_quality_target* targets, rbt_job** job);
int rbt_wait_gof_quality(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_quality_result* results);   /* results: n entries */
int rbt_transcode_gof_quality(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_quality_target* targets,
                              uint8_t** annexb_out, size_t* n_out, rbt_quality_result* results);   /* submit + wait */
/* The kernel on host arrays (tests): a and b are n_frames planar 4:2:0 pictures each (width x height luma, then two planes of width/2 x height/2, back to back); occ is NULL
 * or n_frames planes of ow x oh samples, one per picture. out: n_frames x 3 x {sse, sse_occ, n_occ}. RBT_ERR_PARAM: odd sizes, sizes above 8192, a map whose scale is
 * not whole and equal in both directions. rbt_get_stats afterwards: gpu_ms = the device time between events around the kernel's launches, everything else 0. */
int rbt_picture_sse(rbt_ctx* ctx, const uint16_t* a, const uint16_t* b, int width, int height, int n_frames, const uint16_t* occ, int ow, int oh, uint64_t* out);

/* ---- transcoding geometry to a D1 floor (csrc/rbt_cloudmaps.h, host/rbt_d1_walk.h) ----
 * "The cheapest geometry stream that keeps the point-to-point distortion D1 within X dB." The luma PSNR of a geometry map is a proxy for D1: the occupancy map of the
 * output decides which samples become points at all, and pooling it from precision 2 to 4 adds and removes points whatever the geometry QP. Here the cloud of every trial
 * encode is rebuilt and scored on the GPU: when a round of trial encodes ends, the decoded input and the encoder's reconstructions are in device memory; a gather kernel
 * (k_gather_luma) makes the packed luma planes of them, the reconstruction kernels of rbt_reconstruct emit the positions, the cloud is indexed as rbt_pcloud_upload indexes
 * one and scored as rbt_score scores it. Only counts and the D1 sums come back to the host. The types of the atlas, patches, clouds and D1 results are declared further
 * down in this header.
 *
 * 1. Occupancy source of a geometry entry: the nearest occupancy entry in front of it in the call that this call pools (occupancy_precision 4; the rule of occupancy_rd and
 *    of the PSNR floor). Its output luma is the pooled plane. Without such an entry: RBT_ERR_PARAM. (Not built: an occupancy entry that is passed through, whose decoded
 *    input plane would be the output's - the library does not decode a stream it hands back unchanged.)
 * 2. Shapes. The entry's displayed picture size equals atlas.width x atlas.height; its picture count is atlas.map_count x n_frames; the occupancy entry has n_frames
 *    pictures; atlas.occupancy_precision equals width / (output occupancy width), and the input occupancy width divides width by a whole number, the same in both
 *    directions. Anything else is RBT_ERR_PARAM with the reason in rbt_last_error.
 * 3. Cloud of a trial. B_f(q) is the positions rbt_reconstruct returns for the atlas and the patches of frame f, the output occupancy luma of frame f and the luma of output
 *    pictures map_count * f (and + 1) of the stream rbt_transcode_gof gives at qp = q. No attribute pictures. Geometry smoothing runs as atlas.geometry_smoothing says.
 * 4. Reference. A_f is the handle given for frame f. Where it is NULL, A_f is the same reconstruction on the decoded input: input occupancy luma, input geometry luma, the
 *    same atlas with occupancy_precision = width / input occupancy width.
 * 5. Score. D_f(q) = rbt_d1(A_f, B_f(q), peak): the integer fields from the search rbt_score runs, the float fields from the routine both public calls use. D(q) is the
 *    minimum over f of (double)psnr (RBT_D1_MIN), or the sum in frame order in double divided by n_frames (RBT_D1_MEAN). meets(q): D(q) >= min_d1_mdb / 1000.0; +inf meets
 *    any floor.
 * 6. Walk. The PSNR floor's walk (rule 5 there), word for word, with D in place of the PSNR: probe at q0 = clamp(params[i].qp, lo, hi); qs = q0 when D(q0) is infinite,
 *    otherwise clamp(q0 + (int)(D(q0) - F), lo, hi); toward larger QPs while meets holds, else down; met and q* as there; n_encodes <= |q* - qs| + 5. The 1 dB-per-step
 *    model behind qs is poor for D1 - about 0.2 dB per step on the synthetic atlases of the tests, and D is far from monotone (58.5, 59.3, 58.2, 59.1 dB at QP 24..27) -
 *    which costs encodes, not correctness: the walk is the definition. The rule is kept so that the probe is the PSNR floor's.
 * 7. Stream. The returned stream is byte for byte rbt_transcode_gof's at qp = q*, occupancy_rd included. A floor that even lo misses is no error (met = 0, RBT_OK).
 * min_d1_mdb 0: the entry is coded at params[i].qp and its D1 is reported (qp = qp_probe = qp_start = params[i].qp, met = 1, n_encodes = 1).
 * Other entries - attribute, occupancy, geometry without a target - are coded as rbt_submit_gof codes them; their target is empty (every field but struct_size zero) and
 * their result carries qp, bytes and zeros.
 * RBT_ERR_PARAM (reason in rbt_last_error; nothing is submitted and the context stays usable): a wrong struct_size; a target on a non-geometry entry; a bad range; an unknown
 * stat; a negative floor; n_frames < 1; a missing patch list; a reference handle of another context; rules 1 and 2; an atlas or a patch rbt_reconstruct refuses;
 * occupancy_rd together with verify_md5. An empty cloud or a coordinate outside 0..1023 is found when the cloud is built: the job fails in its wait call as the PCC stage
 * reports it (RBT_ERR_PARAM, "empty point cloud" / "coordinate outside 0..1023") and the context stays usable.
 * The patch lists are copied at submit; a reference handle must stay alive until the job is collected. A job of rbt_submit_gof_d1 is collected by rbt_wait_gof_d1 only, and
 * rbt_wait_gof_d1 collects no other job: any other pairing is RBT_ERR_PARAM and the job stays collectable.
 * Memory: the clouds of a round are scored one after the other. A job holds one 128 MB volume per frame without a reference handle (for the whole job), one more for the
 * trial being scored, and three packed planes per frame; rbt_job_memory counts them with the arenas of the first round.
 * Not built: a container-level call (the library does not parse the atlas sub-bitstream, so rbt_transcode_v3c cannot know the patches), a D1 floor (a D2 floor: "D2 floors" at the end of this header; a colour floor: rbt_submit_gof_color below)
 * together with a byte budget or a PSNR floor, a floor per frame other than through RBT_D1_MIN. */
enum { RBT_D1_MIN = 0, RBT_D1_MEAN = 1 };
typedef struct rbt_d1_target rbt_d1_target;                  /* both defined behind rbt_score_summary, where the types of their fields are known */
typedef struct rbt_d1_floor_result rbt_d1_floor_result;
int rbt_submit_gof_d1(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_d1_target* targets, rbt_job** job);
int rbt_wait_gof_d1(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_d1_floor_result* results);   /* results: n entries */
int rbt_transcode_gof_d1(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_d1_target* targets,
                         uint8_t** annexb_out, size_t* n_out, rbt_d1_floor_result* results);   /* submit + wait */
/* ---- transcoding attributes to a colour PSNR floor (csrc/rbt_score.h, csrc/rbt_cloudmaps.h, host/rbt_color_walk.h) ----
 * "The cheapest attribute stream that keeps the colour PSNR of the decoded cloud within X dB." The luma PSNR of an attribute map is a proxy for what the common test
 * conditions report: the output occupancy map and the output geometry decide which samples become points and where, the cloud's colour is taken after the 4:2:0 -> 4:4:4
 * up-conversion and after the attribute transfer that follows geometry smoothing, and the metric merges duplicates and averages tie sets. Here the cloud of every trial
 * encode is scored on the GPU. Its geometry does not change with the attribute QP, so it is made once per job and frame, behind the geometry pipeline's only encode
 * (positions before and after smoothing, the moved flags, the index of the final cloud, and against the reference a score pair: rbt_score_pair_create below); per trial
 * the three planes of every attribute picture are gathered (k_gather_luma, three descriptors a picture), up-converted, fetched per point, transferred, converted to RGB,
 * and the cloud is recoloured (rbt_pcloud_set_colors' kernels) and scored by the colour walks alone. Only the colour sums come back to the host.
 *
 * 1. Sources. A target sits on an attribute entry only. Its occupancy source is the D1 rule's: the nearest pooled occupancy entry in front of it. Its geometry source is
 *    the nearest geometry entry in front of it that has the same occupancy source; that entry is coded at its own params[i].qp, exactly as rbt_submit_gof codes it,
 *    occupancy_rd included. A missing source is RBT_ERR_PARAM.
 * 2. Shapes. The displayed size of the geometry and of the attribute entry equals atlas.width x atlas.height, both hold atlas.map_count x n_frames pictures, the
 *    attribute bit depth is 8 or 10; the occupancy rules are those of D1 rule 2.
 * 3. Cloud of a trial. B_f(q) is what rbt_pcloud_from_maps makes of the atlas and the patches of frame f, the output occupancy luma of frame f, the luma of the geometry
 *    entry's output pictures map_count * f (and + 1), the attribute entry's output pictures map_count * f (and + 1) at qp = q, upsample_filter and attr_transfer.
 * 4. Reference. A_f is the handle given for frame f; it must carry colours and belong to the same context. Where it is NULL, A_f is the same route on the decoded input
 *    occupancy, geometry and attribute, with the atlas at the input occupancy's precision.
 * 5. Score. C_f(q) is the .color part of rbt_score(A_f, B_f(q), peak, RBT_SCORE_COLOR): the integer sums from the colour walks, the float fields from the routine both
 *    public calls use. D(q) is the minimum over f of (double)psnr[channel] (RBT_D1_MIN), or the sum in frame order in double divided by n_frames (RBT_D1_MEAN).
 *    meets(q): D(q) >= min_psnr_mdb / 1000.0; +inf meets any floor.
 * 6. Walk and stream. The PSNR floor's walk, word for word, with D in place of the PSNR (D1 rule 6; n_encodes <= |q* - qs| + 5). The returned stream is byte for byte
 *    rbt_transcode_gof's at qp = q*. min_psnr_mdb 0: the entry is coded at params[i].qp and its colour results are reported (met = 1, n_encodes = 1). A floor that even
 *    qp_min misses is no error (met = 0, RBT_OK).
 * 7. Errors are the D1 section's, applied to this shape: RBT_ERR_PARAM (reason in rbt_last_error; nothing is submitted, the context stays usable) for a wrong struct_size,
 *    a target on a non-attribute entry, a bad range, an unknown stat, channel or up-sampling filter, a negative floor, n_frames < 1, a missing patch list, a reference
 *    handle of another context or without colours, rules 1 and 2, an atlas or patch rbt_reconstruct refuses. An empty cloud, a coordinate outside 0..1023 or more than 2^21
 *    merged points in a cloud fail the job in its wait call (RBT_ERR_PARAM) and the context stays usable. A job of rbt_submit_gof_color is collected by rbt_wait_gof_color
 *    only, and rbt_wait_gof_color collects no other job: any other pairing is RBT_ERR_PARAM and the job stays collectable.
 * The patch lists are copied at submit; a reference handle must stay alive, and keep its colours (no rbt_pcloud_set_colors on it), until the job is collected. Entries
 * without a target carry an empty target (every field but
 * struct_size zero) and their result carries qp, bytes and zeros.
 * Memory: a job holds, per frame, one 128 MB volume and one set of maps for B_f, the same for a reference of its own, 8 bytes per point of distances and the packed
 * geometry planes; per trial the packed attribute planes, their 4:4:4 planes and the two volumes of the attribute transfer. rbt_job_memory counts them with the arenas of
 * the first round. The volumes go back to the context's cache when the rounds end.
 * Not built: a container-level call (the library does not parse the atlas sub-bitstream), a colour floor together with a D1 floor, a byte budget or a PSNR floor in one
 * job, a floor per frame other than through RBT_D1_MIN, batched scoring across frames, transfer neighbour sets kept across trials, colour smoothing. */
typedef struct rbt_color_target rbt_color_target;             /* both defined behind rbt_d1_floor_result */
typedef struct rbt_color_floor_result rbt_color_floor_result;
int rbt_submit_gof_color(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_color_target* targets, rbt_job** job);
int rbt_wait_gof_color(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_color_floor_result* results);   /* results: n entries */
int rbt_transcode_gof_color(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_color_target* targets,
                            uint8_t** annexb_out, size_t* n_out, rbt_color_floor_result* results);   /* submit + wait */
/* The gather kernel on host arrays (tests): src holds n_pics planes of `stride` x `rows` samples; the w x h window at (x0, y0) of each comes back packed in out
 * (n_pics x w x h). The planes go to the device with their first sample src_misalign (0..7) samples behind a 256-byte boundary, the packed planes start on one. */
int rbt_gather_luma(rbt_ctx* ctx, const uint16_t* src, int n_pics, int stride, int rows, int x0, int y0, int w, int h, int src_misalign, uint16_t* out);
/* The same kernel on all three planes of coded 4:2:0 pictures (tests): a picture of src is its luma plane (`stride` x `rows` samples) followed by Cb and Cr (`chroma_stride`
 * x `chroma_rows` each). The even w x h window at the even offset (x0, y0), and the w/2 x h/2 windows at (x0/2, y0/2) of the chroma planes, come back as packed planar
 * 4:2:0 pictures - w*h luma samples, then w*h/4 of Cb, then of Cr - which is the layout rbt_yuv420_to_yuv444 reads. One descriptor per plane: a chroma row of 1, 7 or 36
 * samples is cut into chunks as a luma row is. Misalignment as for rbt_gather_luma. RBT_ERR_PARAM: an odd window or offset, a window outside a plane. */
int rbt_gather_420(rbt_ctx* ctx, const uint16_t* src, int n_pics, int stride, int rows, int chroma_stride, int chroma_rows, int x0, int y0, int w, int h, int src_misalign,
                   uint16_t* out);

/* The two halves exposed on their own (SURVEY.md 8(b) alternative seam; used by the parity tests).
 * Picture sizes: any even width / height. Sizes that are not multiples of 8 (all-intra) / 16 (gop 2) are coded padded with a
 * conformance window in the SPS (as libx265 does for the reference); rbt_decode returns the cropped pictures. */
int rbt_decode(rbt_ctx* ctx, const uint8_t* annexb, size_t n, int verify_md5, rbt_video* out);
int rbt_encode(rbt_ctx* ctx, const uint16_t* yuv, int width, int height, int bit_depth, int n_frames, int qp, int gop, int lossless,
               int log2_ctb, int ctb_rows_per_slice, int md5_sei, uint8_t** annexb_out, size_t* n_out);   /* md5_sei: RBT_HASH_* */

/* resize_frame2 (PCCTranscoder.cpp:594-646) on a host plane (tests): out[v][u] = any(in block > 0) */
int rbt_or_pool(rbt_ctx* ctx, const uint16_t* plane, int width, int height, int factor, uint16_t* out);
/* Decoded picture hash (RBT_HASH_MD5 / _CRC / _CHECKSUM) of n_frames host pictures (planar 4:2:0, width x height luma, even sizes, bit depth 8..16), computed by the
 * device kernels the transcoder uses: out gets 48 bytes per picture, 16 per component in SEI byte order (MD5 digest; CRC 2 bytes, checksum 4 bytes, most significant
 * first), zero-padded. */
int rbt_picture_hash(rbt_ctx* ctx, const uint16_t* yuv, int width, int height, int bit_depth, int n_frames, int kind, uint8_t* out);

/* PCCVideoBitstream::sampleStreamToByteStream / byteStreamToSampleStream (PCCVideoBitstream.cpp:85-172), host side */
int rbt_sample_to_byte_stream(const uint8_t* in, size_t n, uint8_t** out, size_t* n_out);
int rbt_byte_to_sample_stream(const uint8_t* in, size_t n, uint8_t** out, size_t* n_out);

int rbt_get_stats(rbt_ctx* ctx, rbt_stats* out);
/* Decoded pictures of the context's last collected job (rbt_wait_gof*, the blocking transcode calls) or rbt_decode that were reconstructed with flat chroma: no coded
 * chroma block, no chroma SAO, default weighting, flat references - both chroma planes are then 1 << (bit_depth - 1) by H.265's text and are filled, not computed
 * (DESIGN.md 14). A failed call leaves the count of the call before it. */
int rbt_flat_pictures(const rbt_ctx* ctx);
/* Device self-test of the 32-point transform stages on the matrix cores (v_mfma_i32_32x32x32_i8) against the vector-ALU form of the same stages:
 * n_blocks blocks of 32 x 32 int16 (coefficients for the inverse, residuals for the forward transform); *n_mismatch = differing output samples. */
int rbt_selftest_transform32(rbt_ctx* ctx, const int16_t* blocks, int n_blocks, int bit_depth, uint32_t* n_mismatch);
/* Test hook: single transform blocks through the decoder's own reconstruction routine (csrc/rbt_recon.h rc_tile_tb / rc_tile_tb_cpair), one wave per case, so that the
 * block's arithmetic can be held against H.265 8.4.4.2 / 8.6 directly (tests/tb_spec.py). A case is staged into a CTB tile the way the CTB kernel stages a CTB: the 4N+1
 * neighbour samples around the block at (x0, y0) inside the CTB (samples of the block's component), the availability of the neighbours' 4x4 luma units, the levels where
 * the block's samples will be; what the routine leaves at the block's position comes back (samples; for an inter block the residual as int16 bit patterns).
 * kind: RBT_TB_LUMA / _CB / _CR = one block of that component through rc_tile_tb, RBT_TB_PAIR = Cb and Cr of one transform unit through rc_tile_tb_cpair (cbf / qp [0] = Cb,
 * [1] = Cr; no transform skip). log2: 2..5 (chroma 2..4); bit_depth 8..12; log2_ctb 4..6; x0, y0 multiples of 4 with the block inside the CTB; qp as the kernels take it
 * (including 6 * (bit_depth - 8)), 0 .. 51 + 6 * (bit_depth - 8).
 * nb: [n][2][RBT_TB_NB] samples in reference order (0 = p[-1][2N-1] .. 2N-1 = p[-1][0], 2N = corner, 2N+1+x = p[x][-1]); unit_av: [n][RBT_TB_UNITS] flags of the units of
 * 4 (chroma: 2) samples in the same order (2N / unit up the left column, the corner, 2N / unit along the row above) - a unit below the CTB, or right of it in a row of
 * the CTB itself, is never available and its flag is ignored; levels, out: [n][2][1024], row pitch N; plane slot 1 is used by RBT_TB_PAIR only. */
enum { RBT_TB_LUMA = 0, RBT_TB_CB = 1, RBT_TB_CR = 2, RBT_TB_PAIR = 3, RBT_TB_NB = 129, RBT_TB_UNITS = 33 };
typedef struct rbt_tb_case {
  int32_t kind, log2, bit_depth, log2_ctb, x0, y0, strong_intra_smoothing, intra, mode, cbf[2], transform_skip, cu_transquant_bypass, qp[2], pad;
} rbt_tb_case;
int rbt_selftest_tb(rbt_ctx* ctx, const rbt_tb_case* cases, int n_cases, const uint16_t* nb, const uint8_t* unit_av, const int16_t* levels, uint16_t* out);

/* ---- decoder-side verification stage: what turns transcoded maps into the D1 figure of the metric ----
 * Replaces PCCCodec::generateOccupancyMap (PCCCodec.cpp:1584-1606), generateBlockToPatchFromOccupancyMapVideo (:1725-1763),
 * generatePointCloud / generatePoints (:517-978, :327-515) and the colour fetch of colorPointCloud (:1308-1449) for the configuration of the
 * CTC streams (two geometry maps with absolute D1; no EOM, raw patches, point-local reconstruction or patch border filtering; one tile),
 * and the point-to-point part of QualityMetrics::compute (PCCMetrics.cpp:75-231, :44-48, :299-309). */
typedef struct {             /* the fields of PCCPatch the reconstruction reads (PCCPatch.h) */
  int32_t u0, v0, size_u0, size_v0;      /* position / size in the atlas in occupancy-resolution blocks */
  int32_t u1, v1, d1;                    /* 3-D offset along the tangent, bitangent and normal axis */
  int32_t normal_axis, tangent_axis, bitangent_axis;   /* 0..2, all different */
  int32_t projection_mode;               /* 0: depth + d1, 1: d1 - depth */
  int32_t orientation;                   /* PATCH_ORIENTATION_* (PCCCommon.h:128-137) */
  int32_t lod_x, lod_y;
} rbt_patch;
typedef struct {
  int32_t width, height;                 /* atlas frame size (multiples of occupancy_resolution) */
  int32_t occupancy_resolution;          /* 16 in the CTC (cfg/common/ctc-common.cfg) */
  int32_t occupancy_precision;           /* atlas size / occupancy video size: 2 at R5, 4 after the transcoder's OR-pool */
  int32_t map_count, absolute_d1, remove_duplicate_points, threshold_lossy_om;
  /* Geometry smoothing of the decoder's post-processing, which the CTC switches on (cfg/common/ctc-common.cfg:57-60: flagGeometrySmoothing 1, gridSmoothing 1, gridSize 8,
   * thresholdSmoothing 64; PCCDecoder.cpp:434-437 -> PCCCodec::smoothPointCloudPostprocess, PCCCodec.cpp:52-145, :980-1104): boundary points (identifyBoundaryPoints, :266-325)
   * next to cells that hold points of more than one patch move towards the tri-linear blend of the 8 surrounding cell centroids. geometry_smoothing 0 = off (the cloud as
   * generatePointCloud leaves it); grid_size 2..255, even (the reference's cfg uses 8). Exact for cells of fewer than 16384 points (the reference sums centroids in float). */
  int32_t geometry_smoothing, grid_size, threshold_smoothing;
} rbt_atlas_params;
typedef struct {             /* host memory, released with rbt_cloud_free */
  int n_points;
  int16_t* xyz;              /* 3 per point, in the order PCCCodec::generatePointCloud emits them */
  uint16_t* yuv;             /* 3 per point: the attribute samples at the point's pixel (chroma at the co-sited 4:2:0 sample; the reference
                                converts to 4:4:4 first, PccLibColorConverter: rbt_reconstruct_rgb does, and returns the 16-bit 4:4:4 triples here) */
  uint8_t* occupancy_map;    /* width x height: the up-scaled, binarised occupancy map */
  uint32_t* block_to_patch;  /* (width / res) x (height / res): patch index + 1 */
  int n_smoothed;            /* points the geometry smoothing moved */
} rbt_cloud;
/* occ_luma: occupancy video luma, (width / precision) x (height / precision); geo_d0 / geo_d1: luma of the near / far geometry map, width x
 * height samples of geo_bit_depth bits (mapped to 8 bits like PCCImage::set, PCCImage.h:107-124); attr_t0 / attr_t1: planar 4:2:0 attribute
 * pictures or NULL. */
int rbt_reconstruct(rbt_ctx* ctx, const rbt_atlas_params* atlas, const rbt_patch* patches, int n_patches, const uint16_t* occ_luma, const uint16_t* geo_d0,
                    const uint16_t* geo_d1, int geo_bit_depth, const uint16_t* attr_t0, const uint16_t* attr_t1, int attr_bit_depth, rbt_cloud* out);
void rbt_cloud_free(rbt_cloud* c);
typedef struct {
  int n_a, n_b;                          /* points after merging duplicates (PCCMetricsParameters.cpp:50) */
  uint64_t sse_ab, sse_ba, max_ab, max_ba;   /* sum / maximum of squared nearest-neighbour distances, A -> B and B -> A (exact integers) */
  float mse_ab, mse_ba, psnr_ab, psnr_ba, psnr;   /* psnr = 10 log10(3 peak^2 / max(mse_ab, mse_ba)) (PCCMetrics.cpp:44-48, :299-309) */
} rbt_d1_result;
/* point-to-point (D1) metric between two clouds; coordinates 0..1023 (peak = 1023 in the CTC).
 * rbt_d1, rbt_d2 and rbt_color_metric are each the upload, one score and the release of two temporary clouds ("frame scoring on clouds that stay on the device" below:
 * the same index, search and walks, so out is that part of rbt_score's result, field for field and bit for bit, and two calls return the same bits). RBT_ERR_PARAM with
 * the reason in rbt_last_error: an empty cloud (for D1 and D2 also peak <= 0) and, checked on the device, cloud A before cloud B, a coordinate outside 0..1023 or more
 * than 2^26 points in a cloud. Device memory while a call runs, all of it back in the pool when it returns (the context's cloud cache, rbt_device_memory's cached
 * figure and rbt_trim see nothing of it): per cloud a 128 MB bit volume with its 256 KB coarse level, the points, and 28 bytes per slot of the voxel map, whose slot
 * count is the power of two that is at least 2 n (16 at the least); the score's scratch of 4 bytes per point (for D2 also 8 per point, 28 per point of B and 16 per 256 points of the larger cloud). For
 * rbt_d1 that is more than the byte per point it took next to the volumes before it shared the index. */
int rbt_d1(rbt_ctx* ctx, const int16_t* xyz_a, int n_a, const int16_t* xyz_b, int n_b, int peak, rbt_d1_result* out);
/* point-to-plane (D2) metric, the other half of BASELINE's "D1/D2 geom PSNR": QualityMetrics::compute with computeC2p_ (PCCMetrics.cpp:100-124, :213-215), symmetric (:299-309),
 * between a source cloud A that comes with normals (three per point, fixed point Q14: 16384 = 1.0) and a decoded cloud B that gets its normals from A the way
 * PCCMetrics::compute arranges it (:371-376: copyNormals on the source, scaleNormals on the reconstruction, PCCPointSet.cpp:2322-2380: every source point gives its normal to
 * the points of B nearest to it, a point of B that got none takes the mean of the source points nearest to it). Per point of one cloud: the mean, over the other cloud's points
 * at the nearest distance, of the squared projection of the difference on that point's normal. Where the reference depends on the order its kd-tree returns equidistant points
 * in, this is defined instead: duplicates are merged first and a merged point keeps the normal of its lowest-index duplicate; ALL points at exactly the nearest squared
 * distance count (the reference looks at up to 30 results). The two sums are added in the fixed order given at rbt_score. Upload + score + release, refusals and
 * memory as at rbt_d1; normals_a is required. */
typedef struct {
  int n_a, n_b;
  double sse_ab, sse_ba, max_ab, max_ba;              /* sum / maximum of the per-point values, A -> B and B -> A */
  float mse_ab, mse_ba, psnr_ab, psnr_ba, psnr;       /* psnr = 10 log10(3 peak^2 / max(mse_ab, mse_ba)) */
} rbt_d2_result;
int rbt_d2(rbt_ctx* ctx, const int16_t* xyz_a, const int16_t* normals_a, int n_a, const int16_t* xyz_b, int n_b, int peak, rbt_d2_result* out);

/* ---- V3C sample stream: the container either side of the path ----
 * What PccAppTranscoder's decompressVideo does around transcodeData (PccAppTranscoder.cpp:277-349): read the sample stream (PCCBitstreamReader::read,
 * PCCBitstreamReader.cpp:51-70, C.2: one header byte with the unit size precision, then size + unit), walk it GOF by GOF (a GOF starts at each
 * V3C_VPS unit, :72-96), transcode the video units of every GOF, collect the units of all GOFs (PCCBitstreamWriter::encode, PCCBitstreamWriter.cpp:96-237) and
 * write them as ONE sample stream whose unit size precision follows the largest unit (PCCBitstreamWriter::write, :57-91).
 * The library does not parse the V3C parameter set or the atlas sub-bitstream: the reference reads both into its context and writes them back
 * (with the end-of-tile patch type its reader dropped put back, PCCTranscoder::addEndTile :906-914), which for a stream its own writer made reproduces
 * the bytes; here V3C_VPS and V3C_AD units are copied. The payload of an OVD / GVD / AVD unit is the video sub-bitstream in sample stream form
 * (PCCBitstream::readVideoStream, PCCBitstream.cpp:88-97; unit size - 4, PCCBitstreamReader.cpp:225). */
enum { RBT_V3C_VPS = 0, RBT_V3C_AD = 1, RBT_V3C_OVD = 2, RBT_V3C_GVD = 3, RBT_V3C_AVD = 4 };   /* V3CUnitType, PCCBitstreamCommon.h:133-137 */
typedef struct {
  int type;                  /* vuh_unit_type (first 5 bits of the unit, PCCBitstreamReader.cpp:1381-1383) */
  int gof;                   /* GOF the unit belongs to (units in front of the first V3C_VPS: 0) */
  int parameter_set_id, atlas_id;                     /* v3cUnitHeader, PCCBitstreamReader.cpp:182-211; 0 where the unit type has none */
  int attribute_index, attribute_dimension_index, map_index, auxiliary_video;
  int video_type;            /* RBT_VIDEO_* the unit's sub-bitstream is filed under where transcodeData looks for it (videoSubStream, :98-158): OVD -> occupancy,
                                GVD without auxiliary video -> geometry, AVD without auxiliary video, partition 0 -> attribute; -1 for every other unit */
  size_t offset, size;       /* the unit (4-byte header + payload) inside the input */
} rbt_v3c_unit;
/* Lists the units of a sample stream (host only, no GPU needed; *units is malloc'd, rbt_free). RBT_ERR_BITSTREAM if a unit overruns the input. */
int rbt_v3c_index(const uint8_t* in, size_t n, rbt_v3c_unit** units, int* n_units);
/* PCCBitstreamWriter::write (:57-91) + sampleStreamV3CHeader / sampleStreamV3CUnit (:1492-1507): precision = min(max(ceil(ceilLog2(largest unit) / 8), 1), 8)
 * bytes, at least forced_precision_bytes (forcedSsvhUnitSizePrecisionBytes_); then every unit behind its size. Host only. */
int rbt_v3c_write(const uint8_t* const* unit, const size_t* unit_size, int n_units, int forced_precision_bytes, uint8_t** out, size_t* n_out);
/* PCCBitstreamStat as decompressVideo prints it for the input and the output file (PccAppTranscoder.cpp:351-352, PCCBitstream.h:48-154), from the bytes alone. Host only. */
typedef struct {
  int n_units, n_gofs, unit_size_precision_bytes;
  uint64_t header;                                    /* sample stream header + the size fields of all units (PCCBitstreamReader.cpp:51-70) */
  uint64_t unit_size[5];                              /* V3CUnitSize[type]: unit headers + payloads */
  uint64_t occupancy_video, geometry_video, geometry_aux_video, attribute_video, attribute_aux_video;   /* videoBinSize: payloads of the video units */
  uint64_t total_metadata, total_geometry, total_attribute, total;   /* getTotalMetadata() + header, getTotalGeometry(), getTotalAttribute(), their sum (:138-148) */
} rbt_v3c_stat;
int rbt_v3c_stats(const uint8_t* in, size_t n, rbt_v3c_stat* out);
typedef struct {
  int occupancy_precision;   /* occupancyPrecision_: the occupancy video is transcoded (2x2 OR-pool, lossless) only when 4 (PCCTranscoder.cpp:150) */
  int geometry_qp, attribute_qp;                      /* geometryQP_, attributeQP_ */
  int forced_unit_size_precision_bytes;               /* forcedSsvhUnitSizePrecisionBytes_, 0 = none */
  int log2_ctb, ctb_rows_per_slice, md5_sei, verify_md5;   /* as in rbt_stream_params; md5_sei: RBT_HASH_* */
  int gofs_per_job;          /* GOFs handed to the GPU per job; 0 = by rbt_job_shape from the number of GOFs this context owns, which also lowers the announced depth for
                              * the duration of the call when the walk is short (the depth announced with rbt_set_depth is the cap and is restored) */
  int occupancy_rd;          /* occupancy-aware coding of the geometry / attribute units of every GOF (rbt_stream_params.occupancy_rd): with the occupancy map that GOF's
                              * occupancy unit comes out with, when occupancy_precision is 4 */
  int preset;                /* RBT_PRESET_* for the geometry / attribute units (rbt_stream_params.preset) */
} rbt_v3c_params;
/* The whole walk: index, per GOF the video units through rbt_submit_gof / rbt_wait_gof with as many jobs in flight as rbt_set_depth announced (fewer for a short walk
 * with gofs_per_job = 0), write.
 * Video units transcodeData does not look at (auxiliary video, attribute partitions beyond the first) are copied; a GOF with several
 * geometry or attribute map streams (multipleMapStreamsPresentFlag) is refused (RBT_ERR_UNSUPPORTED) - the reference looks for VIDEO_GEOMETRY / VIDEO_ATTRIBUTE, which such a GOF does not have.
 * In a multi-GPU job (rbt_create with world_size > 1) the output holds the GOFs this rank owns (rbt_owns_gof) and nothing else: rank 0 of the host
 * program gathers the partial streams and merges them with rbt_v3c_index + rbt_v3c_write (gof_shard.transcode_v3c does). */
int rbt_transcode_v3c(rbt_ctx* ctx, const uint8_t* in, size_t n, const rbt_v3c_params* p, uint8_t** out, size_t* n_out);
/* The same walk with the output handed over GOF by GOF, in GOF order, as soon as the job that holds a GOF has been collected (the jobs behind it are still running): the
 * sink gets the units of one GOF this context owns - carried-over units point into `in`, transcoded ones into memory that is released when the sink returns. A sink that
 * writes a sample stream itself chooses the unit size precision up front (PCCBitstreamWriter::write derives it from the largest unit of the whole file, which a streaming
 * writer does not know yet: forcedSsvhUnitSizePrecisionBytes_ = 4 is what fits every file). A non-zero return of the sink ends the walk (RBT_ERR_PARAM; jobs in flight are drained). */
typedef int (*rbt_v3c_sink)(void* user, int gof, int n_units, const uint8_t* const* unit, const size_t* unit_size);
int rbt_transcode_v3c_stream(rbt_ctx* ctx, const uint8_t* in, size_t n, const rbt_v3c_params* p, rbt_v3c_sink sink, void* user);

/* rbt_transcode_v3c's walk with byte budgets (rbt_submit_gof_rate / rbt_wait_gof_rate, above): the budget of a GOF's geometry / attribute unit is
 * ceil(bits_per_picture x pictures in that unit / 8) bytes of Annex-B, walked over the QPs 0..51; a value of 0 means constant QP (geometry_qp / attribute_qp) for that type, and
 * with both 0 the output is rbt_transcode_v3c's. rbt_v3c_params has no size field and is not changed. *per_gof (may be NULL; malloc'd, rbt_free): two results per GOF of the input
 * (rbt_v3c_stat.n_gofs), geometry then attribute, zeros for a GOF this context does not own or a unit it does not have. Multi-GPU ownership and the memory-bounded depth are the
 * walk's. Any rate target together with occupancy_rd: RBT_ERR_PARAM. */
int rbt_transcode_v3c_rate(rbt_ctx* ctx, const uint8_t* in, size_t n, const rbt_v3c_params* p, uint32_t geometry_bits_per_picture, uint32_t attribute_bits_per_picture,
                           uint8_t** out, size_t* n_out, rbt_rate_result** per_gof);

/* rbt_transcode_v3c's walk with PSNR floors per unit type (rbt_submit_gof_quality / rbt_wait_gof_quality, above), walked over the QPs 0..51 from geometry_qp / attribute_qp;
 * 0 for a type means constant QP, and with both 0 the output is rbt_transcode_v3c's. region: RBT_QUALITY_*. p->occupancy_rd is allowed. *per_gof as in
 * rbt_transcode_v3c_rate: two results per GOF of the input, geometry then attribute. Multi-GPU ownership and the memory-bounded depth are the walk's. */
int rbt_transcode_v3c_quality(rbt_ctx* ctx, const uint8_t* in, size_t n, const rbt_v3c_params* p, int32_t geometry_min_psnr_mdb, int32_t attribute_min_psnr_mdb, int region,
                              uint8_t** out, size_t* n_out, rbt_quality_result** per_gof);

/* ---- colour half of the metric: 4:4:4 up-conversion, RGB, colour PSNR (csrc/rbt_color.h) ----
 * Planar 4:2:0 pictures (samples of bit_depth 8 or 10 in uint16_t) -> n_frames x 3 planes of width x height 16-bit samples, as the decoder converts an attribute video
 * under the CTC settings: PCCInternalColorConverter::convertYUV420ToYUV444 with g_filter420to444[0] (float round trip, four-tap up-sampling, bit for bit), or the
 * sample replication of PCCImage::convertYUV420ToYUV444 (values unchanged). width and height even. */
enum { RBT_UPSAMPLE_REPLICATE = -1, RBT_UPSAMPLE_F0 = 0 };
int rbt_yuv420_to_yuv444(rbt_ctx* ctx, const uint16_t* yuv420, int width, int height, int bit_depth, int n_frames, int filter, uint16_t* yuv444);
/* PCCPointSet3::convertYUV16ToRGB8 (PCCPointSet.h:133-166): n triples of 16-bit 4:4:4 samples -> n RGB triples */
int rbt_yuv16_to_rgb8(rbt_ctx* ctx, const uint16_t* yuv16, int n, uint8_t* rgb);
/* rbt_reconstruct with the colours as the decoder leaves them: the two attribute pictures are up-converted (upsample_filter: RBT_UPSAMPLE_*), every point takes the three
 * 4:4:4 samples at its pixel (out->yuv, what colorPointCloud does on the converted video) and these are converted to RGB8 (*rgb: 3 bytes per point, released with rbt_free).
 * attr_t0 is required (attr_t1 too with two maps); attr_bit_depth 8 or 10. Geometry smoothing moves points, not colours: the re-colouring the reference decoder does after
 * its smoothing is rbt_reconstruct_decoded below. */
int rbt_reconstruct_rgb(rbt_ctx* ctx, const rbt_atlas_params* atlas, const rbt_patch* patches, int n_patches, const uint16_t* occ_luma, const uint16_t* geo_d0,
                        const uint16_t* geo_d1, int geo_bit_depth, const uint16_t* attr_t0, const uint16_t* attr_t1, int attr_bit_depth, int upsample_filter,
                        rbt_cloud* out, uint8_t** rgb);
/* Colour metric of QualityMetrics::compute (PCCMetrics.cpp:127-179, :221-225) with the reference's defaults dropDuplicates_ = 2 and neighborsProc_ = 1, both directions:
 *  - the points of a voxel are merged into one whose channels are sum / count in integer division (PCCPointSet.cpp:190-203);
 *  - a merged point of P is compared with the mean colour, rounded half up, of ALL merged points of Q at exactly the nearest squared distance (the reference looks at up to
 *    30 kd-tree results, in its order; here the set does not depend on any order, as in rbt_d2);
 *  - per channel the error term is the BT.709 row of convertRGBtoYUVBT709 (:50-55) times 10000 applied to the RGB difference, an integer of magnitude <= 2.55e6; sse is the
 *    sum of its squares, exact in 64 bits for up to 2^21 merged points per cloud (more are refused, RBT_ERR_PARAM);
 *  - mse = (float)(sse / (2550000^2 n)), psnr = 10 log10f(1 / mse) (getPSNR(mse, 1.0)): identical clouds give mse 0 and psnr +inf.
 * Coordinates 0..1023. Index 0, 1, 2 = Y, U, V. Upload + score + release, refusals and memory as at rbt_d1 (3 more bytes per point for the colours); both clouds need
 * colours, and the merged points are counted, and more than 2^21 refused, after the two uploads and before the score. */
typedef struct {
  int n_a, n_b;                            /* points after merging duplicates */
  uint64_t sse_ab[3], sse_ba[3];           /* exact integers */
  float mse_ab[3], mse_ba[3], psnr_ab[3], psnr_ba[3], mse[3], psnr[3];   /* mse = the larger, psnr = the smaller of the two directions (PCCMetrics.cpp:321-325) */
} rbt_color_result;
int rbt_color_metric(rbt_ctx* ctx, const int16_t* xyz_a, const uint8_t* rgb_a, int n_a, const int16_t* xyz_b, const uint8_t* rgb_b, int n_b, rbt_color_result* out);
/* Device time in milliseconds (events around the launches) the three stages took in this context's last call of each: [0] up-conversion, [1] RGB conversion,
 * [2] colour metric (the device_ms of its score: the search, the walks and the sums; the building of the two indices is outside); 0 for a stage that has not run and after a call that was refused. The stages are
 * separate launches inside calls that also copy and allocate: this is the only way to time them without a profiling build (tools/color_quality.py). */
int rbt_color_stage_ms(rbt_ctx* ctx, double ms[3]);

/* ---- attribute transfer after geometry smoothing (csrc/rbt_color.h) ----
 * Under the CTC settings the reference decoder copies the cloud, smooths the geometry and then re-colours every point the smoothing moved (PCCDecoder.cpp:434-494:
 * tempFrameBuffer.transferColors16bitBP(reconstruct, 1, 0, isAttributes444, 8, 1, true, true, true, false, 4, 4, 1000, 1000, 1000 * 256, 1000 * 256), PCCPointSet.cpp:1126-1485;
 * attrTransferFilterType_ 1). With these arguments the distance and colour pruning never fires and the search range is 0, and what is left is this.
 * Source S: the cloud before smoothing (positions, 16-bit 4:4:4 triples). Target T: the cloud after it, with the same colours, and one byte per point, "moved". Distances are
 * squared Euclidean distances of integer positions.
 *   forward, for every moved u:  N(u) = the 8 source points nearest to T[u]. If the nearest is at distance 0, color1[u] is its colour; else per channel
 *            color1[u] = clip16(round(sum(c_i w_i) / sum(w_i))), w_i = 1 / (dist_i + 4.0), in double, summed over N(u) in its order. The 8 neighbours of all moved points, moved
 *            points in index order, form the list E.
 *   backward, for every entry e of E:  v = the target point nearest to e's position (among ALL target points). If |e.colour - T.colour[v]| < 40 in all three channels (the
 *            colours before any update), (dist(e, v), e.colour) joins the list L(v).
 *   result, for every moved u:  L(u) empty: color1[u]; one entry: its colour; else per channel clip16(round(sum(c w) / sum(w))), w = 1 / (sqrt(dist) + 4.0), in list order.
 * round is C's (half away from zero); sqrt and the divisions are the correctly rounded double operations. Points that did not move keep their colour.
 * Where the reference depends on the order its kd-tree (nanoflann) returns equidistant points in, or on an unstable std::sort, this is defined instead, as rbt_d2 and
 * rbt_color_metric define their tie sets: N(u) is ordered by (distance, source index) - ties at the 8th place and among coincident points go to the lower index; v is the
 * lowest-index target point at the nearest distance; L(v) is ordered by (distance, position in E).
 * Coordinates 0..1023. tgt_yuv: the colours before on entry, after on return. *n_changed: points whose triple is another one afterwards. n_src < 8 (the reference's search
 * asserts there), a coordinate out of range or a null pointer: RBT_ERR_PARAM. n_tgt == 0 or no moved point: nothing to do, RBT_OK. `moved` may be set for a point whose
 * position is unchanged: it takes the colour of its source twin. A moved point with fewer than 8 source points within 64 grid units (per axis) is refused,
 * RBT_ERR_UNSUPPORTED: the search is bounded, and the smoothing does not carry a point that far from the cloud it came from. Two more limits, RBT_ERR_UNSUPPORTED as well, keep
 * the two single-lane sorts short: at most 256 source points at one position, at most 1024 entries in one list L(v). */
int rbt_transfer_colors(rbt_ctx* ctx, const int16_t* src_xyz, const uint16_t* src_yuv, int n_src, const int16_t* tgt_xyz, uint16_t* tgt_yuv, const uint8_t* moved, int n_tgt,
                        int* n_changed);
/* rbt_reconstruct_rgb followed by what the reference decoder does next: the positions before smoothing stay on the device, the smoothing runs with a flag per point, the
 * colours are transferred from the unsmoothed to the smoothed cloud as above, and the RGB conversion runs on the transferred triples (out->yuv holds them).
 * attr_transfer: 0 = off, 1 = the filter above; any other value (the reference's filter types 2, 3, 5, 7, 9) RBT_ERR_UNSUPPORTED. *moved (may be NULL): one byte per point, 1 for
 * the out->n_smoothed points the smoothing moved, released with rbt_free. With attr_transfer 0 or atlas->geometry_smoothing 0 the cloud and *rgb are rbt_reconstruct_rgb's.
 * Unlike rbt_reconstruct_rgb, the transfer needs the cloud inside the 1024^3 volume of the metrics: with attr_transfer 1 and at least one moved point, a coordinate outside
 * 0..1023 before or after smoothing gives RBT_ERR_PARAM (as do fewer than 8 points), and the limits of rbt_transfer_colors apply. */
int rbt_reconstruct_decoded(rbt_ctx* ctx, const rbt_atlas_params* atlas, const rbt_patch* patches, int n_patches, const uint16_t* occ_luma, const uint16_t* geo_d0,
                            const uint16_t* geo_d1, int geo_bit_depth, const uint16_t* attr_t0, const uint16_t* attr_t1, int attr_bit_depth, int upsample_filter, int attr_transfer,
                            rbt_cloud* out, uint8_t** rgb, uint8_t** moved);
/* The fourth colour stage next to rbt_color_stage_ms (whose array of three is part of the ABI): device milliseconds of the transfer's kernels (index building, forward,
 * backward, lists; in rbt_reconstruct_decoded also the two copies that keep the cloud from before the smoothing and the filter pass that writes the per-point flags; events
 * around the launches; the clears of the two 128 MB volumes and of the maps, the allocations and the read-back are outside) and the number of colours changed, in this context's last
 * rbt_transfer_colors or rbt_reconstruct_decoded; 0 when that call had nothing to transfer. Either pointer may be NULL. */
int rbt_transfer_stage(rbt_ctx* ctx, double* ms, int* n_changed);

/* ---- frame scoring on clouds that stay on the device (csrc/rbt_score.h) ----
 * This is the one implementation of the three metrics. A cloud is uploaded (or reconstructed) once and indexed once - bit volume, a coarse level over it, one map
 * voxel -> lowest point index + merged colour - and rbt_score runs one nearest-distance search per direction that feeds all three metrics. rbt_d1, rbt_d2 and
 * rbt_color_metric take host arrays and are this path on two clouds that live for the call: each uploads both clouds, scores its one part and releases them, so a caller
 * with more than one metric to take, or a cloud to score more than once, is better served here. out->d1 is what rbt_d1(a, b, peak) returns, out->color what
 * rbt_color_metric(a, b) returns and out->d2 what rbt_d2(a, normals_a, b, peak) returns, field for field and bit for bit (merged points and representatives, tie sets -
 * all points at exactly the nearest squared distance -, the give / take rule for the decoded cloud's normals). The order of the two D2 sums, of rbt_score and rbt_d2 alike:
 *   no floating-point atomics. The value v[i] of every point i is stored (0 for a point that is not the lowest-index point of its voxel) and the values are added in
 *   an order that depends on the input alone. Block b holds s[t] = v[256 b + t], t = 0..255 (0 past the last point) and
 *   is folded by s[t] = s[t] + s[t + h] for all t < h, h = 128, 64, .. 1; its sum is s[0]. Then S[t] = the sums of blocks t, t + 256, t + 512, .. added in ascending
 *   order starting from 0, t = 0..255, and S is folded the same way; sse = S[0]. Every operation is a double addition rounded on its own. Two calls therefore return the
 *   same bits, of rbt_score and of rbt_d2 alike, and so does the serial host emulation of the kernels. A sum taken in another order - the oracle's, or rbt_d2's before
 *   it became this path, which added with floating-point atomics in order of arrival - differs in the last bits (relative 1e-9 at most for these sizes); max_* and the
 *   counts are exact.
 * A handle belongs to the context that made it: used with another context it is refused (RBT_ERR_PARAM); rbt_destroy releases the handles still outstanding.
 * Limits: 1 .. 2^26 points a cloud, coordinates 0..1023 (a coordinate outside is RBT_ERR_PARAM: a kernel checks them and reports through an error word before any
 * word of the volume is touched). The colour part needs at most 2^21 merged points in each cloud (rbt_color_metric's limit: its integer sums are exact up to there); larger
 * clouds do not allow it, as clouds without colours do not. A handle holds a 128 MB volume; the volume of a released cloud is
 * cleaned (the cloud's own words) and kept by the context for its next cloud: rbt_device_memory counts such volumes as cached, rbt_trim hands them back. */
typedef struct rbt_pcloud rbt_pcloud;
/* xyz: 3 per point; rgb (3 bytes per point) and normals_q14 (3 per point, 16384 = 1.0) may be NULL: the colour part needs colours on both clouds, D2 normals on the source */
int rbt_pcloud_upload(rbt_ctx* ctx, const int16_t* xyz, const uint8_t* rgb, const int16_t* normals_q14, int n, rbt_pcloud** out);
/* rbt_reconstruct_decoded whose result stays on the device: positions after smoothing, the transferred 4:4:4 triples and their RGB8 triples are kept and indexed (no normals).
 * Arguments, limits and error codes are rbt_reconstruct_decoded's; in addition an empty cloud or a coordinate outside 0..1023 is RBT_ERR_PARAM. host_copy and rgb may be
 * NULL; given, they receive exactly what rbt_reconstruct_decoded returns (rbt_cloud_free / rbt_free). rbt_transfer_stage reports on the transfer as after
 * rbt_reconstruct_decoded. */
int rbt_pcloud_from_maps(rbt_ctx* ctx, const rbt_atlas_params* atlas, const rbt_patch* patches, int n_patches, const uint16_t* occ_luma, const uint16_t* geo_d0,
                         const uint16_t* geo_d1, int geo_bit_depth, const uint16_t* attr_t0, const uint16_t* attr_t1, int attr_bit_depth, int upsample_filter, int attr_transfer,
                         rbt_pcloud** out, rbt_cloud* host_copy, uint8_t** rgb);
int rbt_pcloud_points(const rbt_pcloud* cloud, int* n_points, int* n_merged);
void rbt_pcloud_release(rbt_ctx* ctx, rbt_pcloud* cloud);
enum { RBT_SCORE_D1 = 1, RBT_SCORE_D2 = 2, RBT_SCORE_COLOR = 4 };
typedef struct {
  int parts;                             /* RBT_SCORE_* computed; the results of the other parts are zero */
  rbt_d1_result d1; rbt_d2_result d2; rbt_color_result color;
  double device_ms;                      /* device time between events around the score's kernels (searches, walks, sums); index building, clears and read-back are outside */
  int n_points_a, n_points_b, n_merged_a, n_merged_b;
} rbt_frame_score;
/* a: the source (D2 needs its normals), b: the decoded cloud. parts: RBT_SCORE_* wanted, 0 = all the two clouds allow (out->parts says which); a part the clouds cannot
 * give, or peak < 1, is RBT_ERR_PARAM. */
int rbt_score(rbt_ctx* ctx, const rbt_pcloud* a, const rbt_pcloud* b, int peak, int parts, rbt_frame_score* out);
/* New colours for a cloud that is indexed already: rgb holds 3 bytes per point, in the cloud's point order (rbt_pcloud_points: n_points of them). Positions, volume, the
 * map's keys and lowest point indices stay; the colour sums, counts and merged colours of the index are remade (k_sc_recolor_zero, k_sc_recolor_add, then the merge of
 * rbt_pcloud_upload). Afterwards the cloud scores exactly as a fresh rbt_pcloud_upload of the same points with the new colours would - every integer and every float
 * field of every part; D1 and D2 do not change. A cloud uploaded without colours has them afterwards. The 4:4:4 triples a cloud of rbt_pcloud_from_maps keeps are not
 * touched. RBT_ERR_PARAM: a handle of another context. Score pairs of the cloud stay valid: their distances depend on positions only - and they read the clouds' colours of
 * the moment they are asked: recolouring a cloud that is the `reference` of a job of rbt_submit_gof_color in flight changes that job's scores, so leave a reference's colours
 * alone until the job is collected. */
int rbt_pcloud_set_colors(rbt_ctx* ctx, rbt_pcloud* cloud, const uint8_t* rgb);
/* A score pair keeps what of rbt_score(a, b) depends on positions only: the nearest squared distance of every merged point, both directions (8 bytes per point of the two
 * clouds; the two searches of rbt_score run once, at create). rbt_score_pair_color runs the colour walks alone on the stored distances (k_sc_color_walk: the tie sets, the
 * averaged tie colour and the error terms of rbt_score, integer sums, one 64-bit atomic per workgroup and sum) with the colours the two clouds have at that moment: out is
 * the .color part of rbt_score(a, b, peak, RBT_SCORE_COLOR), bit for bit, before and after rbt_pcloud_set_colors on either cloud. Where a sequence of candidates differs in
 * colour only - the trial encodes of an attribute stream over one geometry - this is the score without the searches, which are most of rbt_score's time.
 * RBT_ERR_PARAM: a handle of another context; at rbt_score_pair_color a cloud without colours, more than 2^21 merged points in a cloud, or a pair one of whose clouds has
 * been released (the pair itself is still released by rbt_score_pair_release; rbt_destroy releases the pairs still outstanding). */
typedef struct rbt_score_pair rbt_score_pair;
int rbt_score_pair_create(rbt_ctx* ctx, const rbt_pcloud* a, const rbt_pcloud* b, rbt_score_pair** out);
int rbt_score_pair_color(rbt_ctx* ctx, const rbt_score_pair* pair, rbt_color_result* out);
void rbt_score_pair_release(rbt_ctx* ctx, rbt_score_pair* pair);
/* ---- D1 per patch of the decoded cloud (csrc/rbt_score.h) ----
 * A is the reference cloud and B the decoded cloud. B carries a label L[j] in 0..P-1 per point: its patch index. Merging and representatives are rbt_score's, with the
 * lowest point index of a voxel as representative. Per patch k, with exact integers:
 *   B -> A   over the representatives j of B with L[j] = k: n_ba[k] counts them, sse_ba[k] is the sum of their nearest squared distances to A, max_ba[k] the maximum.
 *   A -> B   every representative i of A has a nearest squared distance d_i to B. Its owner is the representative of B with the lowest point index among all merged
 *            points of B at exactly distance d_i - rbt_score's tie set. n_ab[k], sse_ab[k] and max_ab[k] are taken over the i whose owner has label k. This holds for
 *            any reference, uploaded or decoded input; A needs no labels.
 *   figure   mse_*[k] = sse / n and psnr[k] = 10 log10(3 peak^2 / max(mse_ab, mse_ba)), from the one float routine rbt_d1 and rbt_score share. A direction without a
 *            point has mse 0; a patch without a point in either direction has psnr +inf.
 * The sums over k of sse_ab, sse_ba, n_ab and n_ba are rbt_score(a, b).d1's sse_ab, sse_ba, n_a and n_b; the maxima over k are its maxima.
 * Labels: a cloud of rbt_pcloud_from_maps carries the patch index of every point (the index into `patches` of the patch that emitted it), with geometry smoothing on or
 * off - smoothing moves points, it changes neither their order nor their patch. An uploaded cloud gets labels through rbt_pcloud_set_labels (one per point, in point
 * order, each below 65536; the cloud keeps the labels it had when the call fails). rbt_pcloud_labels copies them out (n_points words); RBT_ERR_PARAM for a cloud without
 * labels.
 * rbt_score_patches: out receives n_patches entries. whole and device_ms may be NULL; whole is bit for bit rbt_score(a, b, peak, RBT_SCORE_D1).d1, device_ms the time
 * between events around the two searches, the two D1 walks and the two per-patch kernels (k_pd_sums: integer atomics only, one per wave and word where a wave's labels are
 * all the same, so the words do not depend on the order of arrival and two calls return the same bits). RBT_ERR_PARAM, with the reason in rbt_last_error and the context
 * still usable: a handle of another context, b without labels, a label >= n_patches (a kernel checks the labels and reports through an error word before any sum is
 * written), n_patches outside 1..65536, peak < 1.
 * The closed loop on these figures: "D1 floors held patch by patch" below. (Colour figures per patch: "colour PSNR per patch of the decoded cloud" below.) */
typedef struct { uint32_t n_ab, n_ba; uint64_t sse_ab, sse_ba, max_ab, max_ba; float mse_ab, mse_ba, psnr; } rbt_patch_d1;
int rbt_pcloud_set_labels(rbt_ctx* ctx, rbt_pcloud* cloud, const uint32_t* labels);        /* one per point, < 65536 */
int rbt_pcloud_labels(rbt_ctx* ctx, const rbt_pcloud* cloud, uint32_t* labels);            /* of rbt_pcloud_from_maps: the patch index; RBT_ERR_PARAM for a cloud without labels */
int rbt_score_patches(rbt_ctx* ctx, const rbt_pcloud* a, const rbt_pcloud* b, int peak, int n_patches, rbt_patch_d1* out, rbt_d1_result* whole, double* device_ms);
/* ---- D2 per patch of the decoded cloud (csrc/rbt_score.h) ----
 * A is the source with normals, B the decoded cloud with one label per point, as for rbt_score_patches. Merging, representatives, tie sets, the give / take rule for B's
 * normals and the per-point values v_ab[i] (point i of A against B's completed normals) and v_ba[j] (point j of B against A's normals) are rbt_score's with RBT_SCORE_D2,
 * unchanged; a point that is no representative has the value 0. New are the attribution of the values to patches and the order of the sums.
 *   attribution  that of D1 per patch: v_ba[j] belongs to patch L[j]; v_ab[i] belongs to the label of i's owner, the lowest point index among B's merged points at
 *                exactly the nearest distance. n_ab[k] and n_ba[k] are therefore rbt_score_patches' counts.
 *   sums         no floating-point atomics. For patch k and one direction let w[i] = v[i] where the term of point i belongs to k, and 0 elsewhere (also where point i has no
 *                term). sse[k] is the fixed-order sum given at rbt_score - blocks of 256 entries folded by s[t] += s[t + h], h = 128 .. 1; the block sums added by column t,
 *                t + 256, .. in ascending order; the 256 columns folded the same way - applied to w, and max[k] is the maximum of w. The values are >= 0, so adding a 0
 *                changes no bit: the library skips blocks and columns in which a patch has no term and keeps the tree. With n_patches = 1, patch 0's sums and maxima are
 *                rbt_score(a, b, peak, RBT_SCORE_D2).d2's bit for bit; two calls return the same bits, and so does the serial host emulation.
 *   figure       mse_*[k] = sse / n and psnr[k] = 10 log10(3 peak^2 / max(mse_ab, mse_ba)) from the one float routine rbt_d2 and rbt_score use. A direction without a point
 *                has mse 0; a patch without a point in either direction has psnr +inf.
 * The sums over k of n_ab and n_ba are the whole's n_a and n_b; the maxima over k of max_ab and max_ba are its maxima bit for bit; the sums over k of sse_* are its sums
 * up to the rounding of a reordered double sum.
 * rbt_score_patches_d2: out receives n_patches entries. whole and device_ms may be NULL; whole is bit for bit rbt_score(a, b, peak, RBT_SCORE_D2).d2 (the same launches),
 * device_ms the time between events around those launches and the per-patch kernels (k_p2_block, k_p2_cols, k_p2_fold per direction). Scratch next to rbt_score's for D2:
 * 12 bytes per point of the larger cloud rounded up to a multiple of 256, 4 bytes per 256 points of it, and 2 KB + 48 bytes per patch - it grows with points + patches,
 * never with patches x blocks. RBT_ERR_PARAM, with the reason in rbt_last_error and the context still usable: those of rbt_score_patches (a handle of another context, b
 * without labels, a label >= n_patches - checked by a kernel before any sum is written -, n_patches outside 1..65536, peak < 1) and a without normals.
 * The closed loops on these figures: "D2 floors" below. (Colour figures per patch: the next section.) */
typedef struct { uint32_t n_ab, n_ba; double sse_ab, sse_ba, max_ab, max_ba; float mse_ab, mse_ba, psnr; } rbt_patch_d2;
int rbt_score_patches_d2(rbt_ctx* ctx, const rbt_pcloud* a, const rbt_pcloud* b, int peak, int n_patches, rbt_patch_d2* out, rbt_d2_result* whole, double* device_ms);
/* ---- colour PSNR per patch of the decoded cloud (csrc/rbt_score.h) ----
 * A is the reference and B the decoded cloud with one label L[j] per point, as for rbt_score_patches; both carry colours. Merging, representatives, tie sets, the rounded
 * mean tie colour and the three error terms e[0..2] (Y, U, V) of a representative are rbt_score's with RBT_SCORE_COLOR, unchanged (rbt_color_metric above). Only the
 * attribution is new, and it is that of D1 per patch. Per patch k, with exact integers:
 *   B -> A   a representative j of B belongs to patch L[j]: n_ba[k] counts the representatives of patch k, sse_ba[c][k] is the sum of e[c]^2 over them.
 *   A -> B   a representative i of A belongs to the label of its owner, the lowest point index among B's merged points at exactly i's nearest distance. n_ab[k] and
 *            sse_ab[c][k] are taken over the i whose owner has label k: the counts are rbt_score_patches' counts for the same pair.
 *   figure   mse_*[c][k] = (float)(sse / (2550000^2 n)) and psnr = 10 log10f(1 / mse), from the one float routine rbt_color_metric and rbt_score use. A direction without
 *            a point has mse 0. mse[c] is the larger and psnr[c] the smaller of the two directions; a patch without a point in either direction has psnr +inf.
 * All relations are exact - the sums are integers: over k, sse_ab[c], sse_ba[c], n_ab and n_ba add up to the whole's sse_ab[c], sse_ba[c], n_a and n_b; with n_patches = 1
 * patch 0 is the whole, float fields included; two calls return the same bits, and so does the serial host emulation.
 * rbt_score_patches_color: the two searches of rbt_score, then k_pc_sums once per direction in place of the colour walks - one lane per point, one walk over the tie set
 * that yields the tie colour sums and the owner, eight 64-bit words per patch (three sums and a count per direction), integer atomics only, one per wave and non-zero word
 * where a wave's labels are all the same. whole (may be NULL) is made on the host from the per-patch words through the same float routine: bit for bit
 * rbt_score(a, b, peak, RBT_SCORE_COLOR).color for any peak. device_ms (may be NULL): the time between events around the searches and the two launches.
 * rbt_score_pair_patches_color: the same on the distances a score pair keeps, with the colours and labels the clouds have at that moment: no search runs; whole is bit for
 * bit rbt_score_pair_color(pair), out is rbt_score_patches_color's, before and after rbt_pcloud_set_colors on either cloud. Scratch: 64 bytes per patch beside what the
 * score or the pair holds.
 * RBT_ERR_PARAM, with the reason in rbt_last_error and the context still usable: a handle or pair of another context, a pair one of whose clouds has been released, a cloud
 * without colours, b without labels, a label >= n_patches (k_pd_check reports through an error word before any sum is written), n_patches outside 1..65536, more than
 * 2^21 merged points in a cloud.
 * The closed loop on these figures: "colour floors held patch by patch" at the end of this header. */
typedef struct { uint32_t n_ab, n_ba; uint64_t sse_ab[3], sse_ba[3]; float mse_ab[3], mse_ba[3], mse[3], psnr[3]; } rbt_patch_color;
int rbt_score_patches_color(rbt_ctx* ctx, const rbt_pcloud* a, const rbt_pcloud* b, int n_patches, rbt_patch_color* out, rbt_color_result* whole, double* device_ms);
int rbt_score_pair_patches_color(rbt_ctx* ctx, const rbt_score_pair* pair, int n_patches, rbt_patch_color* out, rbt_color_result* whole);
/* Summary over the frames of a sequence, per figure (the symmetric PSNR of D1, D2, Y, U, V): arithmetic mean and minimum, in double, over the frames that carry that part
 * (n_d1 / n_d2 / n_color of them; 0 where there is none); a frame whose PSNR is +inf makes the mean +inf. The reference itself writes one line per frame and averages
 * nothing (PCCMetrics::write); the mean over the frames is what the CTC reporting forms from those lines. points_* / merged_*: sums over all frames. Host only. */
typedef struct {
  int n_frames, n_d1, n_d2, n_color;
  double mean_d1, min_d1, mean_d2, min_d2, mean_color[3], min_color[3];
  int64_t points_a, points_b, merged_a, merged_b;
} rbt_sequence_score;
int rbt_score_summary(const rbt_frame_score* frames, int n_frames, rbt_sequence_score* out);

/* The target and the result of a transcode to a D1 floor ("transcoding geometry to a D1 floor" above). */
struct rbt_d1_target {
  uint32_t struct_size;                  /* sizeof(rbt_d1_target): checked */
  int32_t  min_d1_mdb;                   /* floor on D, 1/1000 dB; 0 = none: coded at params[i].qp, D1 reported */
  int      stat;                         /* RBT_D1_MIN (the default): the floor is on the worst frame; RBT_D1_MEAN: on the mean over the frames */
  int      peak;                         /* 0 = 1023 */
  int      qp_min, qp_max;               /* the walk's range; qp_max 0 = 51 */
  int      n_frames;                     /* point-cloud frames of the entry; 0 in an empty target */
  rbt_atlas_params atlas;                /* the OUTPUT atlas: occupancy_precision is that of the output occupancy video */
  const rbt_patch* const* patches;       /* n_frames lists (a NULL list only with a count of 0) ... */
  const int* n_patches;                  /* ... and their lengths; copied at submit */
  const rbt_pcloud* const* reference;    /* NULL, or n_frames handles: A_f; a NULL handle = the cloud of the decoded input */
};
struct rbt_d1_floor_result {
  int qp, qp_probe, qp_start, met, n_encodes;   /* q*, q0, qs, met, distinct QPs encoded */
  uint64_t bytes;                               /* size of the returned stream */
  double mean_d1, min_d1;                       /* over the frames at q*: the sum of (double)psnr in frame order / n_frames, and the minimum */
  int n_frames;                                 /* 0 for an entry without a target */
  rbt_d1_result* frames;                        /* n_frames results at q* (malloc'd, rbt_free; NULL for an entry without a target) */
  double cloud_ms;                              /* time between events on the pipeline's stream around the gather, the reconstruction, the index and the search of every cloud
                                                 * of the job's rounds for this entry, the reference clouds included: the kernels and the gaps in which the stream waits for the
                                                 * host's read-backs of counts and its launches (the clear of a released volume is outside) */
};

/* The target and the result of a transcode to a colour PSNR floor ("transcoding attributes to a colour PSNR floor" above). */
struct rbt_color_target {
  uint32_t struct_size;                  /* sizeof(rbt_color_target): checked */
  int32_t  min_psnr_mdb;                 /* floor on D, 1/1000 dB; 0 = none: coded at params[i].qp, the colour results reported */
  int      channel;                      /* 0 Y (the default), 1 U, 2 V: the channel of the symmetric colour PSNR the floor is on */
  int      stat;                         /* RBT_D1_MIN (the default): the floor is on the worst frame; RBT_D1_MEAN: on the mean over the frames */
  int      qp_min, qp_max;               /* the walk's range; qp_max 0 = 51 */
  int      n_frames;                     /* point-cloud frames of the entry; 0 in an empty target */
  rbt_atlas_params atlas;                /* the OUTPUT atlas: occupancy_precision is that of the output occupancy video */
  const rbt_patch* const* patches;       /* n_frames lists (a NULL list only with a count of 0) ... */
  const int* n_patches;                  /* ... and their lengths; copied at submit */
  int      upsample_filter;              /* RBT_UPSAMPLE_F0 or RBT_UPSAMPLE_REPLICATE, as rbt_pcloud_from_maps takes it */
  int      attr_transfer;                /* 0 or 1, as rbt_pcloud_from_maps takes it */
  const rbt_pcloud* const* reference;    /* NULL, or n_frames handles: A_f; a NULL handle = the cloud of the decoded input */
};
struct rbt_color_floor_result {
  int qp, qp_probe, qp_start, met, n_encodes;   /* q*, q0, qs, met, distinct QPs encoded */
  uint64_t bytes;                               /* size of the returned stream */
  double mean_psnr[3], min_psnr[3];             /* Y, U, V over the frames at q*: the sum of (double)psnr[c] in frame order / n_frames, and the minimum */
  int n_frames;                                 /* 0 for an entry without a target */
  rbt_color_result* frames;                     /* n_frames results at q* (malloc'd, rbt_free; NULL for an entry without a target) */
  double cloud_ms;                              /* time between events on the pipelines' streams around the work on the clouds: the geometry half and the references once,
                                                 * then per trial gather, up-conversion, fetch, transfer, RGB, recolour and colour walks, with the gaps in which the stream
                                                 * waits for the host */
};

/* ---- floors held frame by frame (host/rbt_frame_walk.h) ----
 * rbt_submit_gof_quality holds the floor on the sums of the whole stream; a D1 floor on the worst frame makes that frame dictate the QP of all. Here every point-cloud
 * frame of an entry walks to its own QP, and the returned stream carries a QP per frame ("a QP per point-cloud frame" above): every frame is coded just as well as
 * required. The entry points take rbt_quality_target unchanged.
 *
 * 1. Figure of frame f at QP q: rule 2 of the PSNR floor applied to the sums of pictures 2f and 2f + 1 together, plane 0 of the chosen region; meets is rule 4 there. By
 *    the composition rule of the QP list it is what a constant-QP trial at q gives for these two pictures.
 * 2. Probe. One pass at q0 = clamp(params[i].qp, lo, hi) for all frames.
 * 3. Start. Per frame qs_f by the PSNR floor's rule: q0 if the figure is infinite, else clamp(q0 + (int)(figure_f(q0) - F), lo, hi).
 * 4. Walk. One walk per frame, the PSNR floor's rule 5 word for word, on frame f's figures alone: q*_f, met_f; n_encodes_f <= |q*_f - qs_f| + 5.
 * 5. Rounds. A pass is one encode launch sequence over (frame, QP) pairs of one entry; frames that are not listed are not encoded. In a round every unsettled frame names
 *    its QPs as the PSNR floor's rounds name them; pass j of the round carries, for each frame that named at least j + 1 QPs, the j-th of them. Settled frames are in no
 *    pass. pictures_encoded = 2 * the sum of n_encodes_f; n_passes counts the passes. The result depends on the figures alone, not on how the passes are formed.
 * 6. Stream. Byte for byte rbt_transcode_gof_frame_qp's for Q = (q*_0, .., q*_{F-1}). It is assembled on the host from the NAL units the passes returned - every pass
 *    writes the parameter sets of params[i].qp -; no further encode runs. frames[f].bytes is the size of frame f's NAL units in it, start codes included.
 * 7. min_psnr_mdb 0: the constant-QP stream at params[i].qp, the figures reported per frame (qp = qp_start = params[i].qp, met = 1, n_encodes = 1). A floor that lo misses
 *    for some frame is no error: that frame comes back at lo with met = 0, and the call returns RBT_OK.
 * 8. Errors, the occupancy source, occupancy_rd and the lifetime of the occupancy planes are the PSNR floor's; a geometry / attribute entry with an odd number of pictures
 *    is refused as well (RBT_ERR_PARAM, nothing submitted). A job of rbt_submit_gof_quality_frames is collected by
 *    rbt_wait_gof_quality_frames only, and rbt_wait_gof_quality_frames collects no other job: any other pairing is RBT_ERR_PARAM and the job stays collectable.
 *    rbt_job_memory counts the first round (the probe passes). Occupancy entries are coded as rbt_submit_gof codes them: n_frames 0, frames NULL, qp_probe = params[i].qp.
 * D1 kind (rbt_submit_gof_d1_frames, with rbt_d1_target unchanged): the figure of frame f at q is (double)psnr of D_f(q), D1 rule 5, with the same references, smoothing and
 * occupancy source; the walk per frame is D1 rule 6 on that figure. stat must be 0 (RBT_D1_MIN) and atlas.map_count 2 (a frame is the pair of pictures), else
 * RBT_ERR_PARAM. The clouds of a pass are made of the frames it carries: the gather descriptors go by the coded picture, the maps, patch lists and references by the frame.
 * results[i].d1 holds the rbt_d1_result of every frame at q*_f, cloud_ms the time of rbt_d1_floor_result.cloud_ms; sums is reported as for the PSNR kind. Entries without
 * a target carry an empty target and are coded at params[i].qp (their frames are reported with the PSNR figure). Errors, pairing and memory are the D1 section's; the job
 * is collected by rbt_wait_gof_d1_frames only. There is no container-level call, as for rbt_submit_gof_d1.
 * Not built: byte caps and colour floors per frame, two kinds of floor in one job. */
typedef struct { int qp, qp_start, met, n_encodes; uint64_t bytes; double figure; } rbt_frame_pick;   /* q*_f, qs_f, met_f, distinct QPs encoded, frame f's bytes, its figure at q*_f */
typedef struct {
  int n_frames, qp_probe, met_all, n_passes;      /* q0; met_all = AND of frames[f].met */
  uint64_t bytes, pictures_encoded;               /* size of the returned stream; 2 * sum of frames[f].n_encodes */
  rbt_frame_pick* frames;                         /* n_frames picks (malloc'd, rbt_free; NULL for an occupancy entry) */
  rbt_quality_result sums;                        /* over the returned stream, as rbt_wait_gof_quality reports them; its qp fields are -1 */
  rbt_d1_result* d1;                              /* D1 kind: n_frames results, frame f at q*_f (malloc'd, rbt_free); else NULL */
  double cloud_ms;                                /* D1 kind: as rbt_d1_floor_result.cloud_ms; else 0 */
} rbt_frame_floor_result;
int rbt_submit_gof_quality_frames(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_quality_target* targets, rbt_job** job);
int rbt_wait_gof_quality_frames(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_frame_floor_result* results);   /* results: n entries */
int rbt_transcode_gof_quality_frames(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_quality_target* targets,
                                     uint8_t** annexb_out, size_t* n_out, rbt_frame_floor_result* results);   /* submit + wait */
int rbt_submit_gof_d1_frames(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_d1_target* targets, rbt_job** job);
int rbt_wait_gof_d1_frames(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_frame_floor_result* results);   /* results: n entries */
int rbt_transcode_gof_d1_frames(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_d1_target* targets,
                                uint8_t** annexb_out, size_t* n_out, rbt_frame_floor_result* results);   /* submit + wait */
/* rbt_transcode_v3c_quality with the floors held frame by frame: the same walk over jobs of rbt_submit_gof_quality_frames, the same arguments. *per_gof (may be NULL): two
 * results per GOF of the input, geometry then attribute, zeros for a GOF this context does not own; the caller releases every frames array, then the array itself
 * (rbt_free). With both floors 0 the output is rbt_transcode_v3c's. */
int rbt_transcode_v3c_quality_frames(rbt_ctx* ctx, const uint8_t* in, size_t n, const rbt_v3c_params* p, int32_t geometry_min_psnr_mdb, int32_t attribute_min_psnr_mdb, int region,
                                     uint8_t** out, size_t* n_out, rbt_frame_floor_result** per_gof);

/* ---- a QP per CTB (csrc/rbt_qpmap.h, host/rbt_transcode.cpp encode_plan) ----
 * Every call above spends one QP on a whole picture. An atlas picture is a few dozen patches and the padding between them, and what a V-PCC user steers is the patch. Here a
 * geometry / attribute entry may carry a map with one QP per CTB and point-cloud frame: M[f][r][c], n_frames * h_ctb * w_ctb values, row-major. It is the building block,
 * as the QP list was for the floors held frame by frame: the PSNR floors held patch by patch (below) are built on it; byte caps per patch are not built yet.
 *
 * Let T be the target QP of a CTB: max(0, M[f][r][c] - 3) in picture 2f and M[f][r][c] in picture 2f + 1, the constant-QP path's own I / P rule.
 * 1. Decisions. Everything the encoder derives from the QP takes T of the CTB it works in instead of the slice's QP: the quantiser and the dequantiser, the chroma QPs, the
 *    lambdas of the analysis, of the closed-loop decisions and of the SAO decision, the rounding offsets. Nothing else about a decision changes.
 * 2. Parameter sets. Those of rbt_transcode_gof at params[i].qp, except cu_qp_delta_enabled_flag = 1 and diff_cu_qp_delta_depth = 0 in the PPS of an entry that carries a
 *    map: the quantisation group is the CTB.
 * 3. Slice QP. SliceQpY of every independent slice segment is T of its first CTB; the dependent segments of a wavefront picture inherit it.
 * 4. Signalling (H.265 7.3.8.14, 8.6.1). In a CTB the first transform unit in decoding order with a luma or chroma cbf carries cu_qp_delta_abs / cu_qp_delta_sign_flag, no
 *    later unit of that CTB does. The value d is the one in -(26 + QpBdOffset / 2) .. 25 + QpBdOffset / 2 with wrap(pred + d) = T, wrap being the modular rule of 8.6.1:
 *    it is not T - pred where that leaves the range (CTB 0 next to CTB 51 is legal).
 * 5. Prediction. With the group as large as the CTB the left and upper neighbours of 8.6.1 are never in the same CTB, so pred = qPY_PREV: the QpY of the last coding unit
 *    of the previous CTB in decoding order, SliceQpY at the first CTB of a slice and, in wavefront mode, of every CTB row. In closed form: pred(c) is T of the nearest
 *    earlier CTB of the same slice (same row under wavefront) that has any cbf, SliceQpY if there is none.
 * 6. The QpY a decoder derives, and the deblocking filter reads: pred(c), not T, for a coding unit of a CTB that comes before the first unit with a cbf, and for every unit
 *    of a CTB without any cbf (skipped P CUs mostly); T from the coding unit with the first cbf on. The encoder's loop filters read the same values, so that the stream
 *    decodes to the encoder's reconstruction (md5_sei says so picture by picture).
 * 7. No map. An entry with n_frames 0 and qp NULL, or maps == NULL, is coded as rbt_submit_gof codes it, byte for byte; the PPS flag stays 0.
 * 8. Uniform map. If every M[f][r][c] == q every cu_qp_delta coded is 0 and every QpY is the slice's: the decoded pictures equal those of C(q), rbt_transcode_gof's stream
 *    at qp = q, sample for sample, and the hash SEI NAL units are those of C(q) byte for byte. A map that is constant per frame, M[f][..] == Q[f], decodes to what
 *    rbt_transcode_gof_frame_qp with the list Q decodes to, hash SEIs included; the bytes differ by the PPS flag and the zero deltas.
 * 9. occupancy_rd, the input-mode hints, the flat-chroma fill, verify_md5, md5_sei, preset, log2_ctb 4..6, every slice structure and every job depth behave as in the
 *    constant-QP path. A slice buffer is sized from the lowest T of its CTBs; overflow stays RBT_ERR_OUTPUT.
 * 10. RBT_ERR_PARAM (reason in rbt_last_error; nothing is submitted and the context stays usable): struct_size that is not sizeof(rbt_qp_map); a map on an occupancy entry
 *    (coded losslessly); n_frames that is not pictures / 2, or a stream with an odd picture count; w_ctb / h_ctb that are not the CTB columns / rows of the output pictures
 *    at the entry's log2_ctb; a value outside 0..51; a map without its counts, or counts without a map.
 * The maps are copied at submit. The job is a job of rbt_submit_gof in every other respect: depth, rbt_job_memory, rbt_wait_gof, shared pipelines. Maps together with a rate,
 * quality, D1 or colour target are not offered.
 * Not built: byte caps per patch (PSNR floors per patch: below), a map in the container-level calls (rbt_transcode_v3c), quantisation groups smaller than the CTB. */
typedef struct {
  uint32_t struct_size;   /* sizeof(rbt_qp_map): checked */
  int n_frames;           /* pictures / 2; 0 with qp NULL = no map */
  int w_ctb, h_ctb;       /* CTB columns / rows of the OUTPUT pictures at the entry's log2_ctb (0 = 5): ceil(w / ctb), ceil(h / ctb) */
  const int8_t* qp;       /* M[f][r][c], n_frames * h_ctb * w_ctb values, row-major, 0..51 */
} rbt_qp_map;
int rbt_submit_gof_qp_map(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_qp_map* maps, rbt_job** job);   /* collected by rbt_wait_gof */
int rbt_transcode_gof_qp_map(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_qp_map* maps,
                             uint8_t** annexb_out, size_t* n_out);   /* submit + wait */
/* Host helper, no device work: the map of one frame from its patches. CTB (c, r) of a picture of atlas->width x atlas->height samples cut into CTBs of 1 << log2_ctb gets the
 * minimum of patch_qp[k] over the patches whose rectangle - u0, v0, size_u0, size_v0 in blocks of atlas->occupancy_resolution - meets the CTB, background_qp where none
 * does. out: h_ctb * w_ctb values, row-major. RBT_ERR_PARAM: a null argument (patches and patch_qp may be NULL with n_patches 0), log2_ctb outside 4..6, w_ctb / h_ctb
 * that are not ceil(width / ctb), ceil(height / ctb), a QP outside 0..51, occupancy_resolution < 1. A patch that reaches beyond the atlas is clipped to it. */
int rbt_qp_map_from_patches(const rbt_atlas_params* atlas, const rbt_patch* patches, int n_patches, const int8_t* patch_qp, int background_qp,
                            int log2_ctb, int8_t* out, int w_ctb, int h_ctb);

/* ---- PSNR floors held patch by patch (csrc/rbt_ctbsse.h, host/rbt_patch_walk.h) ----
 * "Every patch of every frame keeps X dB, bits spent only on the patches that need them": the closed loop on the QP per CTB, for the luma PSNR - the figure that needs nothing
 * but the pictures already in device memory. Per entry with a target the caller gives, per point-cloud frame f, the patch list (the fields rbt_qp_map_from_patches reads).
 *
 * 1. Region. R_k, the region of patch k, is the set of CTBs its rectangle meets - rbt_qp_map_from_patches' rule, clipping included. A CTB two patches meet counts for both.
 * 2. Sums. Behind a trial's last filter k_ctb_sse leaves, per picture and CTB of the output grid, {sse, sse_occ, n_occ} of the luma samples of the CTB that lie in the
 *    displayed area - A, B and "occupied" are those of the PSNR floor's rule 1 -, and k_patch_fold adds them over R_k in pictures 2f and 2f + 1. Only the folded words come
 *    back, with the slice sizes.
 * 3. Figure of patch k in a trial: rule 2 of the PSNR floor on the folded sums of R_k, in the chosen region (RBT_QUALITY_ALL: sse over the displayed samples of R_k in both
 *    pictures; RBT_QUALITY_OCCUPIED: sse_occ over n_occ). meets is rule 4 of the PSNR floor with the patch's floor F_k: a patch without a CTB or without a sample meets.
 * 4. Trial map. A frame's trial with the vector q[] is coded with rbt_qp_map_from_patches(atlas, patches, q, background, log2_ctb): a shared CTB takes the lower QP, the
 *    background takes background_qp, q0 where that is -1.
 * 5. Walk (host/rbt_patch_walk.h). Frames are closed pairs of pictures, so each frame walks alone. lo, hi and q0 = clamp(params[i].qp, lo, hi) are the PSNR floor's.
 *    Trial 0 has q[k] = q0 for all k. After a trial every patch updates: if it does not meet, failed[k] = 1 and, if q[k] > lo, q[k] -= max(1, (int)(F_k - figure_k)),
 *    clamped at lo; if it meets, has never failed, q[k] < hi, its figure is finite and (int)(figure_k - F_k) >= 1, q[k] += (int)(figure_k - F_k), clamped at hi; otherwise
 *    it stays. The casts truncate toward zero. If no q[k] changed the frame has settled on this trial, else the next trial takes the new vector. A patch moves up until its
 *    first failure and only down after it, so a frame's vector never repeats and the walk ends. max_trials (0 = no cap): a frame that reaches it settles on its last trial,
 *    met as measured. The distortion of a patch depends on its neighbours' QPs and is not monotone in its own, so the walk is the definition: the result is a map under
 *    which every patch meets or sits at lo, reached by this walk - it is NOT a proof of the cheapest such map.
 * 6. Rounds. A round is one pass per entry over the frames that have not settled, each with its trial map; settled frames are in no later pass. pictures_encoded = 2 * the
 *    sum of the frames' n_trials, n_passes = the largest n_trials.
 * 7. Stream. Byte for byte rbt_transcode_gof_qp_map's for the final map (results[i].map), assembled on the host from the frames' NAL units of their settling trials; every
 *    pass writes the parameter sets of params[i].qp with cu_qp_delta_enabled_flag = 1. No further encode runs.
 * 8. Floor 0. With min_psnr_mdb 0 and patch_min_psnr_mdb NULL there is one trial at clamp(params[i].qp, 0, 51): the figures per patch are reported, met = 1.
 * 9. Everything is copied at submit. The pairing rule (rbt_wait_gof_quality_patches and no other wait; a wrong pairing is RBT_ERR_PARAM and leaves the job collectable),
 *    rbt_job_memory (the first round at params[i].qp; the map and the words per CTB, 26 bytes a CTB and picture, are not in it), the occupancy source, occupancy_rd, the
 *    lifetime of the pooled planes and the errors are the PSNR floor's. Further refusals, all RBT_ERR_PARAM with a reason, nothing submitted, the context usable: a wrong
 *    struct_size; an odd picture count; n_frames that is not pictures / 2; an atlas size that is not the output pictures'; occupancy_resolution < 1; a background_qp
 *    outside -1..51; a negative max_trials; a negative floor; a QP range or a region the PSNR floor refuses; a frame with patches but no list; a target on an occupancy
 *    entry. An entry without a target (n_frames 0, everything else 0) is coded at params[i].qp: n_frames 0, map and frames NULL, sums filled.
 * There is no container-level call and no rbt_pipeline option: the library does not parse the atlas sub-bitstream.
 * Not built: byte caps per patch (D1, D2 and colour floors per patch: below), a caller's map together with a target, quantisation groups below the CTB. */
typedef struct {
  uint32_t struct_size;                                        /* sizeof(rbt_patch_floor_target): checked */
  int32_t  min_psnr_mdb;  int region;  int qp_min, qp_max;     /* as rbt_quality_target */
  int      background_qp;                                      /* 0..51, -1 = q0 */
  int      max_trials;                                         /* 0 = no cap */
  rbt_atlas_params atlas;                                      /* width, height, occupancy_resolution are read */
  int n_frames;  const rbt_patch* const* patches;  const int* n_patches;
  const int32_t* const* patch_min_psnr_mdb;                    /* NULL, or per frame NULL / one floor per patch: F_k; else F_k = min_psnr_mdb */
} rbt_patch_floor_target;
typedef struct { int qp, met, failed; uint64_t sse, samples; double figure; } rbt_patch_pick;   /* of the settling trial: q[k], met, failed[k], the sums of R_k in the chosen region, the figure */
typedef struct {
  int n_trials, met, n_patches;                                /* met = AND of patches[k].met */
  uint64_t bytes;                                              /* the frame's NAL units in the returned stream, start codes included */
  uint64_t background[3];                                      /* sse, sse_occ, n_occ of the CTBs no patch meets */
  rbt_patch_pick* patches;                                     /* n_patches picks: they point into rbt_patch_floor_result.picks */
} rbt_patch_frame;
typedef struct {
  int n_frames, qp_probe, met_all, n_passes;                   /* q0; met_all = AND of frames[f].met */
  uint64_t bytes, pictures_encoded;                            /* size of the returned stream; 2 * sum of frames[f].n_trials */
  int w_ctb, h_ctb;
  int8_t* map;                                                 /* the final map, n_frames * h_ctb * w_ctb (malloc'd, rbt_free): rbt_transcode_gof_qp_map returns the same stream for it */
  rbt_patch_frame* frames;                                     /* n_frames (malloc'd, rbt_free) */
  rbt_patch_pick* picks;                                       /* every frame's picks back to back (malloc'd, rbt_free) */
  rbt_quality_result sums;                                     /* over the returned stream, as rbt_wait_gof_quality reports them; its qp fields are -1 */
} rbt_patch_floor_result;
int rbt_submit_gof_quality_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_floor_target* targets, rbt_job** job);
int rbt_wait_gof_quality_patches(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_patch_floor_result* results);   /* results: n entries */
int rbt_transcode_gof_quality_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_floor_target* targets,
                                      uint8_t** annexb_out, size_t* n_out, rbt_patch_floor_result* results);   /* submit + wait */
/* The two kernels on host arrays (tests, and users who only want the measurement): pictures laid out as for rbt_picture_sse. out_ctb: n_frames x h_ctb x w_ctb x {sse,
 * sse_occ, n_occ} of the luma plane, the grid being ceil(width / ctb) x ceil(height / ctb). rects (may be NULL with n_rects 0): n_rects x {c0, r0, c1, r1} in CTB units,
 * half-open, the same list for every pair of pictures; out_rect (may be NULL; needs an even n_frames): (n_frames / 2) x (n_rects + 2) x 3 - the rectangles, then the
 * background (the CTBs no rectangle meets), then the whole frame. RBT_ERR_PARAM: rbt_picture_sse's refusals, log2_ctb outside 4..6, a rectangle outside the grid.
 * rbt_get_stats afterwards: gpu_ms = the device time between events around the two launches. */
int rbt_ctb_sse(rbt_ctx* ctx, const uint16_t* a, const uint16_t* b, int width, int height, int n_frames, int log2_ctb, const uint16_t* occ, int ow, int oh,
                const int32_t* rects, int n_rects, uint64_t* out_ctb, uint64_t* out_rect);

/* ---- D1 floors held patch by patch (csrc/rbt_score.h, host/rbt_patch_walk.h) ----
 * The PSNR floor per patch counts every sample of a CTB, although the occupancy map of the output decides which samples become points; the D1 floor per frame measures the
 * right figure but moves one QP per frame, so a frame's worst patch dictates the QP of every other patch in it. Here every patch of every frame of a geometry entry walks
 * to its own QP on its own D1 ("D1 per patch of the decoded cloud" above), and the result names the patch that sets a frame's D1.
 *
 * 1. Cloud and reference of a trial. Rules 1 - 4 of "transcoding geometry to a D1 floor", unchanged: the occupancy source, the shapes, B_f (the cloud of the trial's
 *    reconstruction of frame f through the output atlas) and A_f (reference[f], or the cloud of the decoded input where that is NULL). atlas.map_count must be 2: a
 *    point-cloud frame is the two pictures that are coded as a pair. B_f carries the labels of rbt_pcloud_from_maps: the index of the point's patch in the frame's list.
 * 2. Figure. The figure of patch k of frame f in a trial is (double)psnr[k] of rbt_score_patches on (A_f, B_f(trial map)) with peak (0 = 1023). meets is
 *    figure >= F_k / 1000.0; +inf meets (a patch that contributes no point and owns no reference point).
 * 3. Trial map, walk, rounds, stream: rules 4 - 7 of "PSNR floors held patch by patch", word for word, with this figure (patch_walk_seed / patch_walk_step unchanged). A
 *    round is one pass per entry over the unsettled frames with their trial maps; behind the pass the clouds of the frames it carried are built and scored one after the
 *    other. The returned stream is byte for byte rbt_transcode_gof_qp_map's for the final map, assembled from the settling trials; no further encode runs. The walk moves a
 *    patch by (int)(F_k - figure) QP steps, a model of 1 dB per step: that is poor for D1, which saturates where the quantisation error stays below half a depth level and
 *    depends on the neighbours' points. This costs trials, not correctness: the walk is the definition, and the result is a map under which every patch meets or sits at lo.
 * 4. Floor 0. With min_d1_mdb 0 and patch_min_d1_mdb NULL there is one trial at clamp(params[i].qp, 0, 51): every patch's rbt_patch_d1 is reported and met = 1.
 * 5. Everything is copied at submit. A job is collected by rbt_wait_gof_d1_patches only; a wrong pairing is RBT_ERR_PARAM and leaves the job collectable. rbt_job_memory is
 *    as in the D1 section. Refusals, all RBT_ERR_PARAM with a reason, nothing submitted, the context usable: those of the D1 section (no occupancy source, shapes that do
 *    not fit, a foreign reference handle, a negative floor or peak, a bad QP range, a malformed patch list) and those of the patch-floor section (a wrong struct_size, an
 *    odd picture count, n_frames that is not pictures / 2, an atlas size that is not the output pictures', a background_qp outside -1..51, a negative max_trials, a
 *    negative patch floor, log2_ctb outside 4..6); a target on an attribute or occupancy entry; map_count other than 2; occupancy_rd together with verify_md5 as the PSNR
 *    floor refuses it. An entry without a target (n_frames 0, everything else 0) is coded at params[i].qp: n_frames 0, map, frames and picks NULL.
 * Not built: byte caps per patch, a caller's map together with a target, and a container-level call or rbt_pipeline option - the library does not
 * parse the atlas sub-bitstream. */
typedef struct {
  uint32_t struct_size;                                        /* sizeof(rbt_patch_d1_target): checked */
  int32_t  min_d1_mdb;  int peak;  int qp_min, qp_max;         /* as rbt_d1_target: floor in 1/1000 dB (0 = none), peak 0 = 1023, qp_max 0 = 51 */
  int      background_qp;                                      /* 0..51, -1 = q0 */
  int      max_trials;                                         /* 0 = no cap */
  rbt_atlas_params atlas;                                      /* the OUTPUT atlas, as in rbt_d1_target */
  int n_frames;  const rbt_patch* const* patches;  const int* n_patches;
  const int32_t* const* patch_min_d1_mdb;                      /* NULL, or per frame NULL / one floor per patch: F_k; else F_k = min_d1_mdb */
  const rbt_pcloud* const* reference;                          /* NULL, or n_frames handles: A_f; a NULL handle = the cloud of the decoded input */
} rbt_patch_d1_target;
typedef struct { int qp, met, failed; rbt_patch_d1 d1; double figure; } rbt_patch_d1_pick;   /* of the settling trial: q[k], met, failed[k], the patch's sums and figures, (double)d1.psnr */
typedef struct {
  int n_trials, met, n_patches;                                /* met = AND of patches[k].met */
  uint64_t bytes;                                              /* the frame's NAL units in the returned stream, start codes included */
  rbt_d1_result d1;                                            /* the whole frame's D1 in the settling trial: what rbt_score returns for (A_f, B_f) */
  rbt_patch_d1_pick* patches;                                  /* n_patches picks: they point into rbt_patch_d1_result.picks */
} rbt_patch_d1_frame;
typedef struct {
  int n_frames, qp_probe, met_all, n_passes;                   /* q0; met_all = AND of frames[f].met */
  uint64_t bytes, pictures_encoded;                            /* size of the returned stream; 2 * sum of frames[f].n_trials */
  int w_ctb, h_ctb;
  int8_t* map;                                                 /* the final map, n_frames * h_ctb * w_ctb (malloc'd, rbt_free): rbt_transcode_gof_qp_map returns the same stream for it */
  rbt_patch_d1_frame* frames;                                  /* n_frames (malloc'd, rbt_free) */
  rbt_patch_d1_pick* picks;                                    /* every frame's picks back to back (malloc'd, rbt_free) */
  double cloud_ms;                                             /* as rbt_d1_floor_result.cloud_ms, the per-patch kernels included */
} rbt_patch_d1_result;
int rbt_submit_gof_d1_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_d1_target* targets, rbt_job** job);
int rbt_wait_gof_d1_patches(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_patch_d1_result* results);   /* results: n entries */
int rbt_transcode_gof_d1_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_d1_target* targets,
                                 uint8_t** annexb_out, size_t* n_out, rbt_patch_d1_result* results);   /* submit + wait */

/* ---- normal estimation (csrc/rbt_normals.h) ----
 * D2 needs normals on the source. Where a sequence comes without them, the reference's PccAppNormalGenerator makes them (PCCNormalsGenerator.cpp: a kd-tree query of the
 * 16 nearest neighbours, a covariance matrix and a 3 x 3 eigen-decomposition per point, on the CPU). This is that stage on the index of a device cloud.
 * Normals are computed on the merged cloud - one point per occupied voxel, as D1, D2 and colour see the cloud - and every point of a voxel receives its voxel's normal.
 * For a voxel p:
 *  1. Neighbours. N(p) = the min(k, number of occupied voxels) occupied voxels nearest to p, p itself included at distance 0 (the reference's query returns the query
 *     point too), in the order (squared integer distance, voxel id ascending), voxel id = z << 20 | y << 10 | x. The reference depends on the order in which nanoflann
 *     returns equidistant points; this rule is defined instead, in the spirit of the tie rules of rbt_d2 and rbt_transfer_colors. It uses the voxel id, not the point index:
 *     the result does not depend on the order of the points, and for a cloud without duplicates the neighbour set is always one the reference could have produced. The
 *     search is exact for any cloud inside 0..1023: no bounded radius, no refusal; empty space is skipped with the coarse level of the index.
 *  2. Scatter matrix, exact: with m = |N(p)|, S = m * sum(q q^T) - sum(q) sum(q)^T over q in N(p): a symmetric 3 x 3 integer matrix, |entry| < 2^31 for m <= 32 and
 *     coordinates <= 1023, and a positive multiple of the reference's covariance (PCCNormalsGenerator.cpp:84-101), so the eigenvectors are the same. It becomes double
 *     only after the integer sums.
 *  3. Eigenvector: the Jacobi iteration of PCCDiagonalize (PCCMath.h:505) restated in double - at most 24 rotations, pivot = the largest off-diagonal magnitude with the
 *     reference's comparison order, stop when the pivot is exactly 0 or the rotation's cosine exactly 1 - then the reference's column choice on |D_ii|
 *     (PCCNormalsGenerator.cpp:105-145): column 0 if strictly smallest, else column 1 if D11 < D22, else column 2. Restating the iteration, where another solver would do
 *     for regular neighbourhoods, makes degenerate ones fall where the reference's fall: an isotropic S gives (0, 0, 1). Only + - * /, fabs and sqrt, each rounded on its
 *     own (no contraction, no trigonometric call): the GPU and the serial host emulation return the same bits. m <= 1 gives the zero vector (:77, :83).
 *  4. Orientation. RBT_NORMALS_ORIENT_VIEW_POINT (the default; default view point (0, 0, 0)): the normal is negated when normal . (view_point - p) < 0, evaluated in
 *     double as :147 does. RBT_NORMALS_ORIENT_NONE: the eigenvector as computed. The reference's spanning-tree and cube-map strategies and its normal smoothing are serial
 *     priority-queue walks; they are not built (RBT_ERR_UNSUPPORTED). D2 squares the projection on the normal, so the sign does not enter it directly. The normals handed to
 *     the decoded cloud, however, are sums of source normals: opposite signs at the silhouette seen from the view point do matter there. That is what the view-point rule
 *     gives and what the spanning tree would improve.
 *  5. Output: Q14 per component, round(16384 * n) half away from zero, int16_t. */
enum { RBT_NORMALS_ORIENT_NONE = 0, RBT_NORMALS_ORIENT_SPANNING_TREE = 1, RBT_NORMALS_ORIENT_VIEW_POINT = 2, RBT_NORMALS_ORIENT_CUBEMAP = 3 };
typedef struct {
  uint32_t struct_size;                  /* sizeof(rbt_normals_params): checked, so that a later field is told from a caller built against this layout */
  int k;                                 /* neighbours, the point itself included: 0 = 16 (the reference's default), else 3..32 */
  int orientation;                       /* RBT_NORMALS_ORIENT_* */
  int32_t view_point[3];
} rbt_normals_params;
/* Gives a device cloud its normals - one from rbt_pcloud_from_maps too - in place of any it was uploaded with; the cloud then allows the D2 part of rbt_score as a source.
 * The normals stay on the device; normals_q14 (3 per point, in point order; may be NULL) receives a copy. p == NULL: all defaults. *device_ms (may be NULL): device time
 * between events around the estimation's kernels; index building, clears and read-back are outside, as for rbt_frame_score.device_ms.
 * k outside {0, 3..32}, an unknown orientation, a wrong struct_size or a handle of another context: RBT_ERR_PARAM; orientation 1 or 3: RBT_ERR_UNSUPPORTED. A refused call
 * leaves the cloud, and the normals it had, untouched. */
int rbt_pcloud_estimate_normals(rbt_ctx* ctx, rbt_pcloud* cloud, const rbt_normals_params* p, int16_t* normals_q14, double* device_ms);
/* The same stage for host arrays: upload, index, estimate, release. Limits and error codes of rbt_pcloud_upload, and the above. */
int rbt_estimate_normals(rbt_ctx* ctx, const int16_t* xyz, int n, const rbt_normals_params* p, int16_t* normals_q14);

/* ---- D2 floors: on the stream and held patch by patch (csrc/rbt_score.h, host/rbt_patch_walk.h) ----
 * The common test conditions report D1 and D2. These two job kinds are the D1 kinds ("transcoding geometry to a D1 floor", "D1 floors held patch by patch") with the D2
 * figure: one more figure on the same cloud path, the same walks, the same rounds.
 *
 * On the stream (rbt_submit_gof_d2 / rbt_wait_gof_d2 / rbt_transcode_gof_d2). Rules 1 - 7 of "transcoding geometry to a D1 floor" hold word for word with
 * D_f(q) = (double)rbt_score(A_f, B_f(q), peak, RBT_SCORE_D2).d2.psnr. Reference: a given handle must carry normals (uploaded with them, or given them through
 * rbt_pcloud_estimate_normals), else RBT_ERR_PARAM at submit; a NULL handle is the cloud of the decoded input, which receives normals once per job through the estimation
 * of rbt_pcloud_estimate_normals with target.normals (struct_size 0 = all defaults; else checked as that call checks it) and keeps them for the job. The returned stream is
 * byte for byte rbt_transcode_gof's at q*. min_d2_mdb 0: coded at params[i].qp, D2 reported. stat takes RBT_D2_MIN / RBT_D2_MEAN. Refusals are the D1 kind's, with its
 * words, plus a reference without normals and a bad normals record. cloud_ms includes the estimation.
 *
 * Patch by patch (rbt_submit_gof_d2_patches / rbt_wait_gof_d2_patches / rbt_transcode_gof_d2_patches). Rules 1 - 5 of "D1 floors held patch by patch" hold with the figure
 * (double)psnr[k] of rbt_score_patches_d2 on (A_f, B_f(trial map)); patch_walk_seed and patch_walk_step are unchanged. The stream is byte for byte
 * rbt_transcode_gof_qp_map's for the final map, no further encode runs, and the result names the patch that sets a frame's D2 as the D1 kind does. The reference rule is
 * the one above.
 * A job is collected only by the wait call of its kind; a wrong pairing is RBT_ERR_PARAM and leaves the job collectable.
 * Not built: D2 floors per frame through the QP list (rbt_submit_gof_d1_frames has no D2 sibling), a D2 floor together with
 * another kind of target in one job, and container-level calls - the library does not parse the atlas sub-bitstream. */
enum { RBT_D2_MIN = RBT_D1_MIN, RBT_D2_MEAN = RBT_D1_MEAN };
typedef struct {
  uint32_t struct_size;                  /* sizeof(rbt_d2_target): checked */
  int32_t  min_d2_mdb;                   /* floor on D, 1/1000 dB; 0 = none: coded at params[i].qp, D2 reported */
  int      stat;                         /* RBT_D2_MIN (the default) or RBT_D2_MEAN */
  int      peak;                         /* 0 = 1023 */
  int      qp_min, qp_max;               /* the walk's range; qp_max 0 = 51 */
  int      n_frames;                     /* point-cloud frames of the entry; 0 in an empty target */
  rbt_atlas_params atlas;                /* the OUTPUT atlas, as in rbt_d1_target */
  const rbt_patch* const* patches;       /* n_frames lists ... */
  const int* n_patches;                  /* ... and their lengths; copied at submit */
  const rbt_pcloud* const* reference;    /* NULL, or n_frames handles: A_f with normals; a NULL handle = the cloud of the decoded input with estimated normals */
  rbt_normals_params normals;            /* for the clouds of the decoded input; struct_size 0 = all defaults */
} rbt_d2_target;
typedef struct {
  int qp, qp_probe, qp_start, met, n_encodes;   /* q*, q0, qs, met, distinct QPs encoded */
  uint64_t bytes;                               /* size of the returned stream */
  double mean_d2, min_d2;                       /* over the frames at q*: the sum of (double)psnr in frame order / n_frames, and the minimum */
  int n_frames;                                 /* 0 for an entry without a target */
  rbt_d2_result* frames;                        /* n_frames results at q* (malloc'd, rbt_free; NULL for an entry without a target) */
  double cloud_ms;                              /* as rbt_d1_floor_result.cloud_ms, the normal estimation of the reference clouds included */
} rbt_d2_floor_result;
int rbt_submit_gof_d2(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_d2_target* targets, rbt_job** job);
int rbt_wait_gof_d2(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_d2_floor_result* results);   /* results: n entries */
int rbt_transcode_gof_d2(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_d2_target* targets,
                         uint8_t** annexb_out, size_t* n_out, rbt_d2_floor_result* results);   /* submit + wait */
typedef struct {
  uint32_t struct_size;                                        /* sizeof(rbt_patch_d2_target): checked */
  int32_t  min_d2_mdb;  int peak;  int qp_min, qp_max;         /* as rbt_patch_d1_target */
  int      background_qp;                                      /* 0..51, -1 = q0 */
  int      max_trials;                                         /* 0 = no cap */
  rbt_atlas_params atlas;                                      /* the OUTPUT atlas */
  int n_frames;  const rbt_patch* const* patches;  const int* n_patches;
  const int32_t* const* patch_min_d2_mdb;                      /* NULL, or per frame NULL / one floor per patch: F_k; else F_k = min_d2_mdb */
  const rbt_pcloud* const* reference;                          /* as in rbt_d2_target */
  rbt_normals_params normals;                                  /* as in rbt_d2_target */
} rbt_patch_d2_target;
typedef struct { int qp, met, failed; rbt_patch_d2 d2; double figure; } rbt_patch_d2_pick;   /* of the settling trial: q[k], met, failed[k], the patch's sums and figures, (double)d2.psnr */
typedef struct {
  int n_trials, met, n_patches;                                /* met = AND of patches[k].met */
  uint64_t bytes;                                              /* the frame's NAL units in the returned stream, start codes included */
  rbt_d2_result d2;                                            /* the whole frame's D2 in the settling trial: rbt_score(A_f, B_f, peak, RBT_SCORE_D2).d2 */
  rbt_patch_d2_pick* patches;                                  /* n_patches picks: they point into rbt_patch_d2_result.picks */
} rbt_patch_d2_frame;
typedef struct {
  int n_frames, qp_probe, met_all, n_passes;                   /* q0; met_all = AND of frames[f].met */
  uint64_t bytes, pictures_encoded;                            /* size of the returned stream; 2 * sum of frames[f].n_trials */
  int w_ctb, h_ctb;
  int8_t* map;                                                 /* the final map, n_frames * h_ctb * w_ctb (malloc'd, rbt_free) */
  rbt_patch_d2_frame* frames;                                  /* n_frames (malloc'd, rbt_free) */
  rbt_patch_d2_pick* picks;                                    /* every frame's picks back to back (malloc'd, rbt_free) */
  double cloud_ms;                                             /* as rbt_d2_floor_result.cloud_ms, the per-patch kernels included */
} rbt_patch_d2_result;
int rbt_submit_gof_d2_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_d2_target* targets, rbt_job** job);
int rbt_wait_gof_d2_patches(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_patch_d2_result* results);   /* results: n entries */
int rbt_transcode_gof_d2_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_d2_target* targets,
                                 uint8_t** annexb_out, size_t* n_out, rbt_patch_d2_result* results);   /* submit + wait */

/* ---- colour floors held patch by patch (csrc/rbt_score.h, host/rbt_patch_walk.h) ----
 * The attribute sub-bitstream is where the bytes are, and the QP map codes attribute entries; the PSNR floor per patch on such an entry steers by the luma PSNR of the
 * map, a proxy for what the common test conditions report. Here every patch of every frame of an attribute entry walks to its own QP on the colour PSNR of its points in
 * the decoded cloud ("colour PSNR per patch of the decoded cloud" above): one more figure on the patch walk, over the colour job's "cloud once, recolour per trial" route.
 *
 * 1. Sources, shapes, cloud, reference. Rules 1 - 4 of "transcoding attributes to a colour PSNR floor" hold: the target sits on an attribute entry; its geometry source is
 *    coded once at its own params[i].qp, byte for byte as rbt_transcode_gof codes it, occupancy_rd included. atlas.map_count must be 2: a point-cloud frame is the two
 *    pictures that are coded as a pair. B_f(trial map) is rule 3's cloud with the attribute pictures coded under the trial's QP map; it carries the labels of
 *    rbt_pcloud_from_maps. Everything of B_f that does not depend on the attribute QP - positions, smoothing, index, labels, the score pair against A_f - is made once per
 *    job and frame behind the geometry encode.
 * 2. Figure. The figure of patch k of frame f in a trial is (double)psnr[channel] of patch k from rbt_score_pair_patches_color on the frame's pair. meets is
 *    figure >= F_k / 1000.0; +inf meets.
 * 3. Trial map, walk, rounds, stream: rules 4 - 7 of "PSNR floors held patch by patch", word for word, with this figure (patch_walk_seed / patch_walk_step unchanged). A
 *    round is one pass over the unsettled frames with their trial maps; behind it exactly those frames are gathered, up-converted, recoloured and scored per patch. The
 *    attribute entry's stream is byte for byte rbt_transcode_gof_qp_map's for the final map, assembled from the settling trials; no further encode runs.
 * 4. Floor 0. With min_psnr_mdb 0 and patch_min_psnr_mdb NULL there is one trial at clamp(params[i].qp, 0, 51): every patch's rbt_patch_color is reported and met = 1.
 * 5. Everything is copied at submit. A job is collected by rbt_wait_gof_color_patches only; a wrong pairing is RBT_ERR_PARAM and leaves the job collectable. Refusals, all
 *    RBT_ERR_PARAM with a reason, nothing submitted, the context usable: those of the colour section (rule 7 there, with its words) and those of the patch-floor section
 *    (rule 9 there: a wrong struct_size, an odd picture count, n_frames that is not pictures / 2, an atlas size that is not the output pictures', a background_qp outside
 *    -1..51, a negative max_trials, a negative patch floor, log2_ctb outside 4..6); a target on a non-attribute entry; map_count other than 2. An empty cloud, a coordinate
 *    outside 0..1023 or more than 2^21 merged points fail the job in its wait call, as in the colour section. An entry without a target (every field but struct_size
 *    zero) is coded at params[i].qp: n_frames 0, map, frames and picks NULL.
 * Memory is the colour section's plus 4 bytes per point of labels and 64 bytes per patch of sums.
 * Not built: colour floors per frame through the QP list, byte caps per patch, two kinds of floor in one job, a caller's map together with a target, and a
 * container-level call - the library does not parse the atlas sub-bitstream. */
typedef struct {
  uint32_t struct_size;                                        /* sizeof(rbt_patch_color_target): checked */
  int32_t  min_psnr_mdb;  int channel;  int qp_min, qp_max;    /* floor in 1/1000 dB (0 = none) on the symmetric colour PSNR of channel 0 Y, 1 U, 2 V; qp_max 0 = 51 */
  int      background_qp;                                      /* 0..51, -1 = q0 */
  int      max_trials;                                         /* 0 = no cap */
  rbt_atlas_params atlas;                                      /* the OUTPUT atlas, as in rbt_color_target */
  int n_frames;  const rbt_patch* const* patches;  const int* n_patches;
  const int32_t* const* patch_min_psnr_mdb;                    /* NULL, or per frame NULL / one floor per patch: F_k; else F_k = min_psnr_mdb */
  int      upsample_filter, attr_transfer;                     /* as in rbt_color_target */
  const rbt_pcloud* const* reference;                          /* NULL, or n_frames handles with colours: A_f; a NULL handle = the cloud of the decoded input */
} rbt_patch_color_target;
typedef struct { int qp, met, failed; rbt_patch_color color; double figure; } rbt_patch_color_pick;   /* of the settling trial: q[k], met, failed[k], the patch's sums and figures, (double)color.psnr[channel] */
typedef struct {
  int n_trials, met, n_patches;                                /* met = AND of patches[k].met */
  uint64_t bytes;                                              /* the frame's NAL units in the returned stream, start codes included */
  rbt_color_result color;                                      /* the whole frame's colour result in the settling trial: rbt_score(A_f, B_f, peak, RBT_SCORE_COLOR).color */
  rbt_patch_color_pick* patches;                               /* n_patches picks: they point into rbt_patch_color_result.picks */
} rbt_patch_color_frame;
typedef struct {
  int n_frames, qp_probe, met_all, n_passes;                   /* q0; met_all = AND of frames[f].met */
  uint64_t bytes, pictures_encoded;                            /* size of the returned stream; 2 * sum of frames[f].n_trials */
  int w_ctb, h_ctb;
  int8_t* map;                                                 /* the final map, n_frames * h_ctb * w_ctb (malloc'd, rbt_free) */
  rbt_patch_color_frame* frames;                               /* n_frames (malloc'd, rbt_free) */
  rbt_patch_color_pick* picks;                                 /* every frame's picks back to back (malloc'd, rbt_free) */
  double cloud_ms;                                             /* as rbt_color_floor_result.cloud_ms, the per-patch kernel included */
} rbt_patch_color_result;
int rbt_submit_gof_color_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_color_target* targets, rbt_job** job);
int rbt_wait_gof_color_patches(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_patch_color_result* results);   /* results: n entries */
int rbt_transcode_gof_color_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_color_target* targets,
                                    uint8_t** annexb_out, size_t* n_out, rbt_patch_color_result* results);   /* submit + wait */

#ifdef __cplusplus
}
#endif
#endif
