// C ABI of librbt.so (include/rbt.h). Drop-in for PCCTranscoder::transcodeVideo (PCCTranscoder.cpp:374-546).
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>
#include "rbt_batch.h"
#include "rbt_transcode.h"
#include "rbt_pcc.h"
#include "rbt_internal.h"
#include "rbt_qp_map.h"

struct rbt_pcloud { rbt::PCloud* cloud; rbt_ctx* owner; };
struct rbt_score_pair { rbt::ScorePair* pair; rbt_ctx* owner; bool stale; };      // stale: one of its clouds has been released
struct rbt_ctx { int device, rank, world; rbt_stats stats; std::string last_err; double color_ms[4] = {0, 0, 0, 0}; int n_changed = 0; int n_flat = 0;
                 std::vector<rbt_pcloud*> clouds; std::vector<rbt_score_pair*> pairs; rbt::PCloudCache cloud_cache; };      // handles outstanding; clean volumes of released clouds
struct rbt_job { rbt::GofJob* j; rbt_ctx* owner; };

// Job slots, pipeline depth and the lock are per DEVICE (the 16 HIP streams a job's lanes map onto are the device's, rbt_kernels.hip):
// contexts on different devices run concurrently, contexts on one device share its slots and are serialised, as are the calls on one
// context (the reference's transcoder is called serially too).
struct DevState { rbt_job* jobs[RBT_MAX_JOBS] = {}; int depth = 4; std::mutex mu; };
static DevState g_dev[16];
static_assert(RBT_MAX_JOBS == rbtk::RBT_JOB_SLOTS, "job slots");
// every context entry point starts with an empty error text (rbt_last_error describes the LAST call; the pointer it returns is valid until the next call on the context)
#define RBT_ENTER(ctx) DevState& D = g_dev[(ctx)->device]; std::lock_guard<std::mutex> lk(D.mu); (ctx)->last_err.clear(); if (rbtk::dev_select((ctx)->device)) return RBT_ERR_NO_DEVICE
// no exception crosses the C ABI: allocation failures of the host side (std::vector, std::string) come back as error codes
#define RBT_CATCH catch (const std::bad_alloc&) { return RBT_ERR_NOMEM; } catch (...) { return RBT_ERR_NO_DEVICE; }

// What the checks of a D1 target and of a colour target end with: the QP range, the frames, their patch lists, and the reference handles, which must be clouds of this
// context (colours: with colours); refs: the handles as clouds, nullptr = none
template <class Target> static int check_cloud_target(rbt_ctx* ctx, const std::string& who, const Target& t, bool colours, std::vector<const rbt::PCloud*>& refs) {
  std::string& err = ctx->last_err;
  const int lo = t.qp_min, hi = t.qp_max ? t.qp_max : 51;
  if (lo < 0 || hi > 51 || lo > hi) { err = who + "the QP range must satisfy 0 <= qp_min <= qp_max <= 51 (qp_max 0 = 51)"; return RBT_ERR_PARAM; }
  if (t.n_frames < 1) { err = who + "n_frames must be at least 1"; return RBT_ERR_PARAM; }
  if (!t.patches || !t.n_patches) { err = who + "the patch lists are missing"; return RBT_ERR_PARAM; }
  for (int f = 0; f < t.n_frames; f++) {
    if (t.n_patches[f] < 0 || (!t.patches[f] && t.n_patches[f])) { err = who + "the patch list of frame " + std::to_string(f) + " is missing"; return RBT_ERR_PARAM; }
    std::string why;
    if (rbt::mapframe_check(why, &t.atlas, t.patches[f], t.n_patches[f])) { err = who + "frame " + std::to_string(f) + ": " + why; return RBT_ERR_PARAM; }
    const rbt_pcloud* h = t.reference ? t.reference[f] : nullptr;
    if (h) {
      bool mine = false; for (const rbt_pcloud* c : ctx->clouds) mine |= c == h;
      if (!mine) { err = who + "reference " + std::to_string(f) + " is not a cloud of this context"; return RBT_ERR_PARAM; }
      if (colours && !rbt::pcloud_has_colors(h->cloud)) { err = who + "reference " + std::to_string(f) + " carries no colours"; return RBT_ERR_PARAM; }
    }
    refs.push_back(h ? h->cloud : nullptr);
  }
  return RBT_OK;
}

// Floors held patch by patch: the refusals the two kinds of target share (Target: rbt_patch_floor_target / rbt_patch_d1_target, floors: its floors per patch), behind those of
// the kind's own fields; o: the request the walks read, with the patch lists and the floors F_k copied - floor_mdb where a patch has none of its own
template <class Target> static int fill_patch_request(std::string& err, const std::string& who, const rbt_stream_params& p, const Target& t, int32_t floor_mdb, int region, const int32_t* const* floors,
                                                      rbt::PatchFloorIn& o) {
  const int lo = t.qp_min, hi = t.qp_max ? t.qp_max : 51;
  if (lo < 0 || hi > 51 || lo > hi) { err = who + "the QP range must satisfy 0 <= qp_min <= qp_max <= 51 (qp_max 0 = 51)"; return RBT_ERR_PARAM; }
  if (t.background_qp < -1 || t.background_qp > 51) { err = who + "background_qp is outside -1..51 (-1 = the probe's QP)"; return RBT_ERR_PARAM; }
  if (t.max_trials < 0) { err = who + "max_trials must not be negative (0 = no cap)"; return RBT_ERR_PARAM; }
  if (t.n_frames < 1 || !t.patches || !t.n_patches) { err = who + "a patch target needs n_frames = pictures / 2 with a patch list and a count per frame"; return RBT_ERR_PARAM; }
  if (t.atlas.width < 1 || t.atlas.height < 1 || t.atlas.occupancy_resolution < 1) { err = who + "the atlas needs a size and an occupancy_resolution"; return RBT_ERR_PARAM; }
  if (p.log2_ctb && (p.log2_ctb < 4 || p.log2_ctb > 6)) { err = who + "log2_ctb must be 4..6"; return RBT_ERR_PARAM; }
  for (int f = 0; f < t.n_frames; f++) {
    const int np = t.n_patches[f];
    if (np < 0 || (np > 0 && !t.patches[f])) { err = who + "frame " + std::to_string(f) + " has a patch count without a list"; return RBT_ERR_PARAM; }
    o.patches.emplace_back(np ? t.patches[f] : nullptr, np ? t.patches[f] + np : nullptr);
    const int32_t* fl = floors ? floors[f] : nullptr;
    o.floors.emplace_back((size_t)np, floor_mdb);
    for (int k = 0; k < np && fl; k++) { if (fl[k] < 0) { err = who + "the floor of patch " + std::to_string(k) + " of frame " + std::to_string(f) + " is negative"; return RBT_ERR_PARAM; } o.floors.back()[(size_t)k] = fl[k]; }
  }
  o.floor_mdb = floor_mdb; o.region = region; o.qp_min = t.qp_min; o.qp_max = t.qp_max; o.background_qp = t.background_qp; o.max_trials = t.max_trials;
  o.atlas_width = t.atlas.width; o.atlas_height = t.atlas.height; o.occupancy_resolution = t.atlas.occupancy_resolution; o.n_frames = t.n_frames;
  return RBT_OK;
}
// submit + wait, what every rbt_transcode_gof_* with targets and results is: the two named halves of its kind, one behind the other
template <class Target, class Result>
static int transcode(int (*submit_kind)(rbt_ctx*, int, const uint8_t* const*, const size_t*, const rbt_stream_params*, const Target*, rbt_job**), int (*wait_kind)(rbt_ctx*, rbt_job*, uint8_t**, size_t*, Result*),
                     rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const Target* targets, uint8_t** annexb_out, size_t* n_out, Result* results) {
  if (!annexb_out || !n_out || !results) return RBT_ERR_PARAM;
  rbt_job* job = nullptr;
  if (int rc = submit_kind(ctx, n, annexb_in, n_in, p, targets, &job)) return rc;
  return wait_kind(ctx, job, annexb_out, n_out, results);
}

extern "C" {

const char* rbt_version(void) { return "rabbit-transcoding_amd 0.1 (RBT-E1 encoder, gfx950)"; }

const char* rbt_last_error(rbt_ctx* ctx) { return ctx ? ctx->last_err.c_str() : ""; }
void rbt_internal_set_error(rbt_ctx* ctx, const char* text) { if (ctx) { try { ctx->last_err = text ? text : ""; } catch (...) {} } }
const char* rbt_strerror(int code) {
  switch (code) {
    case RBT_OK: return "ok";
    case RBT_ERR_NO_DEVICE: return "no usable HIP device or HIP runtime failure (this library has no CPU fallback)";
    case RBT_ERR_BITSTREAM: return "corrupt or truncated HEVC bitstream";
    case RBT_ERR_UNSUPPORTED: return "bitstream uses a coding tool outside the supported V-PCC CTC toolset";
    case RBT_ERR_PARAM: return "invalid parameter";
    case RBT_ERR_NOMEM: return "out of memory";
    case RBT_ERR_MD5: return "decoded picture hash mismatch on the input stream";
    case RBT_ERR_BUSY: return "too many transcodes in flight";
    case RBT_ERR_OUTPUT: return "coded data exceeds the output buffer sized for it";
    default: return "unknown error";
  }
}
void rbt_free(void* p) { free(p); }

int rbt_create(rbt_ctx** ctx, int device, int world_rank, int world_size) try {
  if (!ctx) return RBT_ERR_PARAM;
  *ctx = nullptr;
  if (world_size < 1 || world_rank < 0 || world_rank >= world_size) return RBT_ERR_PARAM;
  if (device < 0 || device >= 16) return RBT_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(g_dev[device].mu);
  if (rbtk::dev_init(device)) return RBT_ERR_NO_DEVICE;
  rbt_ctx* c = new rbt_ctx(); c->device = device; c->rank = world_rank; c->world = world_size; memset(&c->stats, 0, sizeof(c->stats));
  *ctx = c;
  return RBT_OK;
} RBT_CATCH
void rbt_destroy(rbt_ctx* ctx) {
  if (ctx) {
    DevState& D = g_dev[ctx->device]; std::lock_guard<std::mutex> lk(D.mu);
    if (!rbtk::dev_select(ctx->device)) {
      for (int s = 0; s < RBT_MAX_JOBS; s++) if (D.jobs[s] && D.jobs[s]->owner == ctx) { rbt::gof_abandon(D.jobs[s]->j); delete D.jobs[s]; D.jobs[s] = nullptr; }
      for (rbt_score_pair* h : ctx->pairs) { rbt::score_pair_release(h->pair); delete h; }
      ctx->pairs.clear();
      for (rbt_pcloud* h : ctx->clouds) { rbt::pcloud_release(ctx->cloud_cache, h->cloud); delete h; }
      ctx->clouds.clear(); rbt::pcloud_cache_trim(ctx->cloud_cache);
      rbtk::dev_release_pool();
    }
  }
  delete ctx;
}
// GOF sharding rule of the multi-GPU transcoder: GOF g of a sequence belongs to rank g mod world_size. A host that
// walks the sequence GOF by GOF (PccAppTranscoder.cpp:307-341) on every rank skips the GOFs its context does not own.
int rbt_owns_gof(const rbt_ctx* ctx, int gof_index) { return ctx && gof_index >= 0 && gof_index % ctx->world == ctx->rank; }
int rbt_world(const rbt_ctx* ctx, int* rank, int* size) { if (!ctx) return RBT_ERR_PARAM; if (rank) *rank = ctx->rank; if (size) *size = ctx->world; return RBT_OK; }
int rbt_flat_pictures(const rbt_ctx* ctx) { return ctx ? ctx->n_flat : 0; }
int rbt_get_stats(rbt_ctx* ctx, rbt_stats* out) { if (!ctx || !out) return RBT_ERR_PARAM; *out = ctx->stats; return RBT_OK; }

int rbt_decode(rbt_ctx* ctx, const uint8_t* annexb, size_t n, int verify_md5, rbt_video* out) try {
  if (!ctx || !annexb || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  memset(out, 0, sizeof(*out));
  rbt::DecodeBatch b; rbt::StreamIn in{annexb, n};
  int rc = rbt::decode_build(b, &in, 1);
  if (!rc && verify_md5) rc = rbt::decode_hash_setup(b, std::vector<char>(1, 1));   // the pictures' hashes on the GPU, behind the decoder's last filter
  if (!rc) rc = rbt::decode_run(b);
  if (!rc && !b.hash.empty()) { rbt::decode_launch_hash(b); if (b.hash.fetch()) { b.err = "device transfer failed"; rc = RBT_ERR_NO_DEVICE; } }
  if (!rc) rc = rbt::decode_fetch(b, 0, out);
  if (!rc && verify_md5) rbt::decode_hash_result(b, 0, out->md5_checked, out->md5_failed);
  if (rc) { ctx->last_err = b.err; free(out->data); memset(out, 0, sizeof(*out)); return rc; }
  ctx->n_flat = b.n_flat;
  ctx->stats.k_parse_ms = rbtk::timer_ms(rbt::T_PARSE); ctx->stats.k_recon_ms = rbtk::timer_ms(rbt::T_RECON);
  if (verify_md5 && out->md5_failed) return RBT_ERR_MD5;
  return RBT_OK;
} RBT_CATCH

// PCCVideoBitstream.cpp:174-184
static size_t end_of_nalu(const uint8_t* d, size_t size, size_t start) {
  if (size < start + 4) return size;
  for (size_t i = start; i < size - 4; i++)
    if (d[i] == 0 && d[i + 1] == 0 && (d[i + 2] == 1 || (d[i + 2] == 0 && d[i + 3] == 1))) return i;
  return size;
}
// PCCVideoBitstream::byteStreamToSampleStream (PCCVideoBitstream.cpp:85-112), precision 4, no emulation prevention handling
int rbt_byte_to_sample_stream(const uint8_t* in, size_t n, uint8_t** out, size_t* n_out) try {
  if (!in || !out || !n_out || n < 4) return RBT_ERR_PARAM;
  std::vector<uint8_t> v; v.reserve(n + 64);
  size_t start = 0, end = 0;
  do {
    size_t sc = in[start + 2] == 0 ? 4 : 3;
    end = end_of_nalu(in, n, start + sc);
    size_t sz = end - (start + sc);
    for (int i = 0; i < 4; i++) v.push_back((uint8_t)(sz >> (8 * (3 - i))));
    v.insert(v.end(), in + start + sc, in + end);
    start = end;
  } while (end < n);
  *out = (uint8_t*)malloc(v.size() ? v.size() : 1); if (!*out) return RBT_ERR_NOMEM;
  memcpy(*out, v.data(), v.size()); *n_out = v.size();
  return RBT_OK;
} RBT_CATCH
// PCCVideoBitstream::sampleStreamToByteStream (PCCVideoBitstream.cpp:114-172), HEVC, precision 4
int rbt_sample_to_byte_stream(const uint8_t* in, size_t n, uint8_t** out, size_t* n_out) try {
  if (!in || !out || !n_out || n < 4) return RBT_ERR_PARAM;
  std::vector<uint8_t> v; v.reserve(n + 64);
  size_t sc = 4, start = 0, end = 0;
  do {
    uint32_t sz = 0; for (int i = 0; i < 4; i++) sz = (sz << 8) + in[start + i];
    end = start + 4 + sz;
    if (end > n) return RBT_ERR_BITSTREAM;
    for (size_t i = 0; i + 1 < sc; i++) v.push_back(0);
    v.push_back(1);
    v.insert(v.end(), in + start + 4, in + end);
    start = end;
    if (start + 4 < n) { int type = (in[start + 4] & 126) >> 1; sc = (type >= 32 && type < 41) ? 4 : 3; }   // the reference resets newFrame before testing it (:146)
  } while (end < n);
  *out = (uint8_t*)malloc(v.size() ? v.size() : 1); if (!*out) return RBT_ERR_NOMEM;
  memcpy(*out, v.data(), v.size()); *n_out = v.size();
  return RBT_OK;
} RBT_CATCH

// what a submit adds to the inputs and their parameters: at most one of the target arrays (per_frame: the floors of quality / d1 are held frame by frame), QP lists or QP maps
struct SubmitExtras {
  bool gof_rule = true; const rbt_rate_target* targets = nullptr; const rbt_quality_target* quality = nullptr; const rbt_d1_target* d1 = nullptr; const rbt_color_target* color = nullptr;
  bool per_frame = false; const rbt_frame_qp* lists = nullptr; const rbt_qp_map* maps = nullptr;
  const rbt_patch_floor_target* patches = nullptr;
  const rbt_patch_d1_target* d1_patches = nullptr;
  const rbt_d2_target* d2 = nullptr; const rbt_patch_d2_target* d2_patches = nullptr;      // the D1 kinds with the D2 figure (check_d2, check_d2_patches)
  const rbt_patch_color_target* color_patches = nullptr;
};
static int submit(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, rbt_job** job, const SubmitExtras& x = SubmitExtras());
// transcodeVideo re-encodes whatever it is handed (an occupancy stream with occupancyPrecision != 4 is re-encoded without pooling)
int rbt_transcode_substream(rbt_ctx* ctx, const uint8_t* annexb_in, size_t n_in, const rbt_stream_params* p, uint8_t** annexb_out, size_t* n_out) try {
  if (!ctx || !annexb_in || !p || !annexb_out || !n_out) return RBT_ERR_PARAM;
  rbt_job* job = nullptr;
  SubmitExtras x; x.gof_rule = false;
  int rc = submit(ctx, 1, &annexb_in, &n_in, p, &job, x);
  if (rc) return rc;
  return rbt_wait_gof(ctx, job, annexb_out, n_out);
} RBT_CATCH
int rbt_transcode_gof(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, uint8_t** annexb_out, size_t* n_out) try {
  if (!ctx || n < 1 || n > RBT_MAX_STREAMS || !annexb_in || !n_in || !p || !annexb_out || !n_out) return RBT_ERR_PARAM;
  rbt_job* job = nullptr;
  int rc = rbt_submit_gof(ctx, n, annexb_in, n_in, p, &job);
  if (rc) return rc;
  return rbt_wait_gof(ctx, job, annexb_out, n_out);
} RBT_CATCH
int rbt_submit_gof(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, rbt_job** job) try { return submit(ctx, n, annexb_in, n_in, p, job); } RBT_CATCH
// the refusals of rbt_submit_gof_rate: nothing has been submitted when one of them fires
static int check_targets(std::string& err, int n, const rbt_stream_params* p, const rbt_rate_target* t) {
  for (int i = 0; i < n; i++) {
    const std::string who = "entry " + std::to_string(i) + ": ";
    if (t[i].struct_size != sizeof(rbt_rate_target)) { err = who + "rbt_rate_target.struct_size is not sizeof(rbt_rate_target)"; return RBT_ERR_PARAM; }
    if (!t[i].target_bytes) continue;
    if (p[i].video_type == RBT_VIDEO_OCCUPANCY) { err = who + "an occupancy stream is coded losslessly and takes no rate target"; return RBT_ERR_PARAM; }
    if (p[i].occupancy_rd) { err = who + "a rate target cannot be combined with occupancy_rd"; return RBT_ERR_PARAM; }
    const int lo = t[i].qp_min, hi = t[i].qp_max ? t[i].qp_max : 51;
    if (lo < 0 || hi > 51 || lo > hi) { err = who + "the QP range must satisfy 0 <= qp_min <= qp_max <= 51 (qp_max 0 = 51)"; return RBT_ERR_PARAM; }
  }
  return RBT_OK;
}
// the refusals of rbt_submit_gof_quality that the parameters alone decide (those that need the streams' sizes: gof_refused)
static int check_quality(std::string& err, int n, const rbt_stream_params* p, const rbt_quality_target* t) {
  for (int i = 0; i < n; i++) {
    const std::string who = "entry " + std::to_string(i) + ": ";
    if (t[i].struct_size != sizeof(rbt_quality_target)) { err = who + "rbt_quality_target.struct_size is not sizeof(rbt_quality_target)"; return RBT_ERR_PARAM; }
    if (t[i].min_psnr_mdb < 0) { err = who + "min_psnr_mdb must not be negative"; return RBT_ERR_PARAM; }
    if (t[i].region != RBT_QUALITY_ALL && t[i].region != RBT_QUALITY_OCCUPIED) { err = who + "region must be RBT_QUALITY_ALL or RBT_QUALITY_OCCUPIED"; return RBT_ERR_PARAM; }
    const int lo = t[i].qp_min, hi = t[i].qp_max ? t[i].qp_max : 51;
    if (lo < 0 || hi > 51 || lo > hi) { err = who + "the QP range must satisfy 0 <= qp_min <= qp_max <= 51 (qp_max 0 = 51)"; return RBT_ERR_PARAM; }
    if (t[i].min_psnr_mdb && p[i].video_type == RBT_VIDEO_OCCUPANCY) { err = who + "an occupancy stream is coded losslessly and takes no PSNR floor"; return RBT_ERR_PARAM; }
  }
  return RBT_OK;
}
static int normals_params(std::string& err, const rbt_normals_params* p, int* k, int* orient, int32_t vp[3]);
// the refusals of rbt_submit_gof_d1 that the parameters alone decide (those that need the streams' sizes: gof_refused); req: the reference handles as clouds
static int check_d1(rbt_ctx* ctx, int n, const rbt_stream_params* p, const rbt_d1_target* t, rbt::CloudRequest<rbt_d1_target>& req) {
  std::string& err = ctx->last_err;
  req.targets = t; req.cache = &ctx->cloud_cache; req.refs.assign((size_t)n, {});
  for (int i = 0; i < n; i++) {
    const std::string who = "entry " + std::to_string(i) + ": ";
    if (t[i].struct_size != sizeof(rbt_d1_target)) { err = who + "rbt_d1_target.struct_size is not sizeof(rbt_d1_target)"; return RBT_ERR_PARAM; }
    rbt_d1_target zero; memset(&zero, 0, sizeof(zero)); zero.struct_size = t[i].struct_size;
    const bool empty = !t[i].min_d1_mdb && !t[i].stat && !t[i].peak && !t[i].qp_min && !t[i].qp_max && !t[i].n_frames && !t[i].patches && !t[i].n_patches && !t[i].reference &&
                       !memcmp(&t[i].atlas, &zero.atlas, sizeof(zero.atlas));
    if (empty) continue;
    if (p[i].video_type != RBT_VIDEO_GEOMETRY) { err = who + "a D1 target on a non-geometry entry (the target of an attribute or occupancy entry must be empty)"; return RBT_ERR_PARAM; }
    if (t[i].min_d1_mdb < 0) { err = who + "min_d1_mdb must not be negative"; return RBT_ERR_PARAM; }
    if (t[i].stat != RBT_D1_MIN && t[i].stat != RBT_D1_MEAN) { err = who + "stat must be RBT_D1_MIN or RBT_D1_MEAN"; return RBT_ERR_PARAM; }
    if (t[i].peak < 0) { err = who + "peak must not be negative (0 = 1023)"; return RBT_ERR_PARAM; }
    if (int rc = check_cloud_target(ctx, who, t[i], false, req.refs[(size_t)i])) return rc;
  }
  return RBT_OK;
}
// the refusals of rbt_submit_gof_color that the parameters alone decide, as check_d1
static int check_color(rbt_ctx* ctx, int n, const rbt_stream_params* p, const rbt_color_target* t, rbt::CloudRequest<rbt_color_target>& req) {
  std::string& err = ctx->last_err;
  req.targets = t; req.cache = &ctx->cloud_cache; req.refs.assign((size_t)n, {});
  for (int i = 0; i < n; i++) {
    const std::string who = "entry " + std::to_string(i) + ": ";
    if (t[i].struct_size != sizeof(rbt_color_target)) { err = who + "rbt_color_target.struct_size is not sizeof(rbt_color_target)"; return RBT_ERR_PARAM; }
    rbt_color_target zero; memset(&zero, 0, sizeof(zero));
    const bool empty = !t[i].min_psnr_mdb && !t[i].channel && !t[i].stat && !t[i].qp_min && !t[i].qp_max && !t[i].n_frames && !t[i].patches && !t[i].n_patches && !t[i].upsample_filter &&
                       !t[i].attr_transfer && !t[i].reference && !memcmp(&t[i].atlas, &zero.atlas, sizeof(zero.atlas));
    if (empty) continue;
    if (p[i].video_type != RBT_VIDEO_ATTRIBUTE) { err = who + "a colour target on a non-attribute entry (the target of a geometry or occupancy entry must be empty)"; return RBT_ERR_PARAM; }
    if (t[i].min_psnr_mdb < 0) { err = who + "min_psnr_mdb must not be negative"; return RBT_ERR_PARAM; }
    if (t[i].channel < 0 || t[i].channel > 2) { err = who + "channel must be 0 (Y), 1 (U) or 2 (V)"; return RBT_ERR_PARAM; }
    if (t[i].stat != RBT_D1_MIN && t[i].stat != RBT_D1_MEAN) { err = who + "stat must be RBT_D1_MIN or RBT_D1_MEAN"; return RBT_ERR_PARAM; }
    if (t[i].upsample_filter != RBT_UPSAMPLE_F0 && t[i].upsample_filter != RBT_UPSAMPLE_REPLICATE) { err = who + "upsample_filter must be RBT_UPSAMPLE_F0 or RBT_UPSAMPLE_REPLICATE"; return RBT_ERR_PARAM; }
    if (t[i].attr_transfer != 0 && t[i].attr_transfer != 1) { err = who + "attr_transfer must be 0 or 1"; return RBT_ERR_PARAM; }
    if (int rc = check_cloud_target(ctx, who, t[i], true, req.refs[(size_t)i])) return rc;
  }
  return RBT_OK;
}
// the refusals of rbt_submit_gof_frame_qp that the parameters alone decide (the count against the stream's pictures: gof_refused); out: the lists, copied
static int check_frame_qp(std::string& err, int n, const rbt_stream_params* p, const rbt_frame_qp* l, std::vector<std::vector<int8_t>>& out) {
  out.assign((size_t)n, {});
  for (int i = 0; i < n; i++) {
    const std::string who = "entry " + std::to_string(i) + ": ";
    if (l[i].struct_size != sizeof(rbt_frame_qp)) { err = who + "rbt_frame_qp.struct_size is not sizeof(rbt_frame_qp)"; return RBT_ERR_PARAM; }
    if (!l[i].n_frames && !l[i].qp) continue;
    if (l[i].n_frames < 1 || !l[i].qp) { err = who + "rbt_frame_qp.n_frames must be pictures / 2 with a list of that many QPs (n_frames 0 and qp NULL: no list)"; return RBT_ERR_PARAM; }
    if (p[i].video_type == RBT_VIDEO_OCCUPANCY) { err = who + "an occupancy stream is coded losslessly and takes no QP list"; return RBT_ERR_PARAM; }
    for (int f = 0; f < l[i].n_frames; f++) if (l[i].qp[f] < 0 || l[i].qp[f] > 51) { err = who + "the QP of frame " + std::to_string(f) + " is outside 0..51"; return RBT_ERR_PARAM; }
    out[(size_t)i].assign(l[i].qp, l[i].qp + l[i].n_frames);
  }
  return RBT_OK;
}
// the refusals of rbt_submit_gof_qp_map that the parameters alone decide (the counts against the stream's pictures: gof_refused); out: the maps, copied
static int check_qp_maps(std::string& err, int n, const rbt_stream_params* p, const rbt_qp_map* m, std::vector<rbt::QpMapIn>& out) {
  out.assign((size_t)n, {});
  for (int i = 0; i < n; i++) {
    const std::string who = "entry " + std::to_string(i) + ": ";
    if (m[i].struct_size != sizeof(rbt_qp_map)) { err = who + "rbt_qp_map.struct_size is not sizeof(rbt_qp_map)"; return RBT_ERR_PARAM; }
    if (!m[i].n_frames && !m[i].w_ctb && !m[i].h_ctb && !m[i].qp) continue;
    if (!m[i].qp) { err = who + "rbt_qp_map carries counts without a map (n_frames, w_ctb and h_ctb 0 with qp NULL: no map)"; return RBT_ERR_PARAM; }
    if (m[i].n_frames < 1 || m[i].w_ctb < 1 || m[i].h_ctb < 1) { err = who + "rbt_qp_map carries a map without its counts: n_frames must be pictures / 2, w_ctb and h_ctb the CTB columns and rows of the output pictures"; return RBT_ERR_PARAM; }
    if (p[i].video_type == RBT_VIDEO_OCCUPANCY) { err = who + "an occupancy stream is coded losslessly and takes no QP map"; return RBT_ERR_PARAM; }
    if (m[i].w_ctb > 8192 / 16 || m[i].h_ctb > 8192 / 16) { err = who + "rbt_qp_map.w_ctb x h_ctb is beyond any picture (8192 samples at most)"; return RBT_ERR_PARAM; }
    const size_t cnt = (size_t)m[i].n_frames * m[i].w_ctb * m[i].h_ctb;
    for (size_t k = 0; k < cnt; k++) if (m[i].qp[k] < 0 || m[i].qp[k] > 51) {
      const size_t per = (size_t)m[i].w_ctb * m[i].h_ctb;
      err = who + "the QP of frame " + std::to_string(k / per) + ", CTB row " + std::to_string(k % per / m[i].w_ctb) + ", column " + std::to_string(k % m[i].w_ctb) + " is outside 0..51"; return RBT_ERR_PARAM; }
    out[(size_t)i].qp.assign(m[i].qp, m[i].qp + cnt); out[(size_t)i].n_frames = m[i].n_frames; out[(size_t)i].w_ctb = m[i].w_ctb; out[(size_t)i].h_ctb = m[i].h_ctb;
  }
  return RBT_OK;
}
// the refusals of rbt_submit_gof_quality_patches that the parameters alone decide (the counts and the atlas against the stream's pictures: gof_refused); out: the requests
static int check_patch_floors(std::string& err, int n, const rbt_stream_params* p, const rbt_patch_floor_target* t, std::vector<rbt::PatchFloorIn>& out) {
  out.assign((size_t)n, rbt::PatchFloorIn());
  for (int i = 0; i < n; i++) {
    const std::string who = "entry " + std::to_string(i) + ": ";
    if (t[i].struct_size != sizeof(rbt_patch_floor_target)) { err = who + "rbt_patch_floor_target.struct_size is not sizeof(rbt_patch_floor_target)"; return RBT_ERR_PARAM; }
    rbt_patch_floor_target zero; memset(&zero, 0, sizeof(zero));
    const bool empty = !t[i].min_psnr_mdb && !t[i].region && !t[i].qp_min && !t[i].qp_max && !t[i].background_qp && !t[i].max_trials && !t[i].n_frames && !t[i].patches && !t[i].n_patches &&
                       !t[i].patch_min_psnr_mdb && !memcmp(&t[i].atlas, &zero.atlas, sizeof(zero.atlas));
    if (empty) continue;
    if (p[i].video_type == RBT_VIDEO_OCCUPANCY) { err = who + "an occupancy stream is coded losslessly and takes no PSNR floor (its target must be empty)"; return RBT_ERR_PARAM; }
    if (t[i].min_psnr_mdb < 0) { err = who + "min_psnr_mdb must not be negative"; return RBT_ERR_PARAM; }
    if (t[i].region != RBT_QUALITY_ALL && t[i].region != RBT_QUALITY_OCCUPIED) { err = who + "region must be RBT_QUALITY_ALL or RBT_QUALITY_OCCUPIED"; return RBT_ERR_PARAM; }
    if (int rc = fill_patch_request(err, who, p[i], t[i], t[i].min_psnr_mdb, t[i].region, t[i].patch_min_psnr_mdb, out[(size_t)i])) return rc;
  }
  return RBT_OK;
}
// The refusals of rbt_submit_gof_d1_patches that the parameters alone decide, in three rounds over the entries as their order of precedence has it: the target's own fields,
// the walks' side (out, fill_patch_request) and the clouds' side (req, check_d1). as_d1: the clouds' side as D1 targets without a floor of their own (atlas, patch lists,
// references, peak), alive until submit returns - check_d1 and the CloudRequest take an array of rbt_d1_target, the type the job keeps its clouds' side in
static int check_d1_patches(rbt_ctx* ctx, int n, const rbt_stream_params* p, const rbt_patch_d1_target* t, std::vector<rbt_d1_target>& as_d1, std::vector<rbt::PatchFloorIn>& out,
                            rbt::CloudRequest<rbt_d1_target>& req) {
  std::string& err = ctx->last_err;
  out.assign((size_t)n, rbt::PatchFloorIn()); as_d1.assign((size_t)n, rbt_d1_target());
  std::vector<char> has((size_t)n, 0);
  for (int i = 0; i < n; i++) {
    const std::string who = "entry " + std::to_string(i) + ": ";
    rbt_d1_target& d = as_d1[(size_t)i]; memset(&d, 0, sizeof(d)); d.struct_size = sizeof(d);
    if (t[i].struct_size != sizeof(rbt_patch_d1_target)) { err = who + "rbt_patch_d1_target.struct_size is not sizeof(rbt_patch_d1_target)"; return RBT_ERR_PARAM; }
    rbt_patch_d1_target zero; memset(&zero, 0, sizeof(zero));
    const bool empty = !t[i].min_d1_mdb && !t[i].peak && !t[i].qp_min && !t[i].qp_max && !t[i].background_qp && !t[i].max_trials && !t[i].n_frames && !t[i].patches && !t[i].n_patches &&
                       !t[i].patch_min_d1_mdb && !t[i].reference && !memcmp(&t[i].atlas, &zero.atlas, sizeof(zero.atlas));
    if (empty) continue;
    if (p[i].video_type != RBT_VIDEO_GEOMETRY) { err = who + "a D1 target on a non-geometry entry (the target of an attribute or occupancy entry must be empty)"; return RBT_ERR_PARAM; }
    if (t[i].min_d1_mdb < 0) { err = who + "min_d1_mdb must not be negative"; return RBT_ERR_PARAM; }
    if (t[i].peak < 0) { err = who + "peak must not be negative (0 = 1023)"; return RBT_ERR_PARAM; }
    if (t[i].atlas.map_count != 2) { err = who + "floors held patch by patch need atlas.map_count 2: a point-cloud frame is the two pictures that are coded as a pair"; return RBT_ERR_PARAM; }
    has[(size_t)i] = 1;
    d.peak = t[i].peak; d.qp_min = t[i].qp_min; d.qp_max = t[i].qp_max; d.n_frames = t[i].n_frames; d.atlas = t[i].atlas; d.patches = t[i].patches; d.n_patches = t[i].n_patches; d.reference = t[i].reference;
  }
  for (int i = 0; i < n; i++) if (has[(size_t)i])
    if (int rc = fill_patch_request(err, "entry " + std::to_string(i) + ": ", p[i], t[i], t[i].min_d1_mdb, RBT_QUALITY_ALL, t[i].patch_min_d1_mdb, out[(size_t)i])) return rc;
  return check_d1(ctx, n, p, as_d1.data(), req);
}
// D2 floors: what a D2 target adds to the D1 target it is turned into - every given reference carries normals, and the record for the normals of the clouds of the
// decoded input is a good one (struct_size 0 = all defaults)
static int check_d2_side(rbt_ctx* ctx, const std::string& who, const rbt_pcloud* const* reference, int n_frames, const rbt_normals_params& np, rbt::NormalsIn& out) {
  if (int rc = normals_params(ctx->last_err, np.struct_size ? &np : nullptr, &out.k, &out.orient, out.vp)) { ctx->last_err = who + ctx->last_err; return rc; }
  for (int f = 0; reference && f < n_frames; f++) if (reference[f] && !rbt::pcloud_has_normals(reference[f]->cloud)) {
    ctx->last_err = who + "reference " + std::to_string(f) + " carries no normals (D2 needs normals on the source)"; return RBT_ERR_PARAM; }
  return RBT_OK;
}
// The refusals of rbt_submit_gof_d2: the target becomes the D1 target of the same fields (as_d1, min_d1_mdb holding the D2 floor) and takes check_d1's refusals with its
// words; then the D2 side
static int check_d2(rbt_ctx* ctx, int n, const rbt_stream_params* p, const rbt_d2_target* t, std::vector<rbt_d1_target>& as_d1, rbt::CloudRequest<rbt_d1_target>& req, std::vector<rbt::NormalsIn>& normals) {
  as_d1.assign((size_t)n, rbt_d1_target()); normals.assign((size_t)n, rbt::NormalsIn());
  for (int i = 0; i < n; i++) {
    rbt_d1_target& d = as_d1[(size_t)i]; memset(&d, 0, sizeof(d)); d.struct_size = sizeof(d);
    if (t[i].struct_size != sizeof(rbt_d2_target)) { ctx->last_err = "entry " + std::to_string(i) + ": rbt_d2_target.struct_size is not sizeof(rbt_d2_target)"; return RBT_ERR_PARAM; }
    d.min_d1_mdb = t[i].min_d2_mdb; d.stat = t[i].stat; d.peak = t[i].peak; d.qp_min = t[i].qp_min; d.qp_max = t[i].qp_max; d.n_frames = t[i].n_frames; d.atlas = t[i].atlas;
    d.patches = t[i].patches; d.n_patches = t[i].n_patches; d.reference = t[i].reference;
  }
  if (int rc = check_d1(ctx, n, p, as_d1.data(), req)) return rc;
  for (int i = 0; i < n; i++) if (as_d1[(size_t)i].n_frames > 0)
    if (int rc = check_d2_side(ctx, "entry " + std::to_string(i) + ": ", t[i].reference, t[i].n_frames, t[i].normals, normals[(size_t)i])) return rc;
  return RBT_OK;
}
// ... and of rbt_submit_gof_d2_patches: the target becomes the rbt_patch_d1_target of the same fields and takes check_d1_patches' refusals; then the D2 side
static int check_d2_patches(rbt_ctx* ctx, int n, const rbt_stream_params* p, const rbt_patch_d2_target* t, std::vector<rbt_patch_d1_target>& as_pd1, std::vector<rbt_d1_target>& as_d1,
                            std::vector<rbt::PatchFloorIn>& out, rbt::CloudRequest<rbt_d1_target>& req, std::vector<rbt::NormalsIn>& normals) {
  as_pd1.assign((size_t)n, rbt_patch_d1_target()); normals.assign((size_t)n, rbt::NormalsIn());
  for (int i = 0; i < n; i++) {
    rbt_patch_d1_target& d = as_pd1[(size_t)i]; memset(&d, 0, sizeof(d)); d.struct_size = sizeof(d);
    if (t[i].struct_size != sizeof(rbt_patch_d2_target)) { ctx->last_err = "entry " + std::to_string(i) + ": rbt_patch_d2_target.struct_size is not sizeof(rbt_patch_d2_target)"; return RBT_ERR_PARAM; }
    d.min_d1_mdb = t[i].min_d2_mdb; d.peak = t[i].peak; d.qp_min = t[i].qp_min; d.qp_max = t[i].qp_max; d.background_qp = t[i].background_qp; d.max_trials = t[i].max_trials; d.atlas = t[i].atlas;
    d.n_frames = t[i].n_frames; d.patches = t[i].patches; d.n_patches = t[i].n_patches; d.patch_min_d1_mdb = t[i].patch_min_d2_mdb; d.reference = t[i].reference;
  }
  if (int rc = check_d1_patches(ctx, n, p, as_pd1.data(), as_d1, out, req)) return rc;
  for (int i = 0; i < n; i++) if (as_d1[(size_t)i].n_frames > 0)
    if (int rc = check_d2_side(ctx, "entry " + std::to_string(i) + ": ", t[i].reference, t[i].n_frames, t[i].normals, normals[(size_t)i])) return rc;
  return RBT_OK;
}
// The refusals of rbt_submit_gof_color_patches that the parameters alone decide, as check_d1_patches has them: the target's own fields, the walks' side (out,
// fill_patch_request) and the clouds' side (req, check_color, with its words). as_color: the clouds' side as colour targets without a floor of their own, alive until
// submit returns
static int check_color_patches(rbt_ctx* ctx, int n, const rbt_stream_params* p, const rbt_patch_color_target* t, std::vector<rbt_color_target>& as_color, std::vector<rbt::PatchFloorIn>& out,
                               rbt::CloudRequest<rbt_color_target>& req) {
  std::string& err = ctx->last_err;
  out.assign((size_t)n, rbt::PatchFloorIn()); as_color.assign((size_t)n, rbt_color_target());
  std::vector<char> has((size_t)n, 0);
  for (int i = 0; i < n; i++) {
    const std::string who = "entry " + std::to_string(i) + ": ";
    rbt_color_target& d = as_color[(size_t)i]; memset(&d, 0, sizeof(d)); d.struct_size = sizeof(d);
    if (t[i].struct_size != sizeof(rbt_patch_color_target)) { err = who + "rbt_patch_color_target.struct_size is not sizeof(rbt_patch_color_target)"; return RBT_ERR_PARAM; }
    rbt_patch_color_target zero; memset(&zero, 0, sizeof(zero));
    const bool empty = !t[i].min_psnr_mdb && !t[i].channel && !t[i].qp_min && !t[i].qp_max && !t[i].background_qp && !t[i].max_trials && !t[i].n_frames && !t[i].patches && !t[i].n_patches &&
                       !t[i].patch_min_psnr_mdb && !t[i].upsample_filter && !t[i].attr_transfer && !t[i].reference && !memcmp(&t[i].atlas, &zero.atlas, sizeof(zero.atlas));
    if (empty) continue;
    if (p[i].video_type != RBT_VIDEO_ATTRIBUTE) { err = who + "a colour target on a non-attribute entry (the target of a geometry or occupancy entry must be empty)"; return RBT_ERR_PARAM; }
    if (t[i].min_psnr_mdb < 0) { err = who + "min_psnr_mdb must not be negative"; return RBT_ERR_PARAM; }
    if (t[i].atlas.map_count != 2) { err = who + "floors held patch by patch need atlas.map_count 2: a point-cloud frame is the two pictures that are coded as a pair"; return RBT_ERR_PARAM; }
    has[(size_t)i] = 1;
    d.channel = t[i].channel; d.stat = RBT_D1_MIN; d.qp_min = t[i].qp_min; d.qp_max = t[i].qp_max; d.n_frames = t[i].n_frames; d.atlas = t[i].atlas; d.patches = t[i].patches; d.n_patches = t[i].n_patches;
    d.upsample_filter = t[i].upsample_filter; d.attr_transfer = t[i].attr_transfer; d.reference = t[i].reference;
  }
  for (int i = 0; i < n; i++) if (has[(size_t)i])
    if (int rc = fill_patch_request(err, "entry " + std::to_string(i) + ": ", p[i], t[i], t[i].min_psnr_mdb, RBT_QUALITY_ALL, t[i].patch_min_psnr_mdb, out[(size_t)i])) return rc;
  return check_color(ctx, n, p, as_color.data(), req);
}
static int submit(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, rbt_job** job, const SubmitExtras& x) {
  if (!ctx || n < 1 || n > RBT_MAX_STREAMS || !annexb_in || !n_in || !p || !job) return RBT_ERR_PARAM;
  *job = nullptr;
  RBT_ENTER(ctx);
  rbt::GofRequest r; r.n = n; r.in = annexb_in; r.n_in = n_in; r.params = p; r.gof_rule = x.gof_rule; r.targets = x.targets; r.quality = x.quality; r.per_frame = x.per_frame;
  if (x.targets) if (int rc = check_targets(ctx->last_err, n, p, x.targets)) return rc;
  if (x.quality) if (int rc = check_quality(ctx->last_err, n, p, x.quality)) return rc;
  rbt::CloudRequest<rbt_d1_target> d1;
  if (x.d1) { if (int rc = check_d1(ctx, n, p, x.d1, d1)) return rc; r.d1 = &d1; }
  if (x.d1 && x.per_frame) for (int i = 0; i < n; i++) if (x.d1[i].stat != RBT_D1_MIN) { ctx->last_err = "entry " + std::to_string(i) + ": stat must be 0 (RBT_D1_MIN): every frame holds the floor on its own"; return RBT_ERR_PARAM; }
  rbt::CloudRequest<rbt_color_target> color;
  if (x.color) { if (int rc = check_color(ctx, n, p, x.color, color)) return rc; r.color = &color; }
  std::vector<std::vector<int8_t>> frame_qp;
  if (x.lists) { if (int rc = check_frame_qp(ctx->last_err, n, p, x.lists, frame_qp)) return rc; r.frame_qp = &frame_qp; }
  std::vector<rbt::QpMapIn> qp_maps;
  if (x.maps) { if (int rc = check_qp_maps(ctx->last_err, n, p, x.maps, qp_maps)) return rc; r.qp_maps = &qp_maps; }
  std::vector<rbt::PatchFloorIn> patch_floors;
  if (x.patches) { if (int rc = check_patch_floors(ctx->last_err, n, p, x.patches, patch_floors)) return rc; r.patch_floors = &patch_floors; }
  std::vector<rbt_d1_target> as_d1;
  if (x.d1_patches) { if (int rc = check_d1_patches(ctx, n, p, x.d1_patches, as_d1, patch_floors, d1)) return rc; r.patch_floors = &patch_floors; r.d1 = &d1; r.patch_d1 = true; }
  std::vector<rbt_patch_d1_target> as_pd1; std::vector<rbt::NormalsIn> normals;
  if (x.d2) { if (int rc = check_d2(ctx, n, p, x.d2, as_d1, d1, normals)) return rc; r.d1 = &d1; r.d2_normals = &normals; }
  if (x.d2_patches) { if (int rc = check_d2_patches(ctx, n, p, x.d2_patches, as_pd1, as_d1, patch_floors, d1, normals)) return rc; r.patch_floors = &patch_floors; r.d1 = &d1; r.patch_d1 = true; r.d2_normals = &normals; }
  std::vector<rbt_color_target> as_color;
  if (x.color_patches) { if (int rc = check_color_patches(ctx, n, p, x.color_patches, as_color, patch_floors, color)) return rc; r.patch_floors = &patch_floors; r.color = &color; r.patch_color = true; }
  int slot = -1;
  for (int s = 0; s < D.depth && slot < 0; s++) if (!D.jobs[s]) slot = s;
  if (slot < 0) return RBT_ERR_BUSY;
  for (int i = 0; i < n; i++) if (p[i].md5_sei < RBT_HASH_NONE || p[i].md5_sei > RBT_HASH_CHECKSUM) { ctx->last_err = "md5_sei of stream " + std::to_string(i) + " is not an RBT_HASH_* kind"; return RBT_ERR_PARAM; }
  rbt_job* j = new rbt_job{rbt::gof_submit(slot, D.depth, r), ctx};
  if (x.quality || x.d1 || x.color || x.lists || x.maps || x.patches || x.d1_patches || x.d2 || x.d2_patches || x.color_patches) if (int rc = rbt::gof_refused(j->j, ctx->last_err)) { rbt::gof_abandon(j->j); delete j; return rc; }      // refused by the plan: nothing was enqueued, the slot stays free
  D.jobs[slot] = j; *job = j;
  return RBT_OK;                       // errors of the build surface in rbt_wait_gof, which also releases the job
}
int rbt_set_depth(rbt_ctx* ctx, int max_in_flight) try {
  if (!ctx || max_in_flight < 1 || max_in_flight > RBT_MAX_JOBS) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  for (int s = 0; s < RBT_MAX_JOBS; s++) if (D.jobs[s]) return RBT_ERR_BUSY;
  D.depth = max_in_flight;
  return RBT_OK;
} RBT_CATCH
int rbt_get_depth(rbt_ctx* ctx) try {
  if (!ctx) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return D.depth;
} RBT_CATCH
// Measured on one MI355X (tools/short_run_sweep.sh, tools/walk_shape_sweep.sh): a long walk keeps max_jobs jobs of 2 GOFs in flight; a walk shorter than 48 GOFs
// is all ramp-up and drain and runs as at most 7 jobs (2 up to 12 GOFs), which then own several hardware queues each. Same rule as gof_shard.job_shape.
int rbt_job_shape(int n_gofs, int max_jobs, int* gofs_per_job, int* jobs_in_flight) try {
  if (n_gofs < 0 || max_jobs < 1 || !gofs_per_job || !jobs_in_flight) return RBT_ERR_PARAM;
  if (max_jobs > RBT_MAX_JOBS) max_jobs = RBT_MAX_JOBS;
  if (n_gofs >= 96) { *gofs_per_job = 3; *jobs_in_flight = max_jobs; return RBT_OK; }      // round 3 (XCD-aware tile order, less HBM traffic): 16 x 3 GOFs 905-909 fps, 16 x 2 874-882, 12 x 4 897
  if (n_gofs >= 48) { *gofs_per_job = 2; *jobs_in_flight = max_jobs; return RBT_OK; }
  const int jobs = n_gofs <= 12 ? 2 : 7;
  int g = (n_gofs + jobs - 1) / jobs; if (g < 1) g = 1;
  int d = (n_gofs + g - 1) / g; if (d > max_jobs) d = max_jobs; if (d < 1) d = 1;
  *gofs_per_job = g; *jobs_in_flight = d;
  return RBT_OK;
} RBT_CATCH
int rbt_preset_from_name(const char* name) try {
  if (!name || !*name) return RBT_PRESET_DEFAULT;
  for (const char* f : {"ultrafast", "superfast"}) if (!strcmp(name, f)) return RBT_PRESET_FAST;
  for (const char* d : {"veryfast", "faster", "fast", "medium", "slow", "slower", "veryslow", "placebo"}) if (!strcmp(name, d)) return RBT_PRESET_DEFAULT;
  return RBT_ERR_PARAM;
} RBT_CATCH
int rbt_device_memory(rbt_ctx* ctx, rbt_memory* out) try {
  if (!ctx || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  memset(out, 0, sizeof(*out));
  if (rbtk::dev_mem_info(&out->free_bytes, &out->total_bytes, &out->cached_bytes, &out->in_use_bytes)) return RBT_ERR_NO_DEVICE;
  out->reserve_bytes = rbtk::dev_reserve_bytes();
  const size_t kept = ctx->cloud_cache.bytes();           // clean volumes of released clouds: cached, not in use
  out->cached_bytes += kept; out->in_use_bytes -= kept < out->in_use_bytes ? kept : out->in_use_bytes;
  return RBT_OK;
} RBT_CATCH
int rbt_job_memory(rbt_ctx* ctx, const rbt_job* job, size_t* bytes) try {
  if (!ctx || !job || !bytes) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  bool mine = false; for (int s = 0; s < RBT_MAX_JOBS; s++) if (D.jobs[s] == job && job->owner == ctx) mine = true;
  if (!mine) return RBT_ERR_PARAM;
  *bytes = rbt::gof_memory(job->j);
  return RBT_OK;
} RBT_CATCH
int rbt_trim(rbt_ctx* ctx) try {
  if (!ctx) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  for (int s = 0; s < RBT_MAX_JOBS; s++) if (D.jobs[s]) return RBT_ERR_BUSY;
  rbt::pcloud_cache_trim(ctx->cloud_cache);
  rbtk::dev_release_pool();
  return RBT_OK;
} RBT_CATCH
// kind: the kind of job the calling wait collects, r: where its results go (the streams and n_flat are filled in here). A job of another kind stays collectable; of the two
// kinds that differ the one that comes first in GofKind is named - by the wait that was called if it is that wait's, by the job's wait if it is the job's
static int wait(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt::GofKind kind = rbt::GOF_PLAIN, rbt::GofResults r = rbt::GofResults()) {
  if (!ctx || !job || !annexb_out || !n_out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  int slot = -1;
  for (int s = 0; s < RBT_MAX_JOBS; s++) if (D.jobs[s] == job) slot = s;
  if (slot < 0 || job->owner != ctx) return RBT_ERR_PARAM;
  static const char* const names[] = {nullptr, "quality", "d1", "color", "d1_frames", "quality_frames", "quality_patches", "d1_patches", "d2", "d2_patches", "color_patches"};      // per GofKind: rbt_submit_gof_<name>, rbt_wait_gof_<name>
  const rbt::GofKind is = rbt::gof_kind(job->j);
  if (is != kind) {      // the wait was called for a job of another kind / the job was handed to another wait
    const bool called = is == rbt::GOF_PLAIN || (kind != rbt::GOF_PLAIN && kind < is);
    const std::string name = names[called ? kind : is], sub = "rbt_submit_gof_" + name, wt = "rbt_wait_gof_" + name;
    ctx->last_err = called ? wt + " collects jobs of " + sub + " only" : "a job of " + sub + " is collected by " + wt;
    return RBT_ERR_PARAM;
  }
  int n_flat = 0; r.out = annexb_out; r.n_out = n_out; r.n_flat = &n_flat;
  int rc = rbt::gof_wait(job->j, ctx->stats, ctx->last_err, r);
  if (!rc) ctx->n_flat = n_flat;
  D.jobs[slot] = nullptr; delete job;
  return rc;
}
int rbt_wait_gof(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out) try { return wait(ctx, job, annexb_out, n_out); } RBT_CATCH
// ---- a QP per point-cloud frame ----
int rbt_submit_gof_frame_qp(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_frame_qp* lists, rbt_job** job) try {
  if (!lists) return RBT_ERR_PARAM;
  SubmitExtras x; x.lists = lists; return submit(ctx, n, annexb_in, n_in, p, job, x);
} RBT_CATCH
int rbt_transcode_gof_frame_qp(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_frame_qp* lists,
                               uint8_t** annexb_out, size_t* n_out) try {
  if (!annexb_out || !n_out) return RBT_ERR_PARAM;
  rbt_job* job = nullptr;
  int rc = rbt_submit_gof_frame_qp(ctx, n, annexb_in, n_in, p, lists, &job);
  if (rc) return rc;
  return rbt_wait_gof(ctx, job, annexb_out, n_out);
} RBT_CATCH
// ---- transcoding to a byte budget ----
int rbt_submit_gof_rate(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_rate_target* targets, rbt_job** job) try {
  if (!targets) return RBT_ERR_PARAM;
  SubmitExtras x; x.targets = targets; return submit(ctx, n, annexb_in, n_in, p, job, x);
} RBT_CATCH
int rbt_wait_gof_rate(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_rate_result* results) try {
  if (!results) return RBT_ERR_PARAM;
  rbt::GofResults r; r.rate = results; return wait(ctx, job, annexb_out, n_out, rbt::GOF_PLAIN, r);
} RBT_CATCH
int rbt_transcode_gof_rate(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_rate_target* targets,
                           uint8_t** annexb_out, size_t* n_out, rbt_rate_result* results) {
  return transcode(rbt_submit_gof_rate, rbt_wait_gof_rate, ctx, n, annexb_in, n_in, p, targets, annexb_out, n_out, results);
}
// ---- transcoding to a PSNR floor ----
int rbt_submit_gof_quality(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_quality_target* targets, rbt_job** job) try {
  if (!targets) return RBT_ERR_PARAM;
  SubmitExtras x; x.quality = targets; return submit(ctx, n, annexb_in, n_in, p, job, x);
} RBT_CATCH
int rbt_wait_gof_quality(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_quality_result* results) try {
  if (!results) return RBT_ERR_PARAM;
  rbt::GofResults r; r.quality = results; return wait(ctx, job, annexb_out, n_out, rbt::GOF_QUALITY, r);
} RBT_CATCH
int rbt_transcode_gof_quality(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_quality_target* targets,
                              uint8_t** annexb_out, size_t* n_out, rbt_quality_result* results) {
  return transcode(rbt_submit_gof_quality, rbt_wait_gof_quality, ctx, n, annexb_in, n_in, p, targets, annexb_out, n_out, results);
}
// ---- a QP per CTB ----
int rbt_submit_gof_qp_map(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_qp_map* maps, rbt_job** job) try {
  SubmitExtras x; x.maps = maps; return submit(ctx, n, annexb_in, n_in, p, job, x);      // maps == NULL: rbt_submit_gof
} RBT_CATCH
int rbt_transcode_gof_qp_map(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_qp_map* maps,
                             uint8_t** annexb_out, size_t* n_out) try {
  if (!annexb_out || !n_out) return RBT_ERR_PARAM;
  rbt_job* job = nullptr;
  int rc = rbt_submit_gof_qp_map(ctx, n, annexb_in, n_in, p, maps, &job);
  if (rc) return rc;
  return rbt_wait_gof(ctx, job, annexb_out, n_out);
} RBT_CATCH
int rbt_qp_map_from_patches(const rbt_atlas_params* atlas, const rbt_patch* patches, int n_patches, const int8_t* patch_qp, int background_qp, int log2_ctb, int8_t* out, int w_ctb, int h_ctb) try {
  std::string err;      // (no context to leave the reason with: the header names every refusal)
  return rbt::qp_map_from_patches(err, atlas, patches, n_patches, patch_qp, background_qp, log2_ctb, out, w_ctb, h_ctb);
} RBT_CATCH
// ---- D1 floors held patch by patch ----
int rbt_submit_gof_d1_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_d1_target* targets, rbt_job** job) try {
  if (!targets) return RBT_ERR_PARAM;
  SubmitExtras x; x.d1_patches = targets; return submit(ctx, n, annexb_in, n_in, p, job, x);
} RBT_CATCH
int rbt_wait_gof_d1_patches(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_patch_d1_result* results) try {
  if (!results) return RBT_ERR_PARAM;
  rbt::GofResults r; r.d1_patches = results; return wait(ctx, job, annexb_out, n_out, rbt::GOF_D1_PATCHES, r);
} RBT_CATCH
int rbt_transcode_gof_d1_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_d1_target* targets,
                                 uint8_t** annexb_out, size_t* n_out, rbt_patch_d1_result* results) {
  if (!ctx || n < 1 || n > RBT_MAX_STREAMS || !annexb_in || !n_in || !p || !targets) return RBT_ERR_PARAM;      // (refused here, before submit would)
  return transcode(rbt_submit_gof_d1_patches, rbt_wait_gof_d1_patches, ctx, n, annexb_in, n_in, p, targets, annexb_out, n_out, results);
}
// ---- D2 floors: on the stream and held patch by patch ----
int rbt_submit_gof_d2(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_d2_target* targets, rbt_job** job) try {
  if (!targets) return RBT_ERR_PARAM;
  SubmitExtras x; x.d2 = targets; return submit(ctx, n, annexb_in, n_in, p, job, x);
} RBT_CATCH
int rbt_wait_gof_d2(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_d2_floor_result* results) try {
  if (!results) return RBT_ERR_PARAM;
  rbt::GofResults r; r.d2 = results; return wait(ctx, job, annexb_out, n_out, rbt::GOF_D2, r);
} RBT_CATCH
int rbt_transcode_gof_d2(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_d2_target* targets,
                         uint8_t** annexb_out, size_t* n_out, rbt_d2_floor_result* results) {
  return transcode(rbt_submit_gof_d2, rbt_wait_gof_d2, ctx, n, annexb_in, n_in, p, targets, annexb_out, n_out, results);
}
int rbt_submit_gof_d2_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_d2_target* targets, rbt_job** job) try {
  if (!targets) return RBT_ERR_PARAM;
  SubmitExtras x; x.d2_patches = targets; return submit(ctx, n, annexb_in, n_in, p, job, x);
} RBT_CATCH
int rbt_wait_gof_d2_patches(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_patch_d2_result* results) try {
  if (!results) return RBT_ERR_PARAM;
  rbt::GofResults r; r.d2_patches = results; return wait(ctx, job, annexb_out, n_out, rbt::GOF_D2_PATCHES, r);
} RBT_CATCH
int rbt_transcode_gof_d2_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_d2_target* targets,
                                 uint8_t** annexb_out, size_t* n_out, rbt_patch_d2_result* results) {
  if (!ctx || n < 1 || n > RBT_MAX_STREAMS || !annexb_in || !n_in || !p || !targets) return RBT_ERR_PARAM;      // (refused here, before submit would)
  return transcode(rbt_submit_gof_d2_patches, rbt_wait_gof_d2_patches, ctx, n, annexb_in, n_in, p, targets, annexb_out, n_out, results);
}
// ---- colour floors held patch by patch ----
int rbt_submit_gof_color_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_color_target* targets, rbt_job** job) try {
  if (!targets) return RBT_ERR_PARAM;
  SubmitExtras x; x.color_patches = targets; return submit(ctx, n, annexb_in, n_in, p, job, x);
} RBT_CATCH
int rbt_wait_gof_color_patches(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_patch_color_result* results) try {
  if (!results) return RBT_ERR_PARAM;
  rbt::GofResults r; r.color_patches = results; return wait(ctx, job, annexb_out, n_out, rbt::GOF_COLOR_PATCHES, r);
} RBT_CATCH
int rbt_transcode_gof_color_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_color_target* targets,
                                    uint8_t** annexb_out, size_t* n_out, rbt_patch_color_result* results) {
  if (!ctx || n < 1 || n > RBT_MAX_STREAMS || !annexb_in || !n_in || !p || !targets) return RBT_ERR_PARAM;      // (refused here, before submit would)
  return transcode(rbt_submit_gof_color_patches, rbt_wait_gof_color_patches, ctx, n, annexb_in, n_in, p, targets, annexb_out, n_out, results);
}
// ---- PSNR floors held patch by patch ----
int rbt_submit_gof_quality_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_floor_target* targets, rbt_job** job) try {
  if (!targets) return RBT_ERR_PARAM;
  SubmitExtras x; x.patches = targets; return submit(ctx, n, annexb_in, n_in, p, job, x);
} RBT_CATCH
int rbt_wait_gof_quality_patches(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_patch_floor_result* results) try {
  if (!results) return RBT_ERR_PARAM;
  rbt::GofResults r; r.patches = results; return wait(ctx, job, annexb_out, n_out, rbt::GOF_QUALITY_PATCHES, r);
} RBT_CATCH
int rbt_transcode_gof_quality_patches(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_patch_floor_target* targets,
                                      uint8_t** annexb_out, size_t* n_out, rbt_patch_floor_result* results) {
  return transcode(rbt_submit_gof_quality_patches, rbt_wait_gof_quality_patches, ctx, n, annexb_in, n_in, p, targets, annexb_out, n_out, results);
}
// ---- floors held frame by frame ----
int rbt_submit_gof_quality_frames(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_quality_target* targets, rbt_job** job) try {
  if (!targets) return RBT_ERR_PARAM;
  SubmitExtras x; x.quality = targets; x.per_frame = true; return submit(ctx, n, annexb_in, n_in, p, job, x);
} RBT_CATCH
int rbt_wait_gof_quality_frames(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_frame_floor_result* results) try {
  if (!results) return RBT_ERR_PARAM;
  rbt::GofResults r; r.frames = results; return wait(ctx, job, annexb_out, n_out, rbt::GOF_QUALITY_FRAMES, r);
} RBT_CATCH
int rbt_transcode_gof_quality_frames(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_quality_target* targets,
                                     uint8_t** annexb_out, size_t* n_out, rbt_frame_floor_result* results) {
  return transcode(rbt_submit_gof_quality_frames, rbt_wait_gof_quality_frames, ctx, n, annexb_in, n_in, p, targets, annexb_out, n_out, results);
}
int rbt_submit_gof_d1_frames(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_d1_target* targets, rbt_job** job) try {
  if (!targets) return RBT_ERR_PARAM;
  SubmitExtras x; x.d1 = targets; x.per_frame = true; return submit(ctx, n, annexb_in, n_in, p, job, x);
} RBT_CATCH
int rbt_wait_gof_d1_frames(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_frame_floor_result* results) try {
  if (!results) return RBT_ERR_PARAM;
  rbt::GofResults r; r.frames = results; return wait(ctx, job, annexb_out, n_out, rbt::GOF_D1_FRAMES, r);
} RBT_CATCH
int rbt_transcode_gof_d1_frames(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_d1_target* targets,
                                uint8_t** annexb_out, size_t* n_out, rbt_frame_floor_result* results) {
  return transcode(rbt_submit_gof_d1_frames, rbt_wait_gof_d1_frames, ctx, n, annexb_in, n_in, p, targets, annexb_out, n_out, results);
}
// ---- transcoding geometry to a D1 floor ----
int rbt_submit_gof_d1(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_d1_target* targets, rbt_job** job) try {
  if (!targets) return RBT_ERR_PARAM;
  SubmitExtras x; x.d1 = targets; return submit(ctx, n, annexb_in, n_in, p, job, x);
} RBT_CATCH
int rbt_wait_gof_d1(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_d1_floor_result* results) try {
  if (!results) return RBT_ERR_PARAM;
  rbt::GofResults r; r.d1 = results; return wait(ctx, job, annexb_out, n_out, rbt::GOF_D1, r);
} RBT_CATCH
int rbt_transcode_gof_d1(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_d1_target* targets,
                         uint8_t** annexb_out, size_t* n_out, rbt_d1_floor_result* results) {
  return transcode(rbt_submit_gof_d1, rbt_wait_gof_d1, ctx, n, annexb_in, n_in, p, targets, annexb_out, n_out, results);
}
// ---- transcoding attributes to a colour PSNR floor ----
int rbt_submit_gof_color(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_color_target* targets, rbt_job** job) try {
  if (!targets) return RBT_ERR_PARAM;
  SubmitExtras x; x.color = targets; return submit(ctx, n, annexb_in, n_in, p, job, x);
} RBT_CATCH
int rbt_wait_gof_color(rbt_ctx* ctx, rbt_job* job, uint8_t** annexb_out, size_t* n_out, rbt_color_floor_result* results) try {
  if (!results) return RBT_ERR_PARAM;
  rbt::GofResults r; r.color = results; return wait(ctx, job, annexb_out, n_out, rbt::GOF_COLOR, r);
} RBT_CATCH
int rbt_transcode_gof_color(rbt_ctx* ctx, int n, const uint8_t* const* annexb_in, const size_t* n_in, const rbt_stream_params* p, const rbt_color_target* targets,
                            uint8_t** annexb_out, size_t* n_out, rbt_color_floor_result* results) {
  return transcode(rbt_submit_gof_color, rbt_wait_gof_color, ctx, n, annexb_in, n_in, p, targets, annexb_out, n_out, results);
}
int rbt_gather_luma(rbt_ctx* ctx, const uint16_t* src, int n_pics, int stride, int rows, int x0, int y0, int w, int h, int src_misalign, uint16_t* out) try {
  if (!ctx || !src || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbt::gather_luma_host(ctx->last_err, src, n_pics, stride, rows, x0, y0, w, h, src_misalign, out);
} RBT_CATCH
int rbt_gather_420(rbt_ctx* ctx, const uint16_t* src, int n_pics, int stride, int rows, int chroma_stride, int chroma_rows, int x0, int y0, int w, int h, int src_misalign, uint16_t* out) try {
  if (!ctx || !src || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbt::gather_420_host(ctx->last_err, src, n_pics, stride, rows, chroma_stride, chroma_rows, x0, y0, w, h, src_misalign, out);
} RBT_CATCH
int rbt_picture_sse(rbt_ctx* ctx, const uint16_t* a, const uint16_t* b, int width, int height, int n_frames, const uint16_t* occ, int ow, int oh, uint64_t* out) try {
  if (!ctx || !a || !b || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbt::picture_sse_host(ctx->last_err, a, b, width, height, n_frames, occ, ow, oh, out, ctx->stats);
} RBT_CATCH
int rbt_ctb_sse(rbt_ctx* ctx, const uint16_t* a, const uint16_t* b, int width, int height, int n_frames, int log2_ctb, const uint16_t* occ, int ow, int oh,
                const int32_t* rects, int n_rects, uint64_t* out_ctb, uint64_t* out_rect) try {
  if (!ctx || !a || !b || !out_ctb) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbt::ctb_sse_host(ctx->last_err, a, b, width, height, n_frames, log2_ctb, occ, ow, oh, rects, n_rects, out_ctb, out_rect, ctx->stats);
} RBT_CATCH
int rbt_level_census(rbt_ctx* ctx, const int16_t* y, const int16_t* cb, const int16_t* cr, int w, int h, const int8_t* qp4, const uint8_t* pm4, uint32_t* hist) try {
  if (!ctx || !y || !cb || !cr || !qp4 || !pm4 || !hist) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbt::level_census_host(ctx->last_err, y, cb, cr, w, h, qp4, pm4, hist);
} RBT_CATCH
int rbt_rate_estimate(rbt_ctx* ctx, const uint8_t* annexb, size_t n, int video_type, rbt_rate_table* out) try {
  if (!ctx || !annexb || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  memset(out, 0, sizeof(*out));
  if (video_type == RBT_VIDEO_OCCUPANCY) { ctx->last_err = "an occupancy stream is coded losslessly: there is no rate estimate for it"; return RBT_ERR_PARAM; }
  return rbt::rate_estimate(ctx->last_err, annexb, n, out);
} RBT_CATCH
int rbt_encode(rbt_ctx* ctx, const uint16_t* yuv, int width, int height, int bit_depth, int n_frames, int qp, int gop, int lossless,
               int log2_ctb, int ctb_rows_per_slice, int md5_sei, uint8_t** annexb_out, size_t* n_out) try {
  if (!ctx || !yuv || !annexb_out || !n_out || n_frames < 1) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbt::encode_yuv(ctx->stats, ctx->last_err, yuv, width, height, bit_depth, n_frames, qp, gop, lossless, log2_ctb, ctb_rows_per_slice, md5_sei, annexb_out, n_out);
} RBT_CATCH
int rbt_or_pool(rbt_ctx* ctx, const uint16_t* plane, int width, int height, int factor, uint16_t* out) try {
  if (!ctx || !plane || !out || factor < 1 || width % factor || height % factor) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbt::or_pool_host(plane, width, height, factor, out);
} RBT_CATCH

int rbt_picture_hash(rbt_ctx* ctx, const uint16_t* yuv, int width, int height, int bit_depth, int n_frames, int kind, uint8_t* out) try {
  if (!ctx || !yuv || !out || n_frames < 1) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbt::picture_hash_host(ctx->last_err, yuv, width, height, bit_depth, n_frames, kind, out);
} RBT_CATCH

int rbt_selftest_transform32(rbt_ctx* ctx, const int16_t* blocks, int n_blocks, int bit_depth, uint32_t* n_mismatch) try {
  if (!ctx || !blocks || n_blocks < 1 || bit_depth < 8 || bit_depth > 12 || !n_mismatch) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbtk::selftest_transform32(blocks, n_blocks, bit_depth, n_mismatch) ? RBT_ERR_NO_DEVICE : RBT_OK;
} RBT_CATCH
// a case the hook can stage without leaving the CTB tile (csrc/rbt_tb_hook.h)
static bool tb_case_ok(const rbt_tb_case& c) {
  if (c.kind < RBT_TB_LUMA || c.kind > RBT_TB_PAIR || c.bit_depth < 8 || c.bit_depth > 12 || c.log2_ctb < 4 || c.log2_ctb > 6) return false;
  const int sh = c.kind != RBT_TB_LUMA, nn = (1 << c.log2_ctb) >> sh;
  if (c.log2 < 2 || c.log2 > (sh ? 4 : 5)) return false;
  const int N = 1 << c.log2, qp_max = 51 + 6 * (c.bit_depth - 8);
  if (c.x0 < 0 || c.y0 < 0 || (c.x0 & 3) || (c.y0 & 3) || c.x0 + N > nn || c.y0 + N > nn || c.mode < 0 || c.mode > 34) return false;
  if (c.qp[0] < 0 || c.qp[0] > qp_max || c.qp[1] < 0 || c.qp[1] > qp_max) return false;
  if (c.kind == RBT_TB_PAIR && c.transform_skip) return false;
  return true;
}
int rbt_selftest_tb(rbt_ctx* ctx, const rbt_tb_case* cases, int n_cases, const uint16_t* nb, const uint8_t* unit_av, const int16_t* levels, uint16_t* out) try {
  if (!ctx || !cases || n_cases < 1 || n_cases > (1 << 16) || !nb || !unit_av || !levels || !out) return RBT_ERR_PARAM;
  for (int i = 0; i < n_cases; i++) if (!tb_case_ok(cases[i])) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
#ifdef RBT_HOSTEMU
  if (!rbtk::selftest_tb) { ctx->last_err = "this stand-in of the launch interface has no selftest_tb"; return RBT_ERR_PARAM; }
#endif
  return rbtk::selftest_tb(cases, n_cases, nb, unit_av, levels, out) ? RBT_ERR_NO_DEVICE : RBT_OK;
} RBT_CATCH
int rbt_reconstruct(rbt_ctx* ctx, const rbt_atlas_params* atlas, const rbt_patch* patches, int n_patches, const uint16_t* occ_luma, const uint16_t* geo_d0,
                    const uint16_t* geo_d1, int geo_bit_depth, const uint16_t* attr_t0, const uint16_t* attr_t1, int attr_bit_depth, rbt_cloud* out) try {
  if (!ctx || !atlas || (!patches && n_patches) || !occ_luma || !geo_d0 || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  int rc = rbt::pcc_reconstruct(ctx->last_err, atlas, patches, n_patches, occ_luma, geo_d0, geo_d1, geo_bit_depth, attr_t0, attr_t1, attr_bit_depth, out);
  if (rc) rbt_cloud_free(out);
  return rc;
} RBT_CATCH
void rbt_cloud_free(rbt_cloud* c) { if (!c) return; free(c->xyz); free(c->yuv); free(c->occupancy_map); free(c->block_to_patch); memset(c, 0, sizeof(*c)); }
int rbt_d1(rbt_ctx* ctx, const int16_t* xyz_a, int n_a, const int16_t* xyz_b, int n_b, int peak, rbt_d1_result* out) try {
  if (!ctx || !xyz_a || !xyz_b || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbt::pcc_d1(ctx->last_err, xyz_a, n_a, xyz_b, n_b, peak, out);
} RBT_CATCH
int rbt_d2(rbt_ctx* ctx, const int16_t* xyz_a, const int16_t* normals_a, int n_a, const int16_t* xyz_b, int n_b, int peak, rbt_d2_result* out) try {
  if (!ctx || !xyz_a || !normals_a || !xyz_b || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbt::pcc_d2(ctx->last_err, xyz_a, normals_a, n_a, xyz_b, n_b, peak, out);
} RBT_CATCH

// colour half of the metric (csrc/rbt_color.h)
int rbt_yuv420_to_yuv444(rbt_ctx* ctx, const uint16_t* yuv420, int width, int height, int bit_depth, int n_frames, int filter, uint16_t* yuv444) try {
  if (!ctx || !yuv420 || !yuv444) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbt::pcc_yuv420_to_yuv444(ctx->last_err, yuv420, width, height, bit_depth, n_frames, filter, yuv444, &ctx->color_ms[0]);
} RBT_CATCH
int rbt_yuv16_to_rgb8(rbt_ctx* ctx, const uint16_t* yuv16, int n, uint8_t* rgb) try {
  if (!ctx || !yuv16 || !rgb) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbt::pcc_yuv16_to_rgb8(ctx->last_err, yuv16, n, rgb, &ctx->color_ms[1]);
} RBT_CATCH
int rbt_reconstruct_rgb(rbt_ctx* ctx, const rbt_atlas_params* atlas, const rbt_patch* patches, int n_patches, const uint16_t* occ_luma, const uint16_t* geo_d0,
                        const uint16_t* geo_d1, int geo_bit_depth, const uint16_t* attr_t0, const uint16_t* attr_t1, int attr_bit_depth, int upsample_filter,
                        rbt_cloud* out, uint8_t** rgb) {
  if (!ctx || !atlas || (!patches && n_patches) || !occ_luma || !geo_d0 || !out || !rgb) return RBT_ERR_PARAM;
  *rgb = nullptr; memset(out, 0, sizeof(*out));
  int rc;
  try {                       // whatever the host side throws half way: nothing allocated so far is left behind
    RBT_ENTER(ctx);
    rc = rbt::pcc_reconstruct_rgb(ctx->last_err, atlas, patches, n_patches, occ_luma, geo_d0, geo_d1, geo_bit_depth, attr_t0, attr_t1, attr_bit_depth, upsample_filter, out, rgb, ctx->color_ms);
  } catch (const std::bad_alloc&) { rc = RBT_ERR_NOMEM; } catch (...) { rc = RBT_ERR_NO_DEVICE; }
  if (rc) { rbt_cloud_free(out); free(*rgb); *rgb = nullptr; }
  return rc;
}
int rbt_color_metric(rbt_ctx* ctx, const int16_t* xyz_a, const uint8_t* rgb_a, int n_a, const int16_t* xyz_b, const uint8_t* rgb_b, int n_b, rbt_color_result* out) try {
  if (!ctx || !xyz_a || !xyz_b || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  return rbt::pcc_color_metric(ctx->last_err, xyz_a, rgb_a, n_a, xyz_b, rgb_b, n_b, out, &ctx->color_ms[2]);
} RBT_CATCH
int rbt_reconstruct_decoded(rbt_ctx* ctx, const rbt_atlas_params* atlas, const rbt_patch* patches, int n_patches, const uint16_t* occ_luma, const uint16_t* geo_d0,
                            const uint16_t* geo_d1, int geo_bit_depth, const uint16_t* attr_t0, const uint16_t* attr_t1, int attr_bit_depth, int upsample_filter, int attr_transfer,
                            rbt_cloud* out, uint8_t** rgb, uint8_t** moved) {
  if (!ctx || !atlas || (!patches && n_patches) || !occ_luma || !geo_d0 || !out || !rgb) return RBT_ERR_PARAM;
  *rgb = nullptr; memset(out, 0, sizeof(*out)); if (moved) *moved = nullptr;
  int rc;
  try {
    RBT_ENTER(ctx);
    ctx->color_ms[3] = 0; ctx->n_changed = 0;
    if (attr_transfer != 0 && attr_transfer != 1) { ctx->last_err = "attribute transfer filter types other than 1 are not built"; return RBT_ERR_UNSUPPORTED; }
    rc = rbt::pcc_reconstruct_decoded(ctx->last_err, atlas, patches, n_patches, occ_luma, geo_d0, geo_d1, geo_bit_depth, attr_t0, attr_t1, attr_bit_depth, upsample_filter, attr_transfer, out, rgb, moved,
                                      &ctx->n_changed, ctx->color_ms);
  } catch (const std::bad_alloc&) { rc = RBT_ERR_NOMEM; } catch (...) { rc = RBT_ERR_NO_DEVICE; }
  if (rc) { rbt_cloud_free(out); free(*rgb); *rgb = nullptr; if (moved) { free(*moved); *moved = nullptr; } }
  return rc;
}
int rbt_transfer_colors(rbt_ctx* ctx, const int16_t* src_xyz, const uint16_t* src_yuv, int n_src, const int16_t* tgt_xyz, uint16_t* tgt_yuv, const uint8_t* moved, int n_tgt, int* n_changed) try {
  if (!ctx || !src_xyz || !src_yuv || !n_changed || (n_tgt > 0 && (!tgt_xyz || !tgt_yuv || !moved))) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  ctx->color_ms[3] = 0; ctx->n_changed = 0;
  const int rc = rbt::pcc_transfer_colors(ctx->last_err, src_xyz, src_yuv, n_src, tgt_xyz, tgt_yuv, moved, n_tgt, n_changed, &ctx->color_ms[3]);
  if (!rc) ctx->n_changed = *n_changed;
  return rc;
} RBT_CATCH
int rbt_transfer_stage(rbt_ctx* ctx, double* ms, int* n_changed) try {
  if (!ctx) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  if (ms) *ms = ctx->color_ms[3];
  if (n_changed) *n_changed = ctx->n_changed;
  return RBT_OK;
} RBT_CATCH
int rbt_color_stage_ms(rbt_ctx* ctx, double ms[3]) try {
  if (!ctx || !ms) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  for (int i = 0; i < 3; i++) ms[i] = ctx->color_ms[i];
  return RBT_OK;
} RBT_CATCH

// ---- clouds on the device and their scoring (csrc/rbt_score.h) ----
static bool cloud_of(const rbt_ctx* ctx, const rbt_pcloud* h) { return h && h->owner == ctx; }
static int cloud_handle(rbt_ctx* ctx, rbt::PCloud* c, rbt_pcloud** out) {
  rbt_pcloud* h = nullptr;
  try { h = new rbt_pcloud{c, ctx}; ctx->clouds.push_back(h); } catch (...) { delete h; rbt::pcloud_release(ctx->cloud_cache, c); return RBT_ERR_NOMEM; }
  *out = h;
  return RBT_OK;
}
int rbt_pcloud_upload(rbt_ctx* ctx, const int16_t* xyz, const uint8_t* rgb, const int16_t* normals_q14, int n, rbt_pcloud** out) try {
  if (!ctx || !out) return RBT_ERR_PARAM;
  *out = nullptr;
  if (!xyz) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  rbt::PCloud* c = nullptr;
  const int rc = rbt::pcloud_upload(ctx->last_err, ctx->cloud_cache, xyz, rgb, normals_q14, n, &c);
  return rc ? rc : cloud_handle(ctx, c, out);
} RBT_CATCH
int rbt_pcloud_from_maps(rbt_ctx* ctx, const rbt_atlas_params* atlas, const rbt_patch* patches, int n_patches, const uint16_t* occ_luma, const uint16_t* geo_d0,
                         const uint16_t* geo_d1, int geo_bit_depth, const uint16_t* attr_t0, const uint16_t* attr_t1, int attr_bit_depth, int upsample_filter, int attr_transfer,
                         rbt_pcloud** out, rbt_cloud* host_copy, uint8_t** rgb) {
  if (!ctx || !out) return RBT_ERR_PARAM;
  *out = nullptr; if (rgb) *rgb = nullptr; if (host_copy) memset(host_copy, 0, sizeof(*host_copy));
  if (!atlas || (!patches && n_patches) || !occ_luma || !geo_d0) return RBT_ERR_PARAM;
  int rc;
  try {
    RBT_ENTER(ctx);
    ctx->color_ms[3] = 0; ctx->n_changed = 0;
    if (attr_transfer != 0 && attr_transfer != 1) { ctx->last_err = "attribute transfer filter types other than 1 are not built"; return RBT_ERR_UNSUPPORTED; }
    rbt::PCloud* c = nullptr;
    rc = rbt::pcloud_from_maps(ctx->last_err, ctx->cloud_cache, atlas, patches, n_patches, occ_luma, geo_d0, geo_d1, geo_bit_depth, attr_t0, attr_t1, attr_bit_depth, upsample_filter, attr_transfer, &c,
                               host_copy, rgb, &ctx->n_changed, ctx->color_ms);
    if (!rc) rc = cloud_handle(ctx, c, out);
  } catch (const std::bad_alloc&) { rc = RBT_ERR_NOMEM; } catch (...) { rc = RBT_ERR_NO_DEVICE; }
  if (rc) { if (host_copy) rbt_cloud_free(host_copy); if (rgb) { free(*rgb); *rgb = nullptr; } }
  return rc;
}
int rbt_pcloud_points(const rbt_pcloud* cloud, int* n_points, int* n_merged) {
  if (!cloud) return RBT_ERR_PARAM;
  rbt::pcloud_points(cloud->cloud, n_points, n_merged);
  return RBT_OK;
}
void rbt_pcloud_release(rbt_ctx* ctx, rbt_pcloud* cloud) {
  if (!ctx || !cloud_of(ctx, cloud)) return;
  DevState& D = g_dev[ctx->device]; std::lock_guard<std::mutex> lk(D.mu);
  for (size_t i = 0; i < ctx->clouds.size(); i++) if (ctx->clouds[i] == cloud) {
    ctx->clouds.erase(ctx->clouds.begin() + (long)i);
    for (rbt_score_pair* p : ctx->pairs) p->stale |= rbt::score_pair_uses(p->pair, cloud->cloud);
    if (!rbtk::dev_select(ctx->device)) rbt::pcloud_release(ctx->cloud_cache, cloud->cloud);
    delete cloud;
    return;
  }
}
// the checked form of rbt_normals_params (NULL = all defaults)
static int normals_params(std::string& err, const rbt_normals_params* p, int* k, int* orient, int32_t vp[3]) {
  *k = 16; *orient = RBT_NORMALS_ORIENT_VIEW_POINT; vp[0] = vp[1] = vp[2] = 0;
  if (!p) return RBT_OK;
  if (p->struct_size != sizeof(rbt_normals_params)) { err = "rbt_normals_params.struct_size is not sizeof(rbt_normals_params)"; return RBT_ERR_PARAM; }
  if (p->k != 0 && (p->k < 3 || p->k > 32)) { err = "k is 0 (= 16) or 3..32"; return RBT_ERR_PARAM; }
  if (p->orientation < RBT_NORMALS_ORIENT_NONE || p->orientation > RBT_NORMALS_ORIENT_CUBEMAP) { err = "orientation is not one of RBT_NORMALS_ORIENT_*"; return RBT_ERR_PARAM; }
  if (p->orientation == RBT_NORMALS_ORIENT_SPANNING_TREE || p->orientation == RBT_NORMALS_ORIENT_CUBEMAP) { err = "spanning-tree and cube-map orientation are not built"; return RBT_ERR_UNSUPPORTED; }
  if (p->k) *k = p->k;
  *orient = p->orientation; for (int i = 0; i < 3; i++) vp[i] = p->view_point[i];
  return RBT_OK;
}
int rbt_pcloud_estimate_normals(rbt_ctx* ctx, rbt_pcloud* cloud, const rbt_normals_params* p, int16_t* normals_q14, double* device_ms) try {
  if (!ctx) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  if (device_ms) *device_ms = 0;
  if (!cloud_of(ctx, cloud)) { ctx->last_err = "not a cloud of this context"; return RBT_ERR_PARAM; }
  int k, orient; int32_t vp[3];
  const int rc = normals_params(ctx->last_err, p, &k, &orient, vp);
  return rc ? rc : rbt::pcloud_estimate_normals(ctx->last_err, cloud->cloud, k, orient, vp, normals_q14, device_ms);
} RBT_CATCH
int rbt_estimate_normals(rbt_ctx* ctx, const int16_t* xyz, int n, const rbt_normals_params* p, int16_t* normals_q14) try {
  if (!ctx || !xyz || !normals_q14) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  int k, orient; int32_t vp[3];
  int rc = normals_params(ctx->last_err, p, &k, &orient, vp);
  if (rc) return rc;
  rbt::PCloud* c = nullptr;
  rc = rbt::pcloud_upload(ctx->last_err, ctx->cloud_cache, xyz, nullptr, nullptr, n, &c);
  if (rc) return rc;
  rc = rbt::pcloud_estimate_normals(ctx->last_err, c, k, orient, vp, normals_q14, nullptr);
  rbt::pcloud_release(ctx->cloud_cache, c);
  return rc;
} RBT_CATCH
int rbt_score(rbt_ctx* ctx, const rbt_pcloud* a, const rbt_pcloud* b, int peak, int parts, rbt_frame_score* out) try {
  if (!ctx || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  if (!cloud_of(ctx, a) || !cloud_of(ctx, b)) { ctx->last_err = "not a cloud of this context"; return RBT_ERR_PARAM; }
  if (parts < 0 || parts > (RBT_SCORE_D1 | RBT_SCORE_D2 | RBT_SCORE_COLOR)) { ctx->last_err = "parts is not a set of RBT_SCORE_*"; return RBT_ERR_PARAM; }
  return rbt::pcloud_score(ctx->last_err, a->cloud, b->cloud, peak, parts, out);
} RBT_CATCH
int rbt_pcloud_set_colors(rbt_ctx* ctx, rbt_pcloud* cloud, const uint8_t* rgb) try {
  if (!ctx || !rgb) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  if (!cloud_of(ctx, cloud)) { ctx->last_err = "not a cloud of this context"; return RBT_ERR_PARAM; }
  return rbt::pcloud_set_colors(ctx->last_err, cloud->cloud, rgb);
} RBT_CATCH
int rbt_pcloud_set_labels(rbt_ctx* ctx, rbt_pcloud* cloud, const uint32_t* labels) try {
  if (!ctx || !labels) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  if (!cloud_of(ctx, cloud)) { ctx->last_err = "not a cloud of this context"; return RBT_ERR_PARAM; }
  return rbt::pcloud_set_labels(ctx->last_err, cloud->cloud, labels);
} RBT_CATCH
int rbt_pcloud_labels(rbt_ctx* ctx, const rbt_pcloud* cloud, uint32_t* labels) try {
  if (!ctx || !labels) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  if (!cloud_of(ctx, cloud)) { ctx->last_err = "not a cloud of this context"; return RBT_ERR_PARAM; }
  return rbt::pcloud_labels(ctx->last_err, cloud->cloud, labels);
} RBT_CATCH
int rbt_score_patches(rbt_ctx* ctx, const rbt_pcloud* a, const rbt_pcloud* b, int peak, int n_patches, rbt_patch_d1* out, rbt_d1_result* whole, double* device_ms) try {
  if (!ctx || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  if (!cloud_of(ctx, a) || !cloud_of(ctx, b)) { ctx->last_err = "not a cloud of this context"; return RBT_ERR_PARAM; }
  return rbt::pcloud_score_patches(ctx->last_err, a->cloud, b->cloud, peak, n_patches, out, whole, device_ms);
} RBT_CATCH
int rbt_score_patches_d2(rbt_ctx* ctx, const rbt_pcloud* a, const rbt_pcloud* b, int peak, int n_patches, rbt_patch_d2* out, rbt_d2_result* whole, double* device_ms) try {
  if (!ctx || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  if (!cloud_of(ctx, a) || !cloud_of(ctx, b)) { ctx->last_err = "not a cloud of this context"; return RBT_ERR_PARAM; }
  return rbt::pcloud_score_patches_d2(ctx->last_err, a->cloud, b->cloud, peak, n_patches, out, whole, device_ms);
} RBT_CATCH
static bool pair_of(const rbt_ctx* ctx, const rbt_score_pair* h) { return h && h->owner == ctx; }
int rbt_score_pair_create(rbt_ctx* ctx, const rbt_pcloud* a, const rbt_pcloud* b, rbt_score_pair** out) try {
  if (!ctx || !out) return RBT_ERR_PARAM;
  *out = nullptr;
  RBT_ENTER(ctx);
  if (!cloud_of(ctx, a) || !cloud_of(ctx, b)) { ctx->last_err = "not a cloud of this context"; return RBT_ERR_PARAM; }
  rbt::ScorePair* p = nullptr;
  if (int rc = rbt::score_pair_create(ctx->last_err, a->cloud, b->cloud, &p)) return rc;
  rbt_score_pair* h = nullptr;
  try { h = new rbt_score_pair{p, ctx, false}; ctx->pairs.push_back(h); } catch (...) { delete h; rbt::score_pair_release(p); return RBT_ERR_NOMEM; }
  *out = h;
  return RBT_OK;
} RBT_CATCH
int rbt_score_pair_color(rbt_ctx* ctx, const rbt_score_pair* pair, rbt_color_result* out) try {
  if (!ctx || !out) return RBT_ERR_PARAM;
  memset(out, 0, sizeof(*out));
  RBT_ENTER(ctx);
  if (!pair_of(ctx, pair)) { ctx->last_err = "not a score pair of this context"; return RBT_ERR_PARAM; }
  if (pair->stale) { ctx->last_err = "a cloud of the pair has been released"; return RBT_ERR_PARAM; }
  return rbt::score_pair_color(ctx->last_err, pair->pair, out);
} RBT_CATCH
int rbt_score_patches_color(rbt_ctx* ctx, const rbt_pcloud* a, const rbt_pcloud* b, int n_patches, rbt_patch_color* out, rbt_color_result* whole, double* device_ms) try {
  if (!ctx || !out) return RBT_ERR_PARAM;
  RBT_ENTER(ctx);
  if (!cloud_of(ctx, a) || !cloud_of(ctx, b)) { ctx->last_err = "not a cloud of this context"; return RBT_ERR_PARAM; }
  return rbt::pcloud_score_patches_color(ctx->last_err, a->cloud, b->cloud, n_patches, out, whole, device_ms);
} RBT_CATCH
int rbt_score_pair_patches_color(rbt_ctx* ctx, const rbt_score_pair* pair, int n_patches, rbt_patch_color* out, rbt_color_result* whole) try {
  if (!ctx || !out) return RBT_ERR_PARAM;
  if (whole) memset(whole, 0, sizeof(*whole));
  RBT_ENTER(ctx);
  if (!pair_of(ctx, pair)) { ctx->last_err = "not a score pair of this context"; return RBT_ERR_PARAM; }
  if (pair->stale) { ctx->last_err = "a cloud of the pair has been released"; return RBT_ERR_PARAM; }
  return rbt::score_pair_patches_color(ctx->last_err, pair->pair, n_patches, out, whole);
} RBT_CATCH
void rbt_score_pair_release(rbt_ctx* ctx, rbt_score_pair* pair) {
  if (!ctx || !pair_of(ctx, pair)) return;
  DevState& D = g_dev[ctx->device]; std::lock_guard<std::mutex> lk(D.mu);
  for (size_t i = 0; i < ctx->pairs.size(); i++) if (ctx->pairs[i] == pair) {
    ctx->pairs.erase(ctx->pairs.begin() + (long)i);
    if (!rbtk::dev_select(ctx->device)) rbt::score_pair_release(pair->pair);
    delete pair;
    return;
  }
}
int rbt_score_summary(const rbt_frame_score* frames, int n_frames, rbt_sequence_score* out) {
  if (!out || n_frames < 0 || (!frames && n_frames)) return RBT_ERR_PARAM;
  memset(out, 0, sizeof(*out));
  out->n_frames = n_frames;
  double sum[5] = {0, 0, 0, 0, 0}, least[5] = {0, 0, 0, 0, 0}; int n[5] = {0, 0, 0, 0, 0};
  for (int f = 0; f < n_frames; f++) {
    const rbt_frame_score& s = frames[f];
    out->points_a += s.n_points_a; out->points_b += s.n_points_b; out->merged_a += s.n_merged_a; out->merged_b += s.n_merged_b;
    const double fig[5] = {s.d1.psnr, s.d2.psnr, s.color.psnr[0], s.color.psnr[1], s.color.psnr[2]};
    const int part[5] = {RBT_SCORE_D1, RBT_SCORE_D2, RBT_SCORE_COLOR, RBT_SCORE_COLOR, RBT_SCORE_COLOR};
    for (int k = 0; k < 5; k++) if (s.parts & part[k]) { sum[k] += fig[k]; if (!n[k] || fig[k] < least[k]) least[k] = fig[k]; n[k]++; }
  }
  out->n_d1 = n[0]; out->n_d2 = n[1]; out->n_color = n[2];
  double mean[5]; for (int k = 0; k < 5; k++) mean[k] = n[k] ? sum[k] / n[k] : 0.0;
  out->mean_d1 = mean[0]; out->min_d1 = least[0]; out->mean_d2 = mean[1]; out->min_d2 = least[1];
  for (int c = 0; c < 3; c++) { out->mean_color[c] = mean[2 + c]; out->min_color[c] = least[2 + c]; }
  return RBT_OK;
}

}  // extern "C"
