// Encode half + the transcode pipeline (decode -> pool -> encode). See rbt_transcode.cpp.
#pragma once
#include <string>
#include <vector>
#include "../../include/rbt.h"
namespace rbt {
struct GofJob;
struct PCloud; struct PCloudCache;
// the cloud targets of rbt_submit_gof_d1 / rbt_submit_gof_color (Target: rbt_d1_target / rbt_color_target), checked by the caller: one per entry, the reference handles of each
// entry resolved to the clouds (n_frames of them, nullptr = the cloud of the decoded input), and the context's cache of cloud volumes
template <class Target> struct CloudRequest { const Target* targets = nullptr; std::vector<std::vector<const PCloud*>> refs; PCloudCache* cache = nullptr; };
// D2 floors: the checked form of an entry's rbt_normals_params, for the clouds of the decoded input (rbt_pcloud_estimate_normals' arguments)
struct NormalsIn { int k = 16, orient = RBT_NORMALS_ORIENT_VIEW_POINT; int32_t vp[3] = {0, 0, 0}; };
struct QpMapIn { std::vector<int8_t> qp; int n_frames = 0, w_ctb = 0, h_ctb = 0; };
// Floors held patch by patch (rbt_submit_gof_quality_patches, rbt_submit_gof_d1_patches), one request per entry, checked and copied by the caller from its own target type: what
// the walks read - the floor where a patch has none of its own, the region of the PSNR figure (RBT_QUALITY_ALL for D1), the QP range, the background's QP (-1 = q0), the cap on
// the trials, of the atlas its size and occupancy_resolution - and per frame (n_frames 0: no target) the patches and their floors F_k
struct PatchFloorIn {
  int32_t floor_mdb = 0; int region = 0, qp_min = 0, qp_max = 0, background_qp = 0, max_trials = 0, atlas_width = 0, atlas_height = 0, occupancy_resolution = 0, n_frames = 0;
  std::vector<std::vector<rbt_patch>> patches; std::vector<std::vector<int32_t>> floors;
};
// What a job is made of: the n inputs with their parameters, and at most one kind of target - each nullptr or one per entry, checked by the caller
struct GofRequest {
  int n = 0; const uint8_t* const* in = nullptr; const size_t* n_in = nullptr; const rbt_stream_params* params = nullptr;
  bool gof_rule = true;                               // transcodeData's rule (PCCTranscoder.cpp:150): an occupancy stream is only transcoded when occupancyPrecision == 4
  const rbt_rate_target* targets = nullptr;           // byte budgets (rbt_submit_gof_rate)
  const rbt_quality_target* quality = nullptr;        // PSNR floors (rbt_submit_gof_quality; with per_frame: rbt_submit_gof_quality_frames)
  const CloudRequest<rbt_d1_target>* d1 = nullptr;    // D1 floors (rbt_submit_gof_d1; with per_frame: rbt_submit_gof_d1_frames)
  const CloudRequest<rbt_color_target>* color = nullptr;   // colour floors (rbt_submit_gof_color)
  bool per_frame = false;                             // the floors of quality / d1 are held frame by frame
  // a QP per point-cloud frame (rbt_submit_gof_frame_qp; values and video types checked by the caller, the count against the stream's pictures here: gof_refused), an empty
  // list = the entry's own QP; not together with a target
  const std::vector<std::vector<int8_t>>* frame_qp = nullptr;
  // a QP per CTB (rbt_submit_gof_qp_map; struct sizes, values and video types checked by the caller, the counts against the stream's pictures here: gof_refused), an empty qp =
  // the entry's own QP; not together with anything else
  const std::vector<QpMapIn>* qp_maps = nullptr;
  const std::vector<PatchFloorIn>* patch_floors = nullptr;   // PSNR floors held patch by patch (rbt_submit_gof_quality_patches); not together with anything else
  // D1 floors held patch by patch (rbt_submit_gof_d1_patches): patch_floors carries the walks' side of the targets (floors, range, background, cap) and d1 their clouds'
  // side (atlas, patch lists, references, peak; min_d1_mdb 0: no walk of its own)
  bool patch_d1 = false;
  // D2 floors (rbt_submit_gof_d2; with patch_d1: rbt_submit_gof_d2_patches): the request is that of the D1 kind - d1 carries the targets as D1 targets, min_d1_mdb holding
  // the D2 floor - and the figure is D2; one record per entry for the normals of the reference clouds made of the decoded input
  const std::vector<NormalsIn>* d2_normals = nullptr;
  // colour floors held patch by patch (rbt_submit_gof_color_patches): patch_floors carries the walks' side of the targets and color their clouds' side (atlas, patch lists,
  // references, channel, filter, transfer; min_psnr_mdb 0: no walk of its own)
  bool patch_color = false;
};
// Where a job's outcome goes: a stream per entry, and of the result arrays - one per entry each - the one of the job's kind; n_flat: nullptr, or the decoded pictures with flat chroma
struct GofResults {
  uint8_t** out = nullptr; size_t* n_out = nullptr; int* n_flat = nullptr;
  rbt_rate_result* rate = nullptr; rbt_quality_result* quality = nullptr; rbt_d1_floor_result* d1 = nullptr; rbt_color_floor_result* color = nullptr; rbt_frame_floor_result* frames = nullptr; rbt_patch_floor_result* patches = nullptr; rbt_patch_d1_result* d1_patches = nullptr;
  rbt_d2_floor_result* d2 = nullptr; rbt_patch_d2_result* d2_patches = nullptr; rbt_patch_color_result* color_patches = nullptr;
};
GofJob* gof_submit(int slot, int depth, const GofRequest& r);
int gof_wait(GofJob* j, rbt_stats& st, std::string& err, const GofResults& r);   // consumes the job
// which submit made the job, in the order the wait half tells a mismatch (rbt_api.cpp wait): the lower of two kinds that differ is the one the message names
enum GofKind { GOF_PLAIN, GOF_QUALITY, GOF_D1, GOF_COLOR, GOF_D1_FRAMES, GOF_QUALITY_FRAMES, GOF_QUALITY_PATCHES, GOF_D1_PATCHES, GOF_D2, GOF_D2_PATCHES, GOF_COLOR_PATCHES };   // GOF_PLAIN: constant QPs, QP lists, QP maps and byte budgets
GofKind gof_kind(const GofJob* j);
int gof_refused(const GofJob* j, std::string& err);   // != 0: the job's plan was refused before anything was built or enqueued (the code; the reason in err)
void gof_abandon(GofJob* j);
size_t gof_memory(const GofJob* j);             // device memory the job's build took (its arenas)
int encode_yuv(rbt_stats& st, std::string& err, const uint16_t* yuv, int w, int h, int bd, int n_frames, int qp, int gop, int lossless, int log2_ctb, int rows, int md5, uint8_t** out, size_t* n_out);
int or_pool_host(const uint16_t* plane, int w, int h, int factor, uint16_t* out);
int level_census_host(std::string& err, const int16_t* y, const int16_t* cb, const int16_t* cr, int w, int h, const int8_t* qp4, const uint8_t* pm4, uint32_t* hist);   // rbt_level_census
int picture_sse_host(std::string& err, const uint16_t* a, const uint16_t* b, int w, int h, int n_frames, const uint16_t* occ, int ow, int oh, uint64_t* out, rbt_stats& st);   // rbt_picture_sse; st.gpu_ms: device time between events around the launches
int ctb_sse_host(std::string& err, const uint16_t* a, const uint16_t* b, int w, int h, int n_frames, int log2_ctb, const uint16_t* occ, int ow, int oh, const int32_t* rects, int n_rects,
                 uint64_t* out_ctb, uint64_t* out_rect, rbt_stats& st);   // rbt_ctb_sse; st.gpu_ms as picture_sse_host's
int rate_estimate(std::string& err, const uint8_t* annexb, size_t n, rbt_rate_table* out);   // rbt_rate_estimate
int picture_hash_host(std::string& err, const uint16_t* yuv, int w, int h, int bd, int n_frames, int kind, uint8_t* out);   // rbt_picture_hash
}
