// Encode half + the transcode pipeline (decode -> pool -> encode). See rbt_transcode.cpp.
#pragma once
#include <string>
#include <vector>
#include "../../include/rbt.h"
namespace rbt {
int transcode_gof(rbt_stats& st, std::string& err, int n, const uint8_t* const* in, const size_t* n_in, const rbt_stream_params* p, uint8_t** out, size_t* n_out);
struct GofJob;
// gof_rule: apply transcodeData's rule (PCCTranscoder.cpp:150): an occupancy stream is only transcoded when occupancyPrecision == 4
// targets: nullptr, or one per entry (checked by the caller: rbt_submit_gof_rate); results: nullptr, or one per entry
// quality: nullptr, or one floor per entry (rbt_submit_gof_quality; not together with targets); quality_results: nullptr, or one per entry of such a job
// d1: nullptr, or the D1 targets of rbt_submit_gof_d1 (checked by the caller; not together with targets or quality): one per entry, the reference handles of each entry
// resolved to the clouds (n_frames of them, nullptr = the cloud of the decoded input), and the context's cache of cloud volumes
struct PCloud; struct PCloudCache;
struct D1Request { const rbt_d1_target* targets; std::vector<std::vector<const PCloud*>> refs; PCloudCache* cache; };
// color: nullptr, or the colour targets of rbt_submit_gof_color (checked by the caller; not together with targets, quality or d1), resolved the same way
struct ColorRequest { const rbt_color_target* targets; std::vector<std::vector<const PCloud*>> refs; PCloudCache* cache; };
// frame_qp: nullptr, or per entry a QP per point-cloud frame (rbt_submit_gof_frame_qp; values and video types checked by the caller, the count against the stream's pictures
// here: gof_refused), empty = the entry's own QP; not together with targets, quality, d1 or color
// qp_maps: nullptr, or per entry a QP per CTB (rbt_submit_gof_qp_map; struct sizes, values and video types checked by the caller, the counts against the stream's pictures here:
// gof_refused), an empty qp = the entry's own QP; not together with anything but p
struct QpMapIn { std::vector<int8_t> qp; int n_frames = 0, w_ctb = 0, h_ctb = 0; };
GofJob* gof_submit(int slot, int depth, int n, const uint8_t* const* in, const size_t* n_in, const rbt_stream_params* p, bool gof_rule, const rbt_rate_target* targets = nullptr, const rbt_quality_target* quality = nullptr,
                   const D1Request* d1 = nullptr, const ColorRequest* color = nullptr, const std::vector<std::vector<int8_t>>* frame_qp = nullptr, bool per_frame = false,   // per_frame: with quality, rbt_submit_gof_quality_frames
                   const std::vector<QpMapIn>* qp_maps = nullptr);
int gof_wait(GofJob* j, rbt_stats& st, std::string& err, uint8_t** out, size_t* n_out, rbt_rate_result* results = nullptr, rbt_quality_result* quality_results = nullptr, int* n_flat = nullptr,
             rbt_d1_floor_result* d1_results = nullptr, rbt_color_floor_result* color_results = nullptr, rbt_frame_floor_result* frame_results = nullptr);   // consumes the job
bool gof_is_quality(const GofJob* j);           // a job of rbt_submit_gof_quality
bool gof_is_quality_frames(const GofJob* j);    // a job of rbt_submit_gof_quality_frames
bool gof_is_d1_frames(const GofJob* j);         // a job of rbt_submit_gof_d1_frames
bool gof_is_d1(const GofJob* j);                // a job of rbt_submit_gof_d1
bool gof_is_color(const GofJob* j);             // a job of rbt_submit_gof_color
int gof_refused(const GofJob* j, std::string& err);   // != 0: the job's plan was refused before anything was built or enqueued (the code; the reason in err)
void gof_abandon(GofJob* j);
size_t gof_memory(const GofJob* j);             // device memory the job's build took (its arenas)
int encode_yuv(rbt_stats& st, std::string& err, const uint16_t* yuv, int w, int h, int bd, int n_frames, int qp, int gop, int lossless, int log2_ctb, int rows, int md5, uint8_t** out, size_t* n_out);
int or_pool_host(const uint16_t* plane, int w, int h, int factor, uint16_t* out);
int level_census_host(std::string& err, const int16_t* y, const int16_t* cb, const int16_t* cr, int w, int h, const int8_t* qp4, const uint8_t* pm4, uint32_t* hist);   // rbt_level_census
int picture_sse_host(std::string& err, const uint16_t* a, const uint16_t* b, int w, int h, int n_frames, const uint16_t* occ, int ow, int oh, uint64_t* out, rbt_stats& st);   // rbt_picture_sse; st.gpu_ms: device time between events around the launches
int rate_estimate(std::string& err, const uint8_t* annexb, size_t n, rbt_rate_table* out);   // rbt_rate_estimate
int picture_hash_host(std::string& err, const uint16_t* yuv, int w, int h, int bd, int n_frames, int kind, uint8_t* out);   // rbt_picture_hash
}
