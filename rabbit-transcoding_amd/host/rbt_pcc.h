// Verification stage: reconstruction of the point cloud from decoded maps and the D1 metric. See rbt_pcc.cpp.
#pragma once
#include <string>
#include <vector>
#include "../../include/rbt.h"
namespace rbt {
int pcc_reconstruct(std::string& err, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, const uint16_t* occ, const uint16_t* d0, const uint16_t* d1, int geo_bd,
                    const uint16_t* t0, const uint16_t* t1, int attr_bd, rbt_cloud* out);
// colour stages (csrc/rbt_color.h); ms / stage_ms: device time of the stage's launches, may be null
int pcc_reconstruct_rgb(std::string& err, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, const uint16_t* occ, const uint16_t* d0, const uint16_t* d1, int geo_bd,
                        const uint16_t* t0, const uint16_t* t1, int attr_bd, int filter, rbt_cloud* out, uint8_t** rgb, double* stage_ms);
// rbt_reconstruct_decoded: pcc_reconstruct_rgb + the attribute transfer after geometry smoothing; stage_ms[3]: device time of the transfer's kernels
int pcc_reconstruct_decoded(std::string& err, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, const uint16_t* occ, const uint16_t* d0, const uint16_t* d1, int geo_bd,
                            const uint16_t* t0, const uint16_t* t1, int attr_bd, int filter, int attr_transfer, rbt_cloud* out, uint8_t** rgb, uint8_t** moved, int* n_changed, double* stage_ms);
int pcc_transfer_colors(std::string& err, const int16_t* sxyz, const uint16_t* syuv, int ns, const int16_t* txyz, uint16_t* tyuv, const uint8_t* moved, int nt, int* n_changed, double* ms);
int pcc_yuv420_to_yuv444(std::string& err, const uint16_t* in, int w, int h, int bd, int n_frames, int filter, uint16_t* out, double* ms);
int pcc_yuv16_to_rgb8(std::string& err, const uint16_t* yuv, int n, uint8_t* rgb, double* ms);
int pcc_color_metric(std::string& err, const int16_t* a, const uint8_t* rgb_a, int na, const int16_t* b, const uint8_t* rgb_b, int nb, rbt_color_result* out, double* ms);
int pcc_d1(std::string& err, const int16_t* a, int na, const int16_t* b, int nb, int peak, rbt_d1_result* out);
int pcc_d2(std::string& err, const int16_t* a, const int16_t* normals_a, int na, const int16_t* b, int nb, int peak, rbt_d2_result* out);
// clouds that stay on the device with their index, and their scoring (csrc/rbt_score.h; rbt_pcloud_*, rbt_score). A context keeps the clean volumes of released clouds.
struct PCloud;
enum : size_t { PCLOUD_VOL_BYTES = ((size_t)1 << 27) + ((size_t)1 << 18) };          // the 1024^3-bit volume and its coarse level (one bit per 8 x 8 x 8 block)
struct PCloudCache { std::vector<void*> vols; size_t bytes() const { return vols.size() * PCLOUD_VOL_BYTES; } };
int pcloud_upload(std::string& err, PCloudCache& cache, const int16_t* xyz, const uint8_t* rgb, const int16_t* nrm, int n, PCloud** out);
int pcloud_from_maps(std::string& err, PCloudCache& cache, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, const uint16_t* occ, const uint16_t* d0, const uint16_t* d1, int geo_bd,
                     const uint16_t* t0, const uint16_t* t1, int attr_bd, int filter, int attr_transfer, PCloud** out, rbt_cloud* host_copy, uint8_t** rgb, int* n_changed, double* stage_ms);
void pcloud_points(const PCloud* c, int* n_points, int* n_merged);
void pcloud_release(PCloudCache& cache, PCloud* c);
void pcloud_cache_trim(PCloudCache& cache);
// normals of the merged cloud (csrc/rbt_normals.h); k, orient and view_point are checked by the caller. out (3 per point) and device_ms may be null
int pcloud_estimate_normals(std::string& err, PCloud* c, int k, int orient, const int32_t view_point[3], int16_t* out, double* device_ms);
int pcloud_score(std::string& err, const PCloud* a, const PCloud* b, int peak, int parts, rbt_frame_score* out);
// Positions-only reconstruction from packed luma planes that are on the device already (rbt_submit_gof_d1), next to reconstruct_impl, which uploads host arrays. What of a
// frame does not depend on the trial encode - patches, items, occupancy map, block-to-patch map - is made once (MapFrame, from the occupancy luma d_occ, which has to stay
// alive as long as the frame); per trial the count, scan, emit, smoothing and index remain (mapframe_cloud: an indexed cloud without colours). Everything is enqueued on the
// current stream (rbtk::set_stream) and waits on that stream alone.
struct MapFrame;
int mapframe_check(std::string& err, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, std::vector<uint32_t>* items = nullptr);   // host only: what rbt_reconstruct refuses
int mapframe_new(std::string& err, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, const uint16_t* d_occ, MapFrame** out);
void mapframe_delete(MapFrame* f);
size_t mapframe_bytes(const rbt_atlas_params* a, int n_patches);         // device memory of a MapFrame, but for its items (bounded by the atlas' blocks per patch list)
int mapframe_cloud(std::string& err, PCloudCache& cache, const MapFrame* f, const uint16_t* d_d0, const uint16_t* d_d1, int geo_bd, PCloud** out, int* n_smoothed);
// the D1 part of pcloud_score: out is what rbt_d1 returns for the two clouds
int pcloud_d1(std::string& err, const PCloud* a, const PCloud* b, int peak, rbt_d1_result* out);
// rbt_gather_luma: the gather kernel (csrc/rbt_cloudmaps.h) on host arrays
int gather_luma_host(std::string& err, const uint16_t* src, int n_pics, int stride, int rows, int x0, int y0, int w, int h, int src_misalign, uint16_t* out);
// rbt_gather_420: the same kernel on the three planes of coded 4:2:0 pictures, three descriptors a picture; out: packed planar 4:2:0, the layout launch_up444 reads
int gather_420_host(std::string& err, const uint16_t* src, int n_pics, int stride, int rows, int cstride, int crows, int x0, int y0, int w, int h, int src_misalign, uint16_t* out);
// rbt_pcloud_set_colors: new RGB triples (3 per point, host) for an indexed cloud; only the colour sums and merged colours of its index are remade (csrc/rbt_score.h)
int pcloud_set_colors(std::string& err, PCloud* c, const uint8_t* rgb);
// D1 per patch of the decoded cloud (csrc/rbt_score.h, "patches"). A cloud of pcloud_from_maps / mapframe_cloud carries the patch index of every point; an uploaded
// cloud gets labels (one per point, < 65536, host) through pcloud_set_labels. pcloud_score_patches: out holds n_patches entries; whole (what pcloud_d1 returns for
// the two clouds) and device_ms may be null.
int pcloud_set_labels(std::string& err, PCloud* c, const uint32_t* labels);
int pcloud_labels(std::string& err, const PCloud* c, uint32_t* labels);
bool pcloud_has_labels(const PCloud* c);
int pcloud_score_patches(std::string& err, const PCloud* a, const PCloud* b, int peak, int n_patches, rbt_patch_d1* out, rbt_d1_result* whole, double* device_ms);
// D2 per patch of the decoded cloud (csrc/rbt_score.h, "D2/patch"): a carries normals, b labels; out holds n_patches entries; whole (the d2 of pcloud_score with
// RBT_SCORE_D2 for the two clouds) and device_ms may be null
bool pcloud_has_normals(const PCloud* c);
int pcloud_score_patches_d2(std::string& err, const PCloud* a, const PCloud* b, int peak, int n_patches, rbt_patch_d2* out, rbt_d2_result* whole, double* device_ms);
// rbt_score_pair_*: the nearest squared distances of both directions between two indexed clouds, kept; pair_color runs the colour walks on them (out: what the colour
// part of pcloud_score returns for the clouds' colours of the moment). The clouds must outlive the pair.
struct ScorePair;
int score_pair_create(std::string& err, const PCloud* a, const PCloud* b, ScorePair** out);
int score_pair_color(std::string& err, const ScorePair* p, rbt_color_result* out);
// Colour per patch of the decoded cloud (csrc/rbt_score.h, "col/patch"): both clouds carry colours, b labels; out holds n_patches entries; whole (the colour part of
// pcloud_score / score_pair_color for the same clouds) and device_ms may be null. The pair form runs no search.
int pcloud_score_patches_color(std::string& err, const PCloud* a, const PCloud* b, int n_patches, rbt_patch_color* out, rbt_color_result* whole, double* device_ms);
int score_pair_patches_color(std::string& err, const ScorePair* p, int n_patches, rbt_patch_color* out, rbt_color_result* whole);
bool score_pair_uses(const ScorePair* p, const PCloud* c);
void score_pair_release(ScorePair* p);
// A frame whose cloud is recoloured per trial (rbt_submit_gof_color): the geometry of a trial does not change with the attribute QP. colorframe_new is the geometry half,
// made once from packed planes on the device (d_occ, d_d0, d_d1 stay alive as long as the frame): the frame's maps, count, scan, emit, smoothing with the per-point moved
// flags, the index of the final cloud. colorframe_color is the colour half for the 4:4:4 planes (3 x W x H each) of one trial's attribute pictures: emit again for the
// colours, attribute transfer, RGB, recolour of the index (launch_sc_recolor); the cloud is then what rbt_pcloud_from_maps makes of the same maps. colorframe_pair keeps
// the distances against a reference, colorframe_score runs the colour walks on them. Everything is enqueued on the current stream and waits on that stream alone.
struct ColorFrame;
int colorframe_new(std::string& err, PCloudCache& cache, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, const uint16_t* d_occ, const uint16_t* d_d0, const uint16_t* d_d1,
                   int geo_bd, int attr_transfer, ColorFrame** out);
int colorframe_color(std::string& err, ColorFrame* f, const uint16_t* d_t0, const uint16_t* d_t1, int attr_bd);
int colorframe_pair(std::string& err, ColorFrame* f, const PCloud* reference);
int colorframe_score(std::string& err, const ColorFrame* f, rbt_color_result* out);
// ... or, in their place, the sums per patch on the same distances (the frame's cloud carries its labels): out holds n_patches entries, whole what colorframe_score returns
int colorframe_score_patches(std::string& err, const ColorFrame* f, int n_patches, rbt_patch_color* out, rbt_color_result* whole);
// packed planar 4:2:0 pictures on the device -> their 4:4:4 planes (3 x w x h each): launch_up444 on the current stream
void colorframe_upconvert(const uint16_t* d_420, int w, int h, int bit_depth, int n_pictures, int filter, uint16_t* d_444);
const PCloud* colorframe_cloud(const ColorFrame* f);
int colorframe_changed(const ColorFrame* f);                              // colours the last colorframe_color's transfer changed
size_t colorframe_bytes(const rbt_atlas_params* a, int n_patches);        // device memory of a frame at most, but for its volume
void colorframe_delete(PCloudCache& cache, ColorFrame* f);
bool pcloud_has_colors(const PCloud* c);
int pcloud_merged(const PCloud* c);
}
