// Host side of the verification stage (csrc/rbt_pcc.h): argument checks, uploads, launches, the point list back to the host.
// Replaces the decoder-side loops of PCCCodec::generatePointCloud (PCCCodec.cpp:517-978) and QualityMetrics::compute (PCCMetrics.cpp:75-231).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "rbt_batch.h"
#include "rbt_pcc.h"
#include "rbt_d1_figures.h"
#include "rbt_color_walk.h"
#include "../csrc/rbt_pcc.h"
#include "../csrc/rbt_cloudmaps.h"
#include "../csrc/rbt_color.h"
#include "../csrc/rbt_score.h"
#include "../csrc/rbt_normals.h"

namespace rbt {
namespace {
struct DevBuf { void* p = nullptr; ~DevBuf() { rbtk::dev_free(p); } bool alloc(size_t n) { p = rbtk::dev_alloc(n); return p != nullptr; } template <class T> T* as() const { return (T*)p; }
                void take(DevBuf& o) { rbtk::dev_free(p); p = o.p; o.p = nullptr; } };
// what reconstruct_impl leaves on the device for rbt_pcloud_from_maps: positions, 4:4:4 triples and RGB8 triples of the finished cloud
// and the patch index of every point (csrc/rbt_score.h, launch_pd_labels)
struct DevCloud { DevBuf xyz, yuv, rgb, labels; };
int block_xy(const rbt_patch& p, int ub, int vb, int* x, int* y) {       // PCCPatch::patchBlock2CanvasBlock
  switch (p.orientation) {
    case RBT_OR_DEFAULT: *x = ub + p.u0; *y = vb + p.v0; return 1;
    case RBT_OR_ROT90: *x = (p.size_v0 - 1 - vb) + p.u0; *y = ub + p.v0; return 1;
    case RBT_OR_ROT180: *x = (p.size_u0 - 1 - ub) + p.u0; *y = (p.size_v0 - 1 - vb) + p.v0; return 1;
    case RBT_OR_ROT270: *x = vb + p.u0; *y = (p.size_u0 - 1 - ub) + p.v0; return 1;
    case RBT_OR_MIRROR: *x = (p.size_u0 - 1 - ub) + p.u0; *y = vb + p.v0; return 1;
    case RBT_OR_MROT90: *x = (p.size_v0 - 1 - vb) + p.u0; *y = (p.size_u0 - 1 - ub) + p.v0; return 1;
    case RBT_OR_MROT180: *x = ub + p.u0; *y = (p.size_v0 - 1 - vb) + p.v0; return 1;
    case RBT_OR_SWAP: *x = vb + p.u0; *y = ub + p.v0; return 1;
  }
  return 0;
}
// device timers of the colour stages (rbt_color_stage_ms), behind the transcoder's (rbt_batch.h)
enum { T_COL_UP = T_COUNT, T_COL_RGB, T_COL_DIST, T_COL_TRANSFER, T_COL_TRANSFER_COPY };    // T_COL_DIST: search, walks and sums of a score (rbt_frame_score.device_ms)
static_assert(T_COL_TRANSFER_COPY < 16, "timer slots");
int lg_of(int n) { int lg = 4; while (((size_t)1 << lg) < 2 * (size_t)n) lg++; return lg; }
// the derived fields of the three results from the sums and counts (shared by the host-array calls and rbt_score)
// QualityMetrics::compute :204-206: float mse, getPSNR with factor 3; symmetric = the worse direction (:299-309)
// (geometry_mse / geometry_psnr: rbt_d1_figures.h, where the figures per patch use them too)
template <class R> void finish_geometry(R* out, int peak) {
  out->mse_ab = geometry_mse((double)out->sse_ab, out->n_a); out->mse_ba = geometry_mse((double)out->sse_ba, out->n_b);
  const float m = out->mse_ab > out->mse_ba ? out->mse_ab : out->mse_ba;
  out->psnr_ab = geometry_psnr(peak, out->mse_ab); out->psnr_ba = geometry_psnr(peak, out->mse_ba); out->psnr = geometry_psnr(peak, m);
}
void finish_color(rbt_color_result* out) {      // (color_mse / color_psnr: rbt_color_walk.h, where the figures per patch use them too)
  for (int c = 0; c < 3; c++) {
    out->mse_ab[c] = color_mse(out->sse_ab[c], (double)out->n_a); out->mse_ba[c] = color_mse(out->sse_ba[c], (double)out->n_b);
    out->psnr_ab[c] = color_psnr(out->mse_ab[c]); out->psnr_ba[c] = color_psnr(out->mse_ba[c]);
    out->mse[c] = out->mse_ab[c] > out->mse_ba[c] ? out->mse_ab[c] : out->mse_ba[c];
    out->psnr[c] = out->psnr_ab[c] < out->psnr_ba[c] ? out->psnr_ab[c] : out->psnr_ba[c];
  }
}

// Attribute transfer (csrc/rbt_color.h) on clouds that are on the device: source = the cloud before smoothing, target = the cloud after it, whose colours are updated in
// place; n_moved = the number of set bytes in d_moved, > 0. flag_G / flag_meta (rbt_reconstruct_decoded): d_moved is still to be written, by the smoothing's filter asked
// once more about the source positions - inside the timed region, it is work of this stage. The volumes and maps are cleared first; the events lie around the kernels only,
// and the scalars are read back after the second event.
int transfer_on_device(std::string& err, const int16_t* d_sxyz, const uint16_t* d_syuv, int ns, const int16_t* d_txyz, uint16_t* d_tyuv, uint8_t* d_moved, int nt, int n_moved,
                       int* n_changed, const RbtSmooth* flag_G = nullptr, const uint32_t* flag_meta = nullptr) {
  const size_t vol_bytes = (size_t)1 << (3 * RBT_PCC_BITS - 3), ne = (size_t)RBT_TC_K * n_moved;
  const int slg = lg_of(ns), tlg = lg_of(nt);
  const size_t sw = (size_t)4 << slg, tw = (size_t)4 << tlg;
  DevBuf svol, tvol, shash, thash, sidx, per_t, mlist, c1, ent, lkey, lsrc, scal;
  if (!svol.alloc(vol_bytes) || !tvol.alloc(vol_bytes) || !shash.alloc(4 * sw) || !thash.alloc(2 * tw) || !sidx.alloc(4 * (size_t)ns) || !per_t.alloc(12 * (size_t)nt) || !mlist.alloc(4 * (size_t)n_moved) ||
      !c1.alloc(6 * (size_t)n_moved) || !ent.alloc(12 * ne) || !lkey.alloc(8 * ne) || !lsrc.alloc(4 * ne) || !scal.alloc(4 * RBT_TC_SCALARS)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  RbtTransfer T; memset(&T, 0, sizeof(T));
  T.sxyz = d_sxyz; T.syuv = d_syuv; T.ns = ns; T.slg = slg; T.svol = svol.as<uint32_t>();
  T.skeys = shash.as<uint32_t>(); T.scnt = T.skeys + ((size_t)1 << slg); T.sfill = T.scnt + ((size_t)1 << slg); T.sfirst = T.sfill + ((size_t)1 << slg); T.sidx = sidx.as<uint32_t>();
  T.txyz = d_txyz; T.tyuv = d_tyuv; T.moved = d_moved; T.nt = nt; T.tlg = tlg; T.tvol = tvol.as<uint32_t>(); T.tkeys = thash.as<uint32_t>(); T.tvals = T.tkeys + ((size_t)1 << tlg);
  T.mlist = mlist.as<uint32_t>(); T.cap = n_moved; T.color1 = c1.as<uint16_t>(); T.ent = ent.as<uint32_t>(); T.ev = T.ent + ne; T.ed = T.ev + ne;
  T.lcnt = per_t.as<uint32_t>(); T.lfill = T.lcnt + nt; T.lfirst = T.lfill + nt; T.lkey = lkey.as<unsigned long long>(); T.lsrc = lsrc.as<uint32_t>(); T.scal = scal.as<uint32_t>();
  if (rbtk::dev_memset(svol.p, 0, vol_bytes) | rbtk::dev_memset(tvol.p, 0, vol_bytes) | rbtk::dev_memset(shash.p, 0, 3 * sw) | rbtk::dev_memset(T.tkeys, 0, tw) | rbtk::dev_memset(T.tvals, 0xFF, tw) |
      rbtk::dev_memset(per_t.p, 0, 8 * (size_t)nt) | rbtk::dev_memset(scal.p, 0, 4 * RBT_TC_SCALARS)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  rbtk::timer_begin(T_COL_TRANSFER);
  if (flag_G) rbtk::launch_tc_flag(flag_G, d_sxyz, flag_meta, d_moved);
  rbtk::launch_transfer(&T);
  rbtk::timer_end(T_COL_TRANSFER);
  uint32_t h[RBT_TC_SCALARS];
  if (rbtk::d2h(h, scal.p, sizeof(h)) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  if (h[RBT_TC_ERR] == RBT_TC_ERR_LIST) { err = "more than 1024 entries chose one moved point"; return RBT_ERR_UNSUPPORTED; }
  if (h[RBT_TC_ERR] == RBT_TC_ERR_BUCKET) { err = "more than 256 coincident source points"; return RBT_ERR_UNSUPPORTED; }
  if (h[RBT_TC_ERR] == RBT_TC_ERR_WALK) { err = "a moved point has fewer than 8 source points within 64 grid units"; return RBT_ERR_UNSUPPORTED; }
  if (h[RBT_TC_ERR] == RBT_TC_ERR_RANGE) { err = "coordinate outside 0..1023"; return RBT_ERR_PARAM; }
  if (h[RBT_TC_ERR] || h[RBT_TC_N_MOVED] != (uint32_t)n_moved) { err = "attribute transfer: inconsistent input"; return RBT_ERR_PARAM; }
  *n_changed = (int)h[RBT_TC_N_CHANGED];
  return RBT_OK;
}
}  // namespace

// rgb != nullptr: rbt_reconstruct_rgb - the attribute pictures are up-converted to 4:4:4 on the device first (csrc/rbt_color.h), the colour fetch reads the three planes at the
// point's pixel (RbtPccParams.has_attr = 2) and the triples are converted to RGB8; stage_ms[0..1]: device time of the up-conversion and of the RGB conversion
static int reconstruct_impl(std::string& err, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, const uint16_t* occ, const uint16_t* d0, const uint16_t* d1, int geo_bd,
                            const uint16_t* t0, const uint16_t* t1, int attr_bd, rbt_cloud* out, int filter, uint8_t** rgb, double* stage_ms, int attr_transfer = 0, uint8_t** moved_out = nullptr,
                            int* n_changed = nullptr, DevCloud* keep_dev = nullptr, bool to_host = true) {
  const bool want_rgb = rgb != nullptr || keep_dev != nullptr;      // the colour path of rbt_reconstruct_rgb; to_host = false (with keep_dev): only the counts of *out are filled
  memset(out, 0, sizeof(*out));
  if (moved_out) *moved_out = nullptr;
  if (n_changed) *n_changed = 0;
  if (rgb) *rgb = nullptr;
  if (want_rgb) {
    if (!t0 || (a->map_count > 1 && !t1) || (attr_bd != 8 && attr_bd != 10) || (filter != RBT_UPSAMPLE_F0 && filter != RBT_UPSAMPLE_REPLICATE)) { err = "attribute pictures of 8 or 10 bits and a known up-sampling filter are needed"; return RBT_ERR_PARAM; }
  }
  const int W = a->width, H = a->height, res = a->occupancy_resolution, prec = a->occupancy_precision;
  if (W <= 0 || H <= 0 || res < 1 || prec < 1 || W % res || H % res || W % prec || H % prec || W % 2 || H % 2 || W > 8192 || H > 8192 || n_patches < 0 || n_patches > 65535 ||
      geo_bd < 8 || geo_bd > 16 || attr_bd < 8 || attr_bd > 16 || a->map_count < 1 || a->map_count > 2 || (a->map_count > 1 && !d1) || ((t0 != nullptr) != (t1 != nullptr) && a->map_count > 1) ||
      (a->geometry_smoothing && (a->grid_size < 2 || a->grid_size > 255 || a->threshold_smoothing < 0))) {
    err = "bad atlas parameters"; return RBT_ERR_PARAM; }
  // an odd grid is refused (rbt.h: "2..255, even"): pc_sm_skip keeps a point whose coordinate is g * w - (g - 1) / 2 - 1, the remainder of that modulo g is g / 2, so its
  // lower cell is w - 1 and pc_sm_mark / pc_sm_filter would touch cell w, outside the w^3 arrays. With an even grid the last point kept has remainder g / 2 - 1: cell w - 2.
  if (a->geometry_smoothing && a->grid_size % 2) { err = "grid_size must be even"; return RBT_ERR_PARAM; }
  const bool smooth = a->geometry_smoothing != 0, transfer = smooth && attr_transfer != 0, keep = transfer || (smooth && moved_out);   // keep: the cloud before smoothing stays
  RbtPccParams P; memset(&P, 0, sizeof(P));
  P.w = W; P.h = H; P.res = res; P.prec = prec; P.map_count = a->map_count; P.absolute_d1 = a->absolute_d1; P.remove_dup = a->remove_duplicate_points; P.threshold = a->threshold_lossy_om;
  P.geo_bd = geo_bd; P.attr_bd = attr_bd; P.bw = W / res; P.bh = H / res; P.ow = W / prec; P.n_patches = n_patches; P.has_attr = want_rgb ? 2 : t0 != nullptr;
  // every patch block must lie on the canvas (the reference exits otherwise, PCCPatch.cpp:238-245); items in the reference's visiting order
  std::vector<uint32_t> items;
  for (int pi = 0; pi < n_patches; pi++) {
    const rbt_patch& p = patches[pi];
    const bool swapped = p.orientation == RBT_OR_ROT90 || p.orientation == RBT_OR_ROT270 || p.orientation == RBT_OR_MROT90 || p.orientation == RBT_OR_SWAP;
    if (p.size_u0 < 1 || p.size_v0 < 1 || (long long)p.size_u0 * p.size_v0 > 65535 || p.orientation < 0 || p.orientation > RBT_OR_ROT90 || p.u0 < 0 || p.v0 < 0 ||
        p.u0 + (swapped ? p.size_v0 : p.size_u0) > P.bw || p.v0 + (swapped ? p.size_u0 : p.size_v0) > P.bh ||
        p.normal_axis < 0 || p.normal_axis > 2 || p.tangent_axis < 0 || p.tangent_axis > 2 || p.bitangent_axis < 0 || p.bitangent_axis > 2 ||
        p.normal_axis == p.tangent_axis || p.normal_axis == p.bitangent_axis || p.tangent_axis == p.bitangent_axis) { err = "patch outside the atlas or malformed"; return RBT_ERR_PARAM; }
    for (int vb = 0; vb < p.size_v0; vb++) for (int ub = 0; ub < p.size_u0; ub++) { int x, y; block_xy(p, ub, vb, &x, &y); if (x < 0 || y < 0 || x >= P.bw || y >= P.bh) { err = "patch block outside the atlas"; return RBT_ERR_PARAM; }
      items.push_back((uint32_t)pi << 16 | (uint32_t)(vb * p.size_u0 + ub)); }
  }
  const int n_items = (int)items.size();
  const size_t ys = (size_t)W * H, os = (size_t)(W / prec) * (H / prec), fs = ys * 3 / 2;
  DevBuf b_occ, b_d0, b_d1, b_t0, b_t1, b_patches, b_items, b_b2p, b_counts, b_off, b_om, b_xyz, b_yuv, b_meta, b_cells, b_scal, b_420, b_rgb, b_xyz0, b_yuv0, b_moved, b_labels;
  if (!b_occ.alloc(os * 2) || !b_d0.alloc(ys * 2) || !b_d1.alloc(ys * 2) || !b_patches.alloc(sizeof(rbt_patch) * (size_t)(n_patches ? n_patches : 1)) || !b_items.alloc(4 * (size_t)(n_items ? n_items : 1)) ||
      !b_b2p.alloc(4 * (size_t)P.bw * P.bh) || !b_counts.alloc(4 * (size_t)(n_items + 1)) || !b_off.alloc(4 * (size_t)(n_items + 1)) || !b_om.alloc(ys) ||
      (t0 && !want_rgb && (!b_t0.alloc(fs * 2) || !b_t1.alloc(fs * 2))) || (want_rgb && (!b_420.alloc(fs * 4) || !b_t0.alloc(ys * 12)))) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  int bad = rbtk::h2d(b_occ.p, occ, os * 2) | rbtk::h2d(b_d0.p, d0, ys * 2) | rbtk::h2d(b_d1.p, d1 ? d1 : d0, ys * 2);
  if (n_patches) bad |= rbtk::h2d(b_patches.p, patches, sizeof(rbt_patch) * (size_t)n_patches);
  if (n_items) bad |= rbtk::h2d(b_items.p, items.data(), 4 * (size_t)n_items);
  if (t0 && !want_rgb) bad |= rbtk::h2d(b_t0.p, t0, fs * 2) | rbtk::h2d(b_t1.p, t1 ? t1 : t0, fs * 2);
  if (want_rgb) bad |= rbtk::h2d(b_420.p, t0, fs * 2) | rbtk::h2d(b_420.as<uint16_t>() + fs, t1 ? t1 : t0, fs * 2);
  bad |= rbtk::dev_memset(b_b2p.p, 0, 4 * (size_t)P.bw * P.bh);
  if (bad) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  const uint16_t *p_t0 = b_t0.as<uint16_t>(), *p_t1 = b_t1.as<uint16_t>();
  if (want_rgb) {        // both pictures in one launch: 2 x 3 planes of W x H in b_t0
    rbtk::timer_begin(T_COL_UP); rbtk::launch_up444(b_420.as<uint16_t>(), W, H, attr_bd, 2, filter, b_t0.as<uint16_t>()); rbtk::timer_end(T_COL_UP);
    p_t1 = p_t0 + 3 * ys;
  }
  rbtk::launch_pcc_occmap(&P, b_occ.as<uint16_t>(), b_om.as<uint8_t>());
  rbtk::launch_pcc_owner(&P, b_patches.as<rbt_patch>(), b_items.as<uint32_t>(), n_items, b_occ.as<uint16_t>(), b_b2p.as<uint32_t>());
  rbtk::launch_pcc_count(&P, b_patches.as<rbt_patch>(), b_items.as<uint32_t>(), n_items, b_occ.as<uint16_t>(), b_d0.as<uint16_t>(), b_d1.as<uint16_t>(), b_b2p.as<uint32_t>(), b_counts.as<uint32_t>());
  rbtk::launch_scan_u32(b_counts.as<uint32_t>(), b_off.as<uint32_t>(), n_items);
  uint32_t total = 0;
  if (rbtk::d2h(&total, b_off.as<uint32_t>() + n_items, 4)) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  if (!b_xyz.alloc(6 * (size_t)(total ? total : 1)) || !b_yuv.alloc(6 * (size_t)(total ? total : 1)) || (smooth && (!b_meta.alloc(4 * (size_t)(total ? total : 1)) || !b_scal.alloc(64)))) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  rbtk::launch_pcc_emit(&P, b_patches.as<rbt_patch>(), b_items.as<uint32_t>(), n_items, b_occ.as<uint16_t>(), b_d0.as<uint16_t>(), b_d1.as<uint16_t>(), p_t0, p_t1,
                        b_b2p.as<uint32_t>(), b_off.as<uint32_t>(), b_xyz.as<int16_t>(), b_yuv.as<uint16_t>(), smooth ? b_om.as<uint8_t>() : nullptr, smooth ? b_meta.as<uint32_t>() : nullptr);
  out->n_points = (int)total;
  if (keep_dev) {                   // the patch of every point, by a kernel of its own over the items' offsets: the emit above is the kernel it was
    if (!b_labels.alloc(4 * (size_t)(total ? total : 1))) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
    rbtk::launch_pd_labels(b_items.as<uint32_t>(), b_off.as<uint32_t>(), n_items, b_labels.as<uint32_t>());
  }
  if (keep && total) {              // rbt_reconstruct_decoded: the cloud before smoothing stays on the device as the source of the attribute transfer
    if (!b_xyz0.alloc(6 * (size_t)total) || !b_yuv0.alloc(6 * (size_t)total) || !b_moved.alloc(total)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
    rbtk::timer_begin(T_COL_TRANSFER_COPY);
    rbtk::launch_tc_copy(b_xyz0.as<uint16_t>(), b_xyz.as<uint16_t>(), 3 * (size_t)total); rbtk::launch_tc_copy(b_yuv0.as<uint16_t>(), b_yuv.as<uint16_t>(), 3 * (size_t)total);
    rbtk::timer_end(T_COL_TRANSFER_COPY);
    if (rbtk::dev_memset(b_moved.p, 0, total)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  }
  // geometry smoothing (PCCCodec::smoothPointCloudPostprocess with gridSmoothing, PCCCodec.cpp:52-145): the grid spans the largest coordinate of the cloud (:70-83)
  if (smooth && total) {
    uint32_t* scal = b_scal.as<uint32_t>();                        // [0] largest coordinate, [1] points moved
    uint32_t maxv = 0;
    if (rbtk::dev_memset(scal, 0, 64)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
    rbtk::launch_sm_max(b_xyz.as<int16_t>(), (int)total, scal);
    if (rbtk::d2h(&maxv, scal, 4)) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
    RbtSmooth G; memset(&G, 0, sizeof(G));
    G.g = a->grid_size; G.w = ((int)maxv + G.g - 1) / G.g; G.disth = std::max(G.g / 2, 1); G.th = G.g * G.w; G.threshold = a->threshold_smoothing; G.n_points = (int)total;
    if (G.w > 0) {
      const size_t w3 = (size_t)G.w * G.w * G.w, o_sum = (w3 + 255) & ~(size_t)255, o_cnt = o_sum + 12 * w3, o_min = o_cnt + 4 * w3, o_max = o_min + 4 * w3, bytes = o_max + 4 * w3;
      if (!b_cells.alloc(bytes)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
      uint8_t* base = b_cells.as<uint8_t>();
      G.flag = base; G.sum = (uint32_t*)(base + o_sum); G.cnt = (uint32_t*)(base + o_cnt); G.pmin = (uint32_t*)(base + o_min); G.pmax = (uint32_t*)(base + o_max); G.moved = scal + 1;
      if (rbtk::dev_memset(base, 0, bytes) || rbtk::dev_memset(G.pmin, 0xFF, 4 * w3)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
      rbtk::launch_sm_passes(&G, b_xyz.as<int16_t>(), b_meta.as<uint32_t>());
      uint32_t moved[16];
      if (rbtk::d2h(moved, scal, 64)) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
      out->n_smoothed = (int)moved[1];
      if (transfer && moved[1]) {   // the flags are written inside the stage (and its events); a coordinate outside the 1024^3 volumes comes back as RBT_ERR_PARAM
        if (total < RBT_TC_K) { err = "fewer than 8 points"; return RBT_ERR_PARAM; }
        int changed = 0;
        const int rc = transfer_on_device(err, b_xyz0.as<int16_t>(), b_yuv0.as<uint16_t>(), (int)total, b_xyz.as<int16_t>(), b_yuv.as<uint16_t>(), b_moved.as<uint8_t>(), (int)total, (int)moved[1], &changed,
                                          &G, b_meta.as<uint32_t>());
        if (rc) return rc;
        if (n_changed) *n_changed = changed;
        if (stage_ms) stage_ms[3] = rbtk::timer_ms(T_COL_TRANSFER) + rbtk::timer_ms(T_COL_TRANSFER_COPY);
      } else if (keep) rbtk::launch_tc_flag(&G, b_xyz0.as<int16_t>(), b_meta.as<uint32_t>(), b_moved.as<uint8_t>());
    }
  }
  bad = 0;
  if (to_host) {
    out->xyz = (int16_t*)malloc(6 * (size_t)(total ? total : 1)); out->yuv = (uint16_t*)malloc(6 * (size_t)(total ? total : 1));
    out->occupancy_map = (uint8_t*)malloc(ys); out->block_to_patch = (uint32_t*)malloc(4 * (size_t)P.bw * P.bh);
    if (!out->xyz || !out->yuv || !out->occupancy_map || !out->block_to_patch) { err = "out of memory"; return RBT_ERR_NOMEM; }
    bad = rbtk::d2h(out->occupancy_map, b_om.p, ys) | rbtk::d2h(out->block_to_patch, b_b2p.p, 4 * (size_t)P.bw * P.bh);
    if (total) bad |= rbtk::d2h(out->xyz, b_xyz.p, 6 * (size_t)total) | rbtk::d2h(out->yuv, b_yuv.p, 6 * (size_t)total);
  }
  if (moved_out) {
    *moved_out = (uint8_t*)calloc(total ? total : 1, 1);
    if (!*moved_out) { err = "out of memory"; return RBT_ERR_NOMEM; }
    if (b_moved.p && total) bad |= rbtk::d2h(*moved_out, b_moved.p, total);
  }
  if (want_rgb) {
    if (!b_rgb.alloc(3 * (size_t)(total ? total : 1))) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
    rbtk::timer_begin(T_COL_RGB); rbtk::launch_yuv16_rgb8(b_yuv.as<uint16_t>(), (int)total, b_rgb.as<uint8_t>()); rbtk::timer_end(T_COL_RGB);
    if (rgb) {
      *rgb = (uint8_t*)malloc(3 * (size_t)(total ? total : 1));
      if (!*rgb) { err = "out of memory"; return RBT_ERR_NOMEM; }
      if (total) bad |= rbtk::d2h(*rgb, b_rgb.p, 3 * (size_t)total);
    }
  }
  if (bad || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  if (want_rgb && stage_ms) { stage_ms[0] = rbtk::timer_ms(T_COL_UP); stage_ms[1] = rbtk::timer_ms(T_COL_RGB); }
  if (keep_dev) { keep_dev->xyz.take(b_xyz); keep_dev->yuv.take(b_yuv); keep_dev->rgb.take(b_rgb); keep_dev->labels.take(b_labels); }
  return RBT_OK;
}
int pcc_reconstruct(std::string& err, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, const uint16_t* occ, const uint16_t* d0, const uint16_t* d1, int geo_bd,
                    const uint16_t* t0, const uint16_t* t1, int attr_bd, rbt_cloud* out) {
  return reconstruct_impl(err, a, patches, n_patches, occ, d0, d1, geo_bd, t0, t1, attr_bd, out, 0, nullptr, nullptr);
}
int pcc_reconstruct_rgb(std::string& err, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, const uint16_t* occ, const uint16_t* d0, const uint16_t* d1, int geo_bd,
                        const uint16_t* t0, const uint16_t* t1, int attr_bd, int filter, rbt_cloud* out, uint8_t** rgb, double* stage_ms) {
  return reconstruct_impl(err, a, patches, n_patches, occ, d0, d1, geo_bd, t0, t1, attr_bd, out, filter, rgb, stage_ms);
}

int pcc_reconstruct_decoded(std::string& err, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, const uint16_t* occ, const uint16_t* d0, const uint16_t* d1, int geo_bd,
                            const uint16_t* t0, const uint16_t* t1, int attr_bd, int filter, int attr_transfer, rbt_cloud* out, uint8_t** rgb, uint8_t** moved, int* n_changed, double* stage_ms) {
  return reconstruct_impl(err, a, patches, n_patches, occ, d0, d1, geo_bd, t0, t1, attr_bd, out, filter, rgb, stage_ms, attr_transfer, moved, n_changed);
}

// the stage on its own (rbt_transfer_colors): host clouds in, the target's colours updated in place
int pcc_transfer_colors(std::string& err, const int16_t* sxyz, const uint16_t* syuv, int ns, const int16_t* txyz, uint16_t* tyuv, const uint8_t* moved, int nt, int* n_changed, double* ms) {
  *n_changed = 0;
  if (ns < RBT_TC_K || nt < 0 || ns > (1 << 26) || nt > (1 << 26)) { err = "at least 8 source points (and at most 2^26 points a cloud) are needed"; return RBT_ERR_PARAM; }
  for (size_t i = 0; i < 3 * (size_t)ns; i++) if (sxyz[i] < 0 || sxyz[i] >= RBT_PCC_DIM) { err = "coordinate outside 0..1023"; return RBT_ERR_PARAM; }
  for (size_t i = 0; i < 3 * (size_t)nt; i++) if (txyz[i] < 0 || txyz[i] >= RBT_PCC_DIM) { err = "coordinate outside 0..1023"; return RBT_ERR_PARAM; }
  std::vector<uint8_t> flag((size_t)nt); int n_moved = 0;
  for (int i = 0; i < nt; i++) { flag[i] = moved[i] != 0; n_moved += flag[i]; }
  if (!n_moved) return RBT_OK;
  DevBuf b_sx, b_sc, b_tx, b_tc, b_m;
  if (!b_sx.alloc(6 * (size_t)ns) || !b_sc.alloc(6 * (size_t)ns) || !b_tx.alloc(6 * (size_t)nt) || !b_tc.alloc(6 * (size_t)nt) || !b_m.alloc((size_t)nt)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  if (rbtk::h2d(b_sx.p, sxyz, 6 * (size_t)ns) | rbtk::h2d(b_sc.p, syuv, 6 * (size_t)ns) | rbtk::h2d(b_tx.p, txyz, 6 * (size_t)nt) | rbtk::h2d(b_tc.p, tyuv, 6 * (size_t)nt) | rbtk::h2d(b_m.p, flag.data(), (size_t)nt)) {
    err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  const int rc = transfer_on_device(err, b_sx.as<int16_t>(), b_sc.as<uint16_t>(), ns, b_tx.as<int16_t>(), b_tc.as<uint16_t>(), b_m.as<uint8_t>(), nt, n_moved, n_changed);
  if (rc) return rc;
  if (rbtk::d2h(tyuv, b_tc.p, 6 * (size_t)nt) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  if (ms) *ms = rbtk::timer_ms(T_COL_TRANSFER);
  return RBT_OK;
}

int pcc_yuv420_to_yuv444(std::string& err, const uint16_t* in, int w, int h, int bd, int n_frames, int filter, uint16_t* out, double* ms) {
  if (w <= 0 || h <= 0 || w % 2 || h % 2 || w > 16384 || h > 16384 || n_frames < 1 || n_frames > 21845 || (bd != 8 && bd != 10) || (filter != RBT_UPSAMPLE_F0 && filter != RBT_UPSAMPLE_REPLICATE)) {
    err = "even picture size, bit depth 8 or 10 and a known up-sampling filter are needed"; return RBT_ERR_PARAM; }
  const size_t ys = (size_t)w * h, fs = ys * 3 / 2;
  DevBuf b_in, b_out;
  if (!b_in.alloc(fs * 2 * n_frames) || !b_out.alloc(ys * 6 * n_frames)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  if (rbtk::h2d(b_in.p, in, fs * 2 * n_frames)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  rbtk::timer_begin(T_COL_UP); rbtk::launch_up444(b_in.as<uint16_t>(), w, h, bd, n_frames, filter, b_out.as<uint16_t>()); rbtk::timer_end(T_COL_UP);
  if (rbtk::d2h(out, b_out.p, ys * 6 * n_frames) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  if (ms) *ms = rbtk::timer_ms(T_COL_UP);
  return RBT_OK;
}
int pcc_yuv16_to_rgb8(std::string& err, const uint16_t* yuv, int n, uint8_t* rgb, double* ms) {
  if (n < 1) { err = "no points"; return RBT_ERR_PARAM; }
  DevBuf b_in, b_out;
  if (!b_in.alloc(6 * (size_t)n) || !b_out.alloc(3 * (size_t)n)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  if (rbtk::h2d(b_in.p, yuv, 6 * (size_t)n)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  rbtk::timer_begin(T_COL_RGB); rbtk::launch_yuv16_rgb8(b_in.as<uint16_t>(), n, b_out.as<uint8_t>()); rbtk::timer_end(T_COL_RGB);
  if (rbtk::d2h(rgb, b_out.p, 3 * (size_t)n) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  if (ms) *ms = rbtk::timer_ms(T_COL_RGB);
  return RBT_OK;
}

// ---- clouds that stay on the device, and their scoring (csrc/rbt_score.h) ----
struct PCloud {
  int n = 0, n_merged = 0, lg = 0; bool indexed = false;
  DevBuf xyz, rgb, yuv, nrm, labels, maps, scal; void* vol = nullptr;
  int label_bound = 0;                                                     // > 0: every label is below it by construction (a cloud made from maps: its patch count); 0: not known             // vol: the bit volume with the coarse level behind it; taken from / returned to the context's cache
  RbtScoreCloud view() const {
    uint32_t* m = maps.as<uint32_t>(); const size_t slots = (size_t)1 << lg;
    return RbtScoreCloud{xyz.as<int16_t>(), rgb.as<uint8_t>(), nrm.as<int16_t>(), n, lg, (uint32_t*)vol, (uint32_t*)vol + (PCLOUD_VOL_BYTES - 4 * (size_t)RBT_SC_COARSE_WORDS) / 4, m, m + slots, m + 2 * slots, m + 6 * slots};
  }
};
static_assert(PCLOUD_VOL_BYTES == ((size_t)1 << (3 * RBT_PCC_BITS - 3)) + 4 * (size_t)RBT_SC_COARSE_WORDS, "volume + coarse level");
void pcloud_cache_trim(PCloudCache& cache) { for (void* v : cache.vols) rbtk::dev_free(v); cache.vols.clear(); }
bool pcloud_has_colors(const PCloud* c) { return c->rgb.p != nullptr; }
int pcloud_merged(const PCloud* c) { return c->n_merged; }
void pcloud_points(const PCloud* c, int* n_points, int* n_merged) { if (n_points) *n_points = c->n; if (n_merged) *n_merged = c->n_merged; }
// The cloud's own volume and coarse words go back to zero and the clean volume to the cache; the maps and the point arrays go back to the device pool.
void pcloud_release(PCloudCache& cache, PCloud* c) {
  if (!c) return;
  if (c->vol) {
    bool clean = true;
    if (c->indexed) { const RbtScoreCloud S = c->view(); rbtk::launch_sc_clear(&S); clean = rbtk::dev_sync() == 0; }
    if (clean) cache.vols.push_back(c->vol); else rbtk::dev_free(c->vol);
  }
  delete c;
}
// xyz (and whatever else the cloud has) is on the device already: check, take a volume, build the index
static int pcloud_index(std::string& err, PCloudCache& cache, PCloud* c) {
  if (c->n > (1 << 26)) { err = "more than 2^26 points"; return RBT_ERR_PARAM; }
  c->lg = lg_of(c->n);
  const size_t slots = (size_t)1 << c->lg;
  if (!c->scal.alloc(4 * RBT_SC_SCALARS) || !c->maps.alloc(4 * 7 * slots)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  uint32_t h[RBT_SC_SCALARS];
  if (rbtk::dev_memset(c->scal.p, 0, sizeof(h))) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  rbtk::launch_sc_check(c->xyz.as<int16_t>(), c->n, c->scal.as<uint32_t>());
  if (rbtk::d2h(h, c->scal.p, sizeof(h)) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  if (h[RBT_SC_ERR]) { err = "coordinate outside 0..1023"; return RBT_ERR_PARAM; }       // nothing of a volume has been touched
  if (!cache.vols.empty()) { c->vol = cache.vols.back(); cache.vols.pop_back(); }
  else {
    c->vol = rbtk::dev_alloc(PCLOUD_VOL_BYTES);
    if (!c->vol) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
    if (rbtk::dev_memset(c->vol, 0, PCLOUD_VOL_BYTES)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  }
  uint32_t* m = c->maps.as<uint32_t>();
  if (rbtk::dev_memset(m, 0, 4 * slots) | rbtk::dev_memset(m + slots, 0xFF, 4 * slots) | rbtk::dev_memset(m + 2 * slots, 0, 4 * 5 * slots)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  const RbtScoreCloud S = c->view();
  c->indexed = true;
  rbtk::launch_sc_index(&S, c->scal.as<uint32_t>());
  if (rbtk::d2h(h, c->scal.p, sizeof(h)) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  c->n_merged = (int)h[RBT_SC_N_MERGED];
  return RBT_OK;
}
int pcloud_upload(std::string& err, PCloudCache& cache, const int16_t* xyz, const uint8_t* rgb, const int16_t* nrm, int n, PCloud** out) {
  *out = nullptr;
  if (n <= 0) { err = "empty point cloud"; return RBT_ERR_PARAM; }
  PCloud* c = new PCloud(); c->n = n;
  int rc = RBT_OK;
  if (!c->xyz.alloc(6 * (size_t)n) || (rgb && !c->rgb.alloc(3 * (size_t)n)) || (nrm && !c->nrm.alloc(6 * (size_t)n))) { err = "device allocation failed"; rc = RBT_ERR_NOMEM; }
  else if (rbtk::h2d(c->xyz.p, xyz, 6 * (size_t)n) | (rgb ? rbtk::h2d(c->rgb.p, rgb, 3 * (size_t)n) : 0) | (nrm ? rbtk::h2d(c->nrm.p, nrm, 6 * (size_t)n) : 0)) { err = "device transfer failed"; rc = RBT_ERR_NO_DEVICE; }
  else rc = pcloud_index(err, cache, c);
  if (rc) { pcloud_release(cache, c); return rc; }
  *out = c;
  return RBT_OK;
}
int pcloud_from_maps(std::string& err, PCloudCache& cache, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, const uint16_t* occ, const uint16_t* d0, const uint16_t* d1, int geo_bd,
                     const uint16_t* t0, const uint16_t* t1, int attr_bd, int filter, int attr_transfer, PCloud** out, rbt_cloud* host_copy, uint8_t** rgb, int* n_changed, double* stage_ms) {
  *out = nullptr;
  DevCloud dev; rbt_cloud counts;
  int rc = reconstruct_impl(err, a, patches, n_patches, occ, d0, d1, geo_bd, t0, t1, attr_bd, host_copy ? host_copy : &counts, filter, rgb, stage_ms, attr_transfer, nullptr, n_changed, &dev, host_copy != nullptr);
  if (rc) return rc;
  const int n = (host_copy ? host_copy : &counts)->n_points;
  if (n <= 0) { err = "empty point cloud"; return RBT_ERR_PARAM; }
  PCloud* c = new PCloud(); c->n = n;
  c->xyz.take(dev.xyz); c->yuv.take(dev.yuv); c->rgb.take(dev.rgb); c->labels.take(dev.labels); c->label_bound = n_patches;
  rc = pcloud_index(err, cache, c);
  if (rc) { pcloud_release(cache, c); return rc; }
  *out = c;
  return RBT_OK;
}
// ---- positions-only reconstruction from device planes (rbt_submit_gof_d1; rbt_pcc.h) ----
// The checks reconstruct_impl makes on the atlas and the patches, for a call without attribute pictures; items in the reference's visiting order
int mapframe_check(std::string& err, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, std::vector<uint32_t>* items) {
  const int W = a->width, H = a->height, res = a->occupancy_resolution, prec = a->occupancy_precision;
  if (W <= 0 || H <= 0 || res < 1 || prec < 1 || W % res || H % res || W % prec || H % prec || W % 2 || H % 2 || W > 8192 || H > 8192 || n_patches < 0 || n_patches > 65535 ||
      a->map_count < 1 || a->map_count > 2 || (a->geometry_smoothing && (a->grid_size < 2 || a->grid_size > 255 || a->threshold_smoothing < 0))) { err = "bad atlas parameters"; return RBT_ERR_PARAM; }
  if (a->geometry_smoothing && a->grid_size % 2) { err = "grid_size must be even"; return RBT_ERR_PARAM; }
  const int bw = W / res, bh = H / res;
  for (int pi = 0; pi < n_patches; pi++) {
    const rbt_patch& p = patches[pi];
    const bool swapped = p.orientation == RBT_OR_ROT90 || p.orientation == RBT_OR_ROT270 || p.orientation == RBT_OR_MROT90 || p.orientation == RBT_OR_SWAP;
    if (p.size_u0 < 1 || p.size_v0 < 1 || (long long)p.size_u0 * p.size_v0 > 65535 || p.orientation < 0 || p.orientation > RBT_OR_ROT90 || p.u0 < 0 || p.v0 < 0 ||
        p.u0 + (swapped ? p.size_v0 : p.size_u0) > bw || p.v0 + (swapped ? p.size_u0 : p.size_v0) > bh ||
        p.normal_axis < 0 || p.normal_axis > 2 || p.tangent_axis < 0 || p.tangent_axis > 2 || p.bitangent_axis < 0 || p.bitangent_axis > 2 ||
        p.normal_axis == p.tangent_axis || p.normal_axis == p.bitangent_axis || p.tangent_axis == p.bitangent_axis) { err = "patch outside the atlas or malformed"; return RBT_ERR_PARAM; }
    for (int vb = 0; vb < p.size_v0; vb++) for (int ub = 0; ub < p.size_u0; ub++) { int x, y; block_xy(p, ub, vb, &x, &y); if (x < 0 || y < 0 || x >= bw || y >= bh) { err = "patch block outside the atlas"; return RBT_ERR_PARAM; }
      if (items) items->push_back((uint32_t)pi << 16 | (uint32_t)(vb * p.size_u0 + ub)); }
  }
  return RBT_OK;
}
struct MapFrame {
  rbt_atlas_params a; RbtPccParams P; int n_items = 0; const uint16_t* d_occ = nullptr;
  std::vector<uint32_t> items; std::vector<rbt_patch> patches;      // host staging of the two uploads, alive as long as the frame
  DevBuf b_patches, b_items, b_b2p, b_om, b_counts, b_off;
};
void mapframe_delete(MapFrame* f) { delete f; }
size_t mapframe_bytes(const rbt_atlas_params* a, int n_patches) {
  const size_t res = (size_t)(a->occupancy_resolution > 0 ? a->occupancy_resolution : 1), blocks = (size_t)a->width / res * ((size_t)a->height / res);
  return sizeof(rbt_patch) * (size_t)(n_patches > 0 ? n_patches : 1) + 4 * blocks + (size_t)a->width * (size_t)a->height;
}
int mapframe_new(std::string& err, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, const uint16_t* d_occ, MapFrame** out) {
  *out = nullptr;
  std::unique_ptr<MapFrame> F(new MapFrame());
  if (int rc = mapframe_check(err, a, patches, n_patches, &F->items)) return rc;
  F->a = *a; F->d_occ = d_occ; F->n_items = (int)F->items.size(); F->patches.assign(patches, patches + n_patches);
  RbtPccParams& P = F->P; memset(&P, 0, sizeof(P));
  P.w = a->width; P.h = a->height; P.res = a->occupancy_resolution; P.prec = a->occupancy_precision; P.map_count = a->map_count; P.absolute_d1 = a->absolute_d1; P.remove_dup = a->remove_duplicate_points;
  P.threshold = a->threshold_lossy_om; P.geo_bd = 8; P.attr_bd = 8; P.bw = P.w / P.res; P.bh = P.h / P.res; P.ow = P.w / P.prec; P.n_patches = n_patches; P.has_attr = 0;
  const int n_items = F->n_items; const size_t ys = (size_t)P.w * P.h;
  if (!F->b_patches.alloc(sizeof(rbt_patch) * (size_t)(n_patches ? n_patches : 1)) || !F->b_items.alloc(4 * (size_t)(n_items ? n_items : 1)) || !F->b_b2p.alloc(4 * (size_t)P.bw * P.bh) ||
      !F->b_counts.alloc(4 * (size_t)(n_items + 1)) || !F->b_off.alloc(4 * (size_t)(n_items + 1)) || !F->b_om.alloc(ys)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  int bad = rbtk::dev_memset(F->b_b2p.p, 0, 4 * (size_t)P.bw * P.bh);
  if (n_patches) bad |= rbtk::h2d(F->b_patches.p, F->patches.data(), sizeof(rbt_patch) * (size_t)n_patches);
  if (n_items) bad |= rbtk::h2d(F->b_items.p, F->items.data(), 4 * (size_t)n_items);
  if (bad) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  rbtk::launch_pcc_occmap(&P, d_occ, F->b_om.as<uint8_t>());
  rbtk::launch_pcc_owner(&P, F->b_patches.as<rbt_patch>(), F->b_items.as<uint32_t>(), n_items, d_occ, F->b_b2p.as<uint32_t>());
  *out = F.release();
  return RBT_OK;
}
// The positions of one pair of geometry planes, as reconstruct_impl makes them: count, scan, emit, and geometry smoothing where the atlas asks for it. xyz / yuv are
// allocated here (yuv: the triples the emit writes, grey without attribute pictures). keep_xyz0 / keep_moved (both or neither; smoothing only): the positions before
// smoothing and, where points moved and `flags` is set, the per-point moved flags (k_tc_flag, while the grid's cells are alive). One routine for mapframe_cloud and
// colorframe_new: the grid's sizing lives here and in reconstruct_impl.
static int mapframe_points(std::string& err, const MapFrame* F, const RbtPccParams& P, const uint16_t* d0, const uint16_t* d1, DevBuf& xyz, DevBuf& yuv, DevBuf* keep_xyz0, DevBuf* keep_moved, bool flags,
                           int* n_points, int* n_moved, DevBuf* labels = nullptr) {
  *n_points = 0; *n_moved = 0;
  const rbt_atlas_params* a = &F->a; const int n_items = F->n_items; const bool smooth = a->geometry_smoothing != 0;
  const rbt_patch* patches = F->b_patches.as<rbt_patch>(); const uint32_t *items = F->b_items.as<uint32_t>(), *b2p = F->b_b2p.as<uint32_t>();
  rbtk::launch_pcc_count(&P, patches, items, n_items, F->d_occ, d0, d1, b2p, F->b_counts.as<uint32_t>());
  rbtk::launch_scan_u32(F->b_counts.as<uint32_t>(), F->b_off.as<uint32_t>(), n_items);
  uint32_t total = 0;
  if (rbtk::d2h(&total, F->b_off.as<uint32_t>() + n_items, 4)) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  if (!total) { err = "empty point cloud"; return RBT_ERR_PARAM; }
  DevBuf b_meta, b_scal, b_cells;
  if (!xyz.alloc(6 * (size_t)total) || !yuv.alloc(6 * (size_t)total) || (smooth && (!b_meta.alloc(4 * (size_t)total) || !b_scal.alloc(64))) ||
      (smooth && keep_xyz0 && (!keep_xyz0->alloc(6 * (size_t)total) || !keep_moved->alloc(total)))) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  rbtk::launch_pcc_emit(&P, patches, items, n_items, F->d_occ, d0, d1, nullptr, nullptr, b2p, F->b_off.as<uint32_t>(), xyz.as<int16_t>(), yuv.as<uint16_t>(),
                        smooth ? F->b_om.as<uint8_t>() : nullptr, smooth ? b_meta.as<uint32_t>() : nullptr);
  if (labels) {                     // the patch of every point (smoothing moves points, it changes neither their order nor their patch)
    if (!labels->alloc(4 * (size_t)total)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
    rbtk::launch_pd_labels(items, F->b_off.as<uint32_t>(), n_items, labels->as<uint32_t>());
  }
  *n_points = (int)total;
  if (!smooth) return RBT_OK;
  if (keep_xyz0) {
    rbtk::launch_tc_copy(keep_xyz0->as<uint16_t>(), xyz.as<uint16_t>(), 3 * (size_t)total);
    if (rbtk::dev_memset(keep_moved->p, 0, total)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  }
  uint32_t* scal = b_scal.as<uint32_t>(); uint32_t maxv = 0;                        // [0] largest coordinate, [1] points moved
  if (rbtk::dev_memset(scal, 0, 64)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  rbtk::launch_sm_max(xyz.as<int16_t>(), (int)total, scal);
  if (rbtk::d2h(&maxv, scal, 4)) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  RbtSmooth G; memset(&G, 0, sizeof(G));
  G.g = a->grid_size; G.w = ((int)maxv + G.g - 1) / G.g; G.disth = std::max(G.g / 2, 1); G.th = G.g * G.w; G.threshold = a->threshold_smoothing; G.n_points = (int)total;
  if (G.w <= 0) return RBT_OK;
  const size_t w3 = (size_t)G.w * G.w * G.w, o_sum = (w3 + 255) & ~(size_t)255, o_cnt = o_sum + 12 * w3, o_min = o_cnt + 4 * w3, o_max = o_min + 4 * w3, bytes = o_max + 4 * w3;
  if (!b_cells.alloc(bytes)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  uint8_t* base = b_cells.as<uint8_t>();
  G.flag = base; G.sum = (uint32_t*)(base + o_sum); G.cnt = (uint32_t*)(base + o_cnt); G.pmin = (uint32_t*)(base + o_min); G.pmax = (uint32_t*)(base + o_max); G.moved = scal + 1;
  if (rbtk::dev_memset(base, 0, bytes) || rbtk::dev_memset(G.pmin, 0xFF, 4 * w3)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  rbtk::launch_sm_passes(&G, xyz.as<int16_t>(), b_meta.as<uint32_t>());
  uint32_t moved[16];
  if (rbtk::d2h(moved, scal, 64)) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  *n_moved = (int)moved[1];
  if (keep_xyz0 && flags && moved[1]) {
    if (total < RBT_TC_K) { err = "fewer than 8 points"; return RBT_ERR_PARAM; }
    rbtk::launch_tc_flag(&G, keep_xyz0->as<int16_t>(), b_meta.as<uint32_t>(), keep_moved->as<uint8_t>());
    if (rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }      // the cells go with this scope
  }
  return RBT_OK;
}
// the cloud of one pair of geometry planes: the positions (mapframe_points), index
int mapframe_cloud(std::string& err, PCloudCache& cache, const MapFrame* F, const uint16_t* d0, const uint16_t* d1, int geo_bd, PCloud** out, int* n_smoothed) {
  *out = nullptr; if (n_smoothed) *n_smoothed = 0;
  if (geo_bd < 8 || geo_bd > 16) { err = "bad atlas parameters"; return RBT_ERR_PARAM; }
  RbtPccParams P = F->P; P.geo_bd = geo_bd; P.attr_bd = geo_bd;
  DevBuf b_xyz, b_yuv, b_labels; int total = 0, moved = 0;
  if (int rc = mapframe_points(err, F, P, d0, d1 ? d1 : d0, b_xyz, b_yuv, nullptr, nullptr, false, &total, &moved, &b_labels)) return rc;
  if (n_smoothed) *n_smoothed = moved;
  PCloud* c = new PCloud(); c->n = total;
  c->xyz.take(b_xyz); c->labels.take(b_labels); c->label_bound = P.n_patches;
  if (int rc = pcloud_index(err, cache, c)) { pcloud_release(cache, c); return rc; }      // (waits for the stream: the buffers that go out of scope here are idle)
  *out = c;
  return RBT_OK;
}
// ---- recolouring a frame's cloud per trial (rbt_submit_gof_color; rbt_pcc.h) ----
// The geometry half of one frame, made once: what reconstruct_impl does with the occupancy and geometry planes - count, scan, emit, smoothing with the per-point moved
// flags - and the index of the final cloud. Kept: the frame's maps and offsets (the colour half emits again, against the trial's 4:4:4 planes), the positions before and
// after smoothing, the flags.
struct ColorFrame {
  MapFrame* maps = nullptr; RbtPccParams P; const uint16_t* d0 = nullptr; const uint16_t* d1 = nullptr;
  int total = 0, n_moved = 0, n_changed = 0; bool transfer = false;
  DevBuf xyz0, moved, scratch_xyz, yuv0, yuv; PCloud* cloud = nullptr; ScorePair* pair = nullptr;
};
void colorframe_delete(PCloudCache& cache, ColorFrame* f) {
  if (!f) return;
  score_pair_release(f->pair); pcloud_release(cache, f->cloud); mapframe_delete(f->maps);
  delete f;
}
void colorframe_upconvert(const uint16_t* d_420, int w, int h, int bit_depth, int n_pictures, int filter, uint16_t* d_444) { rbtk::launch_up444(d_420, w, h, bit_depth, n_pictures, filter, d_444); }
const PCloud* colorframe_cloud(const ColorFrame* f) { return f->cloud; }
int colorframe_changed(const ColorFrame* f) { return f->n_changed; }
size_t colorframe_bytes(const rbt_atlas_params* a, int n_patches) {      // but for its volume: maps, and per possible point positions twice, flags, triples twice, the index's maps
  const size_t pts = (size_t)a->width * (size_t)a->height * (size_t)a->map_count;
  return mapframe_bytes(a, n_patches) + pts * (6 + 6 + 1 + 6 + 6 + 6 + 3 + 4 + 2 * 28);
}
int colorframe_new(std::string& err, PCloudCache& cache, const rbt_atlas_params* a, const rbt_patch* patches, int n_patches, const uint16_t* d_occ, const uint16_t* d_d0, const uint16_t* d_d1,
                   int geo_bd, int attr_transfer, ColorFrame** out) {
  *out = nullptr;
  if (geo_bd < 8 || geo_bd > 16) { err = "bad atlas parameters"; return RBT_ERR_PARAM; }
  struct Guard { PCloudCache& cache; ColorFrame* f; ~Guard() { colorframe_delete(cache, f); } } g{cache, new ColorFrame()};
  ColorFrame* F = g.f;
  if (int rc = mapframe_new(err, a, patches, n_patches, d_occ, &F->maps)) return rc;
  F->P = F->maps->P; F->P.geo_bd = geo_bd; F->P.attr_bd = geo_bd; F->d0 = d_d0; F->d1 = d_d1 ? d_d1 : d_d0;
  DevBuf b_xyz, b_labels;      // (the labels: the colour figures per patch read them, as the D1 route's clouds carry them)
  if (int rc = mapframe_points(err, F->maps, F->P, F->d0, F->d1, b_xyz, F->yuv0, &F->xyz0, &F->moved, attr_transfer != 0, &F->total, &F->n_moved, &b_labels)) return rc;
  F->transfer = a->geometry_smoothing != 0 && attr_transfer != 0 && F->n_moved != 0;
  const size_t total = (size_t)F->total;
  PCloud* c = new PCloud(); c->n = F->total; c->xyz.take(b_xyz); c->labels.take(b_labels); c->label_bound = F->P.n_patches;
  F->cloud = c;
  if (!F->yuv.alloc(6 * total) || !F->scratch_xyz.alloc(6 * total) || !c->rgb.alloc(3 * total)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  if (rbtk::dev_memset(c->rgb.p, 0, 3 * total)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  if (int rc = pcloud_index(err, cache, c)) return rc;                  // (waits for the stream: the buffers that went out of scope above were idle)
  *out = F; g.f = nullptr;
  return RBT_OK;
}
// The colour half for one trial: t0 / t1 = the 4:4:4 planes (3 x W x H each) of the frame's attribute pictures. Emit once more for the colours, transfer, RGB, recolour.
int colorframe_color(std::string& err, ColorFrame* F, const uint16_t* t0, const uint16_t* t1, int attr_bd) {
  const MapFrame* M = F->maps; const size_t n = (size_t)F->total;
  RbtPccParams P = F->P; P.attr_bd = attr_bd; P.has_attr = 2;
  uint16_t* colours = F->transfer ? F->yuv0.as<uint16_t>() : F->yuv.as<uint16_t>();
  rbtk::launch_pcc_emit(&P, M->b_patches.as<rbt_patch>(), M->b_items.as<uint32_t>(), M->n_items, M->d_occ, F->d0, F->d1, t0, t1 ? t1 : t0, M->b_b2p.as<uint32_t>(), M->b_off.as<uint32_t>(),
                        F->scratch_xyz.as<int16_t>(), colours, nullptr, nullptr);
  F->n_changed = 0;
  if (F->transfer) {
    rbtk::launch_tc_copy(F->yuv.as<uint16_t>(), F->yuv0.as<uint16_t>(), 3 * n);
    if (int rc = transfer_on_device(err, F->xyz0.as<int16_t>(), F->yuv0.as<uint16_t>(), F->total, F->cloud->xyz.as<int16_t>(), F->yuv.as<uint16_t>(), F->moved.as<uint8_t>(), F->total, F->n_moved, &F->n_changed)) return rc;
  }
  rbtk::launch_yuv16_rgb8(F->yuv.as<uint16_t>(), F->total, F->cloud->rgb.as<uint8_t>());
  const RbtScoreCloud S = F->cloud->view();
  rbtk::launch_sc_recolor(&S);
  return RBT_OK;
}
int colorframe_pair(std::string& err, ColorFrame* F, const PCloud* ref) { score_pair_release(F->pair); F->pair = nullptr; return score_pair_create(err, ref, F->cloud, &F->pair); }
int colorframe_score(std::string& err, const ColorFrame* F, rbt_color_result* out) { return score_pair_color(err, F->pair, out); }
int colorframe_score_patches(std::string& err, const ColorFrame* F, int n_patches, rbt_patch_color* out, rbt_color_result* whole) { return score_pair_patches_color(err, F->pair, n_patches, out, whole); }

int pcloud_d1(std::string& err, const PCloud* a, const PCloud* b, int peak, rbt_d1_result* out) {
  rbt_frame_score s;
  const int rc = pcloud_score(err, a, b, peak, RBT_SCORE_D1, &s);
  *out = s.d1;
  return rc;
}
int gather_luma_host(std::string& err, const uint16_t* src, int n_pics, int stride, int rows, int x0, int y0, int w, int h, int src_misalign, uint16_t* out) {
  if (n_pics < 1 || w < 1 || h < 1 || x0 < 0 || y0 < 0 || stride < 1 || rows < 1 || x0 + w > stride || y0 + h > rows || stride > 16384 || rows > 16384 || src_misalign < 0 || src_misalign > 7) {
    err = "the window must lie inside planes of at most 16384 x 16384 samples, src_misalign in 0..7"; return RBT_ERR_PARAM; }
  const size_t plane = (size_t)stride * rows, in_n = plane * (size_t)n_pics, out_n = (size_t)w * h * (size_t)n_pics, in_bytes = ((in_n + 8) * 2 + 255) & ~(size_t)255;
  DevBuf buf, desc;
  if (!buf.alloc(256 + in_bytes + out_n * 2) || !desc.alloc(sizeof(RbtGatherPic) * (size_t)n_pics)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  uint8_t* base = (uint8_t*)(((uintptr_t)buf.p + 255) & ~(uintptr_t)255);
  uint16_t* d_in = (uint16_t*)base + src_misalign; uint16_t* d_out = (uint16_t*)(base + in_bytes);
  std::vector<RbtGatherPic> pics((size_t)n_pics);
  for (int k = 0; k < n_pics; k++) pics[k] = RbtGatherPic{d_in + plane * (size_t)k + (size_t)y0 * stride + x0, d_out + (size_t)w * h * (size_t)k, w, h, stride, 0};
  if (rbtk::h2d(d_in, src, in_n * 2) | rbtk::h2d(desc.p, pics.data(), sizeof(RbtGatherPic) * (size_t)n_pics) | rbtk::dev_memset(d_out, 0xEE, out_n * 2)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  rbtk::launch_gather_luma(desc.as<RbtGatherPic>(), n_pics, RBT_GM_PIC_CHUNKS(w, h));
  if (rbtk::d2h(out, d_out, out_n * 2) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  return RBT_OK;
}

// A picture of src: the luma plane (stride x rows), then Cb and Cr (cstride x crows each). Three descriptors a picture - the chroma windows are half the luma window in
// both directions, with a stride of their own - so chroma rows of 1, 7 or 36 samples go through gm_chunk as luma rows do.
int gather_420_host(std::string& err, const uint16_t* src, int n_pics, int stride, int rows, int cstride, int crows, int x0, int y0, int w, int h, int src_misalign, uint16_t* out) {
  if (n_pics < 1 || w < 2 || h < 2 || (w | h | x0 | y0) & 1 || x0 < 0 || y0 < 0 || stride < 1 || rows < 1 || cstride < 1 || crows < 1 || x0 + w > stride || y0 + h > rows ||
      (x0 + w) / 2 > cstride || (y0 + h) / 2 > crows || stride > 16384 || rows > 16384 || cstride > 16384 || crows > 16384 || src_misalign < 0 || src_misalign > 7) {
    err = "an even window inside planes of at most 16384 x 16384 samples, its half inside the chroma planes, src_misalign in 0..7"; return RBT_ERR_PARAM; }
  const size_t luma = (size_t)stride * rows, chroma = (size_t)cstride * crows, pic = luma + 2 * chroma, in_n = pic * (size_t)n_pics, ys = (size_t)w * h, cs = ys / 4, fs = ys + 2 * cs,
               out_n = fs * (size_t)n_pics, in_bytes = ((in_n + 8) * 2 + 255) & ~(size_t)255;
  DevBuf buf, desc;
  if (!buf.alloc(256 + in_bytes + out_n * 2) || !desc.alloc(sizeof(RbtGatherPic) * 3 * (size_t)n_pics)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  uint8_t* base = (uint8_t*)(((uintptr_t)buf.p + 255) & ~(uintptr_t)255);
  uint16_t* d_in = (uint16_t*)base + src_misalign; uint16_t* d_out = (uint16_t*)(base + in_bytes);
  std::vector<RbtGatherPic> pics;
  for (int k = 0; k < n_pics; k++) {
    const uint16_t* p = d_in + pic * (size_t)k; uint16_t* o = d_out + fs * (size_t)k;
    pics.push_back(RbtGatherPic{p + (size_t)y0 * stride + x0, o, w, h, stride, 0});
    for (int c = 0; c < 2; c++) pics.push_back(RbtGatherPic{p + luma + chroma * (size_t)c + (size_t)(y0 / 2) * cstride + x0 / 2, o + ys + cs * (size_t)c, w / 2, h / 2, cstride, 0});
  }
  if (rbtk::h2d(d_in, src, in_n * 2) | rbtk::h2d(desc.p, pics.data(), sizeof(RbtGatherPic) * pics.size()) | rbtk::dev_memset(d_out, 0xEE, out_n * 2)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  rbtk::launch_gather_luma(desc.as<RbtGatherPic>(), (int)pics.size(), RBT_GM_PIC_CHUNKS(w, h));
  if (rbtk::d2h(out, d_out, out_n * 2) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  return RBT_OK;
}

// New colours for an indexed cloud. The triples go to a buffer of their own first: the cloud keeps its colours and its index until the upload has succeeded.
int pcloud_set_colors(std::string& err, PCloud* c, const uint8_t* rgb) {
  DevBuf fresh;
  if (!fresh.alloc(3 * (size_t)c->n)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  if (rbtk::h2d(fresh.p, rgb, 3 * (size_t)c->n)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  if (rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }      // nothing in flight reads the triples that go
  c->rgb.take(fresh);
  const RbtScoreCloud S = c->view();
  rbtk::launch_sc_recolor(&S);
  if (rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  return RBT_OK;
}

// A label per point for a cloud that is indexed already; as with the colours, the cloud keeps what it had until the upload has succeeded.
int pcloud_set_labels(std::string& err, PCloud* c, const uint32_t* labels) {
  for (int i = 0; i < c->n; i++) if (labels[i] >= 65536u) { err = "label " + std::to_string(i) + " is not below 65536"; return RBT_ERR_PARAM; }
  DevBuf fresh;
  if (!fresh.alloc(4 * (size_t)c->n)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  if (rbtk::h2d(fresh.p, labels, 4 * (size_t)c->n) || rbtk::dev_sync()) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  c->labels.take(fresh); c->label_bound = 0;
  return RBT_OK;
}
int pcloud_labels(std::string& err, const PCloud* c, uint32_t* labels) {
  if (!c->labels.p) { err = "the cloud carries no labels"; return RBT_ERR_PARAM; }
  if (rbtk::d2h(labels, c->labels.p, 4 * (size_t)c->n) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  return RBT_OK;
}
bool pcloud_has_labels(const PCloud* c) { return c->labels.p != nullptr; }
// rbt_score_patches: the D1 part of pcloud_score - the same launches, so `whole` is its d1 bit for bit - and the per-patch sums on the distances it leaves
int pcloud_score_patches(std::string& err, const PCloud* a, const PCloud* b, int peak, int n_patches, rbt_patch_d1* out, rbt_d1_result* whole, double* device_ms) {
  if (whole) memset(whole, 0, sizeof(*whole));
  if (device_ms) *device_ms = 0;
  if (peak <= 0) { err = "bad peak"; return RBT_ERR_PARAM; }
  if (n_patches < 1 || n_patches > 65536) { err = "n_patches is 1..65536"; return RBT_ERR_PARAM; }
  if (!b->labels.p) { err = "the decoded cloud carries no labels"; return RBT_ERR_PARAM; }
  memset(out, 0, sizeof(*out) * (size_t)n_patches);
  const size_t na = (size_t)a->n, nb = (size_t)b->n, words = (size_t)RBT_PD_WORDS * (size_t)n_patches;
  DevBuf dist, res, sums, bad;
  if (!dist.alloc(4 * (na + nb)) || !res.alloc(8 * RBT_SC_RESULTS) || !sums.alloc(8 * words) || !bad.alloc(4)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  if (rbtk::dev_memset(res.p, 0, 8 * RBT_SC_RESULTS) | rbtk::dev_memset(sums.p, 0, 8 * words) | rbtk::dev_memset(bad.p, 0, 4)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  // the labels of a cloud made from maps are its items' patch indices, below its patch count: no kernel and no read-back is needed to know them good (the trial clouds
  // of rbt_submit_gof_d1_patches, one per frame and trial). Labels a caller gave are checked on the device.
  uint32_t is_bad = 0;
  if (b->label_bound <= 0 || b->label_bound > n_patches) {
    rbtk::launch_pd_check(b->labels.as<uint32_t>(), b->n, (uint32_t)n_patches, bad.as<uint32_t>());
    if (rbtk::d2h(&is_bad, bad.p, 4) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  }
  if (is_bad) { err = "a label of the decoded cloud is not below n_patches"; return RBT_ERR_PARAM; }      // no sum has been written
  RbtScoreWork W; memset(&W, 0, sizeof(W));
  W.dist_a = dist.as<uint32_t>(); W.dist_b = W.dist_a + na; W.res = res.as<unsigned long long>();
  const RbtScoreCloud A = a->view(), B = b->view();
  rbtk::timer_begin(T_COL_DIST);             // as pcloud_score: every call reads its timers before it returns
  rbtk::launch_sc_score(&A, &B, RBT_SCORE_D1, &W);
  rbtk::launch_pd_sums(&A, &B, b->labels.as<uint32_t>(), W.dist_a, W.dist_b, sums.as<unsigned long long>());
  rbtk::timer_end(T_COL_DIST);
  uint64_t h[RBT_SC_RESULTS]; std::vector<uint64_t> hw(words);
  if (rbtk::d2h(h, res.p, sizeof(h)) || rbtk::d2h(hw.data(), sums.p, 8 * words) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  if (device_ms) *device_ms = rbtk::timer_ms(T_COL_DIST);
  for (int k = 0; k < n_patches; k++) {
    const uint64_t* w = &hw[(size_t)RBT_PD_WORDS * (size_t)k]; rbt_patch_d1* o = &out[k];
    o->n_ab = (uint32_t)w[RBT_PD_N_AB]; o->n_ba = (uint32_t)w[RBT_PD_N_BA]; o->sse_ab = w[RBT_PD_SSE_AB]; o->sse_ba = w[RBT_PD_SSE_BA]; o->max_ab = w[RBT_PD_MAX_AB]; o->max_ba = w[RBT_PD_MAX_BA];
    patch_d1_finish(o, peak);
  }
  if (whole) {
    const uint32_t* mx = (const uint32_t*)&h[RBT_SC_D1_MAX];
    whole->n_a = a->n_merged; whole->n_b = b->n_merged; whole->sse_ab = h[RBT_SC_D1_AB]; whole->sse_ba = h[RBT_SC_D1_BA]; whole->max_ab = mx[0]; whole->max_ba = mx[1];
    finish_geometry(whole, peak);
  }
  return RBT_OK;
}

bool pcloud_has_normals(const PCloud* c) { return c->nrm.p != nullptr; }
// rbt_score_patches_d2: pcloud_score with RBT_SCORE_D2 - the same launches, so `whole` is its d2 bit for bit - and the per-patch sums on the distances and values it leaves
int pcloud_score_patches_d2(std::string& err, const PCloud* a, const PCloud* b, int peak, int n_patches, rbt_patch_d2* out, rbt_d2_result* whole, double* device_ms) {
  if (whole) memset(whole, 0, sizeof(*whole));
  if (device_ms) *device_ms = 0;
  if (peak <= 0) { err = "bad peak"; return RBT_ERR_PARAM; }
  if (n_patches < 1 || n_patches > 65536) { err = "n_patches is 1..65536"; return RBT_ERR_PARAM; }
  if (!b->labels.p) { err = "the decoded cloud carries no labels"; return RBT_ERR_PARAM; }
  if (!a->nrm.p) { err = "D2 needs normals on the source"; return RBT_ERR_PARAM; }
  memset(out, 0, sizeof(*out) * (size_t)n_patches);
  const size_t na = (size_t)a->n, nb = (size_t)b->n, blocks = (std::max(na, nb) + RBT_SC_SUM - 1) / RBT_SC_SUM, words = (size_t)RBT_P2_WORDS * (size_t)n_patches;
  const size_t ents = blocks * RBT_SC_SUM, cols = (size_t)n_patches * RBT_SC_SUM;
  DevBuf dist, nrm_b, val, part, res, sums, bad, ent, S;
  if (!dist.alloc(4 * (na + nb)) || !res.alloc(8 * RBT_SC_RESULTS) || !nrm_b.alloc(28 * nb) || !val.alloc(8 * (na + nb)) || !part.alloc(16 * blocks) || !sums.alloc(8 * words) || !bad.alloc(4) ||
      !ent.alloc(12 * ents + 4 * blocks) || !S.alloc(8 * cols)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  if (rbtk::dev_memset(res.p, 0, 8 * RBT_SC_RESULTS) | rbtk::dev_memset(nrm_b.p, 0, 28 * nb) | rbtk::dev_memset(sums.p, 0, 8 * words) | rbtk::dev_memset(bad.p, 0, 4) | rbtk::dev_memset(S.p, 0, 8 * cols)) {
    err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  uint32_t is_bad = 0;                       // as pcloud_score_patches: labels a caller gave are checked on the device before any sum is written
  if (b->label_bound <= 0 || b->label_bound > n_patches) {
    rbtk::launch_pd_check(b->labels.as<uint32_t>(), b->n, (uint32_t)n_patches, bad.as<uint32_t>());
    if (rbtk::d2h(&is_bad, bad.p, 4) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  }
  if (is_bad) { err = "a label of the decoded cloud is not below n_patches"; return RBT_ERR_PARAM; }
  RbtScoreWork W; memset(&W, 0, sizeof(W));
  W.dist_a = dist.as<uint32_t>(); W.dist_b = W.dist_a + na; W.res = res.as<unsigned long long>();
  W.acc_b = nrm_b.as<long long>(); W.cnt_b = (int32_t*)(W.acc_b + 3 * nb); W.val_ab = val.as<double>(); W.val_ba = W.val_ab + na; W.part = part.as<double>();
  RbtPatchD2Work P; P.ent_sum = ent.as<double>(); P.ent_label = (uint32_t*)(P.ent_sum + ents); P.ent_n = P.ent_label + ents; P.S = S.as<double>();
  const RbtScoreCloud A = a->view(), B = b->view();
  rbtk::timer_begin(T_COL_DIST);             // as pcloud_score: every call reads its timers before it returns
  rbtk::launch_sc_score(&A, &B, RBT_SCORE_D2, &W);
  rbtk::launch_p2_sums(&A, &B, b->labels.as<uint32_t>(), &W, &P, n_patches, sums.as<unsigned long long>());
  rbtk::timer_end(T_COL_DIST);
  uint64_t h[RBT_SC_RESULTS]; std::vector<uint64_t> hw(words);
  if (rbtk::d2h(h, res.p, sizeof(h)) || rbtk::d2h(hw.data(), sums.p, 8 * words) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  if (device_ms) *device_ms = rbtk::timer_ms(T_COL_DIST);
  for (int k = 0; k < n_patches; k++) {
    const uint64_t* w = &hw[(size_t)RBT_P2_WORDS * (size_t)k]; rbt_patch_d2* o = &out[k];
    double v[4]; memcpy(&v[0], &w[RBT_P2_SSE_AB], 16); memcpy(&v[2], &w[RBT_P2_MAX_AB], 16);
    o->n_ab = (uint32_t)w[RBT_P2_N_AB]; o->n_ba = (uint32_t)w[RBT_P2_N_BA]; o->sse_ab = v[0]; o->sse_ba = v[1]; o->max_ab = v[2]; o->max_ba = v[3];
    patch_d2_finish(o, peak);
  }
  if (whole) {
    double v[4]; memcpy(v, &h[RBT_SC_D2_AB], sizeof(v));
    whole->n_a = a->n_merged; whole->n_b = b->n_merged; whole->sse_ab = v[0]; whole->max_ab = v[1]; whole->sse_ba = v[2]; whole->max_ba = v[3];
    finish_geometry(whole, peak);
  }
  return RBT_OK;
}

// The colour sums per patch on stored distances (csrc/rbt_score.h, "col/patch"): the refusals the two calls share, the label check, k_pc_sums per direction, and the
// figures - the whole frame's from the sums over the patches, which are exact. timed: events around search (when dist is still to be made) and sums
static int patch_color_sums(std::string& err, const PCloud* a, const PCloud* b, uint32_t* dist_a, uint32_t* dist_b, bool search, int n_patches, rbt_patch_color* out, rbt_color_result* whole, double* device_ms) {
  if (whole) memset(whole, 0, sizeof(*whole));
  if (device_ms) *device_ms = 0;
  if (n_patches < 1 || n_patches > 65536) { err = "n_patches is 1..65536"; return RBT_ERR_PARAM; }
  if (!a->rgb.p || !b->rgb.p || a->n_merged > (1 << 21) || b->n_merged > (1 << 21)) { err = "the colour part needs colours on both clouds and at most 2^21 merged points in each"; return RBT_ERR_PARAM; }
  if (!b->labels.p) { err = "the decoded cloud carries no labels"; return RBT_ERR_PARAM; }
  memset(out, 0, sizeof(*out) * (size_t)n_patches);
  const size_t words = (size_t)RBT_PC_WORDS * (size_t)n_patches;
  DevBuf sums, bad;
  if (!sums.alloc(8 * words) || !bad.alloc(4)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  if (rbtk::dev_memset(sums.p, 0, 8 * words) | rbtk::dev_memset(bad.p, 0, 4)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  uint32_t is_bad = 0;                       // as pcloud_score_patches: labels a caller gave are checked on the device before any sum is written
  if (b->label_bound <= 0 || b->label_bound > n_patches) {
    rbtk::launch_pd_check(b->labels.as<uint32_t>(), b->n, (uint32_t)n_patches, bad.as<uint32_t>());
    if (rbtk::d2h(&is_bad, bad.p, 4) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  }
  if (is_bad) { err = "a label of the decoded cloud is not below n_patches"; return RBT_ERR_PARAM; }
  const RbtScoreCloud A = a->view(), B = b->view();
  if (device_ms) rbtk::timer_begin(T_COL_DIST);             // as pcloud_score: every call reads its timers before it returns
  if (search) rbtk::launch_sc_search(&A, &B, dist_a, dist_b);
  rbtk::launch_pc_sums(&A, &B, b->labels.as<uint32_t>(), dist_a, dist_b, sums.as<unsigned long long>());
  if (device_ms) rbtk::timer_end(T_COL_DIST);
  std::vector<uint64_t> hw(words);
  if (rbtk::d2h(hw.data(), sums.p, 8 * words) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  if (device_ms) *device_ms = rbtk::timer_ms(T_COL_DIST);
  rbt_color_result all; memset(&all, 0, sizeof(all));
  for (int k = 0; k < n_patches; k++) {
    const uint64_t* w = &hw[(size_t)RBT_PC_WORDS * (size_t)k]; rbt_patch_color* o = &out[k];
    o->n_ab = (uint32_t)w[RBT_PC_N_AB]; o->n_ba = (uint32_t)w[RBT_PC_N_BA];
    for (int c = 0; c < 3; c++) { o->sse_ab[c] = w[RBT_PC_SSE_AB + c]; o->sse_ba[c] = w[RBT_PC_SSE_BA + c]; all.sse_ab[c] += o->sse_ab[c]; all.sse_ba[c] += o->sse_ba[c]; }
    patch_color_finish(o);
  }
  if (whole) { all.n_a = a->n_merged; all.n_b = b->n_merged; finish_color(&all); *whole = all; }
  return RBT_OK;
}
// rbt_score_patches_color: the two searches of pcloud_score, then the sums per patch in place of the colour walks
int pcloud_score_patches_color(std::string& err, const PCloud* a, const PCloud* b, int n_patches, rbt_patch_color* out, rbt_color_result* whole, double* device_ms) {
  DevBuf dist;
  if (!dist.alloc(4 * ((size_t)a->n + (size_t)b->n))) { if (whole) memset(whole, 0, sizeof(*whole)); if (device_ms) *device_ms = 0; err = "device allocation failed"; return RBT_ERR_NOMEM; }
  double ms = 0;
  const int rc = patch_color_sums(err, a, b, dist.as<uint32_t>(), dist.as<uint32_t>() + a->n, true, n_patches, out, whole, &ms);
  if (device_ms) *device_ms = ms;
  return rc;
}

struct ScorePair { const PCloud* a; const PCloud* b; int na, nb; DevBuf dist; };
bool score_pair_uses(const ScorePair* p, const PCloud* c) { return p->a == c || p->b == c; }
void score_pair_release(ScorePair* p) { delete p; }
int score_pair_create(std::string& err, const PCloud* a, const PCloud* b, ScorePair** out) {
  *out = nullptr;
  std::unique_ptr<ScorePair> P(new ScorePair{a, b, a->n, b->n, {}});
  if (!P->dist.alloc(4 * ((size_t)a->n + (size_t)b->n))) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  const RbtScoreCloud A = a->view(), B = b->view();
  rbtk::launch_sc_search(&A, &B, P->dist.as<uint32_t>(), P->dist.as<uint32_t>() + a->n);
  if (rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  *out = P.release();
  return RBT_OK;
}
int score_pair_color(std::string& err, const ScorePair* p, rbt_color_result* out) {
  memset(out, 0, sizeof(*out));
  const PCloud *a = p->a, *b = p->b;
  if (!a->rgb.p || !b->rgb.p || a->n_merged > (1 << 21) || b->n_merged > (1 << 21)) { err = "the colour part needs colours on both clouds and at most 2^21 merged points in each"; return RBT_ERR_PARAM; }
  DevBuf res;
  if (!res.alloc(8 * RBT_SC_COLOR_RESULTS)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  if (rbtk::dev_memset(res.p, 0, 8 * RBT_SC_COLOR_RESULTS)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  const RbtScoreCloud A = a->view(), B = b->view();
  rbtk::launch_sc_color_walks(&A, &B, p->dist.as<uint32_t>(), p->dist.as<uint32_t>() + p->na, res.as<unsigned long long>());
  uint64_t h[RBT_SC_COLOR_RESULTS];
  if (rbtk::d2h(h, res.p, sizeof(h)) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  out->n_a = a->n_merged; out->n_b = b->n_merged;
  for (int c = 0; c < 3; c++) { out->sse_ab[c] = h[c]; out->sse_ba[c] = h[3 + c]; }
  finish_color(out);
  return RBT_OK;
}
// rbt_score_pair_patches_color: the sums per patch on the pair's distances, with the colours and labels of the moment
int score_pair_patches_color(std::string& err, const ScorePair* p, int n_patches, rbt_patch_color* out, rbt_color_result* whole) {
  return patch_color_sums(err, p->a, p->b, p->dist.as<uint32_t>(), p->dist.as<uint32_t>() + p->na, false, n_patches, out, whole, nullptr);
}

// The cloud keeps the normals it had until the new ones are complete: they are written to a buffer of their own, which replaces the old one after the kernels have run.
int pcloud_estimate_normals(std::string& err, PCloud* c, int k, int orient, const int32_t view_point[3], int16_t* out, double* device_ms) {
  const size_t n = (size_t)c->n, slots = (size_t)1 << c->lg;
  DevBuf nrm, slot;
  if (!nrm.alloc(6 * n) || !slot.alloc(8 * slots)) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  RbtNormals N; memset(&N, 0, sizeof(N));
  N.k = k < c->n_merged ? k : c->n_merged; N.orient = orient; for (int i = 0; i < 3; i++) N.vp[i] = view_point[i];
  N.out = nrm.as<int16_t>(); N.slot = slot.as<int16_t>();
  const RbtScoreCloud S = c->view();
  rbtk::timer_begin(T_COL_DIST);             // as pcloud_score: every call reads its timers before it returns
  rbtk::launch_nm_estimate(&S, &N);
  rbtk::timer_end(T_COL_DIST);
  if ((out ? rbtk::d2h(out, nrm.p, 6 * n) : 0) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  if (device_ms) *device_ms = rbtk::timer_ms(T_COL_DIST);
  c->nrm.take(nrm);
  return RBT_OK;
}
int pcloud_score(std::string& err, const PCloud* a, const PCloud* b, int peak, int parts, rbt_frame_score* out) {
  memset(out, 0, sizeof(*out));
  // |colour error term| <= 2.55e6: the sum of 2^21 squares still fits 64 bits - rbt_color_metric refuses larger clouds, and so does the colour part here
  const bool colours = a->rgb.p && b->rgb.p && a->n_merged <= (1 << 21) && b->n_merged <= (1 << 21);
  const int can = RBT_SCORE_D1 | (a->nrm.p ? RBT_SCORE_D2 : 0) | (colours ? RBT_SCORE_COLOR : 0);
  if (parts == 0) parts = can;
  if (peak <= 0 || (parts & ~can)) {
    err = parts & ~can & RBT_SCORE_D2 ? "D2 needs normals on the source" : parts & ~can & RBT_SCORE_COLOR ? "the colour part needs colours on both clouds and at most 2^21 merged points in each" : "bad peak or parts";
    return RBT_ERR_PARAM;
  }
  const size_t na = (size_t)a->n, nb = (size_t)b->n, blocks = (std::max(na, nb) + RBT_SC_SUM - 1) / RBT_SC_SUM;
  const bool d2 = (parts & RBT_SCORE_D2) != 0;
  DevBuf dist, nrm_b, val, part, res;
  if (!dist.alloc(4 * (na + nb)) || !res.alloc(8 * RBT_SC_RESULTS) || (d2 && (!nrm_b.alloc(28 * nb) || !val.alloc(8 * (na + nb)) || !part.alloc(16 * blocks)))) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  if (rbtk::dev_memset(res.p, 0, 8 * RBT_SC_RESULTS) | (d2 ? rbtk::dev_memset(nrm_b.p, 0, 28 * nb) : 0)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  RbtScoreWork W; memset(&W, 0, sizeof(W));
  W.dist_a = dist.as<uint32_t>(); W.dist_b = W.dist_a + na; W.res = res.as<unsigned long long>();
  if (d2) { W.acc_b = nrm_b.as<long long>(); W.cnt_b = (int32_t*)(W.acc_b + 3 * nb); W.val_ab = val.as<double>(); W.val_ba = W.val_ab + na; W.part = part.as<double>(); }
  const RbtScoreCloud A = a->view(), B = b->view();
  rbtk::timer_begin(T_COL_DIST);             // one timer for every score: each call reads its timers before it returns
  rbtk::launch_sc_score(&A, &B, parts, &W);
  rbtk::timer_end(T_COL_DIST);
  uint64_t h[RBT_SC_RESULTS];
  if (rbtk::d2h(h, res.p, sizeof(h)) || rbtk::dev_sync()) { err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  out->parts = parts | RBT_SCORE_D1; out->device_ms = rbtk::timer_ms(T_COL_DIST);
  out->n_points_a = a->n; out->n_points_b = b->n; out->n_merged_a = a->n_merged; out->n_merged_b = b->n_merged;
  const uint32_t* mx = (const uint32_t*)&h[RBT_SC_D1_MAX];
  out->d1.n_a = a->n_merged; out->d1.n_b = b->n_merged; out->d1.sse_ab = h[RBT_SC_D1_AB]; out->d1.sse_ba = h[RBT_SC_D1_BA]; out->d1.max_ab = mx[0]; out->d1.max_ba = mx[1];
  finish_geometry(&out->d1, peak);
  if (d2) {
    double v[4]; memcpy(v, &h[RBT_SC_D2_AB], sizeof(v));
    out->d2.n_a = a->n_merged; out->d2.n_b = b->n_merged; out->d2.sse_ab = v[0]; out->d2.max_ab = v[1]; out->d2.sse_ba = v[2]; out->d2.max_ba = v[3];
    finish_geometry(&out->d2, peak);
  }
  if (parts & RBT_SCORE_COLOR) {
    out->color.n_a = a->n_merged; out->color.n_b = b->n_merged;
    for (int c = 0; c < 3; c++) { out->color.sse_ab[c] = h[RBT_SC_COL_AB + c]; out->color.sse_ba[c] = h[RBT_SC_COL_BA + c]; }
    finish_color(&out->color);
  }
  return RBT_OK;
}

// ---- the host-array metrics (rbt_d1, rbt_d2, rbt_color_metric): upload + score + release of two temporary clouds ----
// The callers have refused empty input, a bad peak and missing colours or normals in their own words; what can still be refused here is a coordinate outside the volume
// or more than 2^26 points (pcloud_index; A before B) and, for the colour part, more than 2^21 merged points. The cache is the call's own and is trimmed when the call
// ends: the volumes go back to the device pool, and the context's cloud cache never sees them.
static int score_host_clouds(std::string& err, const int16_t* a, const uint8_t* rgb_a, const int16_t* normals_a, int na, const int16_t* b, const uint8_t* rgb_b, int nb, int peak, int parts, rbt_frame_score* out) {
  struct Guard { PCloudCache cache; PCloud* a = nullptr; PCloud* b = nullptr; ~Guard() { pcloud_release(cache, a); pcloud_release(cache, b); pcloud_cache_trim(cache); } } g;
  if (int rc = pcloud_upload(err, g.cache, a, rgb_a, normals_a, na, &g.a)) return rc;
  if (int rc = pcloud_upload(err, g.cache, b, rgb_b, nullptr, nb, &g.b)) return rc;
  // |colour error term| <= 2.55e6: the sum of 2^21 squares still fits 64 bits
  if ((parts & RBT_SCORE_COLOR) && (pcloud_merged(g.a) > (1 << 21) || pcloud_merged(g.b) > (1 << 21))) { err = "more than 2^21 merged points"; return RBT_ERR_PARAM; }
  return pcloud_score(err, g.a, g.b, peak, parts, out);
}
// QualityMetrics::compute with the point-to-point error (PCCMetrics.cpp:75-231) both ways (:299-309)
int pcc_d1(std::string& err, const int16_t* a, int na, const int16_t* b, int nb, int peak, rbt_d1_result* out) {
  memset(out, 0, sizeof(*out));
  if (na <= 0 || nb <= 0 || peak <= 0) { err = "empty point cloud"; return RBT_ERR_PARAM; }
  rbt_frame_score s;
  const int rc = score_host_clouds(err, a, nullptr, nullptr, na, b, nullptr, nb, peak, RBT_SCORE_D1, &s);
  if (!rc) *out = s.d1;
  return rc;
}
// QualityMetrics::compute with computeC2p_ (PCCMetrics.cpp:100-124, :213-215) both ways (:299-309), normals as PCCMetrics::compute arranges them (:371-376)
int pcc_d2(std::string& err, const int16_t* a, const int16_t* normals_a, int na, const int16_t* b, int nb, int peak, rbt_d2_result* out) {
  memset(out, 0, sizeof(*out));
  if (na <= 0 || nb <= 0 || peak <= 0 || !normals_a) { err = "empty point cloud or no normals"; return RBT_ERR_PARAM; }
  rbt_frame_score s;
  const int rc = score_host_clouds(err, a, nullptr, normals_a, na, b, nullptr, nb, peak, RBT_SCORE_D2, &s);
  if (!rc) *out = s.d2;
  return rc;
}
// QualityMetrics::compute with computeColor_ (PCCMetrics.cpp:127-179, :221-225) both ways (:321-325) on merged clouds. ms: device time of the score (search, walks, sums)
int pcc_color_metric(std::string& err, const int16_t* a, const uint8_t* rgb_a, int na, const int16_t* b, const uint8_t* rgb_b, int nb, rbt_color_result* out, double* ms) {
  memset(out, 0, sizeof(*out));
  if (ms) *ms = 0;                           // a refused call has run no stage
  if (na <= 0 || nb <= 0 || !rgb_a || !rgb_b) { err = "empty point cloud or no colours"; return RBT_ERR_PARAM; }
  rbt_frame_score s;
  const int rc = score_host_clouds(err, a, rgb_a, nullptr, na, b, rgb_b, nb, RBT_PCC_DIM - 1, RBT_SCORE_COLOR, &s);      // the peak enters the geometry figures only
  if (!rc) { *out = s.color; if (ms) *ms = s.device_ms; }
  return rc;
}
}  // namespace rbt
