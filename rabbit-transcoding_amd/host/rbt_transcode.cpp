// Encode half of the hot path and the transcode pipeline.
// Replaces initEncoder / setEncoderOptions / encodeVideo / resize_frame2 of PCCTranscoder (PCCTranscoder.cpp:683-753,
// :825-904, :548-592, :594-646) and the decode -> pool -> encode loop of transcodeVideo (:428-510).
#include <algorithm>
#include <map>
#include <memory>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include "rbt_batch.h"
#include "rbt_transcode.h"
#include "rbt_rate_walk.h"
#include "rbt_floor_walk.h"
#include "rbt_quality_walk.h"
#include "rbt_d1_walk.h"
#include "rbt_color_walk.h"
#include "rbt_frame_walk.h"
#include "rbt_patch_walk.h"
#include "rbt_qp_map.h"
#include "rbt_pcc.h"
#include "../csrc/rbt_cloudmaps.h"
#ifdef RBT_HOSTEMU
#include "../csrc/rbt_qpmap.h"      // the serial stand-in of launch_enc_qp_fix (the product's launcher is declared in rbt_kernels.h)
#endif

namespace rbt {

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct EncStreamDesc {
  int w, h, bd, n_frames, qp, i_qp_offset, gop, lossless, log2_ctb, rows, md5;   // w, h: display size (any even numbers); md5: RBT_HASH_* of the hash SEI behind every picture
  std::vector<const uint8_t*> hint_pm, hint_dm; int hint_w4 = 0, hint_h4 = 0;       // per frame: the decoded input picture's 4x4 maps (device), empty = no hints
  std::vector<const uint8_t*> occ4; int occ4_w = 0, occ4_h = 0;                      // per frame: occupancy of the 4x4 luma units (device, RbtFrame::occ4), empty = every sample counts
  int sao = 0;                           // SAO on (every stream that is not lossless, unless RBT_ENC_SAO=0)
  int tools_off = 0;                     // RBT_ET_* decision tools left out (rbt_stream_params.preset)
  std::vector<const uint16_t*> src[3];   // device planes per frame
  std::vector<const uint32_t*> src_flat; // per frame: the chroma_flat word (device) of the decoded picture the planes belong to, empty = none (RbtFrame::src_flat)
  bool src_flat_always = false;          // the planes' chroma is the constant 1 << (bd - 1) by construction (pooled occupancy maps)
  // Arena sharing (round 4): per frame, buffers of the DECODED input picture that are dead by the time this picture is encoded and have the encoder's geometry - its
  // coefficient levels (read by the reconstruction of that picture only) and its pre-SAO samples (read by that picture's own loop filters only): the encoder keeps its own
  // levels and reconstruction there instead of in memory of its own (9.8 MB per 1280x1280 picture, 1.26 GB per GOF). Empty / null = the encoder allocates.
  std::vector<uint16_t*> alias_pix; std::vector<int16_t*> alias_coef;
  int src_stride = 0, src_x0 = 0, src_y0 = 0;   // the planes are views: luma row stride (0 = w) and origin of the w x h region (luma samples)
  std::vector<int> pic; int n_total = 0; // a pass over a subset of the frames (desc_subset): the stream's picture behind each coded picture, and how many the stream has; empty = all of them
  std::vector<int8_t> frame_qp;          // a QP per point-cloud frame (rbt_frame_qp): pictures f * gop .. f * gop + gop - 1 are coded from frame_qp[f] where qp would be used; empty = qp. The parameter sets stay those of qp
  // a QP per CTB (rbt_qp_map): M[f][r][c], qm_h rows of qm_w CTBs per point-cloud frame, as the caller gave them; picture f * gop + k takes its targets from frame f as
  // frame_qp's pictures take theirs (encode_plan). Empty = none. The PPS of such a stream says cu_qp_delta_enabled_flag = 1, everything else is that of qp
  std::vector<int8_t> qp_map; int qm_w = 0, qm_h = 0;
};
// Pictures are coded at the display size rounded up to 8 (all-intra) or 16 (I,P pairs: 16x16 inter CUs) and the padding is
// signalled as the conformance window (7.4.3.2.1), like libx265 does for the reference (PCCTranscoder.cpp:706).
struct PadJob { const uint16_t* in; int stride, x0, y0, w, h; uint16_t* out; int dw, dh; };
struct EncodeBatch {
  std::vector<EncStreamDesc> desc;
  std::vector<Sps> sps; std::vector<Pps> pps;
  std::vector<RbtFrame> frames; std::vector<RbtSlice> slices; std::vector<int> frame_stream, frame_is_idr;
  std::vector<int> stream_first;
  void* arena = nullptr; size_t arena_size = 0;
  RbtFrame* d_frames = nullptr; RbtSlice* d_slices = nullptr; int32_t* d_lists = nullptr; uint8_t* d_out = nullptr; uint8_t* d_packed = nullptr; uint32_t* d_dst = nullptr;
  size_t out_total = 0;
  std::vector<PadJob> pad_jobs;                 // source pictures that have to be copied into padded planes before the encoder reads them
  std::vector<std::vector<size_t>> pic_at;     // after encode_finish, per stream: where in its output the NAL units of each picture start (rbt_frame_walk.h frame_cut)
  std::vector<uint16_t> cs_keep; uint16_t* d_cs = nullptr;   // the ctb->slice maps of all pictures back to back: host staging (alive until the copy has completed) and device
  std::vector<int8_t> qm_keep; int8_t* d_qm = nullptr;       // QP per CTB: the target maps (RbtFrame::qp_map) of the pictures that carry one, back to back, staged and uploaded like the maps above
  std::vector<int> frame_qm;                                  // ... per picture where its map starts in qm_keep, -1 = the picture has none
  size_t off_iqm = 0, off_pqm = 0; int n_iqm = 0, n_pqm = 0;  // ... index lists of the I / P pictures with a map (launch_enc_qp_fix)
  uint8_t* d_zero = nullptr; size_t zero_bytes = 0; bool wpp = false;   // launch tickets (3 words) + row progress of the wavefront mode
  int main_stream = 0, aux_stream = -1;          // aux_stream >= 0: the intra part was enqueued there (its timers live there)
  HashSet hash; std::vector<int> hash_idx;      // md5_sei: the reconstructions to hash (after SAO), index of each picture in `hash` (-1: none)
  size_t n_sums = 0; uint64_t* d_sums = nullptr; std::vector<uint64_t> sums;   // quality floors: RBT_SSE_WORDS distortion words per picture behind the slice table (set n_sums before encode_build); after encode_finish: their values
  size_t n_ctb_words = 0; uint64_t* d_ctb_words = nullptr;   // floors per patch: the words per CTB of k_ctb_sse (set before encode_build); they stay here, their folds are the tail of d_sums
  std::vector<int32_t> lists_keep; size_t off_i = 0, off_ideb = 0, off_p = 0, off_sl = 0, off_sl_p = 0, off_isao = 0, off_psao = 0, off_pdeb = 0; int n_pdeb = 0, n_i = 0, n_ideb = 0, n_p = 0, n_sl_i = 0, n_sl_p = 0, n_isao = 0, n_psao = 0;   // index lists (encode_upload_lists)
  std::string err;
  ~EncodeBatch() { rbtk::dev_free(arena); }
};

// RBT-E1 codes SAO unless RBT_ENC_SAO=0 (development switch, read by the oracle the same way)
// ... and transform skip for the 4x4 luma blocks unless RBT_ENC_TS=0
static int e1_ts_on() { static int v = -1; if (v < 0) { const char* e = getenv("RBT_ENC_TS"); v = !e || atoi(e) != 0; } return v; }
static int e1_sao_on() { static int v = -1; if (v < 0) { const char* e = getenv("RBT_ENC_SAO"); v = !e || atoi(e) != 0; } return v; }
// ... and the decision tools of round 3 (RBT_ET_*): SATD block costs, closed-loop mode choice, level-dependent rounding, coded mode trial unless RBT_ENC_SATD / _REFINE / _RQ / _RDM = 0
static int e1_tools(int lossless) {
  static int v = -1;
  if (v < 0) { auto on = [](const char* n) { const char* e = getenv(n); return !e || atoi(e) != 0; }; v = (on("RBT_ENC_SATD") ? RBT_ET_SATD : 0) | (on("RBT_ENC_REFINE") ? RBT_ET_REFINE : 0) | (on("RBT_ENC_RQ") ? RBT_ET_RQ : 0) | (on("RBT_ENC_RDM") ? RBT_ET_RDM : 0); }
  return lossless ? v & ~(RBT_ET_RQ | RBT_ET_RDM) : v;
}
// Every picture takes the in-place deblocking launches before the SAO kernel; RBT_FUSED_ENC_LF=1 deblocks inside the SAO kernel instead (en_sao_ctb: the CTB and its halo
// in LDS; same samples, ~2 GB less HBM traffic per GOF). Off by default: the driver's 20-GOF run is 3 % slower with it, 5 % with the decoder's fused form as well
// (tools/lf_probe.sh: 763 / 741 / 725 point-cloud frames/s) - the path is not HBM-bound, and the LDS-free filter launches fill gaps the LDS-holding kernels leave.
static int e1_fused_lf() { static int v = -1; if (v < 0) { const char* e = getenv("RBT_FUSED_ENC_LF"); v = e && atoi(e) != 0; } return v; }
static int coded_size(int v, int gop) { int al = gop > 1 ? 16 : 8; return (v + al - 1) / al * al; }
static void make_param_sets(const EncStreamDesc& d, Sps& s, Pps& p) {
  s = Sps(); p = Pps();
  const int cw = coded_size(d.w, d.gop), ch = coded_size(d.h, d.gop);
  s.valid = true; s.width = cw; s.height = ch; s.conf_win[1] = (cw - d.w) / 2; s.conf_win[3] = (ch - d.h) / 2; s.bit_depth = d.bd; s.log2_max_poc_lsb = 8; s.max_dec_pic_buffering = 3;
  s.log2_ctb = d.log2_ctb ? d.log2_ctb : 5; s.log2_min_cb = 3; s.log2_diff_max_min_cb = s.log2_ctb - 3;
  s.log2_min_tb = 2; s.log2_max_tb = std::min(5, s.log2_ctb); s.log2_diff_max_min_tb = s.log2_max_tb - 2;
  s.num_st_rps = 1; s.sao = d.sao; s.max_th_depth_intra = 1;   // an intra CU is one transform unit or four (oracle/hevc_enc.c setup_stream)
  s.w_ctb = (cw + (1 << s.log2_ctb) - 1) >> s.log2_ctb; s.h_ctb = (ch + (1 << s.log2_ctb) - 1) >> s.log2_ctb;
  p.valid = true; p.num_ref_idx_default = 1; p.init_qp = std::min(51, std::max(0, d.qp)); p.loop_filter_across_slices = 1;
  p.transform_skip = !d.lossless && e1_ts_on();   // the 4x4 luma blocks are coded with or without the transform, whichever is cheaper (oracle/hevc_enc.c hm_tb_finish)
  if (d.lossless) { p.transquant_bypass = 1; p.deblocking_control_present = 1; p.pps_deblocking_disabled = 1; p.loop_filter_across_slices = 0; }
  if (d.rows < 0) { p.entropy_coding_sync = 1; p.dependent_slice_segments = 1; }   // wavefront rows, one dependent slice segment each (oracle/hevc_enc.c setup_stream)
  if (!d.qp_map.empty()) { p.cu_qp_delta = 1; p.diff_cu_qp_delta_depth = 0; }     // a QP per CTB: the quantisation group is the CTB
}

// HBM layout of an encode batch. Every buffer of the arena is named here, once (Arena in rbt_batch.h: run without a base to measure, then over the allocation to bind),
// and so is every buffer a picture has elsewhere or not at all.
static void encode_lay_out(EncodeBatch& b, Arena& a) {
  const size_t nf = b.frames.size(), ns = b.slices.size();
  // the zero block (zeroed before the first kernel of every job): three launch tickets, then in wavefront mode per picture 2 * h_ctb progress words and two next-row counters
  const size_t z0 = a.mark();
  b.d_zero = a.take<uint8_t>(64); b.zero_bytes = a.used - z0;
  if (b.wpp) for (size_t i = 0; i < nf; i++) { b.frames[i].row_done = a.take<uint32_t>((size_t)b.frames[i].cfg.h_ctb * 2 + 2); b.zero_bytes = a.used - z0; }
  if (b.wpp) for (size_t i = 0; i < nf; i++) b.frames[i].row_ctx = a.take<uint8_t>((size_t)b.frames[i].cfg.h_ctb * 256);
  for (size_t i = 0; i < nf; i++) {
    RbtFrame& f = b.frames[i]; const RbtStreamCfg& c = f.cfg; const size_t ys = (size_t)c.w * c.h, cs = (size_t)c.cw * c.ch, u = (size_t)c.w4 * c.h4, nc = (size_t)c.w_ctb * c.h_ctb, u8 = (size_t)f.w8 * f.h8;
    const EncStreamDesc& d = b.desc[b.frame_stream[i]]; const size_t k = i - (size_t)b.stream_first[b.frame_stream[i]];
    // a padded copy of the source, unless the source already is a whole picture in coded geometry
    if (c.w != d.w || c.h != d.h || d.src_x0 || d.src_y0 || (d.src_stride && d.src_stride != d.w)) {
      uint16_t* pl[3]; a.take_planes(pl, ys, cs); const int st = d.src_stride ? d.src_stride : d.w;
      if (a.base) for (int q = 0; q < 3; q++) { const int sh = q ? 1 : 0;
        b.pad_jobs.push_back(PadJob{f.src[q], st >> sh, d.src_x0 >> sh, d.src_y0 >> sh, d.w >> sh, d.h >> sh, pl[q], c.w >> sh, c.h >> sh}); f.src[q] = pl[q]; }
    }
    // reconstruction and levels: in the decoded input picture's dead buffers where setup_encode found some (arena sharing), else here
    if (!d.alias_pix.empty() && d.alias_pix[k]) Arena::same_planes(f.pix, d.alias_pix[k], ys, cs); else a.take_planes(f.pix, ys, cs);
    if (!d.alias_coef.empty() && d.alias_coef[k]) Arena::same_planes(f.coef, d.alias_coef[k], ys, cs); else a.take_planes(f.coef, ys, cs);
    if (d.sao) a.take_planes(f.out, ys, cs); else Arena::same_planes(f.out, f.pix[0], ys, cs);      // no SAO: out = pix, wherever that is
    f.sao = a.take<RbtSao>(nc);
    f.pm = a.take<uint8_t>(u); f.edges = a.take<uint8_t>(u); f.qp = a.take<int8_t>(u); f.mv = a.take<int16_t>(u * 2); f.ref = a.take<int8_t>(u); f.refpoc = a.take<int32_t>(u);
    f.cu_log2 = a.take<uint8_t>(u8); f.cu_mode = a.take<uint8_t>(u8); f.cu_flags = a.take<uint8_t>(u8); f.cu_ts = a.take<uint8_t>(u8);
  }
  // the CTB -> slice maps of all pictures sit back to back: one upload per batch instead of one per picture (a copy is a queue entry of its own)
  size_t cs_words = 0; for (size_t i = 0; i < nf; i++) cs_words += (size_t)b.frames[i].cfg.w_ctb * b.frames[i].cfg.h_ctb;
  b.d_cs = a.take<uint16_t>(cs_words);
  if (a.base) { uint16_t* at = b.d_cs; for (size_t i = 0; i < nf; i++) { b.frames[i].ctb_slice = at; at += (size_t)b.frames[i].cfg.w_ctb * b.frames[i].cfg.h_ctb; } }
  // QP per CTB: the target maps, and per picture with a map the two bytes per CTB en_qp_fix_ctb keeps (RbtFrame::qp_pred); a batch without a map takes nothing here
  if (!b.qm_keep.empty()) {
    b.d_qm = a.take<int8_t>(b.qm_keep.size());
    for (size_t i = 0; i < nf; i++) if (b.frame_qm[i] >= 0) { uint8_t* pr = a.take<uint8_t>(2 * (size_t)b.frames[i].cfg.w_ctb * b.frames[i].cfg.h_ctb); if (a.base) { b.frames[i].qp_map = b.d_qm + b.frame_qm[i]; b.frames[i].qp_pred = pr; } }
  }
  b.d_frames = a.take<RbtFrame>(nf); b.d_slices = a.take<RbtSlice>(ns);
  if (a.base) for (size_t i = 0; i < nf; i++) if (b.desc[b.frame_stream[i]].src_flat_always) { b.frames[i].src_flat_one = 1; b.frames[i].src_flat = &b.d_frames[i].src_flat_one; }
  if (b.n_sums) b.d_sums = a.take<uint64_t>(b.n_sums);      // right behind the slices: one copy brings both back
  if (b.n_ctb_words) b.d_ctb_words = a.take<uint64_t>(b.n_ctb_words);
  b.d_lists = a.take<int32_t>((nf + ns) * 3); b.d_dst = a.take<uint32_t>(ns);
  // the packed output holds every slice back to back: as large as the slice buffers together, so that slices which fit their buffers always fit it (half of that, which
  // it had before, is less than noise needs in every QP band: DESIGN.md 9.5)
  b.d_out = a.take<uint8_t>(b.out_total); b.d_packed = a.take<uint8_t>(b.out_total);
  a.mark();
}

// host half of encode_build: parameter sets, pictures, slices and the size of the arena (b.arena_size); nothing is allocated
static int encode_plan(EncodeBatch& b) {
  size_t ns = b.desc.size();
  b.qm_keep.clear(); b.frame_qm.clear();
  b.sps.resize(ns); b.pps.resize(ns); b.stream_first.resize(ns);
  for (size_t si = 0; si < ns; si++) {
    const EncStreamDesc& d = b.desc[si];
    if (d.w % 2 || d.h % 2 || d.w <= 0 || d.h <= 0 || d.w > 8192 || d.h > 8192) { b.err = "picture size must be even and at most 8192"; return RBT_ERR_UNSUPPORTED; }
    if (d.log2_ctb && (d.log2_ctb < 4 || d.log2_ctb > 6)) { b.err = "log2_ctb must be 4..6"; return RBT_ERR_PARAM; }
    if ((d.rows < 0) != (b.desc[0].rows < 0)) { b.err = "streams of one call must agree on the wavefront mode (ctb_rows_per_slice < 0)"; return RBT_ERR_PARAM; }
    b.desc[si].sao = !d.lossless && e1_sao_on();
    make_param_sets(b.desc[si], b.sps[si], b.pps[si]);
    const Sps& s = b.sps[si]; const Pps& p = b.pps[si];
    b.stream_first[si] = (int)b.frames.size();
    if (!d.frame_qp.empty() && (d.lossless || d.gop < 1 || (int)d.frame_qp.size() * d.gop != d.n_frames)) { b.err = "internal: a QP list that does not match the stream's pictures"; return RBT_ERR_PARAM; }
    const size_t qm_n = (size_t)s.w_ctb * s.h_ctb;      // CTBs of a picture = entries of a frame's map
    if (!d.qp_map.empty() && (d.lossless || d.gop < 1 || !d.frame_qp.empty() || d.qm_w != s.w_ctb || d.qm_h != s.h_ctb || d.qp_map.size() * d.gop != qm_n * d.n_frames)) { b.err = "internal: a QP map that does not match the stream's pictures"; return RBT_ERR_PARAM; }
    for (int i = 0; i < d.n_frames; i++) {
      bool is_i = d.gop <= 1 || (i % d.gop) == 0;
      const int qp = d.frame_qp.empty() ? d.qp : d.frame_qp[(size_t)(i / d.gop)];      // only slice_qp_delta tells the pictures of a mixed-QP stream apart (write_slice_header: h.qp - init_qp)
      RbtFrame f; memset(&f, 0, sizeof(f));
      fill_stream_cfg(s, p, f.cfg);
      f.poc = is_i ? 0 : (i % d.gop); f.level = is_i ? 0 : 1; f.first_slice = (int)b.slices.size();
      f.w8 = s.width / 8; f.h8 = s.height / 8; f.lossless = d.lossless; f.enc_tools = e1_tools(d.lossless) & ~d.tools_off; f.ref_frame = is_i ? -1 : (int)b.frames.size() - 1; f.ref_poc = is_i ? 0 : f.poc - 1;
      for (int c = 0; c < 3; c++) f.src[c] = d.src[c][i];
      if (!d.src_flat.empty()) f.src_flat = d.src_flat[i];
      if (!d.hint_dm.empty()) { f.hint_pm = d.hint_pm[i]; f.hint_dm = d.hint_dm[i]; f.hint_w4 = d.hint_w4; f.hint_h4 = d.hint_h4; }
      if (!d.occ4.empty() && !d.lossless) { f.occ4 = d.occ4[i]; f.occ4_w = d.occ4_w; f.occ4_h = d.occ4_h; }
      int n_ctb = s.w_ctb * s.h_ctb, step = d.rows > 0 ? d.rows * s.w_ctb : (d.rows < 0 ? s.w_ctb : n_ctb);
      // a QP per CTB: the picture's targets T - the map of its frame with the constant-QP path's I / P rule applied (include/rbt.h "a QP per CTB", definition) - go to the batch's staging
      const int8_t* tq = nullptr;
      if (!d.qp_map.empty()) {
        const int8_t* m = d.qp_map.data() + (size_t)(i / d.gop) * qm_n; const size_t at = b.qm_keep.size();
        for (size_t c = 0; c < qm_n; c++) b.qm_keep.push_back((int8_t)std::min(51, std::max(0, is_i ? m[c] + d.i_qp_offset : (int)m[c])));
        b.frame_qm.push_back((int)at);
      } else b.frame_qm.push_back(-1);
      for (int addr = 0; addr < n_ctb; addr += step) {
        RbtSlice sl; memset(&sl, 0, sizeof(sl));
        sl.next_seg = -1; sl.wpp = (uint8_t)(d.rows < 0); sl.dependent = (uint8_t)(d.rows < 0 && addr > 0);
        sl.frame = (int)b.frames.size(); sl.ctb_addr = addr; sl.n_ctbs = std::min(step, n_ctb - addr);
        sl.slice_type = (int8_t)(is_i ? RBT_SLICE_I : RBT_SLICE_P);
        sl.qp = (int8_t)std::min(51, std::max(0, is_i ? qp + d.i_qp_offset : qp));
        // ... SliceQpY is T of the first CTB of the slice; the dependent segments of a wavefront picture belong to the slice that starts at CTB 0. The buffer is sized from the
        // lowest T of the segment's CTBs (through the bands below)
        int qp_cap = sl.qp;
        if (!d.qp_map.empty()) {
          tq = b.qm_keep.data() + b.frame_qm.back();
          sl.qp = tq[d.rows < 0 ? 0 : addr];
          qp_cap = 51; for (int c = 0; c < sl.n_ctbs; c++) qp_cap = std::min(qp_cap, (int)tq[addr + c]);
        }
        sl.deblocking_disabled = (uint8_t)p.pps_deblocking_disabled; sl.lf_across = (uint8_t)p.loop_filter_across_slices;
        sl.max_merge_cand = 1; sl.num_ref_idx = 1; sl.poc = f.poc; sl.sao_luma = sl.sao_chroma = (uint8_t)b.desc[si].sao;
        if (!is_i) { sl.ref_frame[0] = f.ref_frame; sl.ref_poc[0] = f.ref_poc; }
        // slice data buffer, by the slice's QP, in quarter bytes per luma sample of the slice: 17 for lossless streams, 14 below QP 16, 8 below QP 34, 5 from there on,
        // + slack. The figures are what the oracle (which has no caps) needs for noise pictures - the largest slices: 3.41 bytes per luma sample lossless, 2.74 at QP 0,
        // 1.64 at QP 16, 0.92 at QP 34 (DESIGN.md 9.5 has the table) - plus a fifth, rounded up. They are measured, not derived: log2(2^bit_depth / Qstep) bits per sample, the
        // entropy of a quantised sample, undercounts what CABAC spends - significance maps, greater-than flags and sign bits around every level, escape codes whose
        // Golomb-Rice prefix grows with the level (lossless two-level noise costs 18 bits a sample for 10-bit samples), and per-block syntax - so noise costs more than
        // its raw samples below QP 16. A slice that does not fit ends the call with RBT_ERR_OUTPUT (RbtSlice::out_size = 0xFFFFFFFF), it is never cut short.
        size_t rows = (size_t)(sl.n_ctbs + s.w_ctb - 1) / s.w_ctb;
        const int quarter_bytes_per_sample = d.lossless ? 17 : (qp_cap < 16 ? 14 : (qp_cap < 34 ? 8 : 5));
        sl.out_cap = (uint32_t)(rows * ((size_t)s.width << s.log2_ctb) * quarter_bytes_per_sample / 4 + 4096);
        f.n_slices++;
        b.slices.push_back(sl);
      }
      b.frames.push_back(f); b.frame_stream.push_back((int)si); b.frame_is_idr.push_back(is_i);
    }
  }
  if (b.slices.size() >= 0xFFFF) { b.err = "too many slice segments in one call"; return RBT_ERR_UNSUPPORTED; }
  b.wpp = false; for (auto& d : b.desc) b.wpp |= d.rows < 0;
  size_t out_cap_total = 0; for (auto& sl : b.slices) { sl.out_off = (uint32_t)out_cap_total; out_cap_total += sl.out_cap; }
  if (out_cap_total >= 0xFFFFFFFFull) { b.err = "output buffer too large for one call"; return RBT_ERR_UNSUPPORTED; }
  b.out_total = out_cap_total;
  Arena a; encode_lay_out(b, a);      // measure
  b.arena_size = a.used;
  return 0;
}
static int encode_build(EncodeBatch& b) {
  if (int rc = encode_plan(b)) return rc;
  b.arena = rbtk::dev_alloc(b.arena_size);      // allocate, bind
  if (!b.arena) { b.err = "device allocation failed"; return RBT_ERR_NOMEM; }
  Arena a{(uint8_t*)b.arena}; encode_lay_out(b, a);
  // per CTB: the SLICE it belongs to (index of the slice's independent segment): availability, QP and loop filter flags are per slice
  const size_t nf = b.frames.size(); b.cs_keep.clear();
  for (size_t i = 0; i < nf; i++) {
    const RbtFrame& f = b.frames[i]; const size_t at = b.cs_keep.size(); b.cs_keep.resize(at + (size_t)f.cfg.w_ctb * f.cfg.h_ctb, 0); int head = f.first_slice;
    for (int k = 0; k < f.n_slices; k++) { const RbtSlice& sl = b.slices[f.first_slice + k]; if (!sl.dependent) head = f.first_slice + k; for (int q = 0; q < sl.n_ctbs; q++) b.cs_keep[at + sl.ctb_addr + q] = (uint16_t)head; }
  }
  if (rbtk::h2d(b.d_cs, b.cs_keep.data(), b.cs_keep.size() * 2)) { b.err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  if (!b.qm_keep.empty() && rbtk::h2d(b.d_qm, b.qm_keep.data(), b.qm_keep.size())) { b.err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  // decoded picture hash SEI: the whole coded reconstruction (what a decoder outputs before cropping) after SAO
  b.hash_idx.assign(nf, -1);
  for (size_t i = 0; i < nf; i++) if (const int kind = b.desc[b.frame_stream[i]].md5) {
    const RbtFrame& f = b.frames[i];
    if ((b.hash_idx[i] = b.hash.add(f.out, f.cfg.w, f.cfg.h, f.cfg.bit_depth, kind)) < 0) { b.err = "picture cannot be hashed"; return RBT_ERR_UNSUPPORTED; }
  }
  if (rbtk::h2d(b.d_frames, b.frames.data(), nf * sizeof(RbtFrame)) || rbtk::h2d(b.d_slices, b.slices.data(), b.slices.size() * sizeof(RbtSlice))) { b.err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  return 0;
}

// runs the kernels and packs one Annex-B stream per input stream
// The encoder of one stream is enqueued in three steps so that nothing on the host waits for the GPU in between:
// encode_upload_lists (host -> device copies, issued while the stream is still empty), encode_launch_* (kernels up to the
// entropy coder, may be enqueued behind the decoder's kernels on the same stream), encode_finish (one sync, packing, NALs).
static int encode_upload_lists(EncodeBatch& b) {
  size_t nf = b.frames.size(), ns = b.slices.size();
  std::vector<int32_t>& lists = b.lists_keep; lists.clear(); b.n_i = b.n_ideb = b.n_p = 0;
  b.off_i = lists.size(); for (size_t i = 0; i < nf; i++) if (b.frame_is_idr[i]) { lists.push_back((int)i); b.n_i++; }
  // with RBT_FUSED_ENC_LF=1 pictures with SAO are deblocked inside the SAO kernel (en_sao_ctb: the CTB and a halo in LDS) and only pictures without it (RBT_ENC_SAO=0) take the in-place deblocking launches
  b.off_ideb = lists.size(); for (size_t i = 0; i < nf; i++) if (b.frame_is_idr[i] && !b.frames[i].lossless && (!b.desc[b.frame_stream[i]].sao || !e1_fused_lf())) { lists.push_back((int)i); b.n_ideb++; }
  b.n_pdeb = 0; b.off_pdeb = lists.size(); for (size_t i = 0; i < nf; i++) if (!b.frame_is_idr[i] && !b.frames[i].lossless && (!b.desc[b.frame_stream[i]].sao || !e1_fused_lf())) { lists.push_back((int)i); b.n_pdeb++; }
  b.off_p = lists.size(); for (size_t i = 0; i < nf; i++) if (!b.frame_is_idr[i]) { lists.push_back((int)i); b.n_p++; }
  b.n_isao = b.n_psao = 0;
  b.off_isao = lists.size(); for (size_t i = 0; i < nf; i++) if (b.frame_is_idr[i] && b.desc[b.frame_stream[i]].sao) { lists.push_back((int)i); b.n_isao++; }
  b.off_psao = lists.size(); for (size_t i = 0; i < nf; i++) if (!b.frame_is_idr[i] && b.desc[b.frame_stream[i]].sao) { lists.push_back((int)i); b.n_psao++; }
  // the pictures with a QP map (at most nf more entries: the lists hold 3 * (nf + ns), and a picture has a slice)
  b.n_iqm = b.n_pqm = 0;
  b.off_iqm = lists.size(); for (size_t i = 0; i < nf; i++) if (b.frame_is_idr[i] && b.frames[i].qp_map) { lists.push_back((int)i); b.n_iqm++; }
  b.off_pqm = lists.size(); for (size_t i = 0; i < nf; i++) if (!b.frame_is_idr[i] && b.frames[i].qp_map) { lists.push_back((int)i); b.n_pqm++; }
  // slice segments of the intra pictures first, then the rest: the two groups are entropy-coded by separate launches
  b.n_sl_i = b.n_sl_p = 0;
  b.off_sl = lists.size(); for (size_t i = 0; i < ns; i++) if (b.frame_is_idr[b.slices[i].frame]) { lists.push_back((int)i); b.n_sl_i++; }
  b.off_sl_p = lists.size(); for (size_t i = 0; i < ns; i++) if (!b.frame_is_idr[b.slices[i].frame]) { lists.push_back((int)i); b.n_sl_p++; }
  if (rbtk::h2d(b.d_lists, lists.data(), lists.size() * sizeof(int32_t))) { b.err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  if (!b.hash.empty() && b.hash.upload()) { b.err = "device allocation failed"; return RBT_ERR_NOMEM; }
  return 0;
}
// a batch that holds a picture with a QP map launches the encoder instantiations that read it, every other batch the constant-QP ones (rbtk::enc_qp_map_variant)
struct QpMapVariant { explicit QpMapVariant(const EncodeBatch& b) { rbtk::enc_qp_map_variant(!b.qm_keep.empty()); } ~QpMapVariant() { rbtk::enc_qp_map_variant(0); } };
// intra pictures (analysis, closed-loop intra coding, deblocking): they only read their own source pictures
static void encode_launch_intra(EncodeBatch& b) {
  QpMapVariant variant(b);
  size_t nf = b.frames.size();
  for (const PadJob& j : b.pad_jobs) rbtk::launch_pad(j.in, j.stride, j.x0, j.y0, j.w, j.h, j.out, j.dw, j.dh);
  int mw = 0, mh = 0, mu = 0, mc = 0, row_mode = 1, ml2 = 0, ml = 0;
  for (size_t i = 0; i < nf; i++) {
    const RbtStreamCfg& c = b.frames[i].cfg; ml = std::max(ml, c.w * c.h); ml2 = std::max(ml2, (int)c.log2_ctb); mw = std::max(mw, c.w_ctb); mh = std::max(mh, c.h_ctb); mu = std::max(mu, c.w4 * c.h4); mc = std::max(mc, c.w_ctb * c.h_ctb);
    if (b.desc[b.frame_stream[i]].rows != 1) row_mode = 0;
  }
  if (b.wpp) { row_mode = 2; rbtk::dev_memset(b.d_zero, 0, b.zero_bytes); }   // every stream of the batch is in wavefront mode (encode_build checks)
  rbtk::timer_begin(T_ANALYSE);
  rbtk::launch_enc_analyse(b.d_frames, b.d_slices, b.d_lists + b.off_i, b.n_i, mc);
  rbtk::timer_end(T_ANALYSE);
  rbtk::timer_begin(T_ENCODE);
  rbtk::launch_enc_intra(b.d_frames, b.d_slices, b.d_lists + b.off_i, b.n_i, mw, mh, row_mode, ml2, (uint32_t*)b.d_zero);
  if (b.n_iqm) rbtk::launch_enc_qp_fix(b.d_frames, b.d_slices, b.d_lists + b.off_iqm, b.n_iqm, mc);      // QP per CTB: the QpY the loop filters read, the predictors the entropy coder codes against
  rbtk::launch_deblock(b.d_frames, b.d_slices, b.d_lists + b.off_ideb, b.n_ideb, mu);
  rbtk::launch_enc_sao(b.d_frames, b.d_slices, b.d_lists + b.off_isao, b.n_isao, mc, ml2, e1_fused_lf());   // decides and applies
  rbtk::timer_end(T_ENCODE);
}
// entropy coding of the intra pictures' slices: needs nothing but their levels and CU data
static int max_log2_ctb(const EncodeBatch& b) { int m = 0; for (auto& f : b.frames) m = std::max(m, (int)f.cfg.log2_ctb); return m; }
static int max_w_ctb(const EncodeBatch& b) { int m = 0; for (auto& f : b.frames) m = std::max(m, (int)f.cfg.w_ctb); return m; }
static int max_h_ctb(const EncodeBatch& b) { int m = 0; for (auto& f : b.frames) m = std::max(m, (int)f.cfg.h_ctb); return m; }
static void encode_launch_entropy_intra(EncodeBatch& b) {
  QpMapVariant variant(b);
  rbtk::timer_begin(T_ENTROPY_I);
  if (b.wpp) rbtk::launch_entropy_wave(b.d_frames, b.d_slices, b.d_out, b.d_lists + b.off_i, b.n_i, max_w_ctb(b), max_h_ctb(b), max_log2_ctb(b), (uint32_t*)b.d_zero + 1);
  else rbtk::launch_entropy(b.d_frames, b.d_slices, b.d_out, b.d_lists + b.off_sl, b.n_sl_i, max_log2_ctb(b));
  rbtk::timer_end(T_ENTROPY_I);
}
// inter pictures (need the reconstructed intra pictures and their own sources); after them every reconstruction is final
static void encode_launch_inter(EncodeBatch& b) {
  QpMapVariant variant(b);
  size_t nf = b.frames.size();
  int mu = 0, mc = 0, ml = 0;
  for (size_t i = 0; i < nf; i++) { const RbtStreamCfg& c = b.frames[i].cfg; mu = std::max(mu, c.w4 * c.h4); mc = std::max(mc, c.w_ctb * c.h_ctb); ml = std::max(ml, c.w * c.h); }
  rbtk::timer_begin(T_INTER);
  rbtk::launch_enc_inter(b.d_frames, b.d_slices, b.d_lists + b.off_p, b.n_p, mc);
  if (b.n_pqm) rbtk::launch_enc_qp_fix(b.d_frames, b.d_slices, b.d_lists + b.off_pqm, b.n_pqm, mc);
  rbtk::launch_deblock(b.d_frames, b.d_slices, b.d_lists + b.off_pdeb, b.n_pdeb, mu);
  rbtk::launch_enc_sao(b.d_frames, b.d_slices, b.d_lists + b.off_psao, b.n_psao, mc, max_log2_ctb(b), e1_fused_lf());
  rbtk::timer_end(T_INTER);
}
// the entropy coder for the inter pictures' slices
static void encode_launch_entropy_rest(EncodeBatch& b) {
  QpMapVariant variant(b);
  rbtk::timer_begin(T_ENTROPY);
  if (b.wpp) rbtk::launch_entropy_wave(b.d_frames, b.d_slices, b.d_out, b.d_lists + b.off_p, b.n_p, max_w_ctb(b), max_h_ctb(b), max_log2_ctb(b), (uint32_t*)b.d_zero + 2);
  else rbtk::launch_entropy(b.d_frames, b.d_slices, b.d_out, b.d_lists + b.off_sl_p, b.n_sl_p, max_log2_ctb(b));
  rbtk::timer_end(T_ENTROPY);
}
static int encode_finish(EncodeBatch& b, std::vector<std::vector<uint8_t>>& outs, rbt_stats& st) {
  size_t nf = b.frames.size(), ns = b.slices.size();
  if (b.n_sums) {      // the slice sizes and the distortion words in one copy: the span from the slice table to the end of the words
    const size_t off = (size_t)((uint8_t*)b.d_sums - (uint8_t*)b.d_slices); std::vector<uint8_t> span(off + b.n_sums * 8);
    if (rbtk::d2h(span.data(), b.d_slices, span.size())) { b.err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
    memcpy(b.slices.data(), span.data(), ns * sizeof(RbtSlice)); b.sums.resize(b.n_sums); memcpy(b.sums.data(), span.data() + off, b.n_sums * 8);
  } else
  if (rbtk::d2h(b.slices.data(), b.d_slices, ns * sizeof(RbtSlice))) { b.err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  std::vector<uint32_t> dst(ns); size_t total = 0;
  // (the packed buffer is as large as the slice buffers together: total <= out_total once every slice fits)
  for (size_t i = 0; i < ns; i++) { if (b.slices[i].out_size > b.slices[i].out_cap) { b.err = "slice data exceeds its buffer"; return RBT_ERR_OUTPUT; } dst[i] = (uint32_t)total; total += b.slices[i].out_size; }
  std::vector<uint8_t> packed(total);
  if (rbtk::h2d(b.d_dst, dst.data(), ns * sizeof(uint32_t))) { b.err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  rbtk::launch_pack(b.d_out, b.d_slices, b.d_dst, b.d_packed, (int)ns);
  double t0 = now_ms();
  if (total && rbtk::d2h(packed.data(), b.d_packed, total)) { b.err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  if (rbtk::dev_sync()) { b.err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  if (!b.hash.empty() && b.hash.fetch()) { b.err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }   // 48 bytes per picture
  st.d2h_ms += now_ms() - t0;
  // ---- NAL packing (parameter sets, slice headers, emulation prevention) ----
  double t1 = now_ms();
  outs.assign(b.desc.size(), {}); b.pic_at.assign(b.desc.size(), {});
  for (size_t i = 0; i < nf; i++) {
    int si = b.frame_stream[i]; const Sps& s = b.sps[si]; const Pps& p = b.pps[si]; std::vector<uint8_t>& out = outs[si]; const RbtFrame& f = b.frames[i];
    bool idr = b.frame_is_idr[i] != 0;
    b.pic_at[si].push_back(out.size());
    if (idr) write_param_sets(out, s, p);
    for (int k = 0; k < f.n_slices; k++) {
      const RbtSlice& sl = b.slices[f.first_slice + k];
      SliceHdr h; h.first_slice_in_pic = k == 0; h.dependent = sl.dependent; h.segment_addr = sl.ctb_addr; h.slice_type = sl.slice_type; h.poc = sl.poc; h.num_ref_idx = 1; h.max_merge_cand = 1; h.qp = sl.qp;
      h.sao_luma = sl.sao_luma; h.sao_chroma = sl.sao_chroma; h.deblocking_disabled = sl.deblocking_disabled; h.beta_offset_div2 = p.beta_offset_div2; h.tc_offset_div2 = p.tc_offset_div2; h.lf_across = sl.lf_across;
      BitWriter w; write_slice_header(w, s, p, h, idr, 0);
      w.b.insert(w.b.end(), packed.begin() + dst[f.first_slice + k], packed.begin() + dst[f.first_slice + k] + sl.out_size);
      append_nal(out, idr ? NAL_IDR_W_RADL : NAL_TRAIL_R, w.b.data(), w.b.size(), k == 0);
    }
    if (b.hash_idx[i] >= 0) append_hash_sei(out, b.desc[si].md5, &b.hash.out[(size_t)b.hash_idx[i] * 48]);
  }
  st.host_pack_ms += now_ms() - t1;
  { int cur = b.main_stream; if (b.aux_stream >= 0) rbtk::set_stream(b.aux_stream);
    st.k_analyse_ms += rbtk::timer_ms(T_ANALYSE); st.k_encode_ms += rbtk::timer_ms(T_ENCODE); st.k_entropy_ms += rbtk::timer_ms(T_ENTROPY_I);
    if (b.aux_stream >= 0) rbtk::set_stream(cur);
    st.k_encode_ms += rbtk::timer_ms(T_INTER); st.k_entropy_ms += rbtk::timer_ms(T_ENTROPY); }
  return 0;
}

static int encode_run(EncodeBatch& b, std::vector<std::vector<uint8_t>>& outs, rbt_stats& st) {
  if (int rc = encode_upload_lists(b)) return rc;
  encode_launch_intra(b); encode_launch_entropy_intra(b); encode_launch_inter(b);
  if (!b.hash.empty()) b.hash.launch();
  encode_launch_entropy_rest(b);
  return encode_finish(b, outs, st);
}

static int hand_out(const std::vector<std::vector<uint8_t>>& outs, uint8_t** out, size_t* n_out) {
  for (size_t i = 0; i < outs.size(); i++) {
    out[i] = (uint8_t*)malloc(outs[i].size() ? outs[i].size() : 1);
    if (!out[i]) { for (size_t k = 0; k < i; k++) { free(out[k]); out[k] = nullptr; } return RBT_ERR_NOMEM; }
    memcpy(out[i], outs[i].data(), outs[i].size()); n_out[i] = outs[i].size();
  }
  return 0;
}

// Pool + encoder setup for the one stream of `db` (PCCTranscoder.cpp:466, :825-904).
// Row-band parsing of the longest pipeline (resumable parser + reconstruction of finished bands underneath the rest of the
// parse). Measured on the 32-frame GOF: every band ends with the slowest slice OF THAT BAND, and the sum of those maxima
// exceeds the single maximum by more than the hidden reconstruction saves (4 bands: 311.9 ms, 2 bands: 302.6 ms, off:
// 297.3 ms). Off by default; RBT_PARSE_BANDS=<n> in the environment turns it on for experiments.
static int parse_bands() { static int v = -1; if (v < 0) { const char* e = getenv("RBT_PARSE_BANDS"); v = e ? atoi(e) : 1; if (v < 1) v = 1; if (v > 16) v = 16; } return v; }
struct PoolJob { const uint16_t* in; int stride, w, h; uint16_t *y, *cb, *cr; int grey; };
// occupancy-aware coding: the occupancy maps per 4x4 luma unit (RbtFrame::occ4) that the geometry / attribute streams of a GOF are coded with, made from the pooled
// occupancy pictures of that GOF's occupancy stream by one launch on the occupancy pipeline's stream
struct OccSource { const uint16_t* occ = nullptr; size_t in_step = 0; int n = 0, ow = 0, oh = 0, pipeline = -1; };   // the pooled luma planes of one occupancy stream
struct OccJob { int source; uint8_t* maps; int W, w4, h4; };                                                           // one launch_occ_units: the maps of one consumer stream
// pool_jobs != nullptr: the OR-pool launches are recorded instead of issued (the decoder's kernels are not enqueued yet)
// stream `si` of the decode batch becomes stream `ei` of the encode batch (several target rate points may re-encode one decoded
// stream: BASELINE.json configs[4], rate fan-out)
static int setup_encode(DecodeBatch& db, int si, int ei, const rbt_stream_params& p, EncodeBatch& eb, std::vector<void*>& pooled, std::string& err, std::vector<PoolJob>* pool_jobs = nullptr, const OccSource* occ = nullptr, int occ_index = -1, std::vector<OccJob>* occ_jobs = nullptr) {
  if ((int)eb.desc.size() <= ei) eb.desc.resize((size_t)ei + 1);
  EncStreamDesc& d = eb.desc[ei]; int first = db.stream_first[si], cnt = db.stream_count[si];
  const RbtStreamCfg& c = db.frames[first].cfg; const Sps& isps = db.stream_sps[si];
  // what a player shows of the input: the coded picture minus its conformance window
  const int cl = 2 * isps.conf_win[0], ct = 2 * isps.conf_win[2], dw = c.w - cl - 2 * isps.conf_win[1], dh = c.h - ct - 2 * isps.conf_win[3];
  if (dw <= 0 || dh <= 0) { err = "empty conformance window"; return RBT_ERR_BITSTREAM; }
  if (p.preset != RBT_PRESET_DEFAULT && p.preset != RBT_PRESET_FAST) { err = "preset must be RBT_PRESET_DEFAULT or RBT_PRESET_FAST"; return RBT_ERR_PARAM; }
  if (p.md5_sei < RBT_HASH_NONE || p.md5_sei > RBT_HASH_CHECKSUM) { err = "md5_sei must be an RBT_HASH_* kind"; return RBT_ERR_PARAM; }
  d.bd = c.bit_depth; d.n_frames = cnt; d.qp = p.qp; d.log2_ctb = p.log2_ctb; d.rows = p.ctb_rows_per_slice; d.md5 = p.md5_sei; d.tools_off = p.preset == RBT_PRESET_FAST ? (RBT_ET_SATD | RBT_ET_REFINE | RBT_ET_RQ | RBT_ET_RDM) : 0;
  for (int k = 0; k < 3; k++) d.src[k].resize(cnt);
  auto view = [&](int k, int q) { return (const uint16_t*)db.frames[first + k].out[q]; };
  // flat chroma: a window of a flat decoded picture, and its padding, are flat; the pooled occupancy maps are flat by construction
  d.src_flat.resize(cnt); for (int k = 0; k < cnt; k++) d.src_flat[k] = &db.d_frames[first + k].chroma_flat;
  if (p.video_type == RBT_VIDEO_OCCUPANCY) {
    int factor = p.occupancy_precision / 2; if (factor < 1) factor = 1;
    d.gop = 1; d.lossless = 1; d.i_qp_offset = 0; d.w = dw / factor; d.h = dh / factor;
    if (p.occupancy_precision == 4) {
      if (dw % 4 || dh % 4) { err = "occupancy map size must be a multiple of 4 to pool"; return RBT_ERR_UNSUPPORTED; }
      size_t ys = (size_t)d.w * d.h, cs = (size_t)(d.w / 2) * (d.h / 2);
      uint16_t* buf = (uint16_t*)rbtk::dev_alloc((ys + 2 * cs) * 2 * (size_t)cnt);
      if (!buf) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
      pooled.push_back(buf);
      if (!pool_jobs) rbtk::timer_begin(T_POOL);
      for (int k = 0; k < cnt; k++) {
        uint16_t* y = buf + (ys + 2 * cs) * (size_t)k;
        const uint16_t* in = view(k, 0) + (size_t)ct * c.w + cl;
        // the reference leaves the pooled chroma planes unwritten (PCCTranscoder.cpp:638-641); mid-grey here
        if (pool_jobs) pool_jobs->push_back(PoolJob{in, c.w, dw, dh, y, y + ys, y + ys + cs, 1 << (c.bit_depth - 1)});
        else rbtk::launch_pool(in, c.w, dw, dh, 2, y, y + ys, y + ys + cs, 1 << (c.bit_depth - 1));
        d.src[0][k] = y; d.src[1][k] = y + ys; d.src[2][k] = y + ys + cs;
      }
      d.src_flat.clear(); d.src_flat_always = true;
      if (!pool_jobs) rbtk::timer_end(T_POOL);
    } else { d.src_stride = c.w; d.src_x0 = cl; d.src_y0 = ct; for (int k = 0; k < cnt; k++) for (int q = 0; q < 3; q++) d.src[q][k] = view(k, q); }
  } else {
    d.gop = 2; d.lossless = 0; d.i_qp_offset = -3; d.w = dw; d.h = dh;
    d.src_stride = c.w; d.src_x0 = cl; d.src_y0 = ct;
    for (int k = 0; k < cnt; k++) for (int q = 0; q < 3; q++) d.src[q][k] = view(k, q);
    // arena sharing: the encoder's levels and reconstruction of picture k live in the decoded picture k's dead buffers when the two pictures have one geometry (coded size
    // = the input's coded size, no window offset) and no other target rate of a fan-out took them already. RBT_ARENA_SHARE=0 switches it off.
    // (what orders the encoder's first write to such a buffer behind the decoder's last read of it: enqueue_pipeline)
    // tests/test_arena_share.py runs the same transcodes with the switch off and on.
    { static const int share = [] { const char* e = getenv("RBT_ARENA_SHARE"); return !e || atoi(e) != 0; }();
      if (db.alias_taken.size() < db.stream_first.size()) db.alias_taken.resize(db.stream_first.size(), 0);
      if (share && cl == 0 && ct == 0 && coded_size(dw, 2) == c.w && coded_size(dh, 2) == c.h && !db.alias_taken[si]) {
        db.alias_taken[si] = 1;
        d.alias_pix.assign(cnt, nullptr); d.alias_coef.assign(cnt, nullptr);
        for (int k = 0; k < cnt; k++) {
          const RbtFrame& fr = db.frames[first + k];
          if (fr.cfg.w != c.w || fr.cfg.h != c.h) continue;
          d.alias_coef[k] = fr.coef[0];
          if (fr.out[0] != fr.pix[0]) d.alias_pix[k] = fr.pix[0];        // pictures with SAO: the deblocked samples are dead once the SAO output exists
        }
      } }
    // the input stream's intra modes come along as hints for the re-encode (same sample grid: not with a window offset at the left / top; oracle/vpcc_path.c)
    if (cl == 0 && ct == 0) {
      d.hint_pm.resize(cnt); d.hint_dm.resize(cnt); d.hint_w4 = c.w4; d.hint_h4 = c.h4;
      for (int k = 0; k < cnt; k++) { d.hint_pm[k] = db.frames[first + k].pm; d.hint_dm[k] = db.frames[first + k].dm; }
    }
    // occupancy-aware coding (oracle/vpcc_path.c transcode_substream_occ): picture k belongs to occupancy frame k * n_occ / cnt; the occupancy video must be the
    // atlas scaled down by a whole factor, else every sample counts
    if (occ && occ_jobs && occ->n > 0 && cnt % occ->n == 0 && dw % occ->ow == 0 && dh % occ->oh == 0 && dw / occ->ow == dh / occ->oh) {
      const int w4 = (dw + 3) / 4, h4 = (dh + 3) / 4;
      uint8_t* maps = (uint8_t*)rbtk::dev_alloc((size_t)occ->n * w4 * h4);
      if (!maps) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
      pooled.push_back(maps); occ_jobs->push_back(OccJob{occ_index, maps, dw, w4, h4});
      d.occ4.resize(cnt); d.occ4_w = w4; d.occ4_h = h4;
      for (int k = 0; k < cnt; k++) d.occ4[k] = maps + (size_t)((size_t)k * occ->n / cnt) * w4 * h4;
    }
  }
  return 0;
}

// The sub-bitstreams of a GOF are independent (PCCTranscoder.cpp:122-165 transcodes them one after the other), so each
// gets its own decode/encode batch on its own HIP stream: every decode chain is enqueued up front, longest first, and
// the host then walks the streams shortest first, so the pool / re-encode of the short streams (occupancy, geometry)
// runs underneath the entropy-decoding chain of the longest one (attribute) instead of behind it.
// One transcode call in flight. rbt_transcode_gof = submit + wait; rbt_submit_gof / rbt_wait_gof expose the two halves so that
// a caller can keep two GOFs in flight (job slots use disjoint HIP streams): the next GOF's entropy decoding then runs
// underneath the previous GOF's reconstruction and re-encode.
// Targets - a byte budget or a PSNR floor per entry -: what a pipeline with such an entry keeps between the rounds of its trial encodes (run_rounds, launch_round, finish_round)
struct RoundCand { int q, qp, walk; int fw = -1; FramePass pass; int pw = -1; std::vector<int8_t> qmap; };   // entry q of the group at qp; walk: index of its walk, -1 for a constant-QP entry of the pipeline; fw >= 0: a pass of the entry's frame walks (qp: the entry's own, for the parameter sets)
struct TargetTried : QualityTried { std::vector<rbt_d1_result> d1; std::vector<rbt_d2_result> d2; std::vector<rbt_color_result> color; };      // d1 / d2 / color: a job with D1 / D2 / colour floors, the frames of the trial
// A budget (toward < 0) or a floor (toward > 0, rbt_floor_walk.h) - on the PSNR of `region` at bit_depth, on D1 or on the colour PSNR of `channel` of the clouds, stat over the frames
enum WalkKind { WALK_BUDGET, WALK_PSNR, WALK_D1, WALK_COLOR };
struct TargetWalk : QpWalk<TargetTried> { WalkKind kind = WALK_BUDGET; RateGoal budget; FloorGoal floor; int region = 0, bit_depth = 8, stat = RBT_D1_MIN, channel = 0; bool d2 = false; };      // d2: a WALK_D1 on the D2 figure
// Quality floors: the occupancy source of an entry (include/rbt.h, "transcoding to a PSNR floor", rule 3), kept in the job because the pipelines that use it are encoded in
// the wait half: the pooled luma planes of the occupancy stream, and for occupancy_rd the per-4x4-unit maps made of them (both live in GofJob::pooled until the job goes)
struct QualityOcc { const uint16_t* occ = nullptr; size_t in_step = 0; int n = 0, ow = 0, oh = 0; const uint8_t* maps = nullptr; int w4 = 0, h4 = 0; };
// Floors held patch by patch: the walk of one point-cloud frame (rbt_patch_walk.h) with what its last trial brought - the frame's NAL units, the sums of its two pictures,
// the payload of the job's kind of figure (PatchPsnr, PatchD1, PatchD2 or PatchColor, the others stay empty), the map it was coded with - and the walks of one entry: per frame R_k in CTB units
// (the rectangles k_patch_fold reads, on the device from the first round to the last) and the displayed samples of R_k in both pictures
struct PatchFrame { PatchWalk w; std::vector<uint8_t> stream; QualitySums sums; PatchPsnr psnr; PatchD1 d1; PatchD2 d2; PatchColor color; std::vector<int8_t> map; std::vector<int32_t> rects; std::vector<uint64_t> samples; size_t rect_off = 0; };
struct PatchWalks {
  int q = 0, entry = 0, n_passes = 0, l2 = 5, wc = 0, hc = 0, W = 0, H = 0, bit_depth = 8; std::vector<PatchFrame> frames; int32_t* d_rects = nullptr;
  bool settled() const { for (const PatchFrame& f : frames) if (!f.w.settled) return false; return true; }
};
// the tables of k_ctb_sse and k_patch_fold for the round in flight, used like SseSet: one upload before the round's first kernel, the launches behind its last filter
struct CtbSseSet {
  std::vector<RbtCtbSsePic> pics; std::vector<RbtFoldJob> jobs; int max_ctbs = 0, max_rects = 0; std::vector<uint8_t> staging; uint8_t* d = nullptr; size_t o_jobs = 0;
  int upload() {
    o_jobs = (pics.size() * sizeof(RbtCtbSsePic) + 255) & ~(size_t)255;
    staging.assign(o_jobs + jobs.size() * sizeof(RbtFoldJob), 0);
    memcpy(staging.data(), pics.data(), pics.size() * sizeof(RbtCtbSsePic)); memcpy(staging.data() + o_jobs, jobs.data(), jobs.size() * sizeof(RbtFoldJob));
    d = (uint8_t*)rbtk::dev_alloc(staging.size());
    if (!d) return RBT_ERR_NOMEM;
    return rbtk::h2d(d, staging.data(), staging.size()) ? RBT_ERR_NO_DEVICE : 0;
  }
  void launch() const { rbtk::launch_ctb_sse((const RbtCtbSsePic*)d, (int)pics.size(), max_ctbs); rbtk::launch_patch_fold((const RbtFoldJob*)(d + o_jobs), (int)jobs.size(), max_rects); }
  ~CtbSseSet() { rbtk::dev_free(d); }
};
struct RoundPipe {
  std::vector<PatchWalks> pwalks; std::unique_ptr<CtbSseSet> ctbsse;   // a job with floors held patch by patch: per entry with a target its frames' walks; the round's tables
  std::vector<TargetWalk> walks; std::vector<int> n_enc;
  std::vector<FrameWalks<TargetWalk>> fwalks;  // a job with floors held frame by frame: per entry of the group one walk per point-cloud frame
  std::vector<RoundCand> cands;                // the round to run (eb == nullptr) or running
  std::unique_ptr<EncodeBatch> eb; std::unique_ptr<SseSet> sse;   // the round in flight on the pipeline's stream; sse: a round of a job with floors carries distortion sums
  std::vector<std::vector<uint8_t>> o1; std::vector<QualitySums> sums;   // the pipeline's streams in group order, as they settle, and (floors) their sums
  std::vector<std::vector<rbt_d1_result>> d1;  // (D1 floors) the frames of the constant-QP entries with a target, in group order
  std::vector<std::vector<rbt_d2_result>> d2;  // (D2 floors) the same
  std::vector<std::vector<rbt_color_result>> color;   // (colour floors) the same
  bool done = false;
};
// Cloud targets - D1 floors and colour floors -, what the two kinds share of the target of one entry as the job keeps it: the patch lists copied, the reference clouds
// (nullptr = the cloud of the decoded input), where the decoded input of the occupancy source lies and the device time of the clouds' work
struct CloudEntry { std::vector<std::vector<rbt_patch>> patches; std::vector<const PCloud*> ref; int in_pipe = -1, in_ds = -1, in_ow = 0, in_oh = 0; double cloud_ms = 0; };
// D1 floors: the target of one entry (n_frames 0: none) as the job keeps it, and what its clouds are rebuilt from. The decoded input of the occupancy source (in_*: the
// pipeline and decoded stream that hold it, its displayed size) is what the reference clouds of frames without a handle are made of; the trials' clouds use the pooled
// planes (GofJob::qocc). frames / own_ref live while run_rounds runs (D1Live).
struct D1Entry : CloudEntry { rbt_d1_target t; std::vector<MapFrame*> frames; std::vector<PCloud*> own_ref; };
// Colour floors: the target of one attribute entry (n_frames 0: none) as the job keeps it. geo: the entry that is its geometry source; in_* : where the decoded input of
// the occupancy source lies, as D1Entry has it. frames: the geometry half of every frame (ColorFrame, rbt_pcc.h), made behind the geometry pipeline's encode from its
// reconstruction's luma (geo_planes, packed) and kept until the attribute pipeline's rounds end; own_ref: the same for the decoded input, where no handle was given.
struct ColorEntry : CloudEntry { rbt_color_target t; int geo = -1; uint16_t* geo_planes = nullptr; uint16_t* in_planes = nullptr; std::vector<ColorFrame*> frames, own_ref; };
// what a pipeline's rounds leave of an entry with a cloud target: the walk's result - or the entry's own QP - and the frames' figures there
template <class Result> struct FloorOut { int qp = 0, q0 = 0, qs = 0, met = 0, n_enc = 0; uint64_t bytes = 0; std::vector<Result> frames; double cloud_ms = 0; };
// what a pipeline's rounds leave of an entry of a job with floors held patch by patch, either kind: the header, per frame its trials and bytes with the payload of its
// settling trial, and every frame's picks back to back. An entry without a target has no frames: q0, bytes, bit_depth and sums are those of its only encode
struct PatchOut {
  int q0 = 0, n_passes = 0, wc = 0, hc = 0, bit_depth = 8, region = 0; uint64_t bytes = 0, pictures = 0; std::vector<int8_t> map; QualitySums sums; double cloud_ms = 0;
  struct Frame { int n_trials = 0, met = 1, n_patches = 0; uint64_t bytes = 0; PatchPsnr psnr; PatchD1 d1; PatchD2 d2; PatchColor color; }; std::vector<Frame> frames;
  struct Pick { int qp, met, failed; double figure; }; std::vector<Pick> picks;
};
struct FrameFloorOut { int q0 = 0, n_passes = 0, bit_depth = 8; std::vector<rbt_frame_pick> frames; std::vector<rbt_d1_result> d1; double cloud_ms = 0; uint64_t bytes = 0, pictures = 0; QualitySums sums; };
struct GofJob {
  int n = 0, slot = 0, ng = 0, rc = 0; GofKind kind = GOF_PLAIN;      // kind: which submit made the job, fixed there
  std::vector<std::vector<int>> groups; std::vector<int> order;
  std::vector<DecodeBatch> db; std::vector<EncodeBatch> eb; std::vector<char> chained;
  std::vector<void*> pooled;
  bool has_aux = true;
  std::vector<int> phys;                       // HIP stream of each pipeline
  std::vector<char> parse_timed;               // pipeline recorded its own T_PARSE timer
  std::vector<std::vector<RbtParseTask>> tasks_keep;   // host staging of merged parse launches, alive until the job is collected
  std::vector<std::vector<RbtFrameRef>> refs_keep;     // ... and of merged reconstruction launches
  std::vector<char> recon_timed;
  std::vector<rbt_stream_params> params; std::vector<size_t> n_in;
  std::vector<std::vector<uint8_t>> passthrough;   // transcodeData (PCCTranscoder.cpp:150): occupancy is only transcoded when occupancyPrecision == 4; else the stream stays as it is
  std::vector<char> is_pass;
  std::vector<std::vector<int>> dec_of;            // per pipeline: decode stream of each of its (encode) streams - identical inputs are decoded once
  // rate targets (rbt_submit_gof_rate): a pipeline that holds a targeted entry is decoded and counted at submit and encoded in the wait half (run_rounds)
  std::vector<rbt_rate_target> targets; std::vector<char> rate_pipe; std::vector<rbt_rate_result> results; size_t rate_bytes = 0;   // rate_bytes: arenas of the first round of trial encodes
  std::vector<RoundPipe> pipes;                              // per pipeline
  // quality floors (rbt_submit_gof_quality): every pipeline with a geometry / attribute entry is decoded at submit and encoded in the wait half (run_rounds); it is marked
  // in rate_pipe like a pipeline with a rate target, which keeps it unchained
  std::vector<rbt_quality_target> qtargets; std::vector<QualityOcc> qocc; std::vector<rbt_quality_result> qresults; bool refused = false;
  // D1 floors (rbt_submit_gof_d1): the job runs as a job with quality floors that are all 0 - every geometry / attribute pipeline is encoded in the wait half, the pooled
  // occupancy planes and the maps of occupancy_rd stay in the job - and d1 holds the targets with their patch lists copied (d1_setup, d1_score, run_rounds)
  std::vector<D1Entry> d1; std::vector<FloorOut<rbt_d1_result>> d1out; PCloudCache* cloud_cache = nullptr;
  // colour floors (rbt_submit_gof_color): the same kind of job; the geometry pipelines' rounds run before the attribute pipelines' (gof_wait), because the clouds' geometry
  // half is made behind the geometry encode (color_geometry) and recoloured per attribute trial (color_setup, color_score)
  std::vector<ColorEntry> color; std::vector<FloorOut<rbt_color_result>> colorout;
  // a QP per point-cloud frame (rbt_submit_gof_frame_qp): per entry the list, empty = the entry's own QP; such a job is an ordinary constant-QP job in every other respect
  std::vector<std::vector<int8_t>> frame_qp;
  std::vector<QpMapIn> qp_maps;      // a QP per CTB (rbt_submit_gof_qp_map): per entry the maps, an empty qp = none; the job is a constant-QP job otherwise, as with frame_qp
  // floors held frame by frame (rbt_submit_gof_quality_frames): a job with quality floors whose pipelines walk every frame on its own (RoundPipe::fwalks)
  bool per_frame = false; std::vector<FrameFloorOut> fout;
  // floors held patch by patch (rbt_submit_gof_quality_patches): a job with quality floors that are all 0, like a job with cloud targets; the entries with a target walk
  // every frame's patches (RoundPipe::pwalks), the others are coded once at their own QP
  std::vector<PatchFloorIn> patch; std::vector<PatchOut> pout;
  // D1 floors held patch by patch (rbt_submit_gof_d1_patches): such a job with the figures taken from the trial's cloud - d1 holds the targets' clouds' side as in a job
  // with D1 floors (no walk of its own: min_d1_mdb 0), every pass is scored by d1_score patch by patch (PatchFrame::d1), no sums per CTB run
  bool patch_d1 = false;
  // D2 floors (rbt_submit_gof_d2, rbt_submit_gof_d2_patches): a job with D1 floors, on the stream or patch by patch, whose figure is D2 - d1 holds the targets (min_d1_mdb:
  // the D2 floor), d1_score asks for the D2 part too, the reference clouds made of the decoded input get normals in d1_setup (normals: one record per entry)
  bool d2 = false; std::vector<NormalsIn> normals; std::vector<FloorOut<rbt_d2_result>> d2out;
  // colour floors held patch by patch (rbt_submit_gof_color_patches): a job with floors held patch by patch whose figures come from the trial's cloud, as patch_d1 - color
  // holds the targets' clouds' side as in a job with colour floors (no walk of its own: min_psnr_mdb 0), so the geometry pipelines run first and leave the clouds'
  // geometry half; every pass is scored by color_score patch by patch (PatchFrame::color), no sums per CTB run
  bool patch_color = false;
  bool patch_clouds() const { return patch_d1 || patch_color; }      // the figures per patch come from the trial's cloud
  rbt_stats st; std::string err; double t_all = 0, t_gpu = 0; size_t dev_bytes = 0;
  void color_release(int entry) {        // the frames' volumes go back to the context's cache; their streams have been waited for
    ColorEntry& E = color[entry];
    for (ColorFrame* F : E.frames) colorframe_delete(*cloud_cache, F);
    for (ColorFrame* F : E.own_ref) colorframe_delete(*cloud_cache, F);
    E.frames.clear(); E.own_ref.clear();
    rbtk::dev_free(E.geo_planes); rbtk::dev_free(E.in_planes); E.geo_planes = nullptr; E.in_planes = nullptr;
  }
  ~GofJob() { for (size_t i = 0; i < color.size(); i++) color_release((int)i); for (void* q : pooled) rbtk::dev_free(q); }
};
static int job_stream(const GofJob& j, int pipeline) { return j.slot * rbtk::RBT_STREAMS_PER_JOB + pipeline; }

// Streams of a job. The 16 HIP streams are shared out by the pipeline depth the caller announced (rbt_set_depth): up to 4 jobs
// in flight get four streams each (three pipelines + the auxiliary stream), 5 get three (no auxiliary stream), up to 8 get two
// (the longest pipeline alone, the others behind each other on the second).
static void bind_streams(GofJob& j, int depth) {
  const int spj = depth <= 4 ? 4 : depth == 5 ? 3 : depth <= 8 ? 2 : 1, base = j.slot * spj;
  j.has_aux = spj == 4;
  j.phys.assign(j.ng, 0);
  for (int k = 0; k < j.ng; k++) { j.phys[j.order[k]] = base + (k == 0 || spj == 1 ? 0 : 1 + (k - 1) % (std::min(spj, 3) - 1)); rbtk::map_lane(job_stream(j, j.order[k]), j.phys[j.order[k]]); }
  rbtk::map_lane(job_stream(j, rbtk::RBT_AUX_STREAM), base + spj - 1);
}

size_t gof_memory(const GofJob* j) { return j ? j->dev_bytes + j->rate_bytes : 0; }
GofKind gof_kind(const GofJob* j) { return j ? j->kind : GOF_PLAIN; }
static bool has_color(const GofJob& j, int i) { return !j.color.empty() && j.color[i].t.n_frames > 0; }
static bool has_color_floor(const GofJob& j, int i) { return has_color(j, i) && j.color[i].t.min_psnr_mdb != 0; }
static bool color_pipe(const GofJob& j, int gi) { for (int i : j.groups[gi]) if (has_color(j, i)) return true; return false; }
static bool has_d1(const GofJob& j, int i) { return !j.d1.empty() && j.d1[i].t.n_frames > 0; }
static bool has_d1_floor(const GofJob& j, int i) { return has_d1(j, i) && j.d1[i].t.min_d1_mdb != 0; }
int gof_refused(const GofJob* j, std::string& err) { if (!j || !j->refused) return 0; err = j->err; return j->rc; }
static bool has_target(const GofJob& j, int i) { return !j.targets.empty() && j.targets[i].target_bytes != 0; }
static bool has_floor(const GofJob& j, int i) { return !j.qtargets.empty() && j.qtargets[i].min_psnr_mdb != 0; }
// the displayed size of decoded stream ds - its pictures seen through the conformance window - and its picture count
static int displayed(const DecodeBatch& db, int ds, int* w, int* h) {
  const RbtStreamCfg& c = db.frames[db.stream_first[ds]].cfg; const Sps& sps = db.stream_sps[ds];
  *w = c.w - 2 * sps.conf_win[0] - 2 * sps.conf_win[1]; *h = c.h - 2 * sps.conf_win[2] - 2 * sps.conf_win[3];
  return db.stream_count[ds];
}
// the pipeline that holds an entry of the call, and the entry's position in the pipeline's group
static bool find_entry(const GofJob& j, int entry, int* pipe, size_t* q) {
  for (int g = 0; g < j.ng; g++) for (size_t k = 0; k < j.groups[g].size(); k++) if (j.groups[g][k] == entry) { *pipe = g; *q = k; return true; }
  return false;
}

// What lives only while a job is submitted
struct SubmitPlan {
  const uint8_t* const* in; const rbt_stream_params* p; bool gof_rule;
  std::vector<std::vector<int>> uniq;               // per pipeline: the stream indices that are decoded
  std::vector<std::vector<PoolJob>> pool_jobs;      // per pipeline: the OR-pool launches, recorded by setup_encode and issued behind the decoder's kernels
  // occupancy-aware coding (rbt_stream_params.occupancy_rd): entry i is coded with the occupancy map of the nearest occupancy entry in front of it, if this call pools it
  std::vector<int> occ_of; std::vector<OccSource> occ_src; std::vector<OccJob> occ_jobs;
  std::vector<int> meas_of;                         // quality floors: the occupancy entry whose pooled planes say which samples of entry i are occupied, whether or not it is coded with them
  std::vector<char> feeds_any, consumes; std::vector<int> occ_marks;   // per pipeline: others are coded with its occupancy maps / it is coded with some; where on the feeders' streams the maps are complete
};
// Pipelines: up to three sub-bitstreams get one pipeline (= HIP stream) each. A call with more (several GOFs at once:
// one GOF leaves most of the GPU idle) groups them by video type, so that the slices of all attribute streams parse
// in one launch, all geometry streams in another, ... Host work only.
static int plan_pipelines(GofJob& j, SubmitPlan& s, int depth) {
  const int n = j.n; const rbt_stream_params* p = s.p; const uint8_t* const* in = s.in; const std::vector<size_t>& n_in = j.n_in;
  std::vector<std::vector<int>>& groups = j.groups;
  j.passthrough.resize(n); j.is_pass.assign(n, 0);
  int n_live = 0;
  for (int i = 0; i < n; i++) {
    if (s.gof_rule && p[i].video_type == RBT_VIDEO_OCCUPANCY && p[i].occupancy_precision != 4) { j.is_pass[i] = 1; j.passthrough[i].assign(in[i], in[i] + n_in[i]); }
    else n_live++;
  }
  if (n_live <= rbtk::RBT_AUX_STREAM) { for (int i = 0; i < n; i++) if (!j.is_pass[i]) groups.push_back({i}); }
  else {
    const int types[3] = {RBT_VIDEO_ATTRIBUTE, RBT_VIDEO_GEOMETRY, RBT_VIDEO_OCCUPANCY};
    for (int t = 0; t < 3; t++) { std::vector<int> g; for (int i = 0; i < n; i++) if (!j.is_pass[i] && p[i].video_type == types[t]) g.push_back(i); if (!g.empty()) groups.push_back(g); }
    std::vector<int> rest; for (int i = 0; i < n; i++) if (!j.is_pass[i] && p[i].video_type != types[0] && p[i].video_type != types[1] && p[i].video_type != types[2]) rest.push_back(i);
    if (!rest.empty()) { if (groups.size() < 3) groups.push_back(rest); else groups.back().insert(groups.back().end(), rest.begin(), rest.end()); }
  }
  const int ng = j.ng = (int)groups.size();
  // Streams of a pipeline that are the same input (same buffer: one sub-bitstream re-encoded at several rate points) are decoded once
  j.dec_of.resize(ng); s.uniq.resize(ng);
  for (int g = 0; g < ng; g++) for (int i : groups[g]) {
    std::vector<int>& u = s.uniq[g]; int d = -1;
    for (size_t q = 0; q < u.size(); q++) if (in[u[q]] == in[i] && n_in[u[q]] == n_in[i]) { d = (int)q; break; }
    if (d < 0) { d = (int)u.size(); u.push_back(i); }
    j.dec_of[g].push_back(d);
  }
  auto bytes_of = [&](int g) { size_t t = 0; for (int i : s.uniq[g]) t += n_in[i]; return t; };
  j.db.resize(ng); j.eb.resize(ng); j.chained.assign(ng, 0); j.parse_timed.assign(ng, 1); j.recon_timed.assign(ng, 1);
  j.order.resize(ng); for (int i = 0; i < ng; i++) j.order[i] = i;
  std::stable_sort(j.order.begin(), j.order.end(), [&](int a, int b) { return bytes_of(a) > bytes_of(b); });
  bind_streams(j, depth);
  recon_set_depth(depth);
  j.rate_pipe.assign(ng, 0); j.pipes.resize(ng);
  const bool quality = !j.qtargets.empty();
  for (int g = 0; g < ng; g++) for (int i : groups[g]) j.rate_pipe[g] |= (char)(has_target(j, i) || (quality && p[i].video_type != RBT_VIDEO_OCCUPANCY));
  s.pool_jobs.resize(ng); s.meas_of.assign(n, -1); s.occ_of.assign(n, -1); s.occ_src.resize(n); s.feeds_any.assign(ng, 0); s.consumes.assign(ng, 0);
  int rc = 0;
  for (int i = 0, last = -1; i < n; i++) {
    if (p[i].video_type == RBT_VIDEO_OCCUPANCY) last = (s.gof_rule && !j.is_pass[i] && p[i].occupancy_precision == 4) ? i : -1;
    else if (quality && s.gof_rule) s.meas_of[i] = last;
    if (p[i].video_type != RBT_VIDEO_OCCUPANCY && s.gof_rule && p[i].occupancy_rd && last >= 0) { s.occ_of[i] = last; if (p[i].verify_md5 || p[last].verify_md5) { j.err = "occupancy_rd cannot be combined with verify_md5"; rc = RBT_ERR_PARAM; } }
  }
  // a pipeline with a target is encoded in the wait half, where the occupancy maps of the submission are gone (only calls with more than three streams share pipelines)
  for (int g = 0; g < ng; g++) if (j.rate_pipe[g] && !quality) for (int i : groups[g]) if (s.occ_of[i] >= 0) { j.err = "entry " + std::to_string(i) + ": occupancy_rd on an entry that shares a pipeline with a rate-targeted entry"; rc = RBT_ERR_PARAM; }
  // quality floors keep the maps in the job; the occupancy pipelines themselves are coded at submit, so an occupancy entry cannot share a pipeline with the others
  if (quality) for (int g = 0; g < ng; g++) if (j.rate_pipe[g]) for (int i : groups[g]) if (p[i].video_type == RBT_VIDEO_OCCUPANCY) { j.err = "entry " + std::to_string(i) + ": an occupancy entry shares a pipeline with entries of an unknown video type"; rc = RBT_ERR_PARAM; }
  if (quality) for (int i = 0; i < n; i++) if (j.qtargets[i].region == RBT_QUALITY_OCCUPIED && p[i].video_type != RBT_VIDEO_OCCUPANCY && s.meas_of[i] < 0) {
    j.err = "entry " + std::to_string(i) + ": RBT_QUALITY_OCCUPIED on an entry without an occupancy source (no pooled occupancy entry in front of it)"; rc = RBT_ERR_PARAM; }
  if (rc) j.refused = true;
  return rc;
}

// Decoder batches, longest pipeline first: host parse, arena, uploads (the input's picture hashes - verify_md5 - included: they are checked on the GPU behind the decoder's
// last filter; only the hashes and a mismatch count per decoded stream come back, when the job is collected)
static int build_decoders(GofJob& j, SubmitPlan& s) {
  for (int k = 0; k < j.ng; k++) {
    const int gi = j.order[k]; const std::vector<int>& gs = j.groups[gi]; DecodeBatch& db = j.db[gi]; rbtk::set_stream(job_stream(j, gi));
    std::vector<StreamIn> sins; bool verify = false;
    std::vector<char> verify_ds(s.uniq[gi].size(), 0);   // per decoded stream: some entry it feeds asks for the check
    for (int i : s.uniq[gi]) sins.push_back(StreamIn{s.in[i], j.n_in[i]});
    for (size_t q = 0; q < gs.size(); q++) if (s.p[gs[q]].verify_md5) { verify = true; verify_ds[j.dec_of[gi][q]] = 1; }
    double t0 = now_ms();
    db.want_save = parse_bands() > 1 && k == 0 && j.has_aux && j.ng <= rbtk::RBT_AUX_STREAM && !verify;
    int rc = decode_build(db, sins.data(), (int)sins.size());
    j.st.host_parse_ms += now_ms() - t0;
    if (!rc) rc = decode_upload_lists(db);
    if (!rc && verify) rc = decode_hash_setup(db, verify_ds);
    if (!rc && j.rate_pipe[gi]) {
      std::vector<char> count_ds(s.uniq[gi].size(), 0);    // per decoded stream: some entry it feeds has a target
      for (size_t q = 0; q < gs.size(); q++) if (has_target(j, gs[q])) count_ds[j.dec_of[gi][q]] = 1;
      rc = decode_census_setup(db, count_ds);
    }
    if (rc) { j.err = db.err; return rc; }
  }
  return 0;
}

// A QP per point-cloud frame (include/rbt.h, "a QP per point-cloud frame", rule 1): once the decoders know their pictures, a list must name one QP per pair of them. A
// refusal here is a refusal of the plan: nothing has been enqueued (gof_refused)
static int check_frame_qp(GofJob& j) {
  if (j.frame_qp.empty()) return 0;
  for (int g = 0; g < j.ng; g++) for (size_t q = 0; q < j.groups[g].size(); q++) {
    const int i = j.groups[g][q]; const DecodeBatch& db = j.db[g];
    if (j.frame_qp[i].empty()) continue;
    const int cnt = db.stream_count[j.dec_of[g][q]];
    if (cnt % 2 || (int)j.frame_qp[i].size() != cnt / 2) {
      j.err = "entry " + std::to_string(i) + ": rbt_frame_qp.n_frames is " + std::to_string(j.frame_qp[i].size()) + ", the stream holds " + std::to_string(cnt) + " pictures (n_frames must be pictures / 2)";
      j.refused = true; return RBT_ERR_PARAM;
    }
  }
  return 0;
}
// A QP per CTB (include/rbt.h "a QP per CTB", rule 10): the counts a map came with against the pictures the decoders found - a point-cloud frame per pair of pictures, and the
// CTB grid of the OUTPUT pictures (the input's displayed size, setup_encode) at the entry's log2_ctb. A refusal of the plan, like check_frame_qp's
static int check_qp_maps(GofJob& j) {
  if (j.qp_maps.empty()) return 0;
  for (int g = 0; g < j.ng; g++) for (size_t q = 0; q < j.groups[g].size(); q++) {
    const int i = j.groups[g][q]; const DecodeBatch& db = j.db[g]; const QpMapIn& m = j.qp_maps[i];
    if (m.qp.empty()) continue;
    const std::string who = "entry " + std::to_string(i) + ": ";
    const int ds = j.dec_of[g][q], cnt = db.stream_count[ds];
    if (cnt % 2 || m.n_frames != cnt / 2) {
      j.err = who + "rbt_qp_map.n_frames is " + std::to_string(m.n_frames) + ", the stream holds " + std::to_string(cnt) + " pictures (n_frames must be pictures / 2)";
      j.refused = true; return RBT_ERR_PARAM; }
    int dw, dh; displayed(db, ds, &dw, &dh);
    const int l2 = j.params[i].log2_ctb ? j.params[i].log2_ctb : 5;
    const int wc = (dw + (1 << l2) - 1) >> l2, hc = (dh + (1 << l2) - 1) >> l2;
    if (dw > 0 && dh > 0 && l2 >= 4 && l2 <= 6 && (m.w_ctb != wc || m.h_ctb != hc)) {
      j.err = who + "rbt_qp_map.w_ctb x h_ctb is " + std::to_string(m.w_ctb) + " x " + std::to_string(m.h_ctb) + ", the output pictures (" + std::to_string(dw) + " x " + std::to_string(dh) + ") hold " +
              std::to_string(wc) + " x " + std::to_string(hc) + " CTBs at log2_ctb " + std::to_string(l2);
      j.refused = true; return RBT_ERR_PARAM; }
  }
  return 0;
}
// Floors held patch by patch (include/rbt.h, rule 9): the target's counts and atlas against the pictures the decoders found. A refusal of the plan, like check_frame_qp's
static int check_patch_floors(GofJob& j) {
  if (j.patch.empty()) return 0;
  for (int g = 0; g < j.ng; g++) for (size_t q = 0; q < j.groups[g].size(); q++) {
    const int i = j.groups[g][q]; const DecodeBatch& db = j.db[g]; const PatchFloorIn& t = j.patch[i];
    if (t.n_frames <= 0) continue;
    const std::string who = "entry " + std::to_string(i) + ": ";
    const int ds = j.dec_of[g][q], cnt = db.stream_count[ds];
    if (cnt % 2 || t.n_frames != cnt / 2) {
      j.err = who + "rbt_patch_floor_target.n_frames is " + std::to_string(t.n_frames) + ", the stream holds " + std::to_string(cnt) + " pictures (n_frames must be pictures / 2)";
      j.refused = true; return RBT_ERR_PARAM; }
    int dw, dh; displayed(db, ds, &dw, &dh);
    if (t.atlas_width != dw || t.atlas_height != dh) {
      j.err = who + "the atlas is " + std::to_string(t.atlas_width) + " x " + std::to_string(t.atlas_height) + ", the output pictures are " + std::to_string(dw) + " x " + std::to_string(dh);
      j.refused = true; return RBT_ERR_PARAM; }
  }
  return 0;
}
static int rate_prepare(GofJob& j, int gi);
static int quality_prepare(GofJob& j, SubmitPlan& s, int gi);
static int d1_prepare(GofJob& j, SubmitPlan& s, int gi);
static int color_prepare(GofJob& j, SubmitPlan& s, int gi);
// Encoder batches: the pipelines whose occupancy streams others are coded with first (their pooled planes are what the maps are made of), then the rest
static int build_encoders(GofJob& j, SubmitPlan& s) {
  for (int pass = 0; pass < 2; pass++) for (int k = 0; k < j.ng; k++) {
    const int gi = j.order[k]; const std::vector<int>& gs = j.groups[gi]; EncodeBatch& eb = j.eb[gi]; rbtk::set_stream(job_stream(j, gi));
    bool feeds = false; for (int i : gs) for (int c = 0; c < j.n; c++) feeds |= s.occ_of[c] == i || s.meas_of[c] == i;
    if (feeds != (pass == 0)) continue;
    if (j.rate_pipe[gi]) {      // stays unchained: decoder and census now, encoders in the wait half
      if (int rc = j.qtargets.empty() ? rate_prepare(j, gi) : quality_prepare(j, s, gi)) return rc;
      if (!j.d1.empty()) if (int rc = d1_prepare(j, s, gi)) return rc;
      if (!j.color.empty()) if (int rc = color_prepare(j, s, gi)) return rc;
      continue;
    }
    for (size_t q = 0; q < gs.size(); q++) {
      const int i = gs[q], io = s.occ_of[i];
      if (int rc = setup_encode(j.db[gi], j.dec_of[gi][q], (int)q, s.p[i], eb, j.pooled, j.err, &s.pool_jobs[gi], io >= 0 ? &s.occ_src[io] : nullptr, io, &s.occ_jobs)) return rc;
      if (!j.frame_qp.empty()) eb.desc[q].frame_qp = j.frame_qp[i];
      if (!j.qp_maps.empty() && !j.qp_maps[i].qp.empty()) { eb.desc[q].qp_map = j.qp_maps[i].qp; eb.desc[q].qm_w = j.qp_maps[i].w_ctb; eb.desc[q].qm_h = j.qp_maps[i].h_ctb; }
      const EncStreamDesc& d = eb.desc[q];
      if (feeds && s.p[i].video_type == RBT_VIDEO_OCCUPANCY && d.n_frames > 0) {
        OccSource& os = s.occ_src[i]; os.occ = d.src[0][0]; os.in_step = d.n_frames > 1 ? (size_t)(d.src[0][1] - d.src[0][0]) : 0; os.n = d.n_frames; os.ow = d.w; os.oh = d.h; os.pipeline = gi; }
    }
    int rc = encode_build(eb);
    if (!rc) rc = encode_upload_lists(eb);
    if (rc) { j.err = eb.err; return rc; }
    j.chained[gi] = 1;
  }
  for (const OccJob& oj : s.occ_jobs) s.feeds_any[s.occ_src[oj.source].pipeline] = 1;
  for (int g = 0; g < j.ng; g++) for (const EncStreamDesc& d : j.eb[g].desc) s.consumes[g] |= !d.occ4.empty();
  return 0;
}

// ------------------------------------------------------------------------------------------------ targets: byte budgets (include/rbt.h, "transcoding to a byte budget")
// and PSNR floors ("transcoding to a PSNR floor"). Both are one walk with a direction (rbt_qp_walk.h) over rounds of trial encodes; they differ in how a walk is seeded
// (seed_budgets, seed_floors), in whether a round carries distortion sums, and in how the public result is filled (fill_results).
// the candidates of a round as an encode batch; in a job with floors the entries coded with occupancy_rd get the maps the occupancy pipeline made at submit
// A pass over a subset of an entry's frames: everything the encoder and the distortion stage index by "picture k of the stream" - the source planes, the hints, the flat
// words, the occupancy maps, the shared buffers - is picked through the explicit picture list d.pic, which round_sums_setup reads for the occupancy frame as well
static void desc_subset(EncStreamDesc& d, const FramePass& p) {
  std::vector<int> pic;
  for (int f : p.frames) for (int k = 0; k < d.gop; k++) pic.push_back(f * d.gop + k);
  auto pick = [&](auto& v) { if (v.empty()) return; typename std::remove_reference<decltype(v)>::type o; for (int k : pic) o.push_back(v[(size_t)k]); v.swap(o); };
  for (int c = 0; c < 3; c++) pick(d.src[c]);
  pick(d.hint_pm); pick(d.hint_dm); pick(d.occ4); pick(d.src_flat); pick(d.alias_pix); pick(d.alias_coef);
  d.n_total = d.n_frames; d.n_frames = (int)pic.size(); d.pic.swap(pic);
  d.frame_qp.assign(p.qps.begin(), p.qps.end());
  if (!d.qp_map.empty()) {      // a map per frame of the stream: the maps of the frames the pass carries
    const size_t per = (size_t)d.qm_w * d.qm_h; std::vector<int8_t> m;
    for (int f : p.frames) m.insert(m.end(), d.qp_map.begin() + (ptrdiff_t)(per * (size_t)f), d.qp_map.begin() + (ptrdiff_t)(per * (size_t)(f + 1)));
    d.qp_map.swap(m);
  }
}
static int round_fill_batch(GofJob& j, int gi, const std::vector<RoundCand>& cands, EncodeBatch& eb) {
  for (size_t e = 0; e < cands.size(); e++) {
    rbt_stream_params pp = j.params[j.groups[gi][cands[e].q]]; pp.qp = cands[e].qp;
    if (int rc = setup_encode(j.db[gi], j.dec_of[gi][cands[e].q], (int)e, pp, eb, j.pooled, j.err)) return rc;
  }
  for (size_t e = 0; e < cands.size() && !j.qocc.empty(); e++) {
    const QualityOcc& o = j.qocc[j.groups[gi][cands[e].q]]; EncStreamDesc& d = eb.desc[e];
    if (!o.maps || d.lossless) continue;
    d.occ4.resize(d.n_frames); d.occ4_w = o.w4; d.occ4_h = o.h4;
    for (int k = 0; k < d.n_frames; k++) d.occ4[k] = o.maps + (size_t)((size_t)k * o.n / d.n_frames) * o.w4 * o.h4;
  }
  for (size_t e = 0; e < cands.size(); e++) if (cands[e].pw >= 0) {      // a pass of an entry's patch walks: the trial maps of all its frames (desc_subset picks the pass's)
    const PatchWalks& pw = j.pipes[gi].pwalks[(size_t)cands[e].pw];
    eb.desc[e].qp_map = cands[e].qmap; eb.desc[e].qm_w = pw.wc; eb.desc[e].qm_h = pw.hc;
  }
  for (size_t e = 0; e < cands.size(); e++) if (cands[e].fw >= 0 || cands[e].pw >= 0) desc_subset(eb.desc[e], cands[e].pass);      // last: every table above is per picture of the stream
  return 0;
}
template <class Target> static TargetWalk new_walk(size_t q, int entry, const Target& t) { TargetWalk w; w.q = (int)q; w.entry = entry; w.lo = t.qp_min; w.hi = t.qp_max ? t.qp_max : 51; return w; }
// A budget's walk starts at the estimate: the histograms of the census come back and rate_table turns them and the input's own bytes into E(q). At submit (census false)
// there is no estimate yet: the measurement takes the three QPs of the lowest band, qe = min(hi, lo + 1)
static int seed_budgets(GofJob& j, int gi, RoundPipe& r, bool census) {
  DecodeBatch& db = j.db[gi]; const std::vector<int>& gs = j.groups[gi];
  if (census && db.census.fetch()) { j.err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  for (size_t q = 0; q < gs.size(); q++) if (has_target(j, gs[q])) {
    const rbt_rate_target& t = j.targets[gs[q]];
    TargetWalk w = new_walk(q, gs[q], t); w.budget.T = t.target_bytes; w.start = std::min(w.hi, w.lo + 1);
    if (census) {
      const int ds = j.dec_of[gi][q], first = db.stream_first[ds], cnt = db.stream_count[ds];
      std::vector<uint64_t> bytes(cnt); for (int i = 0; i < cnt; i++) bytes[i] = db.info[first + i].vcl_bytes;
      uint64_t E[52]; rate_table(db.census.hist.data() + (size_t)db.census_first[ds] * RBT_RATE_HIST_WORDS, bytes.data(), cnt, E);
      rate_seed(w, w.budget, E);
    }
    r.walks.push_back(std::move(w));
  }
  return 0;
}
// A floor's walk starts with a probe at the entry's own QP; what the figures of its kind need comes from the target. pinned: the range is the entry's own QP alone
static int entry_bit_depth(const GofJob& j, int gi, size_t q) { const DecodeBatch& db = j.db[gi]; return db.frames[db.stream_first[j.dec_of[gi][q]]].cfg.bit_depth; }
static void walk_goal(TargetWalk& w, const rbt_quality_target& t) { w.kind = WALK_PSNR; w.floor.floor_mdb = t.min_psnr_mdb; w.region = t.region; }
static void walk_goal(TargetWalk& w, const rbt_d1_target& t) { w.kind = WALK_D1; w.floor.floor_mdb = t.min_d1_mdb; w.stat = t.stat; }
static void walk_goal(TargetWalk& w, const rbt_color_target& t) { w.kind = WALK_COLOR; w.floor.floor_mdb = t.min_psnr_mdb; w.stat = t.stat; w.channel = t.channel; }
template <class Target> static TargetWalk floor_walk(const GofJob& j, int gi, size_t q, const Target& t, bool pinned = false) {
  const int i = j.groups[gi][q], qp = j.params[i].qp;
  TargetWalk w = new_walk(q, i, t); walk_goal(w, t); w.bit_depth = entry_bit_depth(j, gi, q); w.d2 = j.d2 && w.kind == WALK_D1;
  if (pinned) w.lo = w.hi = std::min(51, std::max(0, qp));
  floor_seed(w, w.floor, qp);
  return w;
}
// the walks of a pipeline's entries with a floor of the job's kind
static void seed_floors(GofJob& j, int gi, RoundPipe& r, WalkKind kind) {
  const std::vector<int>& gs = j.groups[gi];
  for (size_t q = 0; q < gs.size(); q++) {
    const int i = gs[q];
    if (kind == WALK_D1) { if (has_d1_floor(j, i)) r.walks.push_back(floor_walk(j, gi, q, j.d1[i].t)); }
    else if (kind == WALK_COLOR) { if (has_color_floor(j, i)) r.walks.push_back(floor_walk(j, gi, q, j.color[i].t)); }
    else if (has_floor(j, i)) r.walks.push_back(floor_walk(j, gi, q, j.qtargets[i]));
  }
}
// Floors held frame by frame: every entry of the pipeline gets one walk per point-cloud frame, seeded like the entry's walk - a D1 floor's on the frame's own cloud (one
// result per trial, so the statistic is that result) where the entry has a D1 target, else a PSNR floor's. An entry without a floor is a walk whose range is its own QP
// alone: one pass, the figures reported per frame
static void seed_frame_floors(GofJob& j, int gi, RoundPipe& r) {
  const std::vector<int>& gs = j.groups[gi]; const DecodeBatch& db = j.db[gi];
  for (size_t q = 0; q < gs.size(); q++) {
    const int i = gs[q], nf = db.stream_count[j.dec_of[gi][q]] / 2;
    FrameWalks<TargetWalk> fw; fw.q = (int)q; fw.entry = i; fw.n_enc.assign((size_t)nf, 0);
    const TargetWalk w = has_d1(j, i) ? floor_walk(j, gi, q, j.d1[i].t, !j.d1[i].t.min_d1_mdb) : floor_walk(j, gi, q, j.qtargets[i], !j.qtargets[i].min_psnr_mdb);
    fw.frames.assign((size_t)nf, w);
    r.fwalks.push_back(std::move(fw));
  }
}
// true: settled; false: the walk needs the trial at `need` next (alone: a probe, the round brings nothing else for it)
static bool walk_step(TargetWalk& w, int& need, int& dir, bool& alone) {
  alone = false;
  if (w.kind == WALK_BUDGET) return qp_walk_step(w, rate_fits(w, w.budget), need, dir);
  auto figure = [&w](const TargetTried& t) { return w.d2 ? d1_figure(t.d2, w.stat) : w.kind == WALK_D1 ? d1_figure(t.d1, w.stat) : w.kind == WALK_COLOR ? color_figure(t.color, w.stat, w.channel) : quality_region_psnr(t.sums, w.region, w.bit_depth); };
  auto meets = [&w](const TargetTried& t) {
    return w.d2 ? d1_meets(t.d2, w.stat, w.floor.floor_mdb) : w.kind == WALK_D1 ? d1_meets(t.d1, w.stat, w.floor.floor_mdb) : w.kind == WALK_COLOR ? color_meets(t.color, w.stat, w.channel, w.floor.floor_mdb) : quality_meets(t.sums, w.region, w.floor.floor_mdb, w.bit_depth);
  };
  alone = !floor_probe(w, w.floor, figure);
  if (alone) { need = w.floor.q0; dir = 0; return false; }
  return qp_walk_step(w, floor_holds(w, meets), need, dir);
}
// ------------------------------------------------------------------------------------------------ floors held patch by patch (include/rbt.h, "PSNR floors held patch by patch")
static bool has_patch_floor(const GofJob& j, int i) { return !j.patch.empty() && j.patch[i].n_frames > 0; }
// In the wait half, once the pipeline's decoder has been collected: per entry with a target the walks of its frames - lo, hi and q0 as the PSNR floor has them, a range of
// q0 alone where there is no floor at all (rule 8) -, R_k of every patch in CTB units and its displayed samples, and the rectangles on the device for all rounds
static int seed_patch_walks(GofJob& j, int gi, RoundPipe& r) {
  const std::vector<int>& gs = j.groups[gi]; DecodeBatch& db = j.db[gi];
  for (size_t q = 0; q < gs.size(); q++) if (has_patch_floor(j, gs[q])) {
    const int i = gs[q]; const PatchFloorIn& in = j.patch[i];
    PatchWalks pw; pw.q = (int)q; pw.entry = i; pw.l2 = j.params[i].log2_ctb ? j.params[i].log2_ctb : 5; pw.bit_depth = entry_bit_depth(j, gi, q);
    displayed(db, j.dec_of[gi][q], &pw.W, &pw.H);
    pw.wc = (pw.W + (1 << pw.l2) - 1) >> pw.l2; pw.hc = (pw.H + (1 << pw.l2) - 1) >> pw.l2;
    bool any_floor = in.floor_mdb != 0; for (const std::vector<int32_t>& fl : in.floors) for (int32_t v : fl) any_floor |= v != 0;
    const int qp = std::min(51, std::max(0, j.params[i].qp)), lo = any_floor ? in.qp_min : qp, hi = any_floor ? (in.qp_max ? in.qp_max : 51) : qp;
    pw.frames.resize((size_t)in.n_frames); size_t n_rects = 0;
    for (int f = 0; f < in.n_frames; f++) {
      PatchFrame& F = pw.frames[(size_t)f]; const std::vector<rbt_patch>& ps = in.patches[(size_t)f];
      patch_walk_seed(F.w, qp, lo, hi, in.max_trials, in.floors[(size_t)f]);
      F.rects.resize(4 * ps.size()); F.samples.resize(ps.size()); F.rect_off = n_rects; n_rects += ps.size();
      for (size_t k = 0; k < ps.size(); k++) {
        patch_region(pw.W, pw.H, in.occupancy_resolution, ps[k].u0, ps[k].v0, ps[k].size_u0, ps[k].size_v0, pw.l2, &F.rects[4 * k]);
        F.samples[k] = patch_region_samples(&F.rects[4 * k], pw.W, pw.H, pw.l2);
      }
    }
    pw.d_rects = (int32_t*)rbtk::dev_alloc(std::max<size_t>(1, n_rects) * 16);
    if (!pw.d_rects) { j.err = "device allocation failed"; return RBT_ERR_NOMEM; }
    j.pooled.push_back(pw.d_rects);
    for (const PatchFrame& F : pw.frames) if (!F.rects.empty() && rbtk::h2d(pw.d_rects + 4 * F.rect_off, F.rects.data(), F.rects.size() * 4)) { j.err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
    r.pwalks.push_back(std::move(pw));
  }
  return 0;
}
// the trial maps of an entry's frames: rule 4 for every frame that has not settled (a settled frame is in no pass: its part stays at q0)
static int patch_trial_maps(GofJob& j, const PatchWalks& pw, std::vector<int8_t>& out) {
  const PatchFloorIn& in = j.patch[pw.entry]; const size_t per = (size_t)pw.wc * pw.hc;
  rbt_atlas_params a; memset(&a, 0, sizeof(a)); a.width = pw.W; a.height = pw.H; a.occupancy_resolution = in.occupancy_resolution;      // (what qp_map_from_patches reads)
  out.assign(per * pw.frames.size(), 0);
  for (size_t f = 0; f < pw.frames.size(); f++) {
    const PatchWalk& w = pw.frames[f].w;
    if (w.settled) { std::fill(out.begin() + (ptrdiff_t)(per * f), out.begin() + (ptrdiff_t)(per * (f + 1)), (int8_t)w.q0); continue; }
    std::vector<int8_t> q(w.q.begin(), w.q.end());
    if (int rc = qp_map_from_patches(j.err, &a, in.patches[f].data(), (int)in.patches[f].size(), q.data(), in.background_qp < 0 ? w.q0 : in.background_qp, pw.l2, out.data() + per * f, pw.wc, pw.hc)) return rc;
  }
  return 0;
}
// The round to run next, in group order: what every unsettled walk asks for (qp_round) and, in the first round, the pipeline's entries without a target at their own QP
static void name_round(GofJob& j, int gi, RoundPipe& r, bool first) {
  const std::vector<int>& gs = j.groups[gi]; std::vector<int> qps; size_t k = 0;
  r.cands.clear();
  if (!j.patch.empty()) {      // floors held patch by patch: one pass per entry with a target over its unsettled frames, each with its trial map (rule 6)
    size_t p = 0;
    for (size_t q = 0; q < gs.size(); q++) {
      if (p == r.pwalks.size() || r.pwalks[p].q != (int)q) { if (first) r.cands.push_back(RoundCand{(int)q, j.params[gs[q]].qp, -1}); continue; }
      PatchWalks& pw = r.pwalks[p];
      RoundCand c{pw.q, j.params[pw.entry].qp, -1}; c.pw = (int)p;
      for (size_t f = 0; f < pw.frames.size(); f++) if (!pw.frames[f].w.settled) c.pass.frames.push_back((int)f);
      if (!c.pass.frames.empty() && !patch_trial_maps(j, pw, c.qmap)) r.cands.push_back(std::move(c));
      p++;
    }
    return;
  }
  if (j.per_frame) {      // every entry of the pipeline walks frame by frame: its passes (rbt_frame_walk.h), in group order
    std::vector<FramePass> passes;
    for (size_t e = 0; e < r.fwalks.size(); e++) {
      FrameWalks<TargetWalk>& fw = r.fwalks[e];
      frame_round(fw, [](TargetWalk& w, int& need, int& dir, bool& alone) { return walk_step(w, need, dir, alone); }, passes);
      for (FramePass& p : passes) { RoundCand c{fw.q, j.params[fw.entry].qp, -1}; c.fw = (int)e; c.pass = std::move(p); r.cands.push_back(std::move(c)); }
    }
    return;
  }
  for (size_t q = 0; q < gs.size(); q++) {
    if (k == r.walks.size() || r.walks[k].q != (int)q) { if (first) r.cands.push_back(RoundCand{(int)q, j.params[gs[q]].qp, -1}); continue; }
    TargetWalk& w = r.walks[k]; int need = 0, dir = 0; bool alone = false;
    if (!w.settled && !walk_step(w, need, dir, alone)) { qp_round(w, need, dir, alone, qps); for (int qp : qps) r.cands.push_back(RoundCand{w.q, qp, (int)k}); }
    k++;
  }
}
// at submit: what the first round of trial encodes will take (rbt_job_memory), measured on the layout without allocating
static int measure_round(GofJob& j, int gi, const std::vector<RoundCand>& cands) {
  DecodeBatch& db = j.db[gi];
  const std::vector<char> taken = db.alias_taken;
  EncodeBatch eb; int rc = round_fill_batch(j, gi, cands, eb);
  if (!rc && (rc = encode_plan(eb)) != 0) j.err = eb.err;
  db.alias_taken = taken;
  if (!rc) j.rate_bytes += eb.arena_size;
  return rc;
}
// a pipeline with a budget at submit: the estimate is not known yet, the arenas do not depend on it but for the slice buffers' QP bands
static int rate_prepare(GofJob& j, int gi) {
  for (int i : j.groups[gi]) if (j.params[i].video_type == RBT_VIDEO_OCCUPANCY) return 0;      // (its pooled planes would be allocated: left uncounted)
  RoundPipe r; seed_budgets(j, gi, r, false); name_round(j, gi, r, true);
  return measure_round(j, gi, r.cands);
}
// Rounds. A round of a pipeline is one encode batch of candidates on the pipeline's stream: launch_round builds and enqueues it, finish_round waits for it, packs the
// streams, lets the walks look at what came back and names the next round. In a job with floors the round carries, behind its last filter, the sums of every candidate
// picture against the decoded picture it was coded from - EncStreamDesc::src, which no encoder writes to (arena sharing hands out the decoded pictures' dead buffers only)
static int round_sums_setup(GofJob& j, int gi) {
  RoundPipe& r = j.pipes[gi]; EncodeBatch& eb = *r.eb;
  r.sse.reset(new SseSet()); r.sse->ext = eb.d_sums;
  if (rbtk::dev_memset(eb.d_sums, 0, eb.n_sums * 8)) { j.err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  for (size_t e = 0; e < r.cands.size(); e++) {
    const EncStreamDesc& d = eb.desc[e]; const QualityOcc& o = j.qocc[j.groups[gi][r.cands[e].q]]; const int st = d.src_stride ? d.src_stride : d.w;
    for (int k = 0; k < d.n_frames; k++) {
      const RbtFrame& f = eb.frames[(size_t)eb.stream_first[e] + k];
      RbtSsePic P; memset(&P, 0, sizeof(P));
      for (int c = 0; c < 3; c++) { const int sh = c ? 1 : 0; P.a[c] = d.src[c][k] + (size_t)(d.src_y0 >> sh) * (size_t)(st >> sh) + (d.src_x0 >> sh); P.b[c] = f.out[c]; }
      P.w = d.w; P.h = d.h; P.a_stride = st; P.b_stride = f.cfg.w;
      const size_t pk = d.pic.empty() ? (size_t)k : (size_t)d.pic[k], pn = d.pic.empty() ? (size_t)d.n_frames : (size_t)d.n_total;      // picture pk of the stream's pn
      if (o.occ) { P.occ = o.occ + o.in_step * (pk * o.n / pn); P.ow = o.ow; P.scale = d.w / o.ow; }
      r.sse->add(P);
    }
  }
  if (int rc = r.sse->upload()) { j.err = rc == RBT_ERR_NOMEM ? "device allocation failed" : "device transfer failed"; return rc; }
  // floors held patch by patch: the luma of the same pairs CTB by CTB into the batch's arena, and per frame of a pass the folds of its rectangles behind the words above
  if (j.patch.empty() || j.patch_clouds()) return 0;
  r.ctbsse.reset(new CtbSseSet()); CtbSseSet& cs = *r.ctbsse;
  size_t pic = 0, ctb_at = 0, fold_at = r.sse->pics.size() * RBT_SSE_WORDS;
  for (size_t e = 0; e < r.cands.size(); e++) {
    const EncStreamDesc& d = eb.desc[e]; const RoundCand& c = r.cands[e];
    if (c.pw < 0) { pic += (size_t)d.n_frames; continue; }
    const PatchWalks& pw = r.pwalks[(size_t)c.pw]; const size_t per = (size_t)pw.wc * pw.hc * RBT_CTBSSE_WORDS;
    if (d.gop != 2 || d.w != pw.W || d.h != pw.H) { j.err = "internal: a patch target does not fit its stream"; return RBT_ERR_PARAM; }
    for (size_t i = 0; i < c.pass.frames.size(); i++) {
      const PatchFrame& F = pw.frames[(size_t)c.pass.frames[i]];
      RbtFoldJob J; memset(&J, 0, sizeof(J));
      for (int k = 0; k < d.gop; k++, pic++, ctb_at += per) {
        const RbtSsePic& S = r.sse->pics[pic]; RbtCtbSsePic P; memset(&P, 0, sizeof(P));
        P.a = S.a[0]; P.b = S.b[0]; P.occ = S.occ; P.w = S.w; P.h = S.h; P.a_stride = S.a_stride; P.b_stride = S.b_stride; P.ow = S.ow; P.scale = S.scale;
        P.log2_ctb = pw.l2; P.w_ctb = pw.wc; P.h_ctb = pw.hc; P.out = eb.d_ctb_words + ctb_at;
        if (k < 2) J.ctb[k] = P.out;
        cs.pics.push_back(P);
      }
      J.rects = pw.d_rects + 4 * F.rect_off; J.n_rects = (int)F.samples.size(); J.w_ctb = pw.wc; J.h_ctb = pw.hc; J.out = eb.d_sums + fold_at;
      fold_at += ((size_t)J.n_rects + 2) * RBT_CTBSSE_WORDS;
      cs.jobs.push_back(J); cs.max_rects = std::max(cs.max_rects, J.n_rects); cs.max_ctbs = std::max(cs.max_ctbs, pw.wc * pw.hc);
    }
  }
  if (cs.pics.empty()) { r.ctbsse.reset(); return 0; }
  if (fold_at > eb.n_sums || ctb_at > eb.n_ctb_words) { j.err = "internal: the sums per patch do not fit the round's arena"; return RBT_ERR_PARAM; }
  if (int rc = cs.upload()) { j.err = rc == RBT_ERR_NOMEM ? "device allocation failed" : "device transfer failed"; return rc; }
  return 0;
}
static int launch_round(GofJob& j, int gi) {
  RoundPipe& r = j.pipes[gi]; const bool sums = !j.qtargets.empty();
  if (r.cands.empty()) { r.done = true; return 0; }
  rbtk::set_stream(job_stream(j, gi));
  r.eb.reset(new EncodeBatch()); EncodeBatch& eb = *r.eb;
  int rc = round_fill_batch(j, gi, r.cands, eb);
  if (sums) for (const EncStreamDesc& d : eb.desc) eb.n_sums += (size_t)d.n_frames * RBT_SSE_WORDS;
  for (size_t e = 0; e < r.cands.size() && !rc && !j.patch_clouds(); e++) if (r.cands[e].pw >= 0) {      // floors held patch by patch: the folds behind the words per picture, the words per CTB
    const PatchWalks& pw = r.pwalks[(size_t)r.cands[e].pw];
    for (int f : r.cands[e].pass.frames) eb.n_sums += (pw.frames[(size_t)f].samples.size() + 2) * RBT_CTBSSE_WORDS;
    eb.n_ctb_words += (size_t)eb.desc[e].n_frames * pw.wc * pw.hc * RBT_CTBSSE_WORDS;
  }
  if (!rc && (rc = encode_build(eb)) != 0) j.err = eb.err;
  if (!rc && sums) rc = round_sums_setup(j, gi);
  if (!rc && (rc = encode_upload_lists(eb)) != 0) j.err = eb.err;
  if (rc) return rc;
  encode_launch_intra(eb); encode_launch_entropy_intra(eb); encode_launch_inter(eb);
  if (!eb.hash.empty()) eb.hash.launch();
  if (sums) r.sse->launch();
  if (r.ctbsse) r.ctbsse->launch();
  encode_launch_entropy_rest(eb);
  return 0;
}
// ------------------------------------------------------------------------------------------------ cloud targets: what D1 floors and colour floors share
// The refusals of rules 1 and 2 that the two kinds have in common, nullptr = the target fits. They come in two parts, which each kind calls where its own checks leave
// room for them: a target against the stream it sits on (its displayed size dw x dh, its cnt pictures) ...
template <class Target> static const char* cloud_fits_stream(const Target& t, int dw, int dh, int cnt) {
  if (dw != t.atlas.width || dh != t.atlas.height) return "the displayed picture size is not atlas.width x atlas.height";
  if (cnt != t.atlas.map_count * t.n_frames) return "the picture count is not atlas.map_count x n_frames";
  return nullptr;
}
// ... and against its occupancy source, entry `io` with the pooled planes `os`, whose decoded input is located on the way (E.in_*: what the reference clouds of frames
// without a handle are made of)
template <class Target> static const char* cloud_fits_occupancy(const GofJob& j, const OccSource& os, int io, const Target& t, int dw, int dh, CloudEntry& E) {
  if (os.n != t.n_frames) return "the occupancy source does not hold n_frames pictures";
  if (os.ow * t.atlas.occupancy_precision != dw || os.oh * t.atlas.occupancy_precision != dh) return "atlas.occupancy_precision is not width / (output occupancy width)";
  size_t oq = 0;
  if (!find_entry(j, io, &E.in_pipe, &oq) || j.db[E.in_pipe].frames.empty()) return "the occupancy source was not decoded";
  E.in_ds = j.dec_of[E.in_pipe][oq];
  displayed(j.db[E.in_pipe], E.in_ds, &E.in_ow, &E.in_oh);
  if (E.in_ow <= 0 || E.in_oh <= 0 || dw % E.in_ow || dh % E.in_oh || dw / E.in_ow != dh / E.in_oh) return "the input occupancy size does not divide the atlas by one whole factor";
  return nullptr;
}
// the device time of one cloud's work, between the events of T_CENSUS on the pipeline's stream (no census runs in a job with floors)
static int cloud_timed(GofJob& j, CloudEntry& E, int rc) {
  rbtk::timer_end(T_CENSUS);
  if (rc) return rc;
  if (rbtk::dev_sync()) { j.err = "kernel execution failed"; return RBT_ERR_NO_DEVICE; }
  E.cloud_ms += rbtk::timer_ms(T_CENSUS);
  return 0;
}
// ------------------------------------------------------------------------------------------------ D1 floors (include/rbt.h, "transcoding geometry to a D1 floor")
// At submit, behind quality_prepare (which has found the pooled planes of every entry's occupancy source): rules 1 and 2 for every entry of the pipeline with a target,
// where the decoded input of the occupancy source lies, and what the clouds will take (rbt_job_memory)
static int d1_prepare(GofJob& j, SubmitPlan& s, int gi) {
  DecodeBatch& db = j.db[gi]; const std::vector<int>& gs = j.groups[gi];
  if (db.frames.empty()) return 0;
  auto refuse = [&](int i, const std::string& why) { j.err = "entry " + std::to_string(i) + ": " + why; j.refused = true; return RBT_ERR_PARAM; };
  for (size_t q = 0; q < gs.size(); q++) if (has_d1(j, gs[q])) {
    const int i = gs[q], io = s.meas_of[i];
    D1Entry& E = j.d1[i]; const rbt_atlas_params& a = E.t.atlas;
    if (io < 0 || s.occ_src[io].n <= 0) return refuse(i, "a D1 target needs an occupancy source: a pooled occupancy entry (occupancy_precision 4) in front of it");
    int dw, dh; const int cnt = displayed(db, j.dec_of[gi][q], &dw, &dh);
    if (const char* why = cloud_fits_stream(E.t, dw, dh, cnt)) return refuse(i, why);
    if (j.per_frame && a.map_count != 2) return refuse(i, "floors held frame by frame need atlas.map_count 2: a point-cloud frame is the two pictures that are coded as a pair");
    if (j.patch_d1 && a.map_count != 2) return refuse(i, "floors held patch by patch need atlas.map_count 2: a point-cloud frame is the two pictures that are coded as a pair");
    if (const char* why = cloud_fits_occupancy(j, s.occ_src[io], io, E.t, dw, dh, E)) return refuse(i, why);
    // memory: per frame the frame's maps (twice while a reference cloud is made), per frame without a handle a volume, one more for the trial being scored; the packed
    // planes of one trial and of the decoded input
    size_t bytes = PCLOUD_VOL_BYTES + 2 * (size_t)cnt * (size_t)dw * dh * 2 + (size_t)E.t.n_frames * (size_t)E.in_ow * E.in_oh * 2;
    for (int f = 0; f < E.t.n_frames; f++) bytes += 2 * mapframe_bytes(&a, (int)E.patches[f].size()) + (E.ref[f] ? 0 : PCLOUD_VOL_BYTES);
    j.rate_bytes += bytes;
  }
  return 0;
}
// the luma planes of pictures as packed planes, one launch (csrc/rbt_cloudmaps.h); the descriptors' host staging stays alive in `keep`
struct GatherSet {
  std::vector<RbtGatherPic> pics; void* d = nullptr; int max_chunks = 0;
  ~GatherSet() { rbtk::dev_free(d); }
  void add(const uint16_t* src, int stride, int w, int h, uint16_t* dst) { pics.push_back(RbtGatherPic{src, dst, w, h, stride, 0}); max_chunks = std::max(max_chunks, RBT_GM_PIC_CHUNKS(w, h)); }
  int launch(std::string& err) {
    d = rbtk::dev_alloc(pics.size() * sizeof(RbtGatherPic));
    if (!d) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
    if (rbtk::h2d(d, pics.data(), pics.size() * sizeof(RbtGatherPic))) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
    rbtk::launch_gather_luma((const RbtGatherPic*)d, (int)pics.size(), max_chunks);
    return 0;
  }
  // the luma of picture k of decoded stream ds, seen through its conformance window (w x h: displayed())
  void add_decoded(const DecodeBatch& db, int ds, int k, int w, int h, uint16_t* dst) {
    const int first = db.stream_first[ds]; const RbtStreamCfg& c = db.frames[first].cfg; const Sps& sps = db.stream_sps[ds];
    add((const uint16_t*)db.frames[first + k].out[0] + (size_t)(2 * sps.conf_win[2]) * c.w + 2 * sps.conf_win[0], c.w, w, h, dst);
  }
  // the luma of the reconstructions of stream e of an encode batch - the displayed window starts at the picture's origin - back to back
  void add_coded(const EncodeBatch& eb, size_t e, int w, int h, uint16_t* dst) {
    for (int k = 0; k < eb.desc[e].n_frames; k++) { const RbtFrame& f = eb.frames[(size_t)eb.stream_first[e] + k]; add(f.out[0], f.cfg.w, w, h, dst + (size_t)w * h * (size_t)k); }
  }
};
struct DevPlanes { uint16_t* p = nullptr; ~DevPlanes() { rbtk::dev_free(p); } bool alloc(size_t samples) { p = (uint16_t*)rbtk::dev_alloc(samples * 2); return p != nullptr; } };
// In the wait half, once the pipeline's decoder has been collected (the occupancy pipelines were collected before it, gof_wait): per entry with a target and per frame
// what does not depend on the QP - the maps of the frame from the pooled occupancy plane (MapFrame) and, for a frame without a handle, the reference cloud from the decoded
// input. On the pipeline's stream; waits are on that stream.
static int d1_setup(GofJob& j, int gi) {
  DecodeBatch& db = j.db[gi]; const std::vector<int>& gs = j.groups[gi]; PCloudCache& cache = *j.cloud_cache;
  rbtk::set_stream(job_stream(j, gi));
  for (size_t q = 0; q < gs.size(); q++) if (has_d1(j, gs[q])) {
    const int i = gs[q], ds = j.dec_of[gi][q], first = db.stream_first[ds], nf = j.d1[i].t.n_frames;
    D1Entry& E = j.d1[i]; const rbt_atlas_params& a = E.t.atlas; const QualityOcc& o = j.qocc[i]; const int W = a.width, H = a.height, mc = a.map_count;
    if (!o.occ) { j.err = "internal: no occupancy source"; return RBT_ERR_PARAM; }
    E.frames.assign(nf, nullptr); E.own_ref.assign(nf, nullptr);
    for (int f = 0; f < nf; f++) if (int rc = mapframe_new(j.err, &a, E.patches[f].data(), (int)E.patches[f].size(), o.occ + o.in_step * (size_t)f, &E.frames[f])) return rc;
    bool any = false; for (int f = 0; f < nf; f++) any |= E.ref[f] == nullptr;
    if (!any) continue;
    // the decoded input seen through its conformance windows, packed: occupancy luma and geometry luma of the frames without a handle
    const size_t ys = (size_t)W * H, os = (size_t)E.in_ow * E.in_oh; const int bd = db.frames[first].cfg.bit_depth;
    DevPlanes geo, occ; GatherSet gs_in;
    if (!geo.alloc(ys * (size_t)mc * nf) || !occ.alloc(os * (size_t)nf)) { j.err = "device allocation failed"; return RBT_ERR_NOMEM; }
    rbtk::timer_begin(T_CENSUS);
    for (int f = 0; f < nf; f++) if (!E.ref[f]) {
      gs_in.add_decoded(j.db[E.in_pipe], E.in_ds, f, E.in_ow, E.in_oh, occ.p + os * (size_t)f);
      for (int m = 0; m < mc; m++) gs_in.add_decoded(db, ds, mc * f + m, W, H, geo.p + ys * (size_t)(mc * f + m));
    }
    int rc = gs_in.launch(j.err);
    rbt_atlas_params ain = a; ain.occupancy_precision = W / E.in_ow;
    for (int f = 0; f < nf && !rc; f++) if (!E.ref[f]) {
      MapFrame* F = nullptr;
      rc = mapframe_new(j.err, &ain, E.patches[f].data(), (int)E.patches[f].size(), occ.p + os * (size_t)f, &F);
      if (!rc) rc = mapframe_cloud(j.err, cache, F, geo.p + ys * (size_t)(mc * f), mc > 1 ? geo.p + ys * (size_t)(mc * f + 1) : nullptr, bd, &E.own_ref[f], nullptr);
      if (!rc && j.d2) { const NormalsIn& N = j.normals[(size_t)i]; rc = pcloud_estimate_normals(j.err, E.own_ref[f], N.k, N.orient, N.vp, nullptr, nullptr); }      // D2: once per job, kept with the cloud
      if (rbtk::dev_sync() && !rc) { j.err = "kernel execution failed"; rc = RBT_ERR_NO_DEVICE; }      // F's buffers are idle before they go
      mapframe_delete(F);
    }
    if (int bad = cloud_timed(j, E, rc)) return bad;
  }
  return 0;
}
// what d1_setup made, released on every way out of run_rounds (the clouds' volumes go back to the context's cache)
struct D1Live {
  GofJob& j; int gi;
  ~D1Live() {
    if (j.d1.empty()) return;
    rbtk::set_stream(job_stream(j, gi)); rbtk::dev_sync();
    for (int i : j.groups[gi]) { D1Entry& E = j.d1[i];
      for (MapFrame* F : E.frames) mapframe_delete(F);
      for (PCloud* c : E.own_ref) pcloud_release(*j.cloud_cache, c);
      E.frames.clear(); E.own_ref.clear(); }
  }
};
// The clouds of candidate e of the round in flight - stream `q` of the pipeline's group at one QP - against the entry's references: the luma of the encoder's
// reconstructions (the displayed window starts at the picture's origin: make_param_sets pads at the right and at the bottom) is gathered into packed planes by one launch,
// then frame after frame: cloud, index, search, release (one recycled volume). The round's encode has been waited for (encode_finish).
// per_patch (D1 floors held patch by patch): per frame of the pass the figures of its patches too - rbt_score_patches in place of the D1 part of rbt_score, out unchanged
// A job with D2 floors: g2->whole receives the frames' D2 - rbt_score with RBT_SCORE_D2, whose D1 part still fills out - or, patch by patch, rbt_score_patches_d2's
// whole with g2->patches its figures per patch (out then stays zero: the kind reports no D1)
struct CloudScoresD2 { std::vector<rbt_d2_result> whole; std::vector<std::vector<rbt_patch_d2>> patches; };
static int d1_score(GofJob& j, int gi, int q, const EncodeBatch& eb, size_t e, std::vector<rbt_d1_result>& out, std::vector<std::vector<rbt_patch_d1>>* per_patch = nullptr, CloudScoresD2* g2 = nullptr) {
  const int i = j.groups[gi][q]; D1Entry& E = j.d1[i]; const rbt_atlas_params& a = E.t.atlas; PCloudCache& cache = *j.cloud_cache;
  const EncStreamDesc& d = eb.desc[e]; const int W = a.width, H = a.height, mc = a.map_count, nf = E.t.n_frames, peak = E.t.peak ? E.t.peak : 1023;
  const size_t ys = (size_t)W * H;
  // a pass over a subset of the frames (desc_subset) codes np of the nf frames: coded pictures mc * i .. of the pass are stream pictures d.pic[mc * i] .., frame d.pic[mc * i] / mc -
  // the gather descriptors go by the coded picture, the maps, the patch lists and the references by the frame; out is in pass order
  const int np = d.n_frames / mc;
  if (d.w != W || d.h != H || d.n_frames != mc * np || (d.pic.empty() ? np != nf : d.n_total != mc * nf) || (int)E.frames.size() != nf) { j.err = "internal: a D1 target does not fit its stream"; return RBT_ERR_PARAM; }
  DevPlanes geo; GatherSet gs;
  if (!geo.alloc(ys * (size_t)d.n_frames)) { j.err = "device allocation failed"; return RBT_ERR_NOMEM; }
  out.assign(np, rbt_d1_result());
  if (per_patch) per_patch->assign((size_t)np, {});
  if (j.d2 && !g2) { j.err = "internal: a D2 job scored without its figure"; return RBT_ERR_PARAM; }
  if (g2) { g2->whole.assign((size_t)np, rbt_d2_result()); g2->patches.assign((size_t)np, {}); }
  rbtk::timer_begin(T_CENSUS);
  gs.add_coded(eb, e, W, H, geo.p);
  int rc = gs.launch(j.err);
  for (int i = 0; i < np && !rc; i++) {
    const int f = d.pic.empty() ? i : d.pic[(size_t)(mc * i)] / mc; PCloud* c = nullptr;
    rc = mapframe_cloud(j.err, cache, E.frames[f], geo.p + ys * (size_t)(mc * i), mc > 1 ? geo.p + ys * (size_t)(mc * i + 1) : nullptr, d.bd, &c, nullptr);
    const PCloud* A = E.ref[f] ? E.ref[f] : E.own_ref[f];
    if (!rc && g2 && per_patch) {
      std::vector<rbt_patch_d2>& pp = g2->patches[(size_t)i]; pp.resize(E.patches[f].size());
      rc = pcloud_score_patches_d2(j.err, A, c, peak, (int)pp.size(), pp.data(), &g2->whole[(size_t)i], nullptr);
    } else if (!rc && g2) {
      rbt_frame_score s; rc = pcloud_score(j.err, A, c, peak, RBT_SCORE_D2, &s);
      out[i] = s.d1; g2->whole[(size_t)i] = s.d2;
    } else if (!rc && per_patch) {
      std::vector<rbt_patch_d1>& pp = (*per_patch)[(size_t)i]; pp.resize(E.patches[f].size());
      rc = pcloud_score_patches(j.err, A, c, peak, (int)pp.size(), pp.data(), &out[i], nullptr);
    } else if (!rc) rc = pcloud_d1(j.err, A, c, peak, &out[i]);
    pcloud_release(cache, c);
  }
  return cloud_timed(j, E, rc);
}
// ------------------------------------------------------------------------------------------------ colour floors (include/rbt.h, "transcoding attributes to a colour PSNR floor")
// At submit, behind quality_prepare: rules 1 and 2 for every entry of the pipeline with a target - its occupancy source, its geometry source, their shapes -, where the
// decoded input of the occupancy source lies, and what the clouds will take (rbt_job_memory)
static int color_prepare(GofJob& j, SubmitPlan& s, int gi) {
  DecodeBatch& db = j.db[gi]; const std::vector<int>& gs = j.groups[gi];
  if (db.frames.empty()) return 0;
  auto refuse = [&](int i, const std::string& why) { j.err = "entry " + std::to_string(i) + ": " + why; j.refused = true; return RBT_ERR_PARAM; };
  for (size_t q = 0; q < gs.size(); q++) if (has_color(j, gs[q])) {
    const int i = gs[q], io = s.meas_of[i], ds = j.dec_of[gi][q];
    ColorEntry& E = j.color[i]; const rbt_atlas_params& a = E.t.atlas;
    if (io < 0 || s.occ_src[io].n <= 0) return refuse(i, "a colour target needs an occupancy source: a pooled occupancy entry (occupancy_precision 4) in front of it");
    for (int g = i - 1; g > io && E.geo < 0; g--) if (s.p[g].video_type == RBT_VIDEO_GEOMETRY && s.meas_of[g] == io) E.geo = g;
    if (E.geo < 0) return refuse(i, "a colour target needs a geometry source: a geometry entry in front of it with the same occupancy source");
    int dw, dh; const int cnt = displayed(db, ds, &dw, &dh), bd = db.frames[db.stream_first[ds]].cfg.bit_depth;
    if (const char* why = cloud_fits_stream(E.t, dw, dh, cnt)) return refuse(i, why);
    if (bd != 8 && bd != 10) return refuse(i, "the attribute bit depth is neither 8 nor 10");
    int gp = -1; size_t gq = 0;
    if (!find_entry(j, E.geo, &gp, &gq) || gp == gi || j.db[gp].frames.empty()) return refuse(i, "the geometry source was not decoded in a pipeline of its own");
    int gw, gh; const int gcnt = displayed(j.db[gp], j.dec_of[gp][gq], &gw, &gh);
    if (gw != dw || gh != dh || gcnt != cnt) return refuse(i, "the geometry source's displayed size or picture count is not the attribute entry's");
    if (const char* why = cloud_fits_occupancy(j, s.occ_src[io], io, E.t, dw, dh, E)) return refuse(i, why);
    // memory: per frame a volume, the frame's buffers and 8 bytes per point of distances - twice where the reference is the job's own, with the packed
    // planes of the decoded input -, the packed geometry planes; per trial the packed attribute planes, their 4:4:4 planes and the two volumes of the transfer
    const size_t ys = (size_t)dw * dh, vol = (size_t)1 << 27;
    size_t bytes = (size_t)cnt * ys * 2 + (size_t)cnt * ys * 3 + (size_t)cnt * ys * 6 + (a.geometry_smoothing && E.t.attr_transfer ? 2 * vol : 0);
    for (int f = 0; f < E.t.n_frames; f++) {
      const size_t one = PCLOUD_VOL_BYTES + colorframe_bytes(&a, (int)E.patches[f].size()) + 8 * ys * (size_t)a.map_count;
      bytes += one + (E.ref[f] ? 0 : one + (size_t)a.map_count * ys * 2 + (size_t)E.in_ow * E.in_oh * 2);
    }
    j.rate_bytes += bytes;
  }
  return 0;
}
// The geometry half, behind the only encode of a geometry entry that is some colour target's geometry source (finish_round; candidate e of the round in flight): the luma
// of its reconstruction gathered into packed planes, which stay until the attribute rounds end, and per frame the ColorFrame - maps from the pooled occupancy plane, count,
// scan, emit, smoothing with the moved flags, index. On the geometry pipeline's stream, waited for before the round's arena goes.
static int color_geometry(GofJob& j, int gi, int q, const EncodeBatch& eb, size_t e) {
  const int g = j.groups[gi][q]; const EncStreamDesc& d = eb.desc[e];
  for (int i = 0; i < j.n; i++) if (has_color(j, i) && j.color[i].geo == g) {
    ColorEntry& E = j.color[i]; const rbt_atlas_params& a = E.t.atlas; const QualityOcc& o = j.qocc[i];
    const int W = a.width, H = a.height, mc = a.map_count, nf = E.t.n_frames; const size_t ys = (size_t)W * H;
    if (d.w != W || d.h != H || d.n_frames != mc * nf || !o.occ || !E.frames.empty()) { j.err = "internal: a colour target does not fit its geometry source"; return RBT_ERR_PARAM; }
    E.geo_planes = (uint16_t*)rbtk::dev_alloc(ys * (size_t)d.n_frames * 2);
    if (!E.geo_planes) { j.err = "device allocation failed"; return RBT_ERR_NOMEM; }
    GatherSet gs;
    rbtk::timer_begin(T_CENSUS);
    gs.add_coded(eb, e, W, H, E.geo_planes);
    int rc = gs.launch(j.err);
    E.frames.assign(nf, nullptr);
    for (int f = 0; f < nf && !rc; f++)
      rc = colorframe_new(j.err, *j.cloud_cache, &a, E.patches[f].data(), (int)E.patches[f].size(), o.occ + o.in_step * (size_t)f, E.geo_planes + ys * (size_t)(mc * f),
                          mc > 1 ? E.geo_planes + ys * (size_t)(mc * f + 1) : nullptr, d.bd, E.t.attr_transfer, &E.frames[f]);
    if (int bad = cloud_timed(j, E, rc)) return bad;
  }
  return 0;
}
// the three planes of coded 4:2:0 pictures as packed planar pictures (the layout launch_up444 reads): x0, y0 = the displayed window's offset in luma samples
static void gather_420(GatherSet& gs, uint16_t* const planes[3], int stride, int x0, int y0, int w, int h, uint16_t* dst) {
  const size_t ys = (size_t)w * h, cs = ys / 4;
  gs.add(planes[0] + (size_t)y0 * stride + x0, stride, w, h, dst);
  for (int c = 1; c < 3; c++) gs.add(planes[c] + (size_t)(y0 / 2) * (stride / 2) + x0 / 2, stride / 2, w / 2, h / 2, dst + ys + cs * (size_t)(c - 1));
}
static const char* merged_limit = "more than 2^21 merged points in a cloud";
// In the wait half of an attribute pipeline with colour targets, once its decoder has been collected (the geometry pipelines ran before it, gof_wait): for a frame
// without a handle the reference - the same route on the decoded input occupancy, geometry and attribute -, then per frame the score pair against the reference.
static int color_setup(GofJob& j, int gi) {
  DecodeBatch& db = j.db[gi]; const std::vector<int>& gs = j.groups[gi]; PCloudCache& cache = *j.cloud_cache;
  rbtk::set_stream(job_stream(j, gi));
  for (size_t q = 0; q < gs.size(); q++) if (has_color(j, gs[q])) {
    const int i = gs[q], ds = j.dec_of[gi][q], first = db.stream_first[ds], nf = j.color[i].t.n_frames;
    ColorEntry& E = j.color[i]; const rbt_atlas_params& a = E.t.atlas; const int W = a.width, H = a.height, mc = a.map_count;
    if ((int)E.frames.size() != nf) { j.err = "internal: the geometry half of a colour target was not made"; return RBT_ERR_PARAM; }
    bool any = false; for (int f = 0; f < nf; f++) any |= E.ref[f] == nullptr;
    E.own_ref.assign(nf, nullptr);
    rbtk::timer_begin(T_CENSUS);
    int rc = 0;
    if (any) {
      int gp = -1; size_t gq = 0; find_entry(j, E.geo, &gp, &gq);
      const DecodeBatch& gb = j.db[gp]; const int gds = j.dec_of[gp][gq]; const RbtStreamCfg& gc = gb.frames[gb.stream_first[gds]].cfg;
      const RbtStreamCfg& c = db.frames[first].cfg; const Sps& isps = db.stream_sps[ds];
      const size_t ys = (size_t)W * H, os = (size_t)E.in_ow * E.in_oh, fs = ys * 3 / 2, n_pic = (size_t)mc * nf;
      // packed: input occupancy luma, input geometry luma (both stay with the frames), input attribute 4:2:0 and its 4:4:4 planes (this block only)
      E.in_planes = (uint16_t*)rbtk::dev_alloc((os * (size_t)nf + ys * n_pic) * 2);
      DevPlanes attr, up; GatherSet gin;
      if (!E.in_planes || !attr.alloc(fs * n_pic) || !up.alloc(3 * ys * n_pic)) { j.err = "device allocation failed"; rc = RBT_ERR_NOMEM; }
      uint16_t* occ = E.in_planes; uint16_t* geo = E.in_planes + os * (size_t)nf;
      for (int f = 0; f < nf && !rc; f++) if (!E.ref[f]) {
        gin.add_decoded(j.db[E.in_pipe], E.in_ds, f, E.in_ow, E.in_oh, occ + os * (size_t)f);
        for (int m = 0; m < mc; m++) {
          gin.add_decoded(gb, gds, mc * f + m, W, H, geo + ys * (size_t)(mc * f + m));
          gather_420(gin, db.frames[first + mc * f + m].out, c.w, 2 * isps.conf_win[0], 2 * isps.conf_win[2], W, H, attr.p + fs * (size_t)(mc * f + m));
        }
      }
      if (!rc) rc = gin.launch(j.err);
      if (!rc) colorframe_upconvert(attr.p, W, H, c.bit_depth, (int)n_pic, E.t.upsample_filter, up.p);      // (pictures of frames with a handle: never gathered, never read)
      rbt_atlas_params ain = a; ain.occupancy_precision = W / E.in_ow;
      for (int f = 0; f < nf && !rc; f++) if (!E.ref[f]) {
        rc = colorframe_new(j.err, cache, &ain, E.patches[f].data(), (int)E.patches[f].size(), occ + os * (size_t)f, geo + ys * (size_t)(mc * f), mc > 1 ? geo + ys * (size_t)(mc * f + 1) : nullptr,
                            gc.bit_depth, E.t.attr_transfer, &E.own_ref[f]);
        if (!rc) rc = colorframe_color(j.err, E.own_ref[f], up.p + 3 * ys * (size_t)(mc * f), mc > 1 ? up.p + 3 * ys * (size_t)(mc * f + 1) : nullptr, c.bit_depth);
      }
      if (rbtk::dev_sync() && !rc) { j.err = "kernel execution failed"; rc = RBT_ERR_NO_DEVICE; }      // attr and up are idle before they go
    }
    for (int f = 0; f < nf && !rc; f++) {
      const PCloud* A = E.ref[f] ? E.ref[f] : colorframe_cloud(E.own_ref[f]);
      if (pcloud_merged(A) > (1 << 21) || pcloud_merged(colorframe_cloud(E.frames[f])) > (1 << 21)) { j.err = merged_limit; rc = RBT_ERR_PARAM; }
      else rc = colorframe_pair(j.err, E.frames[f], A);
    }
    if (int bad = cloud_timed(j, E, rc)) return bad;
  }
  return 0;
}
// what color_geometry and color_setup made for the pipeline's entries, released on every way out of run_rounds (the clouds' volumes go back to the context's cache)
struct ColorLive {
  GofJob& j; int gi;
  ~ColorLive() {
    if (j.color.empty() || !color_pipe(j, gi)) return;
    rbtk::set_stream(job_stream(j, gi)); rbtk::dev_sync();
    for (int i : j.groups[gi]) if (has_color(j, i)) j.color_release(i);
  }
};
// The clouds of candidate e of the round in flight - stream `q` of the pipeline's group at one QP - against the entry's references, while the round's arena is alive: the
// three planes of every reconstructed attribute picture gathered into packed 4:2:0 (the displayed window starts at the picture's origin), one up-conversion for all of
// them, then frame after frame the colour half (colorframe_color) and the colour walks on the pair's distances. Only the colour sums come back.
// A pass over a subset of the frames (desc_subset) codes np of the nf frames, as in d1_score: the gathered pictures go by the coded picture, the ColorFrames by the frame
// d.pic names; out is in pass order. per_patch (colour floors held patch by patch): per frame of the pass the figures of its patches - the sums per patch in place of
// the colour walks, out[i] made of them
static int color_score(GofJob& j, int gi, int q, const EncodeBatch& eb, size_t e, std::vector<rbt_color_result>& out, std::vector<std::vector<rbt_patch_color>>* per_patch = nullptr) {
  const int i = j.groups[gi][q]; ColorEntry& E = j.color[i]; const rbt_atlas_params& a = E.t.atlas;
  const EncStreamDesc& d = eb.desc[e]; const int W = a.width, H = a.height, mc = a.map_count, nf = E.t.n_frames, np = d.n_frames / mc;
  const size_t ys = (size_t)W * H, fs = ys * 3 / 2;
  if (d.w != W || d.h != H || d.n_frames != mc * np || (d.pic.empty() ? np != nf : d.n_total != mc * nf) || (int)E.frames.size() != nf) { j.err = "internal: a colour target does not fit its stream"; return RBT_ERR_PARAM; }
  DevPlanes attr, up; GatherSet gs;
  if (!attr.alloc(fs * (size_t)d.n_frames) || !up.alloc(3 * ys * (size_t)d.n_frames)) { j.err = "device allocation failed"; return RBT_ERR_NOMEM; }
  out.assign(np, rbt_color_result());
  if (per_patch) per_patch->assign((size_t)np, {});
  rbtk::timer_begin(T_CENSUS);
  for (int k = 0; k < d.n_frames; k++) { const RbtFrame& f = eb.frames[(size_t)eb.stream_first[e] + k]; gather_420(gs, f.out, f.cfg.w, 0, 0, W, H, attr.p + fs * (size_t)k); }
  int rc = gs.launch(j.err);
  if (!rc) colorframe_upconvert(attr.p, W, H, d.bd, d.n_frames, E.t.upsample_filter, up.p);
  for (int i = 0; i < np && !rc; i++) {
    const int f = d.pic.empty() ? i : d.pic[(size_t)(mc * i)] / mc;
    rc = colorframe_color(j.err, E.frames[f], up.p + 3 * ys * (size_t)(mc * i), mc > 1 ? up.p + 3 * ys * (size_t)(mc * i + 1) : nullptr, d.bd);
    if (!rc && per_patch) {
      std::vector<rbt_patch_color>& pp = (*per_patch)[(size_t)i]; pp.resize(E.patches[f].size());
      rc = pp.empty() ? colorframe_score(j.err, E.frames[f], &out[i]) : colorframe_score_patches(j.err, E.frames[f], (int)pp.size(), pp.data(), &out[i]);
    } else if (!rc) rc = colorframe_score(j.err, E.frames[f], &out[i]);
  }
  return cloud_timed(j, E, rc);
}
static int finish_round(GofJob& j, int gi) {
  RoundPipe& r = j.pipes[gi]; std::vector<std::vector<uint8_t>> outs;
  rbtk::set_stream(job_stream(j, gi));
  if (int rc = encode_finish(*r.eb, outs, j.st)) { j.err = r.eb->err; return rc; }
  size_t at = 0, fold_at = 0;                                       // (the words came back with the slice sizes)
  for (const EncStreamDesc& d : r.eb->desc) fold_at += (size_t)d.n_frames * RBT_SSE_WORDS;      // the folds per patch lie behind the words per picture
  for (size_t e = 0; e < r.cands.size(); e++) {
    const EncStreamDesc& d = r.eb->desc[e]; const RoundCand& c = r.cands[e]; QualitySums sums;
    if (c.pw >= 0) {      // a pass of patch walks: every frame it carried keeps this trial - NAL units, sums, payload, map - and takes the walk's step on what the trial said
      PatchWalks& pw = r.pwalks[(size_t)c.pw]; const int region = j.patch[pw.entry].region; const size_t per = (size_t)pw.wc * pw.hc;
      std::vector<rbt_d1_result> whole; std::vector<std::vector<rbt_patch_d1>> clouds;      // D1 floors: the clouds of the frames the pass carried, in pass order, patch by patch
      CloudScoresD2 g2;                                                // D2 floors: the same of the D2 figure
      if (j.patch_d1) if (int rc = d1_score(j, gi, c.q, *r.eb, e, whole, &clouds, j.d2 ? &g2 : nullptr)) return rc;
      std::vector<rbt_color_result> cwhole; std::vector<std::vector<rbt_patch_color>> cclouds;      // colour floors: the same frames recoloured, patch by patch
      if (j.patch_color) if (int rc = color_score(j, gi, c.q, *r.eb, e, cwhole, &cclouds)) return rc;
      // the pass's figure source (rbt_patch_walk.h): frame i of the pass from its cloud, or from its fold words, which lie in pass order behind the words per picture
      PatchTrial said;
      auto figures = [&](size_t i, PatchFrame& F) {
        if (j.patch_color) { patch_trial_color(cclouds[i], cwhole[i], j.color[pw.entry].t.channel, F.w.floor_mdb, said, F.color); return; }
        if (j.patch_d1 && j.d2) { patch_trial_d2(g2.patches[i], g2.whole[i], F.w.floor_mdb, said, F.d2); return; }
        if (j.patch_d1) { patch_trial_d1(clouds[i], whole[i], F.w.floor_mdb, said, F.d1); return; }
        patch_trial_psnr(&r.eb->sums[fold_at], F.samples, region, pw.bit_depth, F.w.floor_mdb, said, F.psnr);
        fold_at += (F.samples.size() + 2) * RBT_CTBSSE_WORDS;
      };
      for (size_t i = 0; i < c.pass.frames.size(); i++) {
        const size_t f = (size_t)c.pass.frames[i]; PatchFrame& F = pw.frames[f];
        frame_cut(outs[e], r.eb->pic_at[e], i, (size_t)d.gop, F.stream);
        F.sums = QualitySums();
        for (int k = 0; k < d.gop; k++, at++) quality_add_picture(F.sums, &r.eb->sums[at * RBT_SSE_WORDS], d.w, d.h);
        figures(i, F);
        F.map.assign(c.qmap.begin() + (ptrdiff_t)(per * f), c.qmap.begin() + (ptrdiff_t)(per * (f + 1)));
        patch_walk_step(F.w, said.figure.data(), said.meets.data());
      }
      pw.n_passes++;
      continue;
    }
    if (c.fw >= 0) {      // a pass: every frame it carried goes to its own walk - its NAL units and the sums of its pictures
      FrameWalks<TargetWalk>& fw = r.fwalks[c.fw];
      std::vector<rbt_d1_result> clouds;                               // a D1 target: the clouds of the frames the pass carried, in pass order
      if (has_d1(j, j.groups[gi][c.q])) if (int rc = d1_score(j, gi, c.q, *r.eb, e, clouds)) return rc;
      for (size_t i = 0; i < c.pass.frames.size(); i++) {
        TargetTried& t = fw.frames[c.pass.frames[i]].tried[c.pass.qps[i]];
        frame_cut(outs[e], r.eb->pic_at[e], i, (size_t)d.gop, t.stream);
        for (int k = 0; k < d.gop; k++, at++) quality_add_picture(t.sums, &r.eb->sums[at * RBT_SSE_WORDS], d.w, d.h);
        if (!clouds.empty()) t.d1.assign(1, clouds[i]);
        fw.n_enc[c.pass.frames[i]]++;
      }
      fw.n_passes++;
      continue;
    }
    for (int k = 0; r.sse && k < d.n_frames; k++, at++) quality_add_picture(sums, &r.eb->sums[at * RBT_SSE_WORDS], d.w, d.h);
    std::vector<rbt_d1_result> frames;                                // a D1 target: the candidate's clouds, from its reconstruction while the round's arena is alive
    CloudScoresD2 g2;                                                 // a D2 target: the same clouds' D2
    if (has_d1(j, j.groups[gi][c.q])) if (int rc = d1_score(j, gi, c.q, *r.eb, e, frames, nullptr, j.d2 ? &g2 : nullptr)) return rc;
    std::vector<rbt_color_result> cframes;                            // a colour target: the candidate's clouds, recoloured from its reconstruction
    if (!j.color.empty()) {
      if (has_color(j, j.groups[gi][c.q])) { if (int rc = color_score(j, gi, c.q, *r.eb, e, cframes)) return rc; }
      else if (c.walk < 0) if (int rc = color_geometry(j, gi, c.q, *r.eb, e)) return rc;      // a geometry source: the geometry half of its clouds, behind its only encode
    }
    if (c.walk < 0) { r.o1[c.q].swap(outs[e]); r.sums[c.q] = sums; r.d1[c.q].swap(frames); r.d2[c.q].swap(g2.whole); r.color[c.q].swap(cframes); }
    else { TargetTried& t = r.walks[c.walk].tried[c.qp]; t.stream.swap(outs[e]); t.sums = sums; t.d1.swap(frames); t.d2.swap(g2.whole); t.color.swap(cframes); r.n_enc[c.walk]++; }
  }
  r.eb.reset(); r.sse.reset(); r.ctbsse.reset();
  name_round(j, gi, r, false);
  return 0;
}
// a decoded pipeline's checks, shared by the constant-QP path and run_rounds: error words and coverage, timers, the input's picture hashes (verify_md5)
static int pipeline_decoded(GofJob& j, int gi) {
  DecodeBatch& db = j.db[gi]; const std::vector<int>& gs = j.groups[gi];
  int rc = decode_finish(db);
  if (rc) { j.err = db.err; return rc; }
  if (j.parse_timed.empty() || j.parse_timed[gi]) j.st.k_parse_ms += rbtk::timer_ms(T_PARSE);
  if (j.recon_timed.empty() || j.recon_timed[gi]) j.st.k_recon_ms += rbtk::timer_ms(T_RECON);
  // verify_md5: the hashes of the decoded pictures were compared on the GPU; a mismatch fails the job and nothing is packed
  if (!db.hash.empty()) {
    if (db.hash.fetch()) { j.err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
    for (size_t q = 0; q < gs.size(); q++) if (j.params[gs[q]].verify_md5) {
      int checked = 0, failed = 0; decode_hash_result(db, j.dec_of[gi][q], checked, failed);
      if (failed) { j.err = "input " + std::to_string(gs[q]) + ": decoded picture hash mismatch (" + std::to_string(failed) + " of " + std::to_string(checked) + " pictures)"; return RBT_ERR_MD5; }
    }
  }
  return 0;
}
static void quality_fill_result(rbt_quality_result& o, int qp, int q0, int qs, int met, int n_enc, uint64_t bytes, const QualitySums& s, int bit_depth) {
  memset(&o, 0, sizeof(o));
  o.qp = qp; o.qp_probe = q0; o.qp_start = qs; o.met = met; o.n_encodes = n_enc; o.bytes = bytes;
  for (int c = 0; c < 3; c++) {
    o.sse[c] = s.sse[c]; o.samples[c] = s.samples[c]; o.sse_occ[c] = s.sse_occ[c]; o.samples_occ[c] = s.samples_occ[c];
    o.psnr[c] = quality_psnr(s.sse[c], s.samples[c], bit_depth); o.psnr_occ[c] = quality_psnr(s.sse_occ[c], s.samples_occ[c], bit_depth);
  }
}
// Cloud targets: of every entry of the pipeline with a target the frames at the entry's own QP (own[q], the entry's only encode) or, where a walk of `kind` ran for a
// floor, at its q*
template <class Entry, class Result> static void fill_cloud_outs(GofJob& j, int gi, const std::vector<Entry>& in, std::vector<FloorOut<Result>>& out, WalkKind kind, const std::vector<std::vector<Result>>& own,
                                                                  std::vector<Result> TargetTried::*tried) {
  RoundPipe& r = j.pipes[gi]; const std::vector<int>& gs = j.groups[gi];
  if (in.empty()) return;
  out.resize(j.n);
  for (size_t q = 0; q < gs.size(); q++) if (in[gs[q]].t.n_frames > 0) {
    FloorOut<Result>& o = out[gs[q]]; const int qp = j.params[gs[q]].qp;
    o.qp = o.q0 = o.qs = qp; o.met = 1; o.n_enc = 1; o.bytes = r.o1[q].size(); o.frames = own[q]; o.cloud_ms = in[gs[q]].cloud_ms;
  }
  for (size_t k = 0; k < r.walks.size(); k++) if (r.walks[k].kind == kind) {
    const TargetWalk& w = r.walks[k]; const TargetTried& t = w.tried.find(w.qstar)->second; FloorOut<Result>& o = out[w.entry];
    o.qp = w.qstar; o.q0 = w.floor.q0; o.qs = w.start; o.met = w.met; o.n_enc = r.n_enc[k]; o.bytes = t.stream.size(); o.frames = t.*tried;
  }
}
// the public results of a pipeline whose walks have settled: a budget's (qe = the walk's start), or a floor's and the distortion of the entries without one
static void fill_results(GofJob& j, int gi) {
  RoundPipe& r = j.pipes[gi]; const std::vector<int>& gs = j.groups[gi];
  if (j.qtargets.empty()) j.results.resize(j.n); else j.qresults.resize(j.n);
  for (size_t q = 0; q < gs.size() && !j.qtargets.empty(); q++) if (!has_floor(j, gs[q])) { const int qp = j.params[gs[q]].qp; quality_fill_result(j.qresults[gs[q]], qp, qp, qp, 1, 1, r.o1[q].size(), r.sums[q], entry_bit_depth(j, gi, q)); }
  for (size_t k = 0; k < r.walks.size(); k++) {
    const TargetWalk& w = r.walks[k]; const QualityTried& t = w.tried.find(w.qstar)->second;
    if (w.kind == WALK_BUDGET) j.results[w.entry] = rbt_rate_result{w.qstar, w.start, w.met, r.n_enc[k], (uint64_t)t.stream.size(), w.budget.e_qe};
    else if (w.kind == WALK_PSNR) quality_fill_result(j.qresults[w.entry], w.qstar, w.floor.q0, w.start, w.met, r.n_enc[k], t.stream.size(), t.sums, w.bit_depth);
  }
  fill_cloud_outs(j, gi, j.d1, j.d1out, WALK_D1, r.d1, &TargetTried::d1);
  if (j.d2) fill_cloud_outs(j, gi, j.d1, j.d2out, WALK_D1, r.d2, &TargetTried::d2);
  fill_cloud_outs(j, gi, j.color, j.colorout, WALK_COLOR, r.color, &TargetTried::color);
}
// ... and of a pipeline whose entries walked frame by frame: per frame q*, qs, met, its encodes, its bytes and its figure at q*; the stream assembled from the passes
static void fill_frame_results(GofJob& j, int gi) {
  RoundPipe& r = j.pipes[gi];
  j.fout.resize(j.n);
  for (const FrameWalks<TargetWalk>& fw : r.fwalks) {
    FrameFloorOut& o = j.fout[fw.entry]; std::vector<uint64_t> bytes;
    frame_assemble(fw, r.o1[fw.q], bytes);
    o.n_passes = fw.n_passes; o.bytes = r.o1[fw.q].size();
    if (has_d1(j, fw.entry)) o.cloud_ms = j.d1[fw.entry].cloud_ms;
    for (size_t f = 0; f < fw.frames.size(); f++) {
      const TargetWalk& w = fw.frames[f]; const TargetTried& at = w.tried.find(w.qstar)->second; const QualitySums& s = at.sums;
      const bool d1 = w.kind == WALK_D1;
      o.q0 = w.floor.q0; o.bit_depth = w.bit_depth; o.pictures += 2 * (uint64_t)fw.n_enc[f];
      if (d1) o.d1.push_back(at.d1[0]);
      o.frames.push_back(rbt_frame_pick{w.qstar, w.start, w.met, fw.n_enc[f], bytes[f], d1 ? (double)at.d1[0].psnr : quality_region_psnr(s, w.region, w.bit_depth)});
      for (int c = 0; c < 3; c++) { o.sums.sse[c] += s.sse[c]; o.sums.samples[c] += s.samples[c]; o.sums.sse_occ[c] += s.sse_occ[c]; o.sums.samples_occ[c] += s.samples_occ[c]; }
    }
  }
}
// ... and of a pipeline whose entries walked patch by patch: per frame its trials, bytes, background and the picks of its settling trial; the final map; the stream assembled
// from the frames' NAL units (rule 7). The entries without a target keep their only encode (r.o1) and its sums
static void fill_patch_results(GofJob& j, int gi) {
  RoundPipe& r = j.pipes[gi]; const std::vector<int>& gs = j.groups[gi];
  j.pout.resize(j.n);
  for (size_t q = 0; q < gs.size(); q++) if (!has_patch_floor(j, gs[q])) { PatchOut& o = j.pout[gs[q]]; o.q0 = j.params[gs[q]].qp; o.bytes = r.o1[q].size(); o.sums = r.sums[q]; o.bit_depth = entry_bit_depth(j, gi, q); }
  for (const PatchWalks& pw : r.pwalks) {
    PatchOut& o = j.pout[pw.entry]; std::vector<uint8_t>& out = r.o1[pw.q];
    out.clear(); o.n_passes = pw.n_passes; o.wc = pw.wc; o.hc = pw.hc; o.bit_depth = pw.bit_depth; o.region = j.patch[pw.entry].region;
    if (has_d1(j, pw.entry)) o.cloud_ms = j.d1[pw.entry].cloud_ms;
    if (has_color(j, pw.entry)) o.cloud_ms = j.color[pw.entry].cloud_ms;
    for (const PatchFrame& F : pw.frames) {
      out.insert(out.end(), F.stream.begin(), F.stream.end()); o.map.insert(o.map.end(), F.map.begin(), F.map.end());
      o.q0 = F.w.q0; o.pictures += 2 * (uint64_t)F.w.n_trials;
      PatchOut::Frame pf; pf.n_trials = F.w.n_trials; pf.n_patches = (int)F.w.q.size(); pf.bytes = F.stream.size(); pf.psnr = F.psnr; pf.d1 = F.d1; pf.d2 = F.d2; pf.color = F.color;
      for (size_t k = 0; k < F.w.q.size(); k++) { pf.met &= F.w.met[k]; o.picks.push_back(PatchOut::Pick{F.w.q[k], F.w.met[k], F.w.failed[k], F.w.figure[k]}); }
      o.frames.push_back(std::move(pf));
      for (int c = 0; c < 3; c++) { o.sums.sse[c] += F.sums.sse[c]; o.sums.samples[c] += F.sums.samples[c]; o.sums.sse_occ[c] += F.sums.sse_occ[c]; o.sums.samples_occ[c] += F.sums.samples_occ[c]; }
    }
    o.bytes = out.size();
  }
}
// A pipeline with targets, in the wait half: its decoder is collected, the walks are seeded and the rounds run, one after the other, until every walk has settled. In a
// job with floors the occupancy pipelines have been collected by then (gof_wait), so the pooled planes and the maps the rounds read are complete. (Measured and not
// adopted, DESIGN.md 12: the rounds of a job's pipelines side by side, and the first rounds of the other jobs in flight enqueued ahead of their turn - both were slower
// than one pipeline's rounds at a time.)
static int run_rounds(GofJob& j, int gi) {
  RoundPipe& r = j.pipes[gi]; const size_t n = j.groups[gi].size();
  if (int rc = pipeline_decoded(j, gi)) return rc;
  D1Live d1_live{j, gi};                                            // (releases the pipeline's frames and reference clouds on every way out)
  ColorLive color_live{j, gi};                                      // (releases the frames of the pipeline's colour entries on every way out)
  if (!j.patch.empty()) { if (int rc = seed_patch_walks(j, gi, r)) return rc; }
  else if (j.per_frame) seed_frame_floors(j, gi, r);
  else if (j.kind == GOF_D1 || j.kind == GOF_D2) seed_floors(j, gi, r, WALK_D1);
  else if (j.kind == GOF_COLOR) seed_floors(j, gi, r, WALK_COLOR);
  else if (j.kind == GOF_QUALITY) seed_floors(j, gi, r, WALK_PSNR);
  else if (int rc = seed_budgets(j, gi, r, true)) return rc;
  if (!j.d1.empty()) if (int rc = d1_setup(j, gi)) return rc;
  if (!j.color.empty()) if (int rc = color_setup(j, gi)) return rc;
  r.o1.assign(n, {}); r.sums.assign(n, QualitySums()); r.d1.assign(n, {}); r.d2.assign(n, {}); r.color.assign(n, {}); r.n_enc.assign(r.walks.size(), 0);
  name_round(j, gi, r, true);
  for (;;) {
    if (int rc = launch_round(j, gi)) return rc;
    if (r.done) break;
    if (int rc = finish_round(j, gi)) return rc;
  }
  for (const TargetWalk& w : r.walks) if (!w.settled) { j.err = "internal: QP walk did not settle"; return RBT_ERR_PARAM; }
  for (const FrameWalks<TargetWalk>& fw : r.fwalks) if (!fw.settled()) { j.err = "internal: QP walk did not settle"; return RBT_ERR_PARAM; }
  for (const PatchWalks& pw : r.pwalks) if (!pw.settled()) { j.err = "internal: patch walk did not settle"; return RBT_ERR_PARAM; }
  if (!j.patch.empty()) { fill_patch_results(j, gi); return 0; }
  if (j.per_frame) { fill_frame_results(j, gi); return 0; }
  fill_results(j, gi);
  for (TargetWalk& w : r.walks) r.o1[w.q].swap(w.tried[w.qstar].stream);
  return 0;
}

// ------------------------------------------------------------------------------------------------ quality floors (include/rbt.h, "transcoding to a PSNR floor")
void SseSet::add(const RbtSsePic& p) { max_chunks = std::max(max_chunks, RBT_SSE_PIC_CHUNKS(p.w, p.h)); pics.push_back(p); }
int SseSet::upload() {
  const size_t n = pics.size();
  o_out = (n * sizeof(RbtSsePic) + 255) & ~(size_t)255;
  const size_t end = ext ? n * sizeof(RbtSsePic) : o_out + n * RBT_SSE_WORDS * 8;
  rbtk::dev_free(d);
  d = (uint8_t*)rbtk::dev_alloc(end);
  if (!d) return RBT_ERR_NOMEM;
  for (size_t i = 0; i < n; i++) pics[i].out = (ext ? ext : (uint64_t*)(d + o_out)) + i * RBT_SSE_WORDS;
  staging.assign(end, 0);
  memcpy(staging.data(), pics.data(), n * sizeof(RbtSsePic));
  return rbtk::h2d(d, staging.data(), end) ? RBT_ERR_NO_DEVICE : 0;
}
void SseSet::launch() const { rbtk::launch_picture_sse((const RbtSsePic*)d, (int)pics.size(), max_chunks); }
int SseSet::fetch() {
  words.assign(pics.size() * RBT_SSE_WORDS, 0);
  return !words.empty() && rbtk::d2h(words.data(), d + o_out, words.size() * 8) ? RBT_ERR_NO_DEVICE : 0;
}
// At submit, behind the encoder batches of the occupancy pipelines: the occupancy source of every entry of the pipeline (rule 3), the maps of occupancy_rd - allocated
// here, made by the occupancy pipeline's launch_occ_units like those of a constant-QP job -, and what the first round will take (rbt_job_memory): one encode per entry
static int quality_prepare(GofJob& j, SubmitPlan& s, int gi) {
  DecodeBatch& db = j.db[gi]; const std::vector<int>& gs = j.groups[gi];
  if (db.frames.empty()) return 0;
  for (size_t q = 0; q < gs.size(); q++) {
    const int i = gs[q], io = s.meas_of[i], ds = j.dec_of[gi][q], cnt = db.stream_count[ds];
    bool has = false;
    if (j.per_frame && cnt % 2) {      // a frame is two pictures: a stream that ends with half a frame has no walk for it
      j.err = "entry " + std::to_string(i) + ": floors held frame by frame need two pictures per point-cloud frame, the stream holds " + std::to_string(cnt);
      j.refused = true; return RBT_ERR_PARAM; }
    if (io >= 0 && s.occ_src[io].n > 0 && cnt > 0) {
      const OccSource& os = s.occ_src[io]; int dw, dh; displayed(db, ds, &dw, &dh);
      if (dw > 0 && dh > 0 && cnt % os.n == 0 && dw % os.ow == 0 && dh % os.oh == 0 && dw / os.ow == dh / os.oh) {
        has = true; QualityOcc& o = j.qocc[i]; o.occ = os.occ; o.in_step = os.in_step; o.n = os.n; o.ow = os.ow; o.oh = os.oh;
        if (s.occ_of[i] >= 0) {
          o.w4 = (dw + 3) / 4; o.h4 = (dh + 3) / 4;
          uint8_t* maps = (uint8_t*)rbtk::dev_alloc((size_t)os.n * o.w4 * o.h4);
          if (!maps) { j.err = "device allocation failed"; return RBT_ERR_NOMEM; }
          j.pooled.push_back(maps); s.occ_jobs.push_back(OccJob{io, maps, dw, o.w4, o.h4}); o.maps = maps;
        }
      }
    }
    if (j.qtargets[i].region == RBT_QUALITY_OCCUPIED && !has) {
      j.err = "entry " + std::to_string(i) + ": RBT_QUALITY_OCCUPIED on an entry whose occupancy source does not fit it (picture count a multiple of the occupancy frames, one whole scale in both directions)";
      j.refused = true; return RBT_ERR_PARAM; }
  }
  std::vector<RoundCand> cands; for (size_t q = 0; q < gs.size(); q++) cands.push_back(RoundCand{(int)q, j.params[gs[q]].qp, -1});
  return measure_round(j, gi, cands);
}
// Pipelines that share a HIP stream would parse one after the other; their slices go into one merged launch instead, so
// that all parsers of the stream run side by side and only the (short) tails of the pipelines follow each other.
static int launch_merged(GofJob& j) {
  const int ng = j.ng; std::vector<DecodeBatch>& db = j.db;
  for (int k = 0; k < ng; k++) {
    const int lead = j.order[k];
    if (!j.chained[lead] || db[lead].parse_external) continue;
    std::vector<int> grp;
    for (int q = k; q < ng; q++) { const int gi = j.order[q]; if (j.phys[gi] == j.phys[lead] && j.chained[gi] && !db[gi].ordered_parse && !db[gi].d_save) grp.push_back(gi); }
    if (grp.size() < 2 || grp[0] != lead) continue;
    j.tasks_keep.emplace_back(); std::vector<RbtParseTask>& tasks = j.tasks_keep.back(); int mw4 = 0;
    std::vector<uint32_t> task_bytes; bool row_tasks = false;
    for (int gi : grp) {
      for (size_t i = 0; i < db[gi].slices.size(); i++) { tasks.push_back(RbtParseTask{db[gi].d_frames, db[gi].d_slices, db[gi].d_rbsp, db[gi].lists_keep[i], 0}); task_bytes.push_back(db[gi].slices[(size_t)db[gi].lists_keep[i]].data_size); }
      mw4 = std::max(mw4, decode_max_w4(db[gi])); db[gi].parse_external = true; j.parse_timed[gi] = gi == lead; row_tasks |= db[gi].has_row_tasks;
    }
    // Longest first: a launch's waves start in list order, and when more slices are in flight than the GPU holds waves (several jobs' launches side by side) the ones that
    // wait should be the short ones - the launch lasts as long as its largest slice (an attribute IDR) however late that one starts. Not for lists with row tasks of
    // wavefront streams: there a task must come after the task of the row above it.
    if (!row_tasks) {
      std::vector<size_t> ord(tasks.size()); for (size_t i = 0; i < ord.size(); i++) ord[i] = i;
      std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return task_bytes[a] > task_bytes[b]; });
      std::vector<RbtParseTask> sorted; sorted.reserve(tasks.size()); for (size_t i : ord) sorted.push_back(tasks[i]);
      tasks.swap(sorted);
    }
    // ... and the pictures of one dependency level of all of them go on one wavefront (58 launches per level instead of 58
    // per level and pipeline, one after the other)
    size_t n_levels = 0; for (int gi : grp) n_levels = std::max(n_levels, db[gi].level_frames.size());
    j.refs_keep.emplace_back(); std::vector<RbtFrameRef>& refs = j.refs_keep.back();
    std::vector<ReconLevel> levels; size_t queue_words = 0;
    for (size_t l = 0; l < n_levels; l++) {
      std::vector<LevelPic> pics;
      for (int gi : grp) if (l < db[gi].level_frames.size()) for (int fi : db[gi].level_frames[l]) pics.push_back(LevelPic{&db[gi], fi});
      levels.push_back(recon_level_of(pics, &refs)); queue_words += rbtk::recon_queue_words(levels.back().ctbs);
    }
    const int rmode = recon_mode_for(levels.data(), levels.size());
    RbtParseTask* d_tasks = (RbtParseTask*)rbtk::dev_alloc(tasks.size() * sizeof(RbtParseTask));
    RbtFrameRef* d_refs = (RbtFrameRef*)rbtk::dev_alloc(refs.size() * sizeof(RbtFrameRef));
    if (d_tasks) j.pooled.push_back(d_tasks);
    if (d_refs) j.pooled.push_back(d_refs);
    uint32_t* d_queue = rmode == 2 ? (uint32_t*)rbtk::dev_alloc(queue_words * 4) : nullptr;
    if (d_queue) j.pooled.push_back(d_queue);
    if (!d_tasks || !d_refs || (rmode == 2 && !d_queue)) { j.err = "device allocation failed"; return RBT_ERR_NOMEM; }
    { size_t r = 0, q = 0;      // the merged levels' share of the refs and the queue memory; the lead batch's spare ticket words
      for (size_t l = 0; l < n_levels; l++) { ReconLevel& lv = levels[l]; lv.refs = d_refs + r; r += (size_t)lv.n; lv.ticket = db[lead].d_tickets + TICKET_MERGED_LEVEL + l;
        if (d_queue) { lv.queue = d_queue + q; q += rbtk::recon_queue_words(lv.ctbs); } } }
    rbtk::set_stream(job_stream(j, lead));
    if (d_queue && rbtk::dev_memset(d_queue, 0, queue_words * 4)) { j.err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
    if (rbtk::h2d(d_tasks, tasks.data(), tasks.size() * sizeof(RbtParseTask)) || rbtk::h2d(d_refs, refs.data(), refs.size() * sizeof(RbtFrameRef))) { j.err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
    rbtk::timer_begin(T_PARSE); rbtk::launch_parse_tasks(d_tasks, (int)tasks.size(), mw4, row_tasks ? db[lead].d_tickets + TICKET_MERGED_PARSE : nullptr); rbtk::timer_end(T_PARSE);
    rbtk::timer_begin(T_RECON);
    for (size_t l = 0; l < n_levels; l++) {
      launch_recon(levels[l], rmode);
      for (int gi : grp) if (l < db[gi].level_frames.size()) decode_launch_filters(db[gi], l);
    }
    rbtk::timer_end(T_RECON);
    for (int gi : grp) { db[gi].recon_external = true; j.recon_timed[gi] = gi == lead; }
  }
  return 0;
}

// One pipeline onto its stream: decode -> pool -> encode without a host round trip in between (PCCTranscoder.cpp:428-448, :466, :825-904).
// Arena sharing (setup_encode) rests on the order made here: the encoder's first write to a buffer of a decoded picture has to come behind the decoder's last read of it.
// The reconstruction of picture k reads its levels; its deblocking and SAO launches - decode_launch_filters, the last thing decode_launch_level enqueues for a level - read
// its pre-SAO samples; nothing later does (reference pictures and the input's hash check read the SAO output). So:
//  - one HIP stream: every level of the decoder is enqueued on the pipeline's stream before encode_launch_intra, the encoder's first kernel, goes onto the same stream
//    (the merged launches of pipelines that share a stream, launch_merged, are enqueued earlier still, on that same stream);
//  - intra coding forked onto the auxiliary stream: rbtk::stream_wait(aux, sid) below records an event on the pipeline's stream right behind decode_launch_level(fork_level),
//    fork_level being the highest dependency level of any decoded picture an output I picture is coded from - so those pictures' filters are behind the event, and I
//    pictures alias nothing else. The P pictures (encode_launch_inter) stay on the pipeline's stream, behind every level.
static int enqueue_pipeline(GofJob& j, SubmitPlan& s, int gi) {
  const int sid = job_stream(j, gi), aux = job_stream(j, rbtk::RBT_AUX_STREAM); rbtk::set_stream(sid);
  DecodeBatch& db = j.db[gi]; const std::vector<PoolJob>& jobs = s.pool_jobs[gi];
  if (!j.chained[gi]) {      // a pipeline with rate targets: the decoder, the input's hash check and the census; run_rounds encodes when the job is collected
    if (int rc = decode_launch(db)) { j.err = db.err; return rc; }
    if (!db.hash.empty()) decode_launch_hash(db);
    if (!db.census.empty()) db.census.launch();
    return 0;
  }
  // Intra pictures of the output only read the decoded pictures they are re-encoded from. When those are complete
  // before the last dependency level of the decoder, analysis + intra coding run on an auxiliary stream underneath the
  // remaining reconstruction levels.
  EncodeBatch& e = j.eb[gi]; e.main_stream = sid;
  size_t n_levels = db.level_frames.size(), fork_level = 0;
  for (size_t q = 0; q < e.frames.size(); q++) if (e.frame_is_idr[q]) {
    const int si = e.frame_stream[q], local = (int)q - e.stream_first[si], ds = j.dec_of[gi][si];
    fork_level = std::max(fork_level, (size_t)db.frames[db.stream_first[ds] + local].level);
  }
  int intra_done = 0;
  const bool fork = gi == j.order[0] && j.has_aux && j.ng <= rbtk::RBT_AUX_STREAM && jobs.empty() && e.pad_jobs.empty() && fork_level + 1 < n_levels;   // longest pipeline only: one spare stream
  const bool banded = db.d_save != nullptr && !db.ordered_parse;
  if (int rc = banded ? decode_launch_chunked(db, parse_bands(), sid, aux) : decode_launch_parse(db)) { j.err = db.err; return rc; }
  if (!db.recon_external) rbtk::timer_begin(T_RECON);
  for (size_t l = 0; l < n_levels && !db.recon_external; l++) {
    if (!(banded && l == 0)) decode_launch_level(db, l);
    if (fork && l == fork_level) {
      e.aux_stream = aux;
      rbtk::stream_wait(e.aux_stream, sid);
      if (s.consumes[gi]) for (int m : s.occ_marks) rbtk::stream_wait_mark(e.aux_stream, m);      // occupancy-aware coding: the maps are made on the occupancy pipeline's stream
      rbtk::set_stream(e.aux_stream); encode_launch_intra(e); intra_done = rbtk::stream_mark(e.aux_stream); encode_launch_entropy_intra(e); rbtk::set_stream(sid);
    }
  }
  if (!db.recon_external) rbtk::timer_end(T_RECON);
  // the input's picture hashes behind the decoder's last filter: on the auxiliary stream where the intra coding was forked there, underneath the rest of the encoder
  if (!db.hash.empty()) {
    if (fork) { rbtk::stream_wait(aux, sid); rbtk::set_stream(aux); decode_launch_hash(db); rbtk::set_stream(sid); }
    else decode_launch_hash(db);
  }
  if (!jobs.empty()) {
    // the pictures of one stream are of one size and their pooled copies evenly spaced (setup_encode): one launch per run of such jobs
    rbtk::timer_begin(T_POOL);
    for (size_t a0 = 0; a0 < jobs.size();) {
      size_t a1 = a0 + 1; const PoolJob& p0 = jobs[a0];
      const size_t step = a1 < jobs.size() ? (size_t)(jobs[a1].y - p0.y) : 0;
      while (a1 < jobs.size() && jobs[a1].stride == p0.stride && jobs[a1].w == p0.w && jobs[a1].h == p0.h && jobs[a1].grey == p0.grey && (size_t)(jobs[a1].y - p0.y) == step * (a1 - a0)) a1++;
      std::vector<const uint16_t*> ins; for (size_t q = a0; q < a1; q++) ins.push_back(jobs[q].in);
      rbtk::launch_pool_many(ins.data(), (int)ins.size(), p0.stride, p0.w, p0.h, 2, p0.y, step, p0.grey);
      a0 = a1;
    }
    rbtk::timer_end(T_POOL);
  }
  if (s.feeds_any[gi]) {
    for (const OccJob& oj : s.occ_jobs) { const OccSource& os = s.occ_src[oj.source]; if (os.pipeline == gi) rbtk::launch_occ_units(os.occ, os.in_step, os.n, os.ow, os.oh, oj.W, oj.w4, oj.h4, oj.maps); }
    s.occ_marks.push_back(rbtk::stream_mark(sid));
  }
  if (s.consumes[gi]) for (int m : s.occ_marks) rbtk::stream_wait_mark(sid, m);
  if (fork) rbtk::stream_wait_mark(sid, intra_done); else { encode_launch_intra(e); encode_launch_entropy_intra(e); }
  encode_launch_inter(e);
  // the reconstructions' hashes (md5_sei) once SAO has been applied to all of them: beside the inter pictures' entropy coding where there is an auxiliary stream
  if (!e.hash.empty()) {
    if (fork) { const int m = rbtk::stream_mark(sid); rbtk::stream_wait_mark(aux, m); rbtk::set_stream(aux); e.hash.launch(); rbtk::set_stream(sid); }
    else e.hash.launch();
  }
  encode_launch_entropy_rest(e);
  if (fork) rbtk::stream_wait(sid, e.aux_stream);      // the intra pictures' entropy coding and the hashes on the auxiliary stream
  return 0;
}

// A job with cloud targets runs as a job with quality floors that are all 0; the targets are kept with their patch lists copied (the caller's arrays may go when submit returns)
template <class Entry, class Target> static void keep_cloud_targets(GofJob& j, std::vector<Entry>& to, const CloudRequest<Target>& req) {
  j.qtargets.assign(j.n, rbt_quality_target{(uint32_t)sizeof(rbt_quality_target), 0, RBT_QUALITY_ALL, 0, 0}); j.qocc.assign(j.n, QualityOcc());
  to.resize(j.n); j.cloud_cache = req.cache;
  for (int i = 0; i < j.n; i++) {
    Entry& E = to[i]; E.t = req.targets[i]; E.ref = req.refs[i];
    for (int f = 0; f < E.t.n_frames; f++) E.patches.emplace_back(E.t.patches[f], E.t.patches[f] + E.t.n_patches[f]);
    E.t.patches = nullptr; E.t.n_patches = nullptr; E.t.reference = nullptr;
  }
}
// Phase A of a job: plan, build and upload everything, then enqueue. Every upload of the job is issued before its first kernel: a copy from pageable memory blocks the host
// until the stream has reached it, and pipelines may share a stream. The first failure ends the submission (j.rc, j.err); gof_wait drains what was enqueued.
GofJob* gof_submit(int slot, int depth, const GofRequest& r) {
  GofJob* J = new GofJob(); GofJob& j = *J;
  const int n = r.n; const rbt_stream_params* p = r.params;
  j.per_frame = r.per_frame && (r.quality || r.d1);
  j.patch_d1 = r.patch_d1 && r.patch_floors && r.d1;
  j.d2 = r.d2_normals && r.d1 && !j.per_frame;
  j.patch_color = r.patch_color && r.patch_floors && r.color;
  if (j.d2) j.normals = *r.d2_normals;
  j.kind = j.patch_color ? GOF_COLOR_PATCHES : j.d2 ? (j.patch_d1 ? GOF_D2_PATCHES : GOF_D2) : j.patch_d1 ? GOF_D1_PATCHES : r.patch_floors ? GOF_QUALITY_PATCHES : r.color ? GOF_COLOR : r.d1 ? (j.per_frame ? GOF_D1_FRAMES : GOF_D1) : r.quality ? (j.per_frame ? GOF_QUALITY_FRAMES : GOF_QUALITY) : GOF_PLAIN;
  struct Footprint { GofJob& j; size_t a0; ~Footprint() { j.dev_bytes = rbtk::dev_alloc_total() - a0; } } footprint{j, rbtk::dev_alloc_total()};
  j.t_all = now_ms(); j.n = n; j.slot = slot; memset(&j.st, 0, sizeof(j.st));
  j.params.assign(p, p + n); j.n_in.assign(r.n_in, r.n_in + n);
  if (r.targets) j.targets.assign(r.targets, r.targets + n);
  if (r.frame_qp) j.frame_qp = *r.frame_qp;
  if (r.qp_maps) j.qp_maps = *r.qp_maps;
  if (r.quality) { j.qtargets.assign(r.quality, r.quality + n); j.qocc.assign(n, QualityOcc()); }
  if (r.d1) keep_cloud_targets(j, j.d1, *r.d1);
  if (r.color) keep_cloud_targets(j, j.color, *r.color);
  if (r.patch_floors) {      // runs as a job with quality floors that are all 0, in each entry's region
    j.patch = *r.patch_floors; j.qocc.assign(n, QualityOcc());
    j.qtargets.clear();      // (a job with D1 or colour floors held patch by patch has passed keep_cloud_targets above, which filled them; a job with PSNR floors per patch comes here with none)
    for (int i = 0; i < n; i++) j.qtargets.push_back(rbt_quality_target{(uint32_t)sizeof(rbt_quality_target), 0, j.patch[i].region, 0, 0});
  }
  SubmitPlan s; s.in = r.in; s.p = p; s.gof_rule = r.gof_rule;
  int rc = plan_pipelines(j, s, depth);
  j.t_gpu = now_ms();
  if (!rc) rc = build_decoders(j, s);
  if (!rc) rc = check_frame_qp(j);
  if (!rc) rc = check_qp_maps(j);
  if (!rc) rc = check_patch_floors(j);
  if (!rc) rc = build_encoders(j, s);
  if (!rc) rc = launch_merged(j);
  // enqueue order: longest pipeline first - except that a pipeline whose occupancy maps others wait for goes in front of them (an event has to be recorded before it is waited for)
  for (int feeding = 1; feeding >= 0; feeding--) for (int k = 0; k < j.ng && !rc; k++) if (s.feeds_any[j.order[k]] == feeding) rc = enqueue_pipeline(j, s, j.order[k]);
  j.rc = rc;
  return J;
}

// What gof_wait hands to the caller beside the streams. Every array is a copy made here (malloc'd, rbt_free; never NULL, an empty vector's neither); the first allocation that
// fails ends the copying - copy returns nullptr from then on -, and gof_wait takes back every array given so far together with the streams: all or nothing
struct HandOver {
  std::vector<void*> given; int rc = 0;
  template <class T> T* copy(const std::vector<T>& v) {
    if (rc) return nullptr;
    T* p = (T*)malloc(std::max<size_t>(1, v.size() * sizeof(T)));
    if (!p) { rc = RBT_ERR_NOMEM; return nullptr; }
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    given.push_back(p);
    return p;
  }
  void take_back() { for (void* p : given) free(p); given.clear(); }
};
// the result arrays whose entries carry arrays of their own, zeroed: before anything is filled in, and again when everything is taken back
static void zero_results(const GofResults& r, int n) {
  auto zero = [n](auto* a) { if (a) memset(a, 0, sizeof(*a) * (size_t)n); };
  zero(r.d1); zero(r.color); zero(r.frames); zero(r.patches); zero(r.d1_patches); zero(r.d2); zero(r.d2_patches); zero(r.color_patches);
}
// The public results of a job with cloud targets: per entry its own QP and one encode, or what the rounds left of an entry with a target (FloorOut) with the statistics
// over its frames
template <class Entry, class Result, class Public, class Stats> static void cloud_results(const GofJob& j, HandOver& h, const std::vector<Entry>& in, const std::vector<FloorOut<Result>>& outs, Public* res,
                                                                                         const size_t* n_out, Stats stats) {
  for (int i = 0; i < j.n && !h.rc; i++) {
    Public& o = res[i];
    o.qp = o.qp_probe = o.qp_start = j.params[i].qp; o.met = 1; o.n_encodes = j.is_pass[i] ? 0 : 1; o.bytes = (uint64_t)n_out[i];
    if (in.empty() || in[i].t.n_frames <= 0 || i >= (int)outs.size()) continue;
    const FloorOut<Result>& r = outs[i];
    o.qp = r.qp; o.qp_probe = r.q0; o.qp_start = r.qs; o.met = r.met; o.n_encodes = r.n_enc; o.bytes = r.bytes; o.cloud_ms = r.cloud_ms; o.n_frames = (int)r.frames.size();
    stats(o, r.frames.data());
    o.frames = h.copy(r.frames);
  }
}
// The public results of a job with floors held patch by patch, either kind: per entry its own QP and its stream, or what the rounds left of an entry with a target
// (PatchOut) - the header, the final map, the frames and their picks, every frame pointing at its own. What a kind adds to the result, to a frame and to its picks:
static void patch_payload(rbt_patch_floor_result& o, const PatchOut& r, int met, int n_enc) { quality_fill_result(o.sums, -1, -1, -1, met, n_enc, o.bytes, r.sums, r.bit_depth); }
static void patch_payload(rbt_patch_d1_result& o, const PatchOut& r, int, int) { o.cloud_ms = r.cloud_ms; }
static void patch_payload(rbt_patch_d2_result& o, const PatchOut& r, int, int) { o.cloud_ms = r.cloud_ms; }
static void patch_payload(rbt_patch_color_result& o, const PatchOut& r, int, int) { o.cloud_ms = r.cloud_ms; }
static void patch_payload(rbt_patch_frame& o, rbt_patch_pick* picks, const PatchOut& r, const PatchOut::Frame& f) {
  for (int c = 0; c < 3; c++) o.background[c] = f.psnr.background[c];
  for (size_t k = 0; k < f.psnr.patches.size(); k++) { const PatchSums& s = f.psnr.patches[k]; picks[k].sse = r.region ? s.sse_occ : s.sse; picks[k].samples = r.region ? s.samples_occ : s.samples; }
}
static void patch_payload(rbt_patch_d1_frame& o, rbt_patch_d1_pick* picks, const PatchOut&, const PatchOut::Frame& f) {
  o.d1 = f.d1.whole;
  for (size_t k = 0; k < f.d1.patches.size(); k++) picks[k].d1 = f.d1.patches[k];
}
static void patch_payload(rbt_patch_d2_frame& o, rbt_patch_d2_pick* picks, const PatchOut&, const PatchOut::Frame& f) {
  o.d2 = f.d2.whole;
  for (size_t k = 0; k < f.d2.patches.size(); k++) picks[k].d2 = f.d2.patches[k];
}
static void patch_payload(rbt_patch_color_frame& o, rbt_patch_color_pick* picks, const PatchOut&, const PatchOut::Frame& f) {
  o.color = f.color.whole;
  for (size_t k = 0; k < f.color.patches.size(); k++) picks[k].color = f.color.patches[k];
}
template <class Public> static void patch_results(const GofJob& j, HandOver& h, Public* res, const size_t* n_out) {
  typedef typename std::remove_pointer<decltype(res->frames)>::type Frame; typedef typename std::remove_pointer<decltype(res->picks)>::type Pick;
  const PatchOut none;      // an entry no round coded - a pass-through or occupancy entry -: no frames, no sums
  for (int i = 0; i < j.n && !h.rc; i++) {
    Public& o = res[i];
    const PatchOut& r = i < (int)j.pout.size() && !j.is_pass[i] && j.params[i].video_type != RBT_VIDEO_OCCUPANCY ? j.pout[i] : none;
    o.qp_probe = j.params[i].qp; o.met_all = 1; o.bytes = (uint64_t)n_out[i];
    if (r.frames.empty()) { patch_payload(o, r, 1, j.is_pass[i] ? 0 : 1); continue; }      // no target: the sums of its only encode
    o.n_frames = (int)r.frames.size(); o.qp_probe = r.q0; o.n_passes = r.n_passes; o.pictures_encoded = r.pictures; o.w_ctb = r.wc; o.h_ctb = r.hc;
    std::vector<Frame> frames(r.frames.size()); std::vector<Pick> picks(r.picks.size()); size_t at = 0;
    for (size_t f = 0; f < frames.size(); f++) {
      const PatchOut::Frame& rf = r.frames[f]; Frame& pf = frames[f];
      pf.n_trials = rf.n_trials; pf.met = rf.met; pf.n_patches = rf.n_patches; pf.bytes = rf.bytes; o.met_all &= rf.met;
      for (int k = 0; k < rf.n_patches; k++) { const PatchOut::Pick& rp = r.picks[at + k]; Pick& pk = picks[at + k]; pk.qp = rp.qp; pk.met = rp.met; pk.failed = rp.failed; pk.figure = rp.figure; }
      patch_payload(pf, picks.data() + at, r, rf);
      at += (size_t)rf.n_patches;
    }
    patch_payload(o, r, o.met_all, (int)(r.pictures / 2));
    o.map = h.copy(r.map); o.frames = h.copy(frames); o.picks = h.copy(picks);
    at = 0; for (int f = 0; f < o.n_frames && !h.rc; f++) { o.frames[f].patches = o.picks + at; at += (size_t)o.frames[f].n_patches; }
  }
}
// phase B, shortest pipeline first: one sync per stream, then slice sizes -> pack -> NAL assembly. Consumes the job.
int gof_wait(GofJob* J, rbt_stats& st_out, std::string& err_out, const GofResults& res) {
  std::unique_ptr<GofJob> guard(J); GofJob& j = *J;
  uint8_t** out = res.out; size_t* n_out = res.n_out; int* n_flat = res.n_flat;
  rbt_rate_result* results = res.rate; rbt_quality_result* qresults = res.quality; rbt_d1_floor_result* d1results = res.d1; rbt_color_floor_result* cresults = res.color; rbt_frame_floor_result* fresults = res.frames;
  const int n = j.n, ng = j.ng; int rc = j.rc;
  rbt_stats& st = j.st; std::string& err = j.err;
  std::vector<DecodeBatch>& db = j.db; std::vector<EncodeBatch>& eb = j.eb; const rbt_stream_params* p = j.params.data();
  for (int i = 0; i < n; i++) { out[i] = nullptr; n_out[i] = 0; }
  zero_results(res, n);
  std::vector<std::vector<uint8_t>> outs(n);
  // a job with quality floors: the pipelines that were encoded at submit first - its occupancy pipelines, whose pooled planes and maps the others' rounds read -, then those
  // that are encoded here; every other job has one pass
  const bool quality = !j.qtargets.empty();
  // (a job with colour floors has a third pass: the pipelines with a colour target behind the geometry pipelines, whose reconstructions their clouds are made of)
  for (int pass = 0; pass < (quality ? 3 : 1); pass++) for (int k = ng - 1; k >= 0; k--) {
    const int gi = j.order[k], sid = job_stream(j, gi); const std::vector<int>& gs = j.groups[gi]; rbtk::set_stream(sid);
    if (quality && (j.rate_pipe[gi] ? (color_pipe(j, gi) ? 2 : 1) : 0) != pass) continue;
    if (rc) { rbtk::dev_sync(); continue; }              // drain the remaining streams before their arenas are released
    if (db[gi].frames.empty()) continue;
    std::vector<std::vector<uint8_t>> o1;
    if (j.rate_pipe[gi]) { rc = run_rounds(j, gi); rbtk::set_stream(sid); if (rc) continue; o1.swap(j.pipes[gi].o1); }      // seeds, rounds of trial encodes, walks
    else {
      rc = pipeline_decoded(j, gi);
      if (rc) continue;
      rc = encode_finish(eb[gi], o1, st);
      if (rc) { if (err.empty()) err = eb[gi].err; continue; }
    }
    for (size_t q = 0; q < gs.size(); q++) outs[gs[q]].swap(o1[q]);
  }
  rbtk::set_stream(0);
  if (rc) { err_out = err; st_out = st; return rc; }
  if (n_flat) { *n_flat = 0; for (int g = 0; g < ng; g++) *n_flat += db[g].n_flat; }      // decoded pictures reconstructed with flat chroma (came back with the error words: decode_finish)
  for (int i = 0; i < n; i++) if (j.is_pass[i]) outs[i].swap(j.passthrough[i]);
  st.gpu_ms = now_ms() - j.t_gpu;
  HandOver h; h.rc = hand_out(outs, out, n_out);
  if (results) for (int i = 0; i < n; i++) {
    if (has_target(j, i)) { results[i] = j.results[i]; continue; }
    results[i] = rbt_rate_result{p[i].qp, p[i].qp, 1, j.is_pass[i] ? 0 : 1, (uint64_t)n_out[i], 0};
  }
  if (qresults) for (int i = 0; i < n; i++) {
    if (quality && !j.is_pass[i] && p[i].video_type != RBT_VIDEO_OCCUPANCY && i < (int)j.qresults.size()) { qresults[i] = j.qresults[i]; continue; }
    quality_fill_result(qresults[i], p[i].qp, p[i].qp, p[i].qp, 1, j.is_pass[i] ? 0 : 1, (uint64_t)n_out[i], QualitySums(), 8);
  }
  if (fresults) for (int i = 0; i < n && !h.rc; i++) {
    rbt_frame_floor_result& o = fresults[i];
    o.qp_probe = p[i].qp; o.met_all = 1; o.bytes = (uint64_t)n_out[i];
    quality_fill_result(o.sums, -1, -1, -1, 1, 0, o.bytes, QualitySums(), 8);
    if (i >= (int)j.fout.size() || j.fout[i].frames.empty()) continue;
    const FrameFloorOut& r = j.fout[i];
    o.n_frames = (int)r.frames.size(); o.qp_probe = r.q0; o.n_passes = r.n_passes; o.pictures_encoded = r.pictures; o.cloud_ms = r.cloud_ms;
    for (const rbt_frame_pick& f : r.frames) o.met_all &= f.met;
    quality_fill_result(o.sums, -1, -1, -1, o.met_all, (int)(r.pictures / 2), o.bytes, r.sums, r.bit_depth);
    o.frames = h.copy(r.frames);
    if (!r.d1.empty()) o.d1 = h.copy(r.d1);
  }
  if (res.patches) patch_results(j, h, res.patches, n_out);
  if (res.d1_patches) patch_results(j, h, res.d1_patches, n_out);
  if (res.d2_patches) patch_results(j, h, res.d2_patches, n_out);
  if (res.color_patches) patch_results(j, h, res.color_patches, n_out);
  if (res.d2) cloud_results(j, h, j.d1, j.d2out, res.d2, n_out, [](rbt_d2_floor_result& o, const rbt_d2_result* f) { d1_stats(f, o.n_frames, &o.mean_d2, &o.min_d2); });
  if (d1results) cloud_results(j, h, j.d1, j.d1out, d1results, n_out, [](rbt_d1_floor_result& o, const rbt_d1_result* f) { d1_stats(f, o.n_frames, &o.mean_d1, &o.min_d1); });
  if (cresults) cloud_results(j, h, j.color, j.colorout, cresults, n_out, [](rbt_color_floor_result& o, const rbt_color_result* f) { color_stats(f, o.n_frames, o.mean_psnr, o.min_psnr); });
  rc = h.rc;
  if (rc) { h.take_back(); zero_results(res, n); for (int i = 0; i < n; i++) { free(out[i]); out[i] = nullptr; n_out[i] = 0; } }      // all or nothing
  // SURVEY.md 8(d) algorithmic traffic: per coded picture of S samples (2 bytes each): decode writes S, P pictures read
  // their reference once; encode reads the source S, writes the reconstruction S (I) and reads the reference (P)
  uint64_t bytes = 0;
  for (int g = 0; g < ng; g++) {
    for (size_t k = 0; k < db[g].frames.size(); k++) { uint64_t s2 = frame_samples(db[g].frames[k].cfg) * 2; bytes += s2 + (db[g].frames[k].level ? s2 : 0); }
    for (size_t k = 0; k < eb[g].frames.size(); k++) { uint64_t s2 = frame_samples(eb[g].frames[k].cfg) * 2; bytes += s2 + s2; }
  }
  for (int i = 0; i < n; i++) bytes += j.n_in[i] + n_out[i];
  st.algorithmic_bytes = bytes;
  st.total_ms = now_ms() - j.t_all;
  st_out = st; err_out = err;
  return rc;
}
void gof_abandon(GofJob* J) {   // a job nobody will wait for: drain its streams, then free it
  if (!J) return;
  for (int g = 0; g < J->ng; g++) { rbtk::set_stream(job_stream(*J, g)); rbtk::dev_sync(); }
  rbtk::set_stream(job_stream(*J, rbtk::RBT_AUX_STREAM)); rbtk::dev_sync(); rbtk::set_stream(0);
  delete J;
}

int encode_yuv(rbt_stats& st, std::string& err, const uint16_t* yuv, int w, int h, int bd, int n_frames, int qp, int gop, int lossless, int log2_ctb, int rows, int md5,
               uint8_t** out, size_t* n_out) {
  memset(&st, 0, sizeof(st));
  *out = nullptr; *n_out = 0;
  if (w <= 0 || h <= 0 || w % 2 || h % 2 || bd < 8 || bd > 12) { err = "bad picture format"; return RBT_ERR_PARAM; }
  if (md5 < RBT_HASH_NONE || md5 > RBT_HASH_CHECKSUM) { err = "md5_sei must be an RBT_HASH_* kind"; return RBT_ERR_PARAM; }
  size_t ys = (size_t)w * h, cs = (size_t)(w / 2) * (h / 2), fs = ys + 2 * cs;
  uint16_t* buf = (uint16_t*)rbtk::dev_alloc(fs * 2 * (size_t)n_frames);
  if (!buf) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  struct G { void* p; ~G() { rbtk::dev_free(p); } } g{buf};
  if (rbtk::h2d(buf, yuv, fs * 2 * (size_t)n_frames)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  EncodeBatch eb; eb.desc.resize(1);
  EncStreamDesc& d = eb.desc[0];
  d.w = w; d.h = h; d.bd = bd; d.n_frames = n_frames; d.qp = qp; d.i_qp_offset = lossless ? 0 : -3; d.gop = gop; d.lossless = lossless; d.log2_ctb = log2_ctb; d.rows = rows; d.md5 = md5;
  for (int k = 0; k < 3; k++) d.src[k].resize(n_frames);
  for (int i = 0; i < n_frames; i++) { uint16_t* y = buf + fs * (size_t)i; d.src[0][i] = y; d.src[1][i] = y + ys; d.src[2][i] = y + ys + cs; }
  int rc = encode_build(eb);
  std::vector<std::vector<uint8_t>> outs;
  if (!rc) rc = encode_run(eb, outs, st);
  if (rc) { err = eb.err; return rc; }
  return hand_out(outs, out, n_out);
}

// rbt_picture_hash: the pictures go to the device with every plane 16-byte aligned (the hash kernels' loads), RBT_HASH_MAX_PICS at a time
int picture_hash_host(std::string& err, const uint16_t* yuv, int w, int h, int bd, int n_frames, int kind, uint8_t* out) {
  if (w <= 0 || h <= 0 || w % 2 || h % 2 || w > 16384 || h > 16384 || bd < 8 || bd > 16 || n_frames < 1) { err = "bad picture format"; return RBT_ERR_PARAM; }
  if (kind < RBT_HASH_MD5 || kind > RBT_HASH_CHECKSUM) { err = "kind must be RBT_HASH_MD5, RBT_HASH_CRC or RBT_HASH_CHECKSUM"; return RBT_ERR_PARAM; }
  const size_t ys = (size_t)w * h, cs = (size_t)(w / 2) * (h / 2), fs = ys + 2 * cs;
  const size_t ay = (ys + 7) & ~(size_t)7, ac = (cs + 7) & ~(size_t)7, per = ay + 2 * ac;   // samples per picture on the device
  for (int f0 = 0; f0 < n_frames; f0 += RBT_HASH_MAX_PICS) {
    const int m = std::min(n_frames - f0, (int)RBT_HASH_MAX_PICS);
    std::vector<uint16_t> staging(per * (size_t)m, 0);
    for (int k = 0; k < m; k++) {
      const uint16_t* src = yuv + fs * (size_t)(f0 + k); uint16_t* dst = staging.data() + per * (size_t)k;
      memcpy(dst, src, ys * 2); memcpy(dst + ay, src + ys, cs * 2); memcpy(dst + ay + ac, src + ys + cs, cs * 2);
    }
    uint16_t* buf = (uint16_t*)rbtk::dev_alloc(staging.size() * 2);
    if (!buf) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
    struct G { void* p; ~G() { rbtk::dev_free(p); } } g{buf};
    if (rbtk::h2d(buf, staging.data(), staging.size() * 2)) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
    HashSet hs;
    for (int k = 0; k < m; k++) {
      uint16_t* y = buf + per * (size_t)k; const uint16_t* planes[3] = {y, y + ay, y + ay + ac};
      if (hs.add(planes, w, h, bd, kind) < 0) { err = "picture cannot be hashed"; return RBT_ERR_UNSUPPORTED; }
    }
    int rc = hs.upload();
    if (!rc) { hs.launch(); rc = hs.fetch(); }
    if (rc) { err = "device transfer failed"; return rc; }
    memcpy(out + (size_t)f0 * 48, hs.out.data(), (size_t)m * 48);
  }
  return 0;
}

// rbt_level_census: the planes go to the device back to back (every plane 8-byte aligned: w and h are multiples of 8), the maps behind them
int level_census_host(std::string& err, const int16_t* y, const int16_t* cb, const int16_t* cr, int w, int h, const int8_t* qp4, const uint8_t* pm4, uint32_t* hist) {
  if (w <= 0 || h <= 0 || (w | h) & 7 || w > 8192 || h > 8192) { err = "picture size must be a multiple of 8 and at most 8192"; return RBT_ERR_PARAM; }
  const size_t ys = (size_t)w * h, cs = ys / 4, u = ys / 16;
  std::vector<uint8_t> staging((ys + 2 * cs) * 2 + 2 * u);
  memcpy(staging.data(), y, ys * 2); memcpy(staging.data() + ys * 2, cb, cs * 2); memcpy(staging.data() + (ys + cs) * 2, cr, cs * 2);
  memcpy(staging.data() + (ys + 2 * cs) * 2, qp4, u); memcpy(staging.data() + (ys + 2 * cs) * 2 + u, pm4, u);
  uint8_t* buf = (uint8_t*)rbtk::dev_alloc(staging.size());
  if (!buf) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  struct G { void* p; ~G() { rbtk::dev_free(p); } } g{buf};
  if (rbtk::h2d(buf, staging.data(), staging.size())) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  RbtFrame f; memset(&f, 0, sizeof(f));
  f.cfg.w = w; f.cfg.h = h; Arena::same_planes(f.coef, (int16_t*)buf, ys, cs); f.qp = (int8_t*)(buf + (ys + 2 * cs) * 2); f.pm = buf + (ys + 2 * cs) * 2 + u;
  CensusSet cs1;
  if (cs1.add(f) < 0) { err = "picture cannot be counted"; return RBT_ERR_PARAM; }
  int rc = cs1.upload();
  if (!rc) { cs1.launch(); rc = cs1.fetch(); }
  if (rc) { err = rc == RBT_ERR_NOMEM ? "device allocation failed" : "device transfer failed"; return rc; }
  memcpy(hist, cs1.hist.data(), RBT_RATE_HIST_WORDS * 4);
  return 0;
}

// rbt_picture_sse: the pictures of a, then those of b, then the maps, each block on a multiple of 256 bytes - the rows of a and b are equally far from a 16-byte boundary
int picture_sse_host(std::string& err, const uint16_t* a, const uint16_t* b, int w, int h, int n_frames, const uint16_t* occ, int ow, int oh, uint64_t* out, rbt_stats& st) {
  memset(&st, 0, sizeof(st));
  if (w <= 0 || h <= 0 || w % 2 || h % 2 || w > 8192 || h > 8192 || n_frames < 1) { err = "picture size must be even and at most 8192"; return RBT_ERR_PARAM; }
  if (occ && (ow <= 0 || oh <= 0 || w % ow || h % oh || w / ow != h / oh)) { err = "the occupancy map's scale must be whole and the same in both directions"; return RBT_ERR_PARAM; }
  const size_t ys = (size_t)w * h, cs = (size_t)(w / 2) * (h / 2), fs = ys + 2 * cs, os = occ ? (size_t)ow * oh : 0;
  const size_t blk = (fs * 2 * (size_t)n_frames + 255) & ~(size_t)255;
  std::vector<uint8_t> staging(2 * blk + os * 2 * (size_t)n_frames);
  memcpy(staging.data(), a, fs * 2 * (size_t)n_frames); memcpy(staging.data() + blk, b, fs * 2 * (size_t)n_frames);
  if (occ) memcpy(staging.data() + 2 * blk, occ, os * 2 * (size_t)n_frames);
  uint8_t* buf = (uint8_t*)rbtk::dev_alloc(staging.size());
  if (!buf) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  struct G { void* p; ~G() { rbtk::dev_free(p); } } g{buf};
  if (rbtk::h2d(buf, staging.data(), staging.size())) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  SseSet set;
  for (int k = 0; k < n_frames; k++) {
    RbtSsePic P; memset(&P, 0, sizeof(P));
    const uint16_t* pa = (const uint16_t*)buf + fs * (size_t)k; const uint16_t* pb = (const uint16_t*)(buf + blk) + fs * (size_t)k;
    Arena::same_planes(P.a, pa, ys, cs); Arena::same_planes(P.b, pb, ys, cs);
    P.w = w; P.h = h; P.a_stride = P.b_stride = w;
    if (occ) { P.occ = (const uint16_t*)(buf + 2 * blk) + os * (size_t)k; P.ow = ow; P.scale = w / ow; }
    set.add(P);
  }
  int rc = set.upload();
  if (!rc) { rbtk::timer_begin(T_CENSUS); set.launch(); rbtk::timer_end(T_CENSUS); rc = set.fetch(); }      // (the census timer's events: no census runs inside this call)
  if (rc) { err = rc == RBT_ERR_NOMEM ? "device allocation failed" : "device transfer failed"; return rc; }
  st.gpu_ms = rbtk::timer_ms(T_CENSUS);
  memcpy(out, set.words.data(), set.words.size() * 8);
  return 0;
}

// rbt_ctb_sse: the pictures laid out as picture_sse_host lays them out, the rectangles and the two tables behind them; the words per CTB and, with out_rect, the folded
// triples of every pair of pictures come back
int ctb_sse_host(std::string& err, const uint16_t* a, const uint16_t* b, int w, int h, int n_frames, int log2_ctb, const uint16_t* occ, int ow, int oh, const int32_t* rects, int n_rects,
                 uint64_t* out_ctb, uint64_t* out_rect, rbt_stats& st) {
  memset(&st, 0, sizeof(st));
  if (w <= 0 || h <= 0 || w % 2 || h % 2 || w > 8192 || h > 8192 || n_frames < 1) { err = "picture size must be even and at most 8192"; return RBT_ERR_PARAM; }
  if (occ && (ow <= 0 || oh <= 0 || w % ow || h % oh || w / ow != h / oh)) { err = "the occupancy map's scale must be whole and the same in both directions"; return RBT_ERR_PARAM; }
  if (log2_ctb < 4 || log2_ctb > 6) { err = "log2_ctb must be 4..6"; return RBT_ERR_PARAM; }
  if (n_rects < 0 || (n_rects > 0 && !rects)) { err = "n_rects rectangles need a list"; return RBT_ERR_PARAM; }
  if (out_rect && n_frames % 2) { err = "sums per rectangle are taken over pairs of pictures: n_frames must be even"; return RBT_ERR_PARAM; }
  const int wc = (w + (1 << log2_ctb) - 1) >> log2_ctb, hc = (h + (1 << log2_ctb) - 1) >> log2_ctb;
  for (int k = 0; k < n_rects; k++) {
    const int32_t* r = rects + 4 * k;
    if (r[0] < 0 || r[1] < 0 || r[2] > wc || r[3] > hc || r[0] > r[2] || r[1] > r[3]) { err = "rectangle " + std::to_string(k) + " is outside the grid of " + std::to_string(wc) + " x " + std::to_string(hc) + " CTBs"; return RBT_ERR_PARAM; }
  }
  const size_t ys = (size_t)w * h, cs = (size_t)(w / 2) * (h / 2), fs = ys + 2 * cs, os = occ ? (size_t)ow * oh : 0, nf = (size_t)n_frames, nc = (size_t)wc * hc;
  const size_t n_jobs = out_rect ? nf / 2 : 0, trip = (size_t)n_rects + 2;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t blk = up(fs * 2 * nf), o_occ = 2 * blk, o_rects = up(o_occ + os * 2 * nf), o_pics = up(o_rects + (size_t)n_rects * 16), o_jobs = up(o_pics + nf * sizeof(RbtCtbSsePic));
  const size_t o_ctb = up(o_jobs + n_jobs * sizeof(RbtFoldJob)), o_fold = up(o_ctb + nf * nc * 24), end = o_fold + n_jobs * trip * 24;
  uint8_t* buf = (uint8_t*)rbtk::dev_alloc(end);
  if (!buf) { err = "device allocation failed"; return RBT_ERR_NOMEM; }
  struct G { void* p; ~G() { rbtk::dev_free(p); } } g{buf};
  std::vector<uint8_t> staging(o_ctb, 0);
  memcpy(staging.data(), a, fs * 2 * nf); memcpy(staging.data() + blk, b, fs * 2 * nf);
  if (occ) memcpy(staging.data() + o_occ, occ, os * 2 * nf);
  if (n_rects) memcpy(staging.data() + o_rects, rects, (size_t)n_rects * 16);
  for (size_t k = 0; k < nf; k++) {
    RbtCtbSsePic P; memset(&P, 0, sizeof(P));
    P.a = (const uint16_t*)buf + fs * k; P.b = (const uint16_t*)(buf + blk) + fs * k; P.w = w; P.h = h; P.a_stride = P.b_stride = w;
    if (occ) { P.occ = (const uint16_t*)(buf + o_occ) + os * k; P.ow = ow; P.scale = w / ow; }
    P.log2_ctb = log2_ctb; P.w_ctb = wc; P.h_ctb = hc; P.out = (uint64_t*)(buf + o_ctb) + k * nc * 3;
    memcpy(staging.data() + o_pics + k * sizeof(P), &P, sizeof(P));
  }
  for (size_t f = 0; f < n_jobs; f++) {
    RbtFoldJob J; memset(&J, 0, sizeof(J));
    for (int p = 0; p < 2; p++) J.ctb[p] = (const uint64_t*)(buf + o_ctb) + (2 * f + p) * nc * 3;
    J.rects = (const int32_t*)(buf + o_rects); J.n_rects = n_rects; J.w_ctb = wc; J.h_ctb = hc; J.out = (uint64_t*)(buf + o_fold) + f * trip * 3;
    memcpy(staging.data() + o_jobs + f * sizeof(J), &J, sizeof(J));
  }
  if (rbtk::h2d(buf, staging.data(), staging.size())) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  rbtk::timer_begin(T_CENSUS);      // (the census timer's events: no census runs inside this call)
  rbtk::launch_ctb_sse((const RbtCtbSsePic*)(buf + o_pics), n_frames, (int)nc);
  if (n_jobs) rbtk::launch_patch_fold((const RbtFoldJob*)(buf + o_jobs), (int)n_jobs, n_rects);
  rbtk::timer_end(T_CENSUS);
  if (rbtk::d2h(out_ctb, buf + o_ctb, nf * nc * 24) || (n_jobs && rbtk::d2h(out_rect, buf + o_fold, n_jobs * trip * 24))) { err = "device transfer failed"; return RBT_ERR_NO_DEVICE; }
  st.gpu_ms = rbtk::timer_ms(T_CENSUS);
  return 0;
}

// rbt_rate_estimate: decode, census behind the last filter, table
int rate_estimate(std::string& err, const uint8_t* annexb, size_t n, rbt_rate_table* out) {
  memset(out, 0, sizeof(*out));
  DecodeBatch b; StreamIn in{annexb, n};
  int rc = decode_build(b, &in, 1);
  if (!rc) rc = decode_census_setup(b, std::vector<char>(1, 1));
  if (!rc) rc = decode_launch(b);
  if (!rc) { b.census.launch(); rc = decode_finish(b); }
  if (!rc && b.census.fetch()) { b.err = "device transfer failed"; rc = RBT_ERR_NO_DEVICE; }
  if (rc) { err = b.err; return rc; }
  const int np = b.stream_count[0];
  out->n_pictures = np; out->census_ms = rbtk::timer_ms(T_CENSUS);
  out->hist = (uint32_t*)malloc((size_t)np * RBT_RATE_HIST_WORDS * 4); out->picture_bytes = (uint64_t*)malloc((size_t)np * 8);
  if (!out->hist || !out->picture_bytes) { free(out->hist); free(out->picture_bytes); memset(out, 0, sizeof(*out)); return RBT_ERR_NOMEM; }
  memcpy(out->hist, b.census.hist.data(), (size_t)np * RBT_RATE_HIST_WORDS * 4);
  for (int k = 0; k < np; k++) out->picture_bytes[k] = b.info[b.stream_first[0] + k].vcl_bytes;
  rate_table(out->hist, out->picture_bytes, np, out->estimate);
  return 0;
}

int or_pool_host(const uint16_t* plane, int w, int h, int factor, uint16_t* out) {
  int ow = w / factor, oh = h / factor;
  size_t in_n = (size_t)w * h, out_n = (size_t)ow * oh;
  uint16_t* buf = (uint16_t*)rbtk::dev_alloc((in_n + out_n * 2) * 2);
  if (!buf) return RBT_ERR_NOMEM;
  struct G { void* p; ~G() { rbtk::dev_free(p); } } g{buf};
  if (rbtk::h2d(buf, plane, in_n * 2)) return RBT_ERR_NO_DEVICE;
  rbtk::launch_pool(buf, w, w, h, factor, buf + in_n, buf + in_n + out_n, buf + in_n + out_n + out_n / 4, 0);
  if (rbtk::d2h(out, buf + in_n, out_n * 2)) return RBT_ERR_NO_DEVICE;
  return 0;
}

}  // namespace rbt
