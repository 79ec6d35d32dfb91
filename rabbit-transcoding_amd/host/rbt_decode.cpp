// Decode half of the hot path: replaces initDecoder + the av_read_frame / avcodec_send_packet / avcodec_receive_frame
// loop of PCCTranscoder::transcodeVideo (PCCTranscoder.cpp:404, :428-448).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "rbt_batch.h"

namespace rbt {

size_t frame_samples(const RbtStreamCfg& c) { return (size_t)c.w * c.h + 2 * (size_t)c.cw * c.ch; }

struct DpbEntry { int poc, frame; };

// index lists: slices grouped by level, frames grouped by level
static void build_lists(DecodeBatch& b) {
  std::vector<size_t>& sl_off = b.sl_off; std::vector<size_t>& sl_cnt = b.sl_cnt; sl_off.clear(); sl_cnt.clear();
  std::vector<int32_t>& lists = b.lists_keep; lists.clear(); b.fr_off.clear();
  for (auto& lf : b.level_frames) {
    sl_off.push_back(lists.size());
    for (int fi : lf) for (int k = 0; k < b.frames[fi].n_slices; k++) lists.push_back(b.frames[fi].first_slice + k);
    sl_cnt.push_back(lists.size() - sl_off.back());
  }
  for (auto& lf : b.level_frames) { b.fr_off.push_back(lists.size()); for (int fi : lf) lists.push_back(fi); }
}
static RbtFrameRef frame_ref(const DecodeBatch& b, int fi) { return RbtFrameRef{b.d_frames, b.d_slices, b.d_order + b.order_off[fi], fi, 0}; }

// HBM layout of a decode batch: [zero region | pm region (RBT_MODE_NONE) | ctb_slice region (0xFF) | rest, the rows' hand-over block (zeroed on its own) inside it].
// Every buffer of the arena is named here, once (Arena in rbt_batch.h: run without a base to measure, then over the allocation to bind); returns the extents to fill.
struct DecodeFill { size_t zero_end, pm_begin, pm_end, cs_begin, cs_end, prow_begin, prow_end; };
static DecodeFill decode_lay_out(DecodeBatch& b, Arena& a) {
  DecodeFill m; const size_t nf = b.frames.size(), ns = b.slices.size();
  auto wpp = [&](size_t i) { return b.stream_pps[b.info[i].stream].entropy_coding_sync != 0; };
  for (size_t i = 0; i < nf; i++) { RbtFrame& f = b.frames[i]; const RbtStreamCfg& c = f.cfg; const size_t ys = (size_t)c.w * c.h, cs = (size_t)c.cw * c.ch, u = (size_t)c.w4 * c.h4, nc = (size_t)c.w_ctb * c.h_ctb;
    a.take_planes(f.coef, ys, cs); f.edges = a.take<uint8_t>(u); f.cmd_count = a.take<uint32_t>(nc); f.ctb_done = a.take<uint32_t>(nc * 2); }
  b.d_tickets = a.take<uint32_t>(TICKET_WORDS);
  // ready queues of the reconstruction levels (launch_recon_queue), zeroed with the rest of this region
  size_t queue_words = 0; for (const ReconLevel& lv : b.levels) queue_words += rbtk::recon_queue_words(lv.ctbs);
  uint32_t* d_queue = a.take<uint32_t>(queue_words);
  // wavefront streams: progress counters of the CTB rows (zeroed with the rest of this region)
  for (size_t i = 0; i < nf; i++) if (wpp(i)) b.frames[i].prow_done = a.take<uint32_t>((size_t)b.frames[i].cfg.h_ctb);
  b.d_save = b.want_save ? a.take<uint8_t>(ns * rbtk::parse_save_bytes()) : nullptr;
  m.zero_end = m.pm_begin = a.mark();
  for (size_t i = 0; i < nf; i++) { const RbtStreamCfg& c = b.frames[i].cfg; b.frames[i].pm = a.take<uint8_t>((size_t)c.w4 * c.h4); }
  m.pm_end = m.cs_begin = a.mark();
  for (size_t i = 0; i < nf; i++) { const RbtStreamCfg& c = b.frames[i].cfg; b.frames[i].ctb_slice = a.take<uint16_t>((size_t)c.w_ctb * c.h_ctb); }
  m.cs_end = a.mark();
  for (size_t i = 0; i < nf; i++) {
    RbtFrame& f = b.frames[i]; const RbtStreamCfg& c = f.cfg; const size_t ys = (size_t)c.w * c.h, cs = (size_t)c.cw * c.ch, u = (size_t)c.w4 * c.h4, nc = (size_t)c.w_ctb * c.h_ctb;
    a.take_planes(f.pix, ys, cs);
    if (b.info[i].sao) a.take_planes(f.out, ys, cs); else Arena::same_planes(f.out, f.pix[0], ys, cs);      // no SAO: the deblocked picture is the output
    f.dm = a.take<uint8_t>(u); f.qp = a.take<int8_t>(u); f.mv = a.take<int16_t>(u * 2); f.ref = a.take<int8_t>(u); f.refpoc = a.take<int32_t>(u);
    f.sao = a.take<RbtSao>(nc); f.cmds = a.take<RbtCmd>(nc * (size_t)f.cmd_cap);
  }
  m.prow_begin = a.mark();     // the rows' hand-over records (one block, zeroed per job: recycled pool memory must not pass for the state of a row nobody parsed)
  for (size_t i = 0; i < nf; i++) if (wpp(i)) { RbtFrame& f = b.frames[i]; const size_t rows = (size_t)f.cfg.h_ctb;     // (256 spare bytes each: the records start on a 256-byte address whatever the base)
    f.prow_ctx = Arena::up256(a.take<uint8_t>(rows * 256 + 256)); f.prow_line = Arena::up256(a.take<uint8_t>(rows * f.prow_line_bytes + 256)); }
  m.prow_end = a.mark();
  b.d_frames = a.take<RbtFrame>(nf); b.d_slices = a.take<RbtSlice>(ns);
  b.d_rbsp = a.take<uint8_t>(b.rbsp.size() + 64); b.d_lists = a.take<int32_t>((nf + ns) * 2);
  b.d_order = a.take<uint32_t>(b.order_keep.size()); b.d_refs = a.take<RbtFrameRef>(nf);
  a.mark();
  if (a.base) { size_t r = 0, q = 0;      // the levels' launches: their share of the lists, the refs, the queue memory and the tickets
    for (size_t l = 0; l < b.levels.size(); l++) { ReconLevel& lv = b.levels[l];
      lv.frames = b.d_frames; lv.slices = b.d_slices; lv.list = b.d_lists + b.fr_off[l]; lv.refs = b.d_refs + r; lv.queue = d_queue + q; lv.ticket = b.d_tickets + TICKET_OWN_LEVEL + l;
      r += (size_t)lv.n; q += rbtk::recon_queue_words(lv.ctbs); } }
  return m;
}

int decode_build(DecodeBatch& b, const StreamIn* streams, int n_streams) {
  b.stream_first.assign(n_streams, 0); b.stream_count.assign(n_streams, 0);
  b.stream_sps.resize(n_streams); b.stream_pps.resize(n_streams);
  // ---- host parse ----
  for (int si = 0; si < n_streams; si++) {
    std::vector<Nal> nals; split_annexb(streams[si].p, streams[si].n, b.rbsp, nals);
    ParamSets* ps = new ParamSets();
    std::vector<DpbEntry> dpb; int prev_tid0_poc = 0, cur = -1;
    SliceHdr head_hdr; int head_idx = -1, last_seg = -1;   // the independent segment of the current slice, the last segment of its chain
    b.stream_first[si] = (int)b.frames.size();
    for (const Nal& nal : nals) {
      const uint8_t* r = b.rbsp.data() + nal.rbsp_off; int rc = 0;
      if (nal.type == NAL_SPS) rc = parse_sps(*ps, r, nal.rbsp_size, b.err);
      else if (nal.type == NAL_PPS) rc = parse_pps(*ps, r, nal.rbsp_size, b.err);
      else if (nal.type == NAL_SEI_SUFFIX) { if (cur >= 0) { FrameInfo& fi = b.info[cur]; uint8_t hh[48]; if (int k = parse_hash_sei(r, nal.rbsp_size, hh)) { fi.hash_kind = k; memcpy(fi.hash, hh, 48); } } }
      else if (nal.type <= NAL_TRAIL_R || (nal.type >= 16 && nal.type <= 21)) {
        SliceHdr h; rc = parse_slice_header(*ps, r, nal.rbsp_size, nal.type, h, b.err, head_idx >= 0 ? &head_hdr : nullptr);
        if (rc) { delete ps; b.err_code = rc == -3 ? RBT_ERR_UNSUPPORTED : RBT_ERR_BITSTREAM; return b.err_code; }
        const Pps& pps = ps->pps[h.pps_id]; const Sps& sps = ps->sps[pps.sps_id];
        if (h.first_slice_in_pic) {
          h.poc = slice_poc(sps, nal.type, h.poc_lsb, prev_tid0_poc);
          RbtFrame f; memset(&f, 0, sizeof(f));
          fill_stream_cfg(sps, pps, f.cfg); f.poc = h.poc; f.first_slice = (int)b.slices.size();
          int ctb = 1 << sps.log2_ctb; f.cmd_cap = 2 * (ctb / 4) * (ctb / 4);
          if (b.stream_count[si] > 0 && memcmp(&b.frames[b.stream_first[si]].cfg, &f.cfg, sizeof(f.cfg)) != 0) {
            // parameter sets may be repeated but must not change inside one sub-bitstream of a GOF
            const RbtStreamCfg& c0 = b.frames[b.stream_first[si]].cfg;
            if (c0.w != f.cfg.w || c0.h != f.cfg.h || c0.bit_depth != f.cfg.bit_depth) { delete ps; b.err = "picture size changes inside a stream"; return b.err_code = RBT_ERR_UNSUPPORTED; }
          }
          cur = (int)b.frames.size(); b.frames.push_back(f);
          FrameInfo fi; memset(&fi, 0, sizeof(fi)); fi.stream = si; fi.nal_type = nal.type; b.info.push_back(fi);
          b.stream_count[si]++; b.stream_sps[si] = sps; b.stream_pps[si] = pps;
          dpb.insert(dpb.begin(), DpbEntry{h.poc, cur});
          head_idx = -1;
        } else if (cur < 0) { delete ps; b.err = "slice segment before the first picture"; return b.err_code = RBT_ERR_BITSTREAM; }
        else h.poc = b.frames[cur].poc;
        // slice segments of a picture come in increasing address order (7.4.7.1), the first one at 0: with that, segment i has to cover exactly the CTBs up to the
        // start of segment i + 1 (RbtSlice::end_addr, checked by the parser where the segment ends) - no overlap, no hole, nothing for a row task to wait for in vain
        { const int n_ctb = sps.w_ctb * sps.h_ctb, prev = b.frames[cur].n_slices ? b.slices.back().ctb_addr : -1;
          if ((int)h.segment_addr <= prev || (int)h.segment_addr >= n_ctb || (prev < 0 && h.segment_addr != 0)) { delete ps; b.err = "slice segment address out of order"; return b.err_code = RBT_ERR_BITSTREAM; }
          if (prev >= 0) b.slices.back().end_addr = (int32_t)h.segment_addr; }
        b.info[cur].vcl_bytes += nal.rbsp_size + nal.epb.size();
        RbtSlice s; memset(&s, 0, sizeof(s));
        s.frame = cur; s.data_off = (uint32_t)(nal.rbsp_off + h.data_byte_offset);
        if (h.data_byte_offset > nal.rbsp_size) { delete ps; b.err = "empty slice data"; return b.err_code = RBT_ERR_BITSTREAM; }
        s.data_size = (uint32_t)(nal.rbsp_size - h.data_byte_offset); s.ctb_addr = h.segment_addr;
        s.slice_type = (int8_t)h.slice_type; s.qp = (int8_t)h.qp; s.cb_qp_offset = (int8_t)h.cb_qp_offset; s.cr_qp_offset = (int8_t)h.cr_qp_offset;
        s.sao_luma = (uint8_t)h.sao_luma; s.sao_chroma = (uint8_t)h.sao_chroma; s.deblocking_disabled = (uint8_t)h.deblocking_disabled; s.lf_across = (uint8_t)h.lf_across;
        s.beta_offset_div2 = (int8_t)h.beta_offset_div2; s.tc_offset_div2 = (int8_t)h.tc_offset_div2; s.temporal_mvp = (uint8_t)h.temporal_mvp;
        s.cabac_init_flag = (uint8_t)h.cabac_init_flag; s.max_merge_cand = (uint8_t)h.max_merge_cand; s.num_ref_idx = (uint8_t)h.num_ref_idx;
        s.collocated_ref_idx = (uint8_t)h.collocated_ref_idx; s.poc = h.poc;
        if (h.slice_type == RBT_SLICE_P && h.wp_on) {
          s.wp_on = 1; s.wp_shift[0] = (int8_t)(h.wp_luma_denom + 14 - sps.bit_depth); s.wp_shift[1] = (int8_t)(h.wp_chroma_denom + 14 - sps.bit_depth);
          for (int i = 0; i < h.num_ref_idx && i < RBT_MAX_REFS; i++) for (int c = 0; c < 3; c++) { s.wp_w[i][c] = (int16_t)h.wp_w[i][c]; s.wp_o[i][c] = (int16_t)(h.wp_o[i][c] * (1 << (sps.bit_depth - 8))); }
        }
        if (h.qp < -6 * (sps.bit_depth - 8) || h.qp > 51) { delete ps; b.err = "slice QP out of range"; return b.err_code = RBT_ERR_BITSTREAM; }
        if (h.slice_type == RBT_SLICE_P) {
          int cand[16], nc = 0;
          for (int i = 0; i < h.rps.num; i++) if (h.rps.used[i]) cand[nc++] = h.poc + h.rps.delta_poc[i];
          if (!nc) { delete ps; b.err = "P slice with an empty reference picture set"; return b.err_code = RBT_ERR_BITSTREAM; }
          for (int i = 0; i < h.num_ref_idx; i++) {
            int poc = cand[i % nc], found = -1;
            for (size_t k = 1; k < dpb.size(); k++) if (dpb[k].poc == poc) { found = dpb[k].frame; break; }   // dpb[0] is the current picture
            if (found < 0) { delete ps; b.err = "missing reference picture"; return b.err_code = RBT_ERR_BITSTREAM; }
            s.ref_frame[i] = found; s.ref_poc[i] = poc;
            b.frames[cur].level = std::max(b.frames[cur].level, b.frames[found].level + 1);
            if (h.temporal_mvp && i == h.collocated_ref_idx && b.frames[found].level > 0) b.ordered_parse = true;
          }
        }
        if (h.sao_luma || h.sao_chroma) b.info[cur].sao = true;
        s.wpp = (uint8_t)pps.entropy_coding_sync; s.next_seg = -1; s.head = (int32_t)b.slices.size();
        // a segment of a wavefront stream that starts a CTB row gets a wave of its own (it takes what it needs of the row above from that row's wave:
        // rbt_parse.h); RBT_WPP_PARALLEL=0 keeps one wave per slice
        static const int row_tasks = [] { const char* e = getenv("RBT_WPP_PARALLEL"); return !e || atoi(e) != 0; }();
        s.row_task = (uint8_t)(pps.entropy_coding_sync && row_tasks && h.dependent && h.segment_addr % sps.w_ctb == 0);   // (an independent segment needs nothing of the row above: it is a wave of its own anyway)
        if (s.row_task) b.has_row_tasks = true;
        if (h.dependent) {
          // same slice as the segment before it: parsed by the wave that parsed that one (next_seg chain) unless it starts a row of a wavefront stream
          if (head_idx < 0 || last_seg < 0) { delete ps; b.err = "dependent slice segment without a slice"; return b.err_code = RBT_ERR_BITSTREAM; }
          s.dependent = 1; s.head = head_idx;
          if (!s.row_task) b.slices[last_seg].next_seg = (int32_t)b.slices.size();
        } else { head_hdr = h; head_idx = (int)b.slices.size(); }
        last_seg = (int)b.slices.size();
        b.frames[cur].n_slices++;
        // A segment of a wavefront stream that spans several CTB rows names its substreams by entry points (x265's form): every substream after the first starts
        // a row and becomes a row task of its own. The offsets count bytes AS SENT (emulation prevention bytes included, 7.4.7.1): mapped through the
        // positions where such bytes were removed. Offsets that do not add up leave the segment to one wave, which finds the rows by itself.
        std::vector<RbtSlice> rows;
        if (s.wpp && row_tasks && !h.entry_sizes.empty()) {
          auto sent_to_rbsp = [&](size_t e) { size_t k = 0; while (k < nal.epb.size() && nal.epb[k] < e) k++; return e - k; };   // offset in the NAL as sent -> offset in its RBSP
          size_t e0 = h.data_byte_offset; { size_t k = 0; while (k < nal.epb.size() && (size_t)nal.epb[k] - k < h.data_byte_offset) k++; e0 += k; }
          const int wc = sps.w_ctb, first_row_ctbs = wc - h.segment_addr % wc; bool ok = true;
          std::vector<size_t> u(1, h.data_byte_offset); size_t e = e0;
          for (uint32_t sz : h.entry_sizes) { e += sz; const size_t x = sent_to_rbsp(e); if (x <= u.back() || x >= nal.rbsp_size) { ok = false; break; } u.push_back(x); }
          if (ok && (size_t)h.segment_addr + first_row_ctbs + (h.entry_sizes.size() - 1) * (size_t)wc < (size_t)wc * sps.h_ctb) {
            s.data_size = (uint32_t)(u[1] - u[0]); s.ctb_limit = first_row_ctbs; s.end_addr = (int32_t)h.segment_addr + first_row_ctbs;
            for (size_t i = 1; i < u.size(); i++) {
              RbtSlice t = s; t.dependent = 1; t.row_task = 1; t.next_seg = -1; t.head = s.head;
              t.ctb_addr = h.segment_addr + first_row_ctbs + (int)(i - 1) * wc;
              t.data_off = (uint32_t)(nal.rbsp_off + u[i]); t.data_size = (uint32_t)((i + 1 < u.size() ? u[i + 1] : nal.rbsp_size) - u[i]);
              t.ctb_limit = i + 1 < u.size() ? wc : 0;               // the last substream ends with the segment
              t.end_addr = t.ctb_limit ? t.ctb_addr + wc : 0;        // (the last one: where the next segment starts, filled in when that is known)
              rows.push_back(t);
            }
            b.has_row_tasks = true;
          }
        }
        b.slices.push_back(s);
        for (const RbtSlice& t : rows) { last_seg = (int)b.slices.size(); b.frames[cur].n_slices++; b.slices.push_back(t); }
      } else if (nal.type >= 2 && nal.type <= 9) { rc = -3; b.err = "unsupported VCL NAL unit type"; }
      if (rc) { delete ps; b.err_code = rc == -3 ? RBT_ERR_UNSUPPORTED : RBT_ERR_BITSTREAM; return b.err_code; }
    }
    delete ps;
  }
  if (b.frames.empty()) { b.err = "no pictures in the input"; return b.err_code = RBT_ERR_BITSTREAM; }
  for (size_t i = 0; i < b.slices.size(); i++) if (!b.slices[i].end_addr) { const RbtStreamCfg& c = b.frames[b.slices[i].frame].cfg; b.slices[i].end_addr = c.w_ctb * c.h_ctb; }   // the last entry of a picture ends with the picture
  if (b.has_row_tasks) b.want_save = false;                              // banded (resumable) parsing re-launches the list; row tasks need one ordered launch
  if (b.slices.size() >= 0xFFFF) { b.err = "too many slice segments"; return b.err_code = RBT_ERR_UNSUPPORTED; }
  // flat chroma: what the headers decide. The distinct reference pictures of a picture's slices, whose chroma_flat words its reconstruction reads; never
  // flat under constrained intra prediction, with explicit weights in any slice, with more references than flat_ref holds, or where the reconstruction starts before the
  // parse is complete (banded parse: d_save)
  for (size_t i = 0; i < b.frames.size(); i++) { RbtFrame& f = b.frames[i];
    f.chroma_seen = f.chroma_flat = 0; f.chroma_unknown = f.cfg.cip || b.want_save; for (int k = 0; k < RBT_MAX_REFS; k++) f.flat_ref[k] = -1;
    for (int k = 0; k < f.n_slices; k++) { const RbtSlice& s = b.slices[(size_t)f.first_slice + k];
      if (s.wp_on) f.chroma_unknown = 1;
      for (int r = 0; s.slice_type != RBT_SLICE_I && r < s.num_ref_idx; r++) {
        if (r >= RBT_MAX_REFS) { f.chroma_unknown = 1; break; }
        int q = 0; while (q < RBT_MAX_REFS && f.flat_ref[q] >= 0 && f.flat_ref[q] != s.ref_frame[r]) q++;
        if (q == RBT_MAX_REFS) f.chroma_unknown = 1; else f.flat_ref[q] = s.ref_frame[r]; } } }
  int n_levels = 0; for (auto& f : b.frames) n_levels = std::max(n_levels, f.level + 1);
  b.level_frames.assign(n_levels, {});
  for (size_t i = 0; i < b.frames.size(); i++) b.level_frames[b.frames[i].level].push_back((int)i);
  if (b.level_frames.size() > MAX_LEVELS) { b.err = "too many dependency levels"; return b.err_code = RBT_ERR_UNSUPPORTED; }
  for (size_t i = 0; i < b.frames.size(); i++) if (b.stream_pps[b.info[i].stream].entropy_coding_sync) {   // wavefront streams: the rows hand their bottom lines down (decode_lay_out)
    const RbtStreamCfg& c = b.frames[i].cfg; b.frames[i].prow_line_bytes = (int32_t)(((size_t)c.w4 * 7 + (size_t)c.w_ctb * (2 + sizeof(RbtSao)) + 255) & ~(size_t)255); }
  build_lists(b); b.levels.clear();
  for (auto& lf : b.level_frames) { std::vector<LevelPic> pics; for (int fi : lf) pics.push_back(LevelPic{&b, fi}); b.levels.push_back(recon_level_of(pics)); }
  // CTB dependency order (anti-diagonals x + 2y ascending, top to bottom inside one) per distinct picture geometry
  const size_t nf = b.frames.size();
  b.order_keep.clear(); b.order_off.assign(nf, 0);
  { std::vector<std::pair<std::pair<int, int>, size_t>> seen;
    for (size_t i = 0; i < nf; i++) { const int w = b.frames[i].cfg.w_ctb, h = b.frames[i].cfg.h_ctb; const std::pair<std::pair<int, int>, size_t>* old = nullptr;
      for (auto& s_ : seen) if (s_.first == std::make_pair(w, h)) old = &s_;
      if (!old) { seen.push_back({{w, h}, b.order_keep.size()}); old = &seen.back();
        for (int d = 0; d <= w - 1 + 2 * (h - 1); d++) for (int y = 0; y < h; y++) { int x = d - 2 * y; if (x >= 0 && x < w) b.order_keep.push_back((uint32_t)x | ((uint32_t)y << 16)); } }
      b.order_off[i] = old->second; } }
  Arena a; decode_lay_out(b, a);      // measure, allocate, bind
  b.arena_size = a.used; b.arena = rbtk::dev_alloc(b.arena_size);
  if (!b.arena) { b.err = "device allocation failed"; return b.err_code = RBT_ERR_NOMEM; }
  uint8_t* base = (uint8_t*)b.arena; a = Arena{base};
  const DecodeFill m = decode_lay_out(b, a);
  // the pictures of every level as RbtFrameRef, in the order of the levels (ReconLevel::refs of level l starts where the levels before it end)
  b.refs_keep.clear(); for (auto& lf : b.level_frames) for (int fi : lf) b.refs_keep.push_back(frame_ref(b, fi));
  if (rbtk::dev_memset(base, 0, m.zero_end) || (m.prow_end > m.prow_begin && rbtk::dev_memset(base + m.prow_begin, 0, m.prow_end - m.prow_begin)) || rbtk::dev_memset(base + m.pm_begin, RBT_MODE_NONE, m.pm_end - m.pm_begin) || rbtk::dev_memset(base + m.cs_begin, 0xFF, m.cs_end - m.cs_begin) ||
      rbtk::h2d(b.d_frames, b.frames.data(), nf * sizeof(RbtFrame)) || rbtk::h2d(b.d_slices, b.slices.data(), b.slices.size() * sizeof(RbtSlice)) ||
      rbtk::h2d(b.d_rbsp, b.rbsp.data(), b.rbsp.size()) || rbtk::h2d(b.d_order, b.order_keep.data(), b.order_keep.size() * 4) ||
      rbtk::h2d(b.d_refs, b.refs_keep.data(), b.refs_keep.size() * sizeof(RbtFrameRef))) { b.err = "device transfer failed"; return b.err_code = RBT_ERR_NO_DEVICE; }
  return 0;
}

// Reconstruction of a dependency level: one launch with CTB-to-CTB done flags (launch_recon_level), or one launch per anti-diagonal.
// Measured on MI355X (HM-like 32-frame GOF): the flag kernel shortens the level itself by 13-19 % (blocking call 352.1 -> 349.3 ms, reconstruction 64 -> 52 ms per job),
// but with 16 GOFs in flight its resident waiting workgroups hold LDS and wave slots the other jobs' analysis / intra-coding kernels need (those go from 25-27 / 31 ms
// to 40 / 49 ms per job): 598 against 635 frames/s. So: flags while few jobs are in flight (<= 4: the GPU is mostly idle), diagonals beyond.
// RBT_RECON_DIAG=1 / RBT_RECON_LEVEL=1 force one or the other.
void recon_set_depth(int depth) { rbtk::set_jobs_in_flight(depth); }      // kept with the device (rbt_kernels.hip Dev): contexts on different devices do not share it
// Round 4: one launch per level with a device-side READY queue (launch_recon_queue): a few persistent workgroups - about as many as the level's wavefronts are wide -
// take CTBs in the order they become ready. RBT_RECON_QUEUE=1 / =0 forces it on / off.
int recon_mode() {
  static int force = -1;
  if (force < 0) { const char* d = getenv("RBT_RECON_DIAG"); const char* l = getenv("RBT_RECON_LEVEL"); const char* q = getenv("RBT_RECON_QUEUE");
                   force = d && atoi(d) ? 1 : (l && atoi(l) ? 2 : (q && *q ? (atoi(q) ? 3 : 4) : 0)); }
  if (force == 1) return 0;
  if (force == 2) return 1;
  if (force == 3) return 2;
  return rbtk::jobs_in_flight() > 4 ? 0 : 1;                     // (force 4: the queue off, the round-3 rule)
}
static int recon_queue_width(const RbtStreamCfg& c) { const int w = c.w_ctb, h = c.h_ctb, d = w + 2 * h - 2; return d > 0 ? std::max(1, (w * h + d - 1) / d) : 1; }   // CTBs of a picture that can be reconstructed side by side, on average (workgroups the ready-queue launch gets per picture)
ReconLevel recon_level_of(const std::vector<LevelPic>& pics, std::vector<RbtFrameRef>* refs) {
  ReconLevel lv; lv.n = (int)pics.size();
  for (const LevelPic& p : pics) { const RbtStreamCfg& c = p.b->frames[p.frame].cfg;
    lv.w_ctb = std::max(lv.w_ctb, (int)c.w_ctb); lv.h_ctb = std::max(lv.h_ctb, (int)c.h_ctb); lv.ctbs += (uint32_t)(c.w_ctb * c.h_ctb); lv.queue_wgs += recon_queue_width(c);
    if (refs) refs->push_back(frame_ref(*p.b, p.frame)); }
  return lv;
}
int recon_mode_for(const ReconLevel* lv, size_t n) {
  int mode = recon_mode();
  for (size_t l = 0; l < n && mode == 2; l++) if (lv[l].n >= 8192 || (size_t)lv[l].w_ctb * lv[l].h_ctb >= ((size_t)1 << 18)) mode = 0;
  return mode;
}
// A batch's own level goes by its frame list when it goes by diagonals (the kernel bench.py's depth runs), levels merged across batches have refs only.
void launch_recon(const ReconLevel& lv, int mode) {
  if (mode == 0 && lv.list) rbtk::launch_recon(lv.frames, lv.slices, lv.list, lv.n, lv.w_ctb, lv.h_ctb);
  else if (mode == 0) rbtk::launch_recon_refs(lv.refs, lv.n, lv.w_ctb, lv.h_ctb);
  else if (mode == 1) rbtk::launch_recon_level(lv.refs, lv.n, lv.w_ctb * lv.h_ctb, lv.ticket);
  else rbtk::launch_recon_queue(lv.refs, lv.n, lv.ctbs, lv.queue, lv.queue_wgs);
}

int decode_run(DecodeBatch& b) { int rc = decode_launch(b); return rc ? rc : decode_finish(b); }

int decode_launch(DecodeBatch& b) {
  int rc = decode_launch_parse(b);
  if (rc) return rc;
  rbtk::timer_begin(T_RECON);
  for (size_t l = 0; l < b.level_frames.size(); l++) decode_launch_level(b, l);
  rbtk::timer_end(T_RECON);
  return 0;
}
int decode_max_w4(const DecodeBatch& b) { int m = 0; for (auto& f : b.frames) m = std::max(m, (int)f.cfg.w4); return m; }
int decode_upload_lists(DecodeBatch& b) {
  if (b.lists_uploaded) return 0;
  b.lists_uploaded = true;
  if (b.lists_keep.size() > (b.frames.size() + b.slices.size()) * 2) { b.err = "internal: list overflow"; return b.err_code = RBT_ERR_PARAM; }
  if (rbtk::h2d(b.d_lists, b.lists_keep.data(), b.lists_keep.size() * sizeof(int32_t))) { b.err = "device transfer failed"; return b.err_code = RBT_ERR_NO_DEVICE; }
  return 0;
}
int decode_launch_parse(DecodeBatch& b) {
  int rc = decode_upload_lists(b);
  if (rc) return rc;
  if (b.parse_external) return 0;
  const std::vector<size_t>& sl_off = b.sl_off; const std::vector<size_t>& sl_cnt = b.sl_cnt;
  rbtk::timer_begin(T_PARSE);
  uint32_t* tk = b.has_row_tasks ? b.d_tickets + TICKET_PARSE : nullptr;          // row tasks wait for earlier list entries: hand the list out in start order
  if (b.ordered_parse) { for (size_t l = 0; l < b.level_frames.size(); l++) rbtk::launch_parse(b.d_frames, b.d_slices, b.d_rbsp, b.d_lists + sl_off[l], (int)sl_cnt[l], decode_max_w4(b), nullptr, 0, tk ? tk + l : nullptr); }
  else rbtk::launch_parse(b.d_frames, b.d_slices, b.d_rbsp, b.d_lists, (int)b.slices.size(), decode_max_w4(b), nullptr, 0, tk);
  rbtk::timer_end(T_PARSE);
  return 0;
}
void decode_launch_filters(DecodeBatch& b, size_t l) {
  const std::vector<int>& lf = b.level_frames[l];
  int mu = 0, ml = 0, mc = 0;
  for (int fi : lf) { const RbtStreamCfg& c = b.frames[fi].cfg; mu = std::max(mu, c.w4 * c.h4); ml = std::max(ml, c.w * c.h); mc = std::max(mc, c.w_ctb * c.h_ctb); }
  // SAO: one workgroup per CTB (round 4: a third of the per-sample kernel's instructions); RBT_SAO_PER_SAMPLE=1 keeps the round-1 form
  static const int sao_per_sample = [] { const char* e = getenv("RBT_SAO_PER_SAMPLE"); return e && atoi(e) != 0; }();
  // Deblocking in place, one launch per edge direction, then SAO from `pix` to `out`. RBT_FUSED_LF=1 (round 3) gives pictures with SAO ONE launch through LDS tiles instead
  // (rbt_loopfilter_tile: one read of the reconstruction, one write of the output; same samples): 1-2 % faster for a lone GOF, 3-6 % slower with 16+ GOFs in flight, where the
  // kernels queue for LDS (the reconstruction holds a CTB there) and the LDS-free filter launches fill the gaps - measured in tools/lf_probe.sh, so it is off by default.
  // Runs of pictures with / without SAO inside the level's list get their own launches.
  static const int fused = [] { const char* e = getenv("RBT_FUSED_LF"); return e && atoi(e) != 0; }();
  size_t k = 0;
  while (k < lf.size()) {
    const bool sao = b.info[lf[k]].sao;
    size_t e = k; while (e < lf.size() && b.info[lf[e]].sao == sao) e++;
    int mw_ = 0, mh_ = 0; for (size_t q = k; q < e; q++) { mw_ = std::max(mw_, (int)b.frames[lf[q]].cfg.w); mh_ = std::max(mh_, (int)b.frames[lf[q]].cfg.h); }
    if (sao && fused) rbtk::launch_loopfilter(b.d_frames, b.d_slices, b.d_lists + b.fr_off[l] + k, (int)(e - k), mw_, mh_);
    else {
      rbtk::launch_deblock(b.d_frames, b.d_slices, b.d_lists + b.fr_off[l] + k, (int)(e - k), mu);
      if (sao && sao_per_sample) rbtk::launch_sao(b.d_frames, b.d_slices, b.d_lists + b.fr_off[l] + k, (int)(e - k), ml);
      else if (sao) rbtk::launch_sao_ctb(b.d_frames, b.d_slices, b.d_lists + b.fr_off[l] + k, (int)(e - k), mc);
    }
    k = e;
  }
}
int decode_launch_chunked(DecodeBatch& b, int chunks, int main_stream, int aux_stream) {
  int rc = decode_upload_lists(b);
  if (rc) return rc;
  const std::vector<int>& lf = b.level_frames[0];
  int mw = 0, mh = 0, max_h_all = 0;
  for (int fi : lf) { const RbtStreamCfg& c = b.frames[fi].cfg; mw = std::max(mw, c.w_ctb); mh = std::max(mh, c.h_ctb); }
  for (auto& f : b.frames) max_h_all = std::max(max_h_all, (int)f.cfg.h_ctb);
  rbtk::timer_begin(T_PARSE);
  int y_prev = 0;
  for (int c = 0; c < chunks; c++) {
    int y_lim = c + 1 == chunks ? (1 << 30) : (max_h_all * (c + 1) + chunks - 1) / chunks;
    rbtk::set_stream(main_stream);
    rbtk::launch_parse(b.d_frames, b.d_slices, b.d_rbsp, b.d_lists, (int)b.slices.size(), decode_max_w4(b), b.d_save, y_lim);
    if (c + 1 == chunks) rbtk::timer_end(T_PARSE);
    rbtk::stream_wait(aux_stream, main_stream);
    rbtk::set_stream(aux_stream);
    rbtk::launch_recon(b.d_frames, b.d_slices, b.d_lists + b.fr_off[0], (int)lf.size(), mw, mh, y_prev, y_lim);
    y_prev = y_lim;
  }
  rbtk::set_stream(main_stream);
  rbtk::stream_wait(main_stream, aux_stream);
  decode_launch_filters(b, 0);
  return 0;
}
void decode_launch_level(DecodeBatch& b, size_t l) {
  launch_recon(b.levels[l], recon_mode_for(&b.levels[l], 1));
  decode_launch_filters(b, l);
}

int decode_finish(DecodeBatch& b) {
  size_t nf = b.frames.size();
  if (rbtk::dev_sync()) { b.err = "kernel execution failed"; return b.err_code = RBT_ERR_NO_DEVICE; }
  // per-picture error words and slice coverage
  std::vector<RbtFrame> fr(nf);
  if (rbtk::d2h(fr.data(), b.d_frames, nf * sizeof(RbtFrame))) { b.err = "device transfer failed"; return b.err_code = RBT_ERR_NO_DEVICE; }
  b.n_flat = 0; for (size_t i = 0; i < nf; i++) b.n_flat += fr[i].chroma_flat != 0;
  for (size_t i = 0; i < nf; i++) if (fr[i].error) { b.err = "slice data decoding failed (code " + std::to_string(fr[i].error) + ")"; return b.err_code = RBT_ERR_BITSTREAM; }
  // every CTB of every picture must have been decoded by exactly one slice segment (a truncated stream leaves pictures with holes)
  std::vector<RbtSlice> sl(b.slices.size());
  if (rbtk::d2h(sl.data(), b.d_slices, sl.size() * sizeof(RbtSlice))) { b.err = "device transfer failed"; return b.err_code = RBT_ERR_NO_DEVICE; }
  std::vector<uint64_t> covered(nf, 0);
  for (auto& s_ : sl) covered[(size_t)s_.frame] += s_.n_ctbs_decoded;
  for (size_t i = 0; i < nf; i++) if (covered[i] != (uint64_t)b.frames[i].cfg.w_ctb * b.frames[i].cfg.h_ctb) { b.err = "picture " + std::to_string(i) + " is not completely covered by slice data"; return b.err_code = RBT_ERR_BITSTREAM; }
  return 0;
}

int decode_fetch(DecodeBatch& b, int stream, rbt_video* out) {
  memset(out, 0, sizeof(*out));
  int first = b.stream_first[stream], n = b.stream_count[stream];
  if (n <= 0) return RBT_ERR_BITSTREAM;
  const RbtStreamCfg& c = b.frames[first].cfg; const Sps& sps = b.stream_sps[stream];
  // output = coded picture minus the conformance window (7.4.3.2.1)
  const int cl = 2 * sps.conf_win[0], ct = 2 * sps.conf_win[2], dw = c.w - cl - 2 * sps.conf_win[1], dh = c.h - ct - 2 * sps.conf_win[3];
  if (dw <= 0 || dh <= 0) return RBT_ERR_BITSTREAM;
  const bool crop = dw != c.w || dh != c.h;
  size_t fs = frame_samples(c), ofs = (size_t)dw * dh + 2 * (size_t)(dw / 2) * (dh / 2);
  out->width = dw; out->height = dh; out->bit_depth = c.bit_depth; out->n_frames = n;
  out->data = (uint16_t*)malloc(ofs * 2 * (size_t)n);
  if (!out->data) return RBT_ERR_NOMEM;
  std::vector<uint16_t> full(crop ? fs : 0);
  for (int i = 0; i < n; i++) {
    const RbtFrame& f = b.frames[first + i];
    uint16_t* dst = out->data + ofs * (size_t)i;
    uint16_t* p = crop ? full.data() : dst;
    if (rbtk::d2h(p, f.out[0], fs * 2)) return RBT_ERR_NO_DEVICE;
    if (crop) {
      const uint16_t* src = p; uint16_t* d = dst;
      for (int k = 0; k < 3; k++) { const int sh = k ? 1 : 0, pw = c.w >> sh, ph = c.h >> sh, ow = dw >> sh, oh = dh >> sh;
        for (int y = 0; y < oh; y++) memcpy(d + (size_t)y * ow, src + (size_t)(y + (ct >> sh)) * pw + (cl >> sh), (size_t)ow * 2);
        src += (size_t)pw * ph; d += (size_t)ow * oh; }
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ decoded picture hashes (verify_md5)
// The hash covers the whole coded picture (the decoder's out planes), whichever kind the picture's SEI names.
int decode_hash_setup(DecodeBatch& b, const std::vector<char>& verify) {
  const int ns = (int)b.stream_first.size();
  b.hash_checked.assign(ns, 0); b.hash.n_counters = ns;
  for (int si = 0; si < ns && si < (int)verify.size(); si++) if (verify[si])
    for (int k = 0; k < b.stream_count[si]; k++) {
      const int fi = b.stream_first[si] + k; const FrameInfo& in = b.info[fi]; const RbtFrame& f = b.frames[fi];
      if (!in.hash_kind) continue;
      if (b.hash.add(f.out, f.cfg.w, f.cfg.h, f.cfg.bit_depth, in.hash_kind, si, in.hash) < 0) { b.err = "picture cannot be hashed"; return b.err_code = RBT_ERR_UNSUPPORTED; }
      b.hash_checked[si]++;
    }
  if (b.hash.empty()) return 0;
  if (b.hash.upload()) { b.err = "device allocation failed"; return b.err_code = RBT_ERR_NOMEM; }
  return 0;
}
void decode_launch_hash(const DecodeBatch& b) { if (!b.hash.empty()) b.hash.launch(); }
void decode_hash_result(const DecodeBatch& b, int stream, int& checked, int& failed) {
  checked = stream < (int)b.hash_checked.size() ? b.hash_checked[stream] : 0;
  failed = checked && stream < (int)b.hash.counters.size() ? (int)b.hash.counters[stream] : 0;
}

// ------------------------------------------------------------------------------------------------ level census (rate targets)
int decode_census_setup(DecodeBatch& b, const std::vector<char>& want) {
  const int ns = (int)b.stream_first.size();
  b.census_first.assign(ns, -1);
  for (int si = 0; si < ns && si < (int)want.size(); si++) if (want[si])
    for (int k = 0; k < b.stream_count[si]; k++) {
      const int at = b.census.add(b.frames[b.stream_first[si] + k]);
      if (at < 0) { b.err = "picture size is not a multiple of 8"; return b.err_code = RBT_ERR_UNSUPPORTED; }
      if (k == 0) b.census_first[si] = at;
    }
  if (b.census.empty()) return 0;
  if (int rc = b.census.upload()) { b.err = rc == RBT_ERR_NOMEM ? "device allocation failed" : "device transfer failed"; return b.err_code = rc; }
  return 0;
}
int CensusSet::add(const RbtFrame& f) {
  if (f.cfg.w <= 0 || f.cfg.h <= 0 || (f.cfg.w | f.cfg.h) & 7) return -1;
  RbtCensusPic P; memset(&P, 0, sizeof(P));
  for (int c = 0; c < 3; c++) { if ((uintptr_t)f.coef[c] & 7) return -1; P.coef[c] = f.coef[c]; }   // the kernel reads 8 bytes at a time
  P.qp = f.qp; P.pm = f.pm; P.w = f.cfg.w; P.h = f.cfg.h;
  max_words = std::max(max_words, RBT_RATE_PIC_WORDS(P.w, P.h));
  pics.push_back(P);
  return (int)pics.size() - 1;
}
int CensusSet::upload() {
  const size_t n = pics.size();
  o_hist = (n * sizeof(RbtCensusPic) + 255) & ~(size_t)255;
  const size_t end = o_hist + n * RBT_RATE_HIST_WORDS * 4;
  rbtk::dev_free(d);
  d = (uint8_t*)rbtk::dev_alloc(end);
  if (!d) return RBT_ERR_NOMEM;
  for (size_t i = 0; i < n; i++) pics[i].hist = (uint32_t*)(d + o_hist) + i * RBT_RATE_HIST_WORDS;
  staging.assign(end, 0);
  memcpy(staging.data(), pics.data(), n * sizeof(RbtCensusPic));
  return rbtk::h2d(d, staging.data(), end) ? RBT_ERR_NO_DEVICE : 0;
}
void CensusSet::launch() const {
  rbtk::timer_begin(T_CENSUS);
  rbtk::launch_level_census((const RbtCensusPic*)d, (int)pics.size(), max_words);
  rbtk::timer_end(T_CENSUS);
}
int CensusSet::fetch() {
  hist.assign(pics.size() * RBT_RATE_HIST_WORDS, 0);
  return !hist.empty() && rbtk::d2h(hist.data(), d + o_hist, hist.size() * 4) ? RBT_ERR_NO_DEVICE : 0;
}
static size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
int HashSet::add(const uint16_t* const planes[3], int w, int h, int bit_depth, int kind, int counter, const uint8_t* want) {
  if (kind < RBT_HASH_MD5 || kind > RBT_HASH_CHECKSUM || w <= 0 || h <= 0 || (w | h) & 1 || bit_depth < 8 || bit_depth > 16 || (int)pics.size() >= RBT_HASH_MAX_PICS) return -1;
  RbtHashPic P; memset(&P, 0, sizeof(P));
  for (int c = 0; c < 3; c++) { if ((uintptr_t)planes[c] & 15) return -1; P.plane[c] = planes[c]; }   // the kernels read 16 bytes at a time
  P.w = w; P.h = h; P.bit_depth = bit_depth; P.kind = kind; P.counter = want ? counter : -1;
  if (want) memcpy(P.want, want, 48);
  pics.push_back(P);
  return (int)pics.size() - 1;
}
int HashSet::upload() {
  const size_t n = pics.size();
  std::vector<int32_t> lists;
  for (int cl = 0; cl < 6; cl++) {
    class_off[cl] = (int)lists.size(); n_class[cl] = 0; class_luma[cl] = 0; class_h[cl] = 0;
    for (size_t i = 0; i < n; i++) if ((pics[i].kind - 1) * 2 + (pics[i].bit_depth > 8) == cl) {
      lists.push_back((int32_t)i); n_class[cl]++; class_luma[cl] = std::max(class_luma[cl], pics[i].w * pics[i].h); class_h[cl] = std::max(class_h[cl], pics[i].h); }
  }
  o_lists = align16(n * sizeof(RbtHashPic)); o_state = align16(o_lists + n * 4); o_out = align16(o_state + n * RBT_HASH_STATE_WORDS * 4);
  o_end = o_out + n * 48 + (size_t)n_counters * 4;
  staging.assign(o_end, 0);
  memcpy(staging.data(), pics.data(), n * sizeof(RbtHashPic)); memcpy(staging.data() + o_lists, lists.data(), n * 4);
  rbtk::dev_free(d);
  d = (uint8_t*)rbtk::dev_alloc(o_end);
  if (!d) return RBT_ERR_NOMEM;
  return rbtk::h2d(d, staging.data(), o_end) ? RBT_ERR_NO_DEVICE : 0;
}
void HashSet::launch() const {
  const RbtHashPic* dp = (const RbtHashPic*)d; uint32_t* state = (uint32_t*)(d + o_state);
  for (int cl = 0; cl < 6; cl++) rbtk::launch_hash(dp, (const int32_t*)(d + o_lists) + class_off[cl], n_class[cl], cl / 2 + 1, cl & 1, class_luma[cl], class_h[cl], state);
  rbtk::launch_hash_finish(dp, (int)pics.size(), state, d + o_out, (uint32_t*)(d + o_out + pics.size() * 48));
}
int HashSet::fetch() {
  const size_t n = pics.size();
  std::vector<uint8_t> h(o_end - o_out);
  if (rbtk::d2h(h.data(), d + o_out, h.size())) return RBT_ERR_NO_DEVICE;
  out.assign(h.begin(), h.begin() + n * 48);
  counters.assign((size_t)n_counters, 0); if (n_counters) memcpy(counters.data(), h.data() + n * 48, (size_t)n_counters * 4);
  return 0;
}

}  // namespace rbt
