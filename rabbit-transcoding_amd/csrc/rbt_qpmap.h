// A QP per CTB (include/rbt.h "a QP per CTB"): what stands between the closed-loop stages, which code every CTB at its own target T (RbtFrame::qp_map), and
// the loop filters and the entropy coder, which need the QpY a DECODER derives and the predictor the cu_qp_delta is coded against (H.265 7.3.8.14, 8.6.1).
//
// With cu_qp_delta_enabled_flag = 1 and diff_cu_qp_delta_depth = 0 the quantisation group is the CTB. Its first transform unit with a cbf carries the delta, so
//   pred(c)  = qPY_PRED of CTB c = QpY of the last coding unit of the CTB before it in decoding order = T of the nearest earlier CTB of the same slice (of the same CTB row in
//              wavefront mode) that holds a cbf, SliceQpY if there is none - a closed form, no chain from CTB to CTB;
//   QpY      = pred(c) for every coding unit of c in front of the first one with a cbf (for all of them where c has none), T from that unit on.
// The closed-loop stages stored T in RbtFrame::qp for every unit. Two passes over the CTBs of a picture with a map put that right, both one wave per CTB, both plain loads and
// stores (cu_flags and cu_log2 are 64 bytes a CTB at most, the scan reads one byte per earlier CTB):
//   pass 0   en_qp_scan_ctb   where the CTB's first coded coding unit starts, in 8x8 units in z-order -> qp_pred[n_ctbs + c]
//   pass 1   en_qp_fix_ctb    pred(c) by a backward scan over those bytes, 64 CTBs a step; RbtFrame::qp of the leading units; pred(c) | RBT_QP_CODED -> qp_pred[c] for the
//                             entropy coder, which so has nothing to derive on its serial chain
// A pass is a launch of its own: pass 1 reads what pass 0 wrote for other CTBs. Pictures without a map are in neither.
#pragma once
#include "rbt_platform.h"
#include "rbt_types.h"

// cu_qp_delta (7.4.9.14) that takes the predictor `pred` to the QpY `qp`: the value d in -(26 + QpBdOffset / 2) .. 25 + QpBdOffset / 2 with wrap(pred + d) = qp (8.6.1; the
// parser's pz_wrap_qp). Both are in 0..51, so |qp - pred| <= 51 and one step of the modulus 52 + QpBdOffset brings the difference into the range
RBT_DEV int en_qp_delta(int qp, int pred, int bit_depth) {
  const int bdo = 6 * (bit_depth - 8); int d = qp - pred;
  if (d < -(26 + bdo / 2)) d += 52 + bdo; else if (d > 25 + bdo / 2) d -= 52 + bdo;
  return d;
}
#define RBT_QP_CBF_MASK (RBT_CU_CBF_Y | RBT_CU_CBF_CB | RBT_CU_CBF_CR | 7 * RBT_CU_CBF_Y1)
// 8x8 unit z of a CTB in z-order -> its column (bits 0..2) and row (bits 3..5) inside the CTB
RBT_DEV int en_qp_z_unit(int z) { return (z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4) | ((((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4)) << 3); }
// qp_pred word of pass 0 from what the CTB's units say: coded = bit z set where unit z (z-order) belongs to a block with a cbf, l2_first = cu_log2 of the lowest such unit.
// Coding units are aligned in z-order, so the unit's coding unit starts at z rounded down to the unit count of that size
RBT_DEV int en_qp_first_word(uint64_t coded, int l2_first) {
  if (!coded) return 0;
  const int z = __builtin_ctzll(coded);
  return RBT_QP_CODED | (z & ~((1 << (2 * (l2_first - 3))) - 1));
}

RBT_DEV void en_qp_scan_ctb(RbtFrame* f, int ctb_addr) {
  const int l2 = RBT_UNI(f->cfg.log2_ctb), wc = RBT_UNI(f->cfg.w_ctb), nc = wc * RBT_UNI(f->cfg.h_ctb), n8 = 1 << (l2 - 3), w8 = RBT_UNI(f->w8), h8 = RBT_UNI(f->h8);
  const int x8 = (ctb_addr % wc) * n8, y8 = (ctb_addr / wc) * n8;
  const uint8_t* fl = rbt_uni_ptr(f->cu_flags); const uint8_t* cl = rbt_uni_ptr(f->cu_log2);
  uint64_t coded; RBT_VEC(int, v_l2);
#define EN_QP_UNIT_IN(p) (x8 + (en_qp_z_unit(p) & 7) < w8 && y8 + (en_qp_z_unit(p) >> 3) < h8)
#define EN_QP_UNIT_K(p) ((size_t)(y8 + (en_qp_z_unit(p) >> 3)) * w8 + x8 + (en_qp_z_unit(p) & 7))
  RBT_VBALLOT(coded, p, n8 * n8, EN_QP_UNIT_IN(p) && (fl[EN_QP_UNIT_K(p)] & RBT_QP_CBF_MASK) != 0);
  RBT_VFOR(p, n8 * n8) RBT_V(v_l2, p) = EN_QP_UNIT_IN(p) ? (int)cl[EN_QP_UNIT_K(p)] : 3;
#undef EN_QP_UNIT_K
#undef EN_QP_UNIT_IN
  const int word = en_qp_first_word(coded, coded ? RBT_VGET(v_l2, __builtin_ctzll(coded)) : 3);
  if (RBT_LANE0) f->qp_pred[nc + ctb_addr] = (uint8_t)word;
}
// qPY_PRED of CTB ctb_addr: T (`map`) of the nearest CTB in [lo, ctb_addr) whose pass 0 word (`first`) says it holds a cbf, slice_qp if there is none
RBT_DEV int en_qp_pred(const int8_t* map, const uint8_t* first, int lo, int ctb_addr, int slice_qp) {
  for (int hi = ctb_addr; hi > lo; hi -= 64) {      // lane j looks at CTB hi - 1 - j: the lowest set bit is the nearest
    uint64_t m; RBT_VBALLOT(m, j, 64, hi - 1 - j >= lo && (first[hi - 1 - j] & RBT_QP_CODED) != 0);
    if (m) return RBT_UNI(map[hi - 1 - __builtin_ctzll(m)]);
  }
  return slice_qp;
}
RBT_DEV void en_qp_fix_ctb(RbtFrame* f, const RbtSlice* slices, int ctb_addr) {
  const int l2 = RBT_UNI(f->cfg.log2_ctb), wc = RBT_UNI(f->cfg.w_ctb), nc = wc * RBT_UNI(f->cfg.h_ctb), n8 = 1 << (l2 - 3), w8 = RBT_UNI(f->w8), h8 = RBT_UNI(f->h8), w4 = RBT_UNI(f->cfg.w4);
  const int rx = ctb_addr % wc, x8 = rx * n8, y8 = (ctb_addr / wc) * n8;
  const int8_t* map = rbt_uni_ptr(f->qp_map); uint8_t* pred_out = rbt_uni_ptr(f->qp_pred); const uint8_t* first = pred_out + nc; int8_t* qp = rbt_uni_ptr(f->qp);
  // the slice the CTB belongs to (its independent segment: RbtFrame::ctb_slice); in wavefront mode the prediction restarts from SliceQpY at every CTB row (8.6.1)
  const RbtSlice* sl = &slices[RBT_UNI(f->ctb_slice[ctb_addr])];
  const int lo = RBT_UNI(sl->wpp) ? ctb_addr - rx : RBT_UNI(sl->ctb_addr);
  const int pred = en_qp_pred(map, first, lo, ctb_addr, RBT_UNI(sl->qp));
  const int word = RBT_UNI(first[ctb_addr]), n_lead = (word & RBT_QP_CODED) ? (word & 63) : n8 * n8;
  RBT_PAR_FOR(i, n_lead * 4) {      // the four 4x4 entries of every 8x8 unit in front of the first coded coding unit (the picture is whole 8x8 units)
    const int u = en_qp_z_unit(i >> 2), ux = x8 + (u & 7), uy = y8 + (u >> 3);
    if (ux < w8 && uy < h8) qp[(size_t)(2 * uy + ((i >> 1) & 1)) * w4 + 2 * ux + (i & 1)] = (int8_t)pred;
  }
  if (RBT_LANE0) pred_out[ctb_addr] = (uint8_t)((word & RBT_QP_CODED) | pred);
}

namespace rbtk {
#ifdef RBT_HOSTEMU
inline void enc_qp_map_variant(int) { }      // the serial stand-ins have one instantiation, which asks the picture (rbt_encode.h EN_QP_ASK)
#else
void enc_qp_map_variant(int on);
#endif
// both passes for every CTB of the listed pictures (all of them carry a map); max_ctbs: CTBs of the largest picture
void launch_enc_qp_fix(RbtFrame* frames, const RbtSlice* slices, const int32_t* frame_list, int n_frames, int max_ctbs);
#ifdef RBT_HOSTEMU
// serial stand-in of the launcher (the product's is in rbt_kernels.hip)
inline void launch_enc_qp_fix(RbtFrame* frames, const RbtSlice* slices, const int32_t* frame_list, int n_frames, int) {
  for (int k = 0; k < n_frames; k++) { RbtFrame* f = &frames[frame_list[k]]; const int nc = f->cfg.w_ctb * f->cfg.h_ctb;
    for (int a = 0; a < nc; a++) en_qp_scan_ctb(f, a);
    for (int a = 0; a < nc; a++) en_qp_fix_ctb(f, slices, a); }
}
#endif
}  // namespace rbtk
