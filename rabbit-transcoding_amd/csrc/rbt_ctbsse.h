// Luma distortion sums per CTB, folded per patch (rbt_ctb_sse, rbt_submit_gof_quality_patches; the definitions are in include/rbt.h, "PSNR floors held patch by patch";
// DESIGN.md 20). Between two pictures A and B of one size - RbtSsePic's: a decoded input seen through its conformance window, the encoder's reconstruction without its
// coding padding - and for every CTB of the w x h picture's grid at log2_ctb three unsigned 64-bit words:
//   out[3 * ctb + 0] = sse      the sum of (A - B)^2 over the luma samples of the CTB that lie in the displayed w x h area
//   out[3 * ctb + 1] = sse_occ  the same over the occupied samples (rbt_quality.h: luma sample (x, y) iff O[y / s][x / s] > 0), 0 without a map
//   out[3 * ctb + 2] = n_occ    the count of those
// A CTB of 64x64 at 10 bits reaches 4096 x 1023^2 = 2^32 - 8384512, two of them are beyond 32 bits, and so is one CTB of 16x16 at 16 bits: hence 64-bit words.
//   k_ctb_sse     one wave per CTB, a workgroup of 256 lanes takes four CTBs. A row of the CTB (cw <= 64 samples) is cut into cw / 8 + 2 chunks by the rule of sse_chunk: where
//                 the two row pointers are equally far from a 16-byte boundary, chunk 0 is the head in front of it, the chunks behind it are one 16-byte load from either
//                 picture, the last one is the tail; where they are not (windows have even offsets: the pictures can disagree), every chunk is read sample by sample. A lane
//                 takes every 64th chunk of the CTB - at most ten, 80 samples -, the three sums are folded across the wave in registers (sse_wave_sum), lane 0 writes the
//                 three words with plain stores. Exactly one wave writes a CTB's words: no atomics, no LDS, nothing zeroed beforehand, no wave waits for another; every
//                 loop is bounded by the CTB size; partial CTBs at the right and bottom edge read nothing outside the displayed area.
//   k_patch_fold  per point-cloud frame (pictures 2f and 2f + 1) and rectangle (c0, r0, c1, r1 in CTB units, half-open, inside the grid) the three words summed over the
//                 rectangle's CTBs in both pictures; behind the n_rects rectangles two more triples: the background (the CTBs no rectangle meets) and the whole frame. One
//                 wave per (rectangle, frame), a lane takes the CTBs strided by 64, then the fold, then plain stores by lane 0.
// No floating point. Sums of integers: the result does not depend on the order.
#pragma once
#include "rbt_platform.h"
#include "rbt_quality.h"

enum { RBT_CTBSSE_WG = 256, RBT_CTBSSE_WORDS = 3 };
// one picture pair (luma only): the planes with their row strides, the occupancy plane of ow samples a row (nullptr: none) with its scale, the grid, where the words go
struct RbtCtbSsePic { const uint16_t* a; const uint16_t* b; const uint16_t* occ; int32_t w, h, a_stride, b_stride, ow, scale, log2_ctb, w_ctb, h_ctb, pad_; uint64_t* out; };
// one point-cloud frame: the CTB words of its two pictures, its rectangles (4 x n_rects ints), the grid, and where the (n_rects + 2) triples go
struct RbtFoldJob { const uint64_t* ctb[2]; const int32_t* rects; int32_t n_rects, w_ctb, h_ctb, pad_; uint64_t* out; };

namespace rbtk {
void launch_ctb_sse(const RbtCtbSsePic* pics, int n_pics, int max_ctbs);          // max_ctbs: CTBs of the largest grid
void launch_patch_fold(const RbtFoldJob* jobs, int n_jobs, int max_rects);       // max_rects: the largest n_rects (the two extra triples not counted)
}  // namespace rbtk

// ------------------------------------------------------------------------------------------------ bodies (device and host emulation)
// chunk j of row y of the CTB that starts at column cx0 and is cw samples wide, into the lane's sums
RBT_DEV void ctbsse_chunk(const RbtCtbSsePic* P, int cx0, int cw, int y, int j, uint64_t* sse, uint64_t* sse_occ, uint64_t* n_occ) {
  const uint16_t* ra = P->a + (size_t)y * (size_t)P->a_stride + cx0;
  const uint16_t* rb = P->b + (size_t)y * (size_t)P->b_stride + cx0;
  const int ma = (int)(((uintptr_t)ra >> 1) & 7), mb = (int)(((uintptr_t)rb >> 1) & 7);
  const int head = ma == mb ? rbt_min(cw, (8 - ma) & 7) : 0;
  const int x0 = j == 0 ? 0 : head + 8 * (j - 1), x1 = j == 0 ? head : rbt_min(cw, x0 + 8);
  if (x0 >= x1) return;
  uint16_t va[8], vb[8];
  if (ma == mb && x1 - x0 == 8 && j > 0) {      // both addresses are multiples of 16
    const RbtSseQuad qa = *(const RbtSseQuad*)(ra + x0), qb = *(const RbtSseQuad*)(rb + x0);
    const uint32_t wa[4] = {qa.x, qa.y, qa.z, qa.w}, wb[4] = {qb.x, qb.y, qb.z, qb.w};
    for (int k = 0; k < 8; k++) { va[k] = (uint16_t)(wa[k >> 1] >> (16 * (k & 1))); vb[k] = (uint16_t)(wb[k >> 1] >> (16 * (k & 1))); }
  } else for (int k = 0; k < x1 - x0; k++) { va[k] = ra[x0 + k]; vb[k] = rb[x0 + k]; }
  const int scale = P->occ ? P->scale : 1;      // picture column cx0 + x0: ox = its column in the map, rem = how far it is into that column
  const uint16_t* ro = P->occ ? P->occ + (size_t)(y / scale) * (size_t)P->ow : nullptr;
  int ox = (cx0 + x0) / scale, rem = (cx0 + x0) - ox * scale;
  for (int k = 0; k < x1 - x0; k++) {
    const int64_t d = (int64_t)va[k] - (int64_t)vb[k]; const uint64_t e = (uint64_t)(d * d);
    *sse += e;
    if (ro && ro[ox] > 0) { *sse_occ += e; *n_occ += 1; }
    if (++rem >= scale) { rem = 0; ox++; }
  }
}
// one CTB of one picture: the whole wave
RBT_DEV void ctbsse_ctb(const RbtCtbSsePic* P, int ctb) {
  const int l2 = P->log2_ctb, wc = P->w_ctb, cy = ctb / wc, cx = ctb - cy * wc, cx0 = cx << l2, cy0 = cy << l2;
  const int cw = rbt_min(1 << l2, P->w - cx0), ch = rbt_min(1 << l2, P->h - cy0), per = cw / 8 + 2, n = ch * per;      // (n <= 64 * 10)
  uint64_t s = 0, so = 0, no = 0;
  RBT_PAR_FOR(t, n) { const int row = t / per; ctbsse_chunk(P, cx0, cw, cy0 + row, t - row * per, &s, &so, &no); }
  s = sse_wave_sum(s); so = sse_wave_sum(so); no = sse_wave_sum(no);
  if (RBT_LANE0) { uint64_t* o = P->out + (size_t)ctb * RBT_CTBSSE_WORDS; o[0] = s; o[1] = so; o[2] = no; }
}
// triple r of one frame: rectangle r < n_rects, the background (r == n_rects: the CTBs no rectangle meets), the whole frame (r == n_rects + 1)
RBT_DEV void ctbsse_fold(const RbtFoldJob* J, int r) {
  const int nr = J->n_rects, wc = J->w_ctb, hc = J->h_ctb; const int32_t* rc = J->rects;
  int c0 = 0, r0 = 0, c1 = wc, r1 = hc;
  if (r < nr) { c0 = rc[4 * r]; r0 = rc[4 * r + 1]; c1 = rc[4 * r + 2]; r1 = rc[4 * r + 3]; }
  const int rw = c1 - c0, n = rw > 0 && r1 > r0 ? rw * (r1 - r0) : 0;
  uint64_t s[3] = {0, 0, 0};
  RBT_PAR_FOR(t, n) {
    const int y = t / rw, cx = c0 + t - y * rw, cy = r0 + y;
    bool take = true;
    if (r == nr) for (int k = 0; k < nr && take; k++) take = !(cx >= rc[4 * k] && cx < rc[4 * k + 2] && cy >= rc[4 * k + 1] && cy < rc[4 * k + 3]);
    if (take) for (int p = 0; p < 2; p++) { const uint64_t* w = J->ctb[p] + ((size_t)cy * wc + cx) * RBT_CTBSSE_WORDS; s[0] += w[0]; s[1] += w[1]; s[2] += w[2]; }
  }
  for (int k = 0; k < 3; k++) s[k] = sse_wave_sum(s[k]);
  if (RBT_LANE0) { uint64_t* o = J->out + (size_t)r * RBT_CTBSSE_WORDS; o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; }
}

#ifdef RBT_HOSTEMU
// serial stand-ins of the launchers (the product's are in rbt_quality.hip)
namespace rbtk {
inline void launch_ctb_sse(const RbtCtbSsePic* pics, int n_pics, int) {
  for (int k = 0; k < n_pics; k++) for (int c = 0; c < pics[k].w_ctb * pics[k].h_ctb; c++) ctbsse_ctb(&pics[k], c);
}
inline void launch_patch_fold(const RbtFoldJob* jobs, int n_jobs, int) {
  for (int k = 0; k < n_jobs; k++) for (int r = 0; r < jobs[k].n_rects + 2; r++) ctbsse_fold(&jobs[k], r);
}
}  // namespace rbtk
#endif
