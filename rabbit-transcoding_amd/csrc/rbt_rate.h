// Level census of decoded pictures (rbt_level_census, rbt_rate_estimate, rbt_submit_gof_rate; the definitions are in include/rbt.h): per picture and plane a histogram
// uint32 hist[3][53] that says, for every output QP q, how many of the input's coefficient levels would still be non-zero if they were requantised at q. The host turns
// it into the first guess of a rate-targeted transcode (host/rbt_transcode.cpp); nothing on the device depends on the guess.
//   level    l != 0 of plane c at sample (x, y); qin = RbtFrame::qp of the 4x4 luma unit that covers it (chroma: the unit of luma sample (2x, 2y)), clamped to 0..51;
//            units with RBT_PM_TQ_BYPASS hold residual samples and are left out
//   m        |l| * LS[qin % 6] << (qin / 6): the de-quantised magnitude in units of 1 / 64 (at most 2^15 * 72 * 2^8 < 2^30)
//   survive  3 * m * G[q % 6] >= 2^(21 + q / 6): the level requantised at q is at least 2 / 3 (64-bit integers, < 2^46); monotone in q
//   bin      the number of q in 0..51 the level survives (0..52), found by bisection on the monotone condition: 6 steps
//   lanes    a workgroup of 256 lanes takes a tile of RBT_RATE_TILE_WORDS words of 4 samples (8 bytes a lane and load, a wave reads 512 contiguous bytes), counted over the
//            three planes of the picture back to back; a word of zeros - most of them - costs its load and one compare. Bins are counted in LDS (ds_add_u32); after a
//            barrier every non-empty bin is one global integer add. Sums of integers: the result does not depend on the order of arrival.
// No floating point, no kernel waits for another, every loop is bounded by the tile.
#pragma once
#include "rbt_platform.h"
#include "rbt_types.h"

enum { RBT_RATE_BINS = 53, RBT_RATE_HIST_WORDS = 3 * RBT_RATE_BINS, RBT_RATE_WG = 256, RBT_RATE_TILE_WORDS = 4096 };
// one picture: the three planes of levels (w x h, then two of w/2 x h/2; w, h multiples of 8; each plane 8-byte aligned), the per-4x4-unit maps (w/4 units a row) and where its histogram goes
struct RbtCensusPic { const int16_t* coef[3]; const int8_t* qp; const uint8_t* pm; int32_t w, h; uint32_t* hist; };

namespace rbtk {
// hist of every picture zeroed beforehand; max_words = RBT_RATE_PIC_WORDS of the largest picture
void launch_level_census(const RbtCensusPic* pics, int n_pics, int max_words);
}  // namespace rbtk

// integer add on a global word from any lane of any workgroup; a plain add in the serial host emulation
#ifdef RBT_HOSTEMU
#define RBT_GLOBAL_ADD(p, v) (*(p) += (v))
#else
#define RBT_GLOBAL_ADD(p, v) ((void)__hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
#endif

// ------------------------------------------------------------------------------------------------ bodies (device, host emulation and the host's estimate)
#define RBT_RATE_PIC_WORDS(w, h) (((w) * (h) + 2 * ((w) / 2) * ((h) / 2)) / 4)     // words of 4 samples in the three planes of a picture

RBT_DEV int rate_survives(uint32_t m, int q) {
  const uint32_t G[6] = {26214, 23302, 20560, 18396, 16384, 14564};
  return 3ull * m * G[q % 6] >= 1ull << (21 + q / 6);
}
// bin of level l (!= 0) decoded at QP qin (0..51)
RBT_DEV int rate_bin(int l, int qin) {
  const uint32_t LS[6] = {40, 45, 51, 57, 64, 72};
  const uint32_t a = (uint32_t)(l < 0 ? -l : l);           // -32768 -> 32768
  const uint32_t m = (a * LS[qin % 6]) << (qin / 6);
  int lo = 0, hi = 52;                                     // the first q the level does not survive, 52 if there is none
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (rate_survives(m, mid)) lo = mid + 1; else hi = mid; }
  return lo;
}
// word i of plane c (4 samples of one row): the levels into the workgroup's bins
RBT_DEV void rate_word(const RbtCensusPic* P, int c, int i, RBT_LDS_AS uint32_t* bins) {
  const uint32_t* p32 = (const uint32_t*)P->coef[c] + 2 * (size_t)i;
  const uint32_t w0 = p32[0], w1 = p32[1];
  if (!(w0 | w1)) return;
  const int pw = c ? P->w >> 1 : P->w, w4 = P->w >> 2;
  const int s0 = 4 * i, y = s0 / pw, x = s0 - y * pw;
  for (int k = 0; k < 4; k++) {
    const int l = (int16_t)((k < 2 ? w0 : w1) >> (16 * (k & 1)));
    if (!l) continue;
    const int u = c ? (y >> 1) * w4 + ((x + k) >> 1) : (y >> 2) * w4 + (x >> 2);
    if (P->pm[u] & RBT_PM_TQ_BYPASS) continue;
    const int qin = rbt_clip3(0, 51, P->qp[u]);
    RBT_LDS_ADD(&bins[c * RBT_RATE_BINS + rate_bin(l, qin)], 1u);
  }
}
// tile `tile` of one picture; bins: RBT_RATE_HIST_WORDS words of LDS
RBT_DEV void rate_census_tile(const RbtCensusPic* P, int tile, RBT_LDS_AS uint32_t* bins) {
  const int ny = P->w * P->h / 4, nc = (P->w >> 1) * (P->h >> 1) / 4, total = ny + 2 * nc;
  const int first = tile * RBT_RATE_TILE_WORDS;
  if (first >= total) return;                              // (uniform over the workgroup)
  const int n = rbt_min(RBT_RATE_TILE_WORDS, total - first);
  RBT_BLK_FOR(t, RBT_RATE_HIST_WORDS) bins[t] = 0;
  RBT_SYNC();
  RBT_BLK_FOR(t, n) {
    const int i = first + t;
    if (i < ny) rate_word(P, 0, i, bins); else if (i < ny + nc) rate_word(P, 1, i - ny, bins); else rate_word(P, 2, i - ny - nc, bins);
  }
  RBT_SYNC();
  RBT_BLK_FOR(t, RBT_RATE_HIST_WORDS) { const uint32_t v = bins[t]; if (v) RBT_GLOBAL_ADD(&P->hist[t], v); }
}

#ifdef RBT_HOSTEMU
// serial stand-in of the launcher (the product's is in rbt_rate.hip)
namespace rbtk {
inline void launch_level_census(const RbtCensusPic* pics, int n_pics, int max_words) {
  uint32_t bins[RBT_RATE_HIST_WORDS];
  for (int k = 0; k < n_pics; k++) for (int t = 0; t * RBT_RATE_TILE_WORDS < max_words; t++) rate_census_tile(&pics[k], t, bins);
}
}  // namespace rbtk
#endif
