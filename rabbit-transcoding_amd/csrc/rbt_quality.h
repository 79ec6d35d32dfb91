// Distortion sums of pictures in device memory (rbt_picture_sse, rbt_submit_gof_quality; the definitions are in include/rbt.h): per picture nine unsigned 64-bit words,
// out[3 * c + 0] = sse[c], out[3 * c + 1] = sse_occ[c], out[3 * c + 2] = n_occ[c] for the planes c = Y, Cb, Cr, between two pictures A and B of one size that are given by
// plane pointers and row strides (A: a decoded input seen through its conformance window, B: the encoder's reconstruction without its coding padding).
//   sse      the sum of (A - B)^2 over the plane: w x h samples of luma, w/2 x h/2 of each chroma plane
//   occupied with an occupancy luma plane O of ow x oh samples and the whole scale s = w / ow = h / oh: luma sample (x, y) iff O[y / s][x / s] > 0, chroma sample (x, y) iff
//            luma sample (2x, 2y) is; sse_occ and n_occ are the sum and the count over those. Without a map both stay 0.
//   chunks   a row of pw samples is cut into pw / 8 + 2 chunks: where the two row pointers are equally far from a 16-byte boundary, chunk 0 is the head in front of that
//            boundary (0..7 samples), the chunks behind it hold 8 samples each - one 16-byte load from either picture - and the last one the tail; where they are not, chunk
//            0 is empty and every chunk is read sample by sample, like heads and tails. The chunks of the three planes are counted back to back.
//   lanes    a workgroup of 256 lanes takes a tile of RBT_SSE_TILE_CHUNKS chunks, a lane every 256th of them (a wave reads 1 KB of a row at a time). A lane sums its at most
//            128 samples in 64 bits - a squared difference of 16-bit samples is below 2^32 -, the nine sums are folded across the wave in registers (six exchange steps),
//            lane 0 of each of the four waves adds them into nine 64-bit words of LDS (ds_add_u64), and after a barrier every non-zero word is one 64-bit global integer
//            add: nine at most per workgroup. Sums of integers: the result does not depend on the order of arrival.
//   map      the occupancy sample of a chunk's first sample comes from one division per chunk and direction; along the chunk a remainder counts up to the scale.
// No floating point, no kernel waits for another, every loop is bounded by the tile.
#pragma once
#include "rbt_platform.h"
#include "rbt_rate.h"      // RBT_GLOBAL_ADD

enum { RBT_SSE_WORDS = 9, RBT_SSE_WG = 256, RBT_SSE_TILE_CHUNKS = 4096 };
// one picture pair: the planes (chroma strides are half the luma strides), the occupancy plane of ow samples a row (nullptr: none) with its scale, and where the nine words go
struct RbtSsePic { const uint16_t* a[3]; const uint16_t* b[3]; const uint16_t* occ; int32_t w, h, a_stride, b_stride, ow, scale; uint64_t* out; };

namespace rbtk {
// out of every picture zeroed beforehand; max_chunks = RBT_SSE_PIC_CHUNKS of the largest picture
void launch_picture_sse(const RbtSsePic* pics, int n_pics, int max_chunks);
}  // namespace rbtk

// ------------------------------------------------------------------------------------------------ bodies (device and host emulation)
#define RBT_SSE_ROW_CHUNKS(pw) ((pw) / 8 + 2)
#define RBT_SSE_PIC_CHUNKS(w, h) ((h) * RBT_SSE_ROW_CHUNKS(w) + 2 * ((h) / 2) * RBT_SSE_ROW_CHUNKS((w) / 2))

struct alignas(16) RbtSseQuad { uint32_t x, y, z, w; };      // eight samples, one 16-byte load
// chunk j of row y of plane c into the lane's sums
RBT_DEV void sse_chunk(const RbtSsePic* P, int c, int y, int j, uint64_t* sse, uint64_t* sse_occ, uint32_t* n_occ) {
  const int sh = c ? 1 : 0, pw = P->w >> sh;
  const uint16_t* ra = P->a[c] + (size_t)y * (size_t)(P->a_stride >> sh);
  const uint16_t* rb = P->b[c] + (size_t)y * (size_t)(P->b_stride >> sh);
  const int ma = (int)(((uintptr_t)ra >> 1) & 7), mb = (int)(((uintptr_t)rb >> 1) & 7);
  const int head = ma == mb ? rbt_min(pw, (8 - ma) & 7) : 0;
  const int x0 = j == 0 ? 0 : head + 8 * (j - 1), x1 = j == 0 ? head : rbt_min(pw, x0 + 8);
  if (x0 >= x1) return;
  uint16_t va[8], vb[8];
  if (ma == mb && x1 - x0 == 8 && j > 0) {      // both addresses are multiples of 16
    const RbtSseQuad qa = *(const RbtSseQuad*)(ra + x0), qb = *(const RbtSseQuad*)(rb + x0);
    const uint32_t wa[4] = {qa.x, qa.y, qa.z, qa.w}, wb[4] = {qb.x, qb.y, qb.z, qb.w};
    for (int k = 0; k < 8; k++) { va[k] = (uint16_t)(wa[k >> 1] >> (16 * (k & 1))); vb[k] = (uint16_t)(wb[k >> 1] >> (16 * (k & 1))); }
  } else for (int k = 0; k < x1 - x0; k++) { va[k] = ra[x0 + k]; vb[k] = rb[x0 + k]; }
  const int scale = P->occ ? P->scale : 1, step = 1 << sh;      // luma position (x << sh, y << sh): ox = its column in the map, rem = how far it is into that column
  const uint16_t* ro = P->occ ? P->occ + (size_t)((y << sh) / scale) * (size_t)P->ow : nullptr;
  int ox = (x0 << sh) / scale, rem = (x0 << sh) - ox * scale;
  for (int k = 0; k < x1 - x0; k++) {
    const int64_t d = (int64_t)va[k] - (int64_t)vb[k]; const uint64_t e = (uint64_t)(d * d);
    *sse += e;
    if (ro && ro[ox] > 0) { *sse_occ += e; *n_occ += 1; }
    rem += step;
    while (rem >= scale) { rem -= scale; ox++; }               // (twice at most: step <= 2, scale >= 1)
  }
}
// the sum of v over the lanes of the wave, in every lane; the serial host emulation is its own only lane
#ifdef RBT_HOSTEMU
#define RBT_SSE_LANES 1
RBT_DEV uint64_t sse_wave_sum(uint64_t v) { return v; }
#else
#define RBT_SSE_LANES RBT_SSE_WG
RBT_DEV uint64_t sse_wave_sum(uint64_t v) { for (int o = 32; o; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64); return v; }
#endif
// tile `tile` of one picture; acc: RBT_SSE_WORDS words of LDS
RBT_DEV void sse_tile(const RbtSsePic* P, int tile, RBT_LDS_AS uint64_t* acc) {
  const int ry = RBT_SSE_ROW_CHUNKS(P->w), rc = RBT_SSE_ROW_CHUNKS(P->w >> 1), ny = P->h * ry, nc = (P->h >> 1) * rc, total = ny + 2 * nc;
  const int first = tile * RBT_SSE_TILE_CHUNKS;
  if (first >= total) return;                              // (uniform over the workgroup)
  const int n = rbt_min(RBT_SSE_TILE_CHUNKS, total - first);
  RBT_BLK_FOR(t, RBT_SSE_WORDS) acc[t] = 0;
  RBT_SYNC();
  RBT_BLK_FOR(lane, RBT_SSE_LANES) {                        // every lane of the workgroup, once: the fold below needs whole waves
    uint64_t s[3] = {0, 0, 0}, so[3] = {0, 0, 0}; uint32_t no[3] = {0, 0, 0};
    for (int t = lane; t < n; t += RBT_SSE_LANES) {
      const int i = first + t, c = i < ny ? 0 : i < ny + nc ? 1 : 2, r = i - (c == 0 ? 0 : c == 1 ? ny : ny + nc), per = c ? rc : ry, row = r / per;
      sse_chunk(P, c, row, r - row * per, &s[c], &so[c], &no[c]);
    }
    for (int c = 0; c < 3; c++) {
      const uint64_t f[3] = {sse_wave_sum(s[c]), sse_wave_sum(so[c]), sse_wave_sum((uint64_t)no[c])};
      if ((lane & 63) == 0) for (int k = 0; k < 3; k++) if (f[k]) RBT_LDS_ADD(&acc[3 * c + k], f[k]);
    }
  }
  RBT_SYNC();
  RBT_BLK_FOR(t, RBT_SSE_WORDS) { const uint64_t v = acc[t]; if (v) RBT_GLOBAL_ADD(&P->out[t], v); }
}

#ifdef RBT_HOSTEMU
// serial stand-in of the launcher (the product's is in rbt_quality.hip)
namespace rbtk {
inline void launch_picture_sse(const RbtSsePic* pics, int n_pics, int max_chunks) {
  uint64_t acc[RBT_SSE_WORDS];
  for (int k = 0; k < n_pics; k++) for (int t = 0; t * RBT_SSE_TILE_CHUNKS < max_chunks; t++) sse_tile(&pics[k], t, acc);
}
}  // namespace rbtk
#endif
