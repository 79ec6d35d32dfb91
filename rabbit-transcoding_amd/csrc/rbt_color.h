// Colour half of the verification stage: what lies between the decoded attribute maps and the colour PSNR the reference reports per frame.
//   up-conversion  4:2:0 -> 4:4:4, 16 bit, as the decoder does it to an attribute video under the CTC settings:
//                  PCCVideoDecoder.cpp:126-145 -> PCCInternalColorConverter::convertYUV420ToYUV444 (PCCInternalColorConverter.cpp:466-485) with filter 0,
//                  i.e. YUVtoFloatYUV (:596-610), upsampling (:669-695; the float inner loops of PCCInternalColorConverter.h:187-249), floatYUVToYUV with
//                  nbyte = 2 (:580-593); and the sample replication of PCCImage::convertYUV420ToYUV444 (PCCImage.cpp:111-135)
//   RGB            PCCPointSet3::convertYUV16ToRGB8 (PCCPointSet.h:133-166), in double
//   colour metric  QualityMetrics::compute with computeColor_ (PCCMetrics.cpp:127-179, :221-225) on clouds whose duplicates are merged with averaged colours
//                  (dropDuplicates_ = 2: PCCPointSet3::removeDuplicate, PCCPointSet.cpp:190-203) and neighborsProc_ = 1 (:140-154), both directions (:321-325)
// Floating point: every product and sum below is rounded on its own, in the reference's order and types. csrc/rbt_color.hip is compiled with -ffp-contract=off
// (Makefile), and the functions carry the pragma as well; the double-precision steps stay double. The up-converted samples and the RGB bytes are therefore the same
// bits on the GPU, in the serial host emulation and in a restatement in float32 / float64.
// The metric is integer throughout (the reference's float form and how far the two can differ: DESIGN.md 8): a cloud becomes a bit volume plus a hash map voxel ->
// slot (csrc/rbt_pcc.h), the slot holds the colour sums and the count of the voxel's points, and the set of nearest merged points is walked in the other cloud's
// volume as for D2. The error terms are BT.709 differences times 10000 * 255; their squares are summed in unsigned 64-bit, so the order of arrival does not matter.
//
// The kernel bodies below are shared with the serial host emulation (RBT_HOSTEMU, tests/hostemu): there the launchers at the end of this file run them as plain loops.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "rbt_platform.h"
#include "../../include/rbt.h"
#include "rbt_types.h"
#include "rbt_pcc.h"

// ---- up-conversion ----
// one workgroup (256 threads) makes one RBT_UP_TW x RBT_UP_TH tile of one output plane; a chroma tile needs RBT_UP_TW / 2 x RBT_UP_TH / 2 input samples plus the
// halo of the four-tap filters: two rows above and below, one column left and two right
enum { RBT_UP_TW = 64, RBT_UP_TH = 32, RBT_UP_SW = RBT_UP_TW / 2 + 3, RBT_UP_SH = RBT_UP_TH / 2 + 4, RBT_UP_STRIDE = RBT_UP_SW + 2, RBT_UP_THREADS = 256 };
struct RbtUpLds { float src[RBT_UP_SH * RBT_UP_STRIDE]; float tmp[RBT_UP_TH * RBT_UP_STRIDE]; };   // the staged samples as float; the vertical pass's output
struct alignas(16) RbtU16x8 { uint32_t w[4]; };                                                    // eight samples, two per word (the lower-addressed one in the low half): one 16-byte access, built in registers

// one cloud of the colour metric: acc holds 4 words per hash slot (sums of R, G, B and the number of points of the voxel), col the merged colour (R | G << 8 | B << 16)
struct RbtColSet { const int16_t* xyz; const uint8_t* rgb; int32_t n, lg; uint32_t* vol; uint32_t* keys; uint32_t* acc; uint32_t* col; };

namespace rbtk {
// yuv420: n_frames planar 4:2:0 pictures; yuv444: n_frames x 3 planes of w * h. filter: RBT_UPSAMPLE_F0 or RBT_UPSAMPLE_REPLICATE
void launch_up444(const uint16_t* yuv420, int w, int h, int bit_depth, int n_frames, int filter, uint16_t* yuv444);
void launch_yuv16_rgb8(const uint16_t* yuv, int n, uint8_t* rgb);
// vol, keys, acc zeroed beforehand; *n_unique (zeroed) counts the voxels, i.e. the merged points
void launch_col_insert(const RbtColSet* S, uint32_t* n_unique);
void launch_col_merge(const RbtColSet* S);
// sse[3] (zeroed): sums of the squared error terms of P's merged points against Q
void launch_col_dist(const RbtColSet* P, const RbtColSet* Q, unsigned long long* sse);
}  // namespace rbtk

// ------------------------------------------------------------------------------------------------ bodies (device and host emulation)
// YUVtoFloatYUV (:596-610)
RBT_DEV float cl_to_float(int s, int chroma, int bd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double scale = bd == 8 ? 255.0 : 1023.0, weight = 1.0 / scale;
  const int offset = chroma ? (bd == 8 ? 128 : 512) : 0;
  const float v = (float)(weight * (double)(s - offset)), lo = chroma ? -0.5f : 0.f, hi = chroma ? 0.5f : 1.f;
  return v < lo ? lo : (v > hi ? hi : v);
}
// floatYUVToYUV with nbyte = 2 (:580-593)
RBT_DEV uint16_t cl_to_16(float v, int chroma) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double offset = chroma ? 32768.0 : 0.0;
  float r = __builtin_roundf((float)(65535.0 * (double)v + offset));
  r = r < 0.f ? 0.f : (r > 65535.f ? 65535.f : r);
  return (uint16_t)r;
}
// The tap rows of g_filter420to444[0] (PCCInternalColorConverter.cpp:297-302; member order horizontal0_, vertical0_, horizontal1_, vertical1_), shift 8.
// upsamplingVertical0 at row i (odd = 0) reads rows i - 2 .. i + 1, upsamplingVertical1 at row i + 1 (odd = 1) rows i - 1 .. i + 2: s[0..4] = rows i - 2 .. i + 2
RBT_DEV float cl_up_vertical(int odd, const float s[5]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float value = 0;
  if (!odd) { value += -8.0f * s[0]; value += 64.0f * s[1]; value += 216.0f * s[2]; value += -16.0f * s[3]; }
  else { value += -16.0f * s[1]; value += 216.0f * s[2]; value += 64.0f * s[3]; value += -8.0f * s[4]; }
  return (value + 0.0f) * (1.0f / 256.0f);
}
// upsamplingHorizontal0 at column j (odd = 0) reads columns j - 1, j; upsamplingHorizontal1 at column j + 1 (odd = 1) columns j - 1 .. j + 2: s[0..3] = columns j - 1 .. j + 2
RBT_DEV float cl_up_horizontal(int odd, float s0, float s1, float s2, float s3) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float value = 0;
  if (!odd) { value += 0.0f * s0; value += 256.0f * s1; }
  else { value += -16.0f * s0; value += 144.0f * s1; value += 144.0f * s2; value += -16.0f * s3; }
  return (value + 0.0f) * (1.0f / 256.0f);
}
RBT_DEV int cl_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Tile (tx, ty) of plane `plane` of picture `frame`. Luma: sample by sample through the same float round trip. Chroma: the input samples of the tile and their halo go to
// LDS as float once (indices clamped to the plane, as the reference clamps them), the vertical pass fills tmp (the rows of the reference's widthIn x 2 heightIn plane that
// the tile needs), the horizontal pass reads tmp and stores eight samples per lane.
RBT_DEV void cl_up_tile(const uint16_t* in, uint16_t* out, int w, int h, int bd, int frame, int plane, int tx, int ty, RBT_LDS_AS RbtUpLds* L) {
  const size_t ys = (size_t)w * h; const int cw = w / 2, ch = h / 2;
  const uint16_t* src = in + (size_t)frame * (ys + ys / 2) + (plane ? ys + (size_t)(plane - 1) * cw * ch : 0);
  uint16_t* dst = out + ((size_t)frame * 3 + plane) * ys;
  const int wide = (w & 7) == 0;                                  // rows and planes are 16-byte aligned: vector access
  if (plane == 0) {
    RBT_BLK_FOR(t, RBT_UP_THREADS) {
      const int y = ty * RBT_UP_TH + (t >> 3), x0 = tx * RBT_UP_TW + (t & 7) * 8;
      if (y < h && x0 < w) {
        const size_t o = (size_t)y * w + x0;
        if (wide) {
          const RbtU16x8 a = *(const RbtU16x8*)(src + o); RbtU16x8 r;
#pragma unroll
          for (int k = 0; k < 4; k++)
            r.w[k] = (uint32_t)cl_to_16(cl_to_float((int)(a.w[k] & 0xFFFFu), 0, bd), 0) | (uint32_t)cl_to_16(cl_to_float((int)(a.w[k] >> 16), 0, bd), 0) << 16;
          *(RbtU16x8*)(dst + o) = r;
        } else {
          for (int k = 0; k < 8 && x0 + k < w; k++) dst[o + k] = cl_to_16(cl_to_float(src[o + k], 0, bd), 0);
        }
      }
    }
    return;
  }
  const int cx0 = tx * (RBT_UP_TW / 2), cy0 = ty * (RBT_UP_TH / 2);
  RBT_BLK_FOR(e, RBT_UP_SH * RBT_UP_SW) {
    const int r = e / RBT_UP_SW, c = e - r * RBT_UP_SW;
    const int sy = cl_clamp(cy0 - 2 + r, 0, ch - 1), sx = cl_clamp(cx0 - 1 + c, 0, cw - 1);
    L->src[r * RBT_UP_STRIDE + c] = cl_to_float(src[(size_t)sy * cw + sx], 1, bd);
  }
  RBT_SYNC();
  RBT_BLK_FOR(e, RBT_UP_TH * RBT_UP_SW) {
    const int t = e / RBT_UP_SW, c = e - t * RBT_UP_SW, li = t >> 1;
    float s[5];
#pragma unroll
    for (int k = 0; k < 5; k++) s[k] = L->src[(li + k) * RBT_UP_STRIDE + c];
    L->tmp[t * RBT_UP_STRIDE + c] = cl_up_vertical(t & 1, s);
  }
  RBT_SYNC();
  RBT_BLK_FOR(t, RBT_UP_THREADS) {
    const int row = t >> 3, seg = t & 7, y = ty * RBT_UP_TH + row, x0 = tx * RBT_UP_TW + seg * 8;
    if (y < h && x0 < w) {
      RbtU16x8 r;
#pragma unroll
      for (int k = 0; k < 4; k++) {         // an even and an odd column per word
        const RBT_LDS_AS float* p = &L->tmp[row * RBT_UP_STRIDE + seg * 4 + k];
        r.w[k] = (uint32_t)cl_to_16(cl_up_horizontal(0, p[0], p[1], p[2], p[3]), 1) | (uint32_t)cl_to_16(cl_up_horizontal(1, p[0], p[1], p[2], p[3]), 1) << 16;
      }
      const size_t o = (size_t)y * w + x0;
      if (wide) *(RbtU16x8*)(dst + o) = r;
      else {
#pragma unroll
        for (int k = 0; k < 8; k++) if (x0 + k < w) dst[o + k] = (uint16_t)(r.w[k >> 1] >> (16 * (k & 1)));
      }
    }
  }
  RBT_SYNC();
}
// PCCImage::convertYUV420ToYUV444: sample i of plane `plane` of picture `frame`, values untouched
RBT_DEV void cl_replicate(const uint16_t* in, uint16_t* out, int w, int h, int frame, int plane, int i) {
  const size_t ys = (size_t)w * h; const int cw = w / 2, y = i / w, x = i - y * w;
  const uint16_t* f = in + (size_t)frame * (ys + ys / 2);
  out[((size_t)frame * 3 + plane) * ys + i] = plane ? f[ys + (size_t)(plane - 1) * cw * (h / 2) + (size_t)(y >> 1) * cw + (x >> 1)] : f[i];
}

// PCCPointSet3::convertYUV16ToRGB8 (PCCPointSet.h:133-166)
RBT_DEV void cl_yuv16_to_rgb8(const uint16_t* yuv, uint8_t* rgb) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double y1 = yuv[0], u1 = yuv[1], v1 = yuv[2];
  const double offset = 32768.0, scale = 65535.0, weight = 1.0 / scale;
  y1 = weight * y1; u1 = weight * (u1 - offset); v1 = weight * (v1 - offset);
  y1 = y1 > 0.0 ? y1 : 0.0; y1 = y1 < 1.0 ? y1 : 1.0;
  u1 = u1 > -0.5 ? u1 : -0.5; u1 = u1 < 0.5 ? u1 : 0.5;
  v1 = v1 > -0.5 ? v1 : -0.5; v1 = v1 < 0.5 ? v1 : 0.5;
  double c[3];
  c[0] = y1 + 1.57480 * v1;
  c[1] = y1 - 0.18733 * u1 - 0.46813 * v1;
  c[2] = y1 + 1.85563 * u1;
  for (int k = 0; k < 3; k++) { double r = __builtin_round(c[k] * 255); r = r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r); rgb[k] = (uint8_t)r; }
}

// ---- colour metric ----
// the slot of voxel id in the map, claimed if it is new (*fresh = 1)
RBT_DEV uint32_t cl_slot_claim(uint32_t* keys, int lg, uint32_t id, int* fresh) {
  const uint32_t mask = (1u << lg) - 1;
  for (uint32_t s = pc_hash_slot(id, lg);; s = (s + 1) & mask) {
#ifdef RBT_HOSTEMU
    const uint32_t old = keys[s]; if (old == 0) keys[s] = id + 1;
#else
    const uint32_t old = atomicCAS(&keys[s], 0u, id + 1);
#endif
    if (old == 0 || old == id + 1) { *fresh = old == 0; return s; }
  }
}
RBT_DEV uint32_t cl_slot_find(const uint32_t* keys, int lg, uint32_t id) {     // the voxel is known to be in the map (its bit is set in the volume)
  const uint32_t mask = (1u << lg) - 1;
  for (uint32_t s = pc_hash_slot(id, lg);; s = (s + 1) & mask) if (keys[s] == id + 1 || keys[s] == 0) return s;
}
// point i: its voxel's bit, slot, colour sums and count; returns 1 for the first point of a voxel
RBT_DEV int cl_insert(const RbtColSet* S, int i) {
  const int x = S->xyz[3 * i], y = S->xyz[3 * i + 1], z = S->xyz[3 * i + 2];
  int fresh; const uint32_t s = cl_slot_claim(S->keys, S->lg, pc_voxel_id(x, y, z), &fresh);
#ifdef RBT_HOSTEMU
  S->vol[pc_voxel_word(x, y, z)] |= 1u << (x & 31);
  for (int c = 0; c < 3; c++) S->acc[4 * s + c] += S->rgb[3 * i + c];
  S->acc[4 * s + 3]++;
#else
  atomicOr(&S->vol[pc_voxel_word(x, y, z)], 1u << (x & 31));
  for (int c = 0; c < 3; c++) atomicAdd(&S->acc[4 * s + c], (uint32_t)S->rgb[3 * i + c]);
  atomicAdd(&S->acc[4 * s + 3], 1u);
#endif
  return fresh;
}
// removeDuplicate (PCCPointSet.cpp:190-203): the colour of a voxel is sum / count per channel, in integer division
RBT_DEV void cl_merge(const RbtColSet* S, uint32_t s) {
  if (!S->keys[s]) return;
  const uint32_t n = S->acc[4 * s + 3];
  S->col[s] = (S->acc[4 * s] / n) | (S->acc[4 * s + 1] / n) << 8 | (S->acc[4 * s + 2] / n) << 16;
}
// the merged point in slot s of P against Q: e[0..2] = error terms of Y, U, V; returns 0 for an empty slot.
// Q's colour is the mean over ALL its merged points at exactly the nearest squared distance, rounded half up ((2 sum + n) / (2 n), PCCMetrics.cpp:140-154);
// the terms are the BT.709 rows of convertRGBtoYUVBT709 (:50-55) times 10000 applied to the RGB difference (the + 0.5 offsets cancel)
RBT_DEV int cl_error(const RbtColSet* P, const RbtColSet* Q, uint32_t s, long long e[3]) {
  if (!P->keys[s]) return 0;
  const uint32_t id = P->keys[s] - 1;
  const int x = (int)(id & (RBT_PCC_DIM - 1)), y = (int)((id >> RBT_PCC_BITS) & (RBT_PCC_DIM - 1)), z = (int)(id >> (2 * RBT_PCC_BITS));
  const uint32_t d2 = pc_nearest_d2(Q->vol, x, y, z);
  uint32_t sr = 0, sg = 0, sb = 0, n = 0;
  pc_for_ties(Q->vol, x, y, z, d2, [&](uint32_t qid) { const uint32_t c = Q->col[cl_slot_find(Q->keys, Q->lg, qid)]; sr += c & 255u; sg += (c >> 8) & 255u; sb += c >> 16; n++; });
  const uint32_t pc = P->col[s];
  const int dr = (int)(pc & 255u) - (int)((2 * sr + n) / (2 * n)), dg = (int)((pc >> 8) & 255u) - (int)((2 * sg + n) / (2 * n)), db = (int)(pc >> 16) - (int)((2 * sb + n) / (2 * n));
  e[0] = 2126 * dr + 7152 * dg + 722 * db;
  e[1] = -1146 * dr - 3854 * dg + 5000 * db;
  e[2] = 5000 * dr - 4542 * dg - 458 * db;
  return 1;
}

#ifdef RBT_HOSTEMU
// serial stand-ins of the launchers (the product's are in rbt_color.hip)
namespace rbtk {
inline void launch_up444(const uint16_t* yuv420, int w, int h, int bit_depth, int n_frames, int filter, uint16_t* yuv444) {
  static RbtUpLds lds;
  for (int f = 0; f < n_frames; f++) for (int c = 0; c < 3; c++) {
    if (filter == RBT_UPSAMPLE_REPLICATE) { for (int i = 0; i < w * h; i++) cl_replicate(yuv420, yuv444, w, h, f, c, i); continue; }
    for (int ty = 0; ty < (h + RBT_UP_TH - 1) / RBT_UP_TH; ty++) for (int tx = 0; tx < (w + RBT_UP_TW - 1) / RBT_UP_TW; tx++) cl_up_tile(yuv420, yuv444, w, h, bit_depth, f, c, tx, ty, &lds);
  }
}
inline void launch_yuv16_rgb8(const uint16_t* yuv, int n, uint8_t* rgb) { for (int i = 0; i < n; i++) cl_yuv16_to_rgb8(yuv + 3 * (size_t)i, rgb + 3 * (size_t)i); }
inline void launch_col_insert(const RbtColSet* S, uint32_t* n_unique) { for (int i = 0; i < S->n; i++) *n_unique += (uint32_t)cl_insert(S, i); }
inline void launch_col_merge(const RbtColSet* S) { for (uint32_t s = 0; s < (1u << S->lg); s++) cl_merge(S, s); }
inline void launch_col_dist(const RbtColSet* P, const RbtColSet* Q, unsigned long long* sse) {
  for (uint32_t s = 0; s < (1u << P->lg); s++) { long long e[3]; if (cl_error(P, Q, s, e)) for (int c = 0; c < 3; c++) sse[c] += (unsigned long long)(e[c] * e[c]); }
}
}  // namespace rbtk
#endif
