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
// Index, search and walks are those of frame scoring (csrc/rbt_score.h); the slot look-ups they share with the transfer are below.
//   attribute transfer  the re-colouring of the points geometry smoothing moved (PCCDecoder.cpp:434-494 -> PCCPointSet3::transferColors16bitBP, PCCPointSet.cpp:1126-1485, with
//                  the CTC's arguments): the last section of this file
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

// ---- attribute transfer after geometry smoothing (rbt_transfer_colors; the definition is in include/rbt.h) ----
// Source S = the cloud before smoothing, target T = the cloud after it; both have a 1024^3-bit volume (csrc/rbt_pcc.h). S also has a hash map voxel -> (first, count)
// into sidx, the source indices bucketed by voxel and ascending inside a bucket (coincident points are all candidates); T has the D2 map voxel -> lowest index.
//   forward   one lane per moved point: cubic shells of growing radius around it in S's volume, one row of the shell (a run of bits along x) per step; the 8 best
//             (squared distance, index) pairs live in registers as 64-bit keys, inserted through an unrolled compare-exchange chain. The walk ends when 8 are held and
//             the 8th is closer than anything outside the shell can be; it gives up at RBT_TC_MAX_R and says so in the error word. Then the 8-term sums in double.
//   backward  one lane per entry (8 per moved point): the nearest target point as in D2 (nearest distance, then the lowest index over the tie set), the colour test,
//             and a count per target point. Lists are laid out by an atomic cursor (where a list lies does not matter, its order does), filled, and put into
//             (distance, entry) order by the lane that sums them: the order of every sum is the defined one, whatever order the lanes arrived in.
enum { RBT_TC_K = 8, RBT_TC_MAX_R = 64, RBT_TC_MAX_BUCKET = 256, RBT_TC_MAX_LIST = 1024 };    // the two insertion sorts run in one lane each: what they sort is capped
#define RBT_TC_NONE 0xFFFFFFFFu
enum { RBT_TC_SRC_CURSOR = 0, RBT_TC_N_MOVED, RBT_TC_LIST_CURSOR, RBT_TC_N_CHANGED, RBT_TC_ERR, RBT_TC_SCALARS = 16 };    // words of RbtTransfer.scal (zeroed beforehand)
// coordinate outside 0..1023; fewer than 8 source points within RBT_TC_MAX_R; more than RBT_TC_MAX_BUCKET coincident source points; a list of more than RBT_TC_MAX_LIST entries
enum { RBT_TC_ERR_RANGE = 1, RBT_TC_ERR_WALK = 2, RBT_TC_ERR_BUCKET = 3, RBT_TC_ERR_LIST = 4 };
struct RbtTransfer {
  const int16_t* sxyz; const uint16_t* syuv; int32_t ns, slg;
  uint32_t* svol; uint32_t* skeys; uint32_t* scnt; uint32_t* sfirst; uint32_t* sfill; uint32_t* sidx;     // skeys, scnt, sfill: 1 << slg words, zeroed; sidx: ns words
  const int16_t* txyz; uint16_t* tyuv; const uint8_t* moved; int32_t nt, tlg;                            // tyuv: the colours before, updated in place by the last kernel
  uint32_t* tvol; uint32_t* tkeys; uint32_t* tvals;                                                       // tkeys zeroed, tvals 0xFF (pc_hash_insert)
  uint32_t* mlist; int32_t cap;                                                                           // the moved points, in any order; cap = their number as the host knows it
  uint16_t* color1; uint32_t* ent; uint32_t* ev; uint32_t* ed;                                            // per moved point: forward colour; per entry: source index, target point, distance
  uint32_t* lcnt; uint32_t* lfirst; uint32_t* lfill; unsigned long long* lkey; uint32_t* lsrc;            // lcnt, lfill: nt words, zeroed; lkey / lsrc: 8 * cap
  uint32_t* scal;
};

namespace rbtk {
// dst[0..n) = src[0..n), 16-bit words, on the device
void launch_tc_copy(uint16_t* dst, const uint16_t* src, size_t n);
// the geometry smoothing's filter pass once more on the positions before smoothing (the cell arrays of G are as launch_sm_passes left them): moved[i] = the point moves
void launch_tc_flag(const RbtSmooth* G, const int16_t* xyz_before, const uint32_t* meta, uint8_t* moved);
// the whole stage; needs T->cap > 0. A point outside 0..1023 is left out of the indices and reported in the error word (a moved one is then missing from the list of
// moved points, so nothing walks from it): the kernels stay inside the volumes whatever the input
void launch_transfer(const RbtTransfer* T);
// yuv420: n_frames planar 4:2:0 pictures; yuv444: n_frames x 3 planes of w * h. filter: RBT_UPSAMPLE_F0 or RBT_UPSAMPLE_REPLICATE
void launch_up444(const uint16_t* yuv420, int w, int h, int bit_depth, int n_frames, int filter, uint16_t* yuv444);
void launch_yuv16_rgb8(const uint16_t* yuv, int n, uint8_t* rgb);
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

// ---- attribute transfer ----
RBT_DEV uint32_t tc_add(uint32_t* p, uint32_t v) {
#ifdef RBT_HOSTEMU
  const uint32_t o = *p; *p = o + v; return o;
#else
  return atomicAdd(p, v);
#endif
}
RBT_DEV void tc_fail(uint32_t* scal, uint32_t code) {
#ifdef RBT_HOSTEMU
  if (code > scal[RBT_TC_ERR]) scal[RBT_TC_ERR] = code;
#else
  atomicMax(&scal[RBT_TC_ERR], code);
#endif
}
RBT_DEV int tc_in_range(const int16_t* p) { return ((uint32_t)(int)p[0] | (uint32_t)(int)p[1] | (uint32_t)(int)p[2]) < (uint32_t)RBT_PCC_DIM; }
RBT_DEV uint32_t tc_n_moved(const RbtTransfer* T) { const uint32_t n = T->scal[RBT_TC_N_MOVED]; return n < (uint32_t)T->cap ? n : (uint32_t)T->cap; }
// pc_sm_filter on a copy of point i: 1 when the smoothing moves it
RBT_DEV int tc_flag(const RbtSmooth* G, const int16_t* xyz_before, const uint32_t* meta, int i) {
  int16_t out[3];
  return pc_sm_filter_point(G, xyz_before + 3 * (size_t)i, meta[i], out);
}
// source index, pass 1: the voxel's bit, its slot, one more point in it
RBT_DEV void tc_src_count(const RbtTransfer* T, int i) {
  const int16_t* p = T->sxyz + 3 * (size_t)i;
  if (!tc_in_range(p)) { tc_fail(T->scal, RBT_TC_ERR_RANGE); return; }
  int fresh; const uint32_t s = cl_slot_claim(T->skeys, T->slg, pc_voxel_id(p[0], p[1], p[2]), &fresh);
#ifdef RBT_HOSTEMU
  T->svol[pc_voxel_word(p[0], p[1], p[2])] |= 1u << (p[0] & 31);
#else
  atomicOr(&T->svol[pc_voxel_word(p[0], p[1], p[2])], 1u << (p[0] & 31));
#endif
  tc_add(&T->scnt[s], 1u);
}
// pass 2, per slot: where the voxel's bucket lies in sidx
RBT_DEV void tc_src_alloc(const RbtTransfer* T, uint32_t s) {
  if (!T->skeys[s]) return;
  T->sfirst[s] = tc_add(&T->scal[RBT_TC_SRC_CURSOR], T->scnt[s]);
  if (T->scnt[s] > RBT_TC_MAX_BUCKET) tc_fail(T->scal, RBT_TC_ERR_BUCKET);
}
// pass 3, per point: into its bucket, in the order of arrival
RBT_DEV void tc_src_scatter(const RbtTransfer* T, int i) {
  const int16_t* p = T->sxyz + 3 * (size_t)i;
  if (!tc_in_range(p)) return;
  const uint32_t s = cl_slot_find(T->skeys, T->slg, pc_voxel_id(p[0], p[1], p[2]));
  T->sidx[T->sfirst[s] + tc_add(&T->sfill[s], 1u)] = (uint32_t)i;
}
// pass 4, per slot: indices ascending inside the bucket (buckets hold a handful of points)
RBT_DEV void tc_src_sort(const RbtTransfer* T, uint32_t s) {
  if (!T->skeys[s]) return;
  uint32_t* a = T->sidx + T->sfirst[s]; const uint32_t n = T->scnt[s];
  if (n > RBT_TC_MAX_BUCKET) return;                                 // reported by tc_src_alloc: the call fails, nothing sorts a long bucket
  for (uint32_t i = 1; i < n; i++) { const uint32_t v = a[i]; uint32_t j = i; while (j > 0 && a[j - 1] > v) { a[j] = a[j - 1]; j--; } a[j] = v; }
}
// target index: the D2 map voxel -> lowest index, and the list of moved points
RBT_DEV void tc_tgt_insert(const RbtTransfer* T, int u) {
  const int16_t* p = T->txyz + 3 * (size_t)u;
  if (!tc_in_range(p)) { tc_fail(T->scal, RBT_TC_ERR_RANGE); return; }
#ifdef RBT_HOSTEMU
  T->tvol[pc_voxel_word(p[0], p[1], p[2])] |= 1u << (p[0] & 31);
#else
  atomicOr(&T->tvol[pc_voxel_word(p[0], p[1], p[2])], 1u << (p[0] & 31));
#endif
  pc_hash_insert(T->tkeys, T->tvals, T->tlg, pc_voxel_id(p[0], p[1], p[2]), (uint32_t)u);
  if (T->moved[u]) { const uint32_t m = tc_add(&T->scal[RBT_TC_N_MOVED], 1u); if (m < (uint32_t)T->cap) T->mlist[m] = (uint32_t)u; }
}
RBT_DEV uint16_t tc_round16(double v) { double r = __builtin_round(v); r = r < 0.0 ? 0.0 : (r > 65535.0 ? 65535.0 : r); return (uint16_t)r; }
// forward half for moved point number m: N(u), color1, the 8 entries
RBT_DEV void tc_forward(const RbtTransfer* T, uint32_t m) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (m >= tc_n_moved(T)) return;
  const uint32_t u = T->mlist[m];
  const int x = T->txyz[3 * (size_t)u], y = T->txyz[3 * (size_t)u + 1], z = T->txyz[3 * (size_t)u + 2];
  unsigned long long K[RBT_TC_K];                                    // (squared distance << 32 | source index), ascending; all ones = free
#pragma unroll
  for (int j = 0; j < RBT_TC_K; j++) K[j] = ~0ull;
  auto visit = [&](int xx, int yy, int zz, uint32_t d2) {
    if (d2 > (uint32_t)(K[RBT_TC_K - 1] >> 32)) return;
    const uint32_t s = cl_slot_find(T->skeys, T->slg, pc_voxel_id(xx, yy, zz));
    const uint32_t* a = T->sidx + T->sfirst[s]; const uint32_t n = T->scnt[s];
    for (uint32_t q = 0; q < n; q++) {
      unsigned long long k = (unsigned long long)d2 << 32 | a[q];
      if (k >= K[RBT_TC_K - 1]) break;                               // the bucket ascends: nothing behind this one fits either
#pragma unroll
      for (int j = 0; j < RBT_TC_K; j++) if (k < K[j]) { const unsigned long long t = K[j]; K[j] = k; k = t; }
    }
  };
  int found = 0;
  for (int r = 0; r <= RBT_TC_MAX_R; r++) {
    for (int dz = -r; dz <= r; dz++) {
      const int zz = z + dz; if (zz < 0 || zz >= RBT_PCC_DIM) continue;
      for (int dy = -r; dy <= r; dy++) {
        const int yy = y + dy; if (yy < 0 || yy >= RBT_PCC_DIM) continue;
        const uint32_t base = (uint32_t)(dz * dz + dy * dy);
        if (base > (uint32_t)(K[RBT_TC_K - 1] >> 32)) continue;
        const uint32_t* row = T->svol + pc_voxel_word(0, yy, zz);
        if (dz == -r || dz == r || dy == -r || dy == r) {            // on a face of the shell: the whole run x - r .. x + r, word by word
          const int lo = x - r < 0 ? 0 : x - r, hi = x + r >= RBT_PCC_DIM ? RBT_PCC_DIM - 1 : x + r;
          for (int w = lo >> 5; w <= hi >> 5; w++) {
            uint32_t bits = row[w];
            if (w == lo >> 5) bits &= 0xFFFFFFFFu << (lo & 31);
            if (w == hi >> 5) bits &= 0xFFFFFFFFu >> (31 - (hi & 31));
            while (bits) { const int xx = w * 32 + __builtin_ctz(bits); bits &= bits - 1; visit(xx, yy, zz, base + (uint32_t)((xx - x) * (xx - x))); }
          }
        } else {                                                     // inside: the two ends of the run
          if (x - r >= 0 && ((row[(x - r) >> 5] >> ((x - r) & 31)) & 1)) visit(x - r, yy, zz, base + (uint32_t)(r * r));
          if (x + r < RBT_PCC_DIM && ((row[(x + r) >> 5] >> ((x + r) & 31)) & 1)) visit(x + r, yy, zz, base + (uint32_t)(r * r));
        }
      }
    }
    // everything outside shell r is at least r + 1 away; a point at exactly the 8th distance could still win the tie with a lower index, hence "<"
    if (K[RBT_TC_K - 1] != ~0ull && (uint32_t)(K[RBT_TC_K - 1] >> 32) < (uint32_t)((r + 1) * (r + 1))) { found = 1; break; }
  }
  uint32_t* ent = T->ent + (size_t)RBT_TC_K * m; uint16_t* c1 = T->color1 + 3 * (size_t)m;
  if (!found) {
    tc_fail(T->scal, RBT_TC_ERR_WALK);
#pragma unroll
    for (int j = 0; j < RBT_TC_K; j++) ent[j] = RBT_TC_NONE;
    for (int k = 0; k < 3; k++) c1[k] = T->tyuv[3 * (size_t)u + k];
    return;
  }
#pragma unroll
  for (int j = 0; j < RBT_TC_K; j++) ent[j] = (uint32_t)K[j];
  if ((uint32_t)(K[0] >> 32) == 0) { for (int k = 0; k < 3; k++) c1[k] = T->syuv[3 * (size_t)(uint32_t)K[0] + k]; return; }
  double acc[3] = {0.0, 0.0, 0.0}, sw = 0.0;
#pragma unroll
  for (int j = 0; j < RBT_TC_K; j++) {
    const double w = 1.0 / ((double)(uint32_t)(K[j] >> 32) + 4.0); const uint16_t* c = T->syuv + 3 * (size_t)(uint32_t)K[j];
    for (int k = 0; k < 3; k++) acc[k] += (double)c[k] * w;
    sw += w;
  }
  for (int k = 0; k < 3; k++) c1[k] = tc_round16(acc[k] / sw);
}
// backward half for entry e: the nearest target point of the entry's source point, the colour test, one more entry in that point's list
RBT_DEV void tc_backward(const RbtTransfer* T, uint32_t e) {
  if (e / RBT_TC_K >= tc_n_moved(T)) return;
  T->ev[e] = RBT_TC_NONE;
  const uint32_t s = T->ent[e]; if (s == RBT_TC_NONE) return;
  const int x = T->sxyz[3 * (size_t)s], y = T->sxyz[3 * (size_t)s + 1], z = T->sxyz[3 * (size_t)s + 2];
  const uint32_t d2 = pc_nearest_d2(T->tvol, x, y, z);
  uint32_t v = RBT_TC_NONE;
  pc_for_ties(T->tvol, x, y, z, d2, [&](uint32_t id) { const uint32_t j = pc_hash_find(T->tkeys, T->tvals, T->tlg, id); if (j < v) v = j; });
  if (v == RBT_TC_NONE || !T->moved[v]) return;                      // the lists of points that did not move are never read
  for (int k = 0; k < 3; k++) { const int d = (int)T->syuv[3 * (size_t)s + k] - (int)T->tyuv[3 * (size_t)v + k]; if (d >= 40 || d <= -40) return; }
  T->ev[e] = v; T->ed[e] = d2;
  tc_add(&T->lcnt[v], 1u);
}
RBT_DEV void tc_list_alloc(const RbtTransfer* T, uint32_t m) {
  if (m >= tc_n_moved(T)) return;
  const uint32_t u = T->mlist[m];
  if (T->lcnt[u]) T->lfirst[u] = tc_add(&T->scal[RBT_TC_LIST_CURSOR], T->lcnt[u]);
  if (T->lcnt[u] > RBT_TC_MAX_LIST) tc_fail(T->scal, RBT_TC_ERR_LIST);
}
// key of a list entry: (distance, position in E); the moved points' index order is E's order, so u * 8 + j stands for the position
RBT_DEV void tc_list_scatter(const RbtTransfer* T, uint32_t e) {
  if (e / RBT_TC_K >= tc_n_moved(T)) return;
  const uint32_t v = T->ev[e]; if (v == RBT_TC_NONE) return;
  const uint32_t pos = T->lfirst[v] + tc_add(&T->lfill[v], 1u);
  T->lkey[pos] = (unsigned long long)T->ed[e] << 40 | ((unsigned long long)T->mlist[e / RBT_TC_K] * RBT_TC_K + e % RBT_TC_K);
  T->lsrc[pos] = T->ent[e];
}
// the new colour of moved point number m; returns 1 when it differs from the old one
RBT_DEV int tc_result(const RbtTransfer* T, uint32_t m) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (m >= tc_n_moved(T)) return 0;
  const uint32_t u = T->mlist[m], n = T->lcnt[u];
  if (n > RBT_TC_MAX_LIST) return 0;                                 // reported by tc_list_alloc
  uint16_t c[3];
  if (n == 0) { for (int k = 0; k < 3; k++) c[k] = T->color1[3 * (size_t)m + k]; }
  else if (n == 1) { const uint32_t s = T->lsrc[T->lfirst[u]]; for (int k = 0; k < 3; k++) c[k] = T->syuv[3 * (size_t)s + k]; }
  else {
    unsigned long long* key = T->lkey + T->lfirst[u]; uint32_t* src = T->lsrc + T->lfirst[u];
    for (uint32_t i = 1; i < n; i++) {
      const unsigned long long kv = key[i]; const uint32_t sv = src[i]; uint32_t j = i;
      while (j > 0 && key[j - 1] > kv) { key[j] = key[j - 1]; src[j] = src[j - 1]; j--; }
      key[j] = kv; src[j] = sv;
    }
    double acc[3] = {0.0, 0.0, 0.0}, sw = 0.0;
    for (uint32_t i = 0; i < n; i++) {
      const double w = 1.0 / (__builtin_sqrt((double)(uint32_t)(key[i] >> 40)) + 4.0); const uint16_t* sc = T->syuv + 3 * (size_t)src[i];
      for (int k = 0; k < 3; k++) acc[k] += (double)sc[k] * w;
      sw += w;
    }
    for (int k = 0; k < 3; k++) c[k] = tc_round16(acc[k] / sw);
  }
  uint16_t* t = T->tyuv + 3 * (size_t)u;
  const int changed = c[0] != t[0] || c[1] != t[1] || c[2] != t[2];
  for (int k = 0; k < 3; k++) t[k] = c[k];
  return changed;
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
inline void launch_tc_copy(uint16_t* dst, const uint16_t* src, size_t n) { memcpy(dst, src, 2 * n); }
inline void launch_tc_flag(const RbtSmooth* G, const int16_t* xyz_before, const uint32_t* meta, uint8_t* moved) { for (int i = 0; i < G->n_points; i++) moved[i] = (uint8_t)tc_flag(G, xyz_before, meta, i); }
inline void launch_transfer(const RbtTransfer* T) {
  const uint32_t slots = 1u << T->slg, nm = (uint32_t)T->cap;
  for (int i = 0; i < T->ns; i++) tc_src_count(T, i);
  for (uint32_t s = 0; s < slots; s++) tc_src_alloc(T, s);
  for (int i = 0; i < T->ns; i++) tc_src_scatter(T, i);
  for (uint32_t s = 0; s < slots; s++) tc_src_sort(T, s);
  for (int u = 0; u < T->nt; u++) tc_tgt_insert(T, u);
  for (uint32_t m = 0; m < nm; m++) tc_forward(T, m);
  for (uint32_t e = 0; e < RBT_TC_K * nm; e++) tc_backward(T, e);
  for (uint32_t m = 0; m < nm; m++) tc_list_alloc(T, m);
  for (uint32_t e = 0; e < RBT_TC_K * nm; e++) tc_list_scatter(T, e);
  for (uint32_t m = 0; m < nm; m++) T->scal[RBT_TC_N_CHANGED] += (uint32_t)tc_result(T, m);
}
}  // namespace rbtk
#endif
