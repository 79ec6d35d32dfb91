// Kernels and launchers of the colour stages (rbt_color.h): 4:2:0 -> 4:4:4 up-conversion, YUV16 -> RGB8, colour metric, attribute transfer after geometry smoothing. A translation unit of its own because it is
// compiled with -ffp-contract=off (Makefile): the up-conversion and the RGB conversion must round every product and every sum on its own, as the reference's host code
// does, so that their output is the same bits everywhere. No __fmul_rn / __fadd_rn is needed on top of that; the bodies also carry `#pragma clang fp contract(off)`.
#include <hip/hip_runtime.h>
#include "rbt_color.h"
#include "rbt_score.h"

namespace rbtk {
hipStream_t current_stream();            // rbt_kernels.hip: the stream the host code selected (set_stream)
#define g_stream current_stream()

// grid: x = tile column, y = tile row, z = picture * 3 + plane. LDS per workgroup: sizeof(RbtUpLds), 7.7 KB (the 16-byte output word is built in registers).
__global__ void __launch_bounds__(RBT_UP_THREADS) k_up444(const uint16_t* in, uint16_t* out, int w, int h, int bd) {
  __shared__ RbtUpLds lds;
  const int f = (int)blockIdx.z / 3, c = (int)blockIdx.z - 3 * f;
  cl_up_tile(in, out, w, h, bd, f, c, (int)blockIdx.x, (int)blockIdx.y, RBT_LDS_CAST(RbtUpLds, &lds));
}
__global__ void __launch_bounds__(256) k_replicate(const uint16_t* in, uint16_t* out, int w, int h) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x), f = (int)blockIdx.y / 3, c = (int)blockIdx.y - 3 * f;
  if (i < w * h) cl_replicate(in, out, w, h, f, c, i);
}
__global__ void __launch_bounds__(256) k_yuv16_rgb8(const uint16_t* yuv, int n, uint8_t* rgb) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i < n) cl_yuv16_to_rgb8(yuv + 3 * (size_t)i, rgb + 3 * (size_t)i);
}

// sum of v over the workgroup's 256 threads, valid in thread 0: shuffles inside the wave, then the four waves through LDS
__device__ __forceinline__ unsigned long long col_block_sum(unsigned long long v, unsigned long long* part) {
  for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

// ---- attribute transfer (rbt_color.h): one lane per source point / hash slot / target point / moved point / entry; no LDS ----
__global__ void __launch_bounds__(256) k_tc_copy(uint16_t* dst, const uint16_t* src, size_t n) { const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i < n) dst[i] = src[i]; }
__global__ void __launch_bounds__(256) k_tc_flag(RbtSmooth G, const int16_t* xyz_before, const uint32_t* meta, uint8_t* moved) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i < G.n_points) moved[i] = (uint8_t)tc_flag(&G, xyz_before, meta, i);
}
__global__ void __launch_bounds__(256) k_tc_src_count(RbtTransfer T) { const int i = (int)(blockIdx.x * 256 + threadIdx.x); if (i < T.ns) tc_src_count(&T, i); }
__global__ void __launch_bounds__(256) k_tc_src_alloc(RbtTransfer T) { const uint32_t s = blockIdx.x * 256 + threadIdx.x; if (s < (1u << T.slg)) tc_src_alloc(&T, s); }
__global__ void __launch_bounds__(256) k_tc_src_scatter(RbtTransfer T) { const int i = (int)(blockIdx.x * 256 + threadIdx.x); if (i < T.ns) tc_src_scatter(&T, i); }
__global__ void __launch_bounds__(256) k_tc_src_sort(RbtTransfer T) { const uint32_t s = blockIdx.x * 256 + threadIdx.x; if (s < (1u << T.slg)) tc_src_sort(&T, s); }
__global__ void __launch_bounds__(256) k_tc_tgt_insert(RbtTransfer T) { const int u = (int)(blockIdx.x * 256 + threadIdx.x); if (u < T.nt) tc_tgt_insert(&T, u); }
// 64 lanes per workgroup: the walks of neighbouring moved points differ in length, and a short workgroup frees its slot sooner
__global__ void __launch_bounds__(64) k_tc_forward(RbtTransfer T) { tc_forward(&T, blockIdx.x * 64 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_tc_backward(RbtTransfer T) { tc_backward(&T, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_tc_list_alloc(RbtTransfer T) { tc_list_alloc(&T, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_tc_list_scatter(RbtTransfer T) { tc_list_scatter(&T, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_tc_result(RbtTransfer T) { if (tc_result(&T, blockIdx.x * 256 + threadIdx.x)) atomicAdd(&T.scal[RBT_TC_N_CHANGED], 1u); }

// ---- frame scoring on device clouds (rbt_score.h) ----
__device__ __forceinline__ uint32_t sc_block_max(uint32_t v, uint32_t* part) {     // as col_block_sum
  for (int o = 32; o > 0; o >>= 1) { const uint32_t w = (uint32_t)__shfl_xor((int)v, o); v = w > v ? w : v; }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  const uint32_t a = part[0] > part[1] ? part[0] : part[1], b = part[2] > part[3] ? part[2] : part[3];
  return a > b ? a : b;
}
__global__ void __launch_bounds__(256) k_sc_check(const int16_t* xyz, int n, uint32_t* scal) {
  __shared__ unsigned long long part[4];
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  const unsigned long long bad = col_block_sum(i < n && !tc_in_range(xyz + 3 * (size_t)i) ? 1ull : 0ull, part);
  if (threadIdx.x == 0 && bad) atomicOr(&scal[RBT_SC_ERR], 1u);
}
__global__ void __launch_bounds__(256) k_sc_insert(RbtScoreCloud S, uint32_t* scal) {
  __shared__ unsigned long long part[4];
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  const unsigned long long n = col_block_sum(i < S.n ? (unsigned long long)sc_insert(&S, i) : 0ull, part);
  if (threadIdx.x == 0 && n) atomicAdd(&scal[RBT_SC_N_MERGED], (uint32_t)n);
}
__global__ void __launch_bounds__(256) k_sc_merge(RbtScoreCloud S) { const uint32_t s = blockIdx.x * 256 + threadIdx.x; if (s < (1u << S.lg)) sc_merge(&S, s); }
__global__ void __launch_bounds__(256) k_sc_clear(RbtScoreCloud S) { const int i = (int)(blockIdx.x * 256 + threadIdx.x); if (i < S.n) sc_clear(&S, i); }
// 64 lanes per workgroup, as k_tc_forward: the searches of a wave's points differ in length
__global__ void __launch_bounds__(64) k_sc_search(RbtScoreCloud P, RbtScoreCloud Q, uint32_t* dist) { const int i = (int)(blockIdx.x * 64 + threadIdx.x); if (i < P.n) sc_search(&P, &Q, dist, i); }
// dir 0: A -> B, 1: B -> A (P is the walking cloud). Integer sums: reduced in the workgroup, then one atomic per workgroup and sum
__global__ void __launch_bounds__(256) k_sc_walk(RbtScoreCloud A, RbtScoreCloud B, RbtScoreWork W, int parts, int dir) {
  __shared__ unsigned long long part[4][4]; __shared__ uint32_t pmax[4];
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  uint32_t d = 0; long long e[3] = {0, 0, 0};
  if (i < (dir ? B.n : A.n)) { if (dir) sc_walk_ba(&B, &A, &W, parts, i, &d, e); else sc_walk_ab(&A, &B, &W, parts, i, &d, e); }
  const unsigned long long sd = col_block_sum(d, part[3]);
  if (threadIdx.x == 0 && sd) atomicAdd(&W.res[RBT_SC_D1_AB + dir], sd);
  const uint32_t md = sc_block_max(d, pmax);
  if (threadIdx.x == 0 && md) atomicMax((uint32_t*)&W.res[RBT_SC_D1_MAX] + dir, md);
  if (parts & RBT_SCORE_COLOR)
    for (int c = 0; c < 3; c++) {
      const unsigned long long t = col_block_sum((unsigned long long)(e[c] * e[c]), part[c]);
      if (threadIdx.x == 0 && t) atomicAdd(&W.res[(dir ? RBT_SC_COL_BA : RBT_SC_COL_AB) + c], t);
    }
}
// recolouring (rbt_pcloud_set_colors): per slot, per point; the merge behind them is k_sc_merge
__global__ void __launch_bounds__(256) k_sc_recolor_zero(RbtScoreCloud S) { const uint32_t s = blockIdx.x * 256 + threadIdx.x; if (s < (1u << S.lg)) sc_recolor_zero(&S, s); }
__global__ void __launch_bounds__(256) k_sc_recolor_add(RbtScoreCloud S) { const int i = (int)(blockIdx.x * 256 + threadIdx.x); if (i < S.n) sc_recolor_add(&S, i); }
// the colour sums of k_sc_walk from the distances a score pair keeps; dir 0: A -> B into res[0..2], 1: B -> A into res[3..5]
__global__ void __launch_bounds__(256) k_sc_color_walk(RbtScoreCloud A, RbtScoreCloud B, const uint32_t* dist_a, const uint32_t* dist_b, unsigned long long* res, int dir) {
  __shared__ unsigned long long part[3][4];
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  long long e[3] = {0, 0, 0};
  if (i < (dir ? B.n : A.n)) sc_color_walk(&A, &B, dist_a, dist_b, dir, i, e);
  for (int c = 0; c < 3; c++) {
    const unsigned long long t = col_block_sum((unsigned long long)(e[c] * e[c]), part[c]);
    if (threadIdx.x == 0 && t) atomicAdd(&res[3 * dir + c], t);
  }
}
__global__ void __launch_bounds__(256) k_sc_d2_ab(RbtScoreCloud A, RbtScoreCloud B, RbtScoreWork W) { const int i = (int)(blockIdx.x * 256 + threadIdx.x); if (i < A.n) sc_d2_ab(&A, &B, &W, i); }
__global__ void __launch_bounds__(RBT_SC_SUM) k_sc_sum_block(const double* val, int n, double* part) {
  __shared__ RbtScoreSumLds lds;
  sc_sum_block(val, n, (int)blockIdx.x, part, RBT_LDS_CAST(RbtScoreSumLds, &lds));
}
__global__ void __launch_bounds__(RBT_SC_SUM) k_sc_sum_final(const double* part, int n_blocks, double* out) {
  __shared__ RbtScoreSumLds lds;
  sc_sum_final(part, n_blocks, out, RBT_LDS_CAST(RbtScoreSumLds, &lds));
}
// ---- D1 per patch (rbt_score.h) ----
// one wave per work item: its points are a contiguous run of the cloud
__global__ void __launch_bounds__(64) k_pd_labels(const uint32_t* items, const uint32_t* offsets, uint32_t* labels) { pd_label_item(items, offsets, (int)blockIdx.x, (int)threadIdx.x, 64, labels); }
__global__ void __launch_bounds__(256) k_pd_check(const uint32_t* labels, int n, uint32_t n_patches, uint32_t* err) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (__ballot(i < n && labels[i] >= n_patches) && (threadIdx.x & 63) == 0) atomicOr(err, 1u);
}
// dir 0: one lane per point of A, 1: per point of B. No LDS: every wave adds on its own. A wave whose terms all carry one label - the rule, since points come in patch
// order - folds them with shuffles and lane 0 issues one atomic per word; a mixed wave issues them per lane. Integer atomics: the words do not depend on the order.
__global__ void __launch_bounds__(256) k_pd_sums(RbtScoreCloud A, RbtScoreCloud B, const uint32_t* labels_b, const uint32_t* dist_a, const uint32_t* dist_b, unsigned long long* out, int dir) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  uint32_t label = 0, d = 0; int valid = 0;
  if (i < (dir ? B.n : A.n)) valid = dir ? pd_term_ba(labels_b, dist_b, i, &label, &d) : pd_term_ab(&A, &B, labels_b, dist_a, i, &label, &d);
  const unsigned long long act = __ballot(valid);
  if (!act) return;                                                     // uniform over the wave
  const uint32_t first = (uint32_t)__shfl((int)label, __ffsll((long long)act) - 1);
  if (__ballot(valid && label != first) == 0) {
    unsigned long long s = valid ? d : 0; uint32_t m = valid ? d : 0;
    for (int o = 32; o > 0; o >>= 1) { s += (unsigned long long)__shfl_xor((long long)s, o); const uint32_t w = (uint32_t)__shfl_xor((int)m, o); m = w > m ? w : m; }
    if ((threadIdx.x & 63) == 0) pd_add(out, first, dir, s, (unsigned long long)__popcll(act), m);
  } else if (valid) pd_add(out, label, dir, d, 1, d);
}
// ---- D2 per patch (rbt_score.h) ----
// one workgroup per 256 entries of the walking cloud. LDS per workgroup: sizeof(RbtPatchD2Lds), 8 KB
__global__ void __launch_bounds__(RBT_SC_SUM) k_p2_block(RbtScoreCloud A, RbtScoreCloud B, const uint32_t* labels_b, RbtScoreWork W, RbtPatchD2Work P, unsigned long long* out, int dir) {
  __shared__ RbtPatchD2Lds lds;
  p2_block(&A, &B, labels_b, &W, &P, out, dir, (int)blockIdx.x, RBT_LDS_CAST(RbtPatchD2Lds, &lds));
}
// one workgroup: lane t owns column t of S
__global__ void __launch_bounds__(RBT_SC_SUM) k_p2_cols(RbtPatchD2Work P, int n_blocks) { p2_cols(&P, n_blocks, (int)threadIdx.x); }
// one workgroup per patch
__global__ void __launch_bounds__(RBT_SC_SUM) k_p2_fold(RbtPatchD2Work P, unsigned long long* out, int dir) {
  __shared__ RbtScoreSumLds lds;
  p2_fold(&P, out, dir, (int)blockIdx.x, RBT_LDS_CAST(RbtScoreSumLds, &lds));
}
// ---- colour per patch (rbt_score.h) ----
// dir 0: one lane per point of A, 1: per point of B; in place of k_sc_color_walk. No LDS: every wave adds on its own, as in k_pd_sums. A wave whose terms all carry one
// label folds the three squares with shuffles and lane 0 issues one atomic per non-zero word; a mixed wave issues them per lane. Integer atomics only.
__global__ void __launch_bounds__(256) k_pc_sums(RbtScoreCloud A, RbtScoreCloud B, const uint32_t* labels_b, const uint32_t* dist_a, const uint32_t* dist_b, unsigned long long* out, int dir) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  uint32_t label = 0; long long e[3] = {0, 0, 0}; int valid = 0;
  if (i < (dir ? B.n : A.n)) valid = pc_term(&A, &B, labels_b, dist_a, dist_b, dir, i, &label, e);
  const unsigned long long act = __ballot(valid);
  if (!act) return;                                                     // uniform over the wave
  unsigned long long sq[3];
  for (int c = 0; c < 3; c++) sq[c] = valid ? (unsigned long long)(e[c] * e[c]) : 0;
  const uint32_t first = (uint32_t)__shfl((int)label, __ffsll((long long)act) - 1);
  if (__ballot(valid && label != first) == 0) {
    for (int o = 32; o > 0; o >>= 1) for (int c = 0; c < 3; c++) sq[c] += (unsigned long long)__shfl_xor((long long)sq[c], o);
    if ((threadIdx.x & 63) == 0) pc_add(out, first, dir, sq, (unsigned long long)__popcll(act));
  } else if (valid) pc_add(out, label, dir, sq, 1);
}

void launch_up444(const uint16_t* yuv420, int w, int h, int bit_depth, int n_frames, int filter, uint16_t* yuv444) {
  if (n_frames <= 0) return;
  if (filter == RBT_UPSAMPLE_REPLICATE) hipLaunchKernelGGL(k_replicate, dim3((unsigned)((w * h + 255) / 256), 3u * (unsigned)n_frames), dim3(256), 0, g_stream, yuv420, yuv444, w, h);
  else hipLaunchKernelGGL(k_up444, dim3((unsigned)((w + RBT_UP_TW - 1) / RBT_UP_TW), (unsigned)((h + RBT_UP_TH - 1) / RBT_UP_TH), 3u * (unsigned)n_frames), dim3(RBT_UP_THREADS), 0, g_stream,
                          yuv420, yuv444, w, h, bit_depth);
}
void launch_yuv16_rgb8(const uint16_t* yuv, int n, uint8_t* rgb) { if (n > 0) hipLaunchKernelGGL(k_yuv16_rgb8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g_stream, yuv, n, rgb); }
void launch_tc_copy(uint16_t* dst, const uint16_t* src, size_t n) { if (n) hipLaunchKernelGGL(k_tc_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g_stream, dst, src, n); }
void launch_tc_flag(const RbtSmooth* G, const int16_t* xyz_before, const uint32_t* meta, uint8_t* moved) {
  if (G->n_points > 0) hipLaunchKernelGGL(k_tc_flag, dim3((unsigned)((G->n_points + 255) / 256)), dim3(256), 0, g_stream, *G, xyz_before, meta, moved);
}
void launch_transfer(const RbtTransfer* T) {
  if (T->cap <= 0 || T->ns <= 0 || T->nt <= 0) return;
  const dim3 b(256), gs((unsigned)((T->ns + 255) / 256)), gh((unsigned)(((1u << T->slg) + 255) / 256)), gt((unsigned)((T->nt + 255) / 256)), gm((unsigned)((T->cap + 255) / 256)),
             ge((unsigned)(((size_t)RBT_TC_K * T->cap + 255) / 256));
  hipLaunchKernelGGL(k_tc_src_count, gs, b, 0, g_stream, *T);
  hipLaunchKernelGGL(k_tc_src_alloc, gh, b, 0, g_stream, *T);
  hipLaunchKernelGGL(k_tc_src_scatter, gs, b, 0, g_stream, *T);
  hipLaunchKernelGGL(k_tc_src_sort, gh, b, 0, g_stream, *T);
  hipLaunchKernelGGL(k_tc_tgt_insert, gt, b, 0, g_stream, *T);
  hipLaunchKernelGGL(k_tc_forward, dim3((unsigned)((T->cap + 63) / 64)), dim3(64), 0, g_stream, *T);
  hipLaunchKernelGGL(k_tc_backward, ge, b, 0, g_stream, *T);
  hipLaunchKernelGGL(k_tc_list_alloc, gm, b, 0, g_stream, *T);
  hipLaunchKernelGGL(k_tc_list_scatter, ge, b, 0, g_stream, *T);
  hipLaunchKernelGGL(k_tc_result, gm, b, 0, g_stream, *T);
}
void launch_sc_check(const int16_t* xyz, int n, uint32_t* scal) { if (n > 0) hipLaunchKernelGGL(k_sc_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g_stream, xyz, n, scal); }
void launch_sc_index(const RbtScoreCloud* S, uint32_t* scal) {
  if (S->n <= 0) return;
  hipLaunchKernelGGL(k_sc_insert, dim3((unsigned)((S->n + 255) / 256)), dim3(256), 0, g_stream, *S, scal);
  if (S->rgb) hipLaunchKernelGGL(k_sc_merge, dim3((unsigned)(((1u << S->lg) + 255) / 256)), dim3(256), 0, g_stream, *S);
}
void launch_sc_clear(const RbtScoreCloud* S) { if (S->n > 0) hipLaunchKernelGGL(k_sc_clear, dim3((unsigned)((S->n + 255) / 256)), dim3(256), 0, g_stream, *S); }
void launch_sc_score(const RbtScoreCloud* A, const RbtScoreCloud* B, int parts, const RbtScoreWork* W) {
  if (A->n <= 0 || B->n <= 0) return;
  const dim3 b(256), ga((unsigned)((A->n + 255) / 256)), gb((unsigned)((B->n + 255) / 256));
  hipLaunchKernelGGL(k_sc_search, dim3((unsigned)((A->n + 63) / 64)), dim3(64), 0, g_stream, *A, *B, W->dist_a);
  hipLaunchKernelGGL(k_sc_search, dim3((unsigned)((B->n + 63) / 64)), dim3(64), 0, g_stream, *B, *A, W->dist_b);
  hipLaunchKernelGGL(k_sc_walk, ga, b, 0, g_stream, *A, *B, *W, parts, 0);
  hipLaunchKernelGGL(k_sc_walk, gb, b, 0, g_stream, *A, *B, *W, parts, 1);
  if (!(parts & RBT_SCORE_D2)) return;
  hipLaunchKernelGGL(k_sc_d2_ab, ga, b, 0, g_stream, *A, *B, *W);
  for (int dir = 0; dir < 2; dir++) {
    const int n = dir ? B->n : A->n, nb = (n + RBT_SC_SUM - 1) / RBT_SC_SUM;
    hipLaunchKernelGGL(k_sc_sum_block, dim3((unsigned)nb), dim3(RBT_SC_SUM), 0, g_stream, dir ? W->val_ba : W->val_ab, n, W->part);
    hipLaunchKernelGGL(k_sc_sum_final, dim3(1), dim3(RBT_SC_SUM), 0, g_stream, W->part, nb, (double*)&W->res[dir ? RBT_SC_D2_BA : RBT_SC_D2_AB]);
  }
}
void launch_sc_recolor(const RbtScoreCloud* S) {
  if (S->n <= 0 || !S->rgb) return;
  const dim3 b(256), gs((unsigned)(((1u << S->lg) + 255) / 256));
  hipLaunchKernelGGL(k_sc_recolor_zero, gs, b, 0, g_stream, *S);
  hipLaunchKernelGGL(k_sc_recolor_add, dim3((unsigned)((S->n + 255) / 256)), b, 0, g_stream, *S);
  hipLaunchKernelGGL(k_sc_merge, gs, b, 0, g_stream, *S);
}
void launch_sc_search(const RbtScoreCloud* A, const RbtScoreCloud* B, uint32_t* dist_a, uint32_t* dist_b) {
  if (A->n <= 0 || B->n <= 0) return;
  hipLaunchKernelGGL(k_sc_search, dim3((unsigned)((A->n + 63) / 64)), dim3(64), 0, g_stream, *A, *B, dist_a);
  hipLaunchKernelGGL(k_sc_search, dim3((unsigned)((B->n + 63) / 64)), dim3(64), 0, g_stream, *B, *A, dist_b);
}
void launch_sc_color_walks(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* dist_a, const uint32_t* dist_b, unsigned long long* res) {
  if (A->n <= 0 || B->n <= 0) return;
  hipLaunchKernelGGL(k_sc_color_walk, dim3((unsigned)((A->n + 255) / 256)), dim3(256), 0, g_stream, *A, *B, dist_a, dist_b, res, 0);
  hipLaunchKernelGGL(k_sc_color_walk, dim3((unsigned)((B->n + 255) / 256)), dim3(256), 0, g_stream, *A, *B, dist_a, dist_b, res, 1);
}
void launch_pd_labels(const uint32_t* items, const uint32_t* offsets, int n_items, uint32_t* labels) {
  if (n_items > 0) hipLaunchKernelGGL(k_pd_labels, dim3((unsigned)n_items), dim3(64), 0, g_stream, items, offsets, labels);
}
void launch_pd_check(const uint32_t* labels, int n, uint32_t n_patches, uint32_t* err) {
  if (n > 0) hipLaunchKernelGGL(k_pd_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g_stream, labels, n, n_patches, err);
}
void launch_pd_sums(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* labels_b, const uint32_t* dist_a, const uint32_t* dist_b, unsigned long long* out) {
  if (A->n <= 0 || B->n <= 0) return;
  hipLaunchKernelGGL(k_pd_sums, dim3((unsigned)((A->n + 255) / 256)), dim3(256), 0, g_stream, *A, *B, labels_b, dist_a, dist_b, out, 0);
  hipLaunchKernelGGL(k_pd_sums, dim3((unsigned)((B->n + 255) / 256)), dim3(256), 0, g_stream, *A, *B, labels_b, dist_a, dist_b, out, 1);
}
void launch_p2_sums(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* labels_b, const RbtScoreWork* W, const RbtPatchD2Work* P, int n_patches, unsigned long long* out) {
  if (A->n <= 0 || B->n <= 0 || n_patches <= 0) return;
  for (int dir = 0; dir < 2; dir++) {
    const int n = dir ? B->n : A->n, nb = (n + RBT_SC_SUM - 1) / RBT_SC_SUM;
    hipLaunchKernelGGL(k_p2_block, dim3((unsigned)nb), dim3(RBT_SC_SUM), 0, g_stream, *A, *B, labels_b, *W, *P, out, dir);
    hipLaunchKernelGGL(k_p2_cols, dim3(1), dim3(RBT_SC_SUM), 0, g_stream, *P, nb);
    hipLaunchKernelGGL(k_p2_fold, dim3((unsigned)n_patches), dim3(RBT_SC_SUM), 0, g_stream, *P, out, dir);
  }
}
void launch_pc_sums(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* labels_b, const uint32_t* dist_a, const uint32_t* dist_b, unsigned long long* out) {
  if (A->n <= 0 || B->n <= 0) return;
  hipLaunchKernelGGL(k_pc_sums, dim3((unsigned)((A->n + 255) / 256)), dim3(256), 0, g_stream, *A, *B, labels_b, dist_a, dist_b, out, 0);
  hipLaunchKernelGGL(k_pc_sums, dim3((unsigned)((B->n + 255) / 256)), dim3(256), 0, g_stream, *A, *B, labels_b, dist_a, dist_b, out, 1);
}
}  // namespace rbtk
