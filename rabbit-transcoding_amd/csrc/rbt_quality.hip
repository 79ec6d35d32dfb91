// Kernels and launchers of the distortion sums (rbt_quality.h) and of the sums per CTB and per patch (rbt_ctbsse.h).
#include <hip/hip_runtime.h>
#include "rbt_quality.h"
#include "rbt_ctbsse.h"

namespace rbtk {
hipStream_t current_stream();            // rbt_kernels.hip: the stream the host code selected (set_stream)
#define g_stream current_stream()

// blockIdx.y = picture, blockIdx.x = tile of RBT_SSE_TILE_CHUNKS chunks; a picture smaller than the largest of the launch leaves its last workgroups idle
__global__ void __launch_bounds__(RBT_SSE_WG) k_picture_sse(const RbtSsePic* pics) {
  __shared__ uint64_t acc[RBT_SSE_WORDS];
  sse_tile(&pics[blockIdx.y], (int)blockIdx.x, RBT_LDS_CAST(uint64_t, acc));
}

void launch_picture_sse(const RbtSsePic* pics, int n_pics, int max_chunks) {
  if (n_pics <= 0 || max_chunks <= 0) return;
  const unsigned tiles = (unsigned)((max_chunks + RBT_SSE_TILE_CHUNKS - 1) / RBT_SSE_TILE_CHUNKS);
  for (int k = 0; k < n_pics; k += 32768) hipLaunchKernelGGL(k_picture_sse, dim3(tiles, (unsigned)(n_pics - k < 32768 ? n_pics - k : 32768)), dim3(RBT_SSE_WG), 0, g_stream, pics + k);
}

// blockIdx.y = picture, wave w of workgroup blockIdx.x = CTB 4 * blockIdx.x + w of its grid; a wave past the grid's end (a smaller picture of the launch, the last workgroup) is idle
__global__ void __launch_bounds__(RBT_CTBSSE_WG) k_ctb_sse(const RbtCtbSsePic* pics) {
  const RbtCtbSsePic* P = &pics[blockIdx.y];
  const int ctb = RBT_UNI(blockIdx.x * (RBT_CTBSSE_WG / 64) + (threadIdx.x >> 6));
  if (ctb >= P->w_ctb * P->h_ctb) return;      // (uniform over the wave)
  ctbsse_ctb(P, ctb);
}
// blockIdx.y = frame, wave w of workgroup blockIdx.x = triple 4 * blockIdx.x + w of the frame's n_rects + 2
__global__ void __launch_bounds__(RBT_CTBSSE_WG) k_patch_fold(const RbtFoldJob* jobs) {
  const RbtFoldJob* J = &jobs[blockIdx.y];
  const int r = RBT_UNI(blockIdx.x * (RBT_CTBSSE_WG / 64) + (threadIdx.x >> 6));
  if (r >= J->n_rects + 2) return;             // (uniform over the wave)
  ctbsse_fold(J, r);
}

void launch_ctb_sse(const RbtCtbSsePic* pics, int n_pics, int max_ctbs) {
  if (n_pics <= 0 || max_ctbs <= 0) return;
  const unsigned wgs = (unsigned)((max_ctbs + RBT_CTBSSE_WG / 64 - 1) / (RBT_CTBSSE_WG / 64));
  for (int k = 0; k < n_pics; k += 32768) hipLaunchKernelGGL(k_ctb_sse, dim3(wgs, (unsigned)(n_pics - k < 32768 ? n_pics - k : 32768)), dim3(RBT_CTBSSE_WG), 0, g_stream, pics + k);
}
void launch_patch_fold(const RbtFoldJob* jobs, int n_jobs, int max_rects) {
  if (n_jobs <= 0 || max_rects < 0) return;
  const unsigned wgs = (unsigned)((max_rects + 2 + RBT_CTBSSE_WG / 64 - 1) / (RBT_CTBSSE_WG / 64));
  for (int k = 0; k < n_jobs; k += 32768) hipLaunchKernelGGL(k_patch_fold, dim3(wgs, (unsigned)(n_jobs - k < 32768 ? n_jobs - k : 32768)), dim3(RBT_CTBSSE_WG), 0, g_stream, jobs + k);
}
}  // namespace rbtk
