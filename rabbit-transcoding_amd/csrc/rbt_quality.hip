// Kernel and launcher of the distortion sums (rbt_quality.h).
#include <hip/hip_runtime.h>
#include "rbt_quality.h"

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
}  // namespace rbtk
