// Kernel and launcher of the level census (rbt_rate.h).
#include <hip/hip_runtime.h>
#include "rbt_rate.h"

namespace rbtk {
hipStream_t current_stream();            // rbt_kernels.hip: the stream the host code selected (set_stream)
#define g_stream current_stream()

// blockIdx.y = picture, blockIdx.x = tile of RBT_RATE_TILE_WORDS words; a picture smaller than the largest of the launch leaves its last workgroups idle
__global__ void __launch_bounds__(RBT_RATE_WG) k_level_census(const RbtCensusPic* pics) {
  __shared__ uint32_t bins[RBT_RATE_HIST_WORDS];
  rate_census_tile(&pics[blockIdx.y], (int)blockIdx.x, RBT_LDS_CAST(uint32_t, bins));
}

void launch_level_census(const RbtCensusPic* pics, int n_pics, int max_words) {
  if (n_pics <= 0 || max_words <= 0) return;
  const unsigned tiles = (unsigned)((max_words + RBT_RATE_TILE_WORDS - 1) / RBT_RATE_TILE_WORDS);
  for (int k = 0; k < n_pics; k += 32768) hipLaunchKernelGGL(k_level_census, dim3(tiles, (unsigned)(n_pics - k < 32768 ? n_pics - k : 32768)), dim3(RBT_RATE_WG), 0, g_stream, pics + k);
}
}  // namespace rbtk
