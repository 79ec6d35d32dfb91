// Kernel and launcher of the luma gather (rbt_cloudmaps.h).
#include <hip/hip_runtime.h>
#include "rbt_cloudmaps.h"

namespace rbtk {
hipStream_t current_stream();            // rbt_kernels.hip: the stream the host code selected (set_stream)
#define g_stream current_stream()

// blockIdx.y = picture, blockIdx.x * RBT_GM_WG + threadIdx.x = chunk; a picture smaller than the largest of the launch leaves its last lanes idle
__global__ void __launch_bounds__(RBT_GM_WG) k_gather_luma(const RbtGatherPic* pics) {
  gm_chunk(&pics[blockIdx.y], (int)(blockIdx.x * RBT_GM_WG + threadIdx.x));
}

void launch_gather_luma(const RbtGatherPic* pics, int n_pics, int max_chunks) {
  if (n_pics <= 0 || max_chunks <= 0) return;
  const unsigned groups = (unsigned)((max_chunks + RBT_GM_WG - 1) / RBT_GM_WG);
  for (int k = 0; k < n_pics; k += 32768) hipLaunchKernelGGL(k_gather_luma, dim3(groups, (unsigned)(n_pics - k < 32768 ? n_pics - k : 32768)), dim3(RBT_GM_WG), 0, g_stream, pics + k);
}
}  // namespace rbtk
