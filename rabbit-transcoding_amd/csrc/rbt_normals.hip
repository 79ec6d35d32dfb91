// Kernels and launcher of the normal estimation (rbt_normals.h). Compiled with -ffp-contract=off like rbt_color.hip (Makefile): the eigen-solve rounds every product
// and every sum on its own, so that the GPU and the serial host emulation give the same bits.
#include <hip/hip_runtime.h>
#include "rbt_normals.h"

namespace rbtk {
hipStream_t current_stream();            // rbt_kernels.hip: the stream the host code selected (set_stream)
#define g_stream current_stream()

// one lane per point, in point order; 16 or 32 keys in registers (the default k = 16 pays for 16)
template <int KMAX> __global__ void __launch_bounds__(64) k_nm_estimate(RbtScoreCloud S, RbtNormals N) { const int i = (int)(blockIdx.x * 64 + threadIdx.x); if (i < S.n) nm_point<KMAX>(&S, &N, i); }
__global__ void __launch_bounds__(256) k_nm_spread(RbtScoreCloud S, RbtNormals N) { const int i = (int)(blockIdx.x * 256 + threadIdx.x); if (i < S.n) nm_spread(&S, &N, i); }

void launch_nm_estimate(const RbtScoreCloud* S, const RbtNormals* N) {
  if (S->n <= 0) return;
  const dim3 g((unsigned)((S->n + 63) / 64)), b(64);
  if (N->k <= 16) hipLaunchKernelGGL(k_nm_estimate<16>, g, b, 0, g_stream, *S, *N);
  else hipLaunchKernelGGL(k_nm_estimate<32>, g, b, 0, g_stream, *S, *N);
  hipLaunchKernelGGL(k_nm_spread, dim3((unsigned)((S->n + 255) / 256)), dim3(256), 0, g_stream, *S, *N);
}
}  // namespace rbtk
