// Host half of a transcode to a D1 floor (include/rbt.h, "transcoding geometry to a D1 floor"): D(q) of a trial from its frames' D1 results and the floor's condition -
// the figure and the condition that make the floor's walk (rbt_floor_walk.h) the walk of a D1 floor. Plain host code without a device call, so that tests/d1_check.cpp can
// run it under the sanitizers next to the gather kernel's body.
#pragma once
#include <cstdint>
#include <vector>
#include "../../include/rbt.h"

namespace rbt {
// the minimum over the frames of (double)psnr, and their sum in frame order divided by their number; no frames: both 0. Result: rbt_d1_result, or rbt_d2_result for a D2 floor
template <class Result> inline void d1_stats(const Result* f, int n, double* mean, double* least) {
  double sum = 0.0, lo = 0.0;
  for (int i = 0; i < n; i++) { const double p = (double)f[i].psnr; sum += p; if (i == 0 || p < lo) lo = p; }
  *mean = n ? sum / n : 0.0; *least = lo;
}
// stat: RBT_D1_MIN or RBT_D1_MEAN
template <class Result> inline double d1_figure(const std::vector<Result>& frames, int stat) { double mean, least; d1_stats(frames.data(), (int)frames.size(), &mean, &least); return stat == RBT_D1_MEAN ? mean : least; }
template <class Result> inline bool d1_meets(const std::vector<Result>& frames, int stat, int32_t min_d1_mdb) { return d1_figure(frames, stat) >= min_d1_mdb / 1000.0; }      // (+inf meets any floor)
}  // namespace rbt
