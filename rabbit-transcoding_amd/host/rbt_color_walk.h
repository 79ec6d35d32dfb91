// Host half of a transcode to a colour PSNR floor (include/rbt.h, "transcoding attributes to a colour PSNR floor"): D(q) of a trial from its frames' colour results and the
// floor's condition - the figure and the condition that make the floor's walk (rbt_floor_walk.h) the walk of a colour floor, as rbt_d1_walk.h has them for D1. Plain host
// code without a device call, so that tests/color_floor_check.cpp can run it under the sanitizers next to the kernel bodies.
#pragma once
#include <cstdint>
#include <vector>
#include "../../include/rbt.h"

namespace rbt {
// per channel (Y, U, V): the minimum over the frames of (double)psnr[c], and their sum in frame order divided by their number; no frames: both 0
inline void color_stats(const rbt_color_result* f, int n, double mean[3], double least[3]) {
  for (int c = 0; c < 3; c++) {
    double sum = 0.0, lo = 0.0;
    for (int i = 0; i < n; i++) { const double p = (double)f[i].psnr[c]; sum += p; if (i == 0 || p < lo) lo = p; }
    mean[c] = n ? sum / n : 0.0; least[c] = lo;
  }
}
// stat: RBT_D1_MIN or RBT_D1_MEAN; channel: 0 Y, 1 U, 2 V
inline double color_figure(const std::vector<rbt_color_result>& frames, int stat, int channel) {
  double mean[3], least[3]; color_stats(frames.data(), (int)frames.size(), mean, least);
  return stat == RBT_D1_MEAN ? mean[channel] : least[channel];
}
inline bool color_meets(const std::vector<rbt_color_result>& frames, int stat, int channel, int32_t min_psnr_mdb) { return color_figure(frames, stat, channel) >= min_psnr_mdb / 1000.0; }   // (+inf meets any floor)
}  // namespace rbt
