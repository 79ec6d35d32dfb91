// Host half of a transcode to a colour PSNR floor (include/rbt.h, "transcoding attributes to a colour PSNR floor"): D(q) of a trial from its frames' colour results and the
// floor's condition - the figure and the condition that make the floor's walk (rbt_floor_walk.h) the walk of a colour floor, as rbt_d1_walk.h has them for D1 - and, as
// rbt_d1_figures.h has them for D1 and D2, the float routine of the colour results with the figures of a patch ("colour PSNR per patch of the decoded cloud", "colour floors
// held patch by patch"). Plain host code without a device call, so that tests/color_floor_check.cpp and tests/patch_color_check.cpp can run it under the sanitizers next
// to the kernel bodies.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>
#include "../../include/rbt.h"

namespace rbt {
// The one float routine of the colour results (rbt_color_metric, rbt_score, rbt_score_pair_color and the figures per patch): mse in float from a double quotient,
// 10 log10f(1 / mse) (getPSNR(mse, 1.0)); mse 0 gives +inf
inline float color_mse(uint64_t sse, double n) { return (float)((double)sse / (2550000.0 * 2550000.0 * n)); }
inline float color_psnr(float mse) { return 10 * log10f(1.0f / mse); }
// the figures of a patch from its sums and counts (include/rbt.h, "colour PSNR per patch of the decoded cloud"): a direction without a point has mse 0, and so psnr +inf
inline void patch_color_finish(rbt_patch_color* o) {
  for (int c = 0; c < 3; c++) {
    o->mse_ab[c] = o->n_ab ? color_mse(o->sse_ab[c], (double)o->n_ab) : 0.0f; o->mse_ba[c] = o->n_ba ? color_mse(o->sse_ba[c], (double)o->n_ba) : 0.0f;
    const float pa = color_psnr(o->mse_ab[c]), pb = color_psnr(o->mse_ba[c]);
    o->mse[c] = o->mse_ab[c] > o->mse_ba[c] ? o->mse_ab[c] : o->mse_ba[c];
    o->psnr[c] = pa < pb ? pa : pb;
  }
}
// what the walk of the colour floors held patch by patch is told about a patch: the figure is (double)psnr[channel]; +inf meets any floor
inline double patch_color_figure(const rbt_patch_color& p, int channel) { return (double)p.psnr[channel]; }
inline bool patch_color_meets(const rbt_patch_color& p, int channel, int32_t floor_mdb) { return patch_color_figure(p, channel) >= floor_mdb / 1000.0; }
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
