// Host half of a transcode to a colour PSNR floor (include/rbt.h, "transcoding attributes to a colour PSNR floor"): D(q) of a trial from its frames' colour results, the
// floor's condition, and what makes the shared walk (rbt_qp_walk.h) the walk of a colour floor - the PSNR floor's probe (rbt_quality_walk.h) with D in place of the PSNR, as
// rbt_d1_walk.h has it for D1. Plain host code without a device call, so that tests/color_floor_check.cpp can run it under the sanitizers next to the kernel bodies.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include "../../include/rbt.h"
#include "rbt_qp_walk.h"

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

// The floor of one entry: a probe at q0 - the entry's own QP, clamped to the range - says where the walk starts, one QP further per dB the probe is above the floor.
// Trial: anything with a member `color`, the std::vector<rbt_color_result> of the trial's frames.
struct ColorGoal { int32_t floor_mdb = 0; int stat = RBT_D1_MIN, channel = 0, q0 = 0; bool probed = false; };
template <class Trial> inline void color_seed(QpWalk<Trial>& w, ColorGoal& g, int qp) { w.toward = 1; g.q0 = std::min(w.hi, std::max(w.lo, qp)); }
// false: the probe has not been tried, a round has to bring q0 alone; true: w.start is known and qp_walk_step can look
template <class Trial> inline bool color_probe(QpWalk<Trial>& w, ColorGoal& g) {
  const auto t = w.tried.find(g.q0);
  if (g.probed || t == w.tried.end()) return g.probed;
  const double p = color_figure(t->second.color, g.stat, g.channel);
  w.start = std::isinf(p) ? g.q0 : std::min(w.hi, std::max(w.lo, g.q0 + (int)(p - g.floor_mdb / 1000.0)));
  return g.probed = true;
}
template <class Trial> inline auto color_holds(const QpWalk<Trial>& w, const ColorGoal& g) {
  return [&w, &g](int q) { return color_meets(w.tried.find(q)->second.color, g.stat, g.channel, g.floor_mdb); };
}
}  // namespace rbt
