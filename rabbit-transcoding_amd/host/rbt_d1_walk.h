// Host half of a transcode to a D1 floor (include/rbt.h, "transcoding geometry to a D1 floor"): D(q) of a trial from its frames' D1 results, the floor's condition, and
// what makes the shared walk (rbt_qp_walk.h) the walk of a D1 floor - the PSNR floor's probe (rbt_quality_walk.h) with D in place of the PSNR. Plain host code without a
// device call, so that tests/d1_check.cpp can run it under the sanitizers next to the gather kernel's body.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include "../../include/rbt.h"
#include "rbt_qp_walk.h"

namespace rbt {
// the minimum over the frames of (double)psnr, and their sum in frame order divided by their number; no frames: both 0
inline void d1_stats(const rbt_d1_result* f, int n, double* mean, double* least) {
  double sum = 0.0, lo = 0.0;
  for (int i = 0; i < n; i++) { const double p = (double)f[i].psnr; sum += p; if (i == 0 || p < lo) lo = p; }
  *mean = n ? sum / n : 0.0; *least = lo;
}
// stat: RBT_D1_MIN or RBT_D1_MEAN
inline double d1_figure(const std::vector<rbt_d1_result>& frames, int stat) { double mean, least; d1_stats(frames.data(), (int)frames.size(), &mean, &least); return stat == RBT_D1_MEAN ? mean : least; }
inline bool d1_meets(const std::vector<rbt_d1_result>& frames, int stat, int32_t min_d1_mdb) { return d1_figure(frames, stat) >= min_d1_mdb / 1000.0; }      // (+inf meets any floor)

// The floor of one entry: a probe at q0 - the entry's own QP, clamped to the range - says where the walk starts, one QP further per dB the probe is above the floor.
// Trial: anything with a member `d1`, the std::vector<rbt_d1_result> of the trial's frames.
struct D1Goal { int32_t floor_mdb = 0; int stat = RBT_D1_MIN, q0 = 0; bool probed = false; };
template <class Trial> inline void d1_seed(QpWalk<Trial>& w, D1Goal& g, int qp) { w.toward = 1; g.q0 = std::min(w.hi, std::max(w.lo, qp)); }
// false: the probe has not been tried, a round has to bring q0 alone; true: w.start is known and qp_walk_step can look
template <class Trial> inline bool d1_probe(QpWalk<Trial>& w, D1Goal& g) {
  const auto t = w.tried.find(g.q0);
  if (g.probed || t == w.tried.end()) return g.probed;
  const double p = d1_figure(t->second.d1, g.stat);
  w.start = std::isinf(p) ? g.q0 : std::min(w.hi, std::max(w.lo, g.q0 + (int)(p - g.floor_mdb / 1000.0)));
  return g.probed = true;
}
template <class Trial> inline auto d1_holds(const QpWalk<Trial>& w, const D1Goal& g) { return [&w, &g](int q) { return d1_meets(w.tried.find(q)->second.d1, g.stat, g.floor_mdb); }; }
}  // namespace rbt
