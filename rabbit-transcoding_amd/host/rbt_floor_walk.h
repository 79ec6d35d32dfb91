// What makes the shared walk (rbt_qp_walk.h) the walk of a floor, whatever the floor is on - the PSNR of the pictures (rbt_quality_walk.h), D1 of the rebuilt clouds
// (rbt_d1_walk.h) or their colour PSNR (rbt_color_walk.h): a probe in front of the walk, and the floor's condition on a trial. The metric comes in as two callables on a
// trial: figure(trial), its dB figure as a double, which only the probe reads, and meets(trial), the floor's condition, which the walk reads. They stay two things: a PSNR
// floor is met by a region without samples, whose figure is 0. Plain host code without a device call, so that the stand-alone check programs of the three metrics
// (tests/quality_check.cpp, d1_check.cpp, color_floor_check.cpp, frame_qp_check.cpp) can run it under the sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "rbt_qp_walk.h"

namespace rbt {
// The floor of one entry. Its walk goes toward larger QPs while meets holds on the trial at q. A probe at q0 - the entry's own QP, clamped to the range - comes first and
// says where the walk starts: qs (w.start), one QP further per dB the probe's figure is above the floor, q0 itself when the probe came back exactly (a figure of +inf).
struct FloorGoal { int32_t floor_mdb = 0; int q0 = 0; bool probed = false; };
template <class Trial> inline void floor_seed(QpWalk<Trial>& w, FloorGoal& g, int qp) { w.toward = 1; g.q0 = std::min(w.hi, std::max(w.lo, qp)); }
// false: the probe has not been tried, a round has to bring q0 alone; true: w.start is known and qp_walk_step can look
template <class Trial, class Figure> inline bool floor_probe(QpWalk<Trial>& w, FloorGoal& g, Figure figure) {
  const auto t = w.tried.find(g.q0);
  if (g.probed || t == w.tried.end()) return g.probed;
  const double p = figure(t->second);
  w.start = std::isinf(p) ? g.q0 : std::min(w.hi, std::max(w.lo, g.q0 + (int)(p - g.floor_mdb / 1000.0)));
  return g.probed = true;
}
// the condition of qp_walk_step: meets on the trial of a tried QP
template <class Trial, class Meets> inline auto floor_holds(const QpWalk<Trial>& w, Meets meets) { return [&w, meets](int q) { return meets(w.tried.find(q)->second); }; }
}  // namespace rbt
