// Host half of a transcode to a PSNR floor (include/rbt.h, "transcoding to a PSNR floor"): PSNR and the floor's condition on the integer sums of csrc/rbt_quality.h, and what
// makes the shared walk (rbt_qp_walk.h) the walk of a floor: a probe in front of it. Plain host code without a device call, so that tests/quality_check.cpp can run it under the sanitizers next to the kernel body.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include "../csrc/rbt_quality.h"
#include "rbt_qp_walk.h"

namespace rbt {
// the sums of one stream: every picture's nine words added up, and the samples they were taken over
struct QualitySums { uint64_t sse[3] = {0, 0, 0}, samples[3] = {0, 0, 0}, sse_occ[3] = {0, 0, 0}, samples_occ[3] = {0, 0, 0}; };
inline void quality_add_picture(QualitySums& s, const uint64_t* words, int w, int h) {
  for (int c = 0; c < 3; c++) { s.sse[c] += words[3 * c]; s.sse_occ[c] += words[3 * c + 1]; s.samples_occ[c] += words[3 * c + 2]; s.samples[c] += c ? (uint64_t)(w / 2) * (uint64_t)(h / 2) : (uint64_t)w * (uint64_t)h; }
}
inline double quality_psnr(uint64_t sse, uint64_t samples, int bit_depth) {
  if (!samples) return 0.0;
  if (!sse) return std::numeric_limits<double>::infinity();
  const double peak = (double)((1u << bit_depth) - 1);
  return 10.0 * log10((double)peak * peak * (double)samples / (double)sse);
}
// region: 0 = all samples, 1 = the occupied ones (RBT_QUALITY_*); plane 0 decides
inline double quality_region_psnr(const QualitySums& s, int region, int bit_depth) { return region ? quality_psnr(s.sse_occ[0], s.samples_occ[0], bit_depth) : quality_psnr(s.sse[0], s.samples[0], bit_depth); }
inline bool quality_meets(const QualitySums& s, int region, int32_t min_psnr_mdb, int bit_depth) {
  const uint64_t sse = region ? s.sse_occ[0] : s.sse[0], n = region ? s.samples_occ[0] : s.samples[0];
  if (!n || !sse) return true;
  return quality_psnr(sse, n, bit_depth) >= min_psnr_mdb / 1000.0;
}

// The floor of one entry. Its walk goes toward larger QPs while meets(q) holds on the sums of the trial at q. A probe at q0 - the entry's own QP, clamped to the range -
// comes first and says where the walk starts: qs (w.start), one QP further per dB the probe is above the floor, q0 itself when the probe came back exactly.
struct QualityTried { std::vector<uint8_t> stream; QualitySums sums; };
struct QualityGoal { int32_t floor_mdb = 0; int region = 0, bit_depth = 8, q0 = 0; bool probed = false; };
template <class Trial> inline void quality_seed(QpWalk<Trial>& w, QualityGoal& g, int qp) { w.toward = 1; g.q0 = std::min(w.hi, std::max(w.lo, qp)); }
// false: the probe has not been tried, a round has to bring q0 alone; true: w.start is known and qp_walk_step can look
template <class Trial> inline bool quality_probe(QpWalk<Trial>& w, QualityGoal& g) {
  const auto t = w.tried.find(g.q0);
  if (g.probed || t == w.tried.end()) return g.probed;
  const double p = quality_region_psnr(t->second.sums, g.region, g.bit_depth);
  w.start = std::isinf(p) ? g.q0 : std::min(w.hi, std::max(w.lo, g.q0 + (int)(p - g.floor_mdb / 1000.0)));
  return g.probed = true;
}
template <class Trial> inline auto quality_holds(const QpWalk<Trial>& w, const QualityGoal& g) { return [&w, &g](int q) { return quality_meets(w.tried.find(q)->second.sums, g.region, g.floor_mdb, g.bit_depth); }; }
}  // namespace rbt
