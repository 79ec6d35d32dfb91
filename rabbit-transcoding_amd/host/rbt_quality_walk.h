// Host half of a transcode to a PSNR floor (include/rbt.h, "transcoding to a PSNR floor"): PSNR and the floor's condition on the integer sums of csrc/rbt_quality.h, and the
// walk over the distortions of trial encodes. Plain host code without a device call, so that tests/quality_check.cpp can run it under the sanitizers next to the kernel body.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <map>
#include <vector>
#include "../csrc/rbt_quality.h"

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

// The walk of one entry with a floor over the trial encodes run so far. It is the definition restated: it looks at the sums of the QPs it names only, so the result does
// not depend on what else a round happened to bring.
struct QualityTried { std::vector<uint8_t> stream; QualitySums sums; };
struct QualityWalk {
  int q = 0, entry = 0;                        // position in the pipeline's group, index of the entry in the call
  int32_t floor_mdb = 0; int region = 0, bit_depth = 8, lo = 0, hi = 51, q0 = 0;
  std::map<int, QualityTried> tried;           // QP -> what it gave
  bool started = false, settled = false; int qs = 0, qstar = 0, met = 0;
};
// true: settled (qstar, met); false: the walk needs the sums of QP `need` next and is going in direction dir (0: the probe at q0, or the start at qs)
inline bool quality_walk_step(QualityWalk& w, int& need, int& dir) {
  auto known = [&](int q) { return w.tried.count(q) != 0; };
  auto meets = [&](int q) { return quality_meets(w.tried[q].sums, w.region, w.floor_mdb, w.bit_depth); };
  if (!known(w.q0)) { need = w.q0; dir = 0; return false; }
  if (!w.started) {
    const double p = quality_region_psnr(w.tried[w.q0].sums, w.region, w.bit_depth);
    w.qs = std::isinf(p) ? w.q0 : std::min(w.hi, std::max(w.lo, w.q0 + (int)(p - w.floor_mdb / 1000.0)));
    w.started = true;
  }
  if (!known(w.qs)) { need = w.qs; dir = 0; return false; }
  int q = w.qs;
  if (meets(q)) {
    while (q < w.hi) { if (!known(q + 1)) { need = q + 1; dir = 1; return false; } if (meets(q + 1)) q++; else break; }
    w.met = 1;
  } else {
    while (q > w.lo && !meets(q)) { q--; if (!known(q)) { need = q; dir = -1; return false; } }
    w.met = meets(q);
  }
  w.qstar = q; w.settled = true;
  return true;
}
// what a round encodes for a walk: q0 alone first, then the three QPs around qs, then two at a time where the walk is going; a QP already tried is never encoded again
// (one wasted encode at most per round: n_encodes <= |q* - qs| + 5)
inline void quality_round_qps(const QualityWalk& w, int need, int dir, std::vector<int>& qps) {
  qps.clear();
  auto want = [&](int q) { if (q >= w.lo && q <= w.hi && !w.tried.count(q)) qps.push_back(q); };
  if (dir == 0 && !w.started) want(need);
  else if (dir == 0) { for (int q = need - 1; q <= need + 1; q++) want(q); }
  else { want(need); want(need + dir); }
}
}  // namespace rbt
