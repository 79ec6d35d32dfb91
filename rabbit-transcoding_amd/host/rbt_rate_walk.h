// Host half of a rate-targeted transcode (include/rbt.h, "transcoding to a byte budget"): the estimate from the census, and what makes the shared walk (rbt_qp_walk.h) the
// walk of a budget. Plain host code without a device call, so that tests/rate_check.cpp can run it under the sanitizers next to the census body.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../csrc/rbt_rate.h"
#include "rbt_qp_walk.h"

namespace rbt {
// Output picture k of a geometry / attribute stream is an I picture coded at max(0, q - 3) for even k and a P picture coded at q for odd k (RBT-E1, gop 2); per picture the
// input's own bytes per non-zero level, B_k / N0_k, times the levels that survive the picture's QP
inline void rate_table(const uint32_t* hist, const uint64_t* picture_bytes, int n, uint64_t estimate[52]) {
  for (int q = 0; q < 52; q++) {
    uint64_t e = 0;
    for (int k = 0; k < n; k++) {
      const uint32_t* h = hist + (size_t)k * RBT_RATE_HIST_WORDS; const int qk = k % 2 ? q : std::max(0, q - 3);
      uint64_t n0 = 0, nz = 0;
      for (int c = 0; c < 3; c++) for (int b = 0; b < RBT_RATE_BINS; b++) { n0 += h[c * RBT_RATE_BINS + b]; if (b > qk) nz += h[c * RBT_RATE_BINS + b]; }
      e += picture_bytes[k] * nz / std::max<uint64_t>(1, n0);
    }
    estimate[q] = e;
  }
}

// The budget of one targeted entry. Its walk goes toward smaller QPs while s(q) <= T, s(q) being the size of the stream the trial at q gave (Trial::stream), and starts
// at qe (w.start): the smallest QP of the range whose estimate fits the budget, the end of the range if none does; e_qe = E(qe)
struct RateGoal { uint64_t T = 0, e_qe = 0; };
struct RateTrial { std::vector<uint8_t> stream; };
template <class Trial> inline void rate_seed(QpWalk<Trial>& w, RateGoal& g, const uint64_t estimate[52]) {
  w.toward = -1; w.start = w.hi;
  for (int q = w.lo; q <= w.hi; q++) if (estimate[q] <= g.T) { w.start = q; break; }
  g.e_qe = estimate[w.start];
}
template <class Trial> inline auto rate_fits(const QpWalk<Trial>& w, const RateGoal& g) { return [&w, &g](int q) { return (uint64_t)w.tried.find(q)->second.stream.size() <= g.T; }; }
}  // namespace rbt
