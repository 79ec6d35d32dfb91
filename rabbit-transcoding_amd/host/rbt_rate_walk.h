// Host half of a rate-targeted transcode (include/rbt.h, "transcoding to a byte budget"): the estimate from the census and the walk over the sizes of trial encodes. Plain
// host code without a device call, so that tests/rate_check.cpp can run it under the sanitizers next to the census body.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <vector>
#include "../csrc/rbt_rate.h"

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

// The walk of one targeted entry over the sizes of the trial encodes run so far. It is the definition restated: it looks at s(q) and E(q) only, so the result does not
// depend on which sizes a round happened to bring beyond the one it asked for.
struct RateWalk {
  int q = 0, entry = 0;                        // position in the pipeline's group, index of the entry in the call
  uint64_t T = 0, e_qe = 0; int lo = 0, hi = 51, qe = 0;
  std::map<int, std::vector<uint8_t>> tried;   // QP -> the stream it gave
  bool settled = false; int qstar = 0, met = 0;
};
// true: settled (qstar, met); false: the walk needs s(need) next and is going in direction dir (0: it has not started)
inline bool rate_walk_step(RateWalk& w, int& need, int& dir) {
  auto known = [&](int q) { return w.tried.count(q) != 0; };
  auto size_at = [&](int q) { return (uint64_t)w.tried[q].size(); };
  if (!known(w.qe)) { need = w.qe; dir = 0; return false; }
  int q = w.qe;
  if (size_at(q) <= w.T) {
    while (q > w.lo) { if (!known(q - 1)) { need = q - 1; dir = -1; return false; } if (size_at(q - 1) <= w.T) q--; else break; }
    w.met = 1;
  } else {
    while (q < w.hi && size_at(q) > w.T) { q++; if (!known(q)) { need = q; dir = 1; return false; } }
    w.met = size_at(q) <= w.T;
  }
  w.qstar = q; w.settled = true;
  return true;
}
// what a round encodes for a walk: the three QPs around the estimate first, then two at a time where the walk is going (one wasted encode at most per round: n_encodes <= |q* - qe| + 4)
inline void rate_round_qps(const RateWalk& w, int need, int dir, std::vector<int>& qps) {
  qps.clear();
  if (dir == 0) { for (int q = w.qe - 1; q <= w.qe + 1; q++) if (q >= w.lo && q <= w.hi) qps.push_back(q); }
  else for (int q = need, k = 0; k < 2 && q >= w.lo && q <= w.hi; q += dir, k++) qps.push_back(q);
}
}  // namespace rbt
