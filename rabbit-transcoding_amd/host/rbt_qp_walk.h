// The walk that a byte budget and a PSNR floor share (include/rbt.h, "transcoding to a byte budget", "transcoding to a PSNR floor"): both look for the boundary of a
// condition on the trial encodes of one entry - the smallest QP whose stream fits the budget, the largest whose distortion meets the floor. One walk with a direction, and
// one rule for what a round of trial encodes brings it. Plain host code without a device call; rbt_rate_walk.h adds a budget's seed and condition, rbt_floor_walk.h a floor's.
#pragma once
#include <map>
#include <vector>

namespace rbt {
// The walk of one entry over the trial encodes run so far. It is the definition restated: it looks at the trials of the QPs it names only, so the result does not depend
// on what else a round happened to bring.
template <class Trial> struct QpWalk {
  int q = 0, entry = 0;                        // position in the pipeline's group, index of the entry in the call
  int lo = 0, hi = 51, start = 0, toward = -1; // toward: -1 = the smallest QP of [lo, hi] for which the condition holds (a budget), +1 = the largest (a floor)
  std::map<int, Trial> tried;                  // QP -> what it gave
  bool settled = false; int qstar = 0, met = 0;
};
// holds(q): the condition on a tried QP. true: settled (qstar, met); false: the walk needs the trial of QP `need` next and is going in direction dir (0: it is at its start)
template <class Trial, class Holds> inline bool qp_walk_step(QpWalk<Trial>& w, Holds holds, int& need, int& dir) {
  auto known = [&](int q) { return w.tried.count(q) != 0; };
  const int t = w.toward, end = t < 0 ? w.lo : w.hi, back = t < 0 ? w.hi : w.lo;
  if (!known(w.start)) { need = w.start; dir = 0; return false; }
  int q = w.start;
  if (holds(q)) {
    while (q != end) { if (!known(q + t)) { need = q + t; dir = t; return false; } if (holds(q + t)) q += t; else break; }
    w.met = 1;
  } else {
    while (q != back && !holds(q)) { q -= t; if (!known(q)) { need = q; dir = -t; return false; } }
    w.met = holds(q);
  }
  w.qstar = q; w.settled = true;
  return true;
}
// what a round encodes for a walk: at its start the three QPs around `need` - `need` alone for a probe that only says where the start is -, then two at a time where the
// walk is going (one wasted encode at most per round); a QP out of the range or already tried is never named
template <class Trial> inline void qp_round(const QpWalk<Trial>& w, int need, int dir, bool alone, std::vector<int>& qps) {
  qps.clear();
  auto want = [&](int q) { if (q >= w.lo && q <= w.hi && !w.tried.count(q)) qps.push_back(q); };
  if (dir == 0 && alone) want(need);
  else if (dir == 0) { for (int q = need - 1; q <= need + 1; q++) want(q); }
  else { want(need); want(need + dir); }
}
}  // namespace rbt
