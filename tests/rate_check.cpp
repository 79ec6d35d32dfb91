// TEST-ONLY: the body of the level census (csrc/rbt_rate.h) and the host half of a rate-targeted transcode (host/rbt_rate_walk.h: estimate, seed, budget; host/rbt_qp_walk.h: walk, rounds) as a stand-alone
// host program, so that they can be built with -fsanitize=address,undefined and run on the CPU (tests/test_rate.py). The planes and maps are heap blocks of exactly the
// picture's size, so a read past a plane's last word is caught; the census is compared with a per-sample count of the definition, the walk - driven round by round the way
// run_rounds drives it - with the definition's loop on every budget and range of three size tables, one of them not monotone, and every round with the rule of what a
// round encodes. Prints "ok".
#define RBT_HOSTEMU 1
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../rabbit-transcoding_amd/host/rbt_rate_walk.h"

static int fail(const char* what, long a = 0, long b = 0, long c = 0) { printf("FAIL %s %ld %ld %ld\n", what, a, b, c); fflush(stdout); return 1; }
static uint32_t g_seed = 12345;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static int census_case(int w, int h, int density_pct, int extremes) {
  const size_t ys = (size_t)w * h, cs = ys / 4, u = ys / 16;
  std::vector<int16_t> coef(ys + 2 * cs); std::vector<int8_t> qp(u); std::vector<uint8_t> pm(u);
  for (auto& v : coef) v = (int)(rnd() % 100) < density_pct ? (int16_t)((int)(rnd() % 41) - 20) : 0;
  if (extremes) { const int16_t e[6] = {1, -1, 32767, -32767, -32768, 2}; for (int c = 0; c < 3; c++) for (int k = 0; k < 6; k++) coef[(c == 0 ? 0 : c == 1 ? ys : ys + cs) + k] = e[k];
                  coef[ys - 1] = -32768; coef[ys + cs - 1] = 32767; coef[ys + 2 * cs - 1] = -1; }
  for (size_t i = 0; i < u; i++) { qp[i] = (int8_t)((int)(rnd() % 70) - 9); pm[i] = (uint8_t)(1 | (rnd() % 5 == 0 ? RBT_PM_TQ_BYPASS : 0)); }
  uint32_t hist[RBT_RATE_HIST_WORDS] = {0}, want[RBT_RATE_HIST_WORDS] = {0};
  RbtCensusPic P = {{coef.data(), coef.data() + ys, coef.data() + ys + cs}, qp.data(), pm.data(), w, h, hist};
  rbtk::launch_level_census(&P, 1, RBT_RATE_PIC_WORDS(w, h));
  static const long long LS[6] = {40, 45, 51, 57, 64, 72}, G[6] = {26214, 23302, 20560, 18396, 16384, 14564};
  for (int c = 0; c < 3; c++) { const int pw = c ? w / 2 : w, ph = c ? h / 2 : h; const int16_t* p = P.coef[c];
    for (int y = 0; y < ph; y++) for (int x = 0; x < pw; x++) { const int l = p[(size_t)y * pw + x]; if (!l) continue;
      const int unit = c ? (2 * y / 4) * (w / 4) + 2 * x / 4 : (y / 4) * (w / 4) + x / 4;
      if (pm[unit] & RBT_PM_TQ_BYPASS) continue;
      const int qin = qp[unit] < 0 ? 0 : qp[unit] > 51 ? 51 : qp[unit];
      const long long m = (long long)(l < 0 ? -l : l) * LS[qin % 6] * (1ll << (qin / 6)); int bin = 0;
      for (int q = 0; q < 52; q++) bin += 3 * m * G[q % 6] >= 1ll << (21 + q / 6);
      want[c * RBT_RATE_BINS + bin]++; } }
  for (int i = 0; i < RBT_RATE_HIST_WORDS; i++) if (hist[i] != want[i]) return fail("census", w, i, hist[i]);
  return 0;
}

// s(q) for q = 0..51; the rounds as the library runs them; the definition beside them
static int walk_case(const std::vector<uint64_t>& s, const uint64_t E[52], uint64_t T, int lo, int hi) {
  rbt::QpWalk<rbt::RateTrial> w; rbt::RateGoal g; g.T = T; w.lo = lo; w.hi = hi; rbt::rate_seed(w, g, E);
  int qe = hi; for (int q = lo; q <= hi; q++) if (E[q] <= T) { qe = q; break; }
  if (w.start != qe || w.toward != -1 || g.e_qe != E[qe]) return fail("seed", (long)T, w.start, qe);
  int n_enc = 0, need = 0, dir = 0, round = 0; std::vector<int> qps, rule;
  for (; !rbt::qp_walk_step(w, rbt::rate_fits(w, g), need, dir); round++) {
    rbt::qp_round(w, need, dir, false, qps);
    // the rule: the first round is qe - 1, qe, qe + 1; every later one the QP asked for and the next one the same way - down while the budget held at qe, up while it
    // did not -; a QP out of the range or already encoded is left out
    rule.clear();
    if (round == 0) { if (need != qe || dir != 0) return fail("first round", need, dir, qe); rule = {qe - 1, qe, qe + 1}; }
    else { if (dir != (s[qe] <= T ? -1 : 1)) return fail("direction", dir, qe, (long)T); rule = {need, need + dir}; }
    for (size_t i = rule.size(); i-- > 0;) if (rule[i] < lo || rule[i] > hi || w.tried.count(rule[i])) rule.erase(rule.begin() + i);
    if (qps != rule) return fail("round is not the rule's", round, need, dir);
    if (qps.empty()) return fail("empty round", (long)T, lo, hi);
    bool brought = false;
    for (int q : qps) { if (q < lo || q > hi) return fail("round out of range", q, lo, hi); if (w.tried.count(q)) return fail("encoded twice", q, lo, hi); w.tried[q].stream.assign((size_t)s[q], 0); n_enc++; brought |= q == need; }
    if (!brought) return fail("round without the size asked for", need, lo, hi);
  }
  int q = qe, met;
  if (s[q] <= T) { while (q > lo && s[q - 1] <= T) q--; met = 1; } else { while (q < hi && s[q] > T) q++; met = s[q] <= T; }
  if (w.qstar != q || w.met != met) return fail("walk", (long)T, w.qstar, q);
  if (n_enc > abs(q - qe) + 4) return fail("encodes", n_enc, q, qe);
  return 0;
}

int main() {
  const int sizes[][2] = {{8, 8}, {16, 8}, {72, 40}, {208, 120}, {264, 136}};
  for (auto& sz : sizes) for (int d : {0, 7, 100}) if (census_case(sz[0], sz[1], d, d == 7)) return 1;
  // the estimate: two pictures, a level of 1 at QP 20 each (bin 24) and one that survives everything; 1000 and 100 bytes
  { uint32_t hist[2 * RBT_RATE_HIST_WORDS] = {0}; hist[24] = 3; hist[RBT_RATE_BINS + 52] = 1; hist[RBT_RATE_HIST_WORDS + 24] = 1;
    const uint64_t B[2] = {1000, 100}; uint64_t E[52]; rbt::rate_table(hist, B, 2, E);
    for (int q = 0; q < 52; q++) { const uint64_t want = (q - 3 < 24 ? 1000u : 250u) + (q < 24 ? 100u : 0u); if (E[q] != want) return fail("estimate", q, (long)E[q], (long)want); }
    const uint64_t B0[2] = {0, 0}; uint32_t none[2 * RBT_RATE_HIST_WORDS] = {0}; rbt::rate_table(none, B0, 2, E); for (int q = 0; q < 52; q++) if (E[q]) return fail("empty estimate", q); }
  // the walk on a monotone table, one with a plateau that steps up (368, 369, 369 as the 192x128 geometry maps give), and a noisy one; estimates that are good, low and high
  std::vector<uint64_t> mono(52), plateau(52), noisy(52);
  for (int q = 0; q < 52; q++) { mono[q] = 5000 - 90 * (uint64_t)q; plateau[q] = q == 31 ? 368 : q == 32 || q == 33 ? 369 : q < 31 ? 400 + 27 * (uint64_t)(30 - q) : 351 - 12 * (uint64_t)(q - 34); noisy[q] = 3000 - 50 * (uint64_t)q + rnd() % 120; }
  for (const std::vector<uint64_t>* s : {&mono, &plateau, &noisy}) for (int bias = 0; bias < 3; bias++) {
    uint64_t E[52]; for (int q = 0; q < 52; q++) E[q] = bias == 0 ? (*s)[q] : bias == 1 ? (*s)[q] / 3 : (*s)[q] * 2;
    for (int lo = 0; lo < 52; lo += 3) for (int hi = lo; hi < 52; hi += 4) {
      for (int q = lo; q <= hi; q++) for (int d = -1; d <= 1; d++) if (walk_case(*s, E, (*s)[q] + d, lo, hi)) return 1;
      if (walk_case(*s, E, 0, lo, hi) || walk_case(*s, E, 1u << 30, lo, hi)) return 1;
    }
  }
  printf("ok\n");
  return 0;
}
