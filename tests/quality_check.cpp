// TEST-ONLY: the body of the distortion sums (csrc/rbt_quality.h) and the host half of a transcode to a PSNR floor (host/rbt_quality_walk.h: PSNR, the floor's condition;
// host/rbt_floor_walk.h: probe; host/rbt_qp_walk.h: walk, rounds) as a stand-alone host program, so that they can be built with -fsanitize=address,undefined and run on the CPU (tests/test_quality.py). The planes are views
// into heap blocks that end with the last sample of the last row, at every misalignment of the two pictures against a 16-byte boundary and against each other, so a read
// past a row's end or a misaligned 16-byte load is caught; the sums are compared with a per-sample loop of the definition, the walk - driven round by round the way
// run_rounds drives it - with the definition's loop on every floor, start and range of three PSNR tables, one of them not monotone, and every round with the rule of what
// a round encodes. Prints "ok".
#define RBT_HOSTEMU 1
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../rabbit-transcoding_amd/host/rbt_quality_walk.h"
#include "../rabbit-transcoding_amd/host/rbt_floor_walk.h"

static int fail(const char* what, long a = 0, long b = 0, long c = 0) { printf("FAIL %s %ld %ld %ld\n", what, a, b, c); fflush(stdout); return 1; }
static uint32_t g_seed = 4321;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// a plane of pw x ph samples with row stride `stride`, its first sample `mis` samples behind a 16-byte boundary, in a block that ends with its last sample
struct Plane { uint16_t* mem = nullptr; uint16_t* p = nullptr; ~Plane() { free(mem); } };
static void make_plane(Plane& P, int pw, int ph, int stride, int mis, int peak, int fill) {
  const size_t n = (size_t)(ph - 1) * stride + pw;
  P.mem = (uint16_t*)malloc((n + mis) * 2);                      // malloc's blocks start on a multiple of 16
  if (!P.mem || ((uintptr_t)P.mem & 15)) { printf("FAIL malloc\n"); exit(1); }
  P.p = P.mem + mis;
  for (size_t i = 0; i < n; i++) P.p[i] = (uint16_t)(fill >= 0 ? fill : (int)(rnd() % (peak + 1)));
}

static int sse_case(int w, int h, int a_stride, int b_stride, int mis_a, int mis_b, int scale, int peak, int extremes) {
  Plane A[3], B[3]; RbtSsePic P; memset(&P, 0, sizeof(P));
  for (int c = 0; c < 3; c++) { const int sh = c ? 1 : 0;
    make_plane(A[c], w >> sh, h >> sh, a_stride >> sh, mis_a, peak, extremes ? 0 : -1); make_plane(B[c], w >> sh, h >> sh, b_stride >> sh, mis_b, peak, extremes ? peak : -1);
    P.a[c] = A[c].p; P.b[c] = B[c].p; }
  std::vector<uint16_t> occ;
  if (scale) { occ.resize((size_t)(w / scale) * (h / scale)); for (auto& v : occ) v = (uint16_t)(rnd() % 3 == 0 ? 0 : rnd() % 300 + 1); occ.back() = 1; P.occ = occ.data(); P.ow = w / scale; P.scale = scale; }
  uint64_t out[RBT_SSE_WORDS] = {0}, want[RBT_SSE_WORDS] = {0};
  P.w = w; P.h = h; P.a_stride = a_stride; P.b_stride = b_stride; P.out = out;
  rbtk::launch_picture_sse(&P, 1, RBT_SSE_PIC_CHUNKS(w, h));
  for (int c = 0; c < 3; c++) { const int sh = c ? 1 : 0;
    for (int y = 0; y < h >> sh; y++) for (int x = 0; x < w >> sh; x++) {
      const long long d = (long long)P.a[c][(size_t)y * (a_stride >> sh) + x] - (long long)P.b[c][(size_t)y * (b_stride >> sh) + x];
      want[3 * c] += (uint64_t)(d * d);
      if (scale && occ[(size_t)((y << sh) / scale) * (w / scale) + (x << sh) / scale] > 0) { want[3 * c + 1] += (uint64_t)(d * d); want[3 * c + 2]++; }
    } }
  for (int i = 0; i < RBT_SSE_WORDS; i++) if (out[i] != want[i]) return fail("sse", w, i, (long)out[i]);
  if (extremes && out[0] != (uint64_t)w * h * peak * peak) return fail("extremes", w, h);
  return 0;
}

// table: PSNR in 1/1000 dB per q (0..51) turned into sums of a million samples at 10 bits; the rounds as the library runs them; the definition beside them
static rbt::QualitySums sums_of(double db) {
  rbt::QualitySums s; s.samples[0] = 1000000; s.sse[0] = (uint64_t)(1023.0 * 1023.0 * 1e6 / pow(10.0, db / 10.0));
  s.samples_occ[0] = 400000; s.sse_occ[0] = s.sse[0] / 3;
  return s;
}
static int walk_case(const std::vector<rbt::QualitySums>& t, int qp, int32_t floor_mdb, int region, int lo, int hi) {
  rbt::QpWalk<rbt::QualityTried> w; rbt::FloorGoal g; g.floor_mdb = floor_mdb; w.lo = lo; w.hi = hi; rbt::floor_seed(w, g, qp);
  auto figure_of = [&](const rbt::QualityTried& x) { return rbt::quality_region_psnr(x.sums, region, 10); };
  auto trial_meets = [&](const rbt::QualityTried& x) { return rbt::quality_meets(x.sums, region, floor_mdb, 10); };
  const int q0 = qp < lo ? lo : qp > hi ? hi : qp;
  if (g.q0 != q0 || w.toward != 1) return fail("seed", qp, g.q0, q0);
  auto meets = [&](int q) { return rbt::quality_meets(t[q], region, floor_mdb, 10); };
  const double p0 = rbt::quality_region_psnr(t[q0], region, 10);
  int qs = std::isinf(p0) ? q0 : q0 + (int)(p0 - floor_mdb / 1000.0); qs = qs < lo ? lo : qs > hi ? hi : qs;
  int n_enc = 0, need = 0, dir = 0, round = 0; std::vector<int> qps, rule;
  for (;; round++) {
    const bool probe = !rbt::floor_probe(w, g, figure_of);
    if (probe) { need = g.q0; dir = 0; } else if (rbt::qp_walk_step(w, rbt::floor_holds(w, trial_meets), need, dir)) break;
    rbt::qp_round(w, need, dir, probe, qps);
    // the rule: the first round is the probe at q0 alone; the second qs - 1, qs, qs + 1; every later one the QP asked for and the next one the same way - up while the
    // floor was met at qs, down while it was not -; a QP out of the range or already encoded is left out
    rule.clear();
    if (round == 0) { if (!probe || need != q0 || dir != 0) return fail("first round", need, dir, q0); rule = {q0}; }
    else if (dir == 0) { if (probe || round != 1 || need != qs) return fail("start round", round, need, qs); rule = {qs - 1, qs, qs + 1}; }
    else { if (probe || dir != (meets(qs) ? 1 : -1)) return fail("direction", dir, qs, floor_mdb); rule = {need, need + dir}; }
    for (size_t i = rule.size(); i-- > 0;) if (rule[i] < lo || rule[i] > hi || w.tried.count(rule[i])) rule.erase(rule.begin() + i);
    if (qps != rule) return fail("round is not the rule's", round, need, dir);
    if (qps.empty()) return fail("empty round", floor_mdb, lo, hi);
    bool brought = false;
    for (int q : qps) { if (q < lo || q > hi) return fail("round out of range", q, lo, hi); if (w.tried.count(q)) return fail("encoded twice", q, lo, hi); w.tried[q].sums = t[q]; n_enc++; brought |= q == need; }
    if (!brought) return fail("round without the sums asked for", need, lo, hi);
  }
  int q = qs, met;
  if (meets(q)) { while (q < hi && meets(q + 1)) q++; met = 1; } else { while (q > lo && !meets(q)) q--; met = meets(q); }
  if (w.start != qs || w.qstar != q || w.met != met) return fail("walk", floor_mdb, w.qstar, q);
  if (n_enc > abs(q - qs) + 5) return fail("encodes", n_enc, q, qs);
  return 0;
}

// A walk on the occupied region of trials without an occupied sample. The definitions give the expectation, not the functions under test: the figure of a region without
// samples is 0.0, so the probe at q0 puts the start at q0 + (int)(0.0 - floor) clamped to the range; a region without samples meets every floor, so the walk climbs from
// there to hi: q* = hi, met = 1. (A condition derived from the figure - 0.0 >= floor - would stay at lo with met = 0.)
static int empty_region_case(int qp, int32_t floor_mdb, int lo, int hi) {
  rbt::QpWalk<rbt::QualityTried> w; rbt::FloorGoal g; g.floor_mdb = floor_mdb; w.lo = lo; w.hi = hi; rbt::floor_seed(w, g, qp);
  auto figure_of = [](const rbt::QualityTried& x) { return rbt::quality_region_psnr(x.sums, 1, 10); };
  auto trial_meets = [&](const rbt::QualityTried& x) { return rbt::quality_meets(x.sums, 1, floor_mdb, 10); };
  const int q0 = qp < lo ? lo : qp > hi ? hi : qp;
  int qs = q0 + (int)(0.0 - floor_mdb / 1000.0); qs = qs < lo ? lo : qs > hi ? hi : qs;
  int n_enc = 0, need = 0, dir = 0; std::vector<int> qps;
  for (int round = 0;; round++) {
    const bool probe = !rbt::floor_probe(w, g, figure_of);
    if (probe) { need = g.q0; dir = 0; } else if (rbt::qp_walk_step(w, rbt::floor_holds(w, trial_meets), need, dir)) break;
    if (probe != (round == 0) || (probe && need != q0)) return fail("empty region: the probe is the first round, at q0", round, need, q0);
    if (!probe && w.start != qs) return fail("empty region: start", w.start, qs);
    rbt::qp_round(w, need, dir, probe, qps);
    if (qps.empty() || round > 60) return fail("empty region: rounds", round, lo, hi);
    for (int q : qps) {      // every trial: distortion on all samples, not one occupied sample
      if (q < lo || q > hi || w.tried.count(q)) return fail("empty region: round", q, lo, hi);
      rbt::QualitySums s; s.samples[0] = 1000000; s.sse[0] = 5000000 + 100000 * (uint64_t)q; w.tried[q].sums = s; n_enc++;
    }
  }
  if (w.start != qs || w.qstar != hi || w.met != 1) return fail("empty region: walk", w.start, w.qstar, w.met);
  if (n_enc > hi - qs + 5) return fail("empty region: encodes", n_enc, hi, qs);
  return 0;
}

int main() {
  // sizes of the tests and strides that are not the width; every pair of misalignments for the 130-wide picture (chroma rows of 65 samples)
  const int sizes[][2] = {{8, 8}, {16, 8}, {72, 40}, {130, 66}, {264, 136}};
  for (auto& sz : sizes) for (int scale : {0, 1, 2}) {
    if (sse_case(sz[0], sz[1], sz[0], sz[0], 0, 0, scale, 1023, 0)) return 1;
    if (sse_case(sz[0], sz[1], sz[0] + 6, sz[0] + 22, 2, 2, scale, 1023, 0)) return 1;
    if (sse_case(sz[0], sz[1], sz[0] + 16, sz[0], 4, 0, scale, 255, 0)) return 1;
  }
  for (int ma = 0; ma < 8; ma++) for (int mb = 0; mb < 8; mb++) if (sse_case(130, 66, 130, 144, ma, mb, 2, 1023, 0)) return 1;
  if (sse_case(264, 136, 264, 272, 0, 0, 4, 1023, 1) || sse_case(264, 136, 264, 264, 3, 3, 4, 65535, 1) || sse_case(72, 40, 72, 80, 0, 0, 4, 255, 1)) return 1;
  // PSNR and the floor's condition at their corners
  { rbt::QualitySums s; if (rbt::quality_psnr(0, 0, 10) != 0.0 || !std::isinf(rbt::quality_psnr(0, 5, 10)) || !rbt::quality_meets(s, 0, 99000, 10) || !rbt::quality_meets(s, 1, 99000, 10)) return fail("corners");
    s.samples[0] = 100; s.sse[0] = 100; if (fabs(rbt::quality_psnr(100, 100, 8) - 20.0 * log10(255.0)) > 1e-12 || rbt::quality_meets(s, 0, 61000, 10) || !rbt::quality_meets(s, 0, 61000, 16) || !rbt::quality_meets(s, 1, 61000, 10)) return fail("psnr"); }
  // the walk on a monotone table of 0.7 dB a step, one with the inversions of the 64x64 geometry maps, and a noisy one; every start, floors at and between the table's values
  std::vector<double> mono(52), inv(52), noisy(52);
  for (int q = 0; q < 52; q++) { mono[q] = 62.0 - 0.7 * q; inv[q] = 66.0 - 0.72 * q; noisy[q] = 60.0 - 0.6 * q + (rnd() % 1200) / 1000.0; }
  inv[34] = 41.737; inv[35] = 41.116; inv[36] = 41.186; inv[37] = 39.719; inv[40] = 37.0; inv[41] = 37.3; inv[44] = 34.8; inv[45] = 35.1;
  for (const std::vector<double>* tb : {&mono, &inv, &noisy}) {
    std::vector<rbt::QualitySums> t; for (int q = 0; q < 52; q++) t.push_back(sums_of((*tb)[q]));
    for (int region = 0; region < 2; region++) for (int lo = 0; lo < 52; lo += 5) for (int hi = lo; hi < 52; hi += 6) for (int qp = 0; qp < 52; qp += 3) {
      for (int q = lo; q <= hi; q += 2) for (int d = -350; d <= 350; d += 350) if (walk_case(t, qp, (int32_t)((*tb)[q] * 1000) + d + (region ? 4771 : 0), region, lo, hi)) return 1;
      if (walk_case(t, qp, 1, region, lo, hi) || walk_case(t, qp, 120000, region, lo, hi)) return 1;
    }
  }
  // a picture that comes back exactly: psnr +inf, the walk starts at q0 and climbs while the sums stay zero
  { std::vector<rbt::QualitySums> t(52); for (int q = 0; q < 52; q++) { t[q] = sums_of(50.0 - q); if (q < 12) t[q].sse[0] = 0; }
    if (walk_case(t, 5, 45000, 0, 0, 51) || walk_case(t, 11, 30000, 0, 0, 51) || walk_case(t, 0, 99000, 0, 0, 11)) return 1; }
  // no occupied sample in any trial: figure 0.0, floor met (the expected starts, by hand: 26 - 40 and 0 - 40, clamped: 20 and 0)
  if (empty_region_case(26, 40000, 20, 30) || empty_region_case(0, 40000, 0, 51)) return 1;
  printf("ok\n");
  return 0;
}
