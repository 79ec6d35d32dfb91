// TEST-ONLY: the body of the luma gather (csrc/rbt_cloudmaps.h) and the host half of a transcode to a D1 floor (host/rbt_d1_walk.h: D(q), the floor's condition;
// host/rbt_floor_walk.h: probe; host/rbt_qp_walk.h: walk, rounds) as a stand-alone host program, so that they can be built with -fsanitize=address,undefined and run on the CPU (tests/test_d1_floor.py).
// The source planes are views into heap blocks that end with the last sample of the window's last row and the packed planes blocks of exactly w x h samples, at every
// misalignment of the source against a 16-byte boundary, so a read or a write past a row's end or a misaligned 16-byte access is caught; the planes are compared with a
// per-sample loop. The walk - driven round by round the way run_rounds drives it - is held against the definition's loop on every floor, start and range of three D1 tables,
// one of them with the inversions of the synthetic atlas, for the minimum and the mean over two frames. Prints "ok".
#define RBT_HOSTEMU 1
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../rabbit-transcoding_amd/csrc/rbt_cloudmaps.h"
#include "../rabbit-transcoding_amd/host/rbt_d1_walk.h"
#include "../rabbit-transcoding_amd/host/rbt_floor_walk.h"

static int fail(const char* what, long a = 0, long b = 0, long c = 0) { printf("FAIL %s %ld %ld %ld\n", what, a, b, c); fflush(stdout); return 1; }
static uint32_t g_seed = 9753;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// n_pics windows of w x h samples at (x0, y0) of planes with row stride `stride`, the first plane `mis` samples behind a 16-byte boundary; the block ends with the last
// sample any window reads, the packed planes are a block of their own that ends with their last sample
static int gather_case(int w, int h, int stride, int x0, int y0, int mis, int n_pics) {
  const size_t plane = (size_t)stride * (y0 + h), n = plane * (n_pics - 1) + (size_t)(y0 + h - 1) * stride + x0 + w;
  uint16_t* mem = (uint16_t*)malloc((n + mis) * 2); uint16_t* out = (uint16_t*)malloc((size_t)w * h * n_pics * 2);
  if (!mem || !out || ((uintptr_t)mem & 15)) { printf("FAIL malloc\n"); exit(1); }                  // (blocks of 16 bytes and more start on a multiple of 16)
  uint16_t* src = mem + mis;
  for (size_t i = 0; i < n; i++) src[i] = (uint16_t)rnd();
  for (size_t i = 0; i < (size_t)w * h * n_pics; i++) out[i] = 0xEEEE;
  std::vector<RbtGatherPic> pics;
  for (int k = 0; k < n_pics; k++) pics.push_back(RbtGatherPic{src + plane * k + (size_t)y0 * stride + x0, out + (size_t)w * h * k, w, h, stride, 0});
  rbtk::launch_gather_luma(pics.data(), n_pics, RBT_GM_PIC_CHUNKS(w, h) + 300);      // (chunks past the last row do nothing: the launch of the largest picture's size)
  int bad = 0;
  for (int k = 0; k < n_pics && !bad; k++) for (int y = 0; y < h && !bad; y++) for (int x = 0; x < w; x++)
    if (out[((size_t)k * h + y) * w + x] != src[plane * k + (size_t)(y0 + y) * stride + x0 + x]) { bad = fail("gather", w, mis, x); break; }
  free(mem); free(out);
  return bad;
}

// two frames per QP: the second `gap` dB above the first
static std::vector<rbt_d1_result> frames_of(double db, double gap) {
  std::vector<rbt_d1_result> f(2); memset(f.data(), 0, sizeof(rbt_d1_result) * 2);
  f[0].psnr = (float)db; f[1].psnr = (float)(db + gap);
  return f;
}
struct Tried { std::vector<rbt_d1_result> d1; };
static int walk_case(const std::vector<std::vector<rbt_d1_result>>& t, int qp, int32_t floor_mdb, int stat, int lo, int hi) {
  rbt::QpWalk<Tried> w; rbt::FloorGoal g; g.floor_mdb = floor_mdb; w.lo = lo; w.hi = hi; rbt::floor_seed(w, g, qp);
  auto figure_of = [&](const Tried& x) { return rbt::d1_figure(x.d1, stat); };
  auto trial_meets = [&](const Tried& x) { return rbt::d1_meets(x.d1, stat, floor_mdb); };
  const int q0 = qp < lo ? lo : qp > hi ? hi : qp;
  if (g.q0 != q0 || w.toward != 1) return fail("seed", qp, g.q0, q0);
  auto D = [&](int q) { const double a = (double)t[q][0].psnr, b = (double)t[q][1].psnr; return stat == RBT_D1_MEAN ? (a + b) / 2 : (a < b ? a : b); };
  auto meets = [&](int q) { return D(q) >= floor_mdb / 1000.0; };
  if (rbt::d1_figure(t[q0], stat) != D(q0) || rbt::d1_meets(t[q0], stat, floor_mdb) != meets(q0)) return fail("figure", q0, stat);
  int qs = std::isinf(D(q0)) ? q0 : q0 + (int)(D(q0) - floor_mdb / 1000.0); qs = qs < lo ? lo : qs > hi ? hi : qs;
  int n_enc = 0, need = 0, dir = 0, round = 0; std::vector<int> qps, rule;
  for (;; round++) {
    const bool probe = !rbt::floor_probe(w, g, figure_of);
    if (probe) { need = g.q0; dir = 0; } else if (rbt::qp_walk_step(w, rbt::floor_holds(w, trial_meets), need, dir)) break;
    rbt::qp_round(w, need, dir, probe, qps);
    // the rule of the PSNR floor's rounds: the probe at q0 alone; then qs - 1, qs, qs + 1; then the QP asked for and the next one the same way
    rule.clear();
    if (round == 0) { if (!probe || need != q0 || dir != 0) return fail("first round", need, dir, q0); rule = {q0}; }
    else if (dir == 0) { if (probe || round != 1 || need != qs) return fail("start round", round, need, qs); rule = {qs - 1, qs, qs + 1}; }
    else { if (probe || dir != (meets(qs) ? 1 : -1)) return fail("direction", dir, qs, floor_mdb); rule = {need, need + dir}; }
    for (size_t i = rule.size(); i-- > 0;) if (rule[i] < lo || rule[i] > hi || w.tried.count(rule[i])) rule.erase(rule.begin() + i);
    if (qps != rule) return fail("round is not the rule's", round, need, dir);
    if (qps.empty()) return fail("empty round", floor_mdb, lo, hi);
    bool brought = false;
    for (int q : qps) { if (w.tried.count(q)) return fail("encoded twice", q, lo, hi); w.tried[q].d1 = t[q]; n_enc++; brought |= q == need; }
    if (!brought) return fail("round without the trial asked for", need, lo, hi);
  }
  int q = qs, met;
  if (meets(q)) { while (q < hi && meets(q + 1)) q++; met = 1; } else { while (q > lo && !meets(q)) q--; met = meets(q); }
  if (w.start != qs || w.qstar != q || w.met != met) return fail("walk", floor_mdb, w.qstar, q);
  if (n_enc > abs(q - qs) + 5) return fail("encodes", n_enc, q, qs);
  return 0;
}

int main() {
  // the widths of the tests, source rows at every misalignment of 0..7 samples, a window offset in both directions, 1 and 3 pictures a launch
  for (int w : {2, 8, 14, 72, 264}) for (int mis = 0; mis < 8; mis++) for (int n : {1, 3}) {
    if (gather_case(w, 5, w + 19, 0, 0, mis, n) || gather_case(w, 5, w + 19, 3, 2, mis, n) || gather_case(w, 5, w + 19, 19, 4, mis, n) || gather_case(w, 5, w + 19, 8, 1, mis, n)) return 1;
    if (gather_case(w, 3, w, 0, 0, mis, n) || gather_case(w, 1, w + 8, 8, 0, mis, n)) return 1;      // packed sources; one row
  }
  // D(q) and the floor's condition at their corners
  { std::vector<rbt_d1_result> f = frames_of(60.0, 2.0); double mean, least; rbt::d1_stats(f.data(), 2, &mean, &least);
    if (mean != 61.0 || least != 60.0 || rbt::d1_figure(f, RBT_D1_MIN) != 60.0 || rbt::d1_figure(f, RBT_D1_MEAN) != 61.0) return fail("stats");
    if (!rbt::d1_meets(f, RBT_D1_MIN, 60000) || rbt::d1_meets(f, RBT_D1_MIN, 60001) || !rbt::d1_meets(f, RBT_D1_MEAN, 61000) || rbt::d1_meets(f, RBT_D1_MEAN, 61001)) return fail("meets");
    f[1].psnr = INFINITY; if (rbt::d1_figure(f, RBT_D1_MIN) != 60.0 || !std::isinf(rbt::d1_figure(f, RBT_D1_MEAN)) || !rbt::d1_meets(f, RBT_D1_MEAN, 2000000000)) return fail("infinite");
    rbt::d1_stats(f.data(), 0, &mean, &least); if (mean != 0.0 || least != 0.0) return fail("no frames"); }
  // the walk on a monotone table of 0.2 dB a step, one with the inversions of the synthetic atlas, and a noisy one; every start, floors at and between the table's values
  std::vector<double> mono(52), inv(52), noisy(52);
  for (int q = 0; q < 52; q++) { mono[q] = 68.0 - 0.2 * q; inv[q] = 64.0 - 0.22 * q; noisy[q] = 66.0 - 0.2 * q + (rnd() % 1500) / 1000.0; }
  inv[24] = 58.545; inv[25] = 59.295; inv[26] = 58.246; inv[27] = 59.135;
  for (const std::vector<double>* tb : {&mono, &inv, &noisy}) {
    std::vector<std::vector<rbt_d1_result>> t; for (int q = 0; q < 52; q++) t.push_back(frames_of((*tb)[q], (q % 3) * 0.4));
    for (int stat = 0; stat < 2; stat++) for (int lo = 0; lo < 52; lo += 5) for (int hi = lo; hi < 52; hi += 6) for (int qp = 0; qp < 52; qp += 3) {
      for (int q = lo; q <= hi; q += 2) for (int d = -150; d <= 150; d += 150) if (walk_case(t, qp, (int32_t)((*tb)[q] * 1000) + d, stat, lo, hi)) return 1;
      if (walk_case(t, qp, 1, stat, lo, hi) || walk_case(t, qp, 120000, stat, lo, hi)) return 1;
    }
  }
  // clouds that come back exactly: psnr +inf, the walk starts at q0 and climbs while D stays infinite
  { std::vector<std::vector<rbt_d1_result>> t; for (int q = 0; q < 52; q++) t.push_back(frames_of(q < 12 ? (double)INFINITY : 70.0 - q, 0.0));
    if (walk_case(t, 5, 65000, 0, 0, 51) || walk_case(t, 11, 50000, 1, 0, 51) || walk_case(t, 0, 99000, 0, 0, 11)) return 1; }
  printf("ok\n");
  return 0;
}
