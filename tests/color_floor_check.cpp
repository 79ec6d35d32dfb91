// TEST-ONLY: the bodies of the recolouring route - the recolour of an index and the colour walks on stored distances (csrc/rbt_score.h), the gather on the three planes of
// 4:2:0 pictures (csrc/rbt_cloudmaps.h) - and the host half of a colour floor (host/rbt_color_walk.h, host/rbt_floor_walk.h, host/rbt_qp_walk.h) as a stand-alone host program, so that they can be
// built with -fsanitize=address,undefined and run on the CPU (tests/test_color_floor.py). Points, colours, maps and distances are heap blocks that end with the last point /
// slot, the coded pictures blocks that end with the last sample a window reads, so a step past an end is caught. A recoloured index is held against the index of the same
// points built with the new colours, word for word; the colour walks against launch_sc_score's sums. Prints "ok".
#define RBT_HOSTEMU 1
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../rabbit-transcoding_amd/csrc/rbt_score.h"
#include "../rabbit-transcoding_amd/csrc/rbt_cloudmaps.h"
#include "../rabbit-transcoding_amd/host/rbt_color_walk.h"
#include "../rabbit-transcoding_amd/host/rbt_floor_walk.h"

static int fail(const char* what, long a = 0, long b = 0, long c = 0) { printf("FAIL %s %ld %ld %ld\n", what, a, b, c); fflush(stdout); return 1; }
static uint32_t g_seed = 2468;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }
template <class T> static T* block(size_t n) { T* p = (T*)malloc(n ? n * sizeof(T) : 1); if (!p) { printf("FAIL malloc\n"); exit(1); } return p; }

// an indexed cloud on heap blocks of exactly its sizes
struct Cloud {
  int n = 0, lg = 0; int16_t* xyz = nullptr; uint8_t* rgb = nullptr; uint32_t* maps = nullptr; uint32_t* vol = nullptr; uint32_t n_merged = 0;
  size_t slots() const { return (size_t)1 << lg; }
  RbtScoreCloud view() const { uint32_t* m = maps; return RbtScoreCloud{xyz, rgb, nullptr, n, lg, vol, vol + ((size_t)1 << (3 * RBT_PCC_BITS - 5)), m, m + slots(), m + 2 * slots(), m + 6 * slots()}; }
  void build(const std::vector<int16_t>& pts, uint32_t* volume, const uint8_t* colours = nullptr) {
    n = (int)(pts.size() / 3); vol = volume; lg = 4; while (((size_t)1 << lg) < 2 * (size_t)n) lg++;
    xyz = block<int16_t>(3 * (size_t)n); memcpy(xyz, pts.data(), 6 * (size_t)n);
    rgb = block<uint8_t>(3 * (size_t)n); for (int i = 0; i < 3 * n; i++) rgb[i] = colours ? colours[i] : (uint8_t)rnd();
    maps = block<uint32_t>(7 * slots()); memset(maps, 0, 28 * slots()); for (size_t s = 0; s < slots(); s++) maps[slots() + s] = 0xFFFFFFFFu;
    const RbtScoreCloud S = view(); uint32_t scal[RBT_SC_SCALARS] = {0};
    rbtk::launch_sc_index(&S, scal); n_merged = scal[RBT_SC_N_MERGED];
  }
  void drop() { const RbtScoreCloud S = view(); rbtk::launch_sc_clear(&S); free(xyz); free(rgb); free(maps); xyz = nullptr; rgb = nullptr; maps = nullptr; }
};

// new colours through launch_sc_recolor == the index of the same points built with them
static int recolor_case(const std::vector<int16_t>& pts, uint32_t* vol_a, uint32_t* vol_b) {
  Cloud a; a.build(pts, vol_a);
  for (int round = 0; round < 2; round++) {
    for (int i = 0; i < 3 * a.n; i++) a.rgb[i] = (uint8_t)(round ? 255 : rnd());      // (second round: the largest sums)
    const RbtScoreCloud S = a.view();
    rbtk::launch_sc_recolor(&S);
    rbtk::launch_sc_recolor(&S);                                                     // twice: the same words
    Cloud c; c.build(pts, vol_b, a.rgb);
    if (c.n_merged != a.n_merged || c.lg != a.lg) return fail("merged", a.n);
    if (memcmp(a.maps, c.maps, 28 * a.slots())) return fail("recolour differs from a fresh index", a.n, round);
    c.drop();
  }
  a.drop();
  return 0;
}

// the colour sums from stored distances == launch_sc_score's, before and after both clouds get new colours
static int walks_case(const std::vector<int16_t>& pa, const std::vector<int16_t>& pb, uint32_t* vol_a, uint32_t* vol_b) {
  Cloud a, b; a.build(pa, vol_a); b.build(pb, vol_b);
  uint32_t* dist = block<uint32_t>((size_t)a.n + b.n);
  const RbtScoreCloud A = a.view(), B = b.view();
  rbtk::launch_sc_search(&A, &B, dist, dist + a.n);
  for (int round = 0; round < 3; round++) {
    if (round == 1) { for (int i = 0; i < 3 * b.n; i++) b.rgb[i] = (uint8_t)rnd(); rbtk::launch_sc_recolor(&B); }
    if (round == 2) { for (int i = 0; i < 3 * a.n; i++) a.rgb[i] = (uint8_t)(i % 3 ? 0 : 255); rbtk::launch_sc_recolor(&A); }
    unsigned long long* res = block<unsigned long long>(RBT_SC_COLOR_RESULTS); memset(res, 0, 8 * RBT_SC_COLOR_RESULTS);
    rbtk::launch_sc_color_walks(&A, &B, dist, dist + a.n, res);
    uint32_t* d2 = block<uint32_t>((size_t)a.n + b.n); unsigned long long full[RBT_SC_RESULTS] = {0};
    RbtScoreWork W; memset(&W, 0, sizeof(W)); W.dist_a = d2; W.dist_b = d2 + a.n; W.res = full;
    rbtk::launch_sc_score(&A, &B, RBT_SCORE_COLOR, &W);
    if (memcmp(d2, dist, 4 * ((size_t)a.n + b.n))) return fail("distances", a.n, b.n);
    for (int c = 0; c < 3; c++) if (res[c] != full[RBT_SC_COL_AB + c] || res[3 + c] != full[RBT_SC_COL_BA + c]) return fail("colour sums", round, c, a.n);
    free(res); free(d2);
  }
  free(dist); a.drop(); b.drop();
  return 0;
}

// n_pics coded 4:2:0 pictures (luma stride x rows, then two chroma planes cstride x crows) `mis` samples behind a 16-byte boundary, in a block that ends with the last
// sample of the last picture's Cr window; three descriptors a picture into a packed block of exactly n_pics * w * h * 3 / 2 samples
static int gather_case(int w, int h, int stride, int cstride, int x0, int y0, int mis, int n_pics) {
  const int rows = y0 + h, crows = rows / 2, cw = w / 2, ch = h / 2;
  const size_t luma = (size_t)stride * rows, chroma = (size_t)cstride * crows, pic = luma + 2 * chroma, ys = (size_t)w * h, cs = ys / 4, fs = ys + 2 * cs;
  const size_t n = pic * (n_pics - 1) + luma + chroma + (size_t)(y0 / 2 + ch - 1) * cstride + x0 / 2 + cw;
  uint16_t* mem = block<uint16_t>(n + mis); uint16_t* out = block<uint16_t>(fs * n_pics);
  if ((uintptr_t)mem & 15) return fail("malloc alignment");
  uint16_t* src = mem + mis;
  for (size_t i = 0; i < n; i++) src[i] = (uint16_t)rnd();
  for (size_t i = 0; i < fs * n_pics; i++) out[i] = 0xEEEE;
  std::vector<RbtGatherPic> pics;
  for (int k = 0; k < n_pics; k++) {
    const uint16_t* p = src + pic * k; uint16_t* o = out + fs * k;
    pics.push_back(RbtGatherPic{p + (size_t)y0 * stride + x0, o, w, h, stride, 0});
    for (int c = 0; c < 2; c++) pics.push_back(RbtGatherPic{p + luma + chroma * c + (size_t)(y0 / 2) * cstride + x0 / 2, o + ys + cs * c, cw, ch, cstride, 0});
  }
  rbtk::launch_gather_luma(pics.data(), (int)pics.size(), RBT_GM_PIC_CHUNKS(w, h) + 300);
  int bad = 0;
  for (int k = 0; k < n_pics && !bad; k++) {
    for (int y = 0; y < h && !bad; y++) for (int x = 0; x < w; x++) if (out[fs * k + (size_t)y * w + x] != src[pic * k + (size_t)(y0 + y) * stride + x0 + x]) { bad = fail("gather luma", w, mis, x); break; }
    for (int c = 0; c < 2 && !bad; c++) for (int y = 0; y < ch && !bad; y++) for (int x = 0; x < cw; x++)
      if (out[fs * k + ys + cs * c + (size_t)y * cw + x] != src[pic * k + luma + chroma * c + (size_t)(y0 / 2 + y) * cstride + x0 / 2 + x]) { bad = fail("gather chroma", w, mis, x); break; }
  }
  free(mem); free(out);
  return bad;
}

// two frames per QP: the second `gap` dB above the first in the channel under test, the other channels far off
static std::vector<rbt_color_result> frames_of(double db, double gap, int channel) {
  std::vector<rbt_color_result> f(2); memset(f.data(), 0, sizeof(rbt_color_result) * 2);
  for (int c = 0; c < 3; c++) { f[0].psnr[c] = c == channel ? (float)db : 5.0f + c; f[1].psnr[c] = c == channel ? (float)(db + gap) : 95.0f; }
  return f;
}
struct Tried { std::vector<rbt_color_result> color; };
static int walk_case(const std::vector<std::vector<rbt_color_result>>& t, int qp, int32_t floor_mdb, int stat, int ch, int lo, int hi) {
  rbt::QpWalk<Tried> w; rbt::FloorGoal g; g.floor_mdb = floor_mdb; w.lo = lo; w.hi = hi; rbt::floor_seed(w, g, qp);
  auto figure_of = [&](const Tried& x) { return rbt::color_figure(x.color, stat, ch); };
  auto trial_meets = [&](const Tried& x) { return rbt::color_meets(x.color, stat, ch, floor_mdb); };
  const int q0 = qp < lo ? lo : qp > hi ? hi : qp;
  if (g.q0 != q0 || w.toward != 1) return fail("seed", qp, g.q0, q0);
  auto D = [&](int q) { const double a = (double)t[q][0].psnr[ch], b = (double)t[q][1].psnr[ch]; return stat == RBT_D1_MEAN ? (a + b) / 2 : (a < b ? a : b); };
  auto meets = [&](int q) { return D(q) >= floor_mdb / 1000.0; };
  if (rbt::color_figure(t[q0], stat, ch) != D(q0) || rbt::color_meets(t[q0], stat, ch, floor_mdb) != meets(q0)) return fail("figure", q0, stat);
  int qs = std::isinf(D(q0)) ? q0 : q0 + (int)(D(q0) - floor_mdb / 1000.0); qs = qs < lo ? lo : qs > hi ? hi : qs;
  int n_enc = 0, need = 0, dir = 0, round = 0; std::vector<int> qps, rule;
  for (;; round++) {
    const bool probe = !rbt::floor_probe(w, g, figure_of);
    if (probe) { need = g.q0; dir = 0; } else if (rbt::qp_walk_step(w, rbt::floor_holds(w, trial_meets), need, dir)) break;
    rbt::qp_round(w, need, dir, probe, qps);
    rule.clear();
    if (round == 0) { if (!probe || need != q0 || dir != 0) return fail("first round", need, dir, q0); rule = {q0}; }
    else if (dir == 0) { if (probe || round != 1 || need != qs) return fail("start round", round, need, qs); rule = {qs - 1, qs, qs + 1}; }
    else { if (probe || dir != (meets(qs) ? 1 : -1)) return fail("direction", dir, qs, floor_mdb); rule = {need, need + dir}; }
    for (size_t i = rule.size(); i-- > 0;) if (rule[i] < lo || rule[i] > hi || w.tried.count(rule[i])) rule.erase(rule.begin() + i);
    if (qps != rule) return fail("round is not the rule's", round, need, dir);
    if (qps.empty()) return fail("empty round", floor_mdb, lo, hi);
    bool brought = false;
    for (int q : qps) { if (w.tried.count(q)) return fail("encoded twice", q, lo, hi); w.tried[q].color = t[q]; n_enc++; brought |= q == need; }
    if (!brought) return fail("round without the trial asked for", need, lo, hi);
  }
  int q = qs, met;
  if (meets(q)) { while (q < hi && meets(q + 1)) q++; met = 1; } else { while (q > lo && !meets(q)) q--; met = meets(q); }
  if (w.start != qs || w.qstar != q || w.met != met) return fail("walk", floor_mdb, w.qstar, q);
  if (n_enc > abs(q - qs) + 5) return fail("encodes", n_enc, q, qs);
  return 0;
}

int main() {
  const size_t vol_words = ((size_t)1 << (3 * RBT_PCC_BITS - 5)) + RBT_SC_COARSE_WORDS;
  uint32_t* vol_a = (uint32_t*)calloc(vol_words, 4); uint32_t* vol_b = (uint32_t*)calloc(vol_words, 4);
  if (!vol_a || !vol_b) return fail("calloc");
  // clouds of 1, 255, 256, 257 and 700 points from a small cube (voxels of one, two and many points), one voxel of 300 points, the corners of the volume
  std::vector<int16_t> pts;
  auto add = [&](int x, int y, int z) { pts.push_back((int16_t)x); pts.push_back((int16_t)y); pts.push_back((int16_t)z); };
  for (int n : {1, 255, 256, 257, 700}) {
    pts.clear(); for (int i = 0; i < n; i++) add(28 + rnd() % 7, 1017 + rnd() % 7, rnd() % 7);                 // across the word boundary x = 31 | 32, at the faces y = 1023 and z = 0
    if (recolor_case(pts, vol_a, vol_b)) return 1;
  }
  pts.clear(); for (int i = 0; i < 300; i++) add(5, 6, 7); add(5, 6, 8); add(5, 6, 8); add(0, 0, 0); add(1023, 1023, 1023);
  if (recolor_case(pts, vol_a, vol_b)) return 1;
  // the colour walks: clouds with ties (a cube drawn twice), a single point on either side, far neighbours
  std::vector<int16_t> pa, pb;
  auto draw = [&](std::vector<int16_t>& v, int n, int lo, int span) { v.clear(); for (int i = 0; i < 3 * n; i++) v.push_back((int16_t)(lo + rnd() % span)); };
  draw(pa, 600, 100, 9); draw(pb, 500, 100, 9);
  if (walks_case(pa, pb, vol_a, vol_b)) return 1;
  draw(pa, 1, 100, 9); if (walks_case(pa, pb, vol_a, vol_b) || walks_case(pb, pa, vol_a, vol_b) || walks_case(pa, pa, vol_a, vol_b)) return 1;
  draw(pa, 257, 30, 4); draw(pb, 256, 90, 5);
  if (walks_case(pa, pb, vol_a, vol_b)) return 1;
  // the 4:2:0 gather: chroma rows of 1, 7, 36 and 132 samples, a chroma stride of its own, every misalignment, windows offset in both directions, 1 and 3 pictures
  for (int w : {2, 14, 72, 264}) for (int mis = 0; mis < 8; mis++) for (int n : {1, 3}) {
    if (gather_case(w, 6, w + 18, w / 2 + 11, 0, 0, mis, n) || gather_case(w, 6, w + 18, w / 2 + 11, 2, 4, mis, n) || gather_case(w, 6, w + 18, w / 2 + 11, 18, 6, mis, n)) return 1;
    if (gather_case(w, 2, w, w / 2, 0, 0, mis, n) || gather_case(w, 4, w + 16, w / 2 + 8, 16, 0, mis, n)) return 1;      // packed pictures of two rows; equally aligned rows
  }
  // D(q) and the floor's condition at their corners, per channel
  for (int ch = 0; ch < 3; ch++) {
    std::vector<rbt_color_result> f = frames_of(40.0, 2.0, ch); double mean[3], least[3]; rbt::color_stats(f.data(), 2, mean, least);
    if (mean[ch] != 41.0 || least[ch] != 40.0 || rbt::color_figure(f, RBT_D1_MIN, ch) != 40.0 || rbt::color_figure(f, RBT_D1_MEAN, ch) != 41.0) return fail("stats", ch);
    if (!rbt::color_meets(f, RBT_D1_MIN, ch, 40000) || rbt::color_meets(f, RBT_D1_MIN, ch, 40001) || !rbt::color_meets(f, RBT_D1_MEAN, ch, 41000) || rbt::color_meets(f, RBT_D1_MEAN, ch, 41001)) return fail("meets", ch);
    f[1].psnr[ch] = INFINITY; if (rbt::color_figure(f, RBT_D1_MIN, ch) != 40.0 || !std::isinf(rbt::color_figure(f, RBT_D1_MEAN, ch)) || !rbt::color_meets(f, RBT_D1_MEAN, ch, 2000000000)) return fail("infinite", ch);
    rbt::color_stats(f.data(), 0, mean, least); if (mean[ch] != 0.0 || least[ch] != 0.0) return fail("no frames", ch);
  }
  // the walk on a table of about 0.5 dB a step, one with inversions and a noisy one; every start, floors at and between the table's values
  std::vector<double> mono(52), inv(52), noisy(52);
  for (int q = 0; q < 52; q++) { mono[q] = 55.0 - 0.5 * q; inv[q] = 52.0 - 0.45 * q; noisy[q] = 50.0 - 0.4 * q + (rnd() % 1500) / 1000.0; }
  inv[30] = 37.9; inv[31] = 38.6; inv[32] = 37.2; inv[33] = 37.8;
  for (const std::vector<double>* tb : {&mono, &inv, &noisy}) for (int ch = 0; ch < 3; ch++) {
    std::vector<std::vector<rbt_color_result>> t; for (int q = 0; q < 52; q++) t.push_back(frames_of((*tb)[q], (q % 3) * 0.4, ch));
    for (int stat = 0; stat < 2; stat++) for (int lo = 0; lo < 52; lo += 7) for (int hi = lo; hi < 52; hi += 8) for (int qp = 0; qp < 52; qp += 5) {
      for (int q = lo; q <= hi; q += 3) for (int d = -150; d <= 150; d += 150) if (walk_case(t, qp, (int32_t)((*tb)[q] * 1000) + d, stat, ch, lo, hi)) return 1;
      if (walk_case(t, qp, 1, stat, ch, lo, hi) || walk_case(t, qp, 120000, stat, ch, lo, hi)) return 1;
    }
  }
  { std::vector<std::vector<rbt_color_result>> t; for (int q = 0; q < 52; q++) t.push_back(frames_of(q < 12 ? (double)INFINITY : 60.0 - q, 0.0, 0));
    if (walk_case(t, 5, 45000, 0, 0, 0, 51) || walk_case(t, 11, 40000, 1, 0, 0, 51) || walk_case(t, 0, 99000, 0, 0, 0, 11)) return 1; }
  free(vol_a); free(vol_b);
  printf("ok\n");
  return 0;
}
