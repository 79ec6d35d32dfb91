// TEST-ONLY: the serial bodies of the kernels of D1 per patch (csrc/rbt_score.h "patches": pd_label_item, the label check, pd_term_ab / pd_term_ba / pd_add) as a
// stand-alone host program, so that they can be built with -fsanitize=address,undefined and run on the CPU (tests/test_patch_d1.py).
//   sums    small clouds - 1 point, 63 / 64 / 65 and 255 / 256 / 257 points, one patch, one point per patch, labels that change every 37 points, patches without a point,
//           a patch of duplicates, the tie between two patches in both orders, the last patch index of 65536 - indexed and searched by the bodies rbt_score runs
//           (launch_sc_index, launch_sc_search), then summed per patch and compared with a serial restatement of the definition on the points themselves. Points, labels,
//           distances and the words per patch are exact-size heap blocks: a label read past the cloud or a word written past the last patch is caught
//   labels  work items with their offsets, among them items without a point and the last one: every point gets its item's patch, nothing is written past the cloud
//   adapter the figures of a patch from its words (patch_d1_finish) and what the walk is told (patch_d1_figure, patch_d1_meets): a direction without a point has mse 0,
//           a patch without a point has psnr +inf and meets any floor, a floor is met at equality; then a walk driven by such figures through the D1 source of a
//           trial (patch_trial_d1) ends
//   seam    two walks with one seed, one fed by the PSNR source (patch_trial_psnr, from fold words) and one by the D1 source (patch_trial_d1), trial by trial beside walks
//           fed by patch_figure / patch_meets and patch_d1_figure / patch_d1_meets on the same inputs: the same figures, conditions and vectors, and the payloads kept
//   check   the error word is set by a label that equals the patch count and by nothing less
// Prints "ok".
#define RBT_HOSTEMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../rabbit-transcoding_amd/csrc/rbt_score.h"
#include "../rabbit-transcoding_amd/host/rbt_patch_walk.h"      // (with rbt_d1_figures.h)

static int fail(const char* what, long a = 0, long b = 0, long c = 0) { printf("FAIL %s %ld %ld %ld\n", what, a, b, c); fflush(stdout); return 1; }
static uint32_t g_seed = 24680;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static const size_t VOL_WORDS = (size_t)1 << (3 * RBT_PCC_BITS - 5);
struct Cloud {
  int n = 0, lg = 0; int16_t* xyz = nullptr; uint32_t* maps = nullptr; uint32_t* vol = nullptr;      // vol: the bit volume with the coarse level behind it, kept clean between cases
  RbtScoreCloud view() const { const size_t s = (size_t)1 << lg; return RbtScoreCloud{xyz, nullptr, nullptr, n, lg, vol, vol + VOL_WORDS, maps, maps + s, maps + 2 * s, maps + 6 * s}; }
  void set(const std::vector<int16_t>& p) {
    n = (int)(p.size() / 3); lg = 4; while (((size_t)1 << lg) < 2 * (size_t)n) lg++;
    const size_t s = (size_t)1 << lg;
    xyz = (int16_t*)malloc(p.size() * 2); memcpy(xyz, p.data(), p.size() * 2);
    maps = (uint32_t*)calloc(7 * s, 4); memset(maps + s, 0xFF, 4 * s);
    uint32_t scal[RBT_SC_SCALARS] = {0};
    const RbtScoreCloud S = view(); rbtk::launch_sc_index(&S, scal);
  }
  void drop() { const RbtScoreCloud S = view(); rbtk::launch_sc_clear(&S); free(xyz); free(maps); xyz = nullptr; maps = nullptr; }
};

static long d2_of(const int16_t* p, const int16_t* q) { long s = 0; for (int c = 0; c < 3; c++) { const long e = (long)p[c] - q[c]; s += e * e; } return s; }
static bool is_rep(const std::vector<int16_t>& p, int i) { for (int j = 0; j < i; j++) if (!d2_of(&p[3 * i], &p[3 * j])) return false; return true; }

static int sum_case(Cloud& CA, Cloud& CB, const std::vector<int16_t>& a, const std::vector<int16_t>& b, const std::vector<uint32_t>& lab, int n_patches) {
  const int na = (int)(a.size() / 3), nb = (int)(b.size() / 3);
  CA.set(a); CB.set(b);
  uint32_t* labels = (uint32_t*)malloc(4 * (size_t)nb); memcpy(labels, lab.data(), 4 * (size_t)nb);
  uint32_t* dist_a = (uint32_t*)malloc(4 * (size_t)na); uint32_t* dist_b = (uint32_t*)malloc(4 * (size_t)nb);
  unsigned long long* out = (unsigned long long*)calloc((size_t)RBT_PD_WORDS * n_patches, 8);
  const RbtScoreCloud A = CA.view(), B = CB.view();
  int bad = 0;
  uint32_t err = 0;
  rbtk::launch_pd_check(labels, nb, (uint32_t)n_patches, &err);
  if (err) bad = fail("labels refused", nb, n_patches);
  rbtk::launch_sc_search(&A, &B, dist_a, dist_b);
  rbtk::launch_pd_sums(&A, &B, labels, dist_a, dist_b, out);
  // the definition on the points themselves
  std::vector<unsigned long long> want((size_t)RBT_PD_WORDS * n_patches, 0);
  for (int i = 0; i < na && !bad; i++) {
    if (!is_rep(a, i)) continue;
    long best = -1; int owner = -1;
    for (int j = 0; j < nb; j++) { const long d = d2_of(&a[3 * i], &b[3 * j]); if (best < 0 || d < best) { best = d; owner = j; } }      // the first j at the least distance: the lowest index, a representative
    unsigned long long* w = &want[(size_t)RBT_PD_WORDS * lab[owner]];
    w[RBT_PD_SSE_AB] += (unsigned long long)best; w[RBT_PD_N_AB]++; if ((unsigned long long)best > w[RBT_PD_MAX_AB]) w[RBT_PD_MAX_AB] = (unsigned long long)best;
  }
  for (int j = 0; j < nb && !bad; j++) {
    if (!is_rep(b, j)) continue;
    long best = -1;
    for (int i = 0; i < na; i++) { const long d = d2_of(&b[3 * j], &a[3 * i]); if (best < 0 || d < best) best = d; }
    unsigned long long* w = &want[(size_t)RBT_PD_WORDS * lab[j]];
    w[RBT_PD_SSE_BA] += (unsigned long long)best; w[RBT_PD_N_BA]++; if ((unsigned long long)best > w[RBT_PD_MAX_BA]) w[RBT_PD_MAX_BA] = (unsigned long long)best;
  }
  for (size_t i = 0; i < want.size() && !bad; i++) if (out[i] != want[i]) bad = fail("words", na, nb, (long)i);
  free(labels); free(dist_a); free(dist_b); free(out);
  CA.drop(); CB.drop();
  return bad;
}
static std::vector<int16_t> random_points(int n, int lo, int span) { std::vector<int16_t> p(3 * (size_t)n); for (auto& v : p) v = (int16_t)(lo + (int)(rnd() % span)); return p; }
static std::vector<uint32_t> runs(int n, int len) { std::vector<uint32_t> l((size_t)n); for (int i = 0; i < n; i++) l[i] = (uint32_t)(i / len); return l; }

static int label_case() {
  // items of patches 0, 0, 3, 3, 3, 7 with 5, 0, 130, 64, 0, 1 points
  const uint32_t items[6] = {0u << 16 | 0, 0u << 16 | 1, 3u << 16 | 0, 3u << 16 | 1, 3u << 16 | 2, 7u << 16 | 9}, counts[6] = {5, 0, 130, 64, 0, 1};
  uint32_t* it = (uint32_t*)malloc(sizeof(items)); memcpy(it, items, sizeof(items));
  uint32_t* off = (uint32_t*)malloc(7 * 4); off[0] = 0; for (int t = 0; t < 6; t++) off[t + 1] = off[t] + counts[t];
  const uint32_t total = off[6];
  uint32_t* labels = (uint32_t*)malloc(4 * (size_t)total); memset(labels, 0xA5, 4 * (size_t)total);
  rbtk::launch_pd_labels(it, off, 6, labels);
  int bad = 0;
  for (int t = 0; t < 6 && !bad; t++) for (uint32_t i = off[t]; i < off[t + 1]; i++) if (labels[i] != items[t] >> 16) { bad = fail("label", t, (long)i, labels[i]); break; }
  for (int lanes : {64, 7}) {                                          // the kernel's form: the lanes of a wave stride through the item
    memset(labels, 0xA5, 4 * (size_t)total);
    for (int t = 0; t < 6; t++) for (int lane = 0; lane < lanes; lane++) pd_label_item(it, off, t, lane, lanes, labels);
    for (int t = 0; t < 6 && !bad; t++) for (uint32_t i = off[t]; i < off[t + 1]; i++) if (labels[i] != items[t] >> 16) { bad = fail("label by lanes", t, (long)i, lanes); break; }
  }
  uint32_t err = 0;
  rbtk::launch_pd_check(labels, (int)total, 8, &err); if (err) bad = fail("check refuses 7 of 8");
  rbtk::launch_pd_check(labels, (int)total, 7, &err); if (!err) bad = fail("check accepts 7 of 7");
  free(it); free(off); free(labels);
  return bad;
}

static int adapter_case() {
  rbt_patch_d1 d; memset(&d, 0, sizeof(d));
  rbt::patch_d1_finish(&d, 1023);
  if (d.mse_ab != 0.0f || d.mse_ba != 0.0f || !std::isinf(rbt::patch_d1_figure(d)) || rbt::patch_d1_figure(d) < 0 || !rbt::patch_d1_meets(d, 2000000000)) return fail("a patch without a point");
  d.n_ba = 4; d.sse_ba = 8; d.max_ba = 3;                                // mse 2 one way, no point the other way
  rbt::patch_d1_finish(&d, 1023);
  const float want = 10 * log10f(3 * 1023.0f * 1023.0f / 2.0f);
  if (d.mse_ab != 0.0f || d.mse_ba != 2.0f || d.psnr != want) return fail("one direction");
  d.n_ab = 3; d.sse_ab = 9;                                              // the larger mse decides
  rbt::patch_d1_finish(&d, 1023);
  if (d.mse_ab != 3.0f || d.psnr != 10 * log10f(3 * 1023.0f * 1023.0f / 3.0f)) return fail("the worse direction");
  const double fig = rbt::patch_d1_figure(d); const int32_t at = (int32_t)(fig * 1000.0);
  if (!rbt::patch_d1_meets(d, at) || rbt::patch_d1_meets(d, at + 1) || !rbt::patch_d1_meets(d, 0)) return fail("meets", at);
  // a walk on such figures: three patches, one without a point, about 0.4 dB per QP step
  std::vector<int32_t> floors = {60000, 61500, 70000};
  rbt::PatchWalk w; rbt::patch_walk_seed(w, 30, 20, 40, 0, floors);
  for (int trial = 0;; trial++) {
    if (trial > 200) return fail("walk does not end");
    std::vector<rbt_patch_d1> pd(3); rbt_d1_result whole; memset(&whole, 0, sizeof(whole));
    for (int k = 0; k < 3; k++) {
      rbt_patch_d1& p = pd[(size_t)k]; memset(&p, 0, sizeof(p));
      if (k < 2) { p.n_ab = p.n_ba = 1000; p.sse_ab = p.sse_ba = (uint64_t)(1000 * 3.0 * 1023 * 1023 / pow(10.0, (62.0 + k - 0.04 * w.q[k]) / 10.0)); }
      rbt::patch_d1_finish(&p, 1023);
    }
    rbt::PatchTrial said; rbt::PatchD1 kept;
    rbt::patch_trial_d1(pd, whole, floors, said, kept);
    if (said.figure.size() != 3 || said.meets.size() != 3 || kept.patches.size() != 3) return fail("trial size");
    if (rbt::patch_walk_step(w, said.figure.data(), said.meets.data())) break;
  }
  if (!w.met[2] || w.q[2] != 30 || !w.met[0]) return fail("walk result", w.q[0], w.q[1], w.q[2]);
  return 0;
}

// one seed, two kinds of figure: each source against the plain functions on the same inputs, and the walks they drive against each other
static int seam_case() {
  const int np = 5, bit_depth = 10, peak = 1023;
  for (int region = 0; region < 2; region++) {
    const std::vector<int32_t> floors = {38000, 0, 45500, 90000, 41000};
    const std::vector<uint64_t> samples = {2048, 512, 0, 8192, 1024};      // patch 2 has no sample: figure 0, meets
    rbt::PatchWalk ws[4];      // PSNR through the source / by the functions, D1 through the source / by the functions
    for (rbt::PatchWalk& w : ws) rbt::patch_walk_seed(w, 30, 18, 44, 0, floors);
    for (int trial = 0; !ws[0].settled || !ws[2].settled; trial++) {
      if (trial > 400) return fail("seam walks do not end", region);
      if (!ws[0].settled) {
        // fold words as k_patch_fold leaves them: sse, sse_occ, n_occ per patch, then the background's - about a dB per QP step, the occupied half a little better
        uint64_t* words = (uint64_t*)malloc((size_t)(np + 1) * 24);      // an exact-size block: a read past the background's words is caught
        for (int k = 0; k < np; k++) {
          const double mse = 1023.0 * 1023.0 / pow(10.0, (70.0 + 2 * k - 0.9 * ws[0].q[(size_t)k]) / 10.0);
          words[3 * k] = (uint64_t)(mse * (double)samples[(size_t)k]); words[3 * k + 2] = samples[(size_t)k] / 2; words[3 * k + 1] = (uint64_t)(0.8 * mse * (double)words[3 * k + 2]);
        }
        if (trial == 1) words[3] = words[4] = 0;                           // no error at all: the figure is infinite and meets
        for (int c = 0; c < 3; c++) words[3 * np + c] = 1000 + (uint64_t)(7 * trial + c);
        rbt::PatchTrial said; rbt::PatchPsnr kept; std::vector<double> f((size_t)np); std::vector<char> m((size_t)np);
        rbt::patch_trial_psnr(words, samples, region, bit_depth, floors, said, kept);
        if ((int)said.figure.size() != np || (int)said.meets.size() != np || (int)kept.patches.size() != np) return fail("psnr trial size", region, trial);
        for (int k = 0; k < np; k++) {
          rbt::PatchSums s; s.sse = words[3 * k]; s.sse_occ = words[3 * k + 1]; s.samples_occ = words[3 * k + 2]; s.samples = samples[(size_t)k];
          f[(size_t)k] = rbt::patch_figure(s, region, bit_depth); m[(size_t)k] = rbt::patch_meets(s, region, floors[(size_t)k], bit_depth);
          const rbt::PatchSums& g = kept.patches[(size_t)k];
          if (g.sse != s.sse || g.sse_occ != s.sse_occ || g.samples_occ != s.samples_occ || g.samples != s.samples) return fail("psnr payload", region, trial, k);
          if (memcmp(&said.figure[(size_t)k], &f[(size_t)k], sizeof(double)) || (said.meets[(size_t)k] != 0) != (m[(size_t)k] != 0)) return fail("psnr source is not patch_figure / patch_meets", region, trial, k);
        }
        for (int c = 0; c < 3; c++) if (kept.background[c] != words[3 * np + c]) return fail("background", region, trial, c);
        free(words);
        const bool a = rbt::patch_walk_step(ws[0], said.figure.data(), said.meets.data()), b = rbt::patch_walk_step(ws[1], f.data(), m.data());
        if (a != b || ws[0].q != ws[1].q || ws[0].met != ws[1].met || ws[0].failed != ws[1].failed) return fail("psnr walks part", region, trial);
      }
      if (!ws[2].settled) {
        std::vector<rbt_patch_d1> pd((size_t)np), copy; rbt_d1_result whole; memset(&whole, 0, sizeof(whole)); whole.psnr = 60.0f + (float)trial; whole.n_a = 77;
        for (int k = 0; k < np; k++) {
          rbt_patch_d1& p = pd[(size_t)k]; memset(&p, 0, sizeof(p));
          if (k != 2) { p.n_ab = 900 + (uint64_t)k; p.n_ba = 1000; p.sse_ba = (uint64_t)(1000 * 3.0 * peak * peak / pow(10.0, (70.0 + 2 * k - 0.9 * ws[2].q[(size_t)k]) / 10.0)); p.sse_ab = p.sse_ba / 2; }      // patch 2 has no point
          rbt::patch_d1_finish(&p, peak);
        }
        copy = pd;
        rbt::PatchTrial said; rbt::PatchD1 kept; std::vector<double> f((size_t)np); std::vector<char> m((size_t)np);
        rbt::patch_trial_d1(pd, whole, floors, said, kept);
        if ((int)said.figure.size() != np || (int)said.meets.size() != np || (int)kept.patches.size() != np) return fail("d1 trial size", region, trial);
        if (memcmp(&kept.whole, &whole, sizeof(whole))) return fail("whole frame", region, trial);
        for (int k = 0; k < np; k++) {
          f[(size_t)k] = rbt::patch_d1_figure(copy[(size_t)k]); m[(size_t)k] = rbt::patch_d1_meets(copy[(size_t)k], floors[(size_t)k]);
          if (memcmp(&kept.patches[(size_t)k], &copy[(size_t)k], sizeof(rbt_patch_d1))) return fail("d1 payload", region, trial, k);
          if (memcmp(&said.figure[(size_t)k], &f[(size_t)k], sizeof(double)) || (said.meets[(size_t)k] != 0) != (m[(size_t)k] != 0)) return fail("d1 source is not patch_d1_figure / patch_d1_meets", region, trial, k);
        }
        if (!std::isinf(said.figure[2]) || !said.meets[2]) return fail("a patch without a point through the source", region, trial);
        const bool a = rbt::patch_walk_step(ws[2], said.figure.data(), said.meets.data()), b = rbt::patch_walk_step(ws[3], f.data(), m.data());
        if (a != b || ws[2].q != ws[3].q || ws[2].met != ws[3].met || ws[2].failed != ws[3].failed) return fail("d1 walks part", region, trial);
      }
    }
    // what the floors say of either walk's end: the floor nothing reaches sits at lo, the patch without a floor never failed
    for (int w = 0; w < 4; w += 2) if (ws[w].q[3] != 18 || ws[w].met[3] || ws[w].failed[1] || !ws[w].met[2]) return fail("seam walk result", region, w, ws[w].q[3]);
  }
  return 0;
}

int main() {
  if (adapter_case() || seam_case()) return 1;
  Cloud CA, CB;
  CA.vol = (uint32_t*)calloc(VOL_WORDS + RBT_SC_COARSE_WORDS, 4); CB.vol = (uint32_t*)calloc(VOL_WORDS + RBT_SC_COARSE_WORDS, 4);
  if (!CA.vol || !CB.vol) return fail("calloc");
  if (label_case()) return 1;
  if (sum_case(CA, CB, {7, 8, 9}, {7, 8, 12}, {0}, 1)) return 1;
  for (int n : {63, 64, 65, 255, 256, 257}) {
    const std::vector<int16_t> a = random_points(300, 100, 9), b = random_points(n, 100, 9);
    if (sum_case(CA, CB, a, b, runs(n, 37), (n + 36) / 37)) return 1;                              // labels change in mid-wave
    if (sum_case(CA, CB, b, a, runs(300, 1), 300)) return 1;                                        // one point per patch
    if (sum_case(CA, CB, a, b, std::vector<uint32_t>((size_t)n, 0), 1)) return 1;                   // one patch
    std::vector<uint32_t> gap = runs(n, 20); for (auto& l : gap) if (l >= 2) l += 3;                // patches 2, 3, 4 without a point, and room behind the last label
    if (sum_case(CA, CB, a, b, gap, (n + 19) / 20 + 5)) return 1;
  }
  {                                                                                                  // a patch of duplicates of an earlier patch's points
    std::vector<int16_t> a = random_points(200, 500, 7), b = random_points(120, 500, 7); std::vector<uint32_t> lab = runs(120, 60);
    for (int i = 0; i < 30; i++) { for (int c = 0; c < 3; c++) b.push_back(b[3 * (size_t)i + c]); lab.push_back(2); }
    if (sum_case(CA, CB, a, b, lab, 3)) return 1;
  }
  // the tie between two patches, either point first; far points and the corners of the volume
  if (sum_case(CA, CB, {5, 5, 5}, {5, 5, 6, 5, 6, 5, 40, 40, 40}, {1, 0, 2}, 3) || sum_case(CA, CB, {5, 5, 5}, {5, 6, 5, 5, 5, 6, 40, 40, 40}, {1, 0, 2}, 3)) return 1;
  if (sum_case(CA, CB, {0, 0, 0, 1023, 1023, 1023, 31, 32, 33}, {1023, 0, 1023, 0, 1023, 0, 32, 31, 33, 700, 2, 900}, {0, 65535, 40000, 65535}, 65536)) return 1;
  for (size_t i = 0; i < VOL_WORDS + RBT_SC_COARSE_WORDS; i += 4099) if (CA.vol[i] | CB.vol[i]) return fail("volume not clean", (long)i);
  free(CA.vol); free(CB.vol);
  printf("ok\n");
  return 0;
}
