// TEST-ONLY: the serial bodies of the kernels of D2 per patch (csrc/rbt_score.h "D2/patch": p2_block, p2_cols, p2_fold) and the host-only figure / trial source of the D2
// floors (host/rbt_d1_figures.h: patch_d2_finish, patch_d2_figure, patch_d2_meets; host/rbt_patch_walk.h: patch_trial_d2) as a stand-alone host program, so that they can
// be built with -fsanitize=address,undefined and run on the CPU (tests/test_patch_d2.py).
//   sums    small clouds - 1 point, 63 / 64 / 65 and 255 / 256 / 257 points, one patch, one point per patch (256 distinct labels in a block), labels that change every 37
//           points, shuffled labels, patches without a point, a patch of duplicates, the tie between two patches in both orders, the last patch index of 65536, and 66 000
//           points (a second block in column 0) - indexed and scored by the bodies rbt_score runs (launch_sc_index, launch_sc_score with RBT_SCORE_D2), then summed per patch
//           and compared BIT FOR BIT with the definition applied literally: per patch the array w of the whole cloud's length, blocks of 256 folded, block sums added by
//           column, columns folded. Every scratch array is an exact-size heap block: an entry written past a block's range or a column past the last patch is caught.
//           With one patch the words are the whole's; S is zero again after the call.
//   adapter the figures of a patch from its sums and what the walk is told: a direction without a point has mse 0, a patch without a point has psnr +inf and meets any
//           floor, a floor is met at equality; a walk driven through the D2 source of a trial ends, and the source keeps the payload
// Prints "ok".
#define RBT_HOSTEMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../rabbit-transcoding_amd/csrc/rbt_score.h"
#include "../rabbit-transcoding_amd/host/rbt_patch_walk.h"      // (with rbt_d1_figures.h)

static int fail(const char* what, long a = 0, long b = 0, long c = 0) { printf("FAIL %s %ld %ld %ld\n", what, a, b, c); fflush(stdout); return 1; }
static uint32_t g_seed = 13579;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static const size_t VOL_WORDS = (size_t)1 << (3 * RBT_PCC_BITS - 5);
struct Cloud {
  int n = 0, lg = 0; int16_t* xyz = nullptr; int16_t* nrm = nullptr; uint32_t* maps = nullptr; uint32_t* vol = nullptr;      // vol: the bit volume with the coarse level behind it, kept clean between cases
  RbtScoreCloud view() const { const size_t s = (size_t)1 << lg; return RbtScoreCloud{xyz, nullptr, nrm, n, lg, vol, vol + VOL_WORDS, maps, maps + s, maps + 2 * s, maps + 6 * s}; }
  void set(const std::vector<int16_t>& p, bool normals) {
    n = (int)(p.size() / 3); lg = 4; while (((size_t)1 << lg) < 2 * (size_t)n) lg++;
    const size_t s = (size_t)1 << lg;
    xyz = (int16_t*)malloc(p.size() * 2); memcpy(xyz, p.data(), p.size() * 2);
    if (normals) { nrm = (int16_t*)malloc(p.size() * 2); for (size_t i = 0; i < p.size(); i++) nrm[i] = (int16_t)((int)(rnd() % 32769) - 16384); }
    maps = (uint32_t*)calloc(7 * s, 4); memset(maps + s, 0xFF, 4 * s);
    uint32_t scal[RBT_SC_SCALARS] = {0};
    const RbtScoreCloud S = view(); rbtk::launch_sc_index(&S, scal);
  }
  void drop() { const RbtScoreCloud S = view(); rbtk::launch_sc_clear(&S); free(xyz); free(nrm); free(maps); xyz = nullptr; nrm = nullptr; maps = nullptr; }
};

// the fixed order of include/rbt.h applied to an array of n values: -> sum, maximum
static void fixed_order(const std::vector<double>& w, double* sum, double* max) {
  const int n = (int)w.size(), nb = (n + 255) / 256;
  auto fold = [](double* s, double* m) { for (int h = 128; h > 0; h >>= 1) for (int t = 0; t < h; t++) { s[t] = s[t] + s[t + h]; if (m[t + h] > m[t]) m[t] = m[t + h]; } };
  std::vector<double> ps((size_t)nb), pm((size_t)nb);
  for (int b = 0; b < nb; b++) {
    double s[256], m[256];
    for (int t = 0; t < 256; t++) { const int i = b * 256 + t; s[t] = m[t] = i < n ? w[(size_t)i] : 0.0; }
    fold(s, m); ps[(size_t)b] = s[0]; pm[(size_t)b] = m[0];
  }
  double s[256], m[256];
  for (int t = 0; t < 256; t++) { s[t] = 0.0; m[t] = 0.0; for (int b = t; b < nb; b += 256) { s[t] = s[t] + ps[(size_t)b]; if (pm[(size_t)b] > m[t]) m[t] = pm[(size_t)b]; } }
  fold(s, m); *sum = s[0]; *max = m[0];
}

static int sum_case(Cloud& CA, Cloud& CB, const std::vector<int16_t>& a, const std::vector<int16_t>& b, const std::vector<uint32_t>& lab, int n_patches) {
  const int na = (int)(a.size() / 3), nb = (int)(b.size() / 3);
  const size_t blocks = ((size_t)(na > nb ? na : nb) + RBT_SC_SUM - 1) / RBT_SC_SUM, ents = blocks * RBT_SC_SUM;
  CA.set(a, true); CB.set(b, false);
  uint32_t* labels = (uint32_t*)malloc(4 * (size_t)nb); memcpy(labels, lab.data(), 4 * (size_t)nb);
  RbtScoreWork W; memset(&W, 0, sizeof(W));
  W.dist_a = (uint32_t*)malloc(4 * (size_t)na); W.dist_b = (uint32_t*)malloc(4 * (size_t)nb);
  W.acc_b = (long long*)calloc(3 * (size_t)nb, 8); W.cnt_b = (int32_t*)calloc((size_t)nb, 4);
  W.val_ab = (double*)malloc(8 * (size_t)na); W.val_ba = (double*)malloc(8 * (size_t)nb); W.part = (double*)malloc(16 * blocks);
  W.res = (unsigned long long*)calloc(RBT_SC_RESULTS, 8);
  RbtPatchD2Work P; P.ent_sum = (double*)malloc(8 * ents); P.ent_label = (uint32_t*)malloc(4 * ents); P.ent_n = (uint32_t*)malloc(4 * blocks); P.S = (double*)calloc((size_t)n_patches * RBT_SC_SUM, 8);
  unsigned long long* out = (unsigned long long*)calloc((size_t)RBT_P2_WORDS * n_patches, 8);
  const RbtScoreCloud A = CA.view(), B = CB.view();
  int bad = 0;
  rbtk::launch_sc_score(&A, &B, RBT_SCORE_D2, &W);
  rbtk::launch_p2_sums(&A, &B, labels, &W, &P, n_patches, out);
  // the definition: the label of every term, then per patch and direction the fixed order on the masked array
  std::vector<uint32_t> la((size_t)na, RBT_SC_NONE), lb((size_t)nb, RBT_SC_NONE);
  for (int i = 0; i < na; i++) { uint32_t l = 0, d = 0; if (pd_term_ab(&A, &B, labels, W.dist_a, i, &l, &d)) la[(size_t)i] = l; }
  for (int j = 0; j < nb; j++) if (W.dist_b[j] != RBT_SC_NONE) lb[(size_t)j] = lab[(size_t)j];
  const int check_all = n_patches <= 700;
  for (int k = 0; k < n_patches && !bad; k++) {
    if (!check_all && k > 2 && k < n_patches - 2 && k != 40000) { continue; }
    for (int dir = 0; dir < 2 && !bad; dir++) {
      const int n = dir ? nb : na; const std::vector<uint32_t>& l = dir ? lb : la; const double* v = dir ? W.val_ba : W.val_ab;
      std::vector<double> w((size_t)n, 0.0); unsigned long long cnt = 0;
      for (int i = 0; i < n; i++) if (l[(size_t)i] == (uint32_t)k) { w[(size_t)i] = v[i]; cnt++; }
      double s, m; fixed_order(w, &s, &m);
      const unsigned long long* o = out + (size_t)RBT_P2_WORDS * k + dir;
      if (o[RBT_P2_N_AB] != cnt || memcmp(&o[RBT_P2_SSE_AB], &s, 8) || memcmp(&o[RBT_P2_MAX_AB], &m, 8)) bad = fail("words", k, dir, n);
    }
  }
  if (n_patches == 1 && !bad) {
    const unsigned long long* r = W.res;
    if (out[RBT_P2_SSE_AB] != r[RBT_SC_D2_AB] || out[RBT_P2_MAX_AB] != r[RBT_SC_D2_AB + 1] || out[RBT_P2_SSE_BA] != r[RBT_SC_D2_BA] || out[RBT_P2_MAX_BA] != r[RBT_SC_D2_BA + 1]) bad = fail("one patch is not the whole", na, nb);
  }
  for (size_t i = 0; i < (size_t)n_patches * RBT_SC_SUM && !bad; i++) if (P.S[i] != 0.0) bad = fail("S is not zero after the call", (long)i);
  free(labels); free(W.dist_a); free(W.dist_b); free(W.acc_b); free(W.cnt_b); free(W.val_ab); free(W.val_ba); free(W.part); free(W.res);
  free(P.ent_sum); free(P.ent_label); free(P.ent_n); free(P.S); free(out);
  CA.drop(); CB.drop();
  return bad;
}
static std::vector<int16_t> random_points(int n, int lo, int span) { std::vector<int16_t> p(3 * (size_t)n); for (auto& v : p) v = (int16_t)(lo + (int)(rnd() % span)); return p; }
static std::vector<uint32_t> runs(int n, int len) { std::vector<uint32_t> l((size_t)n); for (int i = 0; i < n; i++) l[i] = (uint32_t)(i / len); return l; }

static int adapter_case() {
  rbt_patch_d2 d; memset(&d, 0, sizeof(d));
  rbt::patch_d2_finish(&d, 1023);
  if (d.mse_ab != 0.0f || d.mse_ba != 0.0f || !std::isinf(rbt::patch_d2_figure(d)) || rbt::patch_d2_figure(d) < 0 || !rbt::patch_d2_meets(d, 2000000000)) return fail("a patch without a point");
  d.n_ba = 4; d.sse_ba = 8.0; d.max_ba = 3.0;                            // mse 2 one way, no point the other way
  rbt::patch_d2_finish(&d, 1023);
  if (d.mse_ab != 0.0f || d.mse_ba != 2.0f || d.psnr != 10 * log10f(3 * 1023.0f * 1023.0f / 2.0f)) return fail("one direction");
  d.n_ab = 3; d.sse_ab = 9.0;                                            // the larger mse decides
  rbt::patch_d2_finish(&d, 1023);
  if (d.mse_ab != 3.0f || d.psnr != 10 * log10f(3 * 1023.0f * 1023.0f / 3.0f)) return fail("the worse direction");
  // the whole frame's routine on the same sums gives the same floats
  if (d.mse_ab != rbt::geometry_mse(9.0, 3) || d.psnr != rbt::geometry_psnr(1023, rbt::geometry_mse(9.0, 3))) return fail("not the one float routine");
  const double fig = rbt::patch_d2_figure(d); const int32_t at = (int32_t)(fig * 1000.0);
  if (!rbt::patch_d2_meets(d, at) || rbt::patch_d2_meets(d, at + 1) || !rbt::patch_d2_meets(d, 0)) return fail("meets", at);
  // a walk on such figures through the D2 source: three patches, one without a point, about 0.4 dB per QP step
  std::vector<int32_t> floors = {60000, 61500, 70000};
  rbt::PatchWalk w, plain; rbt::patch_walk_seed(w, 30, 20, 40, 0, floors); rbt::patch_walk_seed(plain, 30, 20, 40, 0, floors);
  for (int trial = 0;; trial++) {
    if (trial > 200) return fail("walk does not end");
    std::vector<rbt_patch_d2> pd(3), copy; rbt_d2_result whole; memset(&whole, 0, sizeof(whole)); whole.psnr = 50.0f + (float)trial; whole.n_b = 9;
    for (int k = 0; k < 3; k++) {
      rbt_patch_d2& p = pd[(size_t)k]; memset(&p, 0, sizeof(p));
      if (k < 2) { p.n_ab = p.n_ba = 1000; p.sse_ab = p.sse_ba = 1000 * 3.0 * 1023 * 1023 / pow(10.0, (62.0 + k - 0.04 * w.q[k]) / 10.0); }
      rbt::patch_d2_finish(&p, 1023);
    }
    copy = pd;
    rbt::PatchTrial said; rbt::PatchD2 kept; double f[3]; char m[3];
    rbt::patch_trial_d2(pd, whole, floors, said, kept);
    if (said.figure.size() != 3 || said.meets.size() != 3 || kept.patches.size() != 3 || memcmp(&kept.whole, &whole, sizeof(whole))) return fail("trial size");
    for (int k = 0; k < 3; k++) {
      f[k] = rbt::patch_d2_figure(copy[(size_t)k]); m[k] = rbt::patch_d2_meets(copy[(size_t)k], floors[(size_t)k]);
      if (memcmp(&kept.patches[(size_t)k], &copy[(size_t)k], sizeof(rbt_patch_d2))) return fail("d2 payload", trial, k);
      if (memcmp(&said.figure[(size_t)k], &f[k], sizeof(double)) || (said.meets[(size_t)k] != 0) != (m[k] != 0)) return fail("d2 source is not patch_d2_figure / patch_d2_meets", trial, k);
    }
    const bool a = rbt::patch_walk_step(w, said.figure.data(), said.meets.data()), b = rbt::patch_walk_step(plain, f, m);
    if (a != b || w.q != plain.q || w.met != plain.met || w.failed != plain.failed) return fail("walks part", trial);
    if (a) break;
  }
  if (!w.met[2] || w.q[2] != 30 || !w.met[0]) return fail("walk result", w.q[0], w.q[1], w.q[2]);
  return 0;
}

int main() {
  if (adapter_case()) return 1;
  Cloud CA, CB;
  CA.vol = (uint32_t*)calloc(VOL_WORDS + RBT_SC_COARSE_WORDS, 4); CB.vol = (uint32_t*)calloc(VOL_WORDS + RBT_SC_COARSE_WORDS, 4);
  if (!CA.vol || !CB.vol) return fail("calloc");
  if (sum_case(CA, CB, {7, 8, 9}, {7, 8, 12}, {0}, 1)) return 1;
  for (int n : {63, 64, 65, 255, 256, 257}) {
    const std::vector<int16_t> a = random_points(300, 100, 9), b = random_points(n, 100, 9);
    if (sum_case(CA, CB, a, b, runs(n, 37), (n + 36) / 37)) return 1;                              // labels change in mid-wave
    if (sum_case(CA, CB, b, a, runs(300, 1), 300)) return 1;                                        // one point per patch: up to 256 distinct labels in a block
    if (sum_case(CA, CB, a, b, std::vector<uint32_t>((size_t)n, 0), 1)) return 1;                   // one patch: the whole's words
    std::vector<uint32_t> gap = runs(n, 20); for (auto& l : gap) if (l >= 2) l += 3;                // patches 2, 3, 4 without a point, and room behind the last label
    if (sum_case(CA, CB, a, b, gap, (n + 19) / 20 + 5)) return 1;
    std::vector<uint32_t> mixed((size_t)n); for (auto& l : mixed) l = rnd() % 11;                   // no wave is uniform
    if (sum_case(CA, CB, a, b, mixed, 11)) return 1;
  }
  {                                                                                                  // a patch of duplicates of an earlier patch's points
    std::vector<int16_t> a = random_points(200, 500, 7), b = random_points(120, 500, 7); std::vector<uint32_t> lab = runs(120, 60);
    for (int i = 0; i < 30; i++) { for (int c = 0; c < 3; c++) b.push_back(b[3 * (size_t)i + c]); lab.push_back(2); }
    if (sum_case(CA, CB, a, b, lab, 3)) return 1;
  }
  // the tie between two patches, either point first; far points and the corners of the volume with the last patch index
  if (sum_case(CA, CB, {5, 5, 5}, {5, 5, 6, 5, 6, 5, 40, 40, 40}, {1, 0, 2}, 3) || sum_case(CA, CB, {5, 5, 5}, {5, 6, 5, 5, 5, 6, 40, 40, 40}, {1, 0, 2}, 3)) return 1;
  if (sum_case(CA, CB, {0, 0, 0, 1023, 1023, 1023, 31, 32, 33}, {1023, 0, 1023, 0, 1023, 0, 32, 31, 33, 700, 2, 900}, {0, 65535, 40000, 65535}, 65536)) return 1;
  {                                                                                                  // 66 000 points in B, 258 blocks: columns 0 and 1 add a second block
    const std::vector<int16_t> a = random_points(3000, 200, 40), b = random_points(66000, 200, 40);
    if (sum_case(CA, CB, a, b, runs(66000, 97), (66000 + 96) / 97)) return 1;
  }
  for (size_t i = 0; i < VOL_WORDS + RBT_SC_COARSE_WORDS; i += 4099) if (CA.vol[i] | CB.vol[i]) return fail("volume not clean", (long)i);
  free(CA.vol); free(CB.vol);
  printf("ok\n");
  return 0;
}
