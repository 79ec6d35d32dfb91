// TEST-ONLY: the serial body of the kernel of the colour PSNR per patch (csrc/rbt_score.h "col/patch": pc_term, pc_add, launch_pc_sums) and the host-only figure / trial source
// of the colour floors held patch by patch (host/rbt_color_walk.h: patch_color_finish, patch_color_figure, patch_color_meets; host/rbt_patch_walk.h: patch_trial_color) as a
// stand-alone host program, so that they can be built with -fsanitize=address,undefined and run on the CPU (tests/test_patch_color.py).
//   sums    small clouds with colours - 1 point, 63 / 64 / 65 and 255 / 256 / 257 points, one patch, one point per patch, labels that change every 37 points, shuffled
//           labels, patches without a point, a patch of duplicates in other colours, the tie between two patches in both orders, the last patch index of 65536, a few
//           thousand points - indexed and searched by the bodies rbt_score runs (launch_sc_index, launch_sc_search), then summed per patch and compared with the two walks
//           the single walk replaces: the colour error of sc_color_walk and the label of pd_term_ab / pd_term_ba, added per patch here. The words are an exact-size heap
//           block: a word written past the last patch is caught. Over the patches the words add up to launch_sc_color_walks' sums.
//   adapter the figures of a patch from its sums and what the walk is told: a direction without a point has mse 0, a patch without a point has psnr +inf and meets any
//           floor, a floor is met at equality, the channel picks the figure; a walk driven through the colour source of a trial ends, and the source keeps the payload
// Prints "ok".
#define RBT_HOSTEMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../rabbit-transcoding_amd/csrc/rbt_score.h"
#include "../rabbit-transcoding_amd/host/rbt_patch_walk.h"      // (with rbt_color_walk.h)

static int fail(const char* what, long a = 0, long b = 0, long c = 0) { printf("FAIL %s %ld %ld %ld\n", what, a, b, c); fflush(stdout); return 1; }
static uint32_t g_seed = 24680;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static const size_t VOL_WORDS = (size_t)1 << (3 * RBT_PCC_BITS - 5);
struct Cloud {
  int n = 0, lg = 0; int16_t* xyz = nullptr; uint8_t* rgb = nullptr; uint32_t* maps = nullptr; uint32_t* vol = nullptr;      // vol: the bit volume with the coarse level behind it, kept clean between cases
  RbtScoreCloud view() const { const size_t s = (size_t)1 << lg; return RbtScoreCloud{xyz, rgb, nullptr, n, lg, vol, vol + VOL_WORDS, maps, maps + s, maps + 2 * s, maps + 6 * s}; }
  void set(const std::vector<int16_t>& p) {
    n = (int)(p.size() / 3); lg = 4; while (((size_t)1 << lg) < 2 * (size_t)n) lg++;
    const size_t s = (size_t)1 << lg;
    xyz = (int16_t*)malloc(p.size() * 2); memcpy(xyz, p.data(), p.size() * 2);
    rgb = (uint8_t*)malloc(p.size()); for (size_t i = 0; i < p.size(); i++) rgb[i] = (uint8_t)(rnd() & 255u);
    maps = (uint32_t*)calloc(7 * s, 4); memset(maps + s, 0xFF, 4 * s);
    uint32_t scal[RBT_SC_SCALARS] = {0};
    const RbtScoreCloud S = view(); rbtk::launch_sc_index(&S, scal);
  }
  void drop() { const RbtScoreCloud S = view(); rbtk::launch_sc_clear(&S); free(xyz); free(rgb); free(maps); xyz = nullptr; rgb = nullptr; maps = nullptr; }
};

static int sum_case(Cloud& CA, Cloud& CB, const std::vector<int16_t>& a, const std::vector<int16_t>& b, const std::vector<uint32_t>& lab, int n_patches) {
  const int na = (int)(a.size() / 3), nb = (int)(b.size() / 3);
  CA.set(a); CB.set(b);
  uint32_t* labels = (uint32_t*)malloc(4 * (size_t)nb); memcpy(labels, lab.data(), 4 * (size_t)nb);
  uint32_t* dist_a = (uint32_t*)malloc(4 * (size_t)na); uint32_t* dist_b = (uint32_t*)malloc(4 * (size_t)nb);
  unsigned long long* out = (unsigned long long*)calloc((size_t)RBT_PC_WORDS * n_patches, 8);
  unsigned long long* res = (unsigned long long*)calloc(RBT_SC_COLOR_RESULTS, 8);
  const RbtScoreCloud A = CA.view(), B = CB.view();
  int bad = 0;
  rbtk::launch_sc_search(&A, &B, dist_a, dist_b);
  rbtk::launch_pc_sums(&A, &B, labels, dist_a, dist_b, out);
  rbtk::launch_sc_color_walks(&A, &B, dist_a, dist_b, res);
  // the two walks the single walk replaces
  std::vector<unsigned long long> want((size_t)RBT_PC_WORDS * n_patches, 0);
  for (int dir = 0; dir < 2; dir++) for (int i = 0; i < (dir ? nb : na); i++) {
    long long e[3] = {0, 0, 0}; uint32_t l = 0, d = 0;
    const int has_e = sc_color_walk(&A, &B, dist_a, dist_b, dir, i, e);
    const int has_l = dir ? pd_term_ba(labels, dist_b, i, &l, &d) : pd_term_ab(&A, &B, labels, dist_a, i, &l, &d);
    if (has_e != has_l) { bad = fail("representatives differ", dir, i); break; }
    if (!has_e) continue;
    if (l >= (uint32_t)n_patches) { bad = fail("label", dir, i, l); break; }
    unsigned long long* w = &want[(size_t)RBT_PC_WORDS * l];
    for (int c = 0; c < 3; c++) w[(dir ? RBT_PC_SSE_BA : RBT_PC_SSE_AB) + c] += (unsigned long long)(e[c] * e[c]);
    w[dir ? RBT_PC_N_BA : RBT_PC_N_AB]++;
  }
  if (!bad && memcmp(out, want.data(), want.size() * 8)) {
    for (size_t k = 0; k < want.size(); k++) if (out[k] != want[k]) { bad = fail("words", (long)(k / RBT_PC_WORDS), (long)(k % RBT_PC_WORDS), na); break; }
  }
  unsigned long long tot[RBT_PC_WORDS] = {0};
  for (int k = 0; k < n_patches; k++) for (int w = 0; w < RBT_PC_WORDS; w++) tot[w] += out[(size_t)RBT_PC_WORDS * k + w];
  for (int c = 0; c < 3 && !bad; c++) if (tot[RBT_PC_SSE_AB + c] != res[c] || tot[RBT_PC_SSE_BA + c] != res[3 + c]) bad = fail("the patches do not add up to the whole", c, na, nb);
  free(labels); free(dist_a); free(dist_b); free(out); free(res);
  CA.drop(); CB.drop();
  return bad;
}
static std::vector<int16_t> random_points(int n, int lo, int span) { std::vector<int16_t> p(3 * (size_t)n); for (auto& v : p) v = (int16_t)(lo + (int)(rnd() % span)); return p; }
static std::vector<uint32_t> runs(int n, int len) { std::vector<uint32_t> l((size_t)n); for (int i = 0; i < n; i++) l[i] = (uint32_t)(i / len); return l; }

static int adapter_case() {
  rbt_patch_color d; memset(&d, 0, sizeof(d));
  rbt::patch_color_finish(&d);
  for (int c = 0; c < 3; c++)
    if (d.mse_ab[c] != 0.0f || d.mse_ba[c] != 0.0f || d.mse[c] != 0.0f || !std::isinf(rbt::patch_color_figure(d, c)) || rbt::patch_color_figure(d, c) < 0 || !rbt::patch_color_meets(d, c, 2000000000)) return fail("a patch without a point", c);
  const double unit = 2550000.0 * 2550000.0;
  d.n_ba = 4; d.sse_ba[0] = (uint64_t)(unit / 250.0); d.sse_ba[1] = (uint64_t)(unit / 2500.0); d.sse_ba[2] = 0;      // mse 1e-3, 1e-4 and 0 one way, no point the other way
  rbt::patch_color_finish(&d);
  if (d.mse_ab[0] != 0.0f || d.mse_ba[0] != rbt::color_mse(d.sse_ba[0], 4.0) || d.mse[0] != d.mse_ba[0] || d.psnr[0] != rbt::color_psnr(d.mse_ba[0]) || !std::isinf(d.psnr[2])) return fail("one direction");
  if (!(d.psnr[0] < d.psnr[1]) || rbt::patch_color_figure(d, 1) != (double)d.psnr[1]) return fail("the channel picks the figure");
  d.n_ab = 2; d.sse_ab[0] = (uint64_t)(unit / 25.0);                      // the larger mse, the smaller psnr decide
  rbt::patch_color_finish(&d);
  if (d.mse[0] != d.mse_ab[0] || d.psnr[0] != rbt::color_psnr(d.mse_ab[0]) || d.mse[1] != d.mse_ba[1]) return fail("the worse direction");
  const double fig = rbt::patch_color_figure(d, 0); const int32_t at = (int32_t)(fig * 1000.0);
  if (!rbt::patch_color_meets(d, 0, at) || rbt::patch_color_meets(d, 0, at + 1) || !rbt::patch_color_meets(d, 0, 0)) return fail("meets", at);
  // a walk on such figures through the colour source: three patches, one without a point, about 0.5 dB per QP step on channel 1
  std::vector<int32_t> floors = {38000, 39500, 70000};
  rbt::PatchWalk w, plain; rbt::patch_walk_seed(w, 30, 20, 40, 0, floors); rbt::patch_walk_seed(plain, 30, 20, 40, 0, floors);
  for (int trial = 0;; trial++) {
    if (trial > 200) return fail("walk does not end");
    std::vector<rbt_patch_color> pc(3), copy; rbt_color_result whole; memset(&whole, 0, sizeof(whole)); whole.psnr[1] = 30.0f + (float)trial; whole.n_b = 9;
    for (int k = 0; k < 3; k++) {
      rbt_patch_color& p = pc[(size_t)k]; memset(&p, 0, sizeof(p));
      if (k < 2) { p.n_ab = p.n_ba = 1000; p.sse_ab[1] = p.sse_ba[1] = (uint64_t)(1000 * unit / pow(10.0, (54.3 + k - 0.5 * w.q[k]) / 10.0)); p.sse_ab[0] = p.sse_ba[0] = 77; }
      rbt::patch_color_finish(&p);
    }
    copy = pc;
    rbt::PatchTrial said; rbt::PatchColor kept; double f[3]; char m[3];
    rbt::patch_trial_color(pc, whole, 1, floors, said, kept);
    if (said.figure.size() != 3 || said.meets.size() != 3 || kept.patches.size() != 3 || memcmp(&kept.whole, &whole, sizeof(whole))) return fail("trial size");
    for (int k = 0; k < 3; k++) {
      f[k] = rbt::patch_color_figure(copy[(size_t)k], 1); m[k] = rbt::patch_color_meets(copy[(size_t)k], 1, floors[(size_t)k]);
      if (memcmp(&kept.patches[(size_t)k], &copy[(size_t)k], sizeof(rbt_patch_color))) return fail("colour payload", trial, k);
      if (memcmp(&said.figure[(size_t)k], &f[k], sizeof(double)) || (said.meets[(size_t)k] != 0) != (m[k] != 0)) return fail("colour source is not patch_color_figure / patch_color_meets", trial, k);
    }
    const bool a = rbt::patch_walk_step(w, said.figure.data(), said.meets.data()), b = rbt::patch_walk_step(plain, f, m);
    if (a != b || w.q != plain.q || w.met != plain.met || w.failed != plain.failed) return fail("walks part", trial);
    if (a) break;
  }
  if (!w.met[2] || w.q[2] != 30 || !w.met[0] || w.q[0] == 30) return fail("walk result", w.q[0], w.q[1], w.q[2]);
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
    if (sum_case(CA, CB, b, a, runs(300, 1), 300)) return 1;                                        // one point per patch
    if (sum_case(CA, CB, a, b, std::vector<uint32_t>((size_t)n, 0), 1)) return 1;                   // one patch
    std::vector<uint32_t> gap = runs(n, 20); for (auto& l : gap) if (l >= 2) l += 3;                // patches 2, 3, 4 without a point, and room behind the last label
    if (sum_case(CA, CB, a, b, gap, (n + 19) / 20 + 5)) return 1;
    std::vector<uint32_t> mixed((size_t)n); for (auto& l : mixed) l = rnd() % 11;                   // shuffled labels
    if (sum_case(CA, CB, a, b, mixed, 11)) return 1;
  }
  {                                                                                                  // a patch of duplicates of an earlier patch's points (their colours differ: Cloud::set)
    std::vector<int16_t> a = random_points(200, 500, 7), b = random_points(120, 500, 7); std::vector<uint32_t> lab = runs(120, 60);
    for (int i = 0; i < 30; i++) { for (int c = 0; c < 3; c++) b.push_back(b[3 * (size_t)i + c]); lab.push_back(2); }
    if (sum_case(CA, CB, a, b, lab, 3)) return 1;
  }
  // the tie between two patches, either point first; far points and the corners of the volume with the last patch index
  if (sum_case(CA, CB, {5, 5, 5}, {5, 5, 6, 5, 6, 5, 40, 40, 40}, {1, 0, 2}, 3) || sum_case(CA, CB, {5, 5, 5}, {5, 6, 5, 5, 5, 6, 40, 40, 40}, {1, 0, 2}, 3)) return 1;
  if (sum_case(CA, CB, {0, 0, 0, 1023, 1023, 1023, 31, 32, 33}, {1023, 0, 1023, 0, 1023, 0, 32, 31, 33, 700, 2, 900}, {0, 65535, 40000, 65535}, 65536)) return 1;
  {                                                                                                  // a few thousand points: many blocks of 256
    const std::vector<int16_t> a = random_points(3000, 200, 14), b = random_points(5000, 200, 14);
    if (sum_case(CA, CB, a, b, runs(5000, 97), (5000 + 96) / 97)) return 1;
  }
  for (size_t i = 0; i < VOL_WORDS + RBT_SC_COARSE_WORDS; i += 4099) if (CA.vol[i] | CB.vol[i]) return fail("volume not clean", (long)i);
  free(CA.vol); free(CB.vol);
  printf("ok\n");
  return 0;
}
