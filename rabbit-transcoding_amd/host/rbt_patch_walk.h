// PSNR floors held patch by patch (include/rbt.h, "PSNR floors held patch by patch"): the walk of one point-cloud frame. Where every other walk of the library
// moves one QP (rbt_qp_walk.h), this one moves a vector - one QP per patch - and what a trial is coded with is the map rbt_qp_map_from_patches makes of that vector. The
// distortion of a patch depends on its neighbours' QPs (shared CTBs take the lower QP; intra prediction and the loop filters cross CTB borders) and is not monotone in its
// own, so the walk is the definition: it ends on a vector whose map was encoded and measured. What it reaches is a map under which every patch meets its floor or sits at lo,
// reached by this walk - NOT a proof of the cheapest such map.
//   trial 0   q[k] = q0 for every patch
//   update    after a trial, every patch on its own figure (PSNR in dB of its region R_k, patch_figure) and condition (patch_meets) with its floor F_k:
//               does not meet:  failed[k] = 1; if q[k] > lo: q[k] -= max(1, (int)(F_k - figure_k)), clamped at lo
//               meets, has never failed, q[k] < hi, figure finite, (int)(figure_k - F_k) >= 1:  q[k] += (int)(figure_k - F_k), clamped at hi
//               else it stays
//             The casts truncate toward zero: one QP step is about 1 dB, the PSNR floor's own argument; no tuned constant.
//   end       no q[k] changed: the frame has settled on this trial. A patch moves up until its first failure and only down after it, so the vector never repeats: at most
//             the sum over the patches of (hi - q0) + (hi - lo) + 1 trials. max_trials (0 = no cap): a frame that reaches it settles on its last trial, met as measured.
// The walk takes figures and `meets` and nothing else. What they are made of is a kind of figure: a source that turns what a trial brought into a PatchTrial and keeps the
// kind's payload for the report (below: luma PSNR from the fold words, D1, D2 and the colour PSNR from the trial's cloud). A further kind is one more payload and one more source.
// Plain host code without a device call, so that tests/patch_floor_check.cpp and tests/patch_d1_check.cpp can run it under the sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#include "rbt_quality_walk.h"
#include "rbt_d1_figures.h"
#include "rbt_color_walk.h"

namespace rbt {
// the folded sums of one region in the two pictures of a frame: the words of k_patch_fold and the displayed luma samples the region holds
struct PatchSums { uint64_t sse = 0, samples = 0, sse_occ = 0, samples_occ = 0; };
// rules 2 and 4 of the PSNR floor on a region's sums; a region without a sample has the figure 0 and meets
inline double patch_figure(const PatchSums& s, int region, int bit_depth) { return region ? quality_psnr(s.sse_occ, s.samples_occ, bit_depth) : quality_psnr(s.sse, s.samples, bit_depth); }
inline bool patch_meets(const PatchSums& s, int region, int32_t floor_mdb, int bit_depth) {
  const uint64_t sse = region ? s.sse_occ : s.sse, n = region ? s.samples_occ : s.samples;
  if (!n || !sse) return true;
  return quality_psnr(sse, n, bit_depth) >= floor_mdb / 1000.0;
}
// R_k in CTB units (c0, r0, c1, r1, half-open): the CTBs the patch's rectangle meets, by rbt_qp_map_from_patches' rule, clipping included; 0, 0, 0, 0 for a patch without one
inline void patch_region(int width, int height, int occupancy_resolution, int u0, int v0, int size_u0, int size_v0, int log2_ctb, int32_t out[4]) {
  const long long res = occupancy_resolution;
  const long long x0 = std::max(0ll, u0 * res), y0 = std::max(0ll, v0 * res);
  const long long x1 = std::min((long long)width, ((long long)u0 + size_u0) * res), y1 = std::min((long long)height, ((long long)v0 + size_v0) * res);
  if (x0 >= x1 || y0 >= y1) { out[0] = out[1] = out[2] = out[3] = 0; return; }
  out[0] = (int32_t)(x0 >> log2_ctb); out[1] = (int32_t)(y0 >> log2_ctb); out[2] = (int32_t)((x1 - 1) >> log2_ctb) + 1; out[3] = (int32_t)((y1 - 1) >> log2_ctb) + 1;
}
// the displayed luma samples of a region in the two pictures of a frame
inline uint64_t patch_region_samples(const int32_t r[4], int width, int height, int log2_ctb) {
  if (r[0] >= r[2] || r[1] >= r[3]) return 0;
  const long long w = std::min((long long)width, (long long)r[2] << log2_ctb) - ((long long)r[0] << log2_ctb), h = std::min((long long)height, (long long)r[3] << log2_ctb) - ((long long)r[1] << log2_ctb);
  return 2 * (uint64_t)w * (uint64_t)h;
}

struct PatchWalk {
  int lo = 0, hi = 51, q0 = 0, max_trials = 0, n_trials = 0; bool settled = false;
  std::vector<int> q;                 // the vector of the trial to run next; once settled, of the last trial
  std::vector<char> failed, met;      // per patch: it has missed its floor in some trial; it met it in the last trial
  std::vector<int32_t> floor_mdb;     // F_k
  std::vector<double> figure;         // of the last trial
};
inline void patch_walk_seed(PatchWalk& w, int q0, int lo, int hi, int max_trials, const std::vector<int32_t>& floors) {
  w = PatchWalk(); w.lo = lo; w.hi = hi; w.q0 = std::min(hi, std::max(lo, q0)); w.max_trials = max_trials;
  const size_t n = floors.size();
  w.q.assign(n, w.q0); w.failed.assign(n, 0); w.met.assign(n, 0); w.floor_mdb = floors; w.figure.assign(n, 0.0);
}
// the trial at w.q has come back with the figure and the condition of every patch; true: the frame has settled on it, false: w.q is the next trial's vector
inline bool patch_walk_step(PatchWalk& w, const double* figure, const char* meets) {
  const size_t n = w.q.size();
  w.n_trials++;
  for (size_t k = 0; k < n; k++) { w.figure[k] = figure[k]; w.met[k] = meets[k] ? 1 : 0; if (!meets[k]) w.failed[k] = 1; }
  if (w.max_trials && w.n_trials >= w.max_trials) return w.settled = true;
  bool changed = false;
  for (size_t k = 0; k < n; k++) {
    const double F = w.floor_mdb[k] / 1000.0; const int was = w.q[k];
    if (!meets[k]) { if (was > w.lo) w.q[k] = std::max(w.lo, was - std::max(1, (int)std::min(64.0, F - figure[k]))); }
    else if (!w.failed[k] && was < w.hi && std::isfinite(figure[k])) { const int up = (int)std::min(64.0, figure[k] - F); if (up >= 1) w.q[k] = std::min(w.hi, was + up); }
    changed |= w.q[k] != was;
  }
  return w.settled = !changed;
}

// What a trial said about the patches of one frame - per patch the figure and its condition against F_k, as patch_walk_step takes them - and per kind of figure what the
// report needs of the trial beside that: the folded sums of every region and of the background; every patch's D1 and the whole frame's
struct PatchTrial { std::vector<double> figure; std::vector<char> meets; };
struct PatchPsnr { std::vector<PatchSums> patches; uint64_t background[3] = {0, 0, 0}; };
struct PatchD1 { std::vector<rbt_patch_d1> patches; rbt_d1_result whole = rbt_d1_result(); };
struct PatchD2 { std::vector<rbt_patch_d2> patches; rbt_d2_result whole = rbt_d2_result(); };
struct PatchColor { std::vector<rbt_patch_color> patches; rbt_color_result whole = rbt_color_result(); };
// the PSNR source: the words k_patch_fold left of the frame - sse, sse_occ, n_occ per patch, then the background's - with the displayed samples of every R_k
inline void patch_trial_psnr(const uint64_t* words, const std::vector<uint64_t>& samples, int region, int bit_depth, const std::vector<int32_t>& floor_mdb, PatchTrial& t, PatchPsnr& p) {
  const size_t np = samples.size();
  t.figure.resize(np); t.meets.resize(np); p.patches.assign(np, PatchSums());
  for (size_t k = 0; k < np; k++) {
    PatchSums& s = p.patches[k]; s.sse = words[3 * k]; s.sse_occ = words[3 * k + 1]; s.samples_occ = words[3 * k + 2]; s.samples = samples[k];
    t.figure[k] = patch_figure(s, region, bit_depth); t.meets[k] = patch_meets(s, region, floor_mdb[k], bit_depth);
  }
  for (int c = 0; c < 3; c++) p.background[c] = words[3 * np + c];
}
// the D1 source: the patches of the trial's cloud as rbt_score_patches left them (taken over, not copied) and the whole frame's result
inline void patch_trial_d1(std::vector<rbt_patch_d1>& patches, const rbt_d1_result& whole, const std::vector<int32_t>& floor_mdb, PatchTrial& t, PatchD1& p) {
  p.patches.swap(patches); p.whole = whole;
  const size_t np = p.patches.size();
  t.figure.resize(np); t.meets.resize(np);
  for (size_t k = 0; k < np; k++) { t.figure[k] = patch_d1_figure(p.patches[k]); t.meets[k] = patch_d1_meets(p.patches[k], floor_mdb[k]); }
}
// the D2 source: the same of rbt_score_patches_d2
inline void patch_trial_d2(std::vector<rbt_patch_d2>& patches, const rbt_d2_result& whole, const std::vector<int32_t>& floor_mdb, PatchTrial& t, PatchD2& p) {
  p.patches.swap(patches); p.whole = whole;
  const size_t np = p.patches.size();
  t.figure.resize(np); t.meets.resize(np);
  for (size_t k = 0; k < np; k++) { t.figure[k] = patch_d2_figure(p.patches[k]); t.meets[k] = patch_d2_meets(p.patches[k], floor_mdb[k]); }
}
// the colour source: the same of rbt_score_pair_patches_color, the figure on `channel` (0 Y, 1 U, 2 V)
inline void patch_trial_color(std::vector<rbt_patch_color>& patches, const rbt_color_result& whole, int channel, const std::vector<int32_t>& floor_mdb, PatchTrial& t, PatchColor& p) {
  p.patches.swap(patches); p.whole = whole;
  const size_t np = p.patches.size();
  t.figure.resize(np); t.meets.resize(np);
  for (size_t k = 0; k < np; k++) { t.figure[k] = patch_color_figure(p.patches[k], channel); t.meets[k] = patch_color_meets(p.patches[k], channel, floor_mdb[k]); }
}
}  // namespace rbt
