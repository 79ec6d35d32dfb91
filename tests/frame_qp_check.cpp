// TEST-ONLY: the host half of floors held frame by frame (host/rbt_frame_walk.h: one walk per point-cloud frame, the passes of a round, the cut of a pass's stream into
// frames and the assembly of the returned stream) as a stand-alone host program, so that it can be built with -fsanitize=address,undefined and run on the CPU
// (tests/test_frame_qp.py). Synthetic figure tables per frame - monotone, with the inversions of the 64x64 geometry maps, noisy, and one that comes back exactly - over the
// lo / hi grids of tests/quality_check.cpp and every seventh qp. The rounds are driven the way run_rounds drives them: every pass is "encoded" into one stream of synthetic frames with
// the picture offsets encode_finish records, cut by frame_cut and handed to the walks. Held against the definition's loop per frame: q*, qs, met, the bound on the
// encodes, the rule of what pass j carries, no settled frame in a pass, no (frame, QP) encoded twice, and the assembled stream. Prints "ok".
#define RBT_HOSTEMU 1
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <cmath>
#include <set>
#include <vector>
#include "../rabbit-transcoding_amd/host/rbt_quality_walk.h"
#include "../rabbit-transcoding_amd/host/rbt_floor_walk.h"
#include "../rabbit-transcoding_amd/host/rbt_frame_walk.h"

static int fail(const char* what, long a = 0, long b = 0, long c = 0) { printf("FAIL %s %ld %ld %ld\n", what, a, b, c); fflush(stdout); return 1; }
static uint32_t g_seed = 97531;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

struct Walk : rbt::QpWalk<rbt::QualityTried> { rbt::FloorGoal floor; };
static rbt::QualitySums sums_of(double db) {
  rbt::QualitySums s; s.samples[0] = 1000000; s.sse[0] = (uint64_t)(1023.0 * 1023.0 * 1e6 / pow(10.0, db / 10.0));
  s.samples_occ[0] = 400000; s.sse_occ[0] = s.sse[0] / 3;
  return s;
}
// the NAL units of frame f at QP q: a length that depends on both, bytes that name both (a frame of `gop` pictures: the first of them carries the length's larger part)
static void synth_frame(int f, int q, size_t gop, std::vector<uint8_t>& stream, std::vector<size_t>& pic_at) {
  const size_t n = 7 + (size_t)((f * 13 + q * 5) % 23);
  for (size_t k = 0; k < gop; k++) { pic_at.push_back(stream.size()); for (size_t i = 0; i < (k ? 3 : n); i++) stream.push_back((uint8_t)(f * 64 + q + (int)k)); }
}

static int entry_case(const std::vector<std::vector<rbt::QualitySums>>& t, int qp, int32_t floor_mdb, int region, int lo, int hi) {
  const size_t F = t.size(), gop = 2;
  rbt::FrameWalks<Walk> fw; fw.n_enc.assign(F, 0);
  for (size_t f = 0; f < F; f++) { Walk w; w.lo = lo; w.hi = hi; w.floor.floor_mdb = floor_mdb; rbt::floor_seed(w, w.floor, qp); fw.frames.push_back(w); }
  auto step = [&](Walk& w, int& need, int& dir, bool& alone) {
    alone = !rbt::floor_probe(w, w.floor, [&](const rbt::QualityTried& x) { return rbt::quality_region_psnr(x.sums, region, 10); });
    if (alone) { need = w.floor.q0; dir = 0; return false; }
    return rbt::qp_walk_step(w, rbt::floor_holds(w, [&](const rbt::QualityTried& x) { return rbt::quality_meets(x.sums, region, floor_mdb, 10); }), need, dir);
  };
  std::vector<rbt::FramePass> passes; std::vector<std::set<int>> seen(F); long pictures = 0;
  for (int round = 0;; round++) {
    std::vector<char> was_settled(F); for (size_t f = 0; f < F; f++) was_settled[f] = fw.frames[f].settled;
    rbt::frame_round(fw, step, passes);
    if (passes.empty()) break;
    if (round > 60) return fail("rounds", floor_mdb, lo, hi);
    if (round == 0 && (passes.size() != 1 || passes[0].frames.size() != F)) return fail("the probe is one pass over all frames", (long)passes.size());
    // pass j carries the j-th QP of every frame that named more than j: so the frames of pass j + 1 are among those of pass j, and every pass is ascending in f
    for (size_t j = 0; j < passes.size(); j++) {
      const rbt::FramePass& p = passes[j];
      if (p.frames.empty() || p.frames.size() != p.qps.size()) return fail("empty pass", round, (long)j);
      for (size_t i = 0; i < p.frames.size(); i++) {
        const int f = p.frames[i], q = p.qps[i];
        if (i && f <= p.frames[i - 1]) return fail("pass not ascending", round, (long)j, f);
        if (was_settled[f]) return fail("a settled frame in a pass", round, f, q);
        if (q < lo || q > hi) return fail("pass out of range", q, lo, hi);
        if (round == 0 && q != fw.frames[f].floor.q0) return fail("probe QP", q);
        if (!seen[f].insert(q).second) return fail("encoded twice", f, q);
        if (j && !std::count(passes[j - 1].frames.begin(), passes[j - 1].frames.end(), f)) return fail("pass j + 1 holds a frame pass j does not", round, (long)j, f);
      }
    }
    // "encode" every pass: one stream, the picture offsets, then the cut
    for (const rbt::FramePass& p : passes) {
      std::vector<uint8_t> stream; std::vector<size_t> pic_at;
      for (size_t i = 0; i < p.frames.size(); i++) synth_frame(p.frames[i], p.qps[i], gop, stream, pic_at);
      for (size_t i = 0; i < p.frames.size(); i++) {
        rbt::QualityTried& tr = fw.frames[p.frames[i]].tried[p.qps[i]];
        rbt::frame_cut(stream, pic_at, i, gop, tr.stream); tr.sums = t[p.frames[i]][p.qps[i]];
        fw.n_enc[p.frames[i]]++; pictures += (long)gop;
      }
      fw.n_passes++;
    }
  }
  if (!fw.settled()) return fail("not settled", floor_mdb, lo, hi);
  // the definition, frame by frame
  const int q0 = qp < lo ? lo : qp > hi ? hi : qp; long enc = 0; std::vector<uint8_t> want;
  for (size_t f = 0; f < F; f++) {
    auto meets = [&](int q) { return rbt::quality_meets(t[f][q], region, floor_mdb, 10); };
    const double p0 = rbt::quality_region_psnr(t[f][q0], region, 10);
    int qs = std::isinf(p0) ? q0 : q0 + (int)(p0 - floor_mdb / 1000.0); qs = qs < lo ? lo : qs > hi ? hi : qs;
    int q = qs, met;
    if (meets(q)) { while (q < hi && meets(q + 1)) q++; met = 1; } else { while (q > lo && !meets(q)) q--; met = meets(q); }
    const Walk& w = fw.frames[f];
    if (w.start != qs || w.qstar != q || w.met != met) return fail("walk", (long)f, w.qstar, q);
    if (fw.n_enc[f] != (int)seen[f].size() || fw.n_enc[f] > abs(q - qs) + 5 || fw.n_enc[f] < 1) return fail("encodes", (long)f, fw.n_enc[f], abs(q - qs));
    enc += fw.n_enc[f];
    std::vector<size_t> at; synth_frame((int)f, q, gop, want, at);
  }
  if (pictures != 2 * enc) return fail("pictures", pictures, enc);
  std::vector<uint8_t> out; std::vector<uint64_t> bytes;
  rbt::frame_assemble(fw, out, bytes);
  uint64_t total = 0; for (uint64_t b : bytes) total += b;
  if (out != want || bytes.size() != F || total != out.size()) return fail("assembled stream", (long)out.size(), (long)want.size());
  return 0;
}

int main() {
  // pass formation on its own: ragged lists, an empty list in the middle, nothing at all
  { std::vector<rbt::FramePass> p;
    rbt::frame_passes({{30, 31, 32}, {}, {20}, {40, 41}}, p);
    if (p.size() != 3 || p[0].frames != std::vector<int>({0, 2, 3}) || p[0].qps != std::vector<int>({30, 20, 40}) || p[1].frames != std::vector<int>({0, 3}) || p[1].qps != std::vector<int>({31, 41}) ||
        p[2].frames != std::vector<int>({0}) || p[2].qps != std::vector<int>({32})) return fail("frame_passes");
    rbt::frame_passes({{}, {}}, p); if (!p.empty()) return fail("frame_passes: empty");
    rbt::frame_passes({}, p); if (!p.empty()) return fail("frame_passes: no frames"); }
  // the cut: the last frame of a pass ends with the stream
  { std::vector<uint8_t> s, c; std::vector<size_t> at; synth_frame(0, 30, 2, s, at); synth_frame(2, 18, 2, s, at);
    rbt::frame_cut(s, at, 1, 2, c); if (c.size() != s.size() - at[2] || c[0] != (uint8_t)(2 * 64 + 18)) return fail("frame_cut");
    rbt::frame_cut(s, at, 0, 2, c); if (c.size() != at[2] || c.back() != (uint8_t)(30 + 1)) return fail("frame_cut 0"); }
  // tables: frame f is the table shifted by a frame's worth of dB, so the frames settle at different QPs
  std::vector<double> mono(52), inv(52), noisy(52);
  for (int q = 0; q < 52; q++) { mono[q] = 62.0 - 0.7 * q; inv[q] = 66.0 - 0.72 * q; noisy[q] = 60.0 - 0.6 * q + (rnd() % 1200) / 1000.0; }
  inv[34] = 41.737; inv[35] = 41.116; inv[36] = 41.186; inv[37] = 39.719; inv[40] = 37.0; inv[41] = 37.3; inv[44] = 34.8; inv[45] = 35.1;
  const double shift[4] = {0.0, 4.3, -1.9, 2.2};
  for (const std::vector<double>* tb : {&mono, &inv, &noisy}) for (size_t F : {(size_t)1, (size_t)4}) {
    std::vector<std::vector<rbt::QualitySums>> t(F);
    for (size_t f = 0; f < F; f++) for (int q = 0; q < 52; q++) t[f].push_back(sums_of((*tb)[q] + shift[f] + (tb == &noisy ? (rnd() % 900) / 1000.0 : 0.0)));
    for (int region = 0; region < 2; region++) for (int lo = 0; lo < 52; lo += 5) for (int hi = lo; hi < 52; hi += 6) for (int qp = (lo + hi) % 4; qp < 52; qp += 7) {
      for (int q = lo; q <= hi; q += 3) for (int d = -350; d <= 350; d += 700) if (entry_case(t, qp, (int32_t)((*tb)[q] * 1000) + d + (region ? 4771 : 0), region, lo, hi)) return 1;
      if (entry_case(t, qp, 1, region, lo, hi) || entry_case(t, qp, 120000, region, lo, hi)) return 1;
    }
  }
  // one frame comes back exactly below QP 12 (+inf: its walk starts at q0), the others do not
  { std::vector<std::vector<rbt::QualitySums>> t(3);
    for (size_t f = 0; f < 3; f++) for (int q = 0; q < 52; q++) { t[f].push_back(sums_of(50.0 - q + shift[f])); if (f == 1 && q < 12) t[f][q].sse[0] = 0; }
    if (entry_case(t, 5, 45000, 0, 0, 51) || entry_case(t, 11, 30000, 0, 0, 51) || entry_case(t, 0, 99000, 0, 0, 11)) return 1; }
  // no floor: a range that is the entry's own QP alone - one pass, every frame at it
  { std::vector<std::vector<rbt::QualitySums>> t(3); for (size_t f = 0; f < 3; f++) for (int q = 0; q < 52; q++) t[f].push_back(sums_of(mono[q] + shift[f]));
    if (entry_case(t, 30, 0, 0, 30, 30)) return 1; }
  printf("ok\n");
  return 0;
}
