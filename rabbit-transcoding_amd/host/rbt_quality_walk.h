// Host half of a transcode to a PSNR floor (include/rbt.h, "transcoding to a PSNR floor"): PSNR and the floor's condition on the integer sums of csrc/rbt_quality.h - the
// figure and the condition that make the floor's walk (rbt_floor_walk.h) the walk of a PSNR floor. Plain host code without a device call, so that tests/quality_check.cpp can run it under the sanitizers next to the kernel body.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include "../csrc/rbt_quality.h"

namespace rbt {
// the sums of one stream: every picture's nine words added up, and the samples they were taken over
struct QualitySums { uint64_t sse[3] = {0, 0, 0}, samples[3] = {0, 0, 0}, sse_occ[3] = {0, 0, 0}, samples_occ[3] = {0, 0, 0}; };
inline void quality_add_picture(QualitySums& s, const uint64_t* words, int w, int h) {
  for (int c = 0; c < 3; c++) { s.sse[c] += words[3 * c]; s.sse_occ[c] += words[3 * c + 1]; s.samples_occ[c] += words[3 * c + 2]; s.samples[c] += c ? (uint64_t)(w / 2) * (uint64_t)(h / 2) : (uint64_t)w * (uint64_t)h; }
}
inline double quality_psnr(uint64_t sse, uint64_t samples, int bit_depth) {
  if (!samples) return 0.0;
  if (!sse) return std::numeric_limits<double>::infinity();
  const double peak = (double)((1u << bit_depth) - 1);
  return 10.0 * log10((double)peak * peak * (double)samples / (double)sse);
}
// region: 0 = all samples, 1 = the occupied ones (RBT_QUALITY_*); plane 0 decides
inline double quality_region_psnr(const QualitySums& s, int region, int bit_depth) { return region ? quality_psnr(s.sse_occ[0], s.samples_occ[0], bit_depth) : quality_psnr(s.sse[0], s.samples[0], bit_depth); }
inline bool quality_meets(const QualitySums& s, int region, int32_t min_psnr_mdb, int bit_depth) {
  const uint64_t sse = region ? s.sse_occ[0] : s.sse[0], n = region ? s.samples_occ[0] : s.samples[0];
  if (!n || !sse) return true;
  return quality_psnr(sse, n, bit_depth) >= min_psnr_mdb / 1000.0;
}

// what a trial of a PSNR floor keeps (the floor itself: rbt_floor_walk.h, with quality_region_psnr as the figure and quality_meets as the condition)
struct QualityTried { std::vector<uint8_t> stream; QualitySums sums; };
}  // namespace rbt
