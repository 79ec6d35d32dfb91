// The float routine of the D1 and D2 results (rbt_d1, rbt_d2, rbt_score, rbt_score_patches, rbt_score_patches_d2) and what the walk of the D1 floors held patch by patch is told about a patch
// (include/rbt.h, "D1 per patch of the decoded cloud", "D1 floors held patch by patch"). Plain host code without a device call, so that tests/patch_d1_check.cpp can run
// it under the sanitizers; host/rbt_patch_walk.h includes this and makes a trial's figures of it (patch_trial_d1), its walk still takes figures and `meets` and nothing else.
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/rbt.h"

namespace rbt {
// mse in float from a double quotient, 10 log10f(3 peak^2 / mse): a direction without a point has mse 0, and 3 peak^2 / 0 = +inf gives
// the patch without a point psnr +inf. The figure of a patch is (double)psnr; meets is figure >= F_k / 1000.0, which +inf does.
inline float geometry_mse(double sse, int n) { return (float)(sse / n); }
inline float geometry_psnr(int peak, float mse) { const float p = (float)peak; return 10 * log10f(3 * p * p / mse); }
inline void patch_d1_finish(rbt_patch_d1* o, int peak) {
  o->mse_ab = o->n_ab ? geometry_mse((double)o->sse_ab, (int)o->n_ab) : 0.0f; o->mse_ba = o->n_ba ? geometry_mse((double)o->sse_ba, (int)o->n_ba) : 0.0f;
  o->psnr = geometry_psnr(peak, o->mse_ab > o->mse_ba ? o->mse_ab : o->mse_ba);
}
inline void patch_d2_finish(rbt_patch_d2* o, int peak) {
  o->mse_ab = o->n_ab ? geometry_mse(o->sse_ab, (int)o->n_ab) : 0.0f; o->mse_ba = o->n_ba ? geometry_mse(o->sse_ba, (int)o->n_ba) : 0.0f;
  o->psnr = geometry_psnr(peak, o->mse_ab > o->mse_ba ? o->mse_ab : o->mse_ba);
}
inline double patch_d1_figure(const rbt_patch_d1& d) { return (double)d.psnr; }
inline bool patch_d1_meets(const rbt_patch_d1& d, int32_t floor_mdb) { return patch_d1_figure(d) >= floor_mdb / 1000.0; }
inline double patch_d2_figure(const rbt_patch_d2& d) { return (double)d.psnr; }
inline bool patch_d2_meets(const rbt_patch_d2& d, int32_t floor_mdb) { return patch_d2_figure(d) >= floor_mdb / 1000.0; }
}  // namespace rbt
