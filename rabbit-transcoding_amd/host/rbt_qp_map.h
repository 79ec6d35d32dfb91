// A QP per CTB, host side (include/rbt.h "a QP per CTB"): the checks a map is refused by before anything is submitted, and the map of a frame from its patches. Plain host
// code without a device call, so that tests/qp_map_check.cpp can run it under the sanitizers.
#pragma once
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/rbt.h"

namespace rbt {
// rbt_qp_map_from_patches; err: the reason of a refusal
inline int qp_map_from_patches(std::string& err, const rbt_atlas_params* atlas, const rbt_patch* patches, int n_patches, const int8_t* patch_qp, int background_qp, int log2_ctb,
                               int8_t* out, int w_ctb, int h_ctb) {
  if (!atlas || !out || n_patches < 0 || (n_patches > 0 && (!patches || !patch_qp))) { err = "rbt_qp_map_from_patches: a null argument"; return RBT_ERR_PARAM; }
  if (log2_ctb < 4 || log2_ctb > 6) { err = "rbt_qp_map_from_patches: log2_ctb must be 4..6"; return RBT_ERR_PARAM; }
  if (atlas->width < 1 || atlas->height < 1 || atlas->occupancy_resolution < 1) { err = "rbt_qp_map_from_patches: the atlas needs a size and an occupancy_resolution"; return RBT_ERR_PARAM; }
  const int ctb = 1 << log2_ctb, wc = (atlas->width + ctb - 1) >> log2_ctb, hc = (atlas->height + ctb - 1) >> log2_ctb;
  if (w_ctb != wc || h_ctb != hc) { err = "rbt_qp_map_from_patches: w_ctb x h_ctb must be " + std::to_string(wc) + " x " + std::to_string(hc) + " for this atlas and log2_ctb"; return RBT_ERR_PARAM; }
  if (background_qp < 0 || background_qp > 51) { err = "rbt_qp_map_from_patches: background_qp is outside 0..51"; return RBT_ERR_PARAM; }
  for (int k = 0; k < n_patches; k++) if (patch_qp[k] < 0 || patch_qp[k] > 51) { err = "rbt_qp_map_from_patches: the QP of patch " + std::to_string(k) + " is outside 0..51"; return RBT_ERR_PARAM; }
  std::vector<int> best((size_t)wc * hc, 52);      // 52: no patch met the CTB yet
  for (int k = 0; k < n_patches; k++) {
    // the patch's rectangle in samples, clipped to the atlas: [x0, x1) x [y0, y1)
    const long long res = atlas->occupancy_resolution;
    const long long x0 = std::max(0ll, patches[k].u0 * res), y0 = std::max(0ll, patches[k].v0 * res);
    const long long x1 = std::min((long long)atlas->width, ((long long)patches[k].u0 + patches[k].size_u0) * res), y1 = std::min((long long)atlas->height, ((long long)patches[k].v0 + patches[k].size_v0) * res);
    if (x0 >= x1 || y0 >= y1) continue;
    for (int r = (int)(y0 >> log2_ctb); r <= (int)((y1 - 1) >> log2_ctb); r++) for (int c = (int)(x0 >> log2_ctb); c <= (int)((x1 - 1) >> log2_ctb); c++)
      best[(size_t)r * wc + c] = std::min(best[(size_t)r * wc + c], (int)patch_qp[k]);
  }
  for (size_t i = 0; i < best.size(); i++) out[i] = (int8_t)(best[i] > 51 ? background_qp : best[i]);
  return RBT_OK;
}
}  // namespace rbt
