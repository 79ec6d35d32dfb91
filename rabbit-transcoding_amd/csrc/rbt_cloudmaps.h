// Luma planes of pictures in device memory as the packed planes the reconstruction kernels read (rbt_submit_gof_d1, rbt_gather_luma; include/rbt.h, "transcoding to a D1
// floor"). A decoded input and an encoder's reconstruction are coded pictures: rows `stride` samples apart, the displayed w x h window somewhere inside. k_pcc_count and
// k_pcc_emit (rbt_pcc.h) index a plane as [y * w + x]; they stay as they are, and this kernel makes them the planes they expect - a device-to-device copy of one luma plane per
// picture, many pictures per launch, one descriptor each. Nothing of a trial's maps visits the host.
//   chunks   a row of w samples is cut into w / 8 + 2 chunks, as csrc/rbt_quality.h cuts it: where the source row and the destination row are equally far from a 16-byte
//            boundary, chunk 0 is the head in front of that boundary (0..7 samples), the chunks behind it hold 8 samples each - one 16-byte load and one 16-byte store -
//            and the last one the tail; where they are not, chunk 0 is empty and every chunk goes sample by sample, like heads and tails.
//   lanes    one lane per chunk, consecutive lanes on consecutive chunks of a row: a wave moves 1 KB of a row with one load and one store instruction.
//   4:2:0    a descriptor is one plane with a width, a height and a stride of its own, so the chroma planes of an attribute picture go through the same kernel: three
//            descriptors a picture, into the packed planar layout launch_up444 reads (rbt_submit_gof_color, rbt_gather_420); a row of 1, 7 or 36 samples is cut like any other.
// No kernel waits for another, a lane has no loop but the at most 8 samples of its chunk, and a chunk index past the picture's last row does nothing.
#pragma once
#include "rbt_platform.h"

enum { RBT_GM_WG = 256 };
// one picture: src = the first displayed luma sample (the plane's origin plus the window's offset), rows `stride` samples apart; dst = w * h samples, packed
struct RbtGatherPic { const uint16_t* src; uint16_t* dst; int32_t w, h, stride, pad; };
#define RBT_GM_ROW_CHUNKS(w) ((w) / 8 + 2)
#define RBT_GM_PIC_CHUNKS(w, h) ((h) * RBT_GM_ROW_CHUNKS(w))

namespace rbtk {
// max_chunks = RBT_GM_PIC_CHUNKS of the largest picture
void launch_gather_luma(const RbtGatherPic* pics, int n_pics, int max_chunks);
}  // namespace rbtk

// ------------------------------------------------------------------------------------------------ body (device and host emulation)
struct alignas(16) RbtGmQuad { uint32_t x, y, z, w; };      // eight samples, one 16-byte access
// chunk i of the picture (rows of RBT_GM_ROW_CHUNKS chunks, back to back)
RBT_DEV void gm_chunk(const RbtGatherPic* P, int i) {
  const int per = RBT_GM_ROW_CHUNKS(P->w), y = i / per, j = i - y * per;
  if (y >= P->h) return;
  const uint16_t* rs = P->src + (size_t)y * (size_t)P->stride;
  uint16_t* rd = P->dst + (size_t)y * (size_t)P->w;
  const int ms = (int)(((uintptr_t)rs >> 1) & 7), md = (int)(((uintptr_t)rd >> 1) & 7);
  const int head = ms == md ? rbt_min(P->w, (8 - ms) & 7) : 0;
  const int x0 = j == 0 ? 0 : head + 8 * (j - 1), x1 = j == 0 ? head : rbt_min(P->w, x0 + 8);
  if (x0 >= x1) return;
  if (ms == md && x1 - x0 == 8 && j > 0) *(RbtGmQuad*)(rd + x0) = *(const RbtGmQuad*)(rs + x0);      // both addresses are multiples of 16
  else for (int k = x0; k < x1; k++) rd[k] = rs[k];
}

#ifdef RBT_HOSTEMU
// serial stand-in of the launcher (the product's is in rbt_cloudmaps.hip)
namespace rbtk {
inline void launch_gather_luma(const RbtGatherPic* pics, int n_pics, int max_chunks) {
  for (int k = 0; k < n_pics; k++) for (int i = 0; i < max_chunks; i++) gm_chunk(&pics[k], i);
}
}  // namespace rbtk
#endif
