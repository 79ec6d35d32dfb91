// Floors held frame by frame (include/rbt.h, "floors held frame by frame"): one QP walk (rbt_qp_walk.h) per point-cloud frame of an entry, the passes a round of such
// walks is encoded in, and the assembly of the returned stream from the frames the passes brought. A frame of a geometry / attribute stream is a closed pair of pictures
// (an I picture and a P picture that refers to it), so a pass may carry any subset of the frames at any QPs and frame f at QP q comes out the same whatever else the pass
// holds. Plain host code without a device call, so that tests/frame_qp_check.cpp can run it under the sanitizers. The walk does not know what a figure is: the caller hands
// in the step of its floor - walk_step of rbt_transcode.cpp, which binds the figure of the walk's kind: a PSNR floor's or a D1 floor's; a byte cap or a colour floor per frame
// would be one more kind there.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "rbt_qp_walk.h"

namespace rbt {
// One pass: an encode launch sequence over (frame, QP) pairs of one entry, frames ascending. Frames that are not listed are not encoded.
struct FramePass { std::vector<int> frames, qps; };
// Rule 5: named[f] holds the QPs frame f asks for in this round, in the order qp_round names them (empty: the frame has settled). Pass j carries, for every frame that
// named at least j + 1 QPs, the j-th of them.
inline void frame_passes(const std::vector<std::vector<int>>& named, std::vector<FramePass>& passes) {
  passes.clear();
  for (size_t j = 0;; j++) {
    FramePass p;
    for (size_t f = 0; f < named.size(); f++) if (named[f].size() > j) { p.frames.push_back((int)f); p.qps.push_back(named[f][j]); }
    if (p.frames.empty()) return;
    passes.push_back(std::move(p));
  }
}
// The walks of one entry: Walk is a QpWalk<Trial> (or derives from one) whose Trial has a member `stream`, the NAL units of the frame at that QP
template <class Walk> struct FrameWalks {
  int q = 0, entry = 0, n_passes = 0;          // position in the pipeline's group, index of the entry in the call, passes that carried frames of the entry
  std::vector<Walk> frames; std::vector<int> n_enc;   // per frame: its walk and the trial encodes run for it
  bool settled() const { for (const Walk& w : frames) if (!w.settled) return false; return true; }
};
// The next round of an entry: every unsettled frame takes its step - step(walk, need, dir, alone) is walk_step of the floor's kind: true = settled - and names its QPs
// through qp_round; the passes are formed of them. No pass: every frame has settled.
template <class Walk, class Step> inline void frame_round(FrameWalks<Walk>& fw, Step step, std::vector<FramePass>& passes) {
  std::vector<std::vector<int>> named(fw.frames.size());
  for (size_t f = 0; f < fw.frames.size(); f++) {
    Walk& w = fw.frames[f]; int need = 0, dir = 0; bool alone = false;
    if (!w.settled && !step(w, need, dir, alone)) qp_round(w, need, dir, alone, named[f]);
  }
  frame_passes(named, passes);
}
// The bytes of the i-th frame of a pass in the pass's stream: pic_at[k] is where the NAL units of coded picture k start (parameter sets in front of an I picture
// included, the hash SEI behind a picture included), a frame is `gop` pictures
inline void frame_cut(const std::vector<uint8_t>& stream, const std::vector<size_t>& pic_at, size_t i, size_t gop, std::vector<uint8_t>& out) {
  const size_t a = pic_at[i * gop], b = (i + 1) * gop < pic_at.size() ? pic_at[(i + 1) * gop] : stream.size();
  out.assign(stream.begin() + (ptrdiff_t)a, stream.begin() + (ptrdiff_t)b);
}
// Rule 6: the returned stream is the frames at their q*, in frame order; bytes[f] = the size of frame f in it. Every pass writes the parameter sets of the entry's own
// QP, so the pieces fit together as rbt_transcode_gof_frame_qp writes them in one go.
template <class Walk> inline void frame_assemble(const FrameWalks<Walk>& fw, std::vector<uint8_t>& out, std::vector<uint64_t>& bytes) {
  out.clear(); bytes.clear();
  for (const Walk& w : fw.frames) { const std::vector<uint8_t>& s = w.tried.find(w.qstar)->second.stream; out.insert(out.end(), s.begin(), s.end()); bytes.push_back((uint64_t)s.size()); }
}
}  // namespace rbt
