// Frame scoring on clouds that stay on the device (rbt_pcloud_*, rbt_score; the definitions are in include/rbt.h): D1, D2 and the colour PSNR from ONE index per cloud
// and ONE nearest-distance search per direction. The host-array calls rbt_d1, rbt_d2 and rbt_color_metric are this path on two temporary clouds (host/rbt_pcc.cpp).
//   index    built once per cloud: the 1024^3-bit volume (csrc/rbt_pcc.h), a coarse level over it (one bit per 8 x 8 x 8 block, 256 KB), one hash map voxel -> slot whose
//            slot holds the lowest point index of the voxel (the representative of the merged point, as in D2) and the colour sums and count (as in the colour metric).
//            Only the first point of a voxel touches the volume and the coarse level. Coordinates are checked by a kernel of their own first (error word), so a
//            refused cloud has touched no volume word.
//   search   one lane per point, in point order (neighbouring lanes are neighbouring points of a patch); lanes of representatives search, the others store
//            RBT_SC_NONE. The volume is read by 32-bit words: first the 5 x 5 rows around the query, masked to x - 2 .. x + 2 (25 to 50 independent loads; a surface
//            within 3 voxels ends here), then shells of coarse blocks of growing Chebyshev radius, where only occupied blocks that can still hold a nearer point have their
//            8 x 8 rows read. The shell loop ends when the shell's nearest possible voxel is no nearer than the best found, at radius 127 at the latest.
//   walks    everything else is pc_for_ties at the stored distance: A -> B gives normals to B (integer atomics) and accumulates the D1 term and the colour error; B -> A
//            accumulates the same, the D2 value against A's own normals, and is the "take" step for points of B that got no normal; a third walk over A's ties computes
//            the D2 value A -> B from B's completed normals. Integer sums: workgroup reduction, then one 64-bit atomic per workgroup.
//   D2 sums  the per-point values are stored (0 for a point that is no representative) and summed in a fixed order (include/rbt.h): no floating-point atomics, the
//            same bits from every call and from the serial host emulation. This file is compiled with -ffp-contract=off like the rest of rbt_color.hip.
//   recolour new colours for an indexed cloud (rbt_pcloud_set_colors): positions, volume, keys and lowest indices stay; the occupied slots' sums, counts and merged colours
//            go back to zero, every point adds its triple through the voxel -> slot lookup, and the slots are merged again (sc_merge). Integer sums: the result is that of
//            a fresh index of the same points with the new colours.
//   pairs    the nearest squared distances of both directions depend on positions only. A score pair (rbt_score_pair_*) keeps them; launch_sc_color_walks runs the walks
//            with the colour part alone on the stored distances - three sums per direction, reduced in the workgroup, one 64-bit atomic per workgroup and sum.
//   patches  D1 per patch of the decoded cloud (rbt_score_patches; the definition is in include/rbt.h): B carries a label per point. Behind the two searches one lane per
//            point reads its stored distance; B -> A adds (label of j, d_j), A -> B walks pc_for_ties on B's volume at d_i, takes the lowest pc_hash_find over the tie
//            voxels - the owner - and adds (label of the owner, d_i). RBT_PD_WORDS 64-bit words per patch, integer atomics only: a wave whose labels are all the same
//            (points arrive in patch order) folds sum, count and maximum in registers and issues one atomic per word, a mixed wave one per lane and word. The labels
//            are checked against the patch count by a kernel of their own first (error word), so a refused call has written no sum. The labels of a cloud made from maps
//            come from a kernel of their own over the work items' offsets (pd_label_item): the reconstruction kernels are the ones they were.
//   D2/patch D2 per patch of the decoded cloud (rbt_score_patches_d2; the definition is in include/rbt.h): behind launch_sc_score with the D2 part, on the values val_ab / val_ba
//            it leaves. The attribution is that of D1 per patch (pd_term_ab / pd_term_ba); the sums keep rbt_score's fixed order with the values of other patches read as 0.
//            p2_block: a workgroup takes 256 entries, and for every distinct label among them - in the order of the lowest lane that carries it - folds the masked tree
//            in LDS and appends (label, sum) to the block's own range of 256 entries; the patch's count and maximum go out as integer atomics (a value >= 0 orders as
//            its bit pattern does). p2_cols: 256 lanes, lane t walks blocks t, t + 256, .. in ascending order and adds every entry into S[label][t] - it owns its
//            column, no atomics. p2_fold: one workgroup per patch folds S[k][0..255] and leaves the row zero for the other direction. No floating-point atomics.
//            Scratch: 12 bytes per entry of the larger cloud rounded up to 256, 4 per 256 entries, 2 KB (S) + 8 RBT_P2_WORDS bytes per patch: O(points + patches).
//   col/patch the colour sums per patch of the decoded cloud (rbt_score_patches_color, rbt_score_pair_patches_color; the definition is in include/rbt.h): behind the two searches,
//            or on the distances a score pair keeps, in place of the colour walks. One lane per point of the walking cloud. pc_term walks the tie set once: A -> B the walk
//            that sums the tie colours also takes the lowest point index among the tie voxels - the owner, pd_term_ab's rule - so the label costs one comparison per tie
//            voxel; B -> A the label is the point's own. RBT_PC_WORDS 64-bit words per patch - three sums of squared error terms and a count per direction -, integer
//            atomics only, added as k_pd_sums adds: a wave whose terms all carry one label folds them with shuffles and lane 0 issues one atomic per non-zero word, a
//            mixed wave one per lane and non-zero word. The whole frame's sums are the sums over the patches, exact: the host adds them, no second kernel runs.
// No kernel waits for another; every loop is bounded by the size of the volume.
#pragma once
#include "rbt_color.h"

enum { RBT_SC_BLOCK_BITS = 3, RBT_SC_CDIM = RBT_PCC_DIM >> RBT_SC_BLOCK_BITS, RBT_SC_CROW = RBT_SC_CDIM / 32, RBT_SC_COARSE_WORDS = RBT_SC_CDIM * RBT_SC_CDIM * RBT_SC_CROW,
       RBT_SC_FINE_R = 2, RBT_SC_SUM = 256 };
#define RBT_SC_NONE 0xFFFFFFFFu
enum { RBT_SC_ERR = 0, RBT_SC_N_MERGED = 1, RBT_SC_SCALARS = 16 };        // words of a cloud's scalars (zeroed beforehand)
// words of the result block of one rbt_score call (zeroed beforehand), 64-bit each; the two D1 maxima are the 32-bit halves of one word
enum { RBT_SC_D1_AB = 0, RBT_SC_D1_BA, RBT_SC_COL_AB, RBT_SC_COL_BA = RBT_SC_COL_AB + 3, RBT_SC_D1_MAX = RBT_SC_COL_BA + 3, RBT_SC_D2_AB, RBT_SC_D2_BA = RBT_SC_D2_AB + 2, RBT_SC_RESULTS = 16 };

// a cloud with its index. keys: voxel id + 1 (0 = empty); vals: lowest point index of the voxel (starts at 0xFFFFFFFF); acc: R, G, B sums and the count per slot (zeroed);
// col: the merged colour per slot. rgb / nrm may be null.
struct RbtScoreCloud { const int16_t* xyz; const uint8_t* rgb; const int16_t* nrm; int32_t n, lg; uint32_t* vol; uint32_t* coarse; uint32_t* keys; uint32_t* vals; uint32_t* acc; uint32_t* col; };
// scratch of one rbt_score call. dist_*: nearest squared distance per point; acc_b / cnt_b: the normals given to B (zeroed beforehand; not part of B's index: B may be
// scored against another source next); val_*: D2 value per point; part: 2 * ceil(max(n) / 256) doubles; res: RBT_SC_RESULTS words (zeroed beforehand)
struct RbtScoreWork { uint32_t* dist_a; uint32_t* dist_b; long long* acc_b; int32_t* cnt_b; double* val_ab; double* val_ba; double* part; unsigned long long* res; };
struct RbtScoreSumLds { double s[RBT_SC_SUM]; double m[RBT_SC_SUM]; };
// scratch of one rbt_score_patches_d2 call beside RbtScoreWork. ent_label / ent_sum: 256 entries per block of 256 points of the larger cloud, ent_n: the entries a block
// wrote; S: n_patches rows of RBT_SC_SUM doubles (zeroed beforehand; zero again when the call has run)
struct RbtPatchD2Work { uint32_t* ent_label; double* ent_sum; uint32_t* ent_n; double* S; };

namespace rbtk {
void launch_sc_check(const int16_t* xyz, int n, uint32_t* scal);        // scal[RBT_SC_ERR] = 1 when a coordinate lies outside 0..1023
void launch_sc_index(const RbtScoreCloud* S, uint32_t* scal);           // insert + merge; scal[RBT_SC_N_MERGED] counts the voxels
void launch_sc_clear(const RbtScoreCloud* S);                           // the volume and coarse words of the cloud's own points back to zero
// parts: RBT_SCORE_* (D1 always runs: its sums come with the walks)
void launch_sc_score(const RbtScoreCloud* A, const RbtScoreCloud* B, int parts, const RbtScoreWork* W);
void launch_sc_recolor(const RbtScoreCloud* S);                         // S->rgb holds the new triples: sums, counts and merged colours of the index remade
void launch_sc_search(const RbtScoreCloud* A, const RbtScoreCloud* B, uint32_t* dist_a, uint32_t* dist_b);   // the two searches of launch_sc_score on their own
// the colour sums of launch_sc_score from stored distances: res[0..2] A -> B, res[3..5] B -> A (RBT_SC_COLOR_RESULTS words, zeroed beforehand)
void launch_sc_color_walks(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* dist_a, const uint32_t* dist_b, unsigned long long* res);
// the label of every point of a cloud made from maps: the points of work item t (items[t] = patch << 16 | block) are offsets[t] .. offsets[t + 1] - 1
void launch_pd_labels(const uint32_t* items, const uint32_t* offsets, int n_items, uint32_t* labels);
void launch_pd_check(const uint32_t* labels, int n, uint32_t n_patches, uint32_t* err);       // *err = 1 when a label is >= n_patches
// behind launch_sc_score / launch_sc_search on the same clouds: out holds RBT_PD_WORDS words per patch (zeroed beforehand); every label of B is below the patch count
void launch_pd_sums(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* labels_b, const uint32_t* dist_a, const uint32_t* dist_b, unsigned long long* out);
// behind launch_sc_score with RBT_SCORE_D2 on the same clouds and the same W (dist_*, val_*): out holds RBT_P2_WORDS words per patch (zeroed beforehand); every label of B
// is below n_patches
void launch_p2_sums(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* labels_b, const RbtScoreWork* W, const RbtPatchD2Work* P, int n_patches, unsigned long long* out);
// behind launch_sc_search on the same clouds, or on the distances of a score pair, in place of launch_sc_color_walks: out holds RBT_PC_WORDS words per patch (zeroed
// beforehand); both clouds carry colours, every label of B is below the patch count
void launch_pc_sums(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* labels_b, const uint32_t* dist_a, const uint32_t* dist_b, unsigned long long* out);
}  // namespace rbtk
enum { RBT_SC_COLOR_RESULTS = 8 };
// words of one patch in the result of launch_pd_sums, 64-bit each; + 1 for the direction B -> A
enum { RBT_PD_SSE_AB = 0, RBT_PD_SSE_BA, RBT_PD_N_AB, RBT_PD_N_BA, RBT_PD_MAX_AB, RBT_PD_MAX_BA, RBT_PD_WORDS };
// words of one patch in the result of launch_pc_sums, 64-bit each: the sums of e[c]^2 at RBT_PC_SSE_AB + c / RBT_PC_SSE_BA + c (c = 0, 1, 2: Y, U, V), then the counts
enum { RBT_PC_SSE_AB = 0, RBT_PC_SSE_BA = 3, RBT_PC_N_AB = 6, RBT_PC_N_BA = 7, RBT_PC_WORDS = 8 };
// words of one patch in the result of launch_p2_sums, 64-bit each; + 1 for the direction B -> A. SSE and MAX hold doubles, N counts
enum { RBT_P2_SSE_AB = 0, RBT_P2_SSE_BA, RBT_P2_N_AB, RBT_P2_N_BA, RBT_P2_MAX_AB, RBT_P2_MAX_BA, RBT_P2_WORDS };
// LDS of p2_block: the fold's arrays, then per lane its label (RBT_SC_NONE: no term), its value, and - for the lowest lane of a label - the label's count of lanes (else 0)
struct RbtPatchD2Lds { RbtScoreSumLds f; double v[RBT_SC_SUM]; uint32_t lab[RBT_SC_SUM]; uint32_t lead[RBT_SC_SUM]; };

// ------------------------------------------------------------------------------------------------ bodies (device and host emulation)
RBT_DEV size_t sc_coarse_word(int cx, int cy, int cz) { return (((size_t)cz * RBT_SC_CDIM + cy) * RBT_SC_CROW) + (cx >> 5); }
// point i into the index; returns 1 for the first point of a voxel. A point out of range is never indexed (launch_sc_check has reported it).
RBT_DEV int sc_insert(const RbtScoreCloud* S, int i) {
  const int16_t* p = S->xyz + 3 * (size_t)i;
  if (!tc_in_range(p)) return 0;
  const int x = p[0], y = p[1], z = p[2];
  int fresh; const uint32_t s = cl_slot_claim(S->keys, S->lg, pc_voxel_id(x, y, z), &fresh);
  uint32_t* vw = &S->vol[pc_voxel_word(x, y, z)]; uint32_t* cw = &S->coarse[sc_coarse_word(x >> RBT_SC_BLOCK_BITS, y >> RBT_SC_BLOCK_BITS, z >> RBT_SC_BLOCK_BITS)];
  const uint32_t vbit = 1u << (x & 31), cbit = 1u << ((x >> RBT_SC_BLOCK_BITS) & 31);
#ifdef RBT_HOSTEMU
  if (fresh) { *vw |= vbit; *cw |= cbit; }
  if ((uint32_t)i < S->vals[s]) S->vals[s] = (uint32_t)i;
  if (S->rgb) { for (int c = 0; c < 3; c++) S->acc[4 * s + c] += S->rgb[3 * (size_t)i + c]; S->acc[4 * s + 3]++; }
#else
  if (fresh) { atomicOr(vw, vbit); atomicOr(cw, cbit); }
  atomicMin(&S->vals[s], (uint32_t)i);
  if (S->rgb) { for (int c = 0; c < 3; c++) atomicAdd(&S->acc[4 * s + c], (uint32_t)S->rgb[3 * (size_t)i + c]); atomicAdd(&S->acc[4 * s + 3], 1u); }
#endif
  return fresh;
}
RBT_DEV void sc_merge(const RbtScoreCloud* S, uint32_t s) {             // removeDuplicate (PCCPointSet.cpp:190-203): the colour of a voxel is sum / count per channel, in integer division
  if (!S->keys[s]) return;
  const uint32_t n = S->acc[4 * s + 3];
  S->col[s] = (S->acc[4 * s] / n) | (S->acc[4 * s + 1] / n) << 8 | (S->acc[4 * s + 2] / n) << 16;
}
// recolouring, per slot: an occupied slot's sums, count and merged colour back to zero
RBT_DEV void sc_recolor_zero(const RbtScoreCloud* S, uint32_t s) {
  if (!S->keys[s]) return;
  for (int c = 0; c < 4; c++) S->acc[4 * s + c] = 0;
  S->col[s] = 0;
}
// recolouring, per point: the point's new triple into its voxel's slot (the voxel is in the map: the cloud is indexed)
RBT_DEV void sc_recolor_add(const RbtScoreCloud* S, int i) {
  const int16_t* p = S->xyz + 3 * (size_t)i;
  if (!tc_in_range(p)) return;
  const uint32_t s = cl_slot_find(S->keys, S->lg, pc_voxel_id(p[0], p[1], p[2]));
#ifdef RBT_HOSTEMU
  for (int c = 0; c < 3; c++) S->acc[4 * s + c] += S->rgb[3 * (size_t)i + c];
  S->acc[4 * s + 3]++;
#else
  for (int c = 0; c < 3; c++) atomicAdd(&S->acc[4 * s + c], (uint32_t)S->rgb[3 * (size_t)i + c]);
  atomicAdd(&S->acc[4 * s + 3], 1u);
#endif
}
RBT_DEV void sc_clear(const RbtScoreCloud* S, int i) {
  const int16_t* p = S->xyz + 3 * (size_t)i;
  if (!tc_in_range(p)) return;
  S->vol[pc_voxel_word(p[0], p[1], p[2])] = 0;
  S->coarse[sc_coarse_word(p[0] >> RBT_SC_BLOCK_BITS, p[1] >> RBT_SC_BLOCK_BITS, p[2] >> RBT_SC_BLOCK_BITS)] = 0;
}

// the set bits of `bits` (bit k = voxel x0 + k of a row at squared distance `base` in y and z) against the query's x
RBT_DEV uint32_t sc_row_best(uint32_t bits, int x0, int x, uint32_t base, uint32_t best) {
  while (bits) { const int dx = x0 + __builtin_ctz(bits) - x; bits &= bits - 1; const uint32_t d = base + (uint32_t)(dx * dx); if (d < best) best = d; }
  return best;
}
RBT_DEV uint32_t sc_mask(int lo, int hi) { return (0xFFFFFFFFu << (lo & 31)) & (0xFFFFFFFFu >> (31 - (hi & 31))); }     // bits lo .. hi of one word
RBT_DEV int sc_gap(int q, int c) { const int lo = c << RBT_SC_BLOCK_BITS, hi = lo + (1 << RBT_SC_BLOCK_BITS) - 1; return q < lo ? lo - q : (q > hi ? q - hi : 0); }   // from coordinate q to block c along one axis
// squared distance from (x, y, z) to the nearest point of Q (Q is not empty)
RBT_DEV uint32_t sc_nearest(const RbtScoreCloud* Q, int x, int y, int z) {
  const uint32_t* vol = Q->vol;
  uint32_t best = 0xFFFFFFFFu;
  const int lo = x - RBT_SC_FINE_R < 0 ? 0 : x - RBT_SC_FINE_R, hi = x + RBT_SC_FINE_R >= RBT_PCC_DIM ? RBT_PCC_DIM - 1 : x + RBT_SC_FINE_R;
  const int w0 = lo >> 5, w1 = hi >> 5;
  for (int dz = -RBT_SC_FINE_R; dz <= RBT_SC_FINE_R; dz++) {
    const int zz = z + dz; if (zz < 0 || zz >= RBT_PCC_DIM) continue;
    for (int dy = -RBT_SC_FINE_R; dy <= RBT_SC_FINE_R; dy++) {
      const int yy = y + dy; if (yy < 0 || yy >= RBT_PCC_DIM) continue;
      const uint32_t* row = vol + pc_voxel_word(0, yy, zz); const uint32_t base = (uint32_t)(dz * dz + dy * dy);
      if (w0 == w1) best = sc_row_best(row[w0] & sc_mask(lo, hi), w0 * 32, x, base, best);
      else { best = sc_row_best(row[w0] & sc_mask(lo, 31), w0 * 32, x, base, best); best = sc_row_best(row[w1] & sc_mask(0, hi), w1 * 32, x, base, best); }
    }
  }
  // everything outside the cube is at least RBT_SC_FINE_R + 1 away
  if (best <= (uint32_t)((RBT_SC_FINE_R + 1) * (RBT_SC_FINE_R + 1))) return best;
  const int bx = x >> RBT_SC_BLOCK_BITS, by = y >> RBT_SC_BLOCK_BITS, bz = z >> RBT_SC_BLOCK_BITS;
  auto block = [&](int cx, int cy, int cz) {                          // an occupied block: its 8 x 8 rows, one byte of a volume word each
    const int gx = sc_gap(x, cx), gy = sc_gap(y, cy), gz = sc_gap(z, cz);
    if ((uint32_t)(gx * gx + gy * gy + gz * gz) >= best) return;
    const int x0 = cx << RBT_SC_BLOCK_BITS;
    for (int zz = cz << RBT_SC_BLOCK_BITS; zz < (cz + 1) << RBT_SC_BLOCK_BITS; zz++)
      for (int yy = cy << RBT_SC_BLOCK_BITS; yy < (cy + 1) << RBT_SC_BLOCK_BITS; yy++) {
        const uint32_t base = (uint32_t)((zz - z) * (zz - z) + (yy - y) * (yy - y));
        if (base >= best) continue;
        best = sc_row_best((vol[pc_voxel_word(x0, yy, zz)] >> (x0 & 31)) & 0xFFu, x0, x, base, best);
      }
  };
  for (int r = 0; r < RBT_SC_CDIM; r++) {
    // a block of shell r lies at least 8 (r - 1) + 1 away along the axis on which it is r blocks off
    if (r > 0) { const uint32_t lb = (uint32_t)(((r - 1) << RBT_SC_BLOCK_BITS) + 1); if (lb * lb >= best) break; }
    const int clo = bx - r < 0 ? 0 : bx - r, chi = bx + r >= RBT_SC_CDIM ? RBT_SC_CDIM - 1 : bx + r;
    for (int dz = -r; dz <= r; dz++) {
      const int cz = bz + dz; if (cz < 0 || cz >= RBT_SC_CDIM) continue;
      for (int dy = -r; dy <= r; dy++) {
        const int cy = by + dy; if (cy < 0 || cy >= RBT_SC_CDIM) continue;
        const int gy = sc_gap(y, cy), gz = sc_gap(z, cz);
        if ((uint32_t)(gy * gy + gz * gz) >= best) continue;
        const uint32_t* crow = Q->coarse + sc_coarse_word(0, cy, cz);
        if (dz == -r || dz == r || dy == -r || dy == r) {              // on a face of the shell: the whole run of blocks, word by word
          for (int w = clo >> 5; w <= chi >> 5; w++) {
            uint32_t bits = crow[w] & sc_mask(w == clo >> 5 ? clo : 0, w == chi >> 5 ? chi : 31);
            while (bits) { const int cx = w * 32 + __builtin_ctz(bits); bits &= bits - 1; block(cx, cy, cz); }
          }
        } else {                                                       // inside: the two ends of the run
          if (bx - r >= 0 && ((crow[(bx - r) >> 5] >> ((bx - r) & 31)) & 1)) block(bx - r, cy, cz);
          if (bx + r < RBT_SC_CDIM && ((crow[(bx + r) >> 5] >> ((bx + r) & 31)) & 1)) block(bx + r, cy, cz);
        }
      }
    }
  }
  return best;
}
// one lane per point of P: representatives search Q
RBT_DEV void sc_search(const RbtScoreCloud* P, const RbtScoreCloud* Q, uint32_t* dist, int i) {
  const int16_t* p = P->xyz + 3 * (size_t)i;
  const uint32_t s = cl_slot_find(P->keys, P->lg, pc_voxel_id(p[0], p[1], p[2]));
  dist[i] = P->vals[s] == (uint32_t)i ? sc_nearest(Q, p[0], p[1], p[2]) : RBT_SC_NONE;
}
// the colour error terms e[0..2] (Y, U, V) of a merged point of colour pc against the tie sums: the other cloud's colour is the mean over ALL its merged points at exactly
// the nearest squared distance, rounded half up ((2 sum + n) / (2 n), PCCMetrics.cpp:140-154); the terms are the BT.709 rows of convertRGBtoYUVBT709 (:50-55) times 10000
// applied to the RGB difference (the + 0.5 offsets cancel)
RBT_DEV void sc_color_error(uint32_t pc, uint32_t sr, uint32_t sg, uint32_t sb, uint32_t n, long long e[3]) {
  const int dr = (int)(pc & 255u) - (int)((2 * sr + n) / (2 * n)), dg = (int)((pc >> 8) & 255u) - (int)((2 * sg + n) / (2 * n)), db = (int)(pc >> 16) - (int)((2 * sb + n) / (2 * n));
  e[0] = 2126 * dr + 7152 * dg + 722 * db;
  e[1] = -1146 * dr - 3854 * dg + 5000 * db;
  e[2] = 5000 * dr - 4542 * dg - 458 * db;
}
// walk A -> B for point i of A: its normal to B's tie points (scaleNormals, first half: PCCPointSet.cpp:2322-2380), the D1 term *d, the colour error e. Returns 0 for a point that is no representative.
RBT_DEV int sc_walk_ab(const RbtScoreCloud* A, const RbtScoreCloud* B, const RbtScoreWork* W, int parts, int i, uint32_t* d, long long e[3]) {
  const uint32_t d2 = W->dist_a[i]; if (d2 == RBT_SC_NONE) return 0;
  const int16_t* p = A->xyz + 3 * (size_t)i; const int x = p[0], y = p[1], z = p[2];
  uint32_t sr = 0, sg = 0, sb = 0, n = 0;
  pc_for_ties(B->vol, x, y, z, d2, [&](uint32_t id) {
    const uint32_t s = cl_slot_find(B->keys, B->lg, id);
    if (parts & RBT_SCORE_COLOR) { const uint32_t c = B->col[s]; sr += c & 255u; sg += (c >> 8) & 255u; sb += c >> 16; }
    n++;
    if (parts & RBT_SCORE_D2) {
      const uint32_t j = B->vals[s];
#ifdef RBT_HOSTEMU
      for (int c = 0; c < 3; c++) W->acc_b[3 * (size_t)j + c] += A->nrm[3 * (size_t)i + c];
      W->cnt_b[j]++;
#else
      for (int c = 0; c < 3; c++) atomicAdd((unsigned long long*)&W->acc_b[3 * (size_t)j + c], (unsigned long long)(long long)A->nrm[3 * (size_t)i + c]);
      atomicAdd(&W->cnt_b[j], 1);
#endif
    }
  });
  *d = d2;
  if (parts & RBT_SCORE_COLOR) sc_color_error(A->col[cl_slot_find(A->keys, A->lg, pc_voxel_id(x, y, z))], sr, sg, sb, n, e);
  return 1;
}
// walk B -> A for point j of B: the D1 term, the colour error, the D2 value against A's own normals (computeC2p_, PCCMetrics.cpp:100-124: the mean over A's points at the
// nearest distance of ((p - q) . normal(q))^2, Q14 normals), and the "take" step of scaleNormals for a point that got no normal from the walk A -> B: the sum and
// count of the normals of the source points nearest to it
RBT_DEV int sc_walk_ba(const RbtScoreCloud* B, const RbtScoreCloud* A, const RbtScoreWork* W, int parts, int j, uint32_t* d, long long e[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const uint32_t d2 = W->dist_b[j];
  if (d2 == RBT_SC_NONE) { if (parts & RBT_SCORE_D2) W->val_ba[j] = 0.0; return 0; }
  const int16_t* p = B->xyz + 3 * (size_t)j; const int x = p[0], y = p[1], z = p[2];
  uint32_t sr = 0, sg = 0, sb = 0, n = 0; long long s0 = 0, s1 = 0, s2 = 0; double sum = 0;
  pc_for_ties(A->vol, x, y, z, d2, [&](uint32_t id) {
    const uint32_t s = cl_slot_find(A->keys, A->lg, id);
    if (parts & RBT_SCORE_COLOR) { const uint32_t c = A->col[s]; sr += c & 255u; sg += (c >> 8) & 255u; sb += c >> 16; }
    n++;
    if (parts & RBT_SCORE_D2) {
      const int16_t* q = A->nrm + 3 * (size_t)A->vals[s];
      const int ex = x - (int)(id & (RBT_PCC_DIM - 1)), ey = y - (int)((id >> RBT_PCC_BITS) & (RBT_PCC_DIM - 1)), ez = z - (int)(id >> (2 * RBT_PCC_BITS));
      const long long dot = (long long)ex * q[0] + (long long)ey * q[1] + (long long)ez * q[2];
      const double v = (double)dot / (double)1;
      sum += v * v; s0 += q[0]; s1 += q[1]; s2 += q[2];
    }
  });
  *d = d2;
  if (parts & RBT_SCORE_COLOR) sc_color_error(B->col[cl_slot_find(B->keys, B->lg, pc_voxel_id(x, y, z))], sr, sg, sb, n, e);
  if (parts & RBT_SCORE_D2) {
    W->val_ba[j] = sum / (int)n / (16384.0 * 16384.0);
    if (W->cnt_b[j] == 0) { W->acc_b[3 * (size_t)j] = s0; W->acc_b[3 * (size_t)j + 1] = s1; W->acc_b[3 * (size_t)j + 2] = s2; W->cnt_b[j] = (int32_t)n; }
  }
  return 1;
}
// the colour error terms of sc_walk_ab (dir 0, point i of A) / sc_walk_ba (dir 1, point i of B) at a stored distance: the walks themselves with the colour part alone
RBT_DEV int sc_color_walk(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* dist_a, const uint32_t* dist_b, int dir, int i, long long e[3]) {
  RbtScoreWork W; W.dist_a = (uint32_t*)dist_a; W.dist_b = (uint32_t*)dist_b; W.acc_b = nullptr; W.cnt_b = nullptr; W.val_ab = nullptr; W.val_ba = nullptr; W.part = nullptr; W.res = nullptr;
  uint32_t d = 0;
  return dir ? sc_walk_ba(B, A, &W, RBT_SCORE_COLOR, i, &d, e) : sc_walk_ab(A, B, &W, RBT_SCORE_COLOR, i, &d, e);
}
// third walk, point i of A: the D2 value against B's normals acc_b / cnt_b, complete now (the same mean, each normal sum / count)
RBT_DEV void sc_d2_ab(const RbtScoreCloud* A, const RbtScoreCloud* B, const RbtScoreWork* W, int i) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const uint32_t d2 = W->dist_a[i];
  if (d2 == RBT_SC_NONE) { W->val_ab[i] = 0.0; return; }
  const int16_t* p = A->xyz + 3 * (size_t)i; const int x = p[0], y = p[1], z = p[2];
  double sum = 0; int n = 0;
  pc_for_ties(B->vol, x, y, z, d2, [&](uint32_t id) {
    const uint32_t j = B->vals[cl_slot_find(B->keys, B->lg, id)];
    const int ex = x - (int)(id & (RBT_PCC_DIM - 1)), ey = y - (int)((id >> RBT_PCC_BITS) & (RBT_PCC_DIM - 1)), ez = z - (int)(id >> (2 * RBT_PCC_BITS));
    const long long dot = ex * W->acc_b[3 * (size_t)j] + ey * W->acc_b[3 * (size_t)j + 1] + ez * W->acc_b[3 * (size_t)j + 2];
    const double v = (double)dot / (double)W->cnt_b[j];
    sum += v * v; n++;
  });
  W->val_ab[i] = sum / n / (16384.0 * 16384.0);
}
// The fixed summation order of the D2 values (include/rbt.h). Block b: entries b * 256 + t, t = 0..255 (0 past the end), folded by s[t] += s[t + h] for h = 128, 64, .. 1.
RBT_DEV void sc_fold(RBT_LDS_AS RbtScoreSumLds* L, double* sum, double* max) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  RBT_SYNC();
  for (int h = RBT_SC_SUM / 2; h > 0; h >>= 1) {
    RBT_BLK_FOR(t, h) { L->s[t] = L->s[t] + L->s[t + h]; if (L->m[t + h] > L->m[t]) L->m[t] = L->m[t + h]; }
    RBT_SYNC();
  }
  RBT_BLK_FOR(t, 1) { *sum = L->s[0]; *max = L->m[0]; }
  RBT_SYNC();
}
RBT_DEV void sc_sum_block(const double* val, int n, int b, double* part, RBT_LDS_AS RbtScoreSumLds* L) {
  RBT_BLK_FOR(t, RBT_SC_SUM) { const int i = b * RBT_SC_SUM + t; const double v = i < n ? val[i] : 0.0; L->s[t] = v; L->m[t] = v; }
  sc_fold(L, &part[2 * b], &part[2 * b + 1]);
}
// the block results: lane t adds those of blocks t, t + 256, .. in ascending order, then the same fold. out[0] = sum, out[1] = maximum
RBT_DEV void sc_sum_final(const double* part, int n_blocks, double* out, RBT_LDS_AS RbtScoreSumLds* L) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  RBT_BLK_FOR(t, RBT_SC_SUM) {
    double s = 0.0, m = 0.0;
    for (int b = t; b < n_blocks; b += RBT_SC_SUM) { s = s + part[2 * b]; if (part[2 * b + 1] > m) m = part[2 * b + 1]; }
    L->s[t] = s; L->m[t] = m;
  }
  sc_fold(L, &out[0], &out[1]);
}

// ---- D1 per patch ----
RBT_DEV void pd_label_item(const uint32_t* items, const uint32_t* offsets, int t, int lane, int lanes, uint32_t* labels) {
  const uint32_t l = items[t] >> 16, end = offsets[t + 1];
  for (uint32_t i = offsets[t] + (uint32_t)lane; i < end; i += (uint32_t)lanes) labels[i] = l;
}
// the term of point j of B: its own label and its stored distance. Returns 0 for a point that is no representative.
RBT_DEV int pd_term_ba(const uint32_t* labels_b, const uint32_t* dist_b, int j, uint32_t* label, uint32_t* d) {
  const uint32_t d2 = dist_b[j]; if (d2 == RBT_SC_NONE) return 0;
  *label = labels_b[j]; *d = d2;
  return 1;
}
// the term of point i of A: the label of its owner - the lowest representative of B among the voxels at exactly the stored distance - and that distance
RBT_DEV int pd_term_ab(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* labels_b, const uint32_t* dist_a, int i, uint32_t* label, uint32_t* d) {
  const uint32_t d2 = dist_a[i]; if (d2 == RBT_SC_NONE) return 0;
  const int16_t* p = A->xyz + 3 * (size_t)i;
  uint32_t owner = 0xFFFFFFFFu;
  pc_for_ties(B->vol, p[0], p[1], p[2], d2, [&](uint32_t id) { const uint32_t j = pc_hash_find(B->keys, B->vals, B->lg, id); if (j < owner) owner = j; });
  if (owner >= (uint32_t)B->n) return 0;            // (the distance is that of a voxel of B: there is an owner)
  *label = labels_b[owner]; *d = d2;
  return 1;
}
// sum, count and maximum of one or more terms into the words of patch `label`, direction dir
RBT_DEV void pd_add(unsigned long long* out, uint32_t label, int dir, unsigned long long sum, unsigned long long cnt, unsigned long long mx) {
  unsigned long long* w = out + (size_t)RBT_PD_WORDS * label + dir;
#ifdef RBT_HOSTEMU
  w[RBT_PD_SSE_AB] += sum; w[RBT_PD_N_AB] += cnt; if (mx > w[RBT_PD_MAX_AB]) w[RBT_PD_MAX_AB] = mx;
#else
  if (sum) atomicAdd(&w[RBT_PD_SSE_AB], sum);
  atomicAdd(&w[RBT_PD_N_AB], cnt);
  if (mx) atomicMax(&w[RBT_PD_MAX_AB], mx);
#endif
}

// ---- D2 per patch ----
// sc_fold's tree on the arrays alone: s[0] and m[0] hold sum and maximum when it returns
RBT_DEV void p2_tree(RBT_LDS_AS RbtScoreSumLds* L) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  RBT_SYNC();
  for (int h = RBT_SC_SUM / 2; h > 0; h >>= 1) {
    RBT_BLK_FOR(t, h) { L->s[t] = L->s[t] + L->s[t + h]; if (L->m[t + h] > L->m[t]) L->m[t] = L->m[t + h]; }
    RBT_SYNC();
  }
}
// Block b of direction dir (0: the points of A, 1: of B): entries b * 256 + t. For every distinct label of the block, in the order of its lowest lane, the masked tree of
// sc_sum_block - the values of the label's lanes, 0 elsewhere - is folded, and (label, sum) becomes entry ent_n[b] of the block's range; count and maximum go to `out`.
RBT_DEV void p2_block(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* labels_b, const RbtScoreWork* W, const RbtPatchD2Work* P, unsigned long long* out, int dir, int b,
                      RBT_LDS_AS RbtPatchD2Lds* L) {
  const int n = dir ? B->n : A->n;
  RBT_BLK_FOR(t, RBT_SC_SUM) {
    const int i = b * RBT_SC_SUM + t;
    uint32_t label = 0, d = 0; int valid = 0;
    if (i < n) valid = dir ? pd_term_ba(labels_b, W->dist_b, i, &label, &d) : pd_term_ab(A, B, labels_b, W->dist_a, i, &label, &d);
    L->lab[t] = valid ? label : RBT_SC_NONE; L->v[t] = valid ? (dir ? W->val_ba[i] : W->val_ab[i]) : 0.0;
  }
  RBT_SYNC();
  RBT_BLK_FOR(t, RBT_SC_SUM) {
    const uint32_t mine = L->lab[t]; uint32_t cnt = 0; int lower = 0;
    if (mine != RBT_SC_NONE) for (int u = 0; u < RBT_SC_SUM; u++) if (L->lab[u] == mine) { cnt++; if (u < t) lower = 1; }
    L->lead[t] = lower ? 0u : cnt;
  }
  RBT_SYNC();
  int e = 0;
  for (int k = 0; k < RBT_SC_SUM; k++) {
    const uint32_t cnt = L->lead[k];                                    // the same word for every lane: the branch is uniform over the workgroup
    if (!cnt) continue;
    const uint32_t label = L->lab[k];
    RBT_BLK_FOR(t, RBT_SC_SUM) { const double v = L->lab[t] == label ? L->v[t] : 0.0; L->f.s[t] = v; L->f.m[t] = v; }
    p2_tree(&L->f);
    RBT_BLK_FOR(t, 1) {
      const size_t slot = (size_t)b * RBT_SC_SUM + (size_t)e;
      P->ent_label[slot] = label; P->ent_sum[slot] = L->f.s[0];
      unsigned long long* w = out + (size_t)RBT_P2_WORDS * label + dir; const double mx = L->f.m[0];
      unsigned long long bits; __builtin_memcpy(&bits, &mx, 8);          // a double >= 0 orders as its bit pattern does
#ifdef RBT_HOSTEMU
      w[RBT_P2_N_AB] += cnt; if (bits > w[RBT_P2_MAX_AB]) w[RBT_P2_MAX_AB] = bits;
#else
      atomicAdd(&w[RBT_P2_N_AB], (unsigned long long)cnt);
      if (bits) atomicMax(&w[RBT_P2_MAX_AB], bits);
#endif
    }
    RBT_SYNC();
    e++;
  }
  RBT_BLK_FOR(t, 1) P->ent_n[b] = (uint32_t)e;
}
// the block sums by column: lane t adds the entries of blocks t, t + 256, .. in ascending order into S[label][t] (sc_sum_final's first step, a patch absent from a block adding 0)
RBT_DEV void p2_cols(const RbtPatchD2Work* P, int n_blocks, int t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int b = t; b < n_blocks; b += RBT_SC_SUM) {
    const uint32_t ne = P->ent_n[b];
    for (uint32_t e = 0; e < ne; e++) { const size_t slot = (size_t)b * RBT_SC_SUM + e; double* s = &P->S[(size_t)P->ent_label[slot] * RBT_SC_SUM + (size_t)t]; *s = *s + P->ent_sum[slot]; }
  }
}
// patch k: the fold of sc_sum_final over S[k][0..255] into the patch's sum of direction dir; the row goes back to zero
RBT_DEV void p2_fold(const RbtPatchD2Work* P, unsigned long long* out, int dir, int k, RBT_LDS_AS RbtScoreSumLds* L) {
  double* row = P->S + (size_t)k * RBT_SC_SUM;
  RBT_BLK_FOR(t, RBT_SC_SUM) { L->s[t] = row[t]; L->m[t] = 0.0; row[t] = 0.0; }
  p2_tree(L);
  RBT_BLK_FOR(t, 1) { double* w = (double*)(out + (size_t)RBT_P2_WORDS * (size_t)k + dir); w[RBT_P2_SSE_AB] = L->s[0]; }
}

// ---- colour per patch ----
// the term of point i of the walking cloud (dir 0: A, 1: B): the colour error e of sc_walk_ab / sc_walk_ba and the label it belongs to. ONE walk over the tie set gives the
// tie colour sums and, A -> B, the owner: the lowest point index among the tie voxels (pd_term_ab's rule). Returns 0 for a point that is no representative.
RBT_DEV int pc_term(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* labels_b, const uint32_t* dist_a, const uint32_t* dist_b, int dir, int i, uint32_t* label, long long e[3]) {
  const uint32_t d2 = dir ? dist_b[i] : dist_a[i]; if (d2 == RBT_SC_NONE) return 0;
  const RbtScoreCloud* P = dir ? B : A; const RbtScoreCloud* Q = dir ? A : B;
  const int16_t* p = P->xyz + 3 * (size_t)i; const int x = p[0], y = p[1], z = p[2];
  uint32_t sr = 0, sg = 0, sb = 0, n = 0, owner = 0xFFFFFFFFu;
  pc_for_ties(Q->vol, x, y, z, d2, [&](uint32_t id) {
    const uint32_t s = cl_slot_find(Q->keys, Q->lg, id), c = Q->col[s];
    sr += c & 255u; sg += (c >> 8) & 255u; sb += c >> 16; n++;
    if (!dir) { const uint32_t j = Q->vals[s]; if (j < owner) owner = j; }
  });
  if (!n) return 0;                                 // (the distance is that of a voxel of Q: there is a tie)
  if (dir) *label = labels_b[i];
  else { if (owner >= (uint32_t)B->n) return 0; *label = labels_b[owner]; }
  sc_color_error(P->col[cl_slot_find(P->keys, P->lg, pc_voxel_id(x, y, z))], sr, sg, sb, n, e);
  return 1;
}
// the sums of e[c]^2 and the count of one or more terms into the words of patch `label`, direction dir
RBT_DEV void pc_add(unsigned long long* out, uint32_t label, int dir, const unsigned long long sq[3], unsigned long long cnt) {
  unsigned long long* w = out + (size_t)RBT_PC_WORDS * label;
  unsigned long long* s = w + (dir ? RBT_PC_SSE_BA : RBT_PC_SSE_AB); unsigned long long* n = w + (dir ? RBT_PC_N_BA : RBT_PC_N_AB);
#ifdef RBT_HOSTEMU
  for (int c = 0; c < 3; c++) s[c] += sq[c];
  *n += cnt;
#else
  for (int c = 0; c < 3; c++) if (sq[c]) atomicAdd(&s[c], sq[c]);
  atomicAdd(n, cnt);
#endif
}

#ifdef RBT_HOSTEMU
// serial stand-ins of the launchers (the product's are in rbt_color.hip)
namespace rbtk {
inline void launch_pc_sums(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* labels_b, const uint32_t* dist_a, const uint32_t* dist_b, unsigned long long* out) {
  for (int dir = 0; dir < 2; dir++) for (int i = 0; i < (dir ? B->n : A->n); i++) {
    uint32_t label = 0; long long e[3] = {0, 0, 0};
    if (!pc_term(A, B, labels_b, dist_a, dist_b, dir, i, &label, e)) continue;
    const unsigned long long sq[3] = {(unsigned long long)(e[0] * e[0]), (unsigned long long)(e[1] * e[1]), (unsigned long long)(e[2] * e[2])};
    pc_add(out, label, dir, sq, 1);
  }
}
inline void launch_pd_labels(const uint32_t* items, const uint32_t* offsets, int n_items, uint32_t* labels) { for (int t = 0; t < n_items; t++) pd_label_item(items, offsets, t, 0, 1, labels); }
inline void launch_pd_check(const uint32_t* labels, int n, uint32_t n_patches, uint32_t* err) { for (int i = 0; i < n; i++) if (labels[i] >= n_patches) *err = 1; }
inline void launch_pd_sums(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* labels_b, const uint32_t* dist_a, const uint32_t* dist_b, unsigned long long* out) {
  uint32_t label = 0, d = 0;
  for (int i = 0; i < A->n; i++) if (pd_term_ab(A, B, labels_b, dist_a, i, &label, &d)) pd_add(out, label, 0, d, 1, d);
  for (int j = 0; j < B->n; j++) if (pd_term_ba(labels_b, dist_b, j, &label, &d)) pd_add(out, label, 1, d, 1, d);
}
inline void launch_p2_sums(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* labels_b, const RbtScoreWork* W, const RbtPatchD2Work* P, int n_patches, unsigned long long* out) {
  static RbtPatchD2Lds lds;
  for (int dir = 0; dir < 2; dir++) {
    const int n = dir ? B->n : A->n, nb = (n + RBT_SC_SUM - 1) / RBT_SC_SUM;
    for (int b = 0; b < nb; b++) p2_block(A, B, labels_b, W, P, out, dir, b, &lds);
    for (int t = 0; t < RBT_SC_SUM; t++) p2_cols(P, nb, t);
    for (int k = 0; k < n_patches; k++) p2_fold(P, out, dir, k, &lds.f);
  }
}
inline void launch_sc_check(const int16_t* xyz, int n, uint32_t* scal) { for (int i = 0; i < n; i++) if (!tc_in_range(xyz + 3 * (size_t)i)) scal[RBT_SC_ERR] = 1; }
inline void launch_sc_index(const RbtScoreCloud* S, uint32_t* scal) {
  for (int i = 0; i < S->n; i++) scal[RBT_SC_N_MERGED] += (uint32_t)sc_insert(S, i);
  if (S->rgb) for (uint32_t s = 0; s < (1u << S->lg); s++) sc_merge(S, s);
}
inline void launch_sc_clear(const RbtScoreCloud* S) { for (int i = 0; i < S->n; i++) sc_clear(S, i); }
inline void launch_sc_score(const RbtScoreCloud* A, const RbtScoreCloud* B, int parts, const RbtScoreWork* W) {
  static RbtScoreSumLds lds;
  uint32_t* mx = (uint32_t*)&W->res[RBT_SC_D1_MAX];
  for (int i = 0; i < A->n; i++) sc_search(A, B, W->dist_a, i);
  for (int j = 0; j < B->n; j++) sc_search(B, A, W->dist_b, j);
  for (int dir = 0; dir < 2; dir++) {
    const int n = dir ? B->n : A->n;
    for (int i = 0; i < n; i++) {
      uint32_t d = 0; long long e[3] = {0, 0, 0};
      if (!(dir ? sc_walk_ba(B, A, W, parts, i, &d, e) : sc_walk_ab(A, B, W, parts, i, &d, e))) continue;
      W->res[RBT_SC_D1_AB + dir] += d; if (d > mx[dir]) mx[dir] = d;
      for (int c = 0; c < 3; c++) W->res[(dir ? RBT_SC_COL_BA : RBT_SC_COL_AB) + c] += (unsigned long long)(e[c] * e[c]);
    }
  }
  if (!(parts & RBT_SCORE_D2)) return;
  for (int i = 0; i < A->n; i++) sc_d2_ab(A, B, W, i);
  for (int dir = 0; dir < 2; dir++) {
    const int n = dir ? B->n : A->n, nb = (n + RBT_SC_SUM - 1) / RBT_SC_SUM;
    for (int b = 0; b < nb; b++) sc_sum_block(dir ? W->val_ba : W->val_ab, n, b, W->part, &lds);
    sc_sum_final(W->part, nb, (double*)&W->res[dir ? RBT_SC_D2_BA : RBT_SC_D2_AB], &lds);
  }
}
inline void launch_sc_recolor(const RbtScoreCloud* S) {
  if (S->n <= 0 || !S->rgb) return;
  for (uint32_t s = 0; s < (1u << S->lg); s++) sc_recolor_zero(S, s);
  for (int i = 0; i < S->n; i++) sc_recolor_add(S, i);
  for (uint32_t s = 0; s < (1u << S->lg); s++) sc_merge(S, s);
}
inline void launch_sc_search(const RbtScoreCloud* A, const RbtScoreCloud* B, uint32_t* dist_a, uint32_t* dist_b) {
  for (int i = 0; i < A->n; i++) sc_search(A, B, dist_a, i);
  for (int j = 0; j < B->n; j++) sc_search(B, A, dist_b, j);
}
inline void launch_sc_color_walks(const RbtScoreCloud* A, const RbtScoreCloud* B, const uint32_t* dist_a, const uint32_t* dist_b, unsigned long long* res) {
  for (int dir = 0; dir < 2; dir++) for (int i = 0; i < (dir ? B->n : A->n); i++) {
    long long e[3] = {0, 0, 0};
    if (!sc_color_walk(A, B, dist_a, dist_b, dir, i, e)) continue;
    for (int c = 0; c < 3; c++) res[3 * dir + c] += (unsigned long long)(e[c] * e[c]);
  }
}
}  // namespace rbtk
#endif
