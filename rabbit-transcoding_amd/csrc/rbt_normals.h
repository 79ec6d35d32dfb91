// Normal estimation on a cloud that stays on the device (rbt_pcloud_estimate_normals, rbt_estimate_normals; the definition is in include/rbt.h): what
// PCCNormalsGenerator3::computeNormal does per point on the CPU - kd-tree query, covariance, 3 x 3 eigen-decomposition, orientation - on the index rbt_score uses.
//   lanes    one lane per point, in point order (neighbouring lanes are neighbouring points of a patch), 64-lane workgroups. Only the representative of a voxel (the lowest
//            point index, S->vals) works; its result goes to the voxel's slot (N->slot, 4 x int16 beside the map's slot) and to its own entry of the output. A second
//            short kernel copies the slot's triple to the voxel's other points.
//   search   the best k keys (squared distance << 32 | voxel id), ascending, in registers; an unrolled insertion as tc_forward's, instantiated for 16 and for 32 keys. A
//            k below the instantiation's size uses the upper k entries, so that the k-th key is always the last register. The volume is read by 32-bit words: first the
//            7 x 7 rows around the query, masked to x - 3 .. x + 3 (a surface has about 28 voxels there, which covers k = 16), then shells of coarse blocks of growing
//            Chebyshev radius as sc_nearest walks them, without the cube's voxels. The walk ends when the next shell's nearest possible voxel is STRICTLY farther than the
//            k-th distance: a voxel at exactly that distance can still win the tie with a lower voxel id. The host passes k = min(k, occupied voxels), so the keys fill up
//            in every cloud and the rule needs no second form.
//   solve    integer sums from the keys, S = m sum(q q^T) - sum(q) sum(q)^T exactly, then double: the quaternion Jacobi iteration the reference uses (PCCMath.h
//            PCCDiagonalize) restated - at most 24 rotations, the largest off-diagonal magnitude as pivot with the reference's comparison order, the same sums in the same
//            order, the same stops - the reference's column choice on |D_ii|, orientation, Q14. + - * /, fabs and sqrt only, each rounded on its own (this file is compiled
//            with -ffp-contract=off like the rest of the colour stages). The rotation count differs from lane to lane: lanes that are done idle, and
//            the loop body has no branch of its own besides the stops. The solve is a few hundred FP64 operations a point, next to a search of 49 to 98 loads.
// No kernel waits for another; every loop is bounded by the size of the volume; no LDS.
#pragma once
#include "rbt_score.h"

enum { RBT_NM_FINE_R = 3, RBT_NM_ROTATIONS = 24, RBT_NM_K_DEFAULT = 16, RBT_NM_K_MIN = 3, RBT_NM_K_MAX = 32 };
// one estimation. k: min(the caller's k, occupied voxels) >= 1; orient: RBT_NORMALS_ORIENT_NONE or _VIEW_POINT; out: 3 per point; slot: 4 per slot of the cloud's map
struct RbtNormals { int32_t k, orient, vp[3]; int16_t* out; int16_t* slot; };

namespace rbtk {
void launch_nm_estimate(const RbtScoreCloud* S, const RbtNormals* N);
}  // namespace rbtk

#ifdef RBT_HOSTEMU
#define RBT_NM_UNROLL
#else
#define RBT_NM_UNROLL _Pragma("unroll")
#endif

// ------------------------------------------------------------------------------------------------ bodies (device and host emulation)
template <int KMAX> RBT_DEV void nm_insert(unsigned long long (&K)[KMAX], int lo, unsigned long long key) {
  if (key >= K[KMAX - 1]) return;
  RBT_NM_UNROLL
  for (int j = 0; j < KMAX; j++) if (j >= lo && key < K[j]) { const unsigned long long t = K[j]; K[j] = key; key = t; }
}
// the set bits of `bits` (bit b = voxel x0 + b of row yy, zz, at squared distance `base` in y and z)
template <int KMAX> RBT_DEV void nm_row(unsigned long long (&K)[KMAX], int lo, uint32_t bits, int x0, int x, int yy, int zz, uint32_t base) {
  while (bits) {
    const int xx = x0 + __builtin_ctz(bits); bits &= bits - 1;
    const int dx = xx - x;
    nm_insert<KMAX>(K, lo, (unsigned long long)(base + (uint32_t)(dx * dx)) << 32 | pc_voxel_id(xx, yy, zz));
  }
}
// bits x - R .. x + R of the byte that starts at voxel x0
RBT_DEV uint32_t nm_cube_byte(int x, int x0) {
  const int sh = x - RBT_NM_FINE_R - x0; const uint32_t m = (1u << (2 * RBT_NM_FINE_R + 1)) - 1;
  return sh <= -(2 * RBT_NM_FINE_R + 1) || sh >= 8 ? 0u : (sh >= 0 ? m << sh : m >> -sh) & 0xFFu;
}
// the k nearest occupied voxels of (x, y, z), itself included, by (squared distance, voxel id): K[KMAX - k .. KMAX - 1]
template <int KMAX> RBT_DEV void nm_search(const RbtScoreCloud* Q, int k, int x, int y, int z, unsigned long long (&K)[KMAX]) {
  const uint32_t* vol = Q->vol;
  const int kl = KMAX - k;
  RBT_NM_UNROLL
  for (int j = 0; j < KMAX; j++) K[j] = ~0ull;
  const int lo = x - RBT_NM_FINE_R < 0 ? 0 : x - RBT_NM_FINE_R, hi = x + RBT_NM_FINE_R >= RBT_PCC_DIM ? RBT_PCC_DIM - 1 : x + RBT_NM_FINE_R;
  const int w0 = lo >> 5, w1 = hi >> 5;
  for (int dz = -RBT_NM_FINE_R; dz <= RBT_NM_FINE_R; dz++) {
    const int zz = z + dz; if (zz < 0 || zz >= RBT_PCC_DIM) continue;
    for (int dy = -RBT_NM_FINE_R; dy <= RBT_NM_FINE_R; dy++) {
      const int yy = y + dy; if (yy < 0 || yy >= RBT_PCC_DIM) continue;
      const uint32_t* row = vol + pc_voxel_word(0, yy, zz); const uint32_t base = (uint32_t)(dz * dz + dy * dy);
      for (int w = w0; w <= w1; w++) nm_row<KMAX>(K, kl, row[w] & sc_mask(w == w0 ? lo : 0, w == w1 ? hi : 31), w * 32, x, yy, zz, base);
    }
  }
  // everything outside the cube is at least RBT_NM_FINE_R + 1 away (the k-th distance is 0xFFFFFFFF while a key is free)
  if ((uint32_t)(K[KMAX - 1] >> 32) < (uint32_t)((RBT_NM_FINE_R + 1) * (RBT_NM_FINE_R + 1))) return;
  const int bx = x >> RBT_SC_BLOCK_BITS, by = y >> RBT_SC_BLOCK_BITS, bz = z >> RBT_SC_BLOCK_BITS;
  auto block = [&](int cx, int cy, int cz) {                            // an occupied block: its 8 x 8 rows, one byte of a volume word each, without the cube's voxels
    const int gx = sc_gap(x, cx), gy = sc_gap(y, cy), gz = sc_gap(z, cz);
    if ((uint32_t)(gx * gx + gy * gy + gz * gz) > (uint32_t)(K[KMAX - 1] >> 32)) return;
    const int x0 = cx << RBT_SC_BLOCK_BITS; const uint32_t cube = nm_cube_byte(x, x0);
    for (int zz = cz << RBT_SC_BLOCK_BITS; zz < (cz + 1) << RBT_SC_BLOCK_BITS; zz++)
      for (int yy = cy << RBT_SC_BLOCK_BITS; yy < (cy + 1) << RBT_SC_BLOCK_BITS; yy++) {
        const int ey = yy - y, ez = zz - z; const uint32_t base = (uint32_t)(ez * ez + ey * ey);
        if (base > (uint32_t)(K[KMAX - 1] >> 32)) continue;
        uint32_t bits = (vol[pc_voxel_word(x0, yy, zz)] >> (x0 & 31)) & 0xFFu;
        if (ey >= -RBT_NM_FINE_R && ey <= RBT_NM_FINE_R && ez >= -RBT_NM_FINE_R && ez <= RBT_NM_FINE_R) bits &= ~cube;
        nm_row<KMAX>(K, kl, bits, x0, x, yy, zz, base);
      }
  };
  for (int r = 0; r < RBT_SC_CDIM; r++) {
    // a block of shell r lies at least 8 (r - 1) + 1 away along the axis on which it is r blocks off
    if (r > 0) { const uint32_t lb = (uint32_t)(((r - 1) << RBT_SC_BLOCK_BITS) + 1); if (lb * lb > (uint32_t)(K[KMAX - 1] >> 32)) break; }
    const int clo = bx - r < 0 ? 0 : bx - r, chi = bx + r >= RBT_SC_CDIM ? RBT_SC_CDIM - 1 : bx + r;
    for (int dz = -r; dz <= r; dz++) {
      const int cz = bz + dz; if (cz < 0 || cz >= RBT_SC_CDIM) continue;
      for (int dy = -r; dy <= r; dy++) {
        const int cy = by + dy; if (cy < 0 || cy >= RBT_SC_CDIM) continue;
        const int gy = sc_gap(y, cy), gz = sc_gap(z, cz);
        if ((uint32_t)(gy * gy + gz * gz) > (uint32_t)(K[KMAX - 1] >> 32)) continue;
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
}

// The eigenvector of the symmetric matrix a (a00 a01 a02 / a11 a12 / a22) that the reference would take as the normal: its Jacobi iteration on a unit quaternion, then
// the column of the smallest |D_ii| (column 0 only if strictly smallest, else column 1 if D11 < D22, else column 2). An isotropic matrix gives (0, 0, 1).
RBT_DEV void nm_eigenvector(double a00, double a01, double a02, double a11, double a12, double a22, double v[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double qx = 0.0, qy = 0.0, qz = 0.0, qw = 1.0;
  double r00 = 1.0, r01 = 0.0, r02 = 0.0, r10 = 0.0, r11 = 1.0, r12 = 0.0, r20 = 0.0, r21 = 0.0, r22 = 1.0, d00 = a00, d11 = a11, d22 = a22;
  for (int it = 0; it < RBT_NM_ROTATIONS; it++) {     // what the loop leaves is the matrix pair of its last pass: after a 24th rotation they are not formed again

    // rotation matrix of the quaternion (row i, column j: r_ij)
    const double xx = qx * qx, yy = qy * qy, zz = qz * qz, ww = qw * qw;
    r00 = xx - yy - zz + ww; r11 = -xx + yy - zz + ww; r22 = -xx - yy + zz + ww;
    double s = qx * qy, t = qz * qw;
    r10 = 2.0 * (s + t); r01 = 2.0 * (s - t);
    s = qx * qz; t = qy * qw;
    r20 = 2.0 * (s - t); r02 = 2.0 * (s + t);
    s = qy * qz; t = qx * qw;
    r21 = 2.0 * (s + t); r12 = 2.0 * (s - t);
    // B = A R, then D = R^T B; every entry a sum of three products, left to right
    const double b00 = r00 * a00 + r10 * a01 + r20 * a02, b01 = r01 * a00 + r11 * a01 + r21 * a02, b02 = r02 * a00 + r12 * a01 + r22 * a02;
    const double b10 = r00 * a01 + r10 * a11 + r20 * a12, b11 = r01 * a01 + r11 * a11 + r21 * a12, b12 = r02 * a01 + r12 * a11 + r22 * a12;
    const double b20 = r00 * a02 + r10 * a12 + r20 * a22, b21 = r01 * a02 + r11 * a12 + r21 * a22, b22 = r02 * a02 + r12 * a12 + r22 * a22;
    d00 = b00 * r00 + b10 * r10 + b20 * r20;
    d11 = b01 * r01 + b11 * r11 + b21 * r21;
    d22 = b02 * r02 + b12 * r12 + b22 * r22;
    const double o0 = b01 * r02 + b11 * r12 + b21 * r22;              // D12
    const double o1 = b00 * r02 + b10 * r12 + b20 * r22;              // D02
    const double o2 = b00 * r01 + b10 * r11 + b20 * r21;              // D01
    const double m0 = __builtin_fabs(o0), m1 = __builtin_fabs(o1), m2 = __builtin_fabs(o2);
    const int p = (m0 > m1 && m0 > m2) ? 0 : (m1 > m2 ? 1 : 2);        // the pivot; the rotation is about axis p and mixes the other two, p + 1 and p + 2 (mod 3)
    const double op = p == 0 ? o0 : (p == 1 ? o1 : o2);
    if (op == 0.0) break;
    const double dn = p == 0 ? d11 : (p == 1 ? d22 : d00), df = p == 0 ? d22 : (p == 1 ? d00 : d11);
    double th = (df - dn) / (2.0 * op);
    const double sg = th > 0.0 ? 1.0 : -1.0;
    th = th * sg;
    const double tn = sg / (th + (th < 1.0e6 ? __builtin_sqrt(th * th + 1.0) : th));
    const double c = 1.0 / __builtin_sqrt(tn * tn + 1.0);
    if (c == 1.0) break;
    const double h = -1.0 * (sg * __builtin_sqrt((1.0 - c) / 2.0));   // sine of the half angle, for the row-vector convention of the matrix above
    const double jx = p == 0 ? h : 0.0, jy = p == 1 ? h : 0.0, jz = p == 2 ? h : 0.0, jw = __builtin_sqrt(1.0 - h * h);
    if (jw == 1.0) break;
    // q <- q * j, component after component, each using the components already replaced (as the reference does), then normalised
    qx = qw * jx + qx * jw + qy * jz - qz * jy;
    qy = qw * jy - qx * jz + qy * jw + qz * jx;
    qz = qw * jz + qx * jy - qy * jx + qz * jw;
    qw = qw * jw - qx * jx - qy * jy - qz * jz;
    const double n = __builtin_sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
    qx = qx / n; qy = qy / n; qz = qz / n; qw = qw / n;
  }
  d00 = __builtin_fabs(d00); d11 = __builtin_fabs(d11); d22 = __builtin_fabs(d22);
  if (d00 < d11 && d00 < d22) { v[0] = r00; v[1] = r10; v[2] = r20; }
  else if (d11 < d22) { v[0] = r01; v[1] = r11; v[2] = r21; }
  else { v[0] = r02; v[1] = r12; v[2] = r22; }
}
RBT_DEV int16_t nm_q14(double v) { return (int16_t)__builtin_round(16384.0 * v); }       // half away from zero, as tc_round16

// the normal of the voxel of (x, y, z) in Q14
template <int KMAX> RBT_DEV void nm_voxel(const RbtScoreCloud* S, const RbtNormals* N, int x, int y, int z, int16_t q[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  unsigned long long K[KMAX];
  nm_search<KMAX>(S, N->k, x, y, z, K);
  long long sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0, m = 0;
  RBT_NM_UNROLL
  for (int j = 0; j < KMAX; j++) if (j >= KMAX - N->k && K[j] != ~0ull) {
    const uint32_t id = (uint32_t)K[j];
    const long long px = id & (RBT_PCC_DIM - 1), py = (id >> RBT_PCC_BITS) & (RBT_PCC_DIM - 1), pz = id >> (2 * RBT_PCC_BITS);
    sx += px; sy += py; sz += pz; sxx += px * px; sxy += px * py; sxz += px * pz; syy += py * py; syz += py * pz; szz += pz * pz; m++;
  }
  q[0] = q[1] = q[2] = 0;
  if (m <= 1) return;
  double v[3];
  nm_eigenvector((double)(m * sxx - sx * sx), (double)(m * sxy - sx * sy), (double)(m * sxz - sx * sz), (double)(m * syy - sy * sy), (double)(m * syz - sy * sz), (double)(m * szz - sz * sz), v);
  if (N->orient == RBT_NORMALS_ORIENT_VIEW_POINT) {
    const double dot = v[0] * ((double)N->vp[0] - (double)x) + v[1] * ((double)N->vp[1] - (double)y) + v[2] * ((double)N->vp[2] - (double)z);
    if (dot < 0.0) { v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
  }
  for (int c = 0; c < 3; c++) q[c] = nm_q14(v[c]);
}
// point i: the representative of a voxel computes the voxel's normal
template <int KMAX> RBT_DEV void nm_point(const RbtScoreCloud* S, const RbtNormals* N, int i) {
  const int16_t* p = S->xyz + 3 * (size_t)i;
  const uint32_t s = cl_slot_find(S->keys, S->lg, pc_voxel_id(p[0], p[1], p[2]));
  if (S->vals[s] != (uint32_t)i) return;
  int16_t q[3];
  nm_voxel<KMAX>(S, N, p[0], p[1], p[2], q);
  for (int c = 0; c < 3; c++) { N->slot[4 * (size_t)s + c] = q[c]; N->out[3 * (size_t)i + c] = q[c]; }
}
// point i: every other point of the voxel takes the voxel's normal
RBT_DEV void nm_spread(const RbtScoreCloud* S, const RbtNormals* N, int i) {
  const int16_t* p = S->xyz + 3 * (size_t)i;
  const uint32_t s = cl_slot_find(S->keys, S->lg, pc_voxel_id(p[0], p[1], p[2]));
  if (S->vals[s] == (uint32_t)i) return;
  for (int c = 0; c < 3; c++) N->out[3 * (size_t)i + c] = N->slot[4 * (size_t)s + c];
}

#ifdef RBT_HOSTEMU
// serial stand-in of the launcher (the product's is in rbt_normals.hip)
namespace rbtk {
inline void launch_nm_estimate(const RbtScoreCloud* S, const RbtNormals* N) {
  for (int i = 0; i < S->n; i++) { if (N->k <= 16) nm_point<16>(S, N, i); else nm_point<32>(S, N, i); }
  for (int i = 0; i < S->n; i++) nm_spread(S, N, i);
}
}  // namespace rbtk
#endif
