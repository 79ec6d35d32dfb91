// TEST HOOK (rbt_selftest_tb, include/rbt.h): one transform block through the decoder's own rc_tile_tb / rc_tile_tb_cpair, one wave per case. The case is staged into a CTB
// tile the way rbt_recon_ctb stages a CTB - neighbour samples in the tile body / the row above / the left border column, unit availability in uav, levels where the block's
// samples will be - then the routine the CTB kernel calls is called, and what it left at the block's position is copied out. Shared by the device kernel
// (rbt_kernels.hip k_selftest_tb), the serial host emulation (tests/hostemu) and the sanitizer program (tests/tb_check.cpp). The host has validated the case
// (host/rbt_api.cpp tb_case_ok): every index below stays inside the tile for a valid case.
#pragma once
#include "rbt_recon.h"
#include "../../include/rbt.h"

RBT_DEV void rc_selftest_tb_case(const rbt_tb_case* cp, const uint16_t* nb, const uint8_t* unit_av, const int16_t* lev, uint16_t* out, RBT_LDS_AS RbtCtbTile* t, RBT_LDS_AS RbtReconRole* R) {
  const int kind = RBT_UNI(cp->kind), log2 = RBT_UNI(cp->log2), bd = RBT_UNI(cp->bit_depth), log2_ctb = RBT_UNI(cp->log2_ctb), x0 = RBT_UNI(cp->x0), y0 = RBT_UNI(cp->y0);
  const int intra = RBT_UNI(cp->intra), mode = RBT_UNI(cp->mode), cbf0 = RBT_UNI(cp->cbf[0]), cbf1 = RBT_UNI(cp->cbf[1]), ts = RBT_UNI(cp->transform_skip), byp = RBT_UNI(cp->cu_transquant_bypass);
  const int qp0 = RBT_UNI(cp->qp[0]), qp1 = RBT_UNI(cp->qp[1]);
  RbtStreamCfg g; __builtin_memset(&g, 0, sizeof g);
  g.bit_depth = (int8_t)bd; g.log2_ctb = (int8_t)log2_ctb; g.strong_intra = (uint8_t)RBT_UNI(cp->strong_intra_smoothing);
  const int sh = kind != RBT_TB_LUMA, N = 1 << log2, nn = (1 << log2_ctb) >> sh, n4 = (1 << log2_ctb) >> 2, n_planes = kind == RBT_TB_PAIR ? 2 : 1, S = sh ? RC_TS_C : RC_TS_Y;
  // everything the case does not set is a pattern no sample takes: a read of something that was not staged shows in the result
  RBT_PAR_FOR(i, (int)(sizeof(RbtCtbTile) / 2)) ((RBT_LDS_AS uint16_t*)t)[i] = 0xA5A5;
  RBT_PAR_FOR(i, 17 * RC_US) R->uav[i] = 0;
  RBT_SYNC_LDS();
  for (int b = 0; b < n_planes; b++) {
    const int pl = kind == RBT_TB_LUMA ? 0 : (kind == RBT_TB_PAIR ? b + 1 : kind);
    RBT_LDS_AS uint16_t* tile = pl == 0 ? t->y : t->c[pl - 1]; RBT_LDS_AS uint16_t* top = pl == 0 ? t->top_y : t->top_c[pl - 1];
    RBT_PAR_FOR(i, 4 * N + 1) {
      const uint16_t v = nb[b * RBT_TB_NB + i];
      if (i < 2 * N) { const int yy = y0 + 2 * N - 1 - i; if (yy < nn) tile[yy * S + x0] = v; }                       // column x0 - 1
      else { const int xx = x0 - 1 + (i - 2 * N); if (y0 == 0) top[xx + 1] = v; else if (xx < nn) tile[(y0 - 1) * S + xx + 1] = v; }
    }
    RBT_PAR_FOR(i, N * N) { const int x = i & (N - 1), y = i >> log2; tile[(y0 + y) * S + x0 + x + 1] = (uint16_t)lev[b * 1024 + i]; }
  }
  RBT_PAR_FOR(p, rc_nb_units(N, sh)) {
    int xn, yn; rc_nb_unit_xy(p, x0, y0, N, sh, &xn, &yn);
    const int ux = (xn * (1 << sh)) >> 2, uy = (yn * (1 << sh)) >> 2;
    if (uy < n4 && (uy < 0 || ux < n4)) R->uav[(uy + 1) * RC_US + ux + 1] = (uint8_t)(unit_av[p] != 0);
  }
  RBT_SYNC_LDS();
  if (kind == RBT_TB_PAIR) rc_tile_tb_cpair(&g, t, R, x0, y0, log2, intra, mode, cbf0, cbf1, byp, qp0, qp1);
  else if (kind == RBT_TB_LUMA) rc_tile_tb(&g, t, R, 0, x0, y0, log2, intra, mode, cbf0, ts, byp, qp0, intra ? log2 - 2 : -1, x0 >> 2, y0 >> 2, 1);
  else rc_tile_tb(&g, t, R, kind, x0, y0, log2, intra, mode, cbf0, ts, byp, qp0, -1, 0, 0, 0);
  RBT_SYNC_LDS();
  for (int b = 0; b < n_planes; b++) {
    const int pl = kind == RBT_TB_LUMA ? 0 : (kind == RBT_TB_PAIR ? b + 1 : kind);
    const RBT_LDS_AS uint16_t* tile = pl == 0 ? t->y : t->c[pl - 1];
    RBT_PAR_FOR(i, N * N) { const int x = i & (N - 1), y = i >> log2; out[b * 1024 + i] = tile[(y0 + y) * S + x0 + x + 1]; }
  }
  RBT_SYNC_LDS();
}
