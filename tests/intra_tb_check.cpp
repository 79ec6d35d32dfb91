// TEST-ONLY: the intra chain's transform-block code (csrc/rbt_encode.h: en_tile_intra_tb, en_tile_intra_tb_cpair, en_intra_cu_luma) as a stand-alone host program, so that
// it can be built with -fsanitize=address,undefined and run on the CPU (tests/test_intra_tb.py). It is linked with the host emulation's sources (tests/hostemu): the kernel
// bodies run as serial host code and the LDS structs are plain objects, so an index past the end of an array of the tile or the scratch is an error here.
// Every argument is a case file written by the test: ten int32 (width, height, bit depth, frames, qp, gop, lossless, log2_ctb, rows per slice, bytes of the expected
// stream), the source frames (uint16, 4:2:0), the expected stream - the oracle's. The case is encoded through rbt_encode and held against it byte for byte, then decoded
// with the hashes checked. The counters of the host build (rbt_hostemu_intra_tb) must have moved. Prints "ok".
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../include/rbt.h"

extern "C" uint32_t rbt_hostemu_intra_tb[5];

static int fail(const char* what, const char* path, long a = 0, long b = 0) { printf("FAIL %s (%s) %ld %ld\n", what, path, a, b); fflush(stdout); return 1; }

static int run_case(rbt_ctx* ctx, const char* path) {
  FILE* fp = fopen(path, "rb");
  if (!fp) return fail("open", path);
  int32_t hd[10];
  if (fread(hd, sizeof hd, 1, fp) != 1) { fclose(fp); return fail("header", path); }
  const int w = hd[0], h = hd[1], bd = hd[2], n = hd[3], qp = hd[4], gop = hd[5], lossless = hd[6], log2_ctb = hd[7], rows = hd[8];
  std::vector<uint16_t> yuv((size_t)n * w * h * 3 / 2); std::vector<uint8_t> want((size_t)hd[9]);
  const bool got_all = fread(yuv.data(), 2, yuv.size(), fp) == yuv.size() && fread(want.data(), 1, want.size(), fp) == want.size();
  fclose(fp);
  if (!got_all) return fail("body", path);
  uint8_t* out = nullptr; size_t n_out = 0;
  int rc = rbt_encode(ctx, yuv.data(), w, h, bd, n, qp, gop, lossless, log2_ctb, rows, 1, &out, &n_out);
  if (rc != 0) return fail("rbt_encode", path, rc);
  if (n_out != want.size() || memcmp(out, want.data(), n_out) != 0) { rbt_free(out); return fail("stream differs from the oracle's", path, (long)n_out, (long)want.size()); }
  rbt_video v; memset(&v, 0, sizeof v);
  rc = rbt_decode(ctx, out, n_out, 1, &v);
  rbt_free(out);
  if (rc != 0) return fail("rbt_decode", path, rc);
  const int bad = v.width != w || v.height != h || v.n_frames != n || v.md5_checked != n || v.md5_failed != 0;
  rbt_free(v.data);
  if (bad) return fail("decoded stream", path);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return fail("usage: intra_tb_check CASE...", "");
  rbt_ctx* ctx = nullptr;
  if (rbt_create(&ctx, 0, 0, 1) != 0) return fail("rbt_create", "");
  for (int i = 1; i < argc; i++) if (run_case(ctx, argv[i])) { rbt_destroy(ctx); return 1; }
  rbt_destroy(ctx);
  // one block or four went both ways, and a coded mode trial left its prediction in the (here: poisoned) tile
  if (!rbt_hostemu_intra_tb[0] || !rbt_hostemu_intra_tb[1] || !rbt_hostemu_intra_tb[4]) return fail("counters", "", rbt_hostemu_intra_tb[0], rbt_hostemu_intra_tb[4]);
  printf("counters %u %u %u %u %u\nok\n", rbt_hostemu_intra_tb[0], rbt_hostemu_intra_tb[1], rbt_hostemu_intra_tb[2], rbt_hostemu_intra_tb[3], rbt_hostemu_intra_tb[4]);
  return 0;
}
