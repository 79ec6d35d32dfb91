// Kernels and launchers of the decoded picture hashes (rbt_hash.h). A translation unit of its own: the MD5 chain is a latency chain
// (one lane per plane) and is compiled with -O3 like the parser.
#include <hip/hip_runtime.h>
#include "rbt_hash.h"

namespace rbtk {
hipStream_t current_stream();            // rbt_kernels.hip: the stream the host code selected (set_stream)
#define g_stream current_stream()

RBT_DEV void hash_plane_of(const RbtHashPic* pics, const int32_t* list, int n_list, int q, int& pi, int& c, const uint16_t*& p, int& pw, int& ph) {
  c = q / n_list; pi = list[q - c * n_list];
  const RbtHashPic& P = pics[pi];
  pw = c ? P.w >> 1 : P.w; ph = c ? P.h >> 1 : P.h; p = P.plane[c];
}

// MD5: lane q hashes plane q of the list (luma planes of all pictures first, then Cb, then Cr: lanes of a wave walk planes of one size).
// The full blocks come from 16-byte loads issued PF blocks ahead of the block being hashed; the last one or two blocks (tail, 0x80,
// length) are built byte by byte (rbt_md5_tail). A wide plane's bytes are its samples as they lie in memory (little-endian: low byte
// first); at bit depth 8 a block is the low bytes of 64 samples.
template <int WIDE>
__global__ void __launch_bounds__(64) k_hash_md5(const RbtHashPic* pics, const int32_t* list, int n_list, uint32_t* state) {
  const int q = (int)(blockIdx.x * 64 + threadIdx.x);
  if (q >= 3 * n_list) return;
  int pi, c, pw, ph; const uint16_t* p;
  hash_plane_of(pics, list, n_list, q, pi, c, p, pw, ph);
  const size_t L = rbt_hash_plane_bytes(pw, ph, WIDE), nb = L / 64;
  constexpr int NR = WIDE ? 4 : 8, PF = WIDE ? 4 : 2;    // 16-byte loads per block, blocks in flight
  const uint4* src = (const uint4*)p;
  uint32_t st[4]; rbt_md5_init(st);
  uint4 r[PF][NR];
#pragma unroll
  for (int u = 0; u < PF; u++) if ((size_t)u < nb) {
#pragma unroll
    for (int i = 0; i < NR; i++) r[u][i] = src[(size_t)u * NR + i];
  }
  for (size_t k = 0; k < nb; k += PF) {
#pragma unroll
    for (int u = 0; u < PF; u++) if (k + u < nb) {
      uint32_t M[16];
      if (WIDE) {
#pragma unroll
        for (int i = 0; i < 4; i++) { M[4 * i] = r[u][i].x; M[4 * i + 1] = r[u][i].y; M[4 * i + 2] = r[u][i].z; M[4 * i + 3] = r[u][i].w; }
      } else {
        // two samples per 32-bit word: the low bytes of four samples make one message word
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const uint32_t a = r[u][i].x, b = r[u][i].y, d = r[u][i].z, e = r[u][i].w;
          M[2 * i] = (a & 0xFFu) | ((a >> 8) & 0xFF00u) | ((b & 0xFFu) << 16) | ((b << 8) & 0xFF000000u);
          M[2 * i + 1] = (d & 0xFFu) | ((d >> 8) & 0xFF00u) | ((e & 0xFFu) << 16) | ((e << 8) & 0xFF000000u);
        }
      }
      if (k + u + PF < nb) {
#pragma unroll
        for (int i = 0; i < NR; i++) r[u][i] = src[(k + u + PF) * NR + i];
      }
      rbt_md5_block(st, M);
    }
  }
  rbt_md5_tail(st, p, L, WIDE, nb);
  uint32_t* o = state + (size_t)pi * RBT_HASH_STATE_WORDS + 4 * c;
  o[0] = st[0]; o[1] = st[1]; o[2] = st[2]; o[3] = st[3];
}

// CRC: lane = one RBT_CRC_SEG-byte segment of a plane (blockIdx.y: the plane), table-driven in LDS; the placed remainders of the wave are
// combined by XOR and the wave's result XORed into the plane's state word
template <int WIDE>
__global__ void __launch_bounds__(64) k_hash_crc(const RbtHashPic* pics, const int32_t* list, int n_list, uint32_t* state) {
  __shared__ uint32_t T[256];
  int pi, c, pw, ph; const uint16_t* p;
  hash_plane_of(pics, list, n_list, (int)blockIdx.y, pi, c, p, pw, ph);
  const size_t L = rbt_hash_plane_bytes(pw, ph, WIDE);
  if ((size_t)blockIdx.x * 64 * RBT_CRC_SEG >= L) return;   // the whole workgroup
  for (int v = (int)threadIdx.x; v < 256; v += 64) T[v] = rbt_crc_table_entry((uint32_t)v);
  __syncthreads();
  const size_t b0 = ((size_t)blockIdx.x * 64 + threadIdx.x) * RBT_CRC_SEG;
  uint32_t part = 0;
  if (b0 < L) {
    const size_t b1 = b0 + RBT_CRC_SEG < L ? b0 + RBT_CRC_SEG : L;
    const size_t s1 = WIDE ? b1 / 2 : b1;       // samples [s, s1) (L is even when wide)
    size_t s = WIDE ? b0 / 2 : b0;              // a multiple of 8: 16-byte aligned
    uint32_t crc = 0;
    auto step = [&](uint32_t smp) {
      crc = ((crc << 8) ^ T[((crc >> 8) ^ smp) & 0xFFu]) & 0xFFFFu;
      if (WIDE) crc = ((crc << 8) ^ T[((crc >> 8) ^ (smp >> 8)) & 0xFFu]) & 0xFFFFu;
    };
    for (; s + 8 <= s1; s += 8) {
      const uint4 v = *(const uint4*)(p + s);
      step(v.x & 0xFFFFu); step(v.x >> 16); step(v.y & 0xFFFFu); step(v.y >> 16);
      step(v.z & 0xFFFFu); step(v.z >> 16); step(v.w & 0xFFFFu); step(v.w >> 16);
    }
    for (; s < s1; s++) step(p[s]);
    part = rbt_crc_place(crc, b0, b1, L);
  }
  for (int o = 32; o > 0; o >>= 1) part ^= (uint32_t)__shfl_xor((int)part, o);
  if (threadIdx.x == 0 && part) atomicXor(state + (size_t)pi * RBT_HASH_STATE_WORDS + 4 * c, part);
}

// checksum: one workgroup per row of a plane (blockIdx.x: the row, blockIdx.y: the plane)
template <int WIDE>
__global__ void __launch_bounds__(256) k_hash_sum(const RbtHashPic* pics, const int32_t* list, int n_list, uint32_t* state) {
  int pi, c, pw, ph; const uint16_t* p;
  hash_plane_of(pics, list, n_list, (int)blockIdx.y, pi, c, p, pw, ph);
  const int y = (int)blockIdx.x;
  if (y >= ph) return;
  const uint16_t* row = p + (size_t)y * pw;
  uint32_t s = 0;
  for (int x = (int)threadIdx.x; x < pw; x += 256) s += rbt_sum_sample(row[x], x, y, WIDE);
  for (int o = 32; o > 0; o >>= 1) s += (uint32_t)__shfl_xor((int)s, o);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(state + (size_t)pi * RBT_HASH_STATE_WORDS + 4 * c, s);
}

__global__ void __launch_bounds__(64) k_hash_finish(const RbtHashPic* pics, int n, const uint32_t* state, uint8_t* out, uint32_t* counters) {
  const int i = (int)(blockIdx.x * 64 + threadIdx.x);
  if (i < n && rbt_hash_finish_pic(pics[i], state + (size_t)i * RBT_HASH_STATE_WORDS, out + (size_t)i * 48)) atomicAdd(counters + pics[i].counter, 1u);
}

void launch_hash(const RbtHashPic* pics, const int32_t* list, int n_list, int kind, int wide, int max_luma, int max_h, uint32_t* state) {
  if (n_list <= 0) return;
  const unsigned planes = 3u * (unsigned)n_list;   // n_list <= RBT_HASH_MAX_PICS: within the grid's y limit
  if (kind == RBT_HASH_MD5) {
    if (wide) hipLaunchKernelGGL(k_hash_md5<1>, dim3((planes + 63) / 64), dim3(64), 0, g_stream, pics, list, n_list, state);
    else hipLaunchKernelGGL(k_hash_md5<0>, dim3((planes + 63) / 64), dim3(64), 0, g_stream, pics, list, n_list, state);
  } else if (kind == RBT_HASH_CRC) {
    const size_t bytes = (size_t)max_luma * (wide ? 2 : 1), per_wg = (size_t)64 * RBT_CRC_SEG;
    const dim3 grid((unsigned)((bytes + per_wg - 1) / per_wg), planes);
    if (wide) hipLaunchKernelGGL(k_hash_crc<1>, grid, dim3(64), 0, g_stream, pics, list, n_list, state);
    else hipLaunchKernelGGL(k_hash_crc<0>, grid, dim3(64), 0, g_stream, pics, list, n_list, state);
  } else if (kind == RBT_HASH_CHECKSUM) {
    const dim3 grid((unsigned)max_h, planes);
    if (wide) hipLaunchKernelGGL(k_hash_sum<1>, grid, dim3(256), 0, g_stream, pics, list, n_list, state);
    else hipLaunchKernelGGL(k_hash_sum<0>, grid, dim3(256), 0, g_stream, pics, list, n_list, state);
  }
}
void launch_hash_finish(const RbtHashPic* pics, int n, const uint32_t* state, uint8_t* out, uint32_t* counters) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_hash_finish, dim3((unsigned)(n + 63) / 64), dim3(64), 0, g_stream, pics, n, state, out, counters);
}
}  // namespace rbtk
