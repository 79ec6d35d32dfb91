// Decoded picture hashes (H.265 D.3.19, decoded_picture_hash SEI): MD5, CRC and checksum of the three planes of pictures that are already
// in device memory, optionally compared with the hashes a stream carries. What is hashed is the whole coded picture (conformance window
// included), plane by plane, in raster order: one byte per sample at bit depth 8, two bytes (low byte first) above.
//   MD5       one serial chain per plane (RFC 1321): one plane per lane, the next 64-byte block loaded while the current one is hashed
//             (rbt_hash.hip k_hash_md5).
//   CRC       CRC-16, polynomial x^16 + x^12 + x^5 + 1 (0x1021), register 0xFFFF, two zero bytes appended. The register after a message of L
//             bytes is R = 0xFFFF * x^(8L + 16) + M(x) * x^16 mod P, which is linear in the message: every lane takes a segment, its remainder
//             is moved into place by x^(8 * bytes behind the segment) mod P and the segments are combined by XOR (k_hash_crc).
//   checksum  sum mod 2^32 of (byte ^ xorMask), xorMask = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8): a reduction (k_hash_sum).
// Results: per picture 48 bytes in SEI byte order, 16 per component (MD5: the digest; CRC: 2 bytes, checksum: 4 bytes, most significant
// first, zero-padded), plus a mismatch count per counter index for the pictures that come with an expected hash.
//
// The kernel bodies below are shared with the serial host emulation (RBT_HOSTEMU, tests/hostemu): there the launchers at the end of
// this file run them as plain loops.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "rbt_platform.h"
#include "../../include/rbt.h"

// one picture to hash: planar 4:2:0 (w x h luma, w/2 x h/2 chroma), every plane 16-byte aligned
struct RbtHashPic {
  const uint16_t* plane[3];
  int32_t w, h, bit_depth;
  int32_t kind;              // RBT_HASH_MD5 / RBT_HASH_CRC / RBT_HASH_CHECKSUM
  int32_t counter;           // >= 0: compare with `want`, a mismatch counts in counters[counter]; < 0: nothing to compare
  uint8_t want[48];          // expected hash, SEI byte order, 16 bytes per component (zero-padded)
  int32_t pad;
};
// per picture: 3 planes x 4 words of hash state (MD5: A, B, C, D; CRC, checksum: word 0); zeroed before a launch
enum { RBT_HASH_STATE_WORDS = 12, RBT_CRC_SEG = 1024 };   // RBT_CRC_SEG: bytes of the message per lane of k_hash_crc (a multiple of 16)
enum { RBT_HASH_MAX_PICS = 16384 };                        // pictures of one launch (3 planes each: grid dimension y)

namespace rbtk {
// One launch per (kind, wide) class of pictures: list = device array of the indices (into pics) of the pictures of that kind whose
// bit depth is > 8 (wide) or 8; max_luma = the largest w * h among them, max_h = the largest h. state: RBT_HASH_STATE_WORDS words per
// picture of pics, zeroed beforehand.
void launch_hash(const RbtHashPic* pics, const int32_t* list, int n_list, int kind, int wide, int max_luma, int max_h, uint32_t* state);
// the 48 result bytes of every picture from its state, and the comparison with the expected hash
void launch_hash_finish(const RbtHashPic* pics, int n, const uint32_t* state, uint8_t* out, uint32_t* counters);
}  // namespace rbtk

// ------------------------------------------------------------------------------------------------ bodies (device and host emulation)
// byte j of a plane's message
RBT_DEV uint32_t rbt_hash_byte(const uint16_t* p, size_t j, int wide) {
  if (!wide) return p[j] & 0xFFu;
  const uint32_t s = p[j >> 1];
  return (j & 1) ? (s >> 8) & 0xFFu : s & 0xFFu;
}
RBT_DEV size_t rbt_hash_plane_bytes(int w, int h, int wide) { return (size_t)w * (size_t)h * (wide ? 2 : 1); }

RBT_DEV uint32_t rbt_rotl32(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }
// one 64-byte block of MD5 (RFC 1321 3.4)
RBT_DEV void rbt_md5_block(uint32_t st[4], const uint32_t M[16]) {
  constexpr uint32_t K[64] = {
      0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u, 0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu,
      0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u, 0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
      0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au, 0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu,
      0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u, 0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
      0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u, 0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u,
      0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
  constexpr int S[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};
  uint32_t A = st[0], B = st[1], C = st[2], D = st[3];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    uint32_t F; int g;
    if (i < 16) { F = (B & C) | (~B & D); g = i; }
    else if (i < 32) { F = (D & B) | (~D & C); g = (5 * i + 1) & 15; }
    else if (i < 48) { F = B ^ C ^ D; g = (3 * i + 5) & 15; }
    else { F = C ^ (B | ~D); g = (7 * i) & 15; }
    F = F + A + K[i] + M[g];
    A = D; D = C; C = B; B = B + rbt_rotl32(F, S[(i >> 4) * 4 + (i & 3)]);
  }
  st[0] += A; st[1] += B; st[2] += C; st[3] += D;
}
RBT_DEV void rbt_md5_init(uint32_t st[4]) { st[0] = 0x67452301u; st[1] = 0xefcdab89u; st[2] = 0x98badcfeu; st[3] = 0x10325476u; }
// the blocks of a plane from block `first` on that hold the message's tail, the 0x80 byte, the padding and the length (built byte by byte)
RBT_DEV void rbt_md5_tail(uint32_t st[4], const uint16_t* p, size_t L, int wide, size_t first) {
  const size_t n_blocks = (L + 8) / 64 + 1;   // message + 0x80 + 8 length bytes, rounded up to whole blocks
  const uint64_t bits = (uint64_t)L * 8;
  for (size_t k = first; k < n_blocks; k++) {
    uint32_t M[16];
    for (int i = 0; i < 16; i++) {
      uint32_t v = 0;
      for (int b = 0; b < 4; b++) {
        const size_t j = k * 64 + (size_t)(4 * i + b);
        uint32_t byte;
        if (j < L) byte = rbt_hash_byte(p, j, wide);
        else if (j == L) byte = 0x80u;
        else if (j >= n_blocks * 64 - 8) byte = (uint32_t)(bits >> (8 * (j - (n_blocks * 64 - 8)))) & 0xFFu;
        else byte = 0;
        v |= byte << (8 * b);
      }
      M[i] = v;
    }
    rbt_md5_block(st, M);
  }
}

// CRC-16 (0x1021) over GF(2): (a * b) mod P for remainders a, b < 2^16
RBT_DEV uint32_t rbt_crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 15; i >= 0; i--) {
    r <<= 1;
    if (r & 0x10000u) r ^= 0x11021u;
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}
// x^e mod P
RBT_DEV uint32_t rbt_crc_xpow(uint64_t e) {
  uint32_t r = 1, b = 2;
  while (e) { if (e & 1) r = rbt_crc_mulmod(r, b); b = rbt_crc_mulmod(b, b); e >>= 1; }
  return r;
}
// the byte-wise table of the direct form: crc' = (crc << 8) ^ T[(crc >> 8) ^ byte] advances crc by one byte, crc = (bytes so far) * x^16 mod P
RBT_DEV uint32_t rbt_crc_table_entry(uint32_t v) {
  uint32_t r = v << 8;
  for (int i = 0; i < 8; i++) r = (r & 0x8000u) ? ((r << 1) ^ 0x1021u) & 0xFFFFu : (r << 1) & 0xFFFFu;
  return r;
}
// a lane's share of the register: (segment bytes [b0, b1) of the message) * x^16 * x^(8 * (L - b1)) mod P, plus the initial register's term for the first segment
RBT_DEV uint32_t rbt_crc_place(uint32_t seg_crc, size_t b0, size_t b1, size_t L) {
  uint32_t r = rbt_crc_mulmod(seg_crc, rbt_crc_xpow((uint64_t)(L - b1) * 8));
  if (b0 == 0) r ^= rbt_crc_mulmod(0xFFFFu, rbt_crc_xpow((uint64_t)L * 8 + 16));
  return r;
}

// checksum of one row of a plane (D.3.19: picture_checksum)
RBT_DEV uint32_t rbt_sum_sample(uint32_t s, int x, int y, int wide) {
  const uint32_t m = (uint32_t)((x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8));
  uint32_t v = (s & 0xFFu) ^ m;
  if (wide) v += ((s >> 8) & 0xFFu) ^ m;
  return v;
}

// the 48 result bytes of a picture from its state words; returns 1 if it has an expected hash that differs
RBT_DEV int rbt_hash_finish_pic(const RbtHashPic& P, const uint32_t* st, uint8_t* out) {
  int bad = 0;
  for (int c = 0; c < 3; c++) {
    uint8_t b[16];
    for (int i = 0; i < 16; i++) b[i] = 0;
    const uint32_t* s = st + 4 * c;
    if (P.kind == RBT_HASH_MD5) { for (int i = 0; i < 16; i++) b[i] = (uint8_t)(s[i >> 2] >> (8 * (i & 3))); }
    else if (P.kind == RBT_HASH_CRC) { b[0] = (uint8_t)(s[0] >> 8); b[1] = (uint8_t)s[0]; }
    else { b[0] = (uint8_t)(s[0] >> 24); b[1] = (uint8_t)(s[0] >> 16); b[2] = (uint8_t)(s[0] >> 8); b[3] = (uint8_t)s[0]; }
    for (int i = 0; i < 16; i++) { out[16 * c + i] = b[i]; bad |= b[i] != P.want[16 * c + i]; }
  }
  return P.counter >= 0 && bad;
}

#ifdef RBT_HOSTEMU
// serial stand-ins of the launchers (the product's are in rbt_hash.hip)
namespace rbtk {
inline void launch_hash(const RbtHashPic* pics, const int32_t* list, int n_list, int kind, int wide, int, int, uint32_t* state) {
  for (int q = 0; q < n_list; q++) for (int c = 0; c < 3; c++) {
    const RbtHashPic& P = pics[list[q]];
    const int pw = c ? P.w / 2 : P.w, ph = c ? P.h / 2 : P.h;
    const uint16_t* p = P.plane[c]; uint32_t* st = state + (size_t)list[q] * RBT_HASH_STATE_WORDS + 4 * c;
    const size_t L = rbt_hash_plane_bytes(pw, ph, wide);
    if (kind == RBT_HASH_MD5) { rbt_md5_init(st); rbt_md5_tail(st, p, L, wide, 0); }
    else if (kind == RBT_HASH_CRC) {
      uint32_t T[256]; for (uint32_t v = 0; v < 256; v++) T[v] = rbt_crc_table_entry(v);
      uint32_t r = 0;
      for (size_t b0 = 0; b0 < L; b0 += RBT_CRC_SEG) {
        const size_t b1 = b0 + RBT_CRC_SEG < L ? b0 + RBT_CRC_SEG : L; uint32_t crc = 0;
        for (size_t j = b0; j < b1; j++) crc = ((crc << 8) ^ T[((crc >> 8) ^ rbt_hash_byte(p, j, wide)) & 0xFFu]) & 0xFFFFu;
        r ^= rbt_crc_place(crc, b0, b1, L);
      }
      if (L == 0) r = rbt_crc_mulmod(0xFFFFu, rbt_crc_xpow(16));
      st[0] = r;
    } else {
      uint32_t s = 0;
      for (int y = 0; y < ph; y++) for (int x = 0; x < pw; x++) s += rbt_sum_sample(p[(size_t)y * pw + x], x, y, wide);
      st[0] = s;
    }
  }
}
inline void launch_hash_finish(const RbtHashPic* pics, int n, const uint32_t* state, uint8_t* out, uint32_t* counters) {
  for (int i = 0; i < n; i++) if (rbt_hash_finish_pic(pics[i], state + (size_t)i * RBT_HASH_STATE_WORDS, out + (size_t)i * 48)) counters[pics[i].counter]++;
}
}  // namespace rbtk
#endif
