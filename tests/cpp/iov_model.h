// What the CPU models of the wave-per-packet kernels share (iov_combine.cpp,
// iov_datagram.cpp, iov_pack.cpp, iov_pack_datagram.cpp, tx_build.cpp,
// rx_split.cpp): source views in exact-size heap blocks, the dword a buffer load
// returns, the destination block that counts its stores, the model of
// range_walk (the single-range walk of k_build and k_split), the scalar
// compositions the kernels are held against, the datagram generator, and the
// counters with the last line every program prints. Each program keeps its own
// transcription of the rest of its kernel's step and its own case loops.
#ifndef YU_TESTS_IOV_MODEL_H
#define YU_TESTS_IOV_MODEL_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "yucsum.h"
#include "yucsum_iov.h"
#include "yucsum_iov_pack.h"

inline int fails = 0;
inline uint64_t checks = 0;

// The program's last line and exit status.
inline int finish() {
  if (fails) return 1;
  printf("%llu packets ok\n", (unsigned long long)checks);
  return 0;
}

struct View {
  uint8_t *blk;   // heap block: the dwords holding the view
  uint64_t addr;  // the view's first byte
  uint64_t len;
};

// A view of `len` bytes at an address congruent to `a` mod 4 (malloc returns
// 16-aligned blocks), in an exact-size block rounded out to whole dwords: what
// the kernel's descriptors allow it to read, so under AddressSanitizer a read
// past it is a report. Empty views get a NULL base when a == 0.
inline View place(const uint8_t *src, uint32_t len, uint32_t a) {
  View v;
  v.len = len;
  if (len == 0) {
    v.blk = nullptr;
    v.addr = a ? 0x1000u + a : 0;  // never dereferenced
    return v;
  }
  const size_t sz = (a + len + 3u) & ~(size_t)3;
  v.blk = (uint8_t *)malloc(sz);
  memset(v.blk, 0xA5, sz);  // what surrounds a view is not zero
  memcpy(v.blk + a, src, len);
  v.addr = (uint64_t)(uintptr_t)v.blk + a;
  return v;
}

// The dword the kernel's buffer load returns at slot offset cr of a slot with
// `lim` window bytes: inside the descriptor's ceil4(lim) bytes memory, else 0.
inline uint32_t load_dword(const yu::IovSlot &S, uint32_t cr, uint32_t lim) {
  if (cr >= ((lim + 3u) & ~3u)) return 0;
  uint32_t x;
  memcpy(&x, (const void *)(uintptr_t)(S.base + cr), 4);
  return x;
}

// The destination block and the stores made into it.
struct Store {
  uint8_t *blk;
  size_t total;
  std::vector<uint8_t> cnt;
  bool bad = false;  // outside the block, or misaligned
  void put(uint64_t a, uint8_t v) {
    const uint64_t i = a - (uint64_t)(uintptr_t)blk;
    if (i >= total) {
      bad = true;
      return;
    }
    blk[i] = v;
    if (cnt[i] < 255) ++cnt[i];
  }
  void b8(uint64_t a, uint8_t v) { put(a, v); }
  void b16(uint64_t a, uint16_t v) {
    if (a & 1u) bad = true;
    put(a, (uint8_t)v);
    put(a + 1, (uint8_t)(v >> 8));
  }
  void b32(uint64_t a, uint32_t v) {
    if (a & 3u) bad = true;
    for (int k = 0; k < 4; ++k) put(a + k, (uint8_t)(v >> (8 * k)));
  }
  void b128(uint64_t a, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
    b32(a, x);
    b32(a + 4, y);
    b32(a + 8, z);
    b32(a + 12, w);
  }
};

// range_walk<4, *> of yucsum_kernels.hip as k_build and k_split drive it: W is on
// the packet's one range and vpk taken from it; steps of U = 4 slots, 64 lanes of
// 4 dwords, each lane's previous source dword taken from its neighbour, lane 0's
// from lane 63 of the slot before, every byte stored through st with nothing
// held back. A, B: the two class sums (swapped, plain).
inline void range_walk(yu::IovWalk &W, int32_t vpk, const yu::IovPackDst &D, Store &st, uint32_t &A, uint32_t &B) {
  constexpr int kU = 4;
  uint32_t cprev = 0;
  A = B = 0;
  while (!yu::iov_walk_done(W)) {
    yu::IovSlot S[kU];
    int32_t pk0[kU];
    for (int u = 0; u < kU; ++u) {
      pk0[u] = yu::iov_pack_po(vpk, W.w, 0);
      yu::iov_walk_slot(W, S[u]);
    }
    for (int u = 0; u < kU; ++u) {
      const uint32_t info = S[u].info, lim = yu::iov_lim(info), hm = yu::iov_head_mask(info);
      if (lim == 0) continue;
      uint32_t c[64][4];
      uint32_t t = 0;
      for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t cr = 16u * lane + 4u * j;
          c[lane][j] = 16u * lane < lim ? load_dword(S[u], cr, lim) : 0u;  // the other lanes load nothing
          t = yu::iov_add(yu::iov_dword(c[lane][j], cr, lim, hm), t);
        }
      for (uint32_t lane = 0; lane < 64; ++lane) {
        yu::IovPackPlan P;
        yu::iov_pack_plan(P, info, D, pk0[u] + (int32_t)(16u * lane), lane);
        const uint32_t prev = lane ? c[lane - 1][3] : cprev;
        yu::iov_pack_lane(st, P, lane, c[lane][0], c[lane][1], c[lane][2], c[lane][3], prev, -1, -1);
      }
      cprev = c[63][3];
      ((info & yu::kIovSwap) ? A : B) += t;
    }
  }
}

// The whole-packet modes: the scalar composition over the concatenated bytes
// (include/yucsum.h modes).
inline uint32_t scalar_value(const uint8_t *pkt, uint32_t len, int mode, bool have_addrs, const uint8_t *rec,
                             uint16_t initial) {
  if (mode == YU_MODE_RAW) return yu_checksum(pkt, len, initial);
  std::vector<uint8_t> z(pkt, pkt + len);
  const uint32_t f = yu::iov_mode_field(mode);
  if (yu::iov_mode_tx(mode) && len >= f + 2u) z[f] = z[f + 1] = 0;
  uint16_t x = 0;
  if (mode != YU_MODE_ICMP) {
    const uint32_t proto = (mode == YU_MODE_TCP || mode == YU_MODE_VERIFY_TCP) ? 6 : 17;
    x = have_addrs ? yu_pseudo_header_checksum(proto, rec, 4, rec + 4, 4) : initial;
    const uint8_t lb[2] = {(uint8_t)(len >> 8), (uint8_t)len};
    x = yu_checksum(lb, 2, x);
  }
  x = yu_checksum(z.data(), len, x);
  return yu::iov_mode_tx(mode) ? (uint16_t)~x : x;
}

// The whole-datagram modes: the byte-wise composition over the concatenated
// bytes (include/yucsum.h: the modes' definitions; the fill rule of
// yu_csum_fill_ragged). field[k]: the packet offset of field k's first byte, -1
// when it is not stored.
inline void scalar_value(const uint8_t *p, uint32_t len, int mode, uint32_t r[2], int field[2]) {
  r[0] = r[1] = 0;
  field[0] = field[1] = -1;
  const uint32_t hl = len ? (p[0] & 15u) * 4u : 0u;
  if (mode == YU_MODE_VERIFY_IPV4) {
    r[0] = yu_checksum(p, hl < len ? hl : len, 0);
    return;
  }
  if (mode == YU_MODE_IPV4) {
    uint8_t h[64] = {0};
    const uint32_t cp = len < 64u ? len : 64u;
    memcpy(h, p, cp);
    if (cp >= 12) h[10] = h[11] = 0;
    r[0] = (uint16_t)~yu_checksum(h, hl < cp ? hl : cp, 0);
    if ((hl < len ? hl : len) >= 12) field[0] = 10;
    return;
  }
  const uint32_t tl = len >= 4 ? ((uint32_t)p[2] << 8) | p[3] : 0u;
  const bool valid = len >= 20 && hl <= tl && tl <= len;
  if (mode == YU_MODE_VERIFY_RX) {
    if (!valid) {
      r[0] = YU_RX_INVALID;
      return;
    }
    const uint16_t x = yu_checksum(p, hl, 0);
    if (x == 0 || x == 0xFFFF) r[0] |= YU_RX_IP_OK;
    const uint32_t proto = p[9], sl = tl - hl;
    if (proto == 6 || proto == 17 || proto == 1) {
      r[0] |= YU_RX_L4;
      uint16_t xs = 0;
      if (proto != 1) {
        xs = yu_pseudo_header_checksum(proto, p + 12, 4, p + 16, 4);
        const uint8_t lb[2] = {(uint8_t)(sl >> 8), (uint8_t)sl};
        xs = yu_checksum(lb, 2, xs);
      }
      xs = yu_checksum(p + hl, sl, xs);
      if (xs == 0 || xs == 0xFFFF) r[0] |= YU_RX_L4_OK;
    }
    return;
  }
  // TX_DATAGRAM
  if (!valid || hl < 20) return;
  {
    uint8_t h[64] = {0};
    memcpy(h, p, hl);
    h[10] = h[11] = 0;
    r[0] = (uint16_t)~yu_checksum(h, hl, 0);
    field[0] = 10;
  }
  const uint32_t proto = p[9], sl = tl - hl;
  const uint32_t fo = proto == 17 ? 6u : (proto == 6 ? 16u : (proto == 1 ? 2u : 0u));
  const uint32_t mn = proto == 17 ? 8u : (proto == 6 ? 20u : 4u);
  if (!fo || sl < mn) return;
  std::vector<uint8_t> z(p + hl, p + tl);
  z[fo] = z[fo + 1] = 0;
  uint16_t xs = 0;
  if (proto != 1) {
    xs = yu_pseudo_header_checksum(proto, p + 12, 4, p + 16, 4);
    const uint8_t lb[2] = {(uint8_t)(sl >> 8), (uint8_t)sl};
    xs = yu_checksum(lb, 2, xs);
  }
  r[1] = (uint16_t)~yu_checksum(z.data(), sl, xs);
  field[1] = (int)(hl + fo);
}

// A datagram of len bytes: payload kind 0 random, 1 all 0x00, 2 all 0xFF, then
// the header fields where the packet holds them.
inline std::vector<uint8_t> datagram(std::mt19937_64 &rng, uint32_t len, int kind, uint32_t ihl, uint32_t tl,
                                     uint32_t proto) {
  std::vector<uint8_t> p(len + 1);
  for (auto &x : p) x = kind == 0 ? (uint8_t)rng() : (kind == 1 ? 0x00 : 0xFF);
  if (len > 0) p[0] = (uint8_t)(0x40u | ihl);
  if (len > 3) p[2] = (uint8_t)(tl >> 8), p[3] = (uint8_t)tl;
  if (len > 9) p[9] = (uint8_t)proto;
  return p;
}

#endif  // YU_TESTS_IOV_MODEL_H
