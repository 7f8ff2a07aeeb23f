// The whole-datagram kind of k_iov (yustack_amd/csrc/yucsum_iov.h, IPV4 /
// VERIFY_IPV4 / VERIFY_RX / TX_DATAGRAM on scatter-gather packets) on a CPU: the
// header gather (lane j takes packet byte j from the view that holds it), the
// parse, the header and pseudo-header sums over the lanes, the walk with the
// window [HL, TL), the load slots, the two classes, the field bytes and the
// epilogue, driven here exactly as the kernel drives them, against a byte-wise
// composition with the scalar library over the concatenated bytes.
//
// Datagrams of 0..96 bytes: IHL 0..15, TotalLength from HL - 1 to len + 1,
// protocols 1, 6, 17 and 47, payloads random, all 0x00 and all 0xFF. Lengths up
// to 40 take every split into 1..4 views (empty views included), the header
// fields cycling over the splits; every (length, IHL, TotalLength, protocol,
// payload) also takes splits that cycle, at every address mod 4. Views sit in
// exact-size heap blocks rounded out to whole dwords (what the kernel's
// descriptors allow it to read), so under AddressSanitizer a read past them is
// a report. TCP segments inside valid datagrams carry DataOffset 5, the one
// input condition YU_MODE_TCP makes.
#include "iov_model.h"

namespace {

constexpr int kU = 4;

struct Result {
  uint32_t r[2];
  bool st[2];
  uint64_t at[2][2];  // addresses of the two bytes of the IPv4 field / the transport field
};

// The datagram's results as the dg kind of k_iov computes them.
Result kernel_value(const std::vector<View> &views, int mode) {
  // the gather: views in order until they hold kIovHdr bytes
  uint64_t ga[64] = {0}, a0 = 0;
  uint32_t off = 0;
  for (size_t k = 0; off < yu::kIovHdr && k < views.size(); ++k) {
    const uint32_t l = views[k].len < 0x10000u ? views[k].len : 0x10000u;
    if (off == 0) a0 = views[k].addr;
    for (uint32_t lane = 0; lane < 64; ++lane)
      if (lane - off < l) ga[lane] = views[k].addr + (lane - off);
    off += l;
  }
  const uint32_t have = off < yu::kIovHdr ? off : yu::kIovHdr;
  uint32_t hb[64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    if (lane >= have) ga[lane] = a0;  // idle lanes load byte 0 again
    hb[lane] = have ? *(const uint8_t *)(uintptr_t)ga[lane] : 0u;
  }
  yu::IovDg D;
  yu::iov_dg_parse(D, mode, have, hb[0], hb[2], hb[3], hb[9]);
  uint32_t hs = 0, ps = 0;
  for (uint32_t lane = 0; lane < 64; ++lane) {
    hs += yu::iov_dg_hdr_term(D.meta, mode, lane, hb[lane]);
    ps += yu::iov_dg_pseudo_term(lane, hb[lane]);
  }
  // the walk with the window
  yu::IovWalk W;
  yu::iov_walk_reset(W);
  size_t vi = 0;
  uint32_t A = 0, B = 0, jA = 0, jB = 0;
  auto next_view = [&] {
    while (yu::iov_walk_done(W) && vi < views.size()) {
      yu::iov_walk_view_win(W, views[vi].addr, views[vi].len, D.lo, D.hi, D.f != 0u, D.f);
      ++vi;
    }
  };
  for (bool last = false; !last;) {
    yu::IovSlot S[kU];
    for (int u = 0; u < kU; ++u) {
      next_view();
      yu::iov_walk_slot(W, S[u]);
    }
    next_view();
    last = yu::iov_walk_done(W) && vi >= views.size();
    for (int u = 0; u < kU; ++u) {
      const uint32_t info = S[u].info, lim = yu::iov_lim(info), hm = yu::iov_head_mask(info);
      const bool swap = (info & yu::kIovSwap) != 0;
      uint32_t t = 0;
      for (uint32_t lane = 0; lane < 64 && 16u * lane < lim; ++lane)  // the other lanes load nothing
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t cr = 16u * lane + 4u * j;
          t = yu::iov_add(yu::iov_dword(load_dword(S[u], cr, lim), cr, lim, hm), t);
        }
      for (int k = 0; k < 2; ++k)
        if (yu::iov_has_field(info, k)) {
          const uint32_t q = yu::iov_field_q(info, k);
          const uint32_t term = yu::iov_field_term(load_dword(S[u], q & ~3u, lim), q);
          (swap ? jA : jB) += term;
        }
      (swap ? A : B) += t;
    }
  }
  Result R;
  yu::iov_dg_value(D, mode, W.off, hs, ps, A - jA, B - jB, R.r[0], R.r[1], R.st[0], R.st[1]);
  R.at[0][0] = ga[10];
  R.at[0][1] = ga[11];
  R.at[1][0] = W.fp[0];
  R.at[1][1] = W.fp[1];
  return R;
}

const int kModes[4] = {YU_MODE_IPV4, YU_MODE_VERIFY_IPV4, YU_MODE_VERIFY_RX, YU_MODE_TX_DATAGRAM};

void check(const uint8_t *pkt, uint32_t len, const uint32_t *cut, int nv, uint32_t aligns, int mode) {
  std::vector<View> views;
  for (int i = 0; i < nv; ++i)
    views.push_back(place(pkt + cut[i], cut[i + 1] - cut[i], (aligns >> (2 * i)) & 3u));
  const Result R = kernel_value(views, mode);
  uint32_t want[2];
  int field[2];
  scalar_value(pkt, len, mode, want, field);
  ++checks;
  bool ok = R.r[0] == want[0] && R.r[1] == want[1];
  for (int k = 0; k < 2; ++k) {
    ok = ok && R.st[k] == (field[k] >= 0);
    if (field[k] < 0) continue;
    for (uint32_t b = 0; b < 2; ++b) {  // the bytes the fill form stores to
      const uint32_t at = (uint32_t)field[k] + b;
      uint64_t want_p = 0;
      for (int i = 0; i < nv; ++i)
        if (at >= cut[i] && at < cut[i + 1]) want_p = views[i].addr + (at - cut[i]);
      ok = ok && R.at[k][b] == want_p;
    }
  }
  if (!ok) {
    fprintf(stderr,
            "mismatch: len %u b0 %02x tl %u proto %u views %d cuts %u %u %u aligns %02x mode %d: %04x %04x want %04x %04x"
            " (stores %d %d want %d %d)\n",
            len, len ? pkt[0] : 0, len >= 4 ? (pkt[2] << 8) | pkt[3] : 0, len >= 10 ? pkt[9] : 0, nv, cut[1], cut[2],
            cut[3], aligns, mode, R.r[0], R.r[1], want[0], want[1], (int)R.st[0], (int)R.st[1], field[0] >= 0,
            field[1] >= 0);
    if (++fails > 10) exit(1);
  }
  for (auto &v : views) free(v.blk);
}

// iov_model.h's datagram; a TCP segment inside a valid one carries DataOffset 5.
std::vector<uint8_t> datagram5(std::mt19937_64 &rng, uint32_t len, int kind, uint32_t ihl, uint32_t tl, uint32_t proto) {
  std::vector<uint8_t> p = datagram(rng, len, kind, ihl, tl, proto);
  const uint32_t hl = 4 * ihl;
  if (proto == 6 && len >= 20 && hl >= 20 && hl <= tl && tl <= len && tl - hl >= 20) p[hl + 12] = 0x50;
  return p;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261020);
  static const uint32_t kProto[4] = {1, 6, 17, 47};
  uint64_t cyc = 0;
  // every split of the lengths up to 40, the header fields and modes cycling
  for (uint32_t len = 0; len <= 40; ++len)
    for (int nv = 1; nv <= 4; ++nv) {
      uint32_t cut[5] = {0, len, len, len, len};
      for (uint32_t c1 = 0; c1 <= (nv >= 2 ? len : 0); ++c1)
        for (uint32_t c2 = c1; c2 <= (nv >= 3 ? len : c1); ++c2)
          for (uint32_t c3 = c2; c3 <= (nv >= 4 ? len : c2); ++c3) {
            if (nv >= 2) cut[1] = c1;
            if (nv >= 3) cut[2] = c2;
            if (nv >= 4) cut[3] = c3;
            cut[nv] = len;
            const uint32_t reps = nv <= 2 ? 64 : (nv == 3 ? 8 : 4);
            for (uint32_t r = 0; r < reps; ++r, ++cyc) {
              // mostly headers that lie inside the packet, so that the window opens
              const uint32_t ihl = (cyc % 5 == 0) ? (uint32_t)(cyc / 5 % 16) : 5u + (uint32_t)(cyc / 5 % 2);
              const uint32_t hl = 4 * ihl;
              const uint32_t span = len + 3 > hl ? len + 3 - hl : 1;  // TL in HL - 1 .. len + 1
              const uint32_t tl = (hl + (uint32_t)(cyc / 7 % span) + 65535u) % 65536u;
              const auto p = datagram5(rng, len, (int)(cyc / 3 % 3), ihl, (cyc % 11 == 0) ? len : tl, kProto[cyc / 2 % 4]);
              check(p.data(), len, cut, nv, nv <= 2 ? r % 16 : (uint32_t)rng() & 0xFF, kModes[cyc % 4]);
            }
          }
    }
  // every (length, IHL, TotalLength, protocol, payload), the splits and alignments cycling
  for (uint32_t len = 0; len <= 96; ++len)
    for (uint32_t ihl = 0; ihl <= 15; ++ihl)
      for (uint32_t tl = ihl ? 4 * ihl - 1 : 0; tl <= len + 1; ++tl)
        for (int pi = 0; pi < 4; ++pi)
          for (int kind = 0; kind < 3; ++kind, ++cyc) {
            const auto p = datagram5(rng, len, kind, ihl, tl, kProto[pi]);
            const int nv = 1 + (int)(cyc % 4);
            uint32_t c[3] = {(uint32_t)(rng() % (len + 1)), (uint32_t)(rng() % (len + 1)), (uint32_t)(rng() % (len + 1))};
            if (cyc % 3 == 0) c[0] = (uint32_t)(rng() % ((len < 24 ? len : 24) + 1));  // a cut inside the header
            if (c[0] > c[1]) std::swap(c[0], c[1]);
            if (c[1] > c[2]) std::swap(c[1], c[2]);
            if (c[0] > c[1]) std::swap(c[0], c[1]);
            uint32_t cut[5] = {0, len, len, len, len};
            for (int i = 1; i < nv; ++i) cut[i] = c[i - 1 + (3 - (nv - 1))];
            cut[nv] = len;
            for (int m = 0; m < 4; ++m) check(p.data(), len, cut, nv, (uint32_t)(cyc * 4 + m) & 0xFF, kModes[m]);
          }
  // past one slot and one step, the limit, and one-byte views through the header
  for (int it = 0; it < 80; ++it) {
    static const uint32_t kSeg[8] = {1023, 1024, 1025, 4095, 4096, 4097, 9000, 65535 - 24};
    const uint32_t ihl = it < 8 ? 6u : 5u + it % 11;
    const uint32_t seg = it < 8 ? kSeg[it] : (uint32_t)(rng() % 9001);
    const uint32_t tl = 4 * ihl + seg, len = tl + (it % 3 == 0 || tl == 65535u ? 0 : (uint32_t)(rng() % 40));
    const auto p = datagram5(rng, len, 0, ihl, tl, kProto[it % 3]);
    uint32_t c[3] = {(uint32_t)(rng() % (len + 1)), (uint32_t)(rng() % (len + 1)), (uint32_t)(rng() % (len + 1))};
    if (c[0] > c[1]) std::swap(c[0], c[1]);
    if (c[1] > c[2]) std::swap(c[1], c[2]);
    if (c[0] > c[1]) std::swap(c[0], c[1]);
    uint32_t cut[5] = {0, c[0], c[1], c[2], len};
    for (int m = 0; m < 4; ++m) check(p.data(), len, cut, 4, (uint32_t)rng() & 0xFF, kModes[m]);
  }
  for (uint32_t proto : kProto) {  // 80 one-byte views, then the rest; 70 empty views first
    const auto p = datagram5(rng, 200, 0, 15, 200, proto);
    for (int m = 0; m < 4; ++m) {
      std::vector<View> v1, v2;
      for (uint32_t i = 0; i < 80; ++i) v1.push_back(place(p.data() + i, 1, i & 3u));
      v1.push_back(place(p.data() + 80, 120, 1));
      for (uint32_t i = 0; i < 70; ++i) v2.push_back(place(p.data(), 0, i & 3u));
      v2.push_back(place(p.data(), 9, 3));
      v2.push_back(place(p.data() + 9, 191, 2));
      uint32_t want[2];
      int field[2];
      scalar_value(p.data(), 200, kModes[m], want, field);
      for (auto *vs : {&v1, &v2}) {
        const Result R = kernel_value(*vs, kModes[m]);
        ++checks;
        if (R.r[0] != want[0] || R.r[1] != want[1] || R.st[0] != (field[0] >= 0) || R.st[1] != (field[1] >= 0)) {
          fprintf(stderr, "many views: proto %u mode %d: %04x %04x want %04x %04x\n", proto, kModes[m], R.r[0], R.r[1],
                  want[0], want[1]);
          ++fails;
        }
        for (auto &v : *vs) free(v.blk);
      }
    }
  }
  // a view that does not fit under the limit: the window takes what lies under it
  {
    std::vector<uint8_t> pkt(70000, 0x5A);
    yu::IovWalk W;
    yu::iov_walk_reset(W);
    yu::iov_walk_view_win(W, (uint64_t)(uintptr_t)pkt.data(), 40000, 20, 65535, false, 0);
    if (W.off != 40000u || W.over || W.E != ((uint32_t)((uintptr_t)pkt.data() + 20u) & 3u) + 39980u) ++fails;
    W.w = W.E;
    yu::iov_walk_view_win(W, (uint64_t)(uintptr_t)pkt.data() + 40000, 30000, 20, 65535, false, 0);
    if (W.off != yu::kIovLimit || !W.over) ++fails;
    W.w = W.E;
    yu::iov_walk_view_win(W, (uint64_t)(uintptr_t)pkt.data(), 1ull << 40, 20, 65535, false, 0);
    if (W.off != yu::kIovLimit || !yu::iov_walk_done(W)) ++fails;
  }
  return finish();
}
