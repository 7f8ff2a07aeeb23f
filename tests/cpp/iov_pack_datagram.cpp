// k_pack_dg on a CPU: the header gather, the parse and the epilogue of the
// datagram kind (yustack_amd/csrc/yucsum_iov.h), the plain walk over whole views,
// the window applied to the sum by each slot's place in the packet, the
// destination geometry and the four held-back bytes (yucsum_iov_pack.h, last
// section), driven here exactly as the kernel drives them (steps of U = 4 slots,
// 64 lanes of 16 bytes, each lane's previous source dword taken from its
// neighbour, lane 0's from lane 63 of the slot before), against the concatenated
// bytes and the byte-wise scalar composition over them.
//
// The store side is iov_pack.cpp's: each packet is packed into an exact-size
// heap block with 0xA5 canaries on both sides and every store is counted per
// byte, so a byte stored twice, a slack byte or a canary touched, a store outside
// the block or a misaligned store is a failure. The copy is every byte of the
// packet whatever the parse says; in the fill form the fields
// yu_csum_fill_ragged stores have the value, every other byte is as read.
//
// Datagrams of 0..96 bytes x IHL 0..15 x TL from HL - 1 to len + 1 x protocols
// 1, 6, 17, 47 x payloads random, all 0x00 and all 0xFF, in 1..4 views (empty
// ones included) at every source address mod 4 and every destination start mod
// 16, slack 0 and 5, the four modes, fill on and off; every split of the short
// lengths; lengths 1020..1030 with HL, TL and a view cut next to the 1024-byte
// slot seam; 70 empty or one-byte views before the header; room one byte short,
// room 0, decreasing offsets, a span cut by dst_offsets[n], and a view over
// 65535 bytes.
#include "iov_model.h"
#include "yucsum_iov_pack.h"

namespace {

constexpr int kU = 4;
constexpr size_t kCanary = 32;

// One packet as k_pack_dg<4, *, FILL> handles it: its results; the copy goes
// through st. dst: the call's dst pointer; (o0, o1, oN): dst_offsets[i], [i + 1], [n].
void kernel_pack_dg(Store &st, const std::vector<View> &views, int mode, bool fill, uint64_t dst, uint64_t o0,
                    uint64_t o1, uint64_t oN, uint32_t r[2]) {
  const yu::IovPackDst Dd = {dst + o0, yu::iov_pack_room(o0, o1, oN)};
  // the gather: views in order until they hold kIovHdr bytes
  uint64_t ga[64] = {0}, a0 = 0;
  uint32_t goff = 0;
  for (size_t k = 0; goff < yu::kIovHdr && k < views.size(); ++k) {
    const uint32_t l = views[k].len < 0x10000u ? (uint32_t)views[k].len : 0x10000u;
    if (goff == 0) a0 = views[k].addr;
    for (uint32_t lane = 0; lane < 64; ++lane)
      if (lane - goff < l) ga[lane] = views[k].addr + (lane - goff);
    goff += l;
  }
  const uint32_t have = goff < yu::kIovHdr ? goff : yu::kIovHdr;
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
  // the plain walk over whole views
  yu::IovWalk W;
  yu::iov_walk_reset(W);
  size_t vi = 0;
  int32_t vpk = 0;
  uint32_t A = 0, B = 0, jA = 0, jB = 0, cprev = 0, fb0 = 0, fb1 = 0;
  auto next_view = [&] {
    while (yu::iov_walk_done(W) && vi < views.size()) {
      const uint64_t l = views[vi].len;
      vpk = yu::iov_pack_view(views[vi].addr, W.off);
      yu::iov_walk_view(W, views[vi].addr, l < 0xFFFFFFFFull ? l : 0xFFFFFFFFull, D.f != 0u, D.f);
      ++vi;
    }
  };
  uint32_t bad = 0;
  for (bool last = false; !last;) {
    yu::IovSlot S[kU];
    int32_t pk0[kU];
    for (int u = 0; u < kU; ++u) {
      next_view();
      pk0[u] = yu::iov_pack_po(vpk, W.w, 0);
      yu::iov_walk_slot(W, S[u]);
    }
    next_view();
    last = yu::iov_walk_done(W) && vi >= views.size();
    if (last) bad = W.over | (W.off > Dd.room ? 1u : 0u);
    for (int u = 0; u < kU; ++u) {
      const uint32_t info = S[u].info, lim = yu::iov_lim(info), hm = yu::iov_head_mask(info);
      if (lim == 0) continue;
      const bool swap = (info & yu::kIovSwap) != 0;
      const int32_t p0 = pk0[u];
      const int span = yu::iov_pack_dg_span(info, p0, D.lo, D.hi);
      uint32_t c[64][4];
      uint32_t t = 0;
      for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t cr = 16u * lane + 4u * j;
          c[lane][j] = 16u * lane < lim ? load_dword(S[u], cr, lim) : 0u;  // the other lanes load nothing
          const uint32_t x = yu::iov_dword(c[lane][j], cr, lim, hm);
          if (span == 1) t = yu::iov_add(x, t);
          if (span == 2) t = yu::iov_add(x & yu::iov_win_mask(p0 + (int32_t)cr, D.lo, D.hi), t);
        }
      yu::IovPackPlan P[64];
      for (uint32_t lane = 0; lane < 64; ++lane)
        yu::iov_pack_plan(P[lane], info, Dd, p0 + (int32_t)(16u * lane), lane);
      int32_t fq[4] = {-1, -1, -1, -1};
      for (int k = 0; k < 2; ++k)
        if (yu::iov_has_field(info, k)) {
          const uint32_t q = yu::iov_field_q7(info, k);
          const uint32_t word = c[q >> 4][(q >> 2) & 3u];
          (swap ? jA : jB) += yu::iov_field_term(word, q);
          if (!fill) continue;
          const bool held = yu::iov_pack_field_held(P[63], q, 63);
          for (uint32_t lane = 0; lane < 64; ++lane)  // the same answer in every lane
            if (yu::iov_pack_field_held(P[lane], q, lane) != held) st.bad = true;
          fq[k] = held ? (int32_t)q : -1;
          (k == 0 ? fb0 : fb1) = (word >> (8u * (q & 3u))) & 0xFFu;
        }
      const bool four = fill && (info & yu::kIovFirst) && p0 <= 11;
      if (four)
        for (int k = 0; k < 2; ++k) {
          fq[2 + k] = yu::iov_pack_dg_held(P[63], info, p0, 10u + (uint32_t)k, 63);
          for (uint32_t lane = 0; lane < 64; ++lane)
            if (yu::iov_pack_dg_held(P[lane], info, p0, 10u + (uint32_t)k, lane) != fq[2 + k]) st.bad = true;
        }
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t prev = lane ? c[lane - 1][3] : cprev;
        if (four)
          yu::iov_pack_lane4(st, P[lane], lane, c[lane][0], c[lane][1], c[lane][2], c[lane][3], prev, fq[0], fq[1],
                             fq[2], fq[3]);
        else
          yu::iov_pack_lane(st, P[lane], lane, c[lane][0], c[lane][1], c[lane][2], c[lane][3], prev, fq[0], fq[1]);
      }
      cprev = c[63][3];
      (swap ? A : B) += t;
    }
  }
  const uint32_t len = W.off;
  bool st0, st1;
  yu::iov_dg_value(D, mode, len, hs, ps, A - jA, B - jB, r[0], r[1], st0, st1);
  if (fill) yu::iov_pack_dg_finish(st, Dd, len, D.f, !bad && st0, !bad && st1, r[0], r[1], hb[10], hb[11], fb0, fb1);
}

const int kModes[4] = {YU_MODE_IPV4, YU_MODE_VERIFY_IPV4, YU_MODE_VERIFY_RX, YU_MODE_TX_DATAGRAM};
bool mode_fills(int m) { return m == YU_MODE_IPV4 || m == YU_MODE_TX_DATAGRAM; }

struct Case {
  int mode;
  bool fill;
  uint32_t dalign;  // dst + dst_offsets[i] mod 16
  uint32_t slack;
  // out of contract: the packet's span is [0, span) of the block's room bytes
  // (span < 0: in contract, span = len + slack)
  int64_t span = -1;
  bool decreasing = false, cut_by_end = false;
};

// Packs the views (their concatenation: pkt[0, len)) and checks everything.
void run(const uint8_t *pkt, uint32_t len, const std::vector<View> &views, const Case &c, const char *what) {
  const bool contract = c.span < 0 && !c.decreasing && !c.cut_by_end && len <= yu::kIovLimit;
  const uint64_t want_room = c.span >= 0 ? (uint64_t)c.span : len + c.slack;
  const uint64_t room = c.decreasing ? 0 : want_room;  // bytes the call may store
  const size_t inner = (size_t)(len + c.slack);       // the block between the canaries
  Store st;
  st.total = kCanary + c.dalign + inner + kCanary;
  st.blk = (uint8_t *)malloc(st.total);
  memset(st.blk, 0xA5, st.total);
  st.cnt.assign(st.total, 0);
  const size_t at = kCanary + c.dalign;  // malloc's blocks are 16-aligned
  const uint64_t o0 = 1000;
  uint64_t o1 = o0 + want_room, oN = o1 + 64;
  if (c.decreasing) o1 = o0 - 1;
  if (c.cut_by_end) {  // dst_offsets[n] cuts the span short
    oN = o0 + want_room;
    o1 = oN + 7;
  }
  const uint64_t dst = (uint64_t)(uintptr_t)st.blk + at - o0;
  uint32_t got[2];
  kernel_pack_dg(st, views, c.mode, c.fill, dst, o0, o1, oN, got);
  ++checks;
  bool ok = !st.bad;
  uint32_t want[2] = {0, 0};
  if (contract) {
    int field[2];
    scalar_value(pkt, len, c.mode, want, field);
    ok = ok && got[0] == want[0] && got[1] == want[1];
    std::vector<uint8_t> img(pkt, pkt + len);
    if (c.fill)
      for (int k = 0; k < 2; ++k)
        if (field[k] >= 0) {
          img[field[k]] = (uint8_t)(want[k] >> 8);
          img[field[k] + 1] = (uint8_t)want[k];
        }
    ok = ok && (len == 0 || memcmp(st.blk + at, img.data(), len) == 0);
    for (size_t i = 0; i < len; ++i) ok = ok && st.cnt[at + i] == 1;  // every byte by exactly one store
    for (size_t i = at + len; i < at + inner; ++i) ok = ok && st.cnt[i] == 0 && st.blk[i] == 0xA5;  // slack
  } else {
    // only inside the span, no byte twice, and what is stored is the byte as read:
    // an out-of-contract packet gets no field value
    for (size_t i = 0; i < inner; ++i) {
      ok = ok && st.cnt[at + i] <= 1;
      if (i >= room) ok = ok && st.cnt[at + i] == 0 && st.blk[at + i] == 0xA5;
      if (st.cnt[at + i] == 1 && i < len) ok = ok && st.blk[at + i] == pkt[i];
    }
  }
  for (size_t i = 0; i < at; ++i) ok = ok && st.cnt[i] == 0 && st.blk[i] == 0xA5;
  for (size_t i = at + inner; i < st.total; ++i) ok = ok && st.cnt[i] == 0 && st.blk[i] == 0xA5;
  if (!ok) {
    fprintf(stderr, "%s: len %u b0 %02x tl %u proto %u views %zu (", what, len, len ? pkt[0] : 0,
            len >= 4 ? (pkt[2] << 8) | pkt[3] : 0, len >= 10 ? pkt[9] : 0, views.size());
    for (auto &v : views) fprintf(stderr, " %llu@%u", (unsigned long long)v.len, (unsigned)(v.addr & 3u));
    fprintf(stderr, " ) mode %d fill %d dalign %u slack %u span %lld dec %d cut %d: %04x %04x want %04x %04x, store-bad %d\n",
            c.mode, (int)c.fill, c.dalign, c.slack, (long long)c.span, (int)c.decreasing, (int)c.cut_by_end, got[0],
            got[1], want[0], want[1], (int)st.bad);
    if (++fails > 10) exit(1);
  }
  free(st.blk);
}

void check(const uint8_t *pkt, uint32_t len, const uint32_t *cut, int nv, uint32_t aligns, const Case &c) {
  std::vector<View> views;
  for (int i = 0; i < nv; ++i) views.push_back(place(pkt + cut[i], cut[i + 1] - cut[i], (aligns >> (2 * i)) & 3u));
  run(pkt, len, views, c, "mismatch");
  for (auto &v : views) free(v.blk);
}

void sort3(uint32_t *c) {
  if (c[0] > c[1]) std::swap(c[0], c[1]);
  if (c[1] > c[2]) std::swap(c[1], c[2]);
  if (c[0] > c[1]) std::swap(c[0], c[1]);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261020);
  static const uint32_t kProto[4] = {1, 6, 17, 47};
  uint64_t cyc = 0;
  // the case a cycling check takes: everything but what its loop fixes
  auto cycled = [&](int mode, uint32_t dalign) {
    Case c;
    c.mode = mode;
    c.fill = mode_fills(mode) && ((cyc / 5) & 1);
    c.dalign = dalign;
    c.slack = ((cyc / 11) & 1) ? 5 : 0;
    ++cyc;
    return c;
  };
  // every split of the lengths up to 40 into 1..3 views, the header fields, modes,
  // alignments and destination starts cycling
  for (uint32_t len = 0; len <= 40; ++len)
    for (int nv = 1; nv <= 3; ++nv) {
      uint32_t cut[5] = {0, len, len, len, len};
      for (uint32_t c1 = 0; c1 <= (nv >= 2 ? len : 0); ++c1)
        for (uint32_t c2 = c1; c2 <= (nv >= 3 ? len : c1); ++c2) {
          if (nv >= 2) cut[1] = c1;
          if (nv >= 3) cut[2] = c2;
          cut[nv] = len;
          const uint32_t reps = nv <= 2 ? 64 : 8;
          for (uint32_t r = 0; r < reps; ++r) {
            const uint32_t ihl = (cyc % 5 == 0) ? (uint32_t)(cyc / 5 % 16) : 5u + (uint32_t)(cyc / 5 % 2);
            const uint32_t hl = 4 * ihl;
            const uint32_t span = len + 3 > hl ? len + 3 - hl : 1;  // TL in HL - 1 .. len + 1
            const uint32_t tl = (hl + (uint32_t)(cyc / 7 % span) + 65535u) % 65536u;
            const auto p = datagram(rng, len, (int)(cyc / 3 % 3), ihl, (cyc % 11 == 0) ? len : tl, kProto[cyc / 2 % 4]);
            const Case c = cycled(kModes[cyc % 4], nv <= 2 ? r / 4 : (uint32_t)rng() & 15u);
            check(p.data(), len, cut, nv, nv <= 2 ? r % 16 : (uint32_t)rng() & 0xFF, c);
          }
        }
    }
  // every (length, IHL, TotalLength, protocol, payload) x mode x fill; the splits,
  // source alignments, destination starts and slack cycling
  for (uint32_t len = 0; len <= 96; ++len)
    for (uint32_t ihl = 0; ihl <= 15; ++ihl)
      for (uint32_t tl = ihl ? 4 * ihl - 1 : 0; tl <= len + 1; ++tl)
        for (int pi = 0; pi < 4; ++pi)
          for (int kind = 0; kind < 3; ++kind) {
            const auto p = datagram(rng, len, kind, ihl, tl, kProto[pi]);
            const int nv = 1 + (int)(cyc % 4);
            uint32_t c[3] = {(uint32_t)(rng() % (len + 1)), (uint32_t)(rng() % (len + 1)), (uint32_t)(rng() % (len + 1))};
            if (cyc % 3 == 0) c[0] = (uint32_t)(rng() % ((len < 24 ? len : 24) + 1));  // a cut inside the header
            sort3(c);
            uint32_t cut[5] = {0, len, len, len, len};
            for (int i = 1; i < nv; ++i) cut[i] = c[i - 1 + (3 - (nv - 1))];
            cut[nv] = len;
            for (int m = 0; m < 4; ++m)
              for (int fill = 0; fill <= (mode_fills(kModes[m]) ? 1 : 0); ++fill) {
                Case cs;
                cs.mode = kModes[m], cs.fill = fill != 0;
                cs.dalign = (uint32_t)(cyc % 16), cs.slack = (cyc / 16 % 2) ? 5 : 0;
                check(p.data(), len, cut, nv, (uint32_t)(cyc / 32) & 0xFF, cs);
                ++cyc;
              }
          }
  // every source address mod 4 x destination start mod 16 x slack x mode x fill: one
  // view, and header view + segment view
  for (uint32_t proto : kProto)
    for (uint32_t ihl : {5u, 6u, 15u})
      for (uint32_t seg : {0u, 3u, 8u, 21u}) {
        const uint32_t tl = 4 * ihl + seg, len = tl + (seg & 1u);
        const auto p = datagram(rng, len, 0, ihl, tl, proto);
        for (uint32_t sa = 0; sa < 16; ++sa)
          for (uint32_t da = 0; da < 16; ++da)
            for (int m = 0; m < 4; ++m)
              for (int fill = 0; fill <= (mode_fills(kModes[m]) ? 1 : 0); ++fill)
                for (uint32_t slack : {0u, 5u}) {
                  Case cs;
                  cs.mode = kModes[m], cs.fill = fill != 0, cs.dalign = da, cs.slack = slack;
                  uint32_t one[2] = {0, len}, two[3] = {0, 4 * ihl, len};
                  if (sa < 4) check(p.data(), len, one, 1, sa, cs);
                  check(p.data(), len, two, 2, sa, cs);
                }
      }
  // the 1024-byte slot seam: lengths 1020..1030, HL = 20, TL and a view cut next to
  // the seam (of the packet, and of the second view's own slots)
  for (uint32_t len = 1020; len <= 1030; ++len)
    for (uint32_t tl : {1019u, 1020u, 1021u, 1023u, 1024u, 1025u, 1027u, 1028u, 1029u, 1030u, 1031u}) {
      if (tl > len + 1) continue;
      for (uint32_t c1 : {0u, 1u, 19u, 20u, 21u, 1019u, 1020u, 1021u, 1023u, 1024u, 1025u, 1026u})
        for (int pi = 0; pi < 3; ++pi) {
          if (c1 > len) continue;
          const auto p = datagram(rng, len, (int)(cyc % 3), 5, tl, kProto[pi]);
          uint32_t cut[3] = {0, c1, len};
          for (uint32_t sa = 0; sa < 16; ++sa)
            for (int m = 2; m < 4; ++m) check(p.data(), len, cut, 2, sa, cycled(kModes[m], (uint32_t)(cyc / 3 % 16)));
        }
    }
  // a header view of HL bytes whose address puts HL (lo) at, before and after a slot
  // seam of the segment view; TL next to the segment view's second seam
  for (uint32_t seg : {1023u, 1024u, 1025u, 2047u, 2048u, 2049u, 2052u})
    for (uint32_t trail : {0u, 1u, 7u})
      for (uint32_t ihl : {5u, 15u})
        for (int pi = 0; pi < 3; ++pi) {
          const uint32_t tl = 4 * ihl + seg, len = tl + trail;
          const auto p = datagram(rng, len, 0, ihl, tl, kProto[pi]);
          for (uint32_t c1 : {4 * ihl - 1, 4 * ihl, 4 * ihl + 1, 4 * ihl + 1024u}) {
            if (c1 > len) continue;
            uint32_t cut[3] = {0, c1, len};
            for (uint32_t sa = 0; sa < 16; ++sa)
              for (int m = 2; m < 4; ++m) check(p.data(), len, cut, 2, sa, cycled(kModes[m], (uint32_t)(cyc / 3 % 16)));
          }
        }
  // past one step, the limit, 4 views
  for (int it = 0; it < 80; ++it) {
    static const uint32_t kSeg[8] = {1023, 1024, 1025, 4095, 4096, 4097, 9000, 65535 - 24};
    const uint32_t ihl = it < 8 ? 6u : 5u + it % 11;
    const uint32_t seg = it < 8 ? kSeg[it] : (uint32_t)(rng() % 9001);
    const uint32_t tl = 4 * ihl + seg, len = tl + (it % 3 == 0 || tl == 65535u ? 0 : (uint32_t)(rng() % 40));
    const auto p = datagram(rng, len, 0, ihl, tl, kProto[it % 3]);
    uint32_t c[3] = {(uint32_t)(rng() % (len + 1)), (uint32_t)(rng() % (len + 1)), (uint32_t)(rng() % (len + 1))};
    sort3(c);
    uint32_t cut[5] = {0, c[0], c[1], c[2], len};
    for (int m = 0; m < 4; ++m) check(p.data(), len, cut, 4, (uint32_t)rng() & 0xFF, cycled(kModes[m], (uint32_t)rng() & 15u));
  }
  // 80 one-byte views, then the rest; 70 empty views first: the header lies past the
  // 64 records the lanes hold
  for (uint32_t proto : kProto) {
    const auto p = datagram(rng, 200, 0, 15, 200, proto);
    for (uint32_t da = 0; da < 16; ++da)
      for (int m = 0; m < 4; ++m) {
        std::vector<View> v1, v2;
        for (uint32_t i = 0; i < 80; ++i) v1.push_back(place(p.data() + i, 1, (i + da) & 3u));
        v1.push_back(place(p.data() + 80, 120, 1));
        for (uint32_t i = 0; i < 70; ++i) v2.push_back(place(p.data(), 0, i & 3u));
        v2.push_back(place(p.data(), 9, 3));
        v2.push_back(place(p.data() + 9, 191, 2));
        Case c = cycled(kModes[m], da);
        c.fill = mode_fills(c.mode) && (da & 1);
        run(p.data(), 200, v1, c, "80 one-byte views");
        run(p.data(), 200, v2, c, "70 empty views");
        for (auto &v : v1) free(v.blk);
        for (auto &v : v2) free(v.blk);
      }
  }
  // out of contract: room one byte short, room 0, decreasing offsets, a span that
  // dst_offsets[n] cuts, a room that ends between the field's bytes; nothing outside
  // the span, nothing twice, no field value
  for (uint32_t seg : {0u, 7u, 8u, 20u, 64u, 1024u, 1029u, 3000u})
    for (uint32_t da = 0; da < 16; ++da)
      for (int m = 0; m < 4; ++m)
        for (int how = 0; how < 7; ++how) {
          const uint32_t len = 20 + seg;
          const auto p = datagram(rng, len, 0, 5, len, kProto[(da + how) % 3]);
          uint32_t cut[3] = {0, (uint32_t)(rng() % (len + 1)), len};
          Case c = cycled(kModes[m], da);
          c.fill = mode_fills(c.mode);
          c.slack = 0;
          if (how == 0) c.span = len - 1;
          if (how == 1) c.span = 0;
          if (how == 2) c.decreasing = true;
          if (how == 3) c.cut_by_end = true, c.span = len / 2;
          if (how == 4) c.span = 11;  // between bytes 10 and 11
          if (how == 5) c.span = len > 37 ? 37 : len - 1;  // between TCP's two field bytes
          if (how == 6) c.span = 10;
          check(p.data(), len, cut, 2, (uint32_t)rng() & 15u, c);
        }
  // a view that does not fit under the limit: what fits is stored once, nothing past the room
  {
    auto pkt = datagram(rng, 70000, 0, 5, 65535, 6);
    std::vector<View> views = {place(pkt.data(), 40000, 1), place(pkt.data() + 40000, 30000, 2)};
    for (int m = 0; m < 4; ++m) {
      Case c = cycled(kModes[m], 3);
      c.fill = mode_fills(c.mode);
      c.slack = 0;
      c.span = yu::kIovLimit;
      run(pkt.data(), yu::kIovLimit, views, c, "over the limit");
    }
    views.push_back({nullptr, 0x1000, 1ull << 40});  // never read: the limit is reached
    Case c = cycled(YU_MODE_TX_DATAGRAM, 5);
    c.fill = true, c.slack = 0, c.span = 100;
    run(pkt.data(), yu::kIovLimit, views, c, "over the limit, small room");
    free(views[0].blk);
    free(views[1].blk);
  }
  return finish();
}
