// k_pack on a CPU: the walk, slots and sums of yustack_amd/csrc/yucsum_iov.h and
// the destination geometry of yucsum_iov_pack.h, driven here exactly as the
// kernel drives them (steps of U = 4 slots, 64 lanes of 16 bytes, each lane's
// previous source dword taken from its neighbour, lane 0's from lane 63 of the
// slot before), against the concatenated bytes and the scalar library's
// composition over them.
//
// Each packet is packed into an exact-size heap block with 0xA5 canaries on both
// sides; a store is counted per byte, so a byte stored twice, a slack byte or a
// canary touched, a store outside the block or a misaligned store is a failure
// (and, for the block's ends, a report under AddressSanitizer). Sources sit in
// exact-size heap blocks rounded out to whole dwords, as in iov_combine.cpp.
//
// Packets of 0..64 and 1020..1030 bytes (the slot seam); random, all 0x00 and all
// 0xFF; split into 1..3 views, empty ones included; every source address mod 4 x
// every destination start mod 16 (all 16 shifts, both parities); the six modes;
// fill on and off; slack 0 and 5. One view takes the whole cross product; two
// views take every cut (the long lengths: the cuts next to both ends and the
// seam) with every first-view alignment x destination start, three views every
// cut pair of the short lengths, the rest cycling. Then: 70 one-byte views, room
// one byte short, room 0, decreasing offsets, a span cut by dst_offsets[n], and a
// view that does not fit under 65535 bytes.
#include "iov_model.h"
#include "yucsum_iov_pack.h"

namespace {

constexpr int kU = 4;
constexpr size_t kCanary = 32;

// One packet as k_pack<4, *, FILL> handles it: its value; the copy goes through st.
// dst: the call's dst pointer; (o0, o1, oN): dst_offsets[i], [i + 1], [n].
uint32_t kernel_pack(Store &st, const std::vector<View> &views, int mode, bool fill, bool have_addrs, uint32_t a,
                     uint32_t b, uint32_t initial, uint64_t dst, uint64_t o0, uint64_t o1, uint64_t oN) {
  const uint32_t f = yu::iov_mode_field(mode);
  const bool tx = yu::iov_mode_tx(mode);
  const yu::IovPackDst D = {dst + o0, yu::iov_pack_room(o0, o1, oN)};
  yu::IovWalk W;
  yu::iov_walk_reset(W);
  size_t vi = 0;
  int32_t vpk = 0;
  uint32_t A = 0, B = 0, jA = 0, jB = 0, cprev = 0, fb0 = 0, fb1 = 0;
  uint64_t fa0 = 0, fa1 = 0;
  auto next_view = [&] {
    while (yu::iov_walk_done(W) && vi < views.size()) {
      const uint64_t l = views[vi].len;
      vpk = yu::iov_pack_view(views[vi].addr, W.off);
      yu::iov_walk_view(W, views[vi].addr, l < 0xFFFFFFFFull ? l : 0xFFFFFFFFull, tx, f);
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
    if (last) bad = W.over | (W.off > D.room ? 1u : 0u);
    for (int u = 0; u < kU; ++u) {
      const uint32_t info = S[u].info, lim = yu::iov_lim(info), hm = yu::iov_head_mask(info);
      if (lim == 0) continue;
      const bool swap = (info & yu::kIovSwap) != 0;
      uint32_t c[64][4];
      uint32_t t = 0;
      for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t cr = 16u * lane + 4u * j;
          c[lane][j] = 16u * lane < lim ? load_dword(S[u], cr, lim) : 0u;  // the other lanes load nothing
          t = yu::iov_add(yu::iov_dword(c[lane][j], cr, lim, hm), t);
        }
      yu::IovPackPlan P[64];
      for (uint32_t lane = 0; lane < 64; ++lane)
        yu::iov_pack_plan(P[lane], info, D, pk0[u] + (int32_t)(16u * lane), lane);
      int32_t fq[2] = {-1, -1};
      for (int k = 0; k < 2; ++k)
        if (yu::iov_has_field(info, k)) {
          const uint32_t q = yu::iov_field_q(info, k);
          const uint32_t word = c[q >> 4][(q >> 2) & 3u];
          (swap ? jA : jB) += yu::iov_field_term(word, q);
          const bool held = yu::iov_pack_field_held(P[63], q, 63);
          for (uint32_t lane = 0; lane < 64; ++lane)  // the same answer in every lane
            if (yu::iov_pack_field_held(P[lane], q, lane) != held) st.bad = true;
          const uint32_t byte = (word >> (8u * (q & 3u))) & 0xFFu;
          fq[k] = held ? (int32_t)q : -1;
          if (k == 0) {
            if (held) fa0 = yu::iov_pack_field_addr(P[63], q, 63);
            fb0 = byte;
          } else {
            if (held) fa1 = yu::iov_pack_field_addr(P[63], q, 63);
            fb1 = byte;
          }
        }
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t prev = lane ? c[lane - 1][3] : cprev;
        yu::iov_pack_lane(st, P[lane], lane, c[lane][0], c[lane][1], c[lane][2], c[lane][3], prev, fq[0], fq[1]);
      }
      cprev = c[63][3];
      (swap ? A : B) += t;
    }
  }
  const uint32_t len = W.off;
  const bool fld = tx && len >= f + 2u;
  if (fld) {
    A -= jA;
    B -= jB;
  }
  const uint32_t r = yu::iov_value(mode, yu::iov_residue(A, B), len, have_addrs, a, b, initial);
  if (tx) {
    const bool put = fill && fld && !bad;
    yu::iov_pack_field_store(st, fa0, fa1, put ? r >> 8 : fb0, put ? r & 0xFFu : fb1);
  }
  return r;
}

const int kModes[6] = {YU_MODE_RAW, YU_MODE_UDP, YU_MODE_TCP, YU_MODE_ICMP, YU_MODE_VERIFY_TCP,
                       YU_MODE_VERIFY_UDP};

struct Case {
  int mode;
  bool fill;
  uint32_t dalign;  // dst + dst_offsets[i] mod 16
  uint32_t slack;
  uint16_t initial;
  bool have_addrs;
  // out of contract: the packet's span is [0, span) of the block's room bytes
  // (span < 0: in contract, span = len + slack)
  int64_t span = -1;
  bool decreasing = false, cut_by_end = false;
};

// Packs the views (their concatenation: pkt[0, len)) and checks everything.
void run(const uint8_t *pkt, uint32_t len, const std::vector<View> &views, const Case &c, const uint8_t *rec,
         const char *what) {
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
  uint32_t a, b;
  memcpy(&a, rec, 4);
  memcpy(&b, rec + 4, 4);
  const uint32_t got = kernel_pack(st, views, c.mode, c.fill, c.have_addrs, a, b, c.initial, dst, o0, o1, oN);
  ++checks;
  bool ok = !st.bad;
  const uint32_t f = yu::iov_mode_field(c.mode);
  if (contract) {
    const uint32_t want = scalar_value(pkt, len, c.mode, c.have_addrs, rec, c.initial);
    ok = ok && got == want;
    std::vector<uint8_t> img(pkt, pkt + len);
    if (c.fill && yu::iov_mode_tx(c.mode) && len >= f + 2u) {
      img[f] = (uint8_t)(want >> 8);
      img[f + 1] = (uint8_t)want;
    }
    ok = ok && (len == 0 || memcmp(st.blk + at, img.data(), len) == 0);
    for (size_t i = 0; i < len; ++i) ok = ok && st.cnt[at + i] == 1;  // every byte by exactly one store
    for (size_t i = at + len; i < at + inner; ++i) ok = ok && st.cnt[i] == 0 && st.blk[i] == 0xA5;  // slack
  } else {
    // only inside the span, no byte twice
    for (size_t i = 0; i < inner; ++i) {
      ok = ok && st.cnt[at + i] <= 1;
      if (i >= room) ok = ok && st.cnt[at + i] == 0 && st.blk[at + i] == 0xA5;
    }
  }
  for (size_t i = 0; i < at; ++i) ok = ok && st.cnt[i] == 0 && st.blk[i] == 0xA5;
  for (size_t i = at + inner; i < st.total; ++i) ok = ok && st.cnt[i] == 0 && st.blk[i] == 0xA5;
  if (!ok) {
    fprintf(stderr, "%s: len %u views %zu (", what, len, views.size());
    for (auto &v : views) fprintf(stderr, " %llu@%u", (unsigned long long)v.len, (unsigned)(v.addr & 3u));
    fprintf(stderr, " ) mode %d fill %d dalign %u slack %u span %lld dec %d cut %d: value %04x, store-bad %d\n", c.mode,
            (int)c.fill, c.dalign, c.slack, (long long)c.span, (int)c.decreasing, (int)c.cut_by_end, got, (int)st.bad);
    if (++fails > 10) exit(1);
  }
  free(st.blk);
}

void check(const uint8_t *pkt, uint32_t len, const uint32_t *cut, int nv, uint32_t aligns, const Case &c,
           const uint8_t *rec) {
  std::vector<View> views;
  for (int i = 0; i < nv; ++i) views.push_back(place(pkt + cut[i], cut[i + 1] - cut[i], (aligns >> (2 * i)) & 3u));
  run(pkt, len, views, c, rec, "mismatch");
  for (auto &v : views) free(v.blk);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261020);
  uint8_t rec[8];
  uint64_t cyc = 0;
  // the case a cycling check takes: everything but what its loop fixes
  auto cycled = [&](uint32_t dalign) {
    Case c;
    c.mode = kModes[(cyc / 3) % 6];
    c.fill = yu::iov_mode_tx(c.mode) && ((cyc / 5) & 1);
    c.dalign = dalign;
    c.slack = ((cyc / 11) & 1) ? 5 : 0;
    c.initial = ((cyc / 7) & 1) ? 0xFFFF : 0;
    c.have_addrs = ((cyc / 13) & 1) != 0;
    ++cyc;
    return c;
  };
  std::vector<uint32_t> lens;
  for (uint32_t l = 0; l <= 64; ++l) lens.push_back(l);
  for (uint32_t l = 1020; l <= 1030; ++l) lens.push_back(l);
  for (uint32_t len : lens) {
    const bool lng = len > 64;
    for (int kind = 0; kind < 3; ++kind) {  // random, all 0x00, all 0xFF
      std::vector<uint8_t> pkt(len + 1);
      for (auto &x : pkt) x = kind == 0 ? (uint8_t)rng() : (kind == 1 ? 0x00 : 0xFF);
      for (auto &x : rec) x = kind == 0 ? (uint8_t)rng() : (kind == 1 ? 0x00 : 0xFF);
      uint32_t cut[4] = {0, len, len, len};
      // one view: source mod 4 x destination mod 16 x mode x fill x slack
      for (uint32_t sa = 0; sa < 4; ++sa)
        for (uint32_t da = 0; da < 16; ++da)
          for (int m = 0; m < 6; ++m)
            for (int fill = 0; fill <= (yu::iov_mode_tx(kModes[m]) ? 1 : 0); ++fill)
              for (uint32_t slack : {0u, 5u}) {
                Case c;
                c.mode = kModes[m], c.fill = fill != 0, c.dalign = da, c.slack = slack;
                c.initial = (uint16_t)(sa * 0x5555u), c.have_addrs = (da & 1) != 0;
                check(pkt.data(), len, cut, 1, sa, c, rec);
              }
      // the cuts taken: all of a short packet, of a long one those next to both ends and the seam
      std::vector<uint32_t> cuts;
      for (uint32_t x = 0; x <= len; ++x)
        if (!lng || x <= 4 || x + 4 >= len || (x >= 1019 && x <= 1026)) cuts.push_back(x);
      // two views: every cut, first view's address mod 4 x destination mod 16
      for (uint32_t c1 : cuts)
        for (uint32_t sa = 0; sa < 4; ++sa)
          for (uint32_t da = 0; da < 16; ++da) {
            cut[1] = c1, cut[2] = len;
            const Case c = cycled(da);
            check(pkt.data(), len, cut, 2, sa | ((uint32_t)(cyc % 4) << 2), c, rec);
          }
      // three views: every cut pair (a long packet: kind 0 only), alignments and destination cycling
      if (lng && kind != 0) continue;
      for (uint32_t c1 : cuts)
        for (uint32_t c2 : cuts) {
          if (c2 < c1) continue;
          cut[1] = c1, cut[2] = c2, cut[3] = len;
          for (int r = 0; r < (lng ? 1 : 2); ++r) {
            const Case c = cycled((uint32_t)((cyc / 17) % 16));
            check(pkt.data(), len, cut, 3, (uint32_t)(cyc % 64), c, rec);
          }
        }
    }
  }
  // past one step and one slot: random packets up to 9000 bytes and the limit, 3 views
  for (int it = 0; it < 48; ++it) {
    static const uint32_t kEdge[4] = {2047, 2048, 2049, 65535};
    const uint32_t len = it < 4 ? kEdge[it] : (uint32_t)(rng() % 9001);
    std::vector<uint8_t> pkt(len + 1);
    for (auto &x : pkt) x = (uint8_t)rng();
    for (auto &x : rec) x = (uint8_t)rng();
    uint32_t cut[4] = {0, (uint32_t)(rng() % (len + 1)), (uint32_t)(rng() % (len + 1)), len};
    if (cut[1] > cut[2]) std::swap(cut[1], cut[2]);
    for (int m = 0; m < 6; ++m) check(pkt.data(), len, cut, 3, (uint32_t)rng() & 63u, cycled((uint32_t)rng() & 15u), rec);
  }
  // one packet of 70 one-byte views, every destination start
  {
    std::vector<uint8_t> pkt(71);
    for (auto &x : pkt) x = (uint8_t)rng();
    std::vector<View> views;
    for (uint32_t i = 0; i < 70; ++i) views.push_back(place(&pkt[i], 1, (uint32_t)rng() & 3u));
    for (uint32_t da = 0; da < 16; ++da)
      for (int m = 0; m < 6; ++m) {
        Case c = cycled(da);
        c.mode = kModes[m];
        c.fill = yu::iov_mode_tx(c.mode) && (da & 1);
        run(pkt.data(), 70, views, c, rec, "70 views");
      }
    for (auto &v : views) free(v.blk);
  }
  // out of contract: room one byte short, room 0, decreasing offsets, a span that
  // dst_offsets[n] cuts; nothing outside the span, nothing twice
  for (uint32_t len : {1u, 7u, 8u, 18u, 21u, 64u, 1024u, 1029u, 3000u})
    for (uint32_t da = 0; da < 16; ++da)
      for (int m = 0; m < 6; ++m)
        for (int how = 0; how < 5; ++how) {
          std::vector<uint8_t> pkt(len + 1);
          for (auto &x : pkt) x = (uint8_t)rng();
          uint32_t cut[4] = {0, (uint32_t)(rng() % (len + 1)), len, len};
          Case c = cycled(da);
          c.mode = kModes[m];
          c.fill = yu::iov_mode_tx(c.mode);
          c.slack = 0;
          if (how == 0) c.span = len - 1;
          if (how == 1) c.span = 0;
          if (how == 2) c.decreasing = true;
          if (how == 3) c.cut_by_end = true, c.span = len / 2;
          if (how == 4) c.span = len > 17 ? 17 : len - 1;  // the room ends between TCP's two field bytes
          check(pkt.data(), len, cut, 2, (uint32_t)rng() & 15u, c, rec);
        }
  // a view that does not fit under the limit: what fits is stored once, nothing past the room
  {
    std::vector<uint8_t> pkt(70000);
    for (auto &x : pkt) x = (uint8_t)rng();
    std::vector<View> views = {place(pkt.data(), 40000, 1), place(pkt.data() + 40000, 30000, 2)};
    for (int m = 0; m < 6; ++m) {
      Case c = cycled(3);
      c.mode = kModes[m];
      c.fill = yu::iov_mode_tx(c.mode);
      c.slack = 0;
      c.span = yu::kIovLimit;
      run(pkt.data(), yu::kIovLimit, views, c, rec, "over the limit");
    }
    views.push_back({nullptr, 0x1000, 1ull << 40});  // never read: the limit is reached
    Case c = cycled(5);
    c.slack = 0, c.span = 100;
    run(pkt.data(), yu::kIovLimit, views, c, rec, "over the limit, small room");
    free(views[0].blk);
    free(views[1].blk);
  }
  return finish();
}
