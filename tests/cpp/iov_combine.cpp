// k_iov's arithmetic (yustack_amd/csrc/yucsum_iov.h) on a CPU: the walk over a
// packet's views, the load slots, the masked little-endian sums, the two
// classes, the field bytes and the epilogue, driven here exactly as the kernel
// drives them (steps of U slots, 64 lanes of 16 bytes), against the scalar
// library's composition over the concatenated bytes.
//
// Packets of 0..64 bytes (random, all 0x00, all 0xFF), every split into 1..4
// views (empty views included), every view at every address mod 4, initial 0 and
// 0xFFFF, pseudo header from `initial` and from an address record. Splits into up
// to 3 views of lengths up to 8 and of the lengths around each TX field take every
// combination; the other splits cycle through the alignments, modes and initial
// values, so every (length, mode) still sees thousands of splits. Views sit in exact-size heap
// blocks rounded out to whole dwords (what the kernel's descriptors allow it to
// read), so under AddressSanitizer a read past them is a report.
#include "iov_model.h"

namespace {

constexpr int kU = 4;

// The packet's value as k_iov computes it.
uint32_t kernel_value(const std::vector<View> &views, int mode, bool have_addrs, uint32_t a, uint32_t b,
                      uint32_t initial, uint64_t fp[2]) {
  const uint32_t f = yu::iov_mode_field(mode);
  const bool tx = yu::iov_mode_tx(mode);
  yu::IovWalk W;
  yu::iov_walk_reset(W);
  size_t vi = 0;
  uint32_t A = 0, B = 0, jA = 0, jB = 0;
  auto next_view = [&] {
    while (yu::iov_walk_done(W) && vi < views.size()) {
      yu::iov_walk_view(W, views[vi].addr, views[vi].len, tx, f);
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
  const uint32_t len = W.off;
  if (tx && len >= f + 2u) {
    A -= jA;
    B -= jB;
  }
  fp[0] = W.fp[0];
  fp[1] = W.fp[1];
  return yu::iov_value(mode, yu::iov_residue(A, B), len, have_addrs, a, b, initial);
}

const int kModes[6] = {YU_MODE_RAW, YU_MODE_UDP, YU_MODE_TCP, YU_MODE_ICMP, YU_MODE_VERIFY_TCP,
                       YU_MODE_VERIFY_UDP};

void check(const uint8_t *pkt, uint32_t len, const uint32_t *cut, int nv, uint32_t aligns, int mode,
           uint16_t initial, bool have_addrs, const uint8_t *rec) {
  std::vector<View> views;
  for (int i = 0; i < nv; ++i)
    views.push_back(place(pkt + cut[i], cut[i + 1] - cut[i], (aligns >> (2 * i)) & 3u));
  uint32_t a, b;
  memcpy(&a, rec, 4);
  memcpy(&b, rec + 4, 4);
  uint64_t fp[2];
  const uint32_t got = kernel_value(views, mode, have_addrs, a, b, initial, fp);
  const uint32_t want = scalar_value(pkt, len, mode, have_addrs, rec, initial);
  ++checks;
  bool ok = got == want;
  // the field bytes the fill form would store to
  const uint32_t f = yu::iov_mode_field(mode);
  if (yu::iov_mode_tx(mode) && len >= f + 2u)
    for (uint32_t k = 0; k < 2; ++k) {
      uint64_t want_p = 0;
      for (int i = 0; i < nv; ++i)
        if (f + k >= cut[i] && f + k < cut[i + 1]) want_p = views[i].addr + (f + k - cut[i]);
      ok = ok && fp[k] == want_p;
    }
  if (!ok) {
    fprintf(stderr, "mismatch: len %u views %d cuts %u %u %u aligns %02x mode %d initial %04x addrs %d: %04x want %04x\n",
            len, nv, cut[1], cut[2], cut[3], aligns, mode, initial, (int)have_addrs, got, want);
    if (++fails > 10) exit(1);
  }
  for (auto &v : views) free(v.blk);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261019);
  uint8_t rec[8];
  uint64_t cyc = 0;
  for (uint32_t len = 0; len <= 64; ++len) {
    for (int kind = 0; kind < 3; ++kind) {  // random, all 0x00, all 0xFF
      std::vector<uint8_t> pkt(len + 1);
      for (auto &x : pkt) x = kind == 0 ? (uint8_t)rng() : (kind == 1 ? 0x00 : 0xFF);
      for (auto &x : rec) x = kind == 0 ? (uint8_t)rng() : (kind == 1 ? 0x00 : 0xFF);
      bool every = len <= 8;  // every alignment x mode x initial
      for (int m : {YU_MODE_UDP, YU_MODE_TCP, YU_MODE_ICMP}) {
        const uint32_t f = yu::iov_mode_field(m);
        every = every || (kind == 0 && (len == f + 2 || len == f + 3));
      }
      for (int nv = 1; nv <= 4; ++nv) {
        uint32_t cut[5] = {0, len, len, len, len};
        // cut points c1 <= c2 <= c3 in [0, len]; views past nv are not used
        for (uint32_t c1 = 0; c1 <= (nv >= 2 ? len : 0); ++c1)
          for (uint32_t c2 = c1; c2 <= (nv >= 3 ? len : c1); ++c2)
            for (uint32_t c3 = c2; c3 <= (nv >= 4 ? len : c2); ++c3) {
              if (nv >= 2) cut[1] = c1;
              if (nv >= 3) cut[2] = c2;
              if (nv >= 4) cut[3] = c3;
              cut[nv] = len;
              const uint32_t combos = 1u << (2 * nv);
              if (every && nv <= 3) {
                for (uint32_t al = 0; al < combos; ++al)
                  for (int m = 0; m < 6; ++m)
                    for (int iv = 0; iv < 4; ++iv)
                      check(pkt.data(), len, cut, nv, al, kModes[m], (iv & 1) ? 0xFFFF : 0, (iv & 2) != 0, rec);
              } else {
                // one combination per split, cycling (4-view splits of the lengths above:
                // four); 2-view splits: every alignment pair
                const uint32_t reps = nv == 2 ? 16 : (every ? 4 : 1);
                for (uint32_t r = 0; r < reps; ++r, ++cyc) {
                  const uint32_t al = nv == 2 ? r : (uint32_t)(cyc % combos);
                  const int m = kModes[(cyc / 3) % 6];
                  const int iv = (int)((cyc / 7) % 4);
                  check(pkt.data(), len, cut, nv, al, m, (iv & 1) ? 0xFFFF : 0, (iv & 2) != 0, rec);
                }
              }
            }
      }
    }
  }
  // past one slot and one step: long views, many views, the limit
  for (int it = 0; it < 60; ++it) {
    static const uint32_t kEdge[4] = {1023, 1024, 1025, 65535};
    const uint32_t len = it < 4 ? kEdge[it] : (uint32_t)(rng() % 9001);
    std::vector<uint8_t> pkt(len + 1);
    for (auto &x : pkt) x = (uint8_t)rng();
    for (auto &x : rec) x = (uint8_t)rng();
    uint32_t cut[5] = {0, 0, 0, 0, len};
    uint32_t c[3] = {(uint32_t)(rng() % (len + 1)), (uint32_t)(rng() % (len + 1)), (uint32_t)(rng() % (len + 1))};
    if (c[0] > c[1]) std::swap(c[0], c[1]);
    if (c[1] > c[2]) std::swap(c[1], c[2]);
    if (c[0] > c[1]) std::swap(c[0], c[1]);
    cut[1] = c[0], cut[2] = c[1], cut[3] = c[2];
    for (int m = 0; m < 6; ++m)
      check(pkt.data(), len, cut, 4, (uint32_t)rng() & 0xFF, kModes[m], (uint16_t)rng(), (it & 1) != 0, rec);
  }
  // a view that does not fit under the limit: its bytes past it are not taken
  {
    std::vector<uint8_t> pkt(70000, 0x5A);
    yu::IovWalk W;
    yu::iov_walk_reset(W);
    yu::iov_walk_view(W, (uint64_t)(uintptr_t)pkt.data(), 40000, false, 0);
    W.w = W.E;
    yu::iov_walk_view(W, (uint64_t)(uintptr_t)pkt.data() + 40000, 30000, false, 0);
    const uint32_t s2 = (uint32_t)(((uintptr_t)pkt.data() + 40000u) & 3u);
    if (W.off != yu::kIovLimit || !W.over || W.E != s2 + 25535u) {
      fprintf(stderr, "limit: off %u over %u E %u\n", W.off, W.over, W.E);
      ++fails;
    }
    W.w = W.E;
    yu::iov_walk_view(W, (uint64_t)(uintptr_t)pkt.data(), 1ull << 40, false, 0);
    if (W.off != yu::kIovLimit || !yu::iov_walk_done(W)) ++fails;
  }
  return finish();
}
