// k_build_iov ("k_build<4,iov>", yu_tx_build_iov) on a CPU: tests/cpp/tx_build.cpp's
// model of k_build fed from views, held byte for byte against that contiguous model.
// Both drive the same functions of yustack_amd/csrc (yucsum_build.h's header encode,
// sums and contract test, yucsum_iov.h's single-view walk, yucsum_iov_pack.h's
// destination geometry, iov_model.h's range_walk) exactly as the two kernels do; the
// iov form takes (addr, plen) from the packet's view as they stand and branches past a
// packet whose destination span is empty (build_iov_skipped) before anything of it is
// used.
//
// One batch is four entries with tight dst_offsets: a built packet, a skipped one whose
// view is an address that must not be dereferenced (it is no memory of this program:
// reading it is a fault, and a report under AddressSanitizer), a second built packet
// naming the SAME view as the first, and a skipped one with a {NULL, 0} view. The
// contiguous model builds the two packets from a payload block at the same byte phase
// into a block of its own at the same offsets; the two destination blocks, their store
// counts per byte (every byte of a datagram exactly once, nothing else at all) and the
// out pairs must be identical, and the skipped entries' out pairs {0, 0}.
//
// Payload byte phases 0..3 x destination byte phases 0..3 x L in {0..5, 1019..1025,
// 4091..4097, 65507 (UDP: T = 65535), 65508 (over the limit)} x UDP, ICMP, TCP and
// protocol 47.
#include "iov_model.h"
#include "yucsum_build.h"
#include "yucsum_iov_pack.h"

namespace {

constexpr size_t kCanary = 48;

struct Pair {
  uint16_t ipsum, xsum;  // what the kernel stores to out
};

// Everything after (addr, plen): shared by the two kernels.
Pair build_tail(Store &st, const yu::BuildRec &R, uint64_t addr, uint64_t plen, bool ranged, const yu::IovPackDst &D) {
  const uint32_t H = yu::build_l4_len(yu::build_proto(R));
  yu::IovWalk W;
  yu::iov_walk_reset(W);
  W.off = yu::kBuildIp + H;
  const int32_t vpk = yu::iov_pack_view(addr, W.off);
  yu::iov_walk_view(W, addr, plen, false, 0u);
  const uint32_t L = W.off - (yu::kBuildIp + H);
  uint32_t A, B;
  range_walk(W, vpk, D, st, A, B);
  uint32_t ipsum, xsum;
  yu::build_values(R, H, L, A, B, ipsum, xsum);
  uint32_t hw[64];
  for (uint32_t lane = 0; lane < 64; ++lane) hw[lane] = yu::build_hdr_src(R, H, L, ipsum, xsum, lane);
  yu::IovPackPlan P;
  yu::build_hdr_plan(P, D, H);
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t hprev = (lane & 15u) ? hw[lane - 1] : 0u;  // row_shr:1, a row's first lane gets 0
    const uint32_t m = lane < yu::kBuildHdrDwords ? yu::iov_pack_mask(P, lane) : 0u;
    if (m) yu::iov_pack_store(st, (P.pa & ~3ull) + 4u * lane, yu::build_hdr_dst(hw[lane], hprev, P.delta), m);
  }
  const bool ok = yu::build_in_contract(R, ranged, W.over != 0u, L, D.room);
  return {(uint16_t)(ok ? ipsum : 0u), (uint16_t)(ok ? xsum : 0u)};
}

// One packet as k_build<4, *> handles it (tests/cpp/tx_build.cpp's kernel_build).
Pair kernel_build(Store &st, uint64_t payload, uint64_t p0, uint64_t p1, uint64_t poN, const yu::BuildRec &R,
                  uint64_t dst, uint64_t o0, uint64_t o1, uint64_t oN) {
  const bool ranged = p0 <= p1 && p1 <= poN;
  const uint64_t pe = p1 < poN ? p1 : poN;
  const uint64_t plen = pe > p0 ? pe - p0 : 0;
  const uint64_t addr = payload + (plen ? p0 : 0);
  const yu::IovPackDst D = {dst + o0, yu::iov_pack_room(o0, o1, oN)};
  return build_tail(st, R, addr, plen, ranged, D);
}

// One packet as k_build_iov<4, *> handles it.
Pair kernel_build_iov(Store &st, const yu_iovec &view, const yu::BuildRec &R, uint64_t dst, uint64_t o0, uint64_t o1,
                      uint64_t oN) {
  if (yu::build_iov_skipped(o0, o1)) return {0, 0};
  const yu::IovPackDst D = {dst + o0, yu::iov_pack_room(o0, o1, oN)};
  return build_tail(st, R, (uint64_t)(uintptr_t)view.base, view.len, true, D);
}

yu::BuildRec random_rec(std::mt19937_64 &rng, uint8_t proto) {
  yu_tx_record t;
  uint8_t raw[32];
  for (auto &x : raw) x = (uint8_t)rng();
  memcpy(&t, raw, 32);
  t.proto = proto, t.doff = 20, t.reserved = 0;
  yu::BuildRec R;
  static_assert(sizeof t == sizeof R.w, "the record is eight dwords");
  memcpy(R.w, &t, sizeof t);
  return R;
}

Store make_store(size_t inner, uint32_t dalign) {
  Store st;
  st.total = kCanary + dalign + inner + kCanary;
  st.blk = (uint8_t *)malloc(st.total);
  memset(st.blk, 0xA5, st.total);
  st.cnt.assign(st.total, 0);
  return st;
}

void run(std::mt19937_64 &rng, const std::vector<uint8_t> &pay, uint32_t L, uint8_t proto, uint32_t palign,
         uint32_t dalign) {
  const uint32_t H = yu::build_l4_len(proto);
  const uint64_t T = 20ull + H + L;  // the span each built packet gets (65536 for the over-limit case)
  const yu::BuildRec R[4] = {random_rec(rng, proto), random_rec(rng, proto), random_rec(rng, proto),
                             random_rec(rng, proto)};
  // entry 0 and 2 built, 1 and 3 skipped; tight
  const uint64_t base_off = 1000;
  const uint64_t off[5] = {base_off, base_off + T, base_off + T, base_off + 2 * T, base_off + 2 * T};
  const size_t inner = (size_t)(2 * T);

  const View v = place(pay.data(), L, palign);
  const yu_iovec views[4] = {{(void *)(uintptr_t)v.addr, v.len},
                             {(void *)(uintptr_t)0x40u, 700},  // skipped: never dereferenced
                             {(void *)(uintptr_t)v.addr, v.len},  // the same view again
                             {nullptr, 0}};
  Store a = make_store(inner, dalign);
  const uint64_t adst = (uint64_t)(uintptr_t)a.blk + kCanary + dalign - base_off;
  Pair got[4];
  for (int i = 0; i < 4; ++i) got[i] = kernel_build_iov(a, views[i], R[i], adst, off[i], off[i + 1], off[4]);

  // the contiguous call over the two built packets: the payload twice, at the same phase
  const size_t psz = (palign + 2 * (size_t)L + 3u + 4u) & ~(size_t)3;
  uint8_t *pblk = (uint8_t *)malloc(psz);
  memset(pblk, 0xA5, psz);
  // the second copy starts at a multiple of 4 past the first, so both have phase palign
  const uint64_t second = ((uint64_t)L + 3u) & ~3ull;
  if (L) memcpy(pblk + palign, pay.data(), L), memcpy(pblk + palign + second, pay.data(), L);
  Store b = make_store(inner, dalign);
  const uint64_t bdst = (uint64_t)(uintptr_t)b.blk + kCanary + dalign - base_off;
  const uint64_t payload = (uint64_t)(uintptr_t)pblk + palign;
  const uint64_t po[3] = {0, L, second + L};
  Pair want[2];
  want[0] = kernel_build(b, payload, po[0], po[1], po[2], R[0], bdst, off[0], off[1], off[4]);
  want[1] = kernel_build(b, payload + second, 0, L, L, R[2], bdst, off[2], off[3], off[4]);
  checks += 4;

  bool ok = !a.bad && !b.bad && memcmp(a.blk, b.blk, a.total) == 0 && a.cnt == b.cnt;
  ok = ok && got[0].ipsum == want[0].ipsum && got[0].xsum == want[0].xsum;
  ok = ok && got[2].ipsum == want[1].ipsum && got[2].xsum == want[1].xsum;
  ok = ok && got[1].ipsum == 0 && got[1].xsum == 0 && got[3].ipsum == 0 && got[3].xsum == 0;
  const size_t at = kCanary + dalign;
  for (size_t i = 0; i < a.total; ++i) {
    const bool in = i >= at && i < at + inner;
    if (!in) ok = ok && a.cnt[i] == 0 && a.blk[i] == 0xA5;  // the guards: nothing outside the spans
    else if (T <= 65535) ok = ok && a.cnt[i] == 1;          // every byte of a datagram exactly once
    else ok = ok && a.cnt[i] <= 1;                          // over the limit: inside the span only
  }
  if (T > 65535) ok = ok && got[0].ipsum == 0 && got[0].xsum == 0 && got[2].ipsum == 0 && got[2].xsum == 0;
  if (!ok) {
    fprintf(stderr, "L %u proto %u palign %u dalign %u: iov {%04x %04x} {%04x %04x}, contiguous {%04x %04x} "
            "{%04x %04x}, store-bad %d %d\n", L, proto, palign, dalign, got[0].ipsum, got[0].xsum, got[2].ipsum,
            got[2].xsum, want[0].ipsum, want[0].xsum, want[1].ipsum, want[1].xsum, (int)a.bad, (int)b.bad);
    if (++fails > 10) exit(1);
  }
  free(a.blk);
  free(b.blk);
  free(pblk);
  free(v.blk);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261021);
  std::vector<uint32_t> lens = {0, 1, 2, 3, 4, 5};
  for (uint32_t l = 1019; l <= 1025; ++l) lens.push_back(l);
  for (uint32_t l = 4091; l <= 4097; ++l) lens.push_back(l);
  lens.push_back(65507);  // UDP: T = 65535
  lens.push_back(65508);  // over
  std::vector<uint8_t> pay(65600);
  for (auto &x : pay) x = (uint8_t)rng();
  for (uint32_t L : lens)
    for (uint8_t proto : {17, 1, 6, 47})
      for (uint32_t pa = 0; pa < 4; ++pa)
        for (uint32_t da = 0; da < 4; ++da) run(rng, pay, L, proto, pa, da);
  return finish();
}
