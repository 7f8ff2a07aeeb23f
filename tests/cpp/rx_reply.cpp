// yu_rx_reply on a CPU (yustack_amd/csrc/yucsum_reply.h): k_reply run as the kernel
// runs it, in wave steps of 64 lanes, each lane with the loads the kernel makes (the ep
// dword and the ep_echo byte only where reply_reads_ep / reply_reads_echo allow them,
// through index-checked blocks), then the scan of yucsum_group.h in its three phases
// (tile sums, one block over the sums in per-thread runs, add-back) in place over
// r_offsets, with its tile sums in a block of exactly yu_rx_reply_workspace_bytes(n)
// bytes. Every array is a heap block of its exact size; every store goes through
// Buf::put, which checks the index and counts the stores per element, and every load of
// ep and ep_echo through Buf::get. Compared with a direct loop over the records' fields.
//
// Prints "<cases> cases ok". CPU only; also run under ASan + UBSan.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "yucsum_reply.h"

namespace {

[[noreturn]] void fail(const char *what, uint64_t a = 0, uint64_t b = 0) {
  printf("FAIL: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
  exit(1);
}

// An exact-size heap block; every access is index-checked, every store counted.
template <typename T>
struct Buf {
  uint64_t n;
  std::unique_ptr<T[]> p;
  std::vector<uint32_t> stores;
  const char *name;
  Buf(uint64_t n_, const char *name_) : n(n_), p(new T[n_ ? n_ : 1]), stores(n_, 0), name(name_) {
    memset(p.get(), 0xA5, sizeof(T) * (n_ ? n_ : 1));
  }
  void put(uint64_t i, const T &v) {
    if (i >= n) fail(name, i, n);
    p[i] = v;
    ++stores[i];
  }
  const T &get(uint64_t i) const {
    if (i >= n) fail(name, i, n);
    return p[i];
  }
  void each_stored(uint32_t times) const {
    for (uint64_t i = 0; i < n; ++i)
      if (stores[i] != times) fail(name, i, stores[i]);
  }
};

uint64_t rng_state = 20261021;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

// group_block_scan: an inclusive scan per wave of 64, the four wave totals combined.
void block_scan(const uint64_t v[256], uint64_t excl[256], uint64_t &total) {
  uint64_t wsum[4], incl[256];
  for (int w = 0; w < 4; ++w) {
    uint64_t acc = 0;
    for (int l = 0; l < 64; ++l) incl[64 * w + l] = acc += v[64 * w + l];
    wsum[w] = acc;
  }
  total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  for (int t = 0; t < 256; ++t) {
    uint64_t before = 0;
    for (int k = 0; k < t / 64; ++k) before += wsum[k];
    excl[t] = before + incl[t] - v[t];
  }
}

// group_scan<uint64_t, uint64_t>(a, n_in, a, n_out, sums): the three launches, in place.
void scan_in_place(Buf<uint64_t> &a, uint64_t n_in, uint64_t n_out, Buf<uint64_t> &sums) {
  const uint64_t tiles = yu::group_scan_tiles(n_out);
  for (uint64_t b = 0; b < tiles; ++b) {
    uint64_t v[256], excl[256], total;
    for (uint32_t t = 0; t < 256; ++t) {
      const uint64_t base = b * yu::kGroupScanTile + t * yu::kGroupScanPer;
      v[t] = 0;
      for (uint32_t k = 0; k < yu::kGroupScanPer; ++k)
        if (base + k < n_in) v[t] += a.get(base + k);
    }
    block_scan(v, excl, total);
    sums.put(b, total);
  }
  {
    const uint64_t run = yu::group_scan_run(tiles);
    uint64_t v[256], excl[256], total;
    for (uint32_t t = 0; t < 256; ++t) {
      const uint64_t lo = std::min<uint64_t>(t * run, tiles), hi = std::min(lo + run, tiles);
      v[t] = 0;
      for (uint64_t i = lo; i < hi; ++i) v[t] += sums.get(i);
    }
    block_scan(v, excl, total);
    for (uint32_t t = 0; t < 256; ++t) {
      const uint64_t lo = std::min<uint64_t>(t * run, tiles), hi = std::min(lo + run, tiles);
      uint64_t acc = excl[t];
      for (uint64_t i = lo; i < hi; ++i) {
        const uint64_t x = sums.get(i);
        sums.put(i, acc);
        acc += x;
      }
    }
  }
  for (uint64_t b = 0; b < tiles; ++b) {
    // a block loads its elements before its barrier and stores the same positions after it
    uint64_t x[256][yu::kGroupScanPer], v[256], excl[256], total;
    for (uint32_t t = 0; t < 256; ++t) {
      const uint64_t base = b * yu::kGroupScanTile + t * yu::kGroupScanPer;
      v[t] = 0;
      for (uint32_t k = 0; k < yu::kGroupScanPer; ++k) v[t] += x[t][k] = base + k < n_in ? a.get(base + k) : 0u;
    }
    block_scan(v, excl, total);
    for (uint32_t t = 0; t < 256; ++t) {
      const uint64_t base = b * yu::kGroupScanTile + t * yu::kGroupScanPer;
      uint64_t acc = excl[t] + sums.get(b);
      for (uint32_t k = 0; k < yu::kGroupScanPer; ++k) {
        if (base + k < n_out) a.put(base + k, acc);
        acc += x[t][k];
      }
    }
  }
}

struct Batch {
  uint64_t n;
  uint32_t m;
  std::vector<yu_tx_record> recs;
  std::vector<yu_iovec> views;
  std::vector<uint16_t> flags;
  std::vector<uint32_t> ep;
};

// Packet i: its kind cycles through the protocols (ICMP types 8 with and without a
// code, 0 and 3; UDP; TCP; GRE), an all-zero record, and view lengths at the limit and
// one past it; ep through 0, m - 1, m and YU_DEMUX_NONE; the flags through every value
// of the five bits.
Batch make(uint64_t n, uint32_t m) {
  Batch b;
  b.n = n, b.m = m;
  b.recs.resize(n), b.views.resize(n), b.flags.resize(n), b.ep.resize(n);
  for (uint64_t i = 0; i < n; ++i) {
    yu_tx_record r;
    uint8_t raw[32];
    for (auto &x : raw) x = (uint8_t)rnd();
    memcpy(&r, raw, 32);
    uint64_t L = rnd() % 1500u;
    const uint32_t kind = (uint32_t)(i % 13u);
    switch (kind) {
      case 0: r.proto = 1, r.sport = 8u << 8; break;
      case 1: r.proto = 1, r.sport = (uint16_t)(8u << 8 | (1u + rnd() % 255u)); break;  // a code: ignored
      case 2: r.proto = 1, r.sport = (uint16_t)(0u << 8 | (rnd() & 0xFFu)); break;      // EchoReply
      case 3: r.proto = 1, r.sport = (uint16_t)(3u << 8 | (rnd() & 0xFFu)); break;      // DstUnreachable
      case 4: case 5: r.proto = 17; break;
      case 6: r.proto = 6; break;
      case 7: r.proto = 47; break;
      case 8: memset(&r, 0, sizeof r), L = 0; break;   // no YU_RX_SPLIT: the all-zero record
      case 9: r.proto = 17, L = 65535u - 28u; break;       // the limit
      case 10: r.proto = 17, L = 65535u - 28u + 1u; break;  // one past it
      case 11: r.proto = 1, r.sport = 8u << 8, L = 65535u - 24u; break;
      default: r.proto = 1, r.sport = 8u << 8, L = 65535u - 24u + 1u + (rnd() & 1u ? 0u : 1ull << 40); break;
    }
    b.recs[i] = r;
    b.views[i] = {(void *)(uintptr_t)(0x10000000ull + 4096ull * i + (rnd() & 3u)), L};  // never dereferenced
    b.flags[i] = (uint16_t)(kind == 8 ? rnd() & 0xFu : rnd() & 0x1Fu);
    const uint32_t eps[4] = {0u, m ? m - 1u : 0u, m, YU_DEMUX_NONE};
    b.ep[i] = eps[(i / 13u + rnd()) % 4u];
  }
  return b;
}

uint64_t cases = 0;

// One call: k_reply over the batch, then the scan; held against the direct loop.
void run(const Batch &b, uint32_t what, int flag_mode, int echo_mode) {
  const uint64_t n = b.n;
  const uint32_t m = b.m;
  const bool have_flags = flag_mode != 0;
  const uint32_t need = flag_mode == 2 ? (YU_RX_IP_OK | YU_RX_L4_OK) : 0u;
  const bool have_echo = echo_mode != 0;
  Buf<uint32_t> ep(n, "ep");
  for (uint64_t i = 0; i < n; ++i) ep.p[i] = b.ep[i];
  Buf<uint8_t> echo(have_echo ? m : 0, "ep_echo");
  for (uint32_t e = 0; e < echo.n; ++e) echo.p[e] = echo_mode == 1 ? 0 : (uint8_t)((e % 3u) ? 1u + (rnd() & 0xFEu) : 0u);
  Buf<yu_tx_record> r_recs(n, "r_recs");
  Buf<uint64_t> r_offsets(n + 1, "r_offsets");
  const uint64_t wb = yu::reply_workspace_bytes(n);
  if (wb % 16u || wb < 8u * yu::group_scan_tiles(n + 1)) fail("workspace bytes", n, wb);
  Buf<uint64_t> sums(wb / 8u, "work");

  // k_reply: wave steps of kReplyPerWave lanes, lanes past n load and store nothing
  for (uint64_t p0 = 0; p0 < n; p0 += yu::kReplyPerWave)
    for (uint32_t lane = 0; lane < yu::kReplyPerWave; ++lane) {
      const uint64_t p = p0 + lane;
      if (p >= n) continue;
      yu::BuildRec in;
      memcpy(in.w, &b.recs[p], 32);
      const uint64_t L = b.views[p].len;
      const uint32_t fl = have_flags ? b.flags[p] : 0u;
      const uint32_t kind = yu::reply_kind(what, yu::reply_gate(have_flags, fl, need), yu::build_proto(in), in.w[2]);
      uint32_t e = yu::kDemuxNone, eb = 0;
      if (yu::reply_reads_ep(kind)) e = ep.get(p);
      if (yu::reply_reads_echo(kind, have_echo, e, m)) eb = echo.get(e);
      yu::BuildRec out;
      const uint64_t T = yu::reply_make(out, in, L, kind, have_echo, e, m, eb);
      yu_tx_record o;
      memcpy(&o, out.w, 32);
      r_recs.put(p, o);
      r_offsets.put(p, T);
    }
  if (n) scan_in_place(r_offsets, n, n + 1, sums);
  else r_offsets.put(0, 0);  // the n == 0 store of the call

  // the direct loop
  r_recs.each_stored(1);
  for (uint64_t i = 0; i <= n; ++i)
    if (r_offsets.stores[i] != (i < n ? 2u : 1u)) fail("r_offsets stores", i, r_offsets.stores[i]);
  uint64_t acc = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const yu_tx_record &r = b.recs[i];
    const uint64_t L = b.views[i].len;
    const uint32_t want = (need | YU_RX_SPLIT);
    const bool gate = !have_flags || (b.flags[i] & want) == want;
    yu_tx_record x;
    memset(&x, 0, sizeof x);
    uint64_t T = 0;
    if ((what & YU_REPLY_ICMP_ECHO) && gate && r.proto == 1 && (r.sport >> 8) == 8 && L <= 65535u - 20u - 4u) {
      memcpy(x.src, r.dst, 4), memcpy(x.dst, r.src, 4);
      x.proto = 1, x.ttl = 64;
      T = 24u + L;
    } else if ((what & YU_REPLY_UDP_ECHO) && gate && r.proto == 17 && b.ep[i] < m &&
               (!have_echo || echo.p[b.ep[i]] != 0) && L <= 65535u - 20u - 8u) {
      memcpy(x.src, r.dst, 4), memcpy(x.dst, r.src, 4);
      x.sport = r.dport, x.dport = r.sport, x.proto = 17, x.ttl = 64;
      T = 28u + L;
    }
    if (memcmp(&x, &r_recs.get(i), 32) != 0) fail("reply record", i, what);
    if (r_offsets.get(i) != acc) fail("r_offsets", i, r_offsets.get(i));
    acc += T;
  }
  if (r_offsets.get(n) != acc) fail("r_offsets[n]", n, r_offsets.get(n));
  ++cases;
}

}  // namespace

int main() {
  static_assert(sizeof(yu_tx_record) == 32 && sizeof(yu::BuildRec) == 32, "a record is eight dwords");
  const uint64_t tile = yu::kGroupScanTile;
  if (tile != 2048u || yu::kReplyPerWave != 64u) fail("the seams below are those of a 2048 tile and a 64 step");
  const uint64_t ns[] = {0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 5};
  uint64_t prev = 0;
  for (uint64_t n = 0; n < 5 * tile; ++n) {  // monotone, and the formula
    const uint64_t w = yu::reply_workspace_bytes(n);
    if (w < prev || w != ((8u * ((n + 1 + 2047u) / 2048u) + 15u) & ~15ull)) fail("workspace formula", n, w);
    prev = w;
  }
  for (uint64_t n : ns)
    for (uint32_t m : {5u, 1u}) {
      if (m == 1u && n != 65) continue;  // m - 1 == 0: one size is enough
      const Batch b = make(n, m);
      for (uint32_t what = 0; what < 4; ++what)
        for (int flag_mode = 0; flag_mode < 3; ++flag_mode)
          for (int echo_mode = 0; echo_mode < 3; ++echo_mode) run(b, what, flag_mode, echo_mode);
    }
  {  // m == 0: no endpoint exists, no UDP reply, and ep_echo is an empty table that is never read
    const Batch b = make(200, 0);
    for (int echo_mode = 0; echo_mode < 3; ++echo_mode) run(b, 3, 0, echo_mode);
  }
  printf("%llu cases ok\n", (unsigned long long)cases);
  return 0;
}
