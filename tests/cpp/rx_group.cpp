// The kernels of yu_rx_group on a CPU (yustack_amd/csrc/yucsum_group.h): the passes run
// as the kernels run them: a block per tile, four waves per block, each on its quarter
// in steps of 64 lanes, the match-by-digit masks as 64-bit ballot words, the per-wave
// digit counts combined in a [4][256] array as in LDS, the digit-major histogram, and
// the scan in its three phases (tile sums, one block over the sums in per-thread runs,
// add-back). Every array is a heap block of its exact size and every store goes through
// Buf::put, which checks the index and counts the stores per element. Compared with
// std::stable_sort, a count, and a direct loop for q_views and q_offsets.
//
// Prints "<cases> cases ok". CPU only; also run under ASan + UBSan.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <numeric>
#include <vector>

#include "yucsum_group.h"

namespace {

[[noreturn]] void fail(const char *what, uint64_t a = 0, uint64_t b = 0) {
  printf("FAIL: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
  exit(1);
}

// An exact-size heap block; every store is index-checked and counted.
template <typename T>
struct Buf {
  uint64_t n;
  std::unique_ptr<T[]> p;
  std::vector<uint32_t> stores;
  const char *name;
  Buf(uint64_t n_, const char *name_) : n(n_), p(new T[n_ ? n_ : 1]), stores(n_, 0), name(name_) {
    for (uint64_t i = 0; i < n; ++i) p[i] = garbage();
  }
  static T garbage();
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
template <> uint32_t Buf<uint32_t>::garbage() { return 0xA5A5A5A5u; }
template <> uint64_t Buf<uint64_t>::garbage() { return 0xA5A5A5A5A5A5A5A5ull; }
template <> yu_iovec Buf<yu_iovec>::garbage() { return {(void *)(uintptr_t)0xA5A5A5A5u, 0xA5A5u}; }

struct Wave {  // one wave step: what the 64 lanes hold
  bool act[64];
  uint32_t key[64], d[64];
  uint64_t same[64];
};

// group_match of the kernel: one ballot per digit bit among the active lanes.
void match(Wave &w) {
  uint64_t active = 0;
  for (int l = 0; l < 64; ++l) active |= (uint64_t)w.act[l] << l;
  uint64_t set[8] = {};
  for (int b = 0; b < 8; ++b)
    for (int l = 0; l < 64; ++l) set[b] |= (uint64_t)(w.act[l] && ((w.d[l] >> b) & 1u)) << l;
  for (int l = 0; l < 64; ++l) {
    uint64_t s = active;
    for (int b = 0; b < 8; ++b) s &= ((w.d[l] >> b) & 1u) ? set[b] : ~set[b];
    w.same[l] = s;
  }
}

struct Pass {
  const uint32_t *ep;          // head pass
  const Buf<uint32_t> *src;    // later passes: n keys then n numbers
  Buf<uint32_t> *dst;          // not the last pass
  Buf<uint32_t> *order;        // the last pass
  Buf<uint32_t> *hist, *count;
  uint64_t n;
  uint32_t m, pass, bits, tile, blocks;
  uint32_t key(uint64_t i) const { return ep ? yu::group_key(ep[i], m) : src->get(i); }
  void load(Wave &w, uint64_t at) const {
    for (int l = 0; l < 64; ++l) {
      w.act[l] = at + l < n;
      w.key[l] = w.act[l] ? key(at + l) : 0u;
      w.d[l] = yu::group_digit(w.key[l], pass, bits);
    }
  }
};

void k_hist(const Pass &A, bool count) {
  for (uint32_t b = 0; b < A.blocks; ++b) {
    uint32_t h[yu::kGroupRadixMax] = {};
    uint32_t none = 0;  // the key m is counted per block
    for (uint32_t w = 0; w < yu::kGroupWaves; ++w) {
      const uint64_t begin = yu::group_wave_begin(b, w, A.tile);
      for (uint32_t s = 0; s < yu::group_wave_steps(A.tile) && begin + 64u * s < A.n; ++s) {
        Wave v;
        A.load(v, begin + 64u * s);
        uint64_t todo = 0;
        for (int l = 0; l < 64; ++l) {
          if (v.act[l]) ++h[v.d[l]];
          todo |= (uint64_t)(v.act[l] && v.key[l] != A.m) << l;
          if (count && v.act[l] && v.key[l] == A.m) ++none;
        }
        while (count && todo) {
          const int first = __builtin_ctzll(todo);
          uint64_t same = 0;
          for (int l = 0; l < 64; ++l) same |= (uint64_t)(v.act[l] && v.key[l] == v.key[first]) << l;
          A.count->put(v.key[first], A.count->get(v.key[first]) + (uint32_t)__builtin_popcountll(same));
          todo &= ~same;
        }
      }
    }
    for (uint32_t t = 0; t < (1u << A.bits); ++t) A.hist->put(yu::group_hist_at(t, b, A.blocks), h[t]);
    if (count && none) A.count->put(A.m, A.count->get(A.m) + none);
  }
}

void k_scatter(const Pass &A) {
  for (uint32_t b = 0; b < A.blocks; ++b) {
    uint32_t cnt[yu::kGroupWaves][yu::kGroupRadixMax] = {};
    for (uint32_t w = 0; w < yu::kGroupWaves; ++w) {
      const uint64_t begin = yu::group_wave_begin(b, w, A.tile);
      for (uint32_t s = 0; s < yu::group_wave_steps(A.tile) && begin + 64u * s < A.n; ++s) {
        Wave v;
        A.load(v, begin + 64u * s);
        match(v);
        for (int l = 0; l < 64; ++l)
          if (v.act[l] && (v.same[l] & (((uint64_t)1 << l) - 1u)) == 0)
            cnt[w][v.d[l]] += (uint32_t)__builtin_popcountll(v.same[l]);
      }
    }
    for (uint32_t d = 0; d < yu::kGroupRadixMax; ++d) {
      uint32_t at = d < (1u << A.bits) ? A.hist->get(yu::group_hist_at(d, b, A.blocks)) : 0u;
      for (uint32_t k = 0; k < yu::kGroupWaves; ++k) {
        const uint32_t c = cnt[k][d];
        cnt[k][d] = at;
        at += c;
      }
    }
    for (uint32_t w = 0; w < yu::kGroupWaves; ++w) {
      const uint64_t begin = yu::group_wave_begin(b, w, A.tile);
      for (uint32_t s = 0; s < yu::group_wave_steps(A.tile) && begin + 64u * s < A.n; ++s) {
        Wave v;
        A.load(v, begin + 64u * s);
        match(v);
        uint32_t pos[64], rank[64];
        for (int l = 0; l < 64; ++l) {  // every lane reads, then the lowest lane of a digit writes
          rank[l] = (uint32_t)__builtin_popcountll(v.same[l] & (((uint64_t)1 << l) - 1u));
          pos[l] = v.act[l] ? cnt[w][v.d[l]] + rank[l] : 0u;
        }
        for (int l = 0; l < 64; ++l)
          if (v.act[l] && rank[l] == 0) cnt[w][v.d[l]] = pos[l] + (uint32_t)__builtin_popcountll(v.same[l]);
        for (int l = 0; l < 64; ++l) {
          if (!(v.act[l] && pos[l] < A.n)) continue;
          const uint64_t i = begin + 64u * s + l;
          const uint32_t num = A.ep ? (uint32_t)i : A.src->get(A.n + i);
          if (A.order) {
            A.order->put(pos[l], num);
          } else {
            A.dst->put(pos[l], v.key[l]);
            A.dst->put(A.n + pos[l], num);
          }
        }
      }
    }
  }
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

// The three launches. in == out is allowed, as in the library.
template <typename TIn, typename TOut>
void scan(const Buf<TIn> &in, uint64_t n_in, Buf<TOut> &out, uint64_t n_out) {
  const uint64_t tiles = yu::group_scan_tiles(n_out);
  Buf<uint64_t> sums(tiles, "scan sums");
  for (uint64_t b = 0; b < tiles; ++b) {
    uint64_t v[256], excl[256], total;
    for (uint32_t t = 0; t < 256; ++t) {
      const uint64_t base = b * yu::kGroupScanTile + t * yu::kGroupScanPer;
      v[t] = 0;
      for (uint32_t k = 0; k < yu::kGroupScanPer; ++k)
        if (base + k < n_in) v[t] += in.get(base + k);
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
  sums.each_stored(2);
  for (uint64_t b = 0; b < tiles; ++b) {
    uint64_t x[256][yu::kGroupScanPer], v[256], excl[256], total;
    for (uint32_t t = 0; t < 256; ++t) {
      const uint64_t base = b * yu::kGroupScanTile + t * yu::kGroupScanPer;
      v[t] = 0;
      for (uint32_t k = 0; k < yu::kGroupScanPer; ++k) v[t] += x[t][k] = base + k < n_in ? (uint64_t)in.get(base + k) : 0u;
    }
    block_scan(v, excl, total);
    for (uint32_t t = 0; t < 256; ++t) {
      const uint64_t base = b * yu::kGroupScanTile + t * yu::kGroupScanPer;
      uint64_t acc = excl[t] + sums.get(b);
      for (uint32_t k = 0; k < yu::kGroupScanPer; ++k) {
        if (base + k < n_out) out.put(base + k, (TOut)acc);
        acc += x[t][k];
      }
    }
  }
}

uint64_t cases = 0;

// One call of yu_rx_group as the library makes it, on a tile of `tile` packets.
void run(const std::vector<uint32_t> &ep, uint32_t m, uint32_t tile) {
  const uint64_t n = ep.size();
  if (n == 0) {  // k_group_zero alone: the empty CSR
    Buf<uint32_t> first_words(2 * ((uint64_t)m + 2), "first"), q0(2, "q_offsets");
    for (uint64_t i = 0; i < first_words.n; ++i) first_words.put(i, 0);
    for (uint32_t t = 0; t < 256; ++t)
      if (t < 2) q0.put(t, 0);
    first_words.each_stored(1);
    q0.each_stored(1);
    ++cases;
    return;
  }
  const uint32_t passes = yu::group_passes(m), bits = yu::group_digit_bits(m);
  const uint32_t blocks = (uint32_t)((n + tile - 1) / tile);
  if (tile == yu::group_tile(n) && blocks != yu::group_blocks(n)) fail("blocks", n, blocks);
  Buf<uint32_t> order(n, "order"), hist(((uint64_t)1 << bits) * blocks, "hist"), count(passes > 1 ? m + 1 : 0, "count");
  Buf<uint32_t> pairs[2] = {Buf<uint32_t>(passes > 1 ? 2 * n : 0, "pair 0"), Buf<uint32_t>(passes > 2 ? 2 * n : 0, "pair 1")};
  Buf<uint64_t> first((uint64_t)m + 2, "first");
  for (uint64_t e = 0; e < count.n; ++e) count.put(e, 0);  // k_group_zero
  for (uint32_t pass = 0; pass < passes; ++pass) {
    const bool head = pass == 0, last = pass + 1 == passes;
    const Pass A = {head ? ep.data() : nullptr, head ? nullptr : &pairs[(pass - 1) & 1], last ? nullptr : &pairs[pass & 1],
                    last ? &order : nullptr, &hist, &count, n, m, pass, bits, tile, blocks};
    k_hist(A, head && passes > 1);
    scan(hist, hist.n, hist, hist.n);
    k_scatter(A);
  }
  if (n) order.each_stored(1);
  hist.each_stored(2 * passes);
  for (int k = 0; k < 2; ++k) pairs[k].each_stored(k == 0 ? (passes > 1) + (passes > 3) : (passes > 2));
  if (passes == 1) {
    for (uint64_t e = 0; e < (uint64_t)m + 2; ++e)
      first.put(e, e <= m ? (uint64_t)hist.get(yu::group_hist_at((uint32_t)e, 0, blocks)) : n);
  } else {
    scan(count, (uint64_t)m + 1, first, (uint64_t)m + 2);
  }
  first.each_stored(1);

  // the expectations
  std::vector<uint32_t> key(n), want(n);
  for (uint64_t i = 0; i < n; ++i) key[i] = ep[i] < m ? ep[i] : m;
  std::iota(want.begin(), want.end(), 0u);
  std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  for (uint64_t j = 0; j < n; ++j)
    if (order.get(j) != want[j]) fail("order", j, order.get(j));
  std::vector<uint64_t> below((uint64_t)m + 2, 0);
  for (uint64_t i = 0; i < n; ++i) ++below[key[i] + 1];
  for (uint64_t e = 1; e < below.size(); ++e) below[e] += below[e - 1];
  for (uint64_t e = 0; e < below.size(); ++e)
    if (first.get(e) != below[e]) fail("first", e, first.get(e));

  // with views: k_group_views, then the lengths scanned in place
  std::vector<yu_iovec> views(n);
  for (uint64_t i = 0; i < n; ++i) views[i] = {(void *)(uintptr_t)(0x1000u + 16u * i), (i * 2654435761u) % 1501u};
  if (n > 2) views[2].len = 0xFFFFFFFFFFFFFF00ull;  // sums are modulo 2^64
  Buf<yu_iovec> q_views(n, "q_views");
  Buf<uint64_t> q_offsets(n + 1, "q_offsets");
  const uint64_t delivered = first.get(m);
  for (uint64_t j = 0; j < n; ++j) {
    const uint32_t o = order.get(j);
    yu_iovec v = {nullptr, 0};
    if (j < delivered && o < n) v = views[o];
    q_views.put(j, v);
    q_offsets.put(j, v.len);
  }
  scan(q_offsets, n, q_offsets, n + 1);
  q_views.each_stored(1);
  for (uint64_t j = 0; j <= n; ++j)
    if (q_offsets.stores[j] != (j < n ? 2u : 1u)) fail("q_offsets stores", j, q_offsets.stores[j]);
  uint64_t acc = 0;
  for (uint64_t j = 0; j < n; ++j) {
    const bool kept = key[want[j]] < m;
    const yu_iovec w = kept ? views[want[j]] : yu_iovec{nullptr, 0};
    if (q_views.get(j).base != w.base || q_views.get(j).len != w.len) fail("q_views", j);
    if (q_offsets.get(j) != acc) fail("q_offsets", j, q_offsets.get(j));
    acc += w.len;
  }
  if (q_offsets.get(n) != acc) fail("q_offsets[n]", n, q_offsets.get(n));
  ++cases;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

std::vector<uint32_t> fill(uint64_t n, uint32_t m, int pattern) {
  std::vector<uint32_t> ep(n);
  const uint32_t bits = yu::group_bitlen(m);
  for (uint64_t i = 0; i < n; ++i) {
    switch (pattern) {
      case 0: ep[i] = m ? m - 1 : 0; break;                                   // all equal
      case 1: ep[i] = YU_DEMUX_NONE; break;                                   // all none
      case 2: ep[i] = (uint32_t)(n - 1 - i); break;                           // distinct, descending (those >= m: none)
      case 3: ep[i] = bits ? (uint32_t)(i & 1u) << (bits - 1) : 0; break;     // the top digit alone differs
      case 4: {                                                               // m, m + 1, 0x7FFFFFFF mixed in
        const uint32_t odd[4] = {m, m + 1, 0x7FFFFFFFu, m ? rnd() % m : 0};
        ep[i] = odd[rnd() & 3u];
        break;
      }
      default: ep[i] = rnd() % (m + 2u); break;                               // seeded random
    }
  }
  return ep;
}

// The scan alone, long enough that the middle launch's threads take runs of more than
// one tile sum, with the total as the extra output.
void scan_alone(uint64_t len) {
  Buf<uint32_t> in(len, "scan in");
  Buf<uint64_t> out(len + 1, "scan out");
  for (uint64_t i = 0; i < len; ++i) in.put(i, rnd());
  scan(in, len, out, len + 1);
  out.each_stored(1);
  uint64_t acc = 0;
  for (uint64_t i = 0; i <= len; ++i) {
    if (out.get(i) != acc) fail("scan alone", i, out.get(i));
    if (i < len) acc += in.get(i);
  }
  if (yu::group_scan_run(yu::group_scan_tiles(len + 1)) < 2) fail("scan alone: runs of one");
  ++cases;
}

}  // namespace

int main() {
  const uint32_t tile = yu::kGroupTile;
  // the last n: a pass histogram of 256 digits x 9 blocks is more than one scan tile
  const uint64_t ns[] = {0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3, 9 * tile - 27};
  const uint32_t ms[] = {0, 1, 255, 256, 65535, 65536};
  for (uint64_t n : ns)
    for (uint32_t m : ms)
      for (int pattern = 0; pattern < 6; ++pattern) {
        if (yu::group_tile(n) != tile) fail("tile", n);
        run(fill(n, m, pattern), m, tile);
      }
  // a grown tile, as batches over 2^23 packets get: the same walk with twice the steps per wave
  for (int pattern = 0; pattern < 6; ++pattern) run(fill(2 * tile * 2 + 77, 300, pattern), 300, 2 * tile);
  // four passes
  for (int pattern = 0; pattern < 6; ++pattern) run(fill(300, 1u << 24, pattern), 1u << 24, tile);
  scan_alone(600000);
  printf("%llu cases ok\n", (unsigned long long)cases);
  return 0;
}
