// plan_rows.h — what tests/cpp/plan_table.cpp and tests/cpp/plan_query.cpp share:
// the names, the knob groups, one row per planned shape
//   <U|R> mode align stride len n fill cu | name form policy blocks ppw uf small_waves xcd
// and the shape axes of the launch-plan table. A row goes to g_sink (default: printed).
#ifndef YU_TESTS_PLAN_ROWS_H
#define YU_TESTS_PLAN_ROWS_H

#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "yucsum.h"
#include "yucsum_internal.h"
#include "yucsum_plan.h"

namespace {

const char *const kModeNames[YU_MODE_COUNT] = {"raw", "udp", "tcp", "ipv4", "icmp", "verify_ipv4",
                                               "verify_tcp", "verify_udp", "verify_rx", "tx_datagram"};
const char *const kFormNames[] = {"plain", "runs", "inter", "fill"};

// each side of every cut-over in pick_uniform
const uint32_t kLens[] = {1,   16,  20,  32,  64,  72,   100,  112,  113,  128,  129,  136, 447,
                          448, 704, 705, 768, 1500, 1533, 1536, 1537, 3072, 3073, 9000, 65535};
const uint32_t kRawLens[] = {131072, 131073, 200000};
// kSmallBurst, kMidBatch and the runs threshold (128 packets per CU) at 256 and 64 CUs
const uint64_t kCounts256[] = {1, 2, 1000, 4096, 4097, 32767, 32768, 65535, 65536, 1u << 20};
const uint64_t kCounts64[] = {1, 2, 1000, 4096, 4097, 8191, 8192, 32767, 32768, 65535, 65536, 1u << 20};
constexpr uint64_t kSeg32Stride = ((1ull << 31) - 65535u - 3u) / 63u;
constexpr uint64_t kBig = 1u << 20;

std::vector<std::string> g_env;  // "NAME=VALUE" of the current knob group
yu::Knobs g_knobs;
bool g_quiet = false;  // no "#" lines (plan_query --reachable)
int g_cus = 0;         // not 0: every row at this CU count (plan_query --reachable)

const char *knob_value(const char *name) {
  const size_t n = strlen(name);
  for (const std::string &e : g_env)
    if (strncmp(e.c_str(), name, n) == 0 && e[n] == '=') return e.c_str() + n + 1;
  return nullptr;
}

void set_knobs(const std::vector<std::string> &env) {
  g_env = env;
  g_knobs = yu::read_knobs(knob_value);
  if (g_quiet) return;
  printf("# knobs:");
  for (const std::string &e : g_env) printf(" %s", e.c_str());
  printf("\n");
}

void knobs(std::initializer_list<const char *> env) {
  set_knobs(std::vector<std::string>(env.begin(), env.end()));
}

void note(const char *text) {
  if (!g_quiet) printf("%s\n", text);
}

void print_row(const yu::Shape &s, int cus, const yu::Plan &p) {
  printf("%c %s %llu %llu %u %llu %d %d | %s %s %u %u %u %u %u %u\n", s.ragged ? 'R' : 'U',
         kModeNames[s.mode], (unsigned long long)s.align, (unsigned long long)s.stride, s.len,
         (unsigned long long)s.n, (int)s.fill, cus, p.name, kFormNames[(int)p.form], p.policy,
         p.blocks, p.ppw, p.uf, p.small_waves, p.xcd);
}

void (*g_sink)(const yu::Shape &, int, const yu::Plan &) = print_row;

void row(const yu::Shape &s, int cus) {
  if (g_cus) cus = g_cus;
  g_sink(s, cus, yu::plan(s, cus, g_knobs));
}

void uniform(int mode, bool fill, uint64_t align, uint64_t stride, uint32_t len, uint64_t n,
             int cus = 256) {
  row({false, align, stride, len, n, mode, fill}, cus);
}

void ragged(int mode, bool fill, uint64_t n, int cus = 256) { row({true, 0, 0, 0, n, mode, fill}, cus); }

uint64_t ceil4(uint64_t x) { return (x + 3u) & ~3ull; }

// every mode, written in place too where the mode allows it
template <typename F>
void each_mode(F f) {
  for (int mode = 0; mode < YU_MODE_COUNT; ++mode)
    for (int fill = 0; fill <= (yu::mode_fills(mode) ? 1 : 0); ++fill) f(mode, fill != 0);
}

template <typename F>
void each_len(int mode, F f) {
  for (uint32_t len : kLens) f(len);
  if (mode == YU_MODE_RAW)
    for (uint32_t len : kRawLens) f(len);
}

void len_axis() {
  note("# uniform, by length: every mode on dense large batches, one mode of each kind on small ones");
  each_mode([](int mode, bool fill) {
    const bool small = fill ? mode == YU_MODE_TCP || mode == YU_MODE_TX_DATAGRAM
                            : mode == YU_MODE_RAW || mode == YU_MODE_IPV4 || mode == YU_MODE_VERIFY_RX;
    each_len(mode, [&](uint32_t len) {
      uniform(mode, fill, 0, len, len, kBig);
      if (small) uniform(mode, fill, 0, len, len, 1000);
    });
  });
}

void stride_axis() {
  note("# uniform, by stride: each side of 2*stride <= 3*len, the k_lane window, the 32-bit k_seg kinds");
  // (the header-only and datagram modes do not look at the stride below kSeg32Stride:
  // three lengths each)
  const struct { int mode; bool fill, every_len; } base[] = {
      {YU_MODE_RAW, false, true},   {YU_MODE_UDP, true, true},        {YU_MODE_IPV4, false, false},
      {YU_MODE_VERIFY_RX, false, false}, {YU_MODE_TX_DATAGRAM, true, false}};
  for (const auto &b : base)
    each_len(b.mode, [&](uint32_t len) {
      if (!b.every_len && len != 64u && len != 1500u && len != 9000u) return;
      const uint64_t dense = (uint64_t)len * 3 / 2;  // the largest stride with 2*stride <= 3*len
      for (uint64_t stride : {ceil4(len), dense / 4 * 4, dense, dense + 1, ceil4(dense + 1), (uint64_t)len * 2})
        if (stride != len) uniform(b.mode, b.fill, 0, stride, len, kBig);  // (stride = len: by length, above)
      if (len <= 136u)
        for (uint64_t stride : {128u, 132u}) uniform(b.mode, b.fill, 0, stride, len, kBig);
      if (b.mode == YU_MODE_RAW) uniform(b.mode, b.fill, 0, dense + 1, len, 1000);
    });
  for (int mode : {YU_MODE_VERIFY_RX, YU_MODE_TX_DATAGRAM})
    for (int fill = 0; fill <= (yu::mode_fills(mode) ? 1 : 0); ++fill)
      for (uint64_t n : {(uint64_t)1, (uint64_t)2, (uint64_t)1000, kBig})
        for (uint64_t stride : {kSeg32Stride, kSeg32Stride + 1}) uniform(mode, fill != 0, 0, stride, 1500, n);
}

void align_axis() {
  note("# uniform, by the first packet's address & 15");
  for (int mode : {YU_MODE_RAW, YU_MODE_TCP})
    each_len(mode, [&](uint32_t len) {
      for (uint64_t align : {1u, 2u, 4u}) {  // (0: by length, above)
        uniform(mode, false, align, len, len, kBig);
        if (mode == YU_MODE_RAW && (len & 3u)) uniform(mode, false, align, ceil4(len), len, kBig);
      }
    });
}

void count_axis() {
  note("# uniform, by packet count, at 256 and 64 CUs");
  each_mode([](int mode, bool fill) {
    const bool every_len = mode == YU_MODE_RAW || (mode == YU_MODE_TCP && fill);
    for (uint32_t len : {64u, 320u, 1500u, 9000u}) {
      if (!every_len && len != 1500u) continue;
      for (uint64_t n : kCounts256) uniform(mode, fill, 0, len, len, n, 256);
      for (uint64_t n : kCounts64) uniform(mode, fill, 0, len, len, n, 64);
    }
  });
}

void ragged_cases() {
  note("# ragged, by packet count, at 256 and 64 CUs");
  each_mode([](int mode, bool fill) {
    for (uint64_t n : kCounts256) ragged(mode, fill, n, 256);
    for (uint64_t n : kCounts64) ragged(mode, fill, n, 64);
  });
}

// the shapes the knobs are shown on: uniform ones, one per kernel family and form
void uniform_shapes() {
  uniform(YU_MODE_RAW, false, 0, 64, 64, kBig);
  uniform(YU_MODE_UDP, true, 0, 72, 72, kBig);
  uniform(YU_MODE_RAW, false, 0, 128, 100, kBig);
  uniform(YU_MODE_RAW, false, 0, 128, 120, kBig);
  uniform(YU_MODE_TCP, true, 0, 64, 20, kBig);
  uniform(YU_MODE_RAW, false, 0, 320, 320, kBig);
  for (uint64_t n : {(uint64_t)1000, kBig}) {
    uniform(YU_MODE_TCP, false, 0, 1500, 1500, n);
    uniform(YU_MODE_TCP, true, 0, 1500, 1500, n);
  }
  uniform(YU_MODE_TCP, false, 0, 1500, 1500, 32768, 64);
  uniform(YU_MODE_TCP, false, 2, 1500, 1500, kBig);
  uniform(YU_MODE_IPV4, false, 0, 1500, 1500, kBig);
  uniform(YU_MODE_VERIFY_IPV4, false, 0, 40, 40, kBig);
  uniform(YU_MODE_RAW, false, 0, 9000, 9000, kBig);
  uniform(YU_MODE_VERIFY_RX, false, 0, 1500, 1500, kBig);
  uniform(YU_MODE_VERIFY_RX, false, 0, kSeg32Stride + 1, 1500, kBig);
  uniform(YU_MODE_TX_DATAGRAM, true, 0, 1500, 1500, kBig);
}

// and ragged ones: a burst, a mid-size batch and a large one
void ragged_shapes() {
  for (uint64_t n : {(uint64_t)1000, (uint64_t)30000, kBig}) {
    ragged(YU_MODE_RAW, false, n);
    ragged(YU_MODE_UDP, false, n);
    ragged(YU_MODE_UDP, true, n);
    ragged(YU_MODE_IPV4, true, n);
    ragged(YU_MODE_VERIFY_RX, false, n);
    ragged(YU_MODE_TX_DATAGRAM, false, n);
    ragged(YU_MODE_TX_DATAGRAM, true, n);
  }
}

// the shape axes of the table, under the current knobs
void shape_axes() {
  len_axis();
  stride_axis();
  align_axis();
  count_axis();
  ragged_cases();
}

}  // namespace

#endif  // YU_TESTS_PLAN_ROWS_H
