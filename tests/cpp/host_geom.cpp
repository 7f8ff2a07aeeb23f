// host_geom.cpp — drives yustack_amd/csrc/yucsum_hostgeom.h (the host path's slice
// cut, burst predicate, shard bounds and field writer) on a CPU, for
// tests/test_host_geom.py. The header makes no HIP call, so a plain g++ compiles
// this; the same program also runs under AddressSanitizer + UBSan.
//
//   host_geom slices IN   one batch per line of IN, its cut on stdout:
//       U id lim_b lim_p direct_max stride len n
//       R id lim_b lim_p direct_max n offsets[0] len_0 .. len_{n-1}
//       V id lim_b lim_p direct_max n  then per packet: k view_len_1 .. view_len_k
//       K id value compiled           (slice_knob; value "-" is an unset knob)
//     -> "id burst=B first:count:bytes ..."   (K: "id limit")
//   host_geom shards IN   E id n ndev | B id ndev n offsets[0] len_0 .. len_{n-1}
//     -> "id b_0 .. b_ndev"
//   host_geom fields OUT  the field writer through the three accessors, for every
//     TX mode, as fixed-size records in OUT (layout: kRecord below); prints the count.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "yucsum_hostgeom.h"

namespace hg = yu::hostgeom;

namespace {

bool rd(FILE *f, uint64_t &v) {
  unsigned long long x;
  if (fscanf(f, "%llu", &x) != 1) return false;
  v = x;
  return true;
}

template <class Count, class Bytes>
void print_cut(uint64_t id, uint64_t n, uint64_t dmax, const Count &count, const Bytes &bytes) {
  std::string line;
  uint64_t max_b = 0, max_pk = 0;
  char tmp[96];
  for (uint64_t first = 0; first < n;) {
    const uint64_t cnt = count(first), b = bytes(first, cnt);
    if (b > max_b) max_b = b;
    if (cnt > max_pk) max_pk = cnt;
    snprintf(tmp, sizeof tmp, " %llu:%llu:%llu", (unsigned long long)first, (unsigned long long)cnt,
             (unsigned long long)b);
    line += tmp;
    if (!cnt) break;  // (never: a slice holds at least one packet; printed, and the test fails)
    first += cnt;
  }
  printf("%llu burst=%d%s\n", (unsigned long long)id, hg::is_burst(max_pk, n, max_b, dmax) ? 1 : 0,
         line.c_str());
}

int slices(const char *path) {
  FILE *f = fopen(path, "r");
  if (!f) return 2;
  char kind[8];
  while (fscanf(f, "%7s", kind) == 1) {
    uint64_t id, lb, lp, dmax, n;
    if (kind[0] == 'K') {
      char val[64];
      uint64_t compiled;
      if (!rd(f, id) || fscanf(f, "%63s", val) != 1 || !rd(f, compiled)) return 3;
      const char *v = strcmp(val, "-") == 0 ? nullptr : (strcmp(val, "''") == 0 ? "" : val);
      printf("%llu %llu\n", (unsigned long long)id, (unsigned long long)hg::slice_knob(v, compiled));
      continue;
    }
    if (!rd(f, id) || !rd(f, lb) || !rd(f, lp) || !rd(f, dmax)) return 3;
    const hg::SliceLimits lim{lb, lp};
    if (kind[0] == 'U') {
      uint64_t stride, len;
      if (!rd(f, stride) || !rd(f, len) || !rd(f, n)) return 3;
      const uint64_t slice = hg::uniform_slice(stride, n, lim);
      print_cut(id, n, dmax, [&](uint64_t first) { return hg::uniform_count(n, slice, first); },
                [&](uint64_t, uint64_t cnt) { return hg::uniform_bytes(stride, (uint32_t)len, cnt); });
    } else if (kind[0] == 'R') {
      uint64_t o0;
      if (!rd(f, n) || !rd(f, o0)) return 3;
      std::vector<uint64_t> off(n + 1, o0);
      for (uint64_t i = 0; i < n; ++i) {
        uint64_t l;
        if (!rd(f, l)) return 3;
        off[i + 1] = off[i] + l;
      }
      print_cut(id, n, dmax, [&](uint64_t first) { return hg::ragged_count(off.data(), n, first, lim); },
                [&](uint64_t first, uint64_t cnt) { return hg::ragged_bytes(off.data(), first, cnt); });
    } else if (kind[0] == 'V') {
      if (!rd(f, n)) return 3;
      static uint8_t somewhere[1];  // a view's base is never read here
      std::vector<yu_iovec> iov;
      std::vector<uint64_t> first_iov(n + 1, 0);
      for (uint64_t i = 0; i < n; ++i) {
        uint64_t k;
        if (!rd(f, k)) return 3;
        for (uint64_t v = 0; v < k; ++v) {
          uint64_t l;
          if (!rd(f, l)) return 3;
          yu_iovec x;
          x.base = l ? somewhere : nullptr;
          x.len = l;
          iov.push_back(x);
        }
        first_iov[i + 1] = iov.size();
      }
      print_cut(id, n, dmax,
                [&](uint64_t first) { return hg::iov_count(iov.data(), first_iov.data(), n, first, lim); },
                [&](uint64_t first, uint64_t cnt) { return hg::iov_bytes(iov.data(), first_iov.data(), first, cnt); });
    } else {
      return 3;
    }
  }
  fclose(f);
  return 0;
}

int shards(const char *path) {
  FILE *f = fopen(path, "r");
  if (!f) return 2;
  char kind[8];
  while (fscanf(f, "%7s", kind) == 1) {
    uint64_t id, n, ndev;
    std::vector<uint64_t> b;
    if (kind[0] == 'E') {
      if (!rd(f, id) || !rd(f, n) || !rd(f, ndev)) return 3;
      b = hg::even_bounds(n, (int)ndev);
    } else {
      uint64_t o0;
      if (!rd(f, id) || !rd(f, ndev) || !rd(f, n) || !rd(f, o0)) return 3;
      std::vector<uint64_t> off(n + 1, o0);
      for (uint64_t i = 0; i < n; ++i) {
        uint64_t l;
        if (!rd(f, l)) return 3;
        off[i + 1] = off[i] + l;
      }
      b = hg::byte_bounds(off.data(), n, (int)ndev);
    }
    printf("%llu", (unsigned long long)id);
    for (uint64_t x : b) printf(" %llu", (unsigned long long)x);
    printf("\n");
  }
  fclose(f);
  return 0;
}

// ---- fields ----------------------------------------------------------------
// A record: mode, accessor (0 uniform, 1 ragged, 2 views), len, view count, the four
// result words handed to the writer (packets 0 and 1, two each), up to kViews views of
// packet 1 as (arena offset, length), the arena before and the arena after. Packet 0 is
// a 4-byte (uniform: len-byte slot) neighbour that is never written.
constexpr int kViews = 14, kArena = 128, kHead = 4 + 8 + 2 * kViews, kRecord = kHead + 2 * kArena;
constexpr uint8_t kGuard = 0xEE;

uint32_t rng_state = 0x9E3779B9u;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

struct View {
  uint32_t off, len;
};

// The cuts of packet 1 into views for the view accessor: pattern 0 one view; 1 a cut
// inside each field with an empty view between its bytes; 2 one-byte views around and
// inside each field, empty views between them; 3 cuts at the field's edges, an empty
// view first and last.
std::vector<uint32_t> view_lens(uint32_t len, const std::vector<uint32_t> &fields, int pattern) {
  std::vector<uint32_t> cuts;
  for (uint32_t f : fields) {
    if (pattern == 1) cuts.push_back(f + 1);
    if (pattern == 2) cuts.insert(cuts.end(), {f, f + 1, f + 2});
    if (pattern == 3) cuts.insert(cuts.end(), {f, f + 2});
  }
  std::vector<bool> at(len + 1, false);
  for (uint32_t c : cuts)
    if (c > 0 && c < len) at[c] = true;
  std::vector<uint32_t> out;
  if (pattern == 3) out.push_back(0);
  uint32_t a = 0;
  for (uint32_t c = 1; c <= len; ++c) {
    if (c == len || at[c]) {
      out.push_back(c - a);
      if (c < len && (pattern == 1 || pattern == 2)) out.push_back(0);
      a = c;
    }
  }
  if (pattern == 3 || len == 0) out.push_back(0);
  return out;
}

uint64_t emit(FILE *out, int mode, int acc, const std::vector<uint8_t> &pkt, const std::vector<uint32_t> &fields,
              int pattern) {
  const uint32_t len = (uint32_t)pkt.size();
  uint8_t rec[kRecord];
  memset(rec, 0, sizeof rec);
  uint8_t *before = rec + kHead, *after = rec + kHead + kArena;
  memset(before, kGuard, kArena);
  uint16_t res[4];
  for (uint16_t &r : res) r = (uint16_t)rnd();
  std::vector<View> views;
  uint64_t off[3] = {0, 0, 0};
  yu_iovec iov[kViews + 1];
  uint64_t first_iov[3] = {0, 1, 1};
  uint64_t stride = 0;
  if (acc == 2) {
    uint32_t pos = 2;
    for (uint32_t l : view_lens(len, fields, pattern)) {
      views.push_back({pos, l});
      pos += l + 1;  // one guard byte between views
    }
    if (views.size() > (size_t)kViews || pos + 1 > (uint32_t)kArena) return 0;  // (never: sizes above)
  } else if (acc == 0) {  // slots of len bytes, 4 guard bytes between: [4][p0][4][p1][4]
    if (2 * len + 12 > (uint32_t)kArena) {  // a 4-byte packet 0 does not fit a uniform slot: one packet
      views.push_back({4, len});
    } else {
      views.push_back({4 + len + 4, len});
      stride = len + 4;
    }
  } else {  // ragged: [4][p0: 4 bytes][p1][guard]
    off[0] = 4;
    off[1] = 8;
    off[2] = 8 + len;
    views.push_back({8, len});
  }
  uint32_t k = 0;
  for (const View &v : views) {
    for (uint32_t j = 0; j < v.len; ++j) before[v.off + j] = pkt[k++];
  }
  if (acc == 1)
    for (int j = 4; j < 8; ++j) before[j] = (uint8_t)rnd();
  if (acc == 0 && stride)
    for (uint32_t j = 0; j < len; ++j) before[4 + j] = (uint8_t)rnd();
  memcpy(after, before, kArena);
  // the call: packet index 1 (index 0 where a uniform batch holds one packet)
  uint64_t i = 1;
  if (acc == 0) {
    i = stride ? 1 : 0;
    hg::put_packet_fields(mode, i, res, hg::UniformAt{after + 4, stride, len});
  } else if (acc == 1) {
    hg::put_packet_fields(mode, i, res, hg::RaggedAt{after, off});
  } else {
    iov[0].base = nullptr;  // packet 0: one empty view
    iov[0].len = 0;
    for (size_t v = 0; v < views.size(); ++v) {
      iov[1 + v].base = views[v].len ? after + views[v].off : nullptr;
      iov[1 + v].len = views[v].len;
    }
    first_iov[2] = 1 + views.size();
    hg::put_packet_fields(mode, i, res, hg::IovAt{iov, first_iov});
  }
  rec[0] = (uint8_t)mode;
  rec[1] = (uint8_t)acc;
  rec[2] = (uint8_t)len;
  rec[3] = (uint8_t)views.size();
  // the packet's own results first, as the rule's reader expects them
  const uint16_t mine[2] = {mode == YU_MODE_TX_DATAGRAM ? res[2 * i] : res[i],
                            mode == YU_MODE_TX_DATAGRAM ? res[2 * i + 1] : (uint16_t)0};
  memcpy(rec + 4, mine, 4);
  memcpy(rec + 8, res, 4);  // (the neighbours' words, for a failure's report)
  for (size_t v = 0; v < views.size(); ++v) {
    rec[12 + 2 * v] = (uint8_t)views[v].off;
    rec[13 + 2 * v] = (uint8_t)views[v].len;
  }
  fwrite(rec, 1, sizeof rec, out);
  return 1;
}

int fields(const char *path) {
  FILE *out = fopen(path, "wb");
  if (!out) return 2;
  uint64_t count = 0, rot = 0;
  const int single[4] = {YU_MODE_UDP, YU_MODE_TCP, YU_MODE_ICMP, YU_MODE_IPV4};
  for (int mode : single) {
    const uint32_t f = yu::mode_field(mode);
    for (uint32_t len = 0; len <= 96; ++len)
      for (uint32_t ihl = 0; ihl < 16; ++ihl) {
        std::vector<uint8_t> pkt(len);
        for (uint8_t &b : pkt) b = (uint8_t)rnd();
        if (len) pkt[0] = (uint8_t)(0x40 | ihl);
        for (int acc = 0; acc < 3; ++acc)
          for (int pattern = 0; pattern < (acc == 2 ? 4 : 1); ++pattern) count += emit(out, mode, acc, pkt, {f}, pattern);
      }
  }
  const uint8_t protos[4] = {1, 6, 17, 47};
  for (uint32_t len = 0; len <= 96; ++len)
    for (uint32_t ihl = 0; ihl < 16; ++ihl) {
      const int hl = 4 * (int)ihl;
      int lo = hl - 1, hi = (int)len + 1;
      if (lo < 0) lo = 0;
      if (hi < lo) hi = lo;  // (the header alone passes the packet: one TotalLength)
      for (int tl = lo; tl <= hi; ++tl, ++rot) {
        std::vector<uint8_t> pkt(len);
        for (uint8_t &b : pkt) b = (uint8_t)rnd();
        const uint8_t proto = protos[rot % 4];
        if (len > 0) pkt[0] = (uint8_t)(0x40 | ihl);
        if (len > 2) pkt[2] = (uint8_t)(tl >> 8);
        if (len > 3) pkt[3] = (uint8_t)tl;
        if (len > 9) pkt[9] = proto;
        std::vector<uint32_t> fl = {10};
        if (yu::l4_field(proto)) fl.push_back((uint32_t)hl + yu::l4_field(proto));
        for (int acc = 0; acc < 3; ++acc) count += emit(out, YU_MODE_TX_DATAGRAM, acc, pkt, fl, acc == 2 ? (int)(rot / 4 % 4) : 0);
      }
    }
  fclose(out);
  printf("%llu records of %d bytes\n", (unsigned long long)count, kRecord);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 3 && strcmp(argv[1], "slices") == 0) return slices(argv[2]);
  if (argc == 3 && strcmp(argv[1], "shards") == 0) return shards(argv[2]);
  if (argc == 3 && strcmp(argv[1], "fields") == 0) return fields(argv[2]);
  fprintf(stderr, "usage: host_geom slices|shards IN | fields OUT\n");
  return 64;
}
