// k_demux on a CPU: one lane's work as yustack_amd/csrc/yucsum_kernels.hip does it,
// with the arithmetic of yucsum_demux.h (eligibility, the three keys out of the
// record's dwords, the hash, the probe chain with its bound, the clamp of an index to
// m), held against a restatement of transportDemuxer.deliverPacketLocked and the gate
// of Nic.DeliverTransportPacket with one std::map: the key is the protocol and the
// TransportEndpointId, an emptied address being -1, which no address equals.
//
// The table sits in an exact-size heap block, so under AddressSanitizer a probe outside
// it is a report. Every probe goes through `Probes`, which also records it: an address
// that is not 16-byte aligned or not inside the table, or a lookup of more than `slots`
// probes, is a failure.
//
// Cases (the program prints each group's count):
//   subsets        every subset of the three kinds registered for one port x a packet
//                  from the connection's peer, from another peer, to another local
//                  address, to another port
//   zero remote    a kind 0 id with remote 0.0.0.0:0 beside a kind 1 id on the same
//                  local pair, and each alone: each catches only its own packets
//   protocols      one 4-tuple under proto 6 and proto 17, and under proto 6 alone
//   gate           proto 1, proto 47 and a zero record, with listeners that would match
//   need x flags   need 0 .. 7 x flags 0 .. 31, and need 0 .. 7 without flags
//   m = 0          the empty table
//   wrapped chain  m = 8 in 16 slots, all eight ids with home slot 15 (found by search
//                  with the hash): the chain wraps past the table's end; a ninth key of
//                  the same home slot misses after nine probes
//   full table     no empty slot: the bound ends every miss after `slots` probes
//   clamp          a slot whose index is m and one whose index is 2^24 - 1
//   fuzz           3000 ids and 5000 packets from small pools, seeded
#include <map>
#include <tuple>

#include "iov_model.h"
#include "yucsum_demux.h"

namespace {

struct Table {
  uint8_t *blk = nullptr;  // exactly `bytes` bytes, 16-byte aligned
  uint64_t bytes = 0;
  uint32_t slots = 0, m = 0;
};

struct Probes {
  const Table &T;
  std::vector<uint64_t> at;  // byte offsets into the table
  bool bad = false;
  explicit Probes(const Table &t) : T(t) {}
  yu::DemuxSlot operator()(uint32_t i) {
    const uint64_t a = (uint64_t)(uintptr_t)T.blk + (uint64_t)yu::kDemuxSlotBytes * i;
    if ((a & 15u) || a < (uint64_t)(uintptr_t)T.blk || a + 16u > (uint64_t)(uintptr_t)T.blk + T.bytes) bad = true;
    at.push_back(a - (uint64_t)(uintptr_t)T.blk);
    yu::DemuxSlot s;
    memcpy(&s, (const void *)(uintptr_t)a, 16);
    return s;
  }
};

// One lane of k_demux: the record's first 16 bytes and the dword holding proto.
uint32_t kernel_demux(Probes &ld, const yu_tx_record &r, bool have_flags, uint32_t flags, uint32_t need) {
  uint32_t w[8];
  memcpy(w, &r, 32);
  const uint32_t proto = yu::demux_rec_proto(w[6]);
  uint32_t e = yu::kDemuxNone;
  if (yu::demux_eligible(proto, have_flags, flags, need)) e = yu::demux_deliver(ld, ld.T.slots, ld.T.m, w[0], w[1], w[2], proto);
  return e;
}

// The restatement. Key: proto, LocalPort, LocalAddress, RemotePort, RemoteAddress.
typedef std::tuple<uint32_t, uint32_t, int64_t, uint32_t, int64_t> Key;
typedef std::map<Key, uint32_t> Model;

int64_t addr_of(const uint8_t *a) { return ((int64_t)a[0] << 24) | (a[1] << 16) | (a[2] << 8) | a[3]; }

Key key_of(const yu_endpoint_id &id) {
  return Key(id.proto, id.local_port, id.kind == 2 ? -1 : addr_of(id.local_addr), id.kind == 0 ? id.remote_port : 0u,
             id.kind == 0 ? addr_of(id.remote_addr) : -1);
}

uint32_t reference(const Model &M, const yu_tx_record &r, bool have_flags, uint32_t flags, uint32_t need) {
  if (r.proto != 6 && r.proto != 17) return YU_DEMUX_NONE;  // no transport protocol: dropped
  if (have_flags && (flags & (need | YU_RX_SPLIT)) != (need | YU_RX_SPLIT)) return YU_DEMUX_NONE;
  const int64_t local = addr_of(r.dst), remote = addr_of(r.src);
  Model::const_iterator it = M.find(Key(r.proto, r.dport, local, r.sport, remote));
  if (it != M.end()) return it->second;
  it = M.find(Key(r.proto, r.dport, local, 0u, -1));
  if (it != M.end()) return it->second;
  it = M.find(Key(r.proto, r.dport, -1, 0u, -1));
  if (it != M.end()) return it->second;
  return YU_DEMUX_NONE;
}

void put_addr(uint8_t *p, uint32_t a) {
  p[0] = (uint8_t)(a >> 24), p[1] = (uint8_t)(a >> 16), p[2] = (uint8_t)(a >> 8), p[3] = (uint8_t)a;
}

yu_endpoint_id id_of(uint32_t kind, uint32_t proto, uint32_t laddr, uint32_t lport, uint32_t raddr, uint32_t rport) {
  yu_endpoint_id id;
  memset(&id, 0, sizeof id);
  if (kind != 2) put_addr(id.local_addr, laddr);
  if (kind == 0) put_addr(id.remote_addr, raddr), id.remote_port = (uint16_t)rport;
  id.local_port = (uint16_t)lport, id.proto = (uint8_t)proto, id.kind = (uint8_t)kind;
  return id;
}

// A received packet's record: from raddr:rport to laddr:lport.
yu_tx_record rec_of(uint32_t proto, uint32_t laddr, uint32_t lport, uint32_t raddr, uint32_t rport, std::mt19937_64 &rng) {
  yu_tx_record r;
  memset(&r, 0, sizeof r);
  put_addr(r.src, raddr), put_addr(r.dst, laddr);
  r.sport = (uint16_t)rport, r.dport = (uint16_t)lport, r.proto = (uint8_t)proto;
  r.seq = (uint32_t)rng(), r.ack = (uint32_t)rng(), r.window = (uint16_t)rng(), r.flags = (uint8_t)rng();  // not part of the key
  r.doff = 20, r.ttl = (uint8_t)rng(), r.ip_id = (uint16_t)rng();
  return r;
}

void table_alloc(Table &T, uint64_t m) {
  free(T.blk);
  T.m = (uint32_t)m, T.slots = yu::demux_slots(m), T.bytes = yu::demux_table_bytes(m);
  T.blk = (uint8_t *)aligned_alloc(16, T.bytes);
  memset(T.blk, 0xEE, T.bytes);
}

// Fills T and the model from ids; all must go in.
void build(Table &T, Model &M, const std::vector<yu_endpoint_id> &ids) {
  table_alloc(T, ids.size());
  const uint64_t bad = yu::demux_fill(ids.data(), ids.size(), T.blk);
  if (bad != ids.size()) {
    fprintf(stderr, "demux_fill refused id %llu\n", (unsigned long long)bad);
    exit(1);
  }
  M.clear();
  for (size_t j = 0; j < ids.size(); ++j) M[key_of(ids[j])] = (uint32_t)j;
  if (M.size() != ids.size()) {
    fprintf(stderr, "the model holds a duplicate the fill took\n");
    exit(1);
  }
}

uint64_t max_probes = 0;

// One packet through the lane and the restatement. expect: a value both must give, or
// kAny. Returns the probes the lane made.
constexpr uint64_t kAny = ~0ull;
size_t check_packet(const Table &T, const Model &M, const yu_tx_record &r, bool have_flags, uint32_t flags, uint32_t need,
                    uint64_t expect, const char *what, bool model = true) {
  Probes ld(T);
  const uint32_t got = kernel_demux(ld, r, have_flags, flags, need);
  const uint32_t want = model ? reference(M, r, have_flags, flags, need) : (uint32_t)expect;
  ++checks;
  bool ok = got == want && (expect == kAny || got == (uint32_t)expect) && !ld.bad;
  ok = ok && (got == YU_DEMUX_NONE || got < T.m) && yu::demux_counter(got, T.m) <= T.m;
  // lookup by lookup: none exceeds `slots` probes, and together they are the lane's
  size_t total = 0;
  if (yu::demux_eligible(r.proto, have_flags, flags, need)) {
    uint32_t w[8];
    memcpy(w, &r, 32);
    for (uint32_t kind = 0; kind < 3; ++kind) {
      Probes one(T);
      const uint32_t e = yu::demux_lookup(one, T.slots, yu::demux_rec_key(kind, w[0], w[1], w[2], r.proto));
      ok = ok && !one.bad && one.at.size() >= 1 && one.at.size() <= T.slots;
      total += one.at.size();
      if (one.at.size() > max_probes) max_probes = one.at.size();
      if (e != yu::kDemuxNone) break;
    }
  }
  ok = ok && total == ld.at.size();
  if (!ok) {
    fprintf(stderr, "%s: proto %u %llx:%u <- %llx:%u flags %d/%x need %x: ep %x (want %x, expect %llx) probes %zu/%zu%s\n", what,
            r.proto, (unsigned long long)addr_of(r.dst), r.dport, (unsigned long long)addr_of(r.src), r.sport,
            (int)have_flags, flags, need, got, want, (unsigned long long)expect, ld.at.size(), total,
            ld.bad ? " PROBE OUT OF BOUNDS" : "");
    if (++fails > 10) exit(1);
  }
  return ld.at.size();
}

uint64_t group(const char *name, uint64_t before) {
  printf("%llu %s\n", (unsigned long long)(checks - before), name);
  return checks;
}

}  // namespace

int main() {
  static_assert(sizeof(yu_endpoint_id) == 16 && sizeof(yu_tx_record) == 32 && sizeof(yu::DemuxSlot) == 16, "layouts");
  std::mt19937_64 rng(20261021);
  Table T;
  Model M;
  uint64_t mark = 0;
  const uint32_t A = 0x0A000001u, B = 0x0A000002u, R = 0xC0A80107u, S = 0xC0A80108u, P = 8080, Q = 8081, RP = 40000;
  const uint32_t NONE = YU_DEMUX_NONE;

  for (uint32_t set = 0; set < 8; ++set) {
    std::vector<yu_endpoint_id> ids;
    uint32_t at[3] = {NONE, NONE, NONE};
    for (uint32_t kind = 0; kind < 3; ++kind)
      if (set >> kind & 1u) at[kind] = (uint32_t)ids.size(), ids.push_back(id_of(kind, 6, A, P, R, RP));
    build(T, M, ids);
    const uint32_t peer = at[0] != NONE ? at[0] : (at[1] != NONE ? at[1] : at[2]);
    const uint32_t other = at[1] != NONE ? at[1] : at[2];
    check_packet(T, M, rec_of(6, A, P, R, RP, rng), false, 0, 0, peer, "the connection's peer");
    check_packet(T, M, rec_of(6, A, P, S, RP, rng), false, 0, 0, other, "another peer");
    check_packet(T, M, rec_of(6, B, P, R, RP, rng), false, 0, 0, at[2], "another local address");
    check_packet(T, M, rec_of(6, A, Q, R, RP, rng), false, 0, 0, NONE, "another port");
  }
  mark = group("subsets", mark);

  {
    const yu_endpoint_id conn0 = id_of(0, 6, A, P, 0, 0), lis = id_of(1, 6, A, P, 0, 0);
    build(T, M, {conn0, lis});
    check_packet(T, M, rec_of(6, A, P, 0, 0, rng), false, 0, 0, 0, "from 0.0.0.0:0, both");
    check_packet(T, M, rec_of(6, A, P, R, RP, rng), false, 0, 0, 1, "from a peer, both");
    build(T, M, {conn0});
    check_packet(T, M, rec_of(6, A, P, 0, 0, rng), false, 0, 0, 0, "from 0.0.0.0:0, connection alone");
    check_packet(T, M, rec_of(6, A, P, R, RP, rng), false, 0, 0, NONE, "from a peer, connection alone");
    build(T, M, {lis});
    check_packet(T, M, rec_of(6, A, P, 0, 0, rng), false, 0, 0, 0, "from 0.0.0.0:0, listener alone");
    check_packet(T, M, rec_of(6, A, P, R, RP, rng), false, 0, 0, 0, "from a peer, listener alone");
  }
  mark = group("zero remote", mark);

  build(T, M, {id_of(0, 6, A, P, R, RP), id_of(0, 17, A, P, R, RP)});
  check_packet(T, M, rec_of(6, A, P, R, RP, rng), false, 0, 0, 0, "proto 6 of both");
  check_packet(T, M, rec_of(17, A, P, R, RP, rng), false, 0, 0, 1, "proto 17 of both");
  build(T, M, {id_of(0, 6, A, P, R, RP)});
  check_packet(T, M, rec_of(6, A, P, R, RP, rng), false, 0, 0, 0, "proto 6 alone");
  check_packet(T, M, rec_of(17, A, P, R, RP, rng), false, 0, 0, NONE, "proto 17 against proto 6");
  mark = group("protocols", mark);

  {
    build(T, M, {id_of(2, 6, 0, 0, 0, 0), id_of(2, 17, 0, 0, 0, 0), id_of(2, 6, 0, P, 0, 0), id_of(2, 17, 0, P, 0, 0)});
    yu_tx_record z;
    memset(&z, 0, sizeof z);
    size_t probes = check_packet(T, M, rec_of(1, A, 0, R, 0x0800, rng), false, 0, 0, NONE, "ICMP");
    probes += check_packet(T, M, rec_of(47, A, P, R, RP, rng), false, 0, 0, NONE, "protocol 47");
    probes += check_packet(T, M, z, false, 0, 0, NONE, "zero record");
    if (probes != 0) ++fails, fprintf(stderr, "an ineligible packet probed the table\n");
  }
  mark = group("gate", mark);

  build(T, M, {id_of(1, 17, A, P, 0, 0)});
  for (uint32_t need = 0; need < 8; ++need) {
    for (uint32_t flags = 0; flags < 32; ++flags) {
      const bool pass = (flags & (need | 16u)) == (need | 16u);
      check_packet(T, M, rec_of(17, A, P, R, RP, rng), true, flags, need, pass ? 0u : NONE, "need x flags");
    }
    check_packet(T, M, rec_of(17, A, P, R, RP, rng), false, 0xFFFFu, need, 0, "need without flags");
  }
  mark = group("need x flags", mark);

  {
    build(T, M, {});
    if (T.slots != 16 || T.bytes != 256) ++fails;
    yu_tx_record z;
    memset(&z, 0, sizeof z);
    size_t probes = check_packet(T, M, rec_of(6, A, P, R, RP, rng), false, 0, 0, NONE, "m = 0, TCP");
    probes += check_packet(T, M, rec_of(17, A, P, R, RP, rng), false, 0, 0, NONE, "m = 0, UDP");
    probes += check_packet(T, M, z, false, 0, 0, NONE, "m = 0, zero record");
    if (probes != 6) ++fails, fprintf(stderr, "m = 0: %zu probes, not one per lookup\n", probes);
  }
  mark = group("m = 0", mark);

  {
    // nine listener ports whose key has home slot 15 of 16
    std::vector<uint32_t> ports;
    for (uint32_t port = 1; port < 65536 && ports.size() < 9; ++port) {
      const yu_endpoint_id id = id_of(2, 6, 0, port, 0, 0);
      if ((yu::demux_hash(yu::demux_id_key(id)) & 15u) == 15u) ports.push_back(port);
    }
    std::vector<yu_endpoint_id> ids;
    for (uint32_t j = 0; j < 8; ++j) ids.push_back(id_of(2, 6, 0, ports[j], 0, 0));
    build(T, M, ids);
    if (T.slots != 16) ++fails;
    for (uint32_t j = 0; j < 9; ++j) {
      Probes ld(T);
      const yu_tx_record r = rec_of(6, A, ports[j], R, RP, rng);
      uint32_t w[8];
      memcpy(w, &r, 32);
      const uint32_t e = yu::demux_lookup(ld, T.slots, yu::demux_rec_key(2, w[0], w[1], w[2], 6));
      // slot 15 first, then 0, 1, ..: id j after j + 1 probes, the ninth key at the first empty slot
      bool ok = e == (j < 8 ? j : NONE) && ld.at.size() == j + 1;
      for (size_t t = 0; t < ld.at.size(); ++t) ok = ok && ld.at[t] == 16u * ((15u + t) & 15u);
      if (!ok) ++fails, fprintf(stderr, "wrapped chain: key %u: ep %x after %zu probes\n", j, e, ld.at.size());
      check_packet(T, M, r, false, 0, 0, j < 8 ? j : NONE, "wrapped chain");
    }
  }
  mark = group("wrapped chain", mark);

  {
    build(T, M, {id_of(2, 6, 0, P, 0, 0)});
    for (uint32_t i = 0; i < T.slots; ++i) {  // every slot taken by something no key equals
      const yu::DemuxSlot s = {(uint32_t)rng() | 1u, (uint32_t)rng() | 1u, (uint32_t)rng() | 0x10000u, 0x00000777u + (i << 8)};
      memcpy(T.blk + 16u * i, &s, 16);
    }
    M.clear();
    for (uint32_t proto : {6u, 17u})
      for (uint32_t port : {P, Q}) {
        const size_t probes = check_packet(T, M, rec_of(proto, A, port, R, RP, rng), false, 0, 0, NONE, "full table");
        if (probes != 3u * T.slots) ++fails, fprintf(stderr, "full table: %zu probes\n", probes);
      }
  }
  mark = group("full table", mark);

  {
    std::vector<yu_endpoint_id> ids;
    for (uint32_t j = 0; j < 4; ++j) ids.push_back(id_of(0, 6, A, P + j, R, RP));
    build(T, M, ids);
    for (uint32_t i = 0; i < T.slots; ++i) {
      yu::DemuxSlot s;
      memcpy(&s, T.blk + 16u * i, 16);
      if (s.tag != 0 && (s.tag >> 8) == 0) s.tag = yu::demux_tag(T.m, s.tag & 0xFFu);
      if (s.tag != 0 && (s.tag >> 8) == 1) s.tag = yu::demux_tag((1u << 24) - 1u, s.tag & 0xFFu);
      memcpy(T.blk + 16u * i, &s, 16);
    }
    check_packet(T, M, rec_of(6, A, P, R, RP, rng), false, 0, 0, NONE, "index m", false);
    check_packet(T, M, rec_of(6, A, P + 1, R, RP, rng), false, 0, 0, NONE, "index 2^24 - 1", false);
    check_packet(T, M, rec_of(6, A, P + 2, R, RP, rng), false, 0, 0, 2, "index 2 beside them");
  }
  mark = group("clamp", mark);

  {
    const uint32_t addrs[8] = {A, B, R, S, 0, 0x7F000001u, 0xFFFFFFFFu, 0x0A000003u};
    std::vector<yu_endpoint_id> ids;
    Model seen;
    while (ids.size() < 3000) {
      const uint32_t kind = (uint32_t)(rng() % 3), proto = rng() & 1 ? 6 : 17;
      const yu_endpoint_id id = id_of(kind, proto, addrs[rng() % 8], 1000 + (uint32_t)(rng() % 64), addrs[rng() % 8],
                                      (uint32_t)(rng() % 16));
      if (seen.insert(std::make_pair(key_of(id), 0u)).second) ids.push_back(id);
    }
    build(T, M, ids);
    for (uint32_t k = 0; k < 5000; ++k) {
      static const uint32_t protos[4] = {6, 17, 6, 1};
      const yu_tx_record r = rec_of(protos[rng() % 4], addrs[rng() % 8], 1000 + (uint32_t)(rng() % 66), addrs[rng() % 8],
                                    (uint32_t)(rng() % 17), rng);
      check_packet(T, M, r, (rng() & 3) != 0, (uint32_t)(rng() % 32), rng() & 1 ? 5u : 0u, kAny, "fuzz");
    }
  }
  mark = group("fuzz", mark);

  printf("at most %llu probes in one lookup\n", (unsigned long long)max_probes);
  free(T.blk);
  return finish();
}
