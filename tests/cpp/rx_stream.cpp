// yu_rx_stream on a CPU (yustack_amd/csrc/yucsum_stream.h): k_stream run as the kernel
// runs it, an endpoint at a time in wave steps of 64 lanes (yu::stream_endpoint with a
// Wave whose lanes are an array: the next step loaded before the current one is
// processed, the plain run found by the header's per-lane tests, a prefix sum and a
// ballot, the general step on the broadcast entry), then the kernel's lane-strided
// stores, its tail and the two exclusive sums. Every table is a heap block of its exact
// size and every access goes through Buf, which checks the index. Each batch runs twice,
// with the run test and with it forced off, and both are compared, output for output,
// with a direct loop that takes one segment at a time and keeps its heap in a
// std::vector with container/heap's swaps.
//
// Prints "<cases> cases ok". CPU only; also run under ASan + UBSan.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "yucsum_stream.h"

namespace {

[[noreturn]] void fail(const char *what, uint64_t a = 0, uint64_t b = 0) {
  printf("FAIL: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
  exit(1);
}

template <typename T>
struct Buf {
  uint64_t n;
  std::unique_ptr<T[]> p;
  std::vector<uint32_t> stores;
  const char *name;
  Buf(uint64_t n_, const char *name_) : n(n_), p(new T[n_ ? n_ : 1]), stores(n_, 0), name(name_) {
    memset((void *)p.get(), 0xA5, sizeof(T) * (n_ ? n_ : 1));
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
  void each_stored() const {
    for (uint64_t i = 0; i < n; ++i)
      if (stores[i] == 0) fail(name, i, 0);
  }
};

uint64_t rng_state = 20261021;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

constexpr uint32_t FIN = 1, SYN = 2, RST = 4, PSH = 8, ACK = 16;
constexpr uint32_t NONE = 0xFFFFFFFFu;

struct Pk {  // what a lane loads for one packet
  uint32_t proto, doff, flags, seq;
  uint64_t base, vlen;
};
struct View {
  uint64_t base, len;
  bool operator==(const View &o) const { return base == o.base && len == o.len; }
};
struct Ent {
  uint64_t base, len;
  uint32_t seq, pkt, flags;
  bool operator==(const Ent &o) const {
    return base == o.base && len == o.len && seq == o.seq && pkt == o.pkt && flags == o.flags;
  }
};
struct St {
  uint32_t w[10];
};
struct Rec {
  uint32_t w[8];
};

// ---------------- the direct loop: one segment at a time ----------------
bool lt(uint32_t a, uint32_t b) { return (int32_t)(a - b) < 0; }

struct Direct {
  uint32_t rcv_nxt, rcv_acc, pend_used, pend_size, buf_size, buf_used, snd_nxt, max_sent_ack, wnd_scale, state;
  std::vector<Ent> heap;
  uint32_t cap, n_acks = 0;
  std::vector<View> delivered;
  std::vector<std::pair<uint32_t, uint32_t>> status;  // (pkt, verdict), in the order given

  void ack() {
    ++n_acks;
    const uint32_t avail = buf_used >= buf_size ? 0 : buf_size - buf_used;
    const uint32_t acc = rcv_nxt + avail;
    if (lt(rcv_acc, acc)) rcv_acc = acc;
    max_sent_ack = rcv_nxt;
  }
  bool consume(uint32_t seq, uint32_t &dlen, uint64_t base, uint32_t flags) {
    if (dlen > 0) {
      if (!((uint32_t)(rcv_nxt - seq) < dlen)) return false;
      if (lt(seq, rcv_nxt)) {
        const uint32_t diff = rcv_nxt - seq;
        seq += diff, dlen -= diff, base += diff;
      }
      delivered.push_back(View{base, dlen});
      buf_used += dlen;
    } else if (seq != rcv_nxt) {
      return false;
    }
    rcv_nxt = seq + dlen;
    if (flags & FIN) {
      ++rcv_nxt;
      ack();
      state = 2;
    }
    return true;
  }
  void push(const Ent &x) {
    heap.push_back(x);
    size_t j = heap.size() - 1;
    while (j > 0) {
      const size_t i = (j - 1) / 2;
      if (!lt(heap[j].seq, heap[i].seq)) break;
      std::swap(heap[i], heap[j]);
      j = i;
    }
  }
  void pop() {
    const size_t n = heap.size() - 1;
    std::swap(heap[0], heap[n]);
    size_t i = 0;
    for (;;) {
      const size_t j1 = 2 * i + 1;
      if (j1 >= n) break;
      size_t j = j1;
      if (j1 + 1 < n && lt(heap[j1 + 1].seq, heap[j1].seq)) j = j1 + 1;
      if (!lt(heap[j].seq, heap[i].seq)) break;
      std::swap(heap[i], heap[j]);
      i = j;
    }
    heap.pop_back();
  }
  static uint32_t logical(uint32_t dlen, uint32_t flags) { return dlen + !!(flags & SYN) + !!(flags & FIN); }

  void walk(const std::vector<Pk> &q, const std::vector<uint32_t> &pkts) {
    if (state == 0 || state == 3) {
      for (uint32_t p : pkts) status.push_back({p, state == 0 ? (uint32_t)YU_SEG_NONE : (uint32_t)YU_SEG_UNPROCESSED});
      return;
    }
    bool stopped = false;
    for (size_t k = 0; k < q.size(); ++k) {
      const Pk &s = q[k];
      const uint32_t i = pkts[k];
      if (stopped) {
        status.push_back({i, YU_SEG_UNPROCESSED});
        continue;
      }
      const uint32_t opt = s.doff - 20;
      if (s.proto != 6 || s.doff < 20 || opt > s.vlen || s.vlen > 65535) {
        status.push_back({i, YU_SEG_NONE});
        continue;
      }
      if (s.flags & RST) {
        status.push_back({i, YU_SEG_RST});
        state = 3;
        stopped = true;
        continue;
      }
      if (!(s.flags & ACK)) {
        status.push_back({i, YU_SEG_IGNORED});
        continue;
      }
      if (state == 2) {
        status.push_back({i, YU_SEG_AFTER_CLOSE});
        continue;
      }
      uint32_t dlen = (uint32_t)s.vlen - opt;
      const uint64_t base = s.base + opt;
      const uint32_t wnd = rcv_acc - rcv_nxt;
      const bool ok = wnd == 0 ? (dlen == 0 && s.seq == rcv_nxt)
                               : ((uint32_t)(s.seq - rcv_nxt) < wnd ||
                                  (lt(rcv_nxt, s.seq + dlen) && lt(s.seq, rcv_acc)));
      if (!ok) {
        ack();
        status.push_back({i, YU_SEG_UNACCEPTABLE});
        continue;
      }
      if (!consume(s.seq, dlen, base, s.flags)) {
        if (dlen > 0 || (s.flags & FIN)) {
          if (pend_used < pend_size && heap.size() < cap) {
            pend_used += logical(dlen, s.flags);
            push(Ent{base, dlen, s.seq, i, s.flags});
            status.push_back({i, YU_SEG_PENDING});
          } else {
            status.push_back({i, YU_SEG_DROPPED});
          }
          ack();
        } else {
          status.push_back({i, YU_SEG_NOOP});
        }
        continue;
      }
      status.push_back({i, YU_SEG_CONSUMED});
      while (state == 1 && !heap.empty()) {
        const Ent t = heap[0];
        uint32_t tl = (uint32_t)t.len;
        bool late = false;
        if (!lt(t.seq + tl - 1, rcv_nxt)) {
          if (!consume(t.seq, tl, t.base, t.flags)) break;
          late = true;
        }
        pop();
        pend_used -= logical(tl, t.flags);
        if (t.pkt != NONE) status.push_back({t.pkt, late ? (uint32_t)YU_SEG_CONSUMED_LATE : (uint32_t)YU_SEG_DUPLICATE});
      }
    }
    if ((state == 1 || state == 2) && rcv_nxt != max_sent_ack) ack();
    for (Ent &t : heap) t.pkt = NONE;
  }
};

// ---------------- a batch ----------------
struct Endpoint {
  St st;
  std::vector<Ent> heap;  // at entry
  std::vector<Pk> q;
};
struct Batch {
  uint64_t n = 0;
  uint32_t m = 0, cap = 0;
  std::vector<Pk> pk;
  std::vector<uint32_t> order;
  std::vector<uint64_t> first;
  std::vector<St> st;
  std::vector<Ent> heap;
  std::vector<std::vector<uint32_t>> pkts;  // per endpoint, its packet numbers
};

Batch assemble(const std::vector<Endpoint> &eps, uint32_t cap, uint32_t nobody) {
  Batch B;
  B.m = (uint32_t)eps.size(), B.cap = cap;
  std::vector<size_t> left(B.m + 1);
  for (uint32_t e = 0; e < B.m; ++e) B.n += left[e] = eps[e].q.size();
  B.n += left[B.m] = nobody;
  B.pk.resize(B.n);
  B.pkts.assign(B.m + 1, {});
  std::vector<size_t> at(B.m + 1, 0);
  for (uint64_t i = 0; i < B.n; ++i) {  // a random merge: arrival order inside a queue is kept
    uint32_t e = rnd() % (B.m + 1);
    while (left[e] == 0) e = (e + 1) % (B.m + 1);
    --left[e];
    Pk p = e < B.m ? eps[e].q[at[e]++] : Pk{17u, 0u, 0u, 0u, 0u, 33u};
    p.base = 0x100000ull + 0x10000ull * i;
    B.pk[i] = p;
    B.pkts[e].push_back((uint32_t)i);
  }
  B.first.assign(B.m + 2, 0);
  for (uint32_t e = 0; e <= B.m; ++e) {
    B.first[e] = B.order.size();
    for (uint32_t p : B.pkts[e]) B.order.push_back(p);
  }
  B.first[B.m + 1] = B.n;
  B.st.resize(B.m);
  B.heap.assign((size_t)B.m * cap, Ent{0xA5A5, 0xA5, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5});
  for (uint32_t e = 0; e < B.m; ++e) {
    B.st[e] = eps[e].st;
    if (eps[e].heap.size() > cap) fail("scenario heap above cap");
    for (size_t i = 0; i < eps[e].heap.size(); ++i) B.heap[(size_t)e * cap + i] = eps[e].heap[i];
  }
  return B;
}

struct Out {
  std::vector<uint8_t> status;
  std::vector<View> s_views;
  std::vector<uint64_t> s_offsets, a_offsets;
  std::vector<St> st;
  std::vector<std::vector<Ent>> heap;  // [0, pend_count) per endpoint
  std::vector<Rec> a_recs;
  std::vector<uint32_t> n_acks;
};

uint32_t id_word(uint32_t e, uint32_t k) { return 0x0A000000u + 977u * e + 0x01010101u * k; }

Out expect(const Batch &B) {
  Out O;
  const uint64_t N = B.n + (uint64_t)B.m * B.cap;
  O.status.assign(B.n, YU_SEG_NONE);
  O.s_views.assign(N, View{0, 0});
  O.st = B.st;
  O.heap.resize(B.m);
  O.a_recs.assign(B.m, Rec{{0, 0, 0, 0, 0, 0, 0, 0}});
  O.n_acks.assign(B.m, 0);
  O.a_offsets.assign(B.m + 1, 0);
  for (uint32_t e = 0; e < B.m; ++e) {
    const uint32_t *w = B.st[e].w;
    for (uint32_t i = 0; i < w[8] && i < B.cap; ++i) O.heap[e].push_back(B.heap[(size_t)e * B.cap + i]);
    if (B.pkts[e].empty()) continue;  // not woken: untouched
    Direct D;
    D.rcv_nxt = w[0], D.rcv_acc = w[1], D.pend_used = w[2], D.pend_size = w[3], D.buf_size = w[4], D.buf_used = w[5];
    D.snd_nxt = w[6], D.max_sent_ack = w[7], D.wnd_scale = w[9] & 0xFF, D.state = (w[9] >> 8) & 0xFF;
    D.heap = O.heap[e], D.cap = B.cap;
    std::vector<Pk> q;
    for (uint32_t p : B.pkts[e]) q.push_back(B.pk[p]);
    const uint32_t entry = D.state;
    D.walk(q, B.pkts[e]);
    for (auto &sv : D.status) O.status[sv.first] = (uint8_t)sv.second;
    const uint64_t lo = B.first[e] + (uint64_t)e * B.cap;
    for (size_t k = 0; k < D.delivered.size(); ++k) O.s_views[lo + k] = D.delivered[k];
    if (entry == 1 || entry == 2) {
      O.st[e] = St{{D.rcv_nxt, D.rcv_acc, D.pend_used, D.pend_size, D.buf_size, D.buf_used, D.snd_nxt,
                    D.max_sent_ack, (uint32_t)D.heap.size(), (w[9] & 0xFFFF00FFu) | (D.state << 8)}};
      O.heap[e] = D.heap;
    }
    O.n_acks[e] = D.n_acks;
    if (D.n_acks) {
      uint32_t win = D.wnd_scale < 32 ? (D.rcv_acc - D.rcv_nxt) >> D.wnd_scale : 0;
      if (win > 0xFFFF) win = 0xFFFF;
      O.a_recs[e] = Rec{{id_word(e, 0), id_word(e, 1), id_word(e, 2), D.snd_nxt, D.rcv_nxt,
                         win | (16u << 16) | (20u << 24), 6u | (64u << 8), 0u}};
    }
  }
  O.s_offsets.assign(N + 1, 0);
  for (uint64_t i = 0; i < N; ++i) O.s_offsets[i + 1] = O.s_offsets[i] + O.s_views[i].len;
  for (uint32_t e = 0; e < B.m; ++e) O.a_offsets[e + 1] = O.a_offsets[e] + (O.n_acks[e] ? 40 : 0);
  return O;
}

// ---------------- k_stream as the kernel runs it ----------------
uint64_t run_lanes = 0;  // lanes that took a plain run, over the whole grid

struct Kernel {
  const Batch &B;
  Buf<Pk> recs;
  Buf<uint32_t> order;
  Buf<uint64_t> first;
  Buf<St> st;
  Buf<Ent> heap;
  Buf<uint8_t> status;
  Buf<View> s_views;
  Buf<uint64_t> s_offsets, a_offsets;
  Buf<Rec> a_recs;
  Buf<uint32_t> n_acks;
  uint64_t heap0 = 0;
  yu::StreamSeg cur[64], nxt[64];

  explicit Kernel(const Batch &b)
      : B(b), recs(b.n, "recs"), order(b.n, "order"), first(b.m + 2, "first"), st(b.m, "st"),
        heap((uint64_t)b.m * b.cap, "heap"), status(b.n, "status"), s_views(b.n + (uint64_t)b.m * b.cap, "s_views"),
        s_offsets(b.n + (uint64_t)b.m * b.cap + 1, "s_offsets"), a_offsets(b.m + 1, "a_offsets"),
        a_recs(b.m, "a_recs"), n_acks(b.m, "n_acks") {
    for (uint64_t i = 0; i < b.n; ++i) recs.p[i] = b.pk[i], order.p[i] = b.order[i];
    for (uint64_t i = 0; i < b.m + 2u; ++i) first.p[i] = b.first[i];
    for (uint64_t i = 0; i < b.m; ++i) st.p[i] = b.st[i];
    for (uint64_t i = 0; i < heap.n; ++i) heap.p[i] = b.heap[i];
  }

  // Wave
  void load(uint64_t j0, uint32_t cnt) {
    for (uint32_t l = 0; l < 64; ++l) {
      nxt[l] = yu::StreamSeg{0, 0, NONE, 0, 0};
      if (l >= cnt) continue;
      const uint32_t pkt = order.get(j0 + l);
      nxt[l].pkt = pkt;
      if (pkt >= B.n) continue;
      const Pk &p = recs.get(pkt);
      nxt[l] = yu::StreamSeg{p.base, p.vlen > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)p.vlen, pkt, p.seq,
                               yu::stream_fdp(p.flags, p.doff, p.proto)};
    }
  }
  void advance() { memcpy(cur, nxt, sizeof cur); }
  uint32_t run(const yu::StreamSt &S, const yu::StreamCtx &C, uint32_t k0, uint32_t cnt, uint32_t &sum) {
    uint32_t pl[64], incl[64], acc = 0;
    uint64_t ballot = 0;
    for (uint32_t l = 0; l < 64; ++l) {
      const bool in = l >= k0 && l < cnt;
      pl[l] = in ? yu::stream_plain_len(cur[l]) : 0;
      incl[l] = acc += pl[l];
      if (in && yu::stream_in_run(cur[l], pl[l], S, incl[l] - pl[l])) ballot |= 1ull << l;
    }
    const uint32_t r = yu::stream_run_len(ballot, k0, cnt);
    sum = 0;
    if (r == 0) return 0;
    sum = incl[k0 + r - 1];
    run_lanes += r;
    for (uint32_t l = k0; l < k0 + r; ++l) {
      const uint64_t slot = C.slot_lo + S.slots + (l - k0);
      if (slot < C.slot_hi) st_slot(slot, cur[l].base + (yu::seg_doff(cur[l]) - 20), pl[l]);
      if (cur[l].pkt < C.n) st_status(cur[l].pkt, YU_SEG_CONSUMED);
    }
    return r;
  }
  void fill(uint32_t k0, uint32_t cnt, uint32_t v) {
    for (uint32_t l = k0; l < cnt; ++l)
      if (cur[l].pkt < B.n) st_status(cur[l].pkt, v);
  }
  yu::StreamSeg seg(uint32_t k) const {
    if (k >= 64) fail("seg lane", k);
    return cur[k];
  }
  // Io
  yu::StreamEnt ld_heap(uint32_t i) const {
    if (i >= B.cap) fail("heap index", i, B.cap);
    const Ent &x = heap.get(heap0 + i);
    return yu::StreamEnt{x.base, x.len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)x.len, x.seq, x.pkt, x.flags & 0xFF};
  }
  uint32_t ld_heap_seq(uint32_t i) const {
    if (i >= B.cap) fail("heap index", i, B.cap);
    return heap.get(heap0 + i).seq;
  }
  void mv_heap(uint32_t to, uint32_t from) {
    if (to >= B.cap || from >= B.cap) fail("heap index", to, from);
    heap.put(heap0 + to, heap.get(heap0 + from));
  }
  void st_heap(uint32_t i, const yu::StreamEnt &x) {
    if (i >= B.cap) fail("heap index", i, B.cap);
    heap.put(heap0 + i, Ent{x.base, x.len, x.seq, x.pkt, x.flags});
  }
  void st_status(uint32_t pkt, uint32_t v) { status.put(pkt, (uint8_t)v); }
  void st_slot(uint64_t slot, uint64_t base, uint32_t len) {
    s_views.put(slot, View{base, len});
    s_offsets.put(slot, len);
  }

  void launch(bool runs) {
    const uint64_t n = B.n;
    for (uint64_t e = 0; e < B.m; ++e) {
      uint64_t lo = 0, hi = 0;
      if (n) {
        const uint64_t f0 = first.get(e), f1 = first.get(e + 1);
        lo = f0 < n ? f0 : n;
        hi = f1 < lo ? lo : (f1 < n ? f1 : n);
      }
      const yu::StreamCtx C = {lo + e * B.cap, hi + (e + 1) * B.cap, (uint32_t)n, B.cap};
      yu::StreamSt S = {};
      bool touched = false;
      if (hi > lo) {
        const St w = st.get(e);
        yu::stream_unpack(S, w.w);
        if (S.pend_count > B.cap) S.pend_count = B.cap;
        touched = S.state == yu::kStreamOpen || S.state == yu::kStreamClosed;
        heap0 = e * B.cap;
        yu::stream_endpoint(*this, C, S, (uint32_t)lo, (uint32_t)(hi - lo), runs);
      }
      const uint64_t room = C.slot_hi - C.slot_lo;
      for (uint64_t slot = C.slot_lo + (S.slots < room ? S.slots : room); slot < C.slot_hi; ++slot) st_slot(slot, 0, 0);
      if (touched) {
        for (uint32_t i = 0; i < S.pend_count; ++i) {
          Ent x = heap.get(e * B.cap + i);
          x.pkt = NONE;
          heap.put(e * B.cap + i, x);
        }
        St w = st.get(e);  // only the words a walk can change, and the state byte, are stored
        for (uint32_t k = 0; k < 10; ++k)
          if (yu::stream_word_changes(k)) w.w[k] = yu::stream_pack_word(S, k);
        ((uint8_t *)w.w)[yu::kStreamStateByte] = (uint8_t)S.state;
        st.put(e, w);
      }
      n_acks.put(e, S.n_acks);
    }
    // k_stream_fin: the ACK records from the state the walk left, then the tail
    for (uint32_t e = 0; e < B.m; ++e) {
      const uint32_t na = n_acks.get(e);
      St w = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};
      if (na) w = st.get(e);
      Rec r;
      for (uint32_t k = 0; k < 8; ++k)
        r.w[k] = yu::stream_ack_word(w.w, na, na ? id_word(e, 0) : 0, na ? id_word(e, 1) : 0, na ? id_word(e, 2) : 0, k);
      a_recs.put(e, r);
      a_offsets.put(e, na ? yu::kStreamAckBytes : 0);
    }
    uint64_t d = 0;
    if (n) d = first.get(B.m) < n ? first.get(B.m) : n;
    for (uint64_t j = d; j < n; ++j)
      if (order.get(j) < n) st_status(order.get(j), YU_SEG_NONE);
    const uint64_t N = n + (uint64_t)B.m * B.cap;
    for (uint64_t slot = d + (uint64_t)B.m * B.cap; slot < N; ++slot) st_slot(slot, 0, 0);
    // the two scans, in place (yucsum_group.h's scan has its own program, rx_group.cpp)
    uint64_t acc = 0;
    for (uint64_t i = 0; i <= N; ++i) {
      const uint64_t x = i < N ? s_offsets.get(i) : 0;
      s_offsets.put(i, acc);
      acc += x;
    }
    acc = 0;
    for (uint64_t i = 0; i <= B.m; ++i) {
      const uint64_t x = i < B.m ? a_offsets.get(i) : 0;
      a_offsets.put(i, acc);
      acc += x;
    }
  }
};

uint64_t cases = 0, seen[12] = {}, parked_left = 0;

void check(const Batch &B, const char *what) {
  const Out want = expect(B);
  for (uint8_t v : want.status) ++seen[v < 12 ? v : 0];
  for (auto &h : want.heap) parked_left += h.size();
  for (int runs = 1; runs >= 0; --runs) {
    Kernel K(B);
    K.launch(runs != 0);
    K.status.each_stored(), K.s_views.each_stored(), K.s_offsets.each_stored();
    K.a_recs.each_stored(), K.a_offsets.each_stored(), K.n_acks.each_stored();
    for (uint64_t i = 0; i < B.n; ++i)
      if (K.status.p[i] != want.status[i]) {
        printf("%s runs=%d: status[%llu] = %u, want %u\n", what, runs, (unsigned long long)i, K.status.p[i],
               want.status[i]);
        fail("status", i, B.n);
      }
    for (uint64_t i = 0; i < K.s_views.n; ++i)
      if (!(K.s_views.p[i] == want.s_views[i])) fail(what, i, 1);
    for (uint64_t i = 0; i < K.s_offsets.n; ++i)
      if (K.s_offsets.p[i] != want.s_offsets[i]) fail(what, i, 2);
    for (uint32_t e = 0; e < B.m; ++e) {
      if (memcmp(K.st.p[e].w, want.st[e].w, 40)) {
        for (int k = 0; k < 10; ++k) printf("  st[%d] = %08x want %08x\n", k, K.st.p[e].w[k], want.st[e].w[k]);
        fail(what, e, 3);
      }
      if (B.pkts[e].empty() && K.st.stores[e] != 0) fail("an endpoint that was not woken was stored", e, 4);
      const uint32_t pc = want.st[e].w[8] < B.cap ? want.st[e].w[8] : B.cap;
      if (want.heap[e].size() != pc) fail("heap size", e, pc);
      for (uint32_t i = 0; i < pc; ++i)
        if (!(K.heap.p[(size_t)e * B.cap + i] == want.heap[e][i])) fail(what, e, 5);
      if (memcmp(K.a_recs.p[e].w, want.a_recs[e].w, 32)) fail(what, e, 6);
      if (K.n_acks.p[e] != want.n_acks[e]) fail(what, e, 7);
    }
    for (uint32_t e = 0; e <= B.m; ++e)
      if (K.a_offsets.p[e] != want.a_offsets[e]) fail(what, e, 8);
  }
  ++cases;
}

// ---------------- scenarios ----------------
St make_st(uint32_t rcv_nxt, uint32_t wnd, uint32_t state = 1) {
  return St{{rcv_nxt, rcv_nxt + wnd, 0, wnd, wnd, 0, 5000 + (rnd() & 0xFFFF), rcv_nxt, 0, (state << 8) | (rnd() % 3)}};
}

Pk data(uint32_t seq, uint32_t dlen, uint32_t flags = ACK, uint32_t doff = 20) {
  return Pk{6, doff, flags, seq, 0, (uint64_t)dlen + (doff - 20)};
}

enum Kind {
  kInOrder, kSwap, kGap, kGapFilledLast, kDuplicates, kOverlap, kOvershoot, kZeroWindow, kZeroWindowReopens,
  kFinInOrder, kFinParked, kFinOnlyParked, kDataAfterFin, kRstMiddle, kNoAckFlag, kPureAcks, kDoff32, kWrap,
  kByteBudget, kFullCap, kState0, kState2, kState3, kCarriedHeap, kShuffle, kNotTcp, kKinds
};

Endpoint scenario(int kind, uint32_t L, uint32_t cap) {
  Endpoint E;
  uint32_t nxt = kind == kWrap ? 0xFFFFFF00u : 1000u + (rnd() & 0xFFFFF);
  uint32_t wnd = 1u << 20;
  E.st = make_st(nxt, wnd);
  std::vector<Pk> s;  // the stream in order
  uint32_t seq = nxt;
  const uint32_t total = L + (kind == kCarriedHeap ? 2u : 0u);
  for (uint32_t i = 0; i < total; ++i) {
    const uint32_t dlen = 1 + rnd() % 1460;
    const uint32_t doff = kind == kDoff32 || (rnd() % 5 == 0) ? 32 : 20;
    s.push_back(data(seq, dlen, ACK | (rnd() & 1 ? PSH : 0), doff));
    seq += dlen;
  }
  auto dl = [](const Pk &p) { return (uint32_t)p.vlen - (p.doff - 20); };
  switch (kind) {
    case kInOrder: case kDoff32: case kWrap: break;
    case kSwap:
      if (L >= 2) std::swap(s[L / 2 - (L / 2 == L - 1)], s[L / 2 - (L / 2 == L - 1) + 1]);
      break;
    case kGap:
      for (uint32_t i = L / 3 + 1; i < L; ++i) s[i].seq += 100;
      break;
    case kGapFilledLast:
      if (L >= 2) std::rotate(s.begin() + L / 3, s.begin() + L / 3 + 1, s.end());
      break;
    case kDuplicates:
      for (uint32_t i = 1; i < L; i += 3) s[i] = s[i - 1];
      break;
    case kOverlap:
      for (uint32_t i = 1; i < L; i += 2) {
        const uint32_t back = 1 + rnd() % 3;
        s[i].seq -= back, s[i].vlen += back;
      }
      if (L >= 4) std::swap(s[2], s[3]);  // a parked overlap: the trimmed length leaves the budget
      break;
    case kOvershoot: {
      uint32_t half = 0;
      for (uint32_t i = 0; i < L / 2; ++i) half += dl(s[i]);
      E.st.w[1] = nxt + half + 1, E.st.w[4] = half + 1;
      break;
    }
    case kZeroWindow: case kZeroWindowReopens:
      E.st.w[1] = nxt;
      if (kind == kZeroWindow) E.st.w[5] = E.st.w[4];  // the buffer is full: the window stays shut
      if (L >= 2) s[1] = data(nxt, 0);                 // the one acceptable segment
      break;
    case kFinInOrder:
      if (L) s[L - 1].flags |= FIN;
      break;
    case kFinParked:
      if (L) s[L - 1].flags |= FIN;
      if (L >= 2) std::swap(s[L - 1], s[L - 2]);
      break;
    case kFinOnlyParked:
      if (L >= 2) {
        s[L - 1] = data(s[L - 1].seq, 0, ACK | FIN);
        std::swap(s[L - 1], s[L - 2]);
      }
      break;
    case kDataAfterFin:
      if (L) s[L / 2].flags |= FIN;
      for (uint32_t i = L / 2 + 1; i < L; ++i) ++s[i].seq;
      break;
    case kRstMiddle:
      if (L) s[L / 2].flags |= RST;
      break;
    case kNoAckFlag:
      if (L) s[L / 2].flags &= ~ACK;
      break;
    case kPureAcks:
      for (uint32_t i = 0; i < L; i += 3) s[i] = data(0, 0, ACK, s[i].doff);
      {
        uint32_t q = nxt;  // a pure ACK takes no sequence space: the data closes up
        for (uint32_t i = 0; i < L; ++i) {
          if (dl(s[i]) == 0) s[i].seq = q + (i % 2 ? 5 : 0);
          else s[i].seq = q, q += dl(s[i]);
        }
      }
      break;
    case kByteBudget:
      std::reverse(s.begin(), s.end());
      E.st.w[3] = 2000;
      break;
    case kFullCap:
      std::reverse(s.begin(), s.end());
      break;
    case kState0: E.st.w[9] = (E.st.w[9] & 0xFF) | (0u << 8); break;
    case kState2: E.st.w[9] = (E.st.w[9] & 0xFF) | (2u << 8); break;
    case kState3: E.st.w[9] = (E.st.w[9] & 0xFF) | (3u << 8); break;
    case kCarriedHeap: {
      // two segments of the stream arrived in an earlier batch and wait in the heap
      Direct D{};
      D.cap = cap;
      uint32_t used = 0;
      std::vector<Pk> rest;
      const uint32_t a = total / 2, b = total - 1;
      for (uint32_t i = 0; i < total; ++i) {
        if ((i == a || i == b) && i > 0 && D.heap.size() < cap) {
          D.push(Ent{0x7000000ull + 0x1000ull * i + (s[i].doff - 20), dl(s[i]), s[i].seq, NONE, s[i].flags});
          used += dl(s[i]);
        } else {
          rest.push_back(s[i]);
        }
      }
      rest.resize(std::min<size_t>(rest.size(), L));
      s = rest;
      E.heap = D.heap;
      E.st.w[2] = used, E.st.w[8] = (uint32_t)D.heap.size();
      break;
    }
    case kShuffle:
      for (uint32_t i = L; i > 1; --i)
        if (rnd() % 3 == 0) std::swap(s[i - 1], s[rnd() % i]);
      break;
    case kNotTcp:
      if (L) s[L / 2].proto = 17;
      if (L > 2) s[1].doff = 16;
      if (L > 3) s[2].vlen = 65536;
      if (L > 4) s[3] = Pk{6, 60, ACK, s[3].seq, 0, 39};  // options longer than the view
      break;
    default: fail("kind", kind);
  }
  s.resize(std::min<size_t>(s.size(), L));
  E.q = s;
  return E;
}

}  // namespace

int main() {
  // the workspace: the tile sums of the longer scan, 0 where the call refuses
  for (uint64_t n : {0ull, 1ull, 2047ull, 2048ull, 5000ull, (1ull << 32) - 1})
    for (uint64_t m : {0ull, 1ull, 70ull, 5000ull, 1ull << 24})
      for (uint64_t cap : {0ull, 1ull, 4ull, 1024ull}) {
        const uint64_t N = n + m * cap, longer = std::max(N, m) + 1;
        if (yu::stream_workspace_bytes(n, m, cap) != ((8 * ((longer + 2047) / 2048) + 15) & ~15ull))
          fail("workspace", n, m);
      }
  if (yu::stream_workspace_bytes(1ull << 32, 1, 1) || yu::stream_workspace_bytes(1, (1ull << 24) + 1, 1) ||
      yu::stream_workspace_bytes(1, 1, 1025))
    fail("workspace zeros");
  for (uint32_t k0 = 0; k0 < 64; ++k0)
    for (uint32_t cnt = k0; cnt <= 64; ++cnt) {
      if (yu::stream_run_len(~0ull, k0, cnt) != cnt - k0) fail("run_len all", k0, cnt);
      if (yu::stream_run_len(0, k0, cnt) != 0) fail("run_len none", k0, cnt);
      if (cnt > k0 + 1 && yu::stream_run_len(~(1ull << (cnt - 1)), k0, cnt) != cnt - 1 - k0) fail("run_len", k0, cnt);
    }

  // the grid: a wave per endpoint and a thread per tail packet, at least one block, at most 8 (or the
  // given number) per CU, monotone in both counts
  for (int cus : {1, 8, 256})
    for (uint32_t per : {0u, 1u, 8u, 64u}) {
      const uint64_t cap = (uint64_t)cus * (per ? per : 8u);
      uint32_t last = 0;
      for (uint64_t k : {0ull, 1ull, 4ull, 5ull, 255ull, 256ull, 257ull, 70000ull, 1ull << 24, (1ull << 32) - 1}) {
        const uint32_t bm = yu::stream_blocks(0, k, cus, per), bn = yu::stream_blocks(k, 0, cus, per);
        if (bm != std::max<uint64_t>(1, std::min<uint64_t>(cap, (k + 3) / 4))) fail("stream_blocks m", k, bm);
        if (bn != std::max<uint64_t>(1, std::min<uint64_t>(cap, (k + 255) / 256))) fail("stream_blocks n", k, bn);
        if (yu::stream_blocks(k, k, cus, per) != std::max(bm, bn) || bm < last) fail("stream_blocks both", k, bm);
        last = bm;
      }
    }

  const uint32_t lens[] = {0, 1, 2, 63, 64, 65, 130};
  const uint32_t caps[] = {0, 1, 4};
  // one endpoint: every case at every queue length and capacity, a few packets of nobody's mixed in
  for (int kind = 0; kind < kKinds; ++kind)
    for (uint32_t L : lens)
      for (uint32_t cap : caps) {
        char what[64];
        snprintf(what, sizeof what, "kind %d L %u cap %u", kind, L, cap);
        check(assemble({scenario(kind, L, cap)}, cap, rnd() % 4), what);
      }
  // m endpoints: 0, 1, 3, 70, the cases and lengths dealt round, state-0 endpoints among them
  for (uint32_t m : {0u, 1u, 3u, 70u})
    for (uint32_t cap : caps)
      for (uint32_t round = 0; round < 3; ++round) {
        std::vector<Endpoint> eps;
        for (uint32_t e = 0; e < m; ++e)
          eps.push_back(scenario((e * 7 + round * 5) % kKinds, lens[(e + round) % 7], cap));
        char what[64];
        snprintf(what, sizeof what, "m %u cap %u round %u", m, cap, round);
        check(assemble(eps, cap, round == 0 ? 0 : rnd() % 70), what);
      }
  // the grid reached every verdict, took runs and left segments parked
  for (int v = 0; v < 12; ++v)
    if (seen[v] == 0) fail("a verdict no case reached", v);
  if (run_lanes < 1000 || parked_left == 0) fail("runs or parked segments missing", run_lanes, parked_left);
  printf("%llu cases ok\n", (unsigned long long)cases);
  return 0;
}
