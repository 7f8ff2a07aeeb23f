// yucsum_stream.h — the arithmetic of k_stream, the kernel of yu_rx_stream
// (include/yucsum.h): what a TCP endpoint does with its queue of received
// segments. The reference does not deliver the queue; it runs
// receiver.handleRcvdSegment over it (transport/tcp/rcv.go): the acceptability
// test against the window (acceptable, rcv.go:44-52), consumeSegment with its trim
// of bytes already delivered (rcv.go:60-96), the heap of out-of-order segments
// bounded by pendingBufSize (rcv.go:131-145, segment_heap.go), the drain of that
// heap when a gap closes (rcv.go:150-163), FIN, and an ACK for everything that is
// not plain in-order data (sendAck -> getSendParams, rcv.go:100-109). Around it
// stand the gates of handleSegments (RST, the ACK flag, the final ACK check).
//
// The rule is sequential per connection, so the mapping is a wave per endpoint.
// What the 64 lanes buy is the common case: a wave step loads up to 64 queue
// entries, one per lane, and the longest PLAIN RUN at the front of what is left
// (in-order data segments with ACK alone, an open window, an empty heap) is
// taken at once: a prefix sum of the data lengths and a ballot find it, every
// lane of the run stores its own delivered slot and status, and rcv_nxt and
// buf_used advance by the sum. The first entry that breaks the run takes the
// general step, stream_step below, wave-uniform code over the heap in memory;
// then the run test starts again.
//
// All sequence arithmetic is uint32 and wraps; stream_lt is seqnum.LessThan.
//
// The one departure inside the rule: `cap`, a fixed number of heap entries per
// endpoint. A segment that would be parked while pend_count == cap is dropped and
// ACKed as if the byte budget were full; cap == 0 is a receiver that keeps nothing
// out of order.
//
// No HIP call is made here: the kernel, yu_rx_stream_workspace_bytes and
// tests/cpp/rx_stream.cpp all use these functions. The memory behind the tables is
// reached through an Io object (heap entries, statuses, delivered slots) and the
// lanes through a Wave object (the step's loads, the run's prefix sum and ballot,
// the broadcast of one entry), so the walk itself, stream_endpoint, is one text.
#ifndef YUCSUM_STREAM_H
#define YUCSUM_STREAM_H

#include <stdint.h>

#include "yucsum.h"
#include "yucsum_demux.h"
#include "yucsum_group.h"

#pragma GCC visibility push(hidden)
namespace yu {

constexpr uint32_t kStreamPerWave = 64u;   // queue entries per wave step, one per lane
constexpr uint32_t kStreamMaxCap = 1024u;  // heap entries per endpoint at most
constexpr uint32_t kStreamAckBytes = 40u;  // an ACK datagram: 20 + 20, no options, no payload
constexpr uint32_t kStreamTtl = 64u;       // WritePacket's TTL (network/ipv4/ipv4.go:89)
constexpr uint32_t kTcpFin = 1u, kTcpSyn = 2u, kTcpRst = 4u, kTcpAck = 16u;
constexpr uint32_t kStreamOff = 0u, kStreamOpen = 1u, kStreamClosed = 2u, kStreamReset = 3u;

// The scratch of the call: the tile sums of the longer of its two scans, over the
// N + 1 slot offsets (N = n + m * cap) or the m + 1 ACK offsets.
YU_IOV_FN uint64_t stream_workspace_bytes(uint64_t n, uint64_t m, uint64_t cap) {
  if (m > kDemuxMax || n >= (1ull << 32) || cap > kStreamMaxCap) return 0u;
  const uint64_t N = n + m * cap;
  const uint64_t longer = N > m ? N : m;
  return group_align16(8u * group_scan_tiles(longer + 1u));
}

YU_IOV_FN bool stream_lt(uint32_t a, uint32_t b) { return (int32_t)(a - b) < 0; }

// What the walk reads and changes of one endpoint's yu_tcp_rcv, in registers, plus
// what it counts. snd_nxt and wnd_scale only shape the ACK record (stream_ack_word).
struct StreamSt {
  uint32_t rcv_nxt, rcv_acc, pend_used, pend_size, buf_size, buf_used, max_sent_ack, pend_count, state;
  uint32_t n_acks;  // ack() calls of this batch
  uint32_t slots;   // delivered views of this batch
};

// yu_tcp_rcv as ten dwords: word 6 = snd_nxt, word 9 = wnd_scale | state << 8 | reserved << 16.
constexpr uint32_t kStreamStWords = 10u;
constexpr uint32_t kStreamStateByte = 37u;  // offsetof(yu_tcp_rcv, state)
YU_IOV_FN void stream_unpack(StreamSt &S, const uint32_t w[10]) {
  S.rcv_nxt = w[0], S.rcv_acc = w[1], S.pend_used = w[2], S.pend_size = w[3], S.buf_size = w[4];
  S.buf_used = w[5], S.max_sent_ack = w[7], S.pend_count = w[8];
  S.state = (w[9] >> 8) & 0xFFu;
  S.n_acks = 0u, S.slots = 0u;
}
// The words a walk may change, and word k of them as it is stored back; the state
// is a byte store of its own. Nothing else of yu_tcp_rcv is written.
YU_IOV_FN bool stream_word_changes(uint32_t k) { return k < 9u && ((0x1A7u >> k) & 1u); }  // 0, 1, 2, 5, 7, 8
YU_IOV_FN uint32_t stream_pack_word(const StreamSt &S, uint32_t k) {
  switch (k) {
    case 0: return S.rcv_nxt;
    case 1: return S.rcv_acc;
    case 2: return S.pend_used;
    case 5: return S.buf_used;
    case 7: return S.max_sent_ack;
    default: return S.pend_count;
  }
}

// One queue entry as a lane holds it: the packet number, the record's TCP fields
// and the payload view (which still starts with the option bytes); vlen is the
// view's length, 2^32 - 1 for anything longer; fdp = flags | doff << 8 | proto << 16.
struct StreamSeg {
  uint64_t base;
  uint32_t vlen, pkt, seq, fdp;
};
YU_IOV_FN uint32_t stream_fdp(uint32_t flags, uint32_t doff, uint32_t proto) {
  return (flags & 0xFFu) | (doff & 0xFFu) << 8 | (proto & 0xFFu) << 16;
}
YU_IOV_FN uint32_t seg_flags(const StreamSeg &s) { return s.fdp & 0xFFu; }
YU_IOV_FN uint32_t seg_doff(const StreamSeg &s) { return (s.fdp >> 8) & 0xFFu; }
YU_IOV_FN uint32_t seg_proto(const StreamSeg &s) { return (s.fdp >> 16) & 0xFFu; }
// One heap entry, yu_tcp_seg (32 bytes), as the walk holds it: a parked segment is
// at most 65535 bytes, so the length's low dword is the length.
struct StreamEnt {
  uint64_t base;
  uint32_t len, seq, pkt, flags;
};

// Step 3: is the record a TCP segment the rule can read?
YU_IOV_FN bool stream_usable(const StreamSeg &s) {
  return seg_proto(s) == 6u && seg_doff(s) >= 20u && seg_doff(s) - 20u <= s.vlen && s.vlen <= 65535u;
}
YU_IOV_FN uint32_t stream_dlen(const StreamSeg &s) { return s.vlen - (seg_doff(s) - 20u); }

// The run test, the part a lane answers alone: a usable data segment with ACK set
// and RST, FIN and SYN clear. Its data length, 0 for a lane that is not plain.
YU_IOV_FN uint32_t stream_plain_len(const StreamSeg &s) {
  if (!stream_usable(s) || (s.fdp & (kTcpAck | kTcpRst | kTcpFin | kTcpSyn)) != kTcpAck) return 0u;
  return stream_dlen(s);
}
// The part that needs the lanes before it: `before` is the sum of the plain
// lengths from the front of what is left up to this lane. The segment starts
// where those end and the window is open there: then acceptable() holds
// (seq - rcv_nxt == 0 < wnd) and consumeSegment takes it whole.
YU_IOV_FN bool stream_in_run(const StreamSeg &s, uint32_t plain_len, const StreamSt &S, uint32_t before) {
  const uint32_t nxt = S.rcv_nxt + before;
  return plain_len != 0u && s.seq == nxt && S.rcv_acc != nxt;
}
// The wave-uniform part: runs exist only on an open connection with an empty heap.
YU_IOV_FN bool stream_may_run(const StreamSt &S) { return S.state == kStreamOpen && S.pend_count == 0u; }
// The run's length from the ballot of stream_in_run: the lanes k0 .. cnt - 1 are
// what is left of the step, bit l of `ballot` is lane l's answer.
YU_IOV_FN uint32_t stream_run_len(uint64_t ballot, uint32_t k0, uint32_t cnt) {
  if (k0 >= cnt || cnt > kStreamPerWave) return 0u;
  const uint64_t miss = ~(ballot >> k0);  // bit r: lane k0 + r is not in the run; k0 > 0 shifts ones in at the top
  const uint32_t r = miss ? (uint32_t)__builtin_ctzll(miss) : kStreamPerWave;
  return r < cnt - k0 ? r : cnt - k0;
}

// The grid: a wave per endpoint, four to a block, and enough threads for the
// tail's stores, on at most `per_cu` (8: every wave slot) blocks per CU; more
// endpoints stride over it.
YU_IOV_FN uint32_t stream_blocks(uint64_t n, uint64_t m, int cus, uint32_t per_cu) {
  const uint64_t cap = (uint64_t)(cus > 0 ? cus : 1) * (per_cu ? per_cu : 8u);
  uint64_t blocks = (m + 3u) / 4u;
  if (blocks < (n + 255u) / 256u) blocks = (n + 255u) / 256u;
  if (blocks > cap) blocks = cap;
  return (uint32_t)(blocks < 1u ? 1u : blocks);
}

// sendAck -> getSendParams (rcv.go:100-109): the window is reopened from the
// receive buffer's free space and never shrinks.
YU_IOV_FN void stream_ack(StreamSt &S) {
  ++S.n_acks;
  const uint32_t avail = S.buf_used >= S.buf_size ? 0u : S.buf_size - S.buf_used;
  const uint32_t acc = S.rcv_nxt + avail;
  if (stream_lt(S.rcv_acc, acc)) S.rcv_acc = acc;
  S.max_sent_ack = S.rcv_nxt;
}

YU_IOV_FN bool stream_acceptable(const StreamSt &S, uint32_t seq, uint32_t dlen) {
  const uint32_t wnd = S.rcv_acc - S.rcv_nxt;
  if (wnd == 0u) return dlen == 0u && seq == S.rcv_nxt;
  return (uint32_t)(seq - S.rcv_nxt) < wnd || (stream_lt(S.rcv_nxt, seq + dlen) && stream_lt(seq, S.rcv_acc));
}

// Where one endpoint's outputs lie: its delivered slots [slot_lo, slot_hi) of
// s_views, the batch's n for the status index, its heap's capacity.
struct StreamCtx {
  uint64_t slot_lo, slot_hi;
  uint32_t n, cap;  // n < 2^32
};

// The ACK record of an endpoint, word k of 8, from the state the walk left (st,
// ten dwords) and the first three dwords of its id (local address, remote address,
// local_port | remote_port << 16). All zero when the batch owes no ACK.
YU_IOV_FN uint32_t stream_ack_word(const uint32_t st[10], uint32_t n_acks, uint32_t id0, uint32_t id1, uint32_t id2,
                                   uint32_t k) {
  if (n_acks == 0u) return 0u;
  const uint32_t scale = st[9] & 0xFFu;
  const uint32_t w = scale < 32u ? (st[1] - st[0]) >> scale : 0u;
  switch (k) {
    case 0: return id0;
    case 1: return id1;
    case 2: return id2;
    case 3: return st[6];
    case 4: return st[0];
    case 5: return (w < 0xFFFFu ? w : 0xFFFFu) | (kTcpAck << 16) | (20u << 24);
    case 6: return 6u | (kStreamTtl << 8);
    default: return 0u;
  }
}

// Io: this endpoint's heap, i < cap: ld_heap(i), ld_heap_seq(i) (the entry's seq
// alone), st_heap(i, ent), mv_heap(to, from) (the 32 bytes copied as they lie);
// st_status(pkt, v), pkt < n; st_slot(slot, base, len), slot in [slot_lo,
// slot_hi). Every index is compared with its bound HERE, before the Io is called.
template <typename Io>
YU_IOV_FN void stream_status(Io &io, const StreamCtx &C, uint32_t pkt, uint32_t v) {
  if (pkt < C.n) io.st_status(pkt, v);
}

// consumeSegment (rcv.go:60-96). dlen comes back trimmed.
template <typename Io>
YU_IOV_FN bool stream_consume(Io &io, const StreamCtx &C, StreamSt &S, uint32_t seq, uint32_t &dlen, uint64_t base,
                              uint32_t flags) {
  if (dlen > 0u) {
    const uint32_t diff = S.rcv_nxt - seq;
    if (!(diff < dlen)) return false;  // !rcvNxt.InWindow(segSeq, segLen): a segment is missing
    seq += diff, dlen -= diff, base += diff;
    const uint64_t slot = C.slot_lo + S.slots;
    if (slot < C.slot_hi) io.st_slot(slot, base, dlen);
    ++S.slots;
    S.buf_used += dlen;
  } else if (seq != S.rcv_nxt) {
    return false;
  }
  S.rcv_nxt = seq + dlen;
  if (flags & kTcpFin) {
    ++S.rcv_nxt;
    stream_ack(S);
    S.state = kStreamClosed;
  }
  return true;
}

// container/heap over segmentHeap, less = stream_lt on seq. Push: append, sift up.
template <typename Io>
YU_IOV_FN void stream_heap_push(Io &io, const StreamCtx &C, StreamSt &S, const StreamEnt &x) {
  uint32_t j = S.pend_count;
  if (j >= C.cap) return;
  ++S.pend_count;
  for (uint32_t it = 0; it < 32u && j > 0u; ++it) {
    const uint32_t i = (j - 1u) / 2u;
    if (!stream_lt(x.seq, io.ld_heap_seq(i))) break;
    io.mv_heap(j, i);
    j = i;
  }
  io.st_heap(j, x);
}
// Pop: swap first and last, sift down over the first n - 1, drop the last.
template <typename Io>
YU_IOV_FN void stream_heap_pop(Io &io, const StreamCtx &C, StreamSt &S) {
  if (S.pend_count == 0u || S.pend_count > C.cap) return;
  const uint32_t n = --S.pend_count;
  if (n == 0u) return;
  const uint32_t xseq = io.ld_heap_seq(n);  // the last entry goes where the sift ends
  uint32_t i = 0;
  for (uint32_t it = 0; it < 32u; ++it) {
    const uint32_t j1 = 2u * i + 1u;
    if (j1 >= n) break;
    uint32_t j = j1;
    uint32_t cseq = io.ld_heap_seq(j1);
    if (j1 + 1u < n) {
      const uint32_t c2 = io.ld_heap_seq(j1 + 1u);
      if (stream_lt(c2, cseq)) j = j1 + 1u, cseq = c2;
    }
    if (!stream_lt(cseq, xseq)) break;
    io.mv_heap(i, j);
    i = j;
  }
  io.mv_heap(i, n);
}

YU_IOV_FN uint32_t stream_logical(uint32_t dlen, uint32_t flags) {
  return dlen + ((flags & kTcpSyn) ? 1u : 0u) + ((flags & kTcpFin) ? 1u : 0u);
}

// The general step: steps 3 to 10 of the rule for one queue entry on a connection
// that is open or closed. Returns false after RST: handleSegments stops there.
template <typename Io>
YU_IOV_FN bool stream_step(Io &io, const StreamCtx &C, StreamSt &S, const StreamSeg &s) {
  const uint32_t flags = seg_flags(s);
  if (!stream_usable(s)) {
    stream_status(io, C, s.pkt, YU_SEG_NONE);
    return true;
  }
  if (flags & kTcpRst) {
    stream_status(io, C, s.pkt, YU_SEG_RST);
    S.state = kStreamReset;
    return false;
  }
  if (!(flags & kTcpAck)) {
    stream_status(io, C, s.pkt, YU_SEG_IGNORED);
    return true;
  }
  if (S.state == kStreamClosed) {
    stream_status(io, C, s.pkt, YU_SEG_AFTER_CLOSE);
    return true;
  }
  uint32_t dlen = stream_dlen(s);
  const uint64_t base = s.base + (seg_doff(s) - 20u);
  if (!stream_acceptable(S, s.seq, dlen)) {
    stream_ack(S);
    stream_status(io, C, s.pkt, YU_SEG_UNACCEPTABLE);
    return true;
  }
  if (!stream_consume(io, C, S, s.seq, dlen, base, flags)) {
    uint32_t verdict = YU_SEG_NOOP;
    if (dlen > 0u || (flags & kTcpFin)) {
      verdict = YU_SEG_DROPPED;
      if (S.pend_used < S.pend_size && S.pend_count < C.cap) {
        S.pend_used += stream_logical(dlen, flags);
        const StreamEnt x = {base, dlen, s.seq, s.pkt, flags};
        stream_heap_push(io, C, S, x);
        verdict = YU_SEG_PENDING;
      }
      stream_ack(S);
    }
    stream_status(io, C, s.pkt, verdict);
    return true;
  }
  stream_status(io, C, s.pkt, YU_SEG_CONSUMED);
  // the drain (rcv.go:150-163): every turn pops one entry or stops
  for (uint32_t turn = 0; turn <= C.cap && S.state == kStreamOpen && S.pend_count > 0u; ++turn) {
    const StreamEnt t = io.ld_heap(0u);
    uint32_t tl = t.len > 65535u ? 65535u : t.len;
    bool late = false;
    if (!stream_lt(t.seq + tl - 1u, S.rcv_nxt)) {  // not wholly acknowledged already
      if (!stream_consume(io, C, S, t.seq, tl, t.base, t.flags)) break;
      late = true;
    }
    stream_heap_pop(io, C, S);
    S.pend_used -= stream_logical(tl, t.flags);  // the length AFTER consume's trim, as the reference
    if (t.pkt != kDemuxNone) stream_status(io, C, t.pkt, late ? YU_SEG_CONSUMED_LATE : YU_SEG_DUPLICATE);
  }
  return true;
}

// One endpoint's queue order[lo, lo + len) in wave steps; positions are below n <
// 2^32. Wave:
//   load(j0, cnt)   the lanes load the entries j0 .. j0 + cnt - 1 into the NEXT step
//   advance()       the next step becomes the current one
//   run(S, C, k0, cnt, sum)   the plain run from lane k0: its lanes store their slot
//                   (C.slot_lo + S.slots + lane - k0) and YU_SEG_CONSUMED; returns
//                   its length and in `sum` its data bytes
//   fill(k0, cnt, v)  the lanes k0 .. cnt - 1 store status v
//   seg(k)          lane k's entry, for every lane
// and the Io functions. `runs` false forces the general step for every entry.
// S.state at entry is what the connection had before the batch.
template <typename Wave>
YU_IOV_FN void stream_endpoint(Wave &w, const StreamCtx &C, StreamSt &S, uint32_t lo, uint32_t len, bool runs) {
  bool stopped = S.state == kStreamReset;  // handleSegments returned false: nothing more is processed
  const uint32_t other = S.state == kStreamOff ? (uint32_t)YU_SEG_NONE : (uint32_t)YU_SEG_UNPROCESSED;
  if (len) w.load(lo, len < kStreamPerWave ? len : kStreamPerWave);
  for (uint32_t done = 0; done < len;) {
    const uint32_t cnt = len - done < kStreamPerWave ? len - done : kStreamPerWave;
    w.advance();
    done += cnt;
    if (done < len) w.load((uint64_t)lo + done, len - done < kStreamPerWave ? len - done : kStreamPerWave);
    uint32_t k = 0;
    while (k < cnt) {
      if (S.state == kStreamOff || stopped) {
        w.fill(k, cnt, other);
        break;
      }
      if (runs && stream_may_run(S)) {
        uint32_t sum = 0;
        const uint32_t r = w.run(S, C, k, cnt, sum);
        S.rcv_nxt += sum, S.buf_used += sum, S.slots += r;
        k += r;
        if (k >= cnt) break;
      }
      const StreamSeg s = w.seg(k);
      if (!stream_step(w, C, S, s)) stopped = true;
      ++k;
    }
  }
  // handleSegments' last act, unless it returned early (a reset connection, at entry or by now)
  if ((S.state == kStreamOpen || S.state == kStreamClosed) && S.rcv_nxt != S.max_sent_ack) stream_ack(S);
}

}  // namespace yu
#pragma GCC visibility pop

#endif  // YUCSUM_STREAM_H
