// yucsum_iov.h — the arithmetic of k_iov, the kernel of the scatter-gather
// device calls (yu_csum_batch_iov / yu_csum_fill_iov, include/yucsum.h): a
// packet is the concatenation of views that lie anywhere in device memory.
//
// One packet, one wave. The wave walks the packet's views and cuts them into
// load slots: a slot is up to 1 KiB (64 lanes x 16 bytes) of one view's window,
// which starts at floor4(base) as every window of yucsum_kernels.hip does. A
// step of the kernel is U slots, so a header view and the start of the payload
// view are in flight together. Each slot's dwords are summed as little-endian
// 16-bit halves (one v_sad_u16 per dword), head and tail bytes masked.
//
// Combining views. Swapping the bytes of a 16-bit word multiplies it by 256
// modulo 65535, so a view's big-endian contribution to the packet's sum is
// congruent to swap16(fold(S_LE)) when the view's bytes pair up the same way in
// memory as in the packet — (address parity XOR the view's byte offset in the
// packet) even — and to fold(S_LE) as it is when odd: the le_to_be rule of
// yucsum_kernels.hip with the packet offset in place of "even start". Both maps
// are linear modulo 65535, so the lanes keep two sums, one per class, over all
// views, and the packet's residue is swap16(fold(A)) + fold(B). A packet is at
// most kIovLimit bytes, so neither sum can wrap and the reference's uint32
// cannot either: the residue and zero-ness are all its result depends on.
// fold() maps a sum to 0 only when it is 0, so the value is 0x0000 only when
// everything summed is zero, as in the reference (0xFFFF for a nonzero sum
// congruent to 0).
//
// The TX checksum field (two bytes at packet offset f, possibly in two views)
// is found by the walk; its bytes are read out of the registers holding them
// and taken off the sum of their view's class, exactly, before folding.
//
// The kernel's whole-datagram kind (yu_csum_batch_iov_datagram /
// yu_csum_fill_iov_datagram) adds a header gather, a parse and a window to the
// walk: the last section of this file.
//
// No HIP call is made here: the kernel and tests/cpp/iov_combine.cpp (the
// datagram kind: tests/cpp/iov_datagram.cpp) both use these functions.
#ifndef YUCSUM_IOV_H
#define YUCSUM_IOV_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YU_IOV_FN __host__ __device__ __forceinline__
#else
#define YU_IOV_FN inline
#endif

#pragma GCC visibility push(hidden)
namespace yu {

constexpr uint32_t kIovLimit = 65535u;  // == YU_MAX_TRANSPORT_LEN: bytes per packet, every mode
constexpr uint32_t kIovSlot = 1024u;    // bytes one load slot covers (64 lanes x 16)

// A slot's `info` word: the window bytes left from the slot's base on (17 bits),
// then what the sum needs to know about its view.
constexpr uint32_t kIovLimMask = 0x1FFFFu;
constexpr uint32_t kIovFirst = 1u << 17;  // the view's first slot: head bytes, field bytes
constexpr uint32_t kIovSwap = 1u << 18;   // the view's class: its LE sum is byte-swapped
constexpr uint32_t kIovF0 = 1u << 19;     // the slot holds the field's first byte, at window byte q
constexpr uint32_t kIovF1 = 1u << 20;     // the field's second byte (at q + 1 when it holds both)
constexpr uint32_t kIovShShift = 21;      // 2 bits: base & 3
constexpr uint32_t kIovQShift = 23;       // 5 bits: q <= 3 + 17

struct IovSlot {
  uint64_t base;  // 4-aligned address the slot's descriptor starts at
  uint32_t info;  // 0: an empty slot, nothing is loaded
};

// The walk over one packet's views (wave-uniform).
struct IovWalk {
  uint64_t base;   // the current view's window base, floor4(address)
  uint32_t E;      // the window's end: (address & 3) + the view's bytes taken
  uint32_t w;      // window offset of the view's next slot; w >= E: the view is used up
  uint32_t flags;  // the info bits of the view's next slot
  uint32_t off;    // packet bytes in the views started so far (<= kIovLimit)
  uint32_t over;   // a view did not fit under kIovLimit: the packet is out of contract
  uint64_t fp[2];  // addresses of the packet's two field bytes (valid once off >= f + 2)
};

YU_IOV_FN void iov_walk_reset(IovWalk &W) {
  W.base = 0;
  W.E = 0;
  W.w = 0;
  W.flags = 0;
  W.off = 0;
  W.over = 0;
  W.fp[0] = 0;
  W.fp[1] = 0;
}

YU_IOV_FN bool iov_walk_done(const IovWalk &W) { return W.w >= W.E; }

// Starts the view [addr, addr + len) (the previous one is used up). Bytes past
// kIovLimit are not taken. A TX mode's field is the two bytes at packet offset
// f (tx false: no field). A view with nothing to take (len 0, any addr) is done
// at once.
YU_IOV_FN void iov_walk_view(IovWalk &W, uint64_t addr, uint64_t len, bool tx, uint32_t f) {
  const uint32_t room = kIovLimit - W.off;
  const uint32_t take = len <= room ? (uint32_t)len : room;
  if (len > room) W.over = 1u;
  const uint32_t s = (uint32_t)addr & 3u;
  W.base = addr & ~3ull;
  W.E = take ? s + take : 0u;
  W.w = 0;
  uint32_t fl = kIovFirst | (s << kIovShShift);
  if ((((uint32_t)addr ^ W.off) & 1u) == 0) fl |= kIovSwap;
  if (tx) {
    const uint32_t lo = W.off, hi = W.off + take;
    const bool h0 = f >= lo && f < hi, h1 = f + 1u >= lo && f + 1u < hi;
    if (h0) {
      fl |= kIovF0 | ((s + f - lo) << kIovQShift);
      W.fp[0] = addr + (f - lo);
    }
    if (h1) {
      fl |= kIovF1;
      if (!h0) fl |= (s + f + 1u - lo) << kIovQShift;
      W.fp[1] = addr + (f + 1u - lo);
    }
  }
  W.flags = fl;
  W.off += take;
}

// The next slot of the current view, or an empty one when it is used up.
YU_IOV_FN void iov_walk_slot(IovWalk &W, IovSlot &S) {
  if (W.w < W.E) {
    S.base = W.base + W.w;
    S.info = (W.E - W.w) | W.flags;
    W.flags &= kIovSwap;
    W.w += kIovSlot;
  } else {
    S.base = 0;
    S.info = 0;
  }
}

YU_IOV_FN uint32_t iov_lim(uint32_t info) { return info & kIovLimMask; }

// Bytes of the slot's dword 0 that belong to the view (all but the head bytes
// of a first slot).
YU_IOV_FN uint32_t iov_head_mask(uint32_t info) {
  const uint32_t s = (info >> kIovShShift) & 3u;
  return (info & kIovFirst) ? ~((1u << (8u * s)) - 1u) : ~0u;
}

// The dword x at slot offset cr (a multiple of 4), cut to the view's bytes:
// whole if it ends by lim, its first lim & 3 bytes if it straddles lim, nothing
// past it; dword 0 also loses the head bytes.
YU_IOV_FN uint32_t iov_dword(uint32_t x, uint32_t cr, uint32_t lim, uint32_t hm) {
  const uint32_t F = lim & ~3u;
  x = cr < F ? x : (cr == F ? (x & ((1u << (8u * (lim & 3u))) - 1u)) : 0u);
  return cr == 0u ? (x & hm) : x;
}

// Sum of the two little-endian 16-bit halves of x, added to acc (v_sad_u16).
YU_IOV_FN uint32_t iov_add(uint32_t x, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sad_u16(x, 0u, acc);
#else
  return acc + (x & 0xFFFFu) + (x >> 16);
#endif
}

// Where a slot's field bytes sit: k = 0 / 1 for the field's first / second
// byte. Window byte q of the slot is byte q & 3 of dword (q >> 2) & 3 of the
// chunk of lane q >> 4.
YU_IOV_FN bool iov_has_field(uint32_t info, int k) { return (info & (k ? kIovF1 : kIovF0)) != 0; }
YU_IOV_FN uint32_t iov_field_q(uint32_t info, int k) {
  const uint32_t q = (info >> kIovQShift) & 31u;
  return q + ((k && (info & kIovF0)) ? 1u : 0u);
}
// What the byte (dword `word` holds it) at window byte q added to the LE sum.
YU_IOV_FN uint32_t iov_field_term(uint32_t word, uint32_t q) {
  return ((word >> (8u * (q & 3u))) & 0xFFu) << (8u * (q & 1u));
}

// ChecksumCombine(uint16(v), uint16(v >> 16)): 0 only for v == 0.
YU_IOV_FN uint32_t iov_fold(uint32_t v) {
  const uint32_t w = (v & 0xFFFFu) + (v >> 16);
  return (w + (w >> 16)) & 0xFFFFu;
}

// The packet's big-endian residue from the two class sums (A: swapped).
YU_IOV_FN uint32_t iov_residue(uint32_t A, uint32_t B) {
  const uint32_t r = iov_fold(A);
  return (((r & 0xFFu) << 8) | (r >> 8)) + iov_fold(B);
}

// Big-endian 16-bit words of a dword read from memory, summed.
YU_IOV_FN uint32_t iov_be_words(uint32_t x) {
  return (((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu)) + (((x >> 16) & 0xFFu) << 8) + (x >> 24);
}

// The epilogue (packet_value of yucsum_kernels.hip for this form's modes): v is
// the packet's residue, len its length; pseudo header from the {src, dst}
// record (a, b) when have_addrs, else `initial` (the packet's initial_arr entry
// or the scalar); complemented for the TX modes.
YU_IOV_FN uint32_t iov_value(int mode, uint32_t v, uint32_t len, bool have_addrs, uint32_t a,
                             uint32_t b, uint32_t initial) {
  const bool pseudo = mode == 1 || mode == 2 || mode == 6 || mode == 7;  // UDP, TCP, VERIFY_TCP, VERIFY_UDP
  const bool tx = mode == 1 || mode == 2 || mode == 4;                   // UDP, TCP, ICMP
  if (mode == 0) {  // RAW
    v += initial;
  } else if (pseudo) {
    const uint32_t proto = (mode == 2 || mode == 6) ? 6u : 17u;
    const uint32_t ph = have_addrs ? iov_be_words(a) + iov_be_words(b) + proto : initial;
    v += ph + (len & 0xFFFFu);
  }
  const uint32_t r = iov_fold(v);
  return tx ? (~r) & 0xFFFFu : r;
}

// The modes the scatter-gather form takes (whole-packet sums), and the offset
// of the field its TX modes take as zero.
YU_IOV_FN bool iov_mode_ok(int m) { return m == 0 || m == 1 || m == 2 || m == 4 || m == 6 || m == 7; }
YU_IOV_FN bool iov_mode_tx(int m) { return m == 1 || m == 2 || m == 4; }
YU_IOV_FN uint32_t iov_mode_field(int m) { return m == 1 ? 6u : (m == 2 ? 16u : (m == 4 ? 2u : 0u)); }

// ---------------------------------------------------------------------
// Whole IPv4 datagrams (yu_csum_batch_iov_datagram / yu_csum_fill_iov_datagram):
// IPV4, VERIFY_IPV4, VERIFY_RX and TX_DATAGRAM parse the header out of the
// packet. Lane j < 60 of the wave holds packet byte j (a byte load from the view
// that holds it, issued a packet ahead); the parse reads bytes 0, 2, 3 and 9,
// the IPv4 header's big-endian sum over b[:min(HL, len)] and the pseudo
// header's over bytes 12..19 are sums over the lanes (iov_dg_term: byte j weighs
// 256 when j is even), and the transport segment is the walk above with a
// window: of each view only the bytes at packet offsets [HL, TL) are cut into
// slots. HL is a multiple of 4, so a byte's class (address parity XOR its
// offset in the packet) is its class in the segment, and the transport field
// is the field mechanism above at f = HL + {6 UDP, 16 TCP, 2 ICMP}. The
// segment's sum is a sum of its own bytes only, never a difference of
// residues, so it is 0 exactly when every byte of it is zero.
// ---------------------------------------------------------------------
constexpr uint32_t kIovHdr = 60u;  // header bytes the lanes gather: IHL <= 15

YU_IOV_FN bool iov_dg_mode_ok(int m) { return m == 3 || m == 5 || m == 8 || m == 9; }  // IPV4, VERIFY_IPV4, VERIFY_RX, TX_DATAGRAM
YU_IOV_FN bool iov_dg_mode_tx(int m) { return m == 3 || m == 9; }                       // the two that store fields

// What the parse of a packet's first bytes fixes before its walk starts.
struct IovDg {
  uint32_t lo, hi;  // the walk's window of packet offsets (lo == hi: nothing is summed)
  uint32_t f;       // TX_DATAGRAM: the transport field's packet offset (0: none)
  uint32_t tl;      // TotalLength()
  uint32_t meta;    // HL | bytes of the header sum << 6 | Protocol() << 12 | kIovDgOk | kIovDgL4
};
constexpr uint32_t kIovDgOk = 1u << 20;  // len >= 20 and HL <= TL (TX_DATAGRAM: and HL >= 20); TL <= len is known after the walk
constexpr uint32_t kIovDgL4 = 1u << 21;  // ... and the protocol is TCP, UDP or ICMP
YU_IOV_FN uint32_t iov_dg_hl(uint32_t meta) { return meta & 63u; }
YU_IOV_FN uint32_t iov_dg_hn(uint32_t meta) { return (meta >> 6) & 63u; }
YU_IOV_FN uint32_t iov_dg_proto(uint32_t meta) { return (meta >> 12) & 0xFFu; }

// have = min(len, kIovHdr); b0, b2, b3, b9: packet bytes 0, 2, 3, 9 (anything
// where the packet is shorter).
YU_IOV_FN void iov_dg_parse(IovDg &D, int mode, uint32_t have, uint32_t b0, uint32_t b2, uint32_t b3,
                            uint32_t b9) {
  const uint32_t hl = have ? (b0 & 15u) * 4u : 0u;      // HeaderLength()
  const uint32_t hn = hl < have ? hl : have;            // b[:IHL*4], clamped to the packet
  const uint32_t tl = ((b2 & 0xFFu) << 8) | (b3 & 0xFFu);
  const uint32_t proto = b9 & 0xFFu;
  const bool walk = mode == 8 || mode == 9;
  const bool ok = have >= 20u && hl <= tl && (mode != 9 || hl >= 20u);
  const bool l4 = ok && (proto == 6u || proto == 17u || proto == 1u);
  uint32_t lo = 0, hi = 0, f = 0;
  if (walk && l4) {
    lo = hl;
    hi = tl;
    if (mode == 9) {  // the field exists when the segment holds its fixed header
      const uint32_t fo = proto == 17u ? 6u : (proto == 6u ? 16u : 2u);
      const uint32_t mn = proto == 17u ? 8u : (proto == 6u ? 20u : 4u);
      if (tl - hl >= mn) f = hl + fo; else hi = lo;
    }
  }
  D.lo = lo;
  D.hi = hi;
  D.f = f;
  D.tl = tl;
  D.meta = hl | (hn << 6) | (proto << 12) | (ok ? kIovDgOk : 0u) | (l4 ? kIovDgL4 : 0u);
}

// What packet byte j (lane j) adds to a big-endian sum that starts at an even offset.
YU_IOV_FN uint32_t iov_dg_term(uint32_t j, uint32_t byte) { return (j & 1u) ? (byte & 0xFFu) : ((byte & 0xFFu) << 8); }
// Lane j's share of the IPv4 header's sum (field bytes 10, 11 taken as zero in
// the modes that store them, when the summed bytes hold both: of an 11-byte
// packet byte 10 is summed as it is) and of the pseudo header's {src, dst}.
YU_IOV_FN uint32_t iov_dg_hdr_term(uint32_t meta, int mode, uint32_t j, uint32_t byte) {
  const bool fld = iov_dg_mode_tx(mode) && iov_dg_hn(meta) >= 12u && (j == 10u || j == 11u);
  return j < iov_dg_hn(meta) && !fld ? iov_dg_term(j, byte) : 0u;
}
YU_IOV_FN uint32_t iov_dg_pseudo_term(uint32_t j, uint32_t byte) {
  return j >= 12u && j < 20u ? iov_dg_term(j, byte) : 0u;
}

// iov_walk_view with the window [lo, hi) of packet offsets: of the view's bytes
// only those inside it are cut into slots (none: the view is done at once and
// costs no slot); W.off and W.over count the whole view as ever.
YU_IOV_FN void iov_walk_view_win(IovWalk &W, uint64_t addr, uint64_t len, uint32_t lo, uint32_t hi,
                                 bool tx, uint32_t f) {
  const uint32_t off = W.off, room = kIovLimit - off;
  const uint32_t take = len <= room ? (uint32_t)len : room;
  const uint32_t over = W.over | (len > room ? 1u : 0u);
  const uint32_t end = off + take;
  const uint32_t a = off > lo ? off : lo, b = end < hi ? end : hi;
  const bool in = a < b;
  W.off = in ? a : off;
  iov_walk_view(W, in ? addr + (a - off) : addr, in ? b - a : 0u, tx, f);
  W.off = end;
  W.over = over;
}

// The epilogue. len: the packet's bytes; hs, ps: the lanes' header and pseudo
// sums; (sA, sB): the window's class sums, the field's bytes taken off. r0 / r1:
// the results (r1: TX_DATAGRAM's transport value); st0 / st1: whether the fill
// form stores the field (bytes 10..11 / the transport field at D.f).
YU_IOV_FN void iov_dg_value(const IovDg &D, int mode, uint32_t len, uint32_t hs, uint32_t ps, uint32_t sA,
                            uint32_t sB, uint32_t &r0, uint32_t &r1, bool &st0, bool &st1) {
  const uint32_t meta = D.meta, hl = iov_dg_hl(meta), proto = iov_dg_proto(meta);
  const uint32_t ip = iov_fold(hs);
  const bool valid = (meta & kIovDgOk) && D.tl <= len;
  uint32_t seg = iov_residue(sA, sB);
  if (proto != 1u) seg += ps + proto + ((D.tl - hl) & 0xFFFFu);  // ICMP has no pseudo header
  seg = iov_fold(seg);
  r0 = r1 = 0;
  st0 = st1 = false;
  if (mode == 5) {  // VERIFY_IPV4
    r0 = ip;
  } else if (mode == 3) {  // IPV4
    r0 = (~ip) & 0xFFFFu;
    st0 = iov_dg_hn(meta) >= 12u;
  } else if (mode == 8) {  // VERIFY_RX
    if (!valid) {
      r0 = 8u;  // YU_RX_INVALID
    } else {
      if (ip == 0u || ip == 0xFFFFu) r0 |= 1u;  // YU_RX_IP_OK
      if (meta & kIovDgL4) {
        r0 |= 2u;                                     // YU_RX_L4
        if (seg == 0u || seg == 0xFFFFu) r0 |= 4u;    // YU_RX_L4_OK
      }
    }
  } else if (valid) {  // TX_DATAGRAM
    r0 = (~ip) & 0xFFFFu;
    st0 = true;
    if (D.f) {
      r1 = (~seg) & 0xFFFFu;
      st1 = true;
    }
  }
}

}  // namespace yu
#pragma GCC visibility pop

#endif  // YUCSUM_IOV_H
