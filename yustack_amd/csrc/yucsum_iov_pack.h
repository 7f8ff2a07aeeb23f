// yucsum_iov_pack.h — the destination geometry of k_pack, the kernel of the
// packing scatter-gather calls (yu_csum_pack_iov / yu_csum_pack_fill_iov,
// include/yucsum.h): while a packet's views are summed where they lie
// (yucsum_iov.h, unchanged), every byte is also stored at its place in one
// contiguous buffer, Linux's csum_and_copy over a view list.
//
// The source side is the one k_iov has, through the functions the scatter-gather
// kernels share (yucsum_kernels.hip): one packet, one wave; the walk cuts each view
// into slots of 1 KiB whose window starts at floor4(address); lane L holds
// window bytes [16L, 16L + 16) as four dwords. New is where those bytes go.
//
// A slot's window byte x goes to dst address d0 + x (d0: where window byte 0
// would go; for a view's first slot that is up to 3 bytes before the view's
// first byte). With delta = d0 & 3, destination dword J of the slot — the
// 4-aligned dword at (d0 & ~3) + 4J — holds window bytes [4J - delta,
// 4J - delta + 4): the top delta bytes of source dword J - 1 and the low
// 4 - delta bytes of source dword J, one v_alignbyte. Lane L stores
// destination dwords 4L .. 4L + 3 from its own four source dwords and its
// neighbour's last (lane 0: the last dword of the view's previous slot, carried
// over). Destination dword 256 holds the slot's last delta bytes: it is dword 0
// of the view's next slot when the copy goes on there, else lane 63 stores it.
// Everything below is written per lane, in bytes y = x - 16L counted from the
// lane's own window byte 0, so each lane works out its stores from its own
// registers (the kernel keeps the geometry in vector registers).
//
// What is stored of a dword is a byte mask: the bytes inside [lo, hi), the
// slot's share of the view cut to the room the packet has left, less the
// packet's checksum field bytes, which are held back until the value is known
// and then stored once. A full mask is a dword store, anything else 16-bit and
// byte stores: never a read-modify-write, the other bytes of that dword belong
// to another view or another wave's packet. Every destination byte is stored by
// exactly one store.
//
// No HIP call is made here: the kernel and tests/cpp/iov_pack.cpp both use
// these functions.
#ifndef YUCSUM_IOV_PACK_H
#define YUCSUM_IOV_PACK_H

#include "yucsum_iov.h"

#pragma GCC visibility push(hidden)
namespace yu {

// The bytes packet i may store: its own span [o0, min(o1, oN)) of dst, where
// (o0, o1) = dst_offsets[i], dst_offsets[i + 1] and oN = dst_offsets[n]; empty
// when that is no range. More than kIovLimit is never needed.
YU_IOV_FN uint32_t iov_pack_room(uint64_t o0, uint64_t o1, uint64_t oN) {
  const uint64_t e = o1 < oN ? o1 : oN;
  const uint64_t r = e > o0 ? e - o0 : 0;
  return r < kIovLimit ? (uint32_t)r : kIovLimit;
}

// Where a packet goes: dst + dst_offsets[i], and its room. (The kernel keeps
// both in vector registers: they come from a vector load.)
struct IovPackDst {
  uint64_t d;
  uint32_t room;
};

// Packet offset of window byte 0 of the view at addr that starts at packet
// offset off (-3 .. kIovLimit), and of lane L's window byte 0 in the view's slot
// at window offset w (the walk's W.w before iov_walk_slot).
YU_IOV_FN int32_t iov_pack_view(uint64_t addr, uint32_t off) { return (int32_t)off - (int32_t)((uint32_t)addr & 3u); }
YU_IOV_FN int32_t iov_pack_po(int32_t vpk, uint32_t w, uint32_t L) { return vpk + (int32_t)w + (int32_t)(16u * L); }

// What lane L stores of a slot, in bytes y counted from the lane's window byte
// 0: the lane's destination dwords j = 0 .. 3 hold y in [4j - delta, 4j - delta
// + 4) (the first delta of them bytes of the source dword before the lane's
// own), a fifth (lane 63 only: `tail`) the slot's last delta bytes.
struct IovPackPlan {
  uint64_t pa;     // where y = 0 goes; the lane's dword 0 is at pa & ~3
  uint32_t delta;  // pa & 3, the same in every lane of the slot
  int32_t lo, hi;  // y in [lo, hi) is stored: the slot's share of the view, cut to the room
  bool tail;       // lane 63, and the copy does not go on in a next slot
};
YU_IOV_FN void iov_pack_plan(IovPackPlan &P, uint32_t info, const IovPackDst &D, int32_t po, uint32_t L) {
  const int32_t y0 = (int32_t)(16u * L);
  const int32_t lim = (int32_t)iov_lim(info);
  const int32_t left = (int32_t)D.room - (po - y0);  // room from the slot's window byte 0 on
  const int32_t m = lim < left ? lim : left;         // the view's window end, cut to the room
  const bool first = (info & kIovFirst) != 0;
  const int32_t s = (int32_t)((info >> kIovShShift) & 3u);
  const bool live = lim != 0 && m > (first ? s : 0);  // the slot stores something (wave-uniform)
  P.pa = D.d + (uint64_t)(int64_t)po;
  P.delta = (uint32_t)P.pa & 3u;
  P.hi = live ? m - y0 : -(1 << 20);  // below every y of every lane
  P.lo = first ? s - y0 : -4;  // a later slot of a view: from the carried bytes on
  P.tail = L == 63u && m <= (int32_t)kIovSlot;
}

// Which bytes of the lane's destination dword j (0 .. 4) are stored.
YU_IOV_FN uint32_t iov_pack_mask(const IovPackPlan &P, uint32_t j) {
  const int32_t x0 = (int32_t)(4u * j) - (int32_t)P.delta;
  int32_t a = P.lo - x0, b = P.hi - x0;
  a = a < 0 ? 0 : (a > 4 ? 4 : a);
  b = b < 0 ? 0 : (b > 4 ? 4 : b);
  return (0xFu << a) & ~(0xFu << b) & 0xFu;
}
// The field byte at window byte q of the slot: held back when it is stored at
// all (it fits the room), then not stored with the dword that holds it, and
// where it goes.
YU_IOV_FN bool iov_pack_field_held(const IovPackPlan &P, uint32_t q, uint32_t L) {
  return (int32_t)q - (int32_t)(16u * L) < P.hi;
}
YU_IOV_FN uint64_t iov_pack_field_addr(const IovPackPlan &P, uint32_t q, uint32_t L) {
  return P.pa + (uint64_t)(int64_t)((int32_t)q - (int32_t)(16u * L));
}
YU_IOV_FN uint32_t iov_pack_field_clear(const IovPackPlan &P, uint32_t mask, uint32_t j, int32_t q, uint32_t L) {
  const int32_t t = q - (int32_t)(16u * L) + (int32_t)P.delta;
  return q >= 0 && t >= 0 && (uint32_t)(t >> 2) == j ? mask & ~(1u << (t & 3)) : mask;
}

// Destination dword J's bytes from source dwords J - 1 (lo) and J (hi).
YU_IOV_FN uint32_t iov_pack_shift(uint32_t hi, uint32_t lo, uint32_t delta) {
#if defined(__HIP_DEVICE_COMPILE__)
  return delta ? __builtin_amdgcn_alignbyte(hi, lo, 4u - delta) : hi;
#else
  return delta ? (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (4u - delta))) : hi;
#endif
}

// Stores the bytes of v that mask names at the 4-aligned address a: a dword, or
// 16-bit and byte stores. St has b8 / b16 / b32 (address, value).
template <typename St>
YU_IOV_FN void iov_pack_store(St &st, uint64_t a, uint32_t v, uint32_t mask) {
  if (mask == 0xFu) {
    st.b32(a, v);
    return;
  }
  if ((mask & 3u) == 3u) {
    st.b16(a, (uint16_t)v);
  } else {
    if (mask & 1u) st.b8(a, (uint8_t)v);
    if (mask & 2u) st.b8(a + 1u, (uint8_t)(v >> 8));
  }
  if ((mask & 12u) == 12u) {
    st.b16(a + 2u, (uint16_t)(v >> 16));
  } else {
    if (mask & 4u) st.b8(a + 2u, (uint8_t)(v >> 16));
    if (mask & 8u) st.b8(a + 3u, (uint8_t)(v >> 24));
  }
}

// The held-back field bytes, stored once the value is known: b0 / b1 at a0 / a1
// (0: not held). Both held: a1 == a0 + 1, one 16-bit store at an even address.
template <typename St>
YU_IOV_FN void iov_pack_field_store(St &st, uint64_t a0, uint64_t a1, uint32_t b0, uint32_t b1) {
  if (a0 && a1 && (a0 & 1u) == 0) {
    st.b16(a0, (uint16_t)((b0 & 0xFFu) | ((b1 & 0xFFu) << 8)));
  } else {
    if (a0) st.b8(a0, (uint8_t)b0);
    if (a1) st.b8(a1, (uint8_t)b1);
  }
}

// One lane's stores for a slot. c: the lane's four source dwords; prev: the
// source dword before them (the neighbour's last, lane 0: the last of the view's
// slot before); fq0 / fq1: window bytes of the field bytes the slot holds and
// holds back (-1: none).
template <typename St>
YU_IOV_FN void iov_pack_lane(St &st, const IovPackPlan &P, uint32_t L, uint32_t cx, uint32_t cy, uint32_t cz,
                             uint32_t cw, uint32_t prev, int32_t fq0, int32_t fq1) {
  const uint32_t v0 = iov_pack_shift(cx, prev, P.delta), v1 = iov_pack_shift(cy, cx, P.delta);
  const uint32_t v2 = iov_pack_shift(cz, cy, P.delta), v3 = iov_pack_shift(cw, cz, P.delta);
  const uint64_t a = P.pa & ~3ull;
  uint32_t m0 = iov_pack_mask(P, 0), m1 = iov_pack_mask(P, 1), m2 = iov_pack_mask(P, 2), m3 = iov_pack_mask(P, 3);
  m0 = iov_pack_field_clear(P, iov_pack_field_clear(P, m0, 0, fq0, L), 0, fq1, L);
  m1 = iov_pack_field_clear(P, iov_pack_field_clear(P, m1, 1, fq0, L), 1, fq1, L);
  m2 = iov_pack_field_clear(P, iov_pack_field_clear(P, m2, 2, fq0, L), 2, fq1, L);
  m3 = iov_pack_field_clear(P, iov_pack_field_clear(P, m3, 3, fq0, L), 3, fq1, L);
  if ((m0 & m1 & m2 & m3) == 0xFu) {
    st.b128(a, v0, v1, v2, v3);
  } else {
    if (m0) iov_pack_store(st, a, v0, m0);
    if (m1) iov_pack_store(st, a + 4u, v1, m1);
    if (m2) iov_pack_store(st, a + 8u, v2, m2);
    if (m3) iov_pack_store(st, a + 12u, v3, m3);
  }
  if (P.tail && P.delta) {  // the slot's last delta bytes (no field byte lies there)
    const uint32_t m = iov_pack_mask(P, 4);
    if (m) iov_pack_store(st, a + 16u, iov_pack_shift(0u, cw, P.delta), m);
  }
}

// ---------------------------------------------------------------------
// Whole IPv4 datagrams, packed (yu_csum_pack_iov_datagram /
// yu_csum_pack_fill_iov_datagram, the kernel k_pack_dg): the header gather, the
// parse and the epilogue are the datagram kind's (yucsum_iov.h, last section;
// iov_dg_gather, iov_dg_header and iov_dg_out in yucsum_kernels.hip),
// the store side is the one above. The two do not agree on which bytes they
// want: the copy takes every byte of the packet, the sums the header (from the
// gathered lanes) and the window [lo, hi) = [HL, TL) only. So the walk is the
// plain one over whole views, and the window is applied to the sum alone, by
// the slot's place in the packet: a slot inside the window is summed as ever,
// one outside it is not summed, one that straddles lo or hi has each dword's
// bytes masked by packet offset first. The sum stays a sum of the segment's
// own bytes.
//
// With whole views the transport field at f = HL + {6, 16, 2} <= 76 no longer
// lies within 17 bytes of its view's start, so its window byte q (<= 3 + 76)
// needs 7 bits of the info word: iov_walk_view already puts them there (bits
// 23..29, nothing above them is used) and iov_field_q7 reads them. A packet
// offset below 78 lies in the first slot of its view, so do all four bytes
// that are held back in the fill form: 10 and 11 (IPv4's field, whose bytes as
// read are the gather's) and f, f + 1.
// ---------------------------------------------------------------------
YU_IOV_FN uint32_t iov_field_q7(uint32_t info, int k) {
  const uint32_t q = (info >> kIovQShift) & 127u;
  return q + ((k && (info & kIovF0)) ? 1u : 0u);
}

// How the slot whose window byte 0 is packet offset p0 lies to the window
// [lo, hi) (wave-uniform): 0 no byte of it is summed, 1 all of them, 2 some.
YU_IOV_FN int iov_pack_dg_span(uint32_t info, int32_t p0, uint32_t lo, uint32_t hi) {
  const uint32_t lim = iov_lim(info);
  const int32_t s = (info & kIovFirst) ? (int32_t)((info >> kIovShShift) & 3u) : 0;
  const int32_t a = p0 + s, b = p0 + (int32_t)(lim < kIovSlot ? lim : kIovSlot);
  if (lo >= hi || b <= (int32_t)lo || a >= (int32_t)hi) return 0;
  return a >= (int32_t)lo && b <= (int32_t)hi ? 1 : 2;
}

// The bytes of the dword at packet offset x0 (-3 ..) that lie inside [lo, hi).
YU_IOV_FN uint32_t iov_win_mask(int32_t x0, uint32_t lo, uint32_t hi) {
  int32_t a = (int32_t)lo - x0, b = (int32_t)hi - x0;
  a = a < 0 ? 0 : a;
  b = b < 0 ? 0 : b;
  const uint32_t from = a >= 4 ? 0u : ~0u << (8 * a);
  const uint32_t upto = b >= 4 ? ~0u : ~(~0u << (8 * b));
  return from & upto;
}

// Window byte of packet offset x in the slot whose window byte 0 is packet
// offset p0 when the slot stores it (-1: it does not): x lies in the slot's
// share of its view and fits the room. The same answer in every lane.
YU_IOV_FN int32_t iov_pack_dg_held(const IovPackPlan &P, uint32_t info, int32_t p0, uint32_t x, uint32_t L) {
  const int32_t q = (int32_t)x - p0;
  const int32_t s = (int32_t)((info >> kIovShShift) & 3u);
  const bool in = (info & kIovFirst) && q >= s && q - (int32_t)(16u * L) < P.hi;
  return in ? q : -1;
}

// iov_pack_lane with four held-back positions.
YU_IOV_FN uint32_t iov_pack_mask4(const IovPackPlan &P, uint32_t j, uint32_t L, int32_t fq0, int32_t fq1,
                                  int32_t fq2, int32_t fq3) {
  uint32_t m = iov_pack_mask(P, j);
  m = iov_pack_field_clear(P, iov_pack_field_clear(P, m, j, fq0, L), j, fq1, L);
  return iov_pack_field_clear(P, iov_pack_field_clear(P, m, j, fq2, L), j, fq3, L);
}
template <typename St>
YU_IOV_FN void iov_pack_lane4(St &st, const IovPackPlan &P, uint32_t L, uint32_t cx, uint32_t cy, uint32_t cz,
                              uint32_t cw, uint32_t prev, int32_t fq0, int32_t fq1, int32_t fq2, int32_t fq3) {
  const uint32_t v0 = iov_pack_shift(cx, prev, P.delta), v1 = iov_pack_shift(cy, cx, P.delta);
  const uint32_t v2 = iov_pack_shift(cz, cy, P.delta), v3 = iov_pack_shift(cw, cz, P.delta);
  const uint64_t a = P.pa & ~3ull;
  const uint32_t m0 = iov_pack_mask4(P, 0, L, fq0, fq1, fq2, fq3), m1 = iov_pack_mask4(P, 1, L, fq0, fq1, fq2, fq3);
  const uint32_t m2 = iov_pack_mask4(P, 2, L, fq0, fq1, fq2, fq3), m3 = iov_pack_mask4(P, 3, L, fq0, fq1, fq2, fq3);
  if ((m0 & m1 & m2 & m3) == 0xFu) {
    st.b128(a, v0, v1, v2, v3);
  } else {
    if (m0) iov_pack_store(st, a, v0, m0);
    if (m1) iov_pack_store(st, a + 4u, v1, m1);
    if (m2) iov_pack_store(st, a + 8u, v2, m2);
    if (m3) iov_pack_store(st, a + 12u, v3, m3);
  }
  if (P.tail && P.delta) {  // the slot's last delta bytes: window bytes past 1020, no held-back byte
    const uint32_t mt = iov_pack_mask(P, 4);
    if (mt) iov_pack_store(st, a + 16u, iov_pack_shift(0u, cw, P.delta), mt);
  }
}

// Where the held-back byte at packet offset x goes when the packet is done: it
// was held back in its slot exactly when the packet has it and the room takes
// it (0: neither stored there nor here).
YU_IOV_FN uint64_t iov_pack_dg_at(const IovPackDst &D, uint32_t len, uint32_t x) {
  return x < len && x < D.room ? D.d + x : 0ull;
}

// The held-back bytes of a finished packet, stored once (the lead lane). put0 /
// put1: the packet is in contract and the fill form stores bytes 10..11 / the
// transport field (r0 / r1, big-endian); else the bytes as read go back: b10,
// b11 from the gather, fb0, fb1 from the slot that held them. f: the transport
// field's packet offset (0: none was held back).
template <typename St>
YU_IOV_FN void iov_pack_dg_finish(St &st, const IovPackDst &D, uint32_t len, uint32_t f, bool put0, bool put1,
                                  uint32_t r0, uint32_t r1, uint32_t b10, uint32_t b11, uint32_t fb0,
                                  uint32_t fb1) {
  iov_pack_field_store(st, iov_pack_dg_at(D, len, 10u), iov_pack_dg_at(D, len, 11u), put0 ? r0 >> 8 : b10,
                       put0 ? r0 & 0xFFu : b11);
  if (f)
    iov_pack_field_store(st, iov_pack_dg_at(D, len, f), iov_pack_dg_at(D, len, f + 1u), put1 ? r1 >> 8 : fb0,
                         put1 ? r1 & 0xFFu : fb1);
}

}  // namespace yu
#pragma GCC visibility pop

#endif  // YUCSUM_IOV_PACK_H
