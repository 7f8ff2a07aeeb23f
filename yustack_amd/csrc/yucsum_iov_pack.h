// yucsum_iov_pack.h — the destination geometry of k_pack, the kernel of the
// packing scatter-gather calls (yu_csum_pack_iov / yu_csum_pack_fill_iov,
// include/yucsum.h): while a packet's views are summed where they lie
// (yucsum_iov.h, unchanged), every byte is also stored at its place in one
// contiguous buffer, Linux's csum_and_copy over a view list.
//
// The source side is k_iov's: one packet, one wave; the walk cuts each view
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

}  // namespace yu
#pragma GCC visibility pop

#endif  // YUCSUM_IOV_PACK_H
