// yucsum_kernels.hip — gfx950 (MI355X, CDNA4, wave64) kernels for yustack's
// per-packet Internet checksum, and the batched device entry points of
// include/yucsum.h.
//
// Semantics reproduced (reference paths relative to /root/reference):
//   Checksum                checksum/checksum.go:4-18
//   ChecksumCombine         checksum/checksum.go:32-35
//   PseudoHeaderChecksum    checksum/checksum.go:24-28
//   compositions            transport/udp/endpoint.go:164-187,
//                           transport/tcp/connect.go:556-586,
//                           network/ipv4/ipv4.go:80-97, network/ipv4/icmp.go:36-45,
//                           checker/checker.go:25-40,71-99
//
// Arithmetic. The reference adds big-endian 16-bit words into a uint32 that
// wraps mod 2^32 and folds once (ChecksumCombine). Two exact formulations:
//
//  * LE (default). Sum the little-endian 16-bit halves of every 32-bit word
//    with v_sad_u16 — ONE VALU op per 4 bytes — into a uint32 S_LE. Swapping
//    the bytes of a 16-bit word multiplies it by 256 modulo 65535, so the
//    big-endian sum S_BE is congruent to swap16(fold(S_LE)) when the packet
//    starts at an even address (to fold(S_LE) when it starts at an odd one),
//    and S_BE is 0 exactly when S_LE is. The reference's result depends on
//    S_BE only through that residue and zero-ness as long as its uint32 does
//    not wrap, i.e. for buffers <= 131072 bytes: every transport/IPv4/ICMP
//    packet and every RAW packet up to that size.
//  * BE (RAW packets that may exceed 131072 bytes). v_perm_b32 turns each
//    16-bit half into the big-endian word first; the uint32 sum then equals
//    the reference's accumulator bit for bit, wrap included (addition mod
//    2^32 is order-free).
//
// Layout. A packet [s, e) is read through 16-byte loads (buffer_load_dwordx4)
// from a window that starts at floor4(s): every chunk but the last lies
// inside the packet and is summed unmasked; the last chunk's dwords are kept
// iff they start before e. The few bytes this gets wrong — up to 3 bytes
// before an unaligned s, up to 3 after an unaligned e, and in TX modes the
// two checksum-field bytes that Encode() zeroes — sit in at most four known
// dwords; the group leader gathers them from the registers of the lanes
// holding them (one cross-lane read each) and subtracts their masked bytes.
// No byte is loaded twice.
//
// Loads go through buffer descriptors based at wave-uniform addresses: a lane
// that must not load passes an out-of-range offset and gets zeros without a
// memory access, so no load sits in an exec-masked block and the compiler's
// vmcnt bookkeeping stays exact. That lets the kernels keep the next step's
// loads in flight while the current step is summed (software pipelining).
//
// Work mapping (wave64-first, not a warp tiling). Which kernel a batch gets
// depends on its layout, mode, packet size and count (yu::plan in
// yucsum_plan.cpp, each cut-over measured):
//   k_lane<U>: dense uniform 4-aligned packets up to 112 bytes (configs 2 and
//     8): 64 whole strides per wave step parked in LDS, one lane per packet
//     summing it from there.
//   k_tiny<G>: uniform 4-aligned packets <= 16G bytes that k_lane does not take
//     (113..128 bytes, sparse small ones): a wave step covers 64 packets, each
//     load instruction one contiguous KiB, and a cross-lane transpose lets
//     every lane finish one packet.
//   k_small<G, U>: uniform stride, packet span <= G*U*16 bytes (705..3072 and
//     sparse ones). A wave holds 64/G packets per step; each group of G lanes
//     loads its packet window in U dwordx4 loads per lane, reduces with log2(G)
//     DPP adds and its last lane finishes the packet (config 3: k_small<16,6>).
//     Dense read-only batches on k_small<16,6> load a step's packets as whole
//     128-byte lines and repack them through LDS instead (yucsum_dense.h).
//   k_seg<U, NT, K, CH>: ragged batches of more than 4096 packets, VERIFY_RX,
//     and dense uniform packets of other sizes: a segmented sum over the byte
//     stream of CH consecutive packets per wave (64, or 16 below 64K packets),
//     U KiB tiles, packet sums as prefix differences (config 4, tun RX). Its
//     TXW kind writes ragged TX batches in place, storing the fields of each
//     chunk's last tile as whole 128-byte lines.
//   k_hdr<NT>: the IPv4 header-only modes (<= 60 bytes of each packet), uniform
//     and ragged: one lane per packet, 32-byte reads.
//   k_loop<U, BE> / k_loop_rx<U>: one wave per packet, for ragged bursts of up
//     to 4096 packets and for few or sparse uniform packets > 4 KiB.
//   k_iov<U, NT, FILL, DG>: scatter-gather packets (yu_csum_batch_iov / yu_csum_fill_iov,
//     planned by yu::plan_wave): one wave per packet walking its views, each step U
//     load slots of 1 KiB of whichever view comes next (yucsum_iov.h). DG: whole IPv4
//     datagrams (yu_csum_batch_iov_datagram / yu_csum_fill_iov_datagram): the header
//     gathered into the lanes a packet ahead, the walk windowed to [HL, TL).
//   k_pack<U, NT, FILL>: the packing scatter-gather calls (yu_csum_pack_iov /
//     yu_csum_pack_fill_iov, planned by yu::plan_wave): k_iov's walk and sums,
//     and every byte stored once at its place in one contiguous buffer
//     (yucsum_iov_pack.h).
//   k_pack_dg<U, NT, FILL>: the same for whole IPv4 datagrams
//     (yu_csum_pack_iov_datagram / yu_csum_pack_fill_iov_datagram): k_iov's header
//     gather, parse and epilogue, k_pack's store side over the plain walk, the window
//     [HL, TL) applied to the sum alone.
//   k_build<U, NT>: yu_tx_build_ragged (planned by yu::plan_wave): one wave per
//     outgoing datagram, the payload as a single view through k_pack's store side,
//     the header encoded and summed from a 32-byte record and stored last
//     (yucsum_build.h).
//   k_split<U, NT>: yu_rx_split_ragged (planned by yu::plan_wave): one wave per
//     received datagram, its first 80 bytes one dword per lane for the parse, the
//     record and the header sums, the payload [HL + H, TL) as a single view
//     through k_pack's store side (yucsum_split.h). k_build and k_split walk
//     their one range with the same function, range_walk.
//   k_parse<VERIFY, NT>: yu_rx_parse_ragged's header pass (planned by
//     yu::plan_parse): one lane per received datagram, k_split's record and
//     YU_RX_SPLIT from the packet's first 80 bytes and a view onto the payload,
//     which is neither read nor copied (yucsum_parse.h).
//   k_demux<FLAGS, COUNT, NT>: yu_rx_demux (planned by yu::plan_demux): one lane
//     per record those two store, the three table lookups of the transport
//     demultiplexer, the endpoint's index per packet and one counter add per
//     distinct endpoint of a wave step (yucsum_demux.h).
//   k_group_*: yu_rx_group (planned by yu::plan_group): the packet numbers
//     grouped by endpoint as a stable radix partition, a block histogram, a
//     device-wide scan and a scatter per pass, and the CSR and the grouped view
//     table after it (yucsum_group.h). A block per tile, not grid-stride.
//   k_reply<FLAGS, NT>: yu_rx_reply (planned by yu::plan_reply): one lane per
//     received packet, the echo's record and length from the packet's record,
//     view, flags and endpoint; k_group_scan_* then turn the lengths into the
//     replies' offsets (yucsum_reply.h).
//   k_build_iov<U, NT>: yu_tx_build_iov (k_build's plan row): k_build with each
//     payload behind a view, an empty destination span a skipped packet.
//   k_stream<RUNS>, k_stream_fin: yu_rx_stream (grid: yu::stream_blocks): a wave
//     per endpoint runs the TCP receiver over the endpoint's queue, 64 entries per
//     wave step, in-order runs taken whole; then a lane per element makes the ACK
//     records and the tail, and k_group_scan_* the offsets (yucsum_stream.h).
//   All others are grid-stride kernels; the grid is sized per CU and over-subscribed
//   (see blocks_per_cu in yucsum_plan.cpp), except that k_seg narrows it for
//   small packets (seg_waves).
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "yucsum.h"
#include "yucsum_build.h"
#include "yucsum_demux.h"
#include "yucsum_dense.h"
#include "yucsum_group.h"
#include "yucsum_internal.h"
#include "yucsum_iov.h"
#include "yucsum_iov_pack.h"
#include "yucsum_parse.h"
#include "yucsum_plan.h"
#include "yucsum_reply.h"
#include "yucsum_split.h"
#include "yucsum_stream.h"

namespace {

constexpr uint32_t kSelSwap = 0x02030001u;  // bytes [1,0,3,2]: BE 16-bit halves
constexpr uint32_t kSelIdent = 0x03020100u; // bytes [0,1,2,3]
using yu::kLEMax;

struct BatchArgs {
  const uint8_t *data;
  const uint64_t *offsets;  // ragged: n+1 offsets; nullptr: uniform
  const uint16_t *initial_arr;
  const uint8_t *addrs;
  uint16_t *out;
  uint8_t *fill;  // non-null: write the field into the packet (== data)
  uint64_t stride;
  uint64_t n;
  uint64_t end;   // one past the batch's last byte (uniform); ragged: 0
  uint32_t len;
  uint32_t initial;
  uint32_t uf;    // k_small: steps u < uf hold only full chunks
  uint32_t xcd;   // 1: XCD-aware block order (grid_wave)
  uint32_t small_waves;  // k_seg: waves that work on small-packet batches (seg_waves)
  int mode;
};

__host__ __device__ __forceinline__ bool mode_is_ipv4(int m) {
  return m == YU_MODE_IPV4 || m == YU_MODE_VERIFY_IPV4;
}
using yu::l4_field;  // protocol tables shared with the host writer (yucsum_internal.h)
using yu::l4_min;
using yu::mode_field;
using yu::mode_fills;
using yu::mode_is_tx;
__host__ __device__ __forceinline__ bool mode_has_pseudo(int m) {
  return m == YU_MODE_UDP || m == YU_MODE_TCP || m == YU_MODE_VERIFY_TCP ||
         m == YU_MODE_VERIFY_UDP;
}
__host__ __device__ __forceinline__ uint32_t mode_proto(int m) {
  return (m == YU_MODE_TCP || m == YU_MODE_VERIFY_TCP) ? 6u : 17u;
}
__host__ __device__ __forceinline__ uint32_t min_len(int m) {
  switch (m) {
    case YU_MODE_UDP: return 8;    // UDPMinimumSize
    case YU_MODE_TCP: return 20;   // TCPMinimumSize
    case YU_MODE_ICMP: return 4;   // ICMPv4MinimumSize
    case YU_MODE_IPV4:
    case YU_MODE_VERIFY_IPV4: return 1;  // byte 0 holds IHL
    default: return 0;
  }
}

// ChecksumCombine(uint16(v), uint16(v>>16)) — checksum/checksum.go:17,32-35
__device__ __forceinline__ uint32_t fold32(uint32_t v) {
  uint32_t w = (v & 0xFFFFu) + (v >> 16);
  return (w + (w >> 16)) & 0xFFFFu;
}

__device__ __forceinline__ uint32_t sad(uint32_t x, uint32_t acc) {
  return __builtin_amdgcn_sad_u16(x, 0u, acc);
}

__device__ __forceinline__ uint32_t sadperm(uint32_t x, uint32_t sel,
                                            uint32_t acc) {
  return __builtin_amdgcn_sad_u16(__builtin_amdgcn_perm(x, x, sel), 0u, acc);
}

template <bool BE>
__device__ __forceinline__ uint32_t add_word(uint32_t x, uint32_t sel,
                                             uint32_t acc) {
  return BE ? sadperm(x, sel, acc) : sad(x, acc);
}

// Residue of the packet's big-endian word sum, from the LE sum of a packet
// starting at an address of parity `odd` (see the header comment).
__device__ __forceinline__ uint32_t le_to_be(uint32_t s_le, uint32_t odd) {
  const uint32_t r = fold32(s_le);
  return odd ? r : (((r & 0xFFu) << 8) | (r >> 8));
}

// Sum over each aligned group of G lanes; the total lands in the group's
// LAST lane (lane % G == G-1). DPP row shifts inside 16-lane rows, then
// row_bcast15/31 across rows — VALU only, no LDS traffic.
template <int G>
__device__ __forceinline__ uint32_t group_total(uint32_t v) {
  static_assert(G >= 1 && G <= 64 && (G & (G - 1)) == 0, "G must be a power of two");
  if (G >= 2) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);  // row_shr:1
  if (G >= 4) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);  // row_shr:2
  if (G >= 8) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);  // row_shr:4
  if (G >= 16) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true); // row_shr:8
  if (G >= 32) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); // row_bcast:15
  if (G >= 64) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); // row_bcast:31
  return v;
}

// OR over the whole wave, in every lane (the same DPP steps as group_total<64>,
// then lane 63's value handed round in a VGPR: the caller is short of SGPRs).
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return (uint32_t)__shfl((int)v, 63, 64);
}

// This wave's index in the grid's packet order. Blocks are dealt round-robin
// over the 8 XCDs (blocks b and b+8 share an L2), so with xcd set the order is
// swizzled to give each XCD a contiguous run of logical blocks: the one
// 128-byte line two neighbouring packets (or 64-packet chunks) share is then
// fetched by a single L2, at about the same time, instead of by two. Bijective
// for any grid size (XCDs x < n%8 hold one block more). Speed only: no
// correctness depends on where a block runs. Off by default (see use_xcd).
__device__ __forceinline__ uint64_t grid_wave(uint32_t xcd) {
  const uint32_t b = blockIdx.x, n = gridDim.x;
  uint32_t lb = b;
  if (xcd) {
    const uint32_t x = b & 7u, i = b >> 3, q = n >> 3, r = n & 7u;
    lb = (x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q) + i;
  }
  return (uint64_t)lb * (blockDim.x >> 6) +
         (uint64_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Wave-uniform 64-bit value (only for values uniform by construction): puts
// buffer bases in SGPRs so no waterfall loop is generated.
__device__ __forceinline__ uint64_t uniform64(uint64_t x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, uint32_t l) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, 64);
  return ((uint64_t)hi << 32) | lo;
}

// Out-of-range offset: the load returns zeros and touches no memory.
using yu::kOOB;

// Descriptor over [base, min(ceil4(end), base + 2 GiB)). The range check is
// per dword (a dword reaching past num_records reads as 0), so the extent is
// rounded up to the dword holding the batch's last byte: loads never leave
// that dword, let alone the allocation.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_at(uint64_t base,
                                                          uint64_t end) {
  end = (end + 3u) & ~3ull;
  const uint64_t n = end > base ? end - base : 0;
  return __builtin_amdgcn_make_buffer_rsrc((void *)base, (short)0,
                                           (int)(n < kOOB ? n : kOOB), 0x00020000);
}

// Load policy. Packet bytes are read once, and non-temporal (nt, aux bit 1)
// loads stream them fastest, but an nt line does not stay in L2, so the line
// two neighbouring packets share is fetched twice. NT = 0: plain loads;
// 1: all nt; 2 (default): nt except the first and last step of a window,
// which hold the shared lines.
__device__ __forceinline__ uint4 bld16(__amdgpu_buffer_rsrc_t r, uint32_t off,
                                       bool nt) {
  const u32x4 t = nt ? __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 2)
                     : __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
  return make_uint4(t.x, t.y, t.z, t.w);
}

template <int NT>
__device__ __forceinline__ constexpr bool nt_step(int u, int U) {
  return NT == 1 || (NT == 2 && u != 0 && u != U - 1);
}

// ---------------------------------------------------------------------
// Junk: bytes of dwords the dword-granular sum includes but the reference
// does not, other than the unaligned tail (masked in sum_masked). Window
// coordinates (window base = floor4(packet start)); sh = start & 3; E = sh +
// summed length. Item 0: the head bytes [0, sh) of dword 0; items 1/2: the
// TX checksum field [sh+f, sh+f+2) (Encode writes 0 there), which may
// straddle two dwords. All lie in the window's first 24 bytes, i.e. in chunk
// 0 or 1 of step 0, and are read from the registers of the lanes holding
// them — never with an extra load.
// ---------------------------------------------------------------------
struct Junk {
  uint32_t off[3];   // window-relative dword offsets
  uint32_t mask[3];  // bytes to subtract (0 when the item is absent)
};

__device__ __forceinline__ Junk make_junk(uint32_t sh, uint32_t E, int mode) {
  Junk j;
  j.off[0] = 0u;
  j.mask[0] = (1u << (8u * sh)) - 1u;  // 0 for sh == 0
  const uint32_t f = mode_field(mode);
  const bool fld = mode_is_tx(mode) && sh + f + 2u <= E;
  const uint32_t fr = sh + f;
  const uint32_t fb = fr & 3u;
  j.off[1] = fr & ~3u;
  j.mask[1] = !fld ? 0u : (fb == 3u ? 0xFF000000u : (0xFFFFu << (8u * fb)));
  j.off[2] = (fr & ~3u) + 4u;
  j.mask[2] = (fld && fb == 3u) ? 0xFFu : 0u;
  return j;
}

__device__ __forceinline__ uint32_t pick_dword(const uint4 &c, uint32_t q) {
  return q == 0 ? c.x : (q == 1 ? c.y : (q == 2 ? c.z : c.w));
}

// Junk dwords of the group whose first lane is `gbase` (G = 1 << LG lanes;
// chunk k = off/16 is held by lane gbase + k in step 0; c0 = this lane's
// step-0 chunk). Every lane offers the dword its own group asks for, so all
// lanes must execute it.
template <int LG>
__device__ __forceinline__ void junk_take(const uint4 &c0, uint32_t gbase,
                                          const Junk &j, uint32_t (&x)[3]) {
  static_assert(LG >= 1, "junk chunks 0/1 must sit in different lanes of step 0");
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t d = j.off[k];
    x[k] = __shfl(pick_dword(c0, (d >> 2) & 3u), (int)(gbase + (d >> 4)), 64);
  }
}

template <bool BE>
__device__ __forceinline__ uint32_t junk_sum(const uint32_t (&x)[3],
                                             const Junk &j, uint32_t sel) {
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) s = add_word<BE>(x[k] & j.mask[k], sel, s);
  return s;
}

// ---------------------------------------------------------------------
// Per-packet side data (uint16 initial or the 8-byte {src,dst} record),
// fetched together with the packet bytes so the epilogue never waits on a
// dependent load. Absent arrays read a zero word with stride 0, so the side
// loads are unconditional too.
// ---------------------------------------------------------------------
__device__ uint32_t g_side_zero[2] = {0u, 0u};

struct Side {
  uint32_t a, b;
  uint16_t i;  // 16-bit: widened at its use, not right after its load
};

struct SidePtrs {
  const uint8_t *a;
  const uint8_t *i;
  uint32_t as, is;
};

__device__ __forceinline__ SidePtrs side_ptrs(const BatchArgs &A) {
  SidePtrs s;
  const bool use_addrs = A.addrs && mode_has_pseudo(A.mode);
  s.a = use_addrs ? A.addrs : (const uint8_t *)g_side_zero;
  s.as = use_addrs ? 8u : 0u;
  s.i = A.initial_arr ? (const uint8_t *)A.initial_arr : (const uint8_t *)g_side_zero;
  s.is = A.initial_arr ? 2u : 0u;
  return s;
}

__device__ __forceinline__ Side load_side(const SidePtrs &sp, uint64_t p) {
  const uint32_t *a = (const uint32_t *)(sp.a + p * sp.as);
  Side s;
  s.a = a[0];
  s.b = a[1];
  s.i = *(const uint16_t *)(sp.i + p * sp.is);
  return s;
}

// Per-packet epilogue. `v` is the packet's word sum (exact uint32 for BE,
// its residue for LE). Adds the non-payload terms of the reference
// composition, folds, complements, stores (and optionally sets the field).
__device__ __forceinline__ uint32_t packet_value(const BatchArgs &A, uint32_t v, uint64_t len,
                                                 const Side &sd) {
  const int mode = A.mode;
  if (mode == YU_MODE_RAW) {
    v += A.initial_arr ? sd.i : A.initial;
  } else if (mode_has_pseudo(mode)) {
    uint32_t ph;
    if (A.addrs) {
      // PseudoHeaderChecksum(proto, src, dst): src/dst big-endian words + proto
      ph = sadperm(sd.a, kSelSwap, 0u);
      ph = sadperm(sd.b, kSelSwap, ph);
      ph += mode_proto(mode);
    } else {
      ph = A.initial_arr ? sd.i : A.initial;
    }
    // + Checksum(BE16(uint16(length))) — header/udp.go:70-72, tcp.go:168-170
    v += ph + (uint32_t)(len & 0xFFFFu);
  }
  uint32_t r = fold32(v);
  if (mode_is_tx(mode)) r = (~r) & 0xFFFFu;
  return r;
}

// The field value r stored big-endian into the packet (TX fill), if the
// field lies inside the first hdr_end bytes.
__device__ __forceinline__ void store_field(const BatchArgs &A, uint32_t r, uint8_t *pkt,
                                            uint32_t hdr_end) {
  const int mode = A.mode;
  if (A.fill && pkt && mode_is_tx(mode)) {
    const uint32_t f = mode_field(mode);
    if (f + 2u <= hdr_end) {
      // binary.BigEndian.PutUint16: one 16-bit store when the field is
      // 2-aligned (always, for the 4-aligned uniform fill), else two bytes
      // Uniform batches store it non-temporally (72-B datagrams: 42.5 -> 36.4 us
      // per 1M; ragged ones measured mixed, tools/kbench KB_FILL=1).
      uint8_t *q = pkt + f;
      const uint16_t be = (uint16_t)((r >> 8) | (r << 8));
      if (((uintptr_t)q & 1u) == 0 && !A.offsets) {
        __builtin_nontemporal_store(be, (uint16_t *)q);
      } else if (((uintptr_t)q & 1u) == 0) {
        *(uint16_t *)q = be;
      } else {
        q[0] = (uint8_t)(r >> 8);
        q[1] = (uint8_t)r;
      }
    }
  }
}

// The batch's extent: the call may touch data[0, offsets[n]) (ragged; offsets
// index the caller's data array), everything for uniform batches (whose geometry
// the host checked). One scalar load per wave.
struct Extent {
  uint64_t hi;
};
__device__ __forceinline__ Extent batch_extent(const BatchArgs &A) {
  Extent e;
  e.hi = A.offsets ? A.offsets[A.n] : ~0ull;
  return e;
}

// The packet [off, off + len) whose field a fill call may write: none when not
// filling, or when the packet is out of contract: longer than
// YU_MAX_TRANSPORT_LEN (decreasing offsets wrap its length there too) or ending
// past offsets[n] (outside what the call may touch: some other packet's offsets
// decrease). Such a packet gets an unspecified value and no byte is written for
// it (include/yucsum.h, "Out of contract"). Every fill mode is a transport /
// IPv4 / ICMP / datagram mode, so the limit is the transport one.
__device__ __forceinline__ uint8_t *fill_at(const BatchArgs &A, const Extent &x, uint64_t off,
                                            uint64_t len) {
  const bool in = len <= YU_MAX_TRANSPORT_LEN && off <= x.hi && len <= x.hi - off;
  return A.fill && in ? A.fill + off : nullptr;
}

__device__ __forceinline__ void finish_packet(const BatchArgs &A, uint64_t p,
                                              uint32_t v, uint64_t len,
                                              const Side &sd, uint8_t *pkt,
                                              uint32_t hdr_end) {
  const uint32_t r = packet_value(A, v, len, sd);
  if (A.out) A.out[p] = (uint16_t)r;
  store_field(A, r, pkt, hdr_end);
}

// Chunk c at window offset cr, cut at the packet end E: dword j (window
// offset cr + 4j) is whole if it ends by E, keeps its first E&3 bytes (tm) if
// it straddles E, and is dropped otherwise. lim[j] = floor4(E) - 4j (signed:
// may be negative).
__device__ __forceinline__ uint32_t tail_cut(uint32_t x, int cr, int lim,
                                             uint32_t tm) {
  return cr < lim ? x : (cr == lim ? (x & tm) : 0u);
}

template <bool BE>
__device__ __forceinline__ uint32_t sum_masked(const uint4 &c, int cr,
                                               const int (&lim)[4], uint32_t tm,
                                               uint32_t sel, uint32_t acc) {
  acc = add_word<BE>(tail_cut(c.x, cr, lim[0], tm), sel, acc);
  acc = add_word<BE>(tail_cut(c.y, cr, lim[1], tm), sel, acc);
  acc = add_word<BE>(tail_cut(c.z, cr, lim[2], tm), sel, acc);
  acc = add_word<BE>(tail_cut(c.w, cr, lim[3], tm), sel, acc);
  return acc;
}

template <bool BE>
__device__ __forceinline__ uint32_t sum_full(const uint4 &c, uint32_t sel,
                                             uint32_t acc) {
  acc = add_word<BE>(c.x, sel, acc);
  acc = add_word<BE>(c.y, sel, acc);
  acc = add_word<BE>(c.z, sel, acc);
  acc = add_word<BE>(c.w, sel, acc);
  return acc;
}

// IPv4 modes: HeaderLength() = (b[0] & 0xf) * 4 (header/ipv4.go:91-93); b[0]
// is byte sh of dword 0 of the window, held by the group's first lane.
__device__ __forceinline__ uint32_t ipv4_hl(uint32_t w0, uint32_t sh) {
  return ((w0 >> (8u * sh)) & 0xFu) * 4u;
}

// Orders one wave's LDS accesses (its slice is its own: no block barrier).
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------
// k_small<G, U, NT>: uniform stride, whole packet window in one step,
// software-pipelined: the loads of step t+1 are issued before step t is
// summed, reduced and stored.
// ---------------------------------------------------------------------
template <int G, int U>
struct SmallItem {
  uint4 c[U];
  Side sd;
  uint32_t sh, len;
};

// Fetch the windows of packets pb+gw (pb = the wave's first packet of the
// step; pb >= n fetches nothing). Dense (wave-uniform; yucsum_dense.h): the
// same U loads per lane, but of the step's whole byte range, line-aligned:
// c[u] then holds chunk 64u + lane of that range, and small_repack turns it
// into the window's chunk before the step is summed.
template <int G, int U, int NT, bool SIDE = true>
__device__ __forceinline__ void small_fetch(const BatchArgs &A,
                                            const SidePtrs &sp, uint64_t pb,
                                            uint32_t gw, uint32_t gl, bool ipv4,
                                            bool dense, SmallItem<G, U> &it) {
  const uint64_t p = pb + gw;
  const bool active = p < A.n;
  const uint64_t data = (uint64_t)(uintptr_t)A.data;
  const uint64_t wbase = (data + pb * A.stride) & ~3ull;
  const uint64_t sabs = data + (active ? p : pb) * A.stride;
  it.sh = (uint32_t)(sabs & 3u);
  it.len = active ? A.len : 0u;
  const uint32_t le = ipv4 ? (it.len < 60u ? it.len : 60u) : it.len;
  // Load u of a lane is at x = x0 + u * dx of its range (this group's window),
  // at buffer offset add + x if x < lim
  uint64_t b = wbase;
  uint32_t x0 = 16u * gl, dx = 16u * G;
  uint32_t lim = active ? it.sh + le : 0u;
  uint32_t add = (uint32_t)((sabs & ~3ull) - wbase);
  if (yu::dense_inst(G, U) && dense) {  // the step's range, counted from ds.lo
    const yu::DenseStep ds = yu::dense_step(data, A.len, A.n, pb, 64 / G);
    b = ds.base;
    x0 = yu::dense_x0(ds, gw * G + gl);
    dx = yu::kDensePiece;
    lim = yu::dense_lim(ds);
    add = ds.lo;
  }
  const __amdgpu_buffer_rsrc_t r = rsrc_at(uniform64(b), A.end);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t x = x0 + (uint32_t)u * dx;
    it.c[u] = bld16(r, x < lim ? add + x : kOOB, nt_step<NT>(u, U));
  }
  if (SIDE) it.sd = load_side(sp, active ? p : A.n - 1);
}

// Dense fetch, second half: park the step's U pieces in the wave's LDS slice
// (a mirror of the step's range) and read each group's window, which begins
// `wo` bytes into the slice, back into the layout the window path loads: c[u]
// = chunk gl + G*u of the window. A chunk holding the packet's end brings the
// bytes after it along, as there; a chunk past the end, zero there, holds
// whatever follows in LDS here: both are masked below (the packet starts
// 4-aligned and is whole dwords, so sum_masked drops every dword from the end
// on, and steps below uf hold no such chunk). W dwords per read: windows
// start 4W-aligned (wave-uniform, see k_small). The last group's window may
// reach past the slice, into those masked bytes: the next wave's slice, or
// the array's pad (yu::dense_pad).
template <int G, int U, int W>
__device__ __forceinline__ void small_repack(SmallItem<G, U> &it, uint4 *slice, uint32_t wo,
                                             uint32_t lane, uint32_t gl) {
#pragma unroll
  for (int u = 0; u < U; ++u) slice[64 * u + lane] = it.c[u];
  wave_lds_fence();
  const uint8_t *win = (const uint8_t *)slice + wo + 16u * gl;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint8_t *q = win + 16 * G * u;
    if (W == 4) {
      it.c[u] = *(const uint4 *)q;
    } else if (W == 2) {
      const uint2 a = *(const uint2 *)q, b = *(const uint2 *)(q + 8);
      it.c[u] = make_uint4(a.x, a.y, b.x, b.y);
    } else {
      const uint32_t *d = (const uint32_t *)q;
      it.c[u] = make_uint4(d[0], d[1], d[2], d[3]);
    }
  }
  wave_lds_fence();  // the next step's stores stay behind these reads
}

// PR (packets per run): 0 = wave w's step t takes packets (w + t*waves)*GPW on
// (the grid's waves interleave over the batch); PR > 0 = wave w takes PR
// consecutive packets in PR/GPW steps, then the run w + waves and so on. A
// run's side records (PR * 8 or 2 bytes) come in with one load by lanes
// 0..PR-1 when its first step is fetched, and its results leave in one store
// (PR * 2 bytes) after its last step: per-step side loads and result stores
// are small scattered requests, and a wave's loads return in order, so one
// slow side load holds up the packet bytes behind it.
// The dense instances are held to the 5 waves per SIMD (96 VGPRs) they had
// before the repack, which the allocator otherwise gives up (113, 4 waves).
template <int G, int U, int NT, int PR = 0>
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(yu::dense_inst(G, U) ? 5 : 1))) void k_small(BatchArgs A) {
  constexpr int GPW = 64 / G;
  constexpr int SPR = PR ? PR / GPW : 1;  // steps per run
  static_assert(PR == 0 || (PR % GPW == 0 && PR <= 64 && (SPR & (SPR - 1)) == 0),
                "a run is whole wave steps and fits the wave's lanes");
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t gl = lane & (G - 1);
  const uint32_t gw = lane / G;
  const uint64_t wave = grid_wave(A.xcd);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const int mode = A.mode;
  const bool ipv4 = mode_is_ipv4(mode);
  const SidePtrs sp = side_ptrs(A);
  const uint32_t uf = A.uf;
  // Dense fetch (G, U of yu::dense_inst only: the others hold no LDS)
  constexpr bool kDense = yu::dense_inst(G, U);
  uint4 *slice = nullptr;
  if constexpr (kDense) {
    __shared__ uint4 park[4 * 64 * U + yu::dense_pad(G, U) / 16];
    slice = park + 64 * U * __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  }
  const bool dense = kDense && yu::dense_ok(G, U, (uint64_t)(uintptr_t)A.data, A.offsets != nullptr,
                                            A.stride, A.len, A.fill != nullptr, ipv4);
  // first packet of the wave's step t
  auto first = [&](uint64_t t) -> uint64_t {
    if (PR == 0) return (wave + t * nwaves) * GPW;
    return (wave + t / SPR * nwaves) * PR + (t % SPR) * GPW;
  };

  uint64_t t = 0;
  uint64_t pb = first(0);
  if (pb >= A.n) return;
  uint32_t res = 0;  // PR: lane s < PR collects the run's result s
  Side rs, nrs;      // PR: the current / next run's side record of packet `lane`
  // Where a run's side records sit. G <= 16 (a group within one DPP row): the
  // record of step j for group g is loaded by the group's lane G-1-j, so the
  // group's last lane, which finishes the packet, holds step 0's and a row_shr:1
  // after each step brings the next one to it (no LDS permute). G > 16: lane s
  // loads the run's record s, fetched with a permute each step.
  constexpr bool kDppSide = G <= 16;
  auto run_side = [&](uint64_t q, Side &d) __attribute__((always_inline)) {
    uint64_t x = q + lane;  // lanes >= PR read the run's first record again
    bool own = lane < (uint32_t)PR;
    if (kDppSide) {
      const uint32_t jj = (uint32_t)(G - 1) - gl;  // step whose record this lane holds
      x = q + (uint64_t)jj * GPW + gw;
      own = jj < (uint32_t)SPR;
    }
    d = load_side(sp, own && x < A.n ? x : (q < A.n ? q : A.n - 1));
  };
  // One step: issue the loads of the next step into `nx`, then sum `it` and
  // finish its packets. Returns false when the wave has no next step. The
  // loop below alternates two items instead of copying nx into it: a copy
  // would wait for the prefetch to land before the back-edge.
  auto step = [&](SmallItem<G, U> &it, SmallItem<G, U> &nx) __attribute__((always_inline)) -> bool {
    const uint64_t pn = first(t + 1);
    const bool more = pn < A.n;  // wave-uniform
    const uint32_t k = (uint32_t)(t % SPR);
    const uint64_t p = pb + gw;
    small_fetch<G, U, NT, PR == 0>(A, sp, more ? pn : A.n, gw, gl, ipv4, dense, nx);
    if (PR && k == 0 && t) rs = nrs;  // after the prefetch: the copy waits for nrs only
    if (PR && k == SPR - 1 && more) run_side(pn, nrs);
    if (kDense && dense) {
      const uint32_t wo = p < A.n ? yu::dense_window((uint64_t)(uintptr_t)A.data, A.len, pb, gw) : 0u;
      // widest LDS read the windows' alignment allows (data is 16-aligned)
      if ((A.len & 15u) == 0) small_repack<G, U, 4>(it, slice, wo, lane, gl);
      else if ((A.len & 7u) == 0) small_repack<G, U, 2>(it, slice, wo, lane, gl);
      else small_repack<G, U, 1>(it, slice, wo, lane, gl);
    }

    uint32_t E = it.sh + it.len;
    if (ipv4) {
      const uint32_t hl = __shfl(ipv4_hl(it.c[0].x, it.sh), (int)(lane & ~(uint32_t)(G - 1)), 64);
      E = it.sh + (it.len < hl ? it.len : hl);
    }
    const int F = (int)(E & ~3u);
    const int lim[4] = {F, F - 4, F - 8, F - 12};
    const uint32_t tm = (1u << (8u * (E & 3u))) - 1u;
    uint32_t acc = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int cr = 16 * (int)(gl + (uint32_t)u * G);
      if ((uint32_t)u < uf)
        acc = sum_full<false>(it.c[u], 0u, acc);
      else
        acc = sum_masked<false>(it.c[u], cr, lim, tm, 0u, acc);
    }
    const Junk j = make_junk(it.sh, E, mode);
    uint32_t jx[3] = {0u, 0u, 0u};
    if (PR && kDppSide) {
      // the junk dwords lie in step 0's chunks of the group's first lanes: each
      // lane takes its own share off its partial sum before the reduction
      uint32_t own = 0;
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if ((j.off[i] >> 4) == gl) own = sad(pick_dword(it.c[0], (j.off[i] >> 2) & 3u) & j.mask[i], own);
      acc -= own;
    } else {
      junk_take<__builtin_ctz(G)>(it.c[0], lane & ~(uint32_t)(G - 1), j, jx);
    }
    acc = group_total<G>(acc);
    if (PR == 0) {
      if (gl == G - 1 && p < A.n) {
        const uint32_t v = le_to_be(acc - junk_sum<false>(jx, j, 0u), it.sh & 1u);
        finish_packet(A, p, v, it.len, it.sd,
                      A.fill ? A.fill + p * A.stride : nullptr, E - it.sh);
      }
    } else {
      // the group's side record: in its last lane (G <= 16, then shifted on for
      // the next step), else from the lane that loaded it for the run
      Side sd;
      if (kDppSide) {
        sd = rs;
        rs.a = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)rs.a, 0x111, 0xf, 0xf, true);  // row_shr:1
        rs.b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)rs.b, 0x111, 0xf, 0xf, true);
        rs.i = (uint16_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)rs.i, 0x111, 0xf, 0xf, true);
      } else {
        const int src = (int)(k * GPW + gw);
        sd.a = (uint32_t)__shfl((int)rs.a, src, 64);
        sd.b = (uint32_t)__shfl((int)rs.b, src, 64);
        sd.i = (uint16_t)__shfl((int)rs.i, src, 64);
      }
      // every lane computes; the group's last lane holds the true value
      const uint32_t v = le_to_be(acc - (kDppSide ? 0u : junk_sum<false>(jx, j, 0u)), it.sh & 1u);
      const uint32_t r = packet_value(A, v, it.len, sd);
      if (gl == G - 1 && p < A.n && A.fill) store_field(A, r, A.fill + p * A.stride, E - it.sh);
      const uint32_t got = (uint32_t)__shfl((int)r, (int)((lane % GPW) * G + G - 1), 64);
      res = lane / GPW == k ? got : res;
      if (k == SPR - 1 || !more) {
        const uint64_t q = pb - (uint64_t)k * GPW + lane;  // the run's packet `lane`
        if (lane < (uint32_t)PR && q < A.n && A.out) A.out[q] = (uint16_t)res;
      }
    }
    pb = pn;
    ++t;
    return more;
  };
  SmallItem<G, U> a, b;
  small_fetch<G, U, NT, PR == 0>(A, sp, pb, gw, gl, ipv4, dense, a);
  if (PR) run_side(pb, rs);
  for (;;) {
    if (!step(a, b)) break;
    if (!step(b, a)) break;
  }
}

// ---------------------------------------------------------------------
// k_tiny<G, NT>: uniform stride, packets of <= 16G bytes starting 4-byte
// aligned: RAW, the TX modes UDP / TCP / ICMP (field masked in place) and
// VERIFY_TCP / VERIFY_UDP — every mode without a per-packet header walk.
// For tiny packets k_small spends a whole per-packet epilogue on every 1 KiB
// loaded; here a wave step covers 64 packets (G KiB): group g (G lanes) loads
// chunk j of G packets (slot k holds packet pb + (64/G)k + g, so each load
// instruction reads 64/G consecutive packets = one contiguous KiB). After the
// per-slot group sums, a cross-lane transpose gives slot j's total to lane j
// of the group, and all 64 lanes finish one packet each.
// ---------------------------------------------------------------------
template <int G>
struct TinyItem {
  uint4 c[G];
  Side sd;  // side data of the packet this lane finishes
};

template <int G, int NT>
__device__ __forceinline__ void tiny_fetch(const BatchArgs &A, const SidePtrs &sp,
                                           uint64_t pb, uint32_t g, uint32_t j,
                                           TinyItem<G> &it) {
  constexpr uint32_t GPW = 64 / G;
  const uint64_t base = uniform64((uint64_t)(uintptr_t)A.data + pb * A.stride);
  const __amdgpu_buffer_rsrc_t r = rsrc_at(base, A.end);
  const bool in = 16u * j < A.len;
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const uint32_t q = GPW * (uint32_t)k + g;  // packet pb + q
    const bool active = in && pb + q < A.n;
    it.c[k] = bld16(r, active ? (uint32_t)(q * A.stride) + 16u * j : kOOB, NT != 0);
  }
  const uint64_t pf = pb + GPW * j + g;
  it.sd = load_side(sp, pf < A.n ? pf : A.n - 1);
}

// Every lane of each G-lane group gets the value of the group's last lane.
template <int G>
__device__ __forceinline__ uint32_t bcast_last(uint32_t v, uint32_t lane) {
  if (G == 4)  // quad_perm [3,3,3,3]
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xFF, 0xf, 0xf, false);
  return (uint32_t)__shfl(v, (int)(lane | (G - 1)), 64);
}

// Fill with whole chunks (k_tiny): lane (g, f/16) of slot k holds the field
// chunk of packet pb + (64/G)k + g, whose value lane (g, k) computed. It patches
// the field in its register copy, and every slot goes back out with the same
// offsets it was loaded from. Only when no chunk reaches into the next packet
// (stride >= the 16-byte-rounded length), and never past the batch's last whole
// dword (the last packet's partial tail dword holds no field).
template <int G>
__device__ __forceinline__ void tiny_store(const BatchArgs &A, uint64_t pb, uint32_t g, uint32_t j,
                                           const TinyItem<G> &it, uint32_t be, uint32_t f) {
  constexpr uint32_t GPW = 64 / G;
  const uint64_t e4 = A.end & ~3ull;  // packets start 4-aligned (fill contract)
  const uint32_t fd = (f >> 2) & 3u, sh = (f & 2u) * 8u;
  const uint32_t m = 0xFFFFu << sh;
  const bool holder = j == (f >> 4);
  const bool in = 16u * j < A.len;
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const uint32_t v = ((uint32_t)__shfl((int)be, (int)(g * G + (uint32_t)k), 64)) << sh;
    uint4 c = it.c[k];
    if (holder) {
      c.x = fd == 0 ? (c.x & ~m) | v : c.x;
      c.y = fd == 1 ? (c.y & ~m) | v : c.y;
      c.z = fd == 2 ? (c.z & ~m) | v : c.z;
      c.w = fd == 3 ? (c.w & ~m) | v : c.w;
    }
    const uint64_t q = pb + GPW * (uint32_t)k + g;
    uint32_t *dst = (uint32_t *)(A.fill + q * A.stride + 16u * j);
    const uint64_t da = (uint64_t)(uintptr_t)dst;
    if (in && q < A.n) {
      if (da + 16u <= e4) {
        *(uint4 *)dst = c;
      } else {  // the batch's last chunk: whole dwords only
        if (da + 4u <= e4) dst[0] = c.x;
        if (da + 8u <= e4) dst[1] = c.y;
        if (da + 12u <= e4) dst[2] = c.z;
      }
    }
  }
}

template <int G, int NT, bool WB = false>
__global__ __launch_bounds__(256) void k_tiny(BatchArgs A) {
  constexpr uint32_t GPW = 64 / G;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = lane & (G - 1);
  const uint32_t g = lane / G;
  const uint64_t wave = grid_wave(A.xcd);
  const uint64_t step = (uint64_t)gridDim.x * (blockDim.x >> 6) * 64u;
  const SidePtrs sp = side_ptrs(A);
  const uint32_t E = A.len;  // window base = packet start (4-aligned)
  const int F = (int)(E & ~3u);
  const int lim[4] = {F, F - 4, F - 8, F - 12};
  const uint32_t tm = (1u << (8u * (E & 3u))) - 1u;
  const bool full = A.uf != 0;  // every chunk of every packet is whole
  // TX modes: Encode leaves the checksum field 0. Starts are 4-aligned and the
  // field offset is even, so the field is 16 bits of one dword: chunk f/16,
  // dword (f%16)/4 — masked in the lanes that load that chunk.
  const uint32_t f = mode_field(A.mode);
  const uint32_t fm = (mode_is_tx(A.mode) && j == f / 16u) ? ~(0xFFFFu << (8u * (f & 3u))) : ~0u;
  const uint32_t fd = (f >> 2) & 3u;
  const uint4 m4 = make_uint4(fd == 0 ? fm : ~0u, fd == 1 ? fm : ~0u, fd == 2 ? fm : ~0u,
                              fd == 3 ? fm : ~0u);
  // fill with whole chunks (tiny_store): its own instantiation, so the plain
  // kernel keeps its registers
  const bool wb = WB && A.fill && A.stride >= ((A.len + 15u) & ~15u);

  uint64_t pb = wave * 64u;
  if (pb >= A.n) return;
  TinyItem<G> it;
  tiny_fetch<G, NT>(A, sp, pb, g, j, it);
  for (;;) {
    const uint64_t pn = pb + step;
    const bool more = pn < A.n;  // wave-uniform
    TinyItem<G> nx;
    tiny_fetch<G, NT>(A, sp, more ? pn : A.n, g, j, nx);

    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const uint4 c = make_uint4(it.c[k].x & m4.x, it.c[k].y & m4.y, it.c[k].z & m4.z,
                                 it.c[k].w & m4.w);
      uint32_t acc = full ? sum_full<false>(c, 0u, 0u)
                          : sum_masked<false>(c, 16 * (int)j, lim, tm, 0u, 0u);
      acc = bcast_last<G>(group_total<G>(acc), lane);
      mine = (j == (uint32_t)k) ? acc : mine;
    }
    const uint64_t pf = pb + GPW * j + g;
    if (wb) {
      const uint32_t r = packet_value(A, le_to_be(mine, 0u), E, it.sd);
      if (pf < A.n && A.out) A.out[pf] = (uint16_t)r;
      tiny_store<G>(A, pb, g, j, it, ((r >> 8) | (r << 8)) & 0xFFFFu, f);
    } else if (pf < A.n) {
      finish_packet(A, pf, le_to_be(mine, 0u), E, it.sd, A.fill ? A.fill + pf * A.stride : nullptr, E);
    }
    if (!more) break;
    it = nx;
    pb = pn;
  }
}

// ---------------------------------------------------------------------
// k_lane<U, NT>: uniform, 4-aligned packets of 65..16U bytes with
// len <= stride <= 16U — the sizes where k_tiny<8> leaves lanes idle (a
// 72-byte UDP datagram fills 5 of its 8 chunks) and k_small pays a group
// reduction per packet. A wave step covers 64 packets, i.e. the contiguous
// 64*stride bytes from packet pb on: U coalesced dwordx4 loads per lane,
// parked in the wave's own LDS slice (no block barrier: LDS operations of one
// wave complete in order). Each lane then sums its own packet from LDS, one
// ds_read_b32 per dword, starting at dword lane % nd so that lanes whose
// packets start on the same bank read different banks.
// ---------------------------------------------------------------------
template <int U>
__device__ __forceinline__ void lane_fetch(const BatchArgs &A, const SidePtrs &sp,
                                           uint64_t pb, uint32_t lane, uint32_t span,
                                           bool nt, uint4 (&c)[U], Side &sd) {
  const uint64_t base = uniform64((uint64_t)(uintptr_t)A.data + pb * A.stride);
  const __amdgpu_buffer_rsrc_t r = rsrc_at(base, A.end);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t off = 16u * (64u * (uint32_t)u + lane);
    c[u] = bld16(r, off < span ? off : kOOB, nt);
  }
  const uint64_t p = pb + lane;
  sd = load_side(sp, p < A.n ? p : A.n - 1);
}

// LE sum of nw W-dword units of a lane's packet in LDS, starting at unit k0
// and wrapping (summation order is free; the rotation spreads the lanes over
// the LDS banks). W = 4 / 2 / 1: ds_read_b128 / b64 / b32.
template <int W>
__device__ __forceinline__ uint32_t lane_sum(const uint32_t *own, uint32_t nw, uint32_t k0) {
  uint32_t acc = 0, k = k0;
  for (uint32_t d = 0; d < nw; ++d) {
    if (W == 4) {
      const uint4 v = *(const uint4 *)(own + 4u * k);
      acc = sad(v.w, sad(v.z, sad(v.y, sad(v.x, acc))));
    } else if (W == 2) {
      const uint2 v = *(const uint2 *)(own + 2u * k);
      acc = sad(v.y, sad(v.x, acc));
    } else {
      acc = sad(own[k], acc);
    }
    k = k + 1u == nw ? 0u : k + 1u;
  }
  return acc;
}

// Stores a step's bytes from the wave's LDS slice back to the batch (fill):
// only whole dwords before the batch end — the last packet's partial tail
// dword holds no field and is left alone.
template <int U>
__device__ __forceinline__ void lane_store(const BatchArgs &A, uint64_t pb, uint32_t lane,
                                           uint32_t span, const uint4 *slice) {
  const uint64_t base = uniform64((uint64_t)(uintptr_t)A.fill + pb * A.stride);
  const uint64_t lim = (A.end & ~3ull) > base ? (A.end & ~3ull) - base : 0u;
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
      (void *)base, (short)0, (int)(lim < span ? lim : span), 0x00020000);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t off = 16u * (64u * (uint32_t)u + lane);
    const uint4 c = slice[64 * u + lane];
    __builtin_amdgcn_raw_buffer_store_b128(u32x4{c.x, c.y, c.z, c.w}, r, (int)(off < span ? off : kOOB), 0, 0);
  }
}

template <int U, int NT>
__global__ __launch_bounds__(256) void k_lane(BatchArgs A) {
  __shared__ uint4 park[4][64 * U];
  const uint32_t lane = threadIdx.x & 63u;
  uint4 *slice = park[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
  const uint64_t wave = grid_wave(A.xcd);
  const uint64_t step = (uint64_t)gridDim.x * (blockDim.x >> 6) * 64u;
  const SidePtrs sp = side_ptrs(A);
  const uint32_t S = (uint32_t)A.stride;
  const uint32_t E = A.len;
  const uint32_t span = 64u * S;
  const uint32_t nd = (E + 3u) >> 2;  // dwords per packet
  // bytes past E in the last dword (the dword-granular sum takes them)
  const uint32_t junk_tail = (E & 3u) ? ~((1u << (8u * (E & 3u))) - 1u) : 0u;
  // TX modes: Encode leaves the 16-bit checksum field 0; starts are 4-aligned
  // and the field offset even, so it is half of dword f/4
  const uint32_t f = mode_field(A.mode);
  const bool tx = mode_is_tx(A.mode);
  const uint32_t junk_field = 0xFFFFu << (8u * (f & 3u));
  // widest LDS read that tiles the packet and stays aligned (wave-uniform)
  const uint32_t W = ((E | S) & 15u) == 0 ? 4u : (((E | S) & 7u) == 0 ? 2u : 1u);
  const uint32_t nw = nd / W;
  const uint32_t k0 = lane % nw;
  const uint32_t *own = (const uint32_t *)slice + lane * (S >> 2);

  uint64_t pb = wave * 64u;
  if (pb >= A.n) return;
  uint4 c[U];
  Side sd;
  lane_fetch<U>(A, sp, pb, lane, span, NT != 0, c, sd);
  for (;;) {
    const uint64_t pn = pb + step;
    const bool more = pn < A.n;  // wave-uniform
    uint4 nx[U];
    Side nsd;
    lane_fetch<U>(A, sp, more ? pn : A.n, lane, span, NT != 0, nx, nsd);

#pragma unroll
    for (int u = 0; u < U; ++u) slice[64 * u + lane] = c[u];
    wave_lds_fence();
    uint32_t acc = W == 4u ? lane_sum<4>(own, nw, k0)
                           : (W == 2u ? lane_sum<2>(own, nw, k0) : lane_sum<1>(own, nw, k0));
    // the sum is exact (<= 128 bytes), so junk bytes come off by subtraction
    if (junk_tail) acc -= sad(own[nd - 1u] & junk_tail, 0u);
    if (tx) acc -= sad(own[f >> 2] & junk_field, 0u);
    wave_lds_fence();  // the next step's stores stay behind these reads

    const uint64_t p = pb + lane;
    if (A.fill) {
      // In place: the field goes into the LDS copy and the step's bytes go back
      // out as whole 16-byte chunks, so memory sees full-line writes instead of
      // one 2-byte write per packet (1M x 72-B datagrams: 42.3 -> 30.0 us,
      // 100-B: 54.9 -> 41.2; tools/kbench 14 KB_FILL=1).
      const uint32_t r = packet_value(A, le_to_be(acc, 0u), E, sd);
      if (p < A.n && A.out) A.out[p] = (uint16_t)r;
      if (p < A.n && f + 2u <= E)
        ((uint16_t *)slice)[(lane * S + f) >> 1] = (uint16_t)((r >> 8) | (r << 8));
      wave_lds_fence();
      lane_store<U>(A, pb, lane, span, slice);
    } else if (p < A.n) {
      finish_packet(A, p, le_to_be(acc, 0u), E, sd, nullptr, E);
    }
    if (!more) break;
#pragma unroll
    for (int u = 0; u < U; ++u) c[u] = nx[u];
    sd = nsd;
    pb = pn;
  }
}

// ---------------------------------------------------------------------
// k_loop<U, NT, BE>: one wave per packet, 64*U*16-byte windows (ragged /
// large packets). The wave walks a stream of (packet, window) items and
// always issues the loads of the next item — the next window of this
// packet, or the first window and side data of its next packet
// (whose offsets were read one packet ahead) — before it sums the current.
// ---------------------------------------------------------------------
struct LoopPkt {
  uint64_t soff, len;
  uint64_t base;  // floor4(packet start) as an address
  uint32_t sh, E, eload;
};

__device__ __forceinline__ void loop_pkt(const BatchArgs &A, uint64_t p,
                                         bool ipv4, LoopPkt &k) {
  if (p >= A.n) {  // no packet: every load of it is out of range
    k.soff = 0;
    k.len = 0;
    k.base = (uint64_t)(uintptr_t)A.data & ~3ull;
    k.sh = 0;
    k.E = 0;
    k.eload = 0;
    return;
  }
  if (A.offsets) {
    k.soff = A.offsets[p];
    k.len = A.offsets[p + 1] - k.soff;
  } else {
    k.soff = p * A.stride;
    k.len = A.len;
  }
  const uint64_t sabs = (uint64_t)(uintptr_t)A.data + k.soff;
  k.base = sabs & ~3ull;
  k.sh = (uint32_t)(sabs & 3u);
  // ragged packets past the limit get an unspecified value, never a hang
  const uint32_t l32 = k.len < YU_MAX_RAW_LEN ? (uint32_t)k.len : YU_MAX_RAW_LEN;
  k.E = k.sh + l32;
  k.eload = k.sh + (ipv4 ? (l32 < 60u ? l32 : 60u) : l32);
}

// Loads of window [wb, wb + 64*U*16) of packet k.
template <int U, int NT>
__device__ __forceinline__ void loop_fetch(const LoopPkt &k, uint32_t wb,
                                           uint32_t lane, uint64_t end,
                                           uint4 (&c)[U]) {
  const __amdgpu_buffer_rsrc_t r = rsrc_at(uniform64(k.base + wb), end);
  const uint32_t lim = k.eload > wb ? k.eload - wb : 0u;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t cr = 16u * (lane + 64u * (uint32_t)u);
    c[u] = bld16(r, cr < lim ? cr : kOOB, NT != 0);
  }
}

template <int U, int NT, bool BE>
__global__ __launch_bounds__(256) void k_loop(BatchArgs A) {
  constexpr uint32_t W = 64u * 16u * U;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = grid_wave(A.xcd);
  const uint64_t nwave = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const int mode = A.mode;
  const bool ipv4 = mode_is_ipv4(mode);
  const SidePtrs sp = side_ptrs(A);
  const bool lead = lane == 63;
  const uint64_t end = A.offsets ? (uint64_t)(uintptr_t)A.data + A.offsets[A.n] : A.end;
  const Extent ext = batch_extent(A);

  uint64_t p = wave;
  if (p >= A.n) return;
  LoopPkt cur, nxt;
  loop_pkt(A, p, ipv4, cur);
  Side sd = load_side(sp, p);
  uint32_t jx[3] = {0u, 0u, 0u};  // junk dwords, taken at window 0
  uint64_t pn = p + nwave;
  loop_pkt(A, pn, ipv4, nxt);

  uint32_t wb = 0;
  uint4 c[U];
  loop_fetch<U, NT>(cur, 0, lane, end, c);
  uint32_t acc = 0;
  for (;;) {
    const bool last = wb + W >= cur.eload;  // wave-uniform
    const bool more = !last || pn < A.n;
    // the next item: window wb+W of this packet, or window 0 of packet pn
    uint4 cn[U];
    loop_fetch<U, NT>(last ? nxt : cur, last ? 0u : wb + W, lane, end, cn);
    const Side sdn = load_side(sp, (last && pn < A.n) ? pn : p);

    uint32_t E = cur.E;
    if (ipv4) {  // single window: eload <= 63 < W
      const uint32_t hl = __shfl(ipv4_hl(c[0].x, cur.sh), 0, 64);
      const uint32_t l32 = (uint32_t)cur.len;
      E = cur.sh + (l32 < hl ? l32 : hl);
    }
    const Junk j = make_junk(cur.sh, E, mode);
    if (wb == 0) junk_take<6>(c[0], 0u, j, jx);
    const uint32_t sel = (cur.sh & 1u) ? kSelIdent : kSelSwap;
    if (wb + W <= E) {  // full window (wave-uniform)
#pragma unroll
      for (int u = 0; u < U; ++u) acc = sum_full<BE>(c[u], sel, acc);
    } else {
      const int f = (int)((E & ~3u) - wb);
      const int lim[4] = {f, f - 4, f - 8, f - 12};
      const uint32_t tm = (1u << (8u * (E & 3u))) - 1u;
#pragma unroll
      for (int u = 0; u < U; ++u)
        acc = sum_masked<BE>(c[u], 16 * (int)(lane + 64u * (uint32_t)u), lim, tm, sel, acc);
    }

    if (last) {
      acc = group_total<64>(acc);
      if (lead) {
        const uint32_t s = acc - junk_sum<BE>(jx, j, sel);
        const uint32_t v = BE ? s : le_to_be(s, cur.sh & 1u);
        finish_packet(A, p, v, cur.len, sd, fill_at(A, ext, cur.soff, cur.len),
                      E - cur.sh);
      }
      if (!more) break;
      // advance to the next packet; read the offsets of the one after it
      p = pn;
      cur = nxt;
      sd = sdn;
      pn = p + nwave;
      loop_pkt(A, pn, ipv4, nxt);
      wb = 0;
      acc = 0;
    } else {
      wb += W;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) c[u] = cn[u];
  }
}

// ---------------------------------------------------------------------
// k_hdr<NT>: the IPv4 header-only modes (IPV4 field value, VERIFY_IPV4) on
// ragged batches, one lane per packet. Only b[:HeaderLength()] (<= 60 bytes)
// of each packet is summed (header/ipv4.go:177-179, checker/checker.go:32),
// so streaming every byte (k_seg) or giving each packet a 16-lane group
// (4 packets per wave step) does far more work than needed. Here a
// wave step covers 64 packets: each lane loads the 64-byte window at
// floor4(start) (four dwordx4, cut at the packet's end), reads IHL from its
// first dword and sums the header bytes under byte masks.
__device__ __forceinline__ uint32_t byte_range_mask(uint32_t lo, uint32_t a, uint32_t b) {
  // bytes [a, b) of the dword holding bytes [lo, lo + 4)
  const uint32_t ka = a > lo ? (a - lo < 4u ? a - lo : 4u) : 0u;
  const uint32_t kb = b > lo ? (b - lo < 4u ? b - lo : 4u) : 0u;
  const uint64_t hi = (1ull << (8u * kb)) - 1ull, low = (1ull << (8u * ka)) - 1ull;
  return (uint32_t)(hi & ~low);
}

template <int NT>
__global__ __launch_bounds__(256) void k_hdr(BatchArgs A) {
  constexpr bool TWO = true;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = grid_wave(A.xcd);
  const uint64_t nwave = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint64_t data = (uint64_t)(uintptr_t)A.data;
  const bool tx = mode_is_tx(A.mode);
  const Extent ext = batch_extent(A);
  for (uint64_t p0 = wave * 64u; p0 < A.n; p0 += nwave * 64u) {
    const uint64_t p = p0 + lane;
    const bool act = p < A.n;
    uint64_t s, e;
    if (A.offsets) {
      s = A.offsets[act ? p : A.n];
      e = A.offsets[act ? p + 1 : A.n];
    } else {  // lanes past the batch sit at the last packet's end
      s = act ? p * A.stride : (A.n - 1) * A.stride + A.len;
      e = act ? s + A.len : s;
    }
    // wave-uniform descriptor over the 64 packets' bytes (lane 0's start to
    // lane 63's end, which is the chunk's end: lanes past the batch sit there)
    const uint64_t base = uniform64((data + s) & ~3ull);
    // (clamped to the batch's end: out-of-contract offsets never widen what the
    // step may read past data[0, offsets[n]))
    const uint64_t le = readlane64(e, 63);
    const uint64_t cend = data + (le < ext.hi ? le : ext.hi);
    const __amdgpu_buffer_rsrc_t r = rsrc_at(base, cend);
    const uint64_t sa = data + s;
    const uint32_t sh = (uint32_t)sa & 3u;
    const uint64_t len = e - s;
    // The descriptor starts at lane 0's packet, so one out-of-contract packet of the
    // step (decreasing offsets, or longer than YU_MAX_TRANSPORT_LEN: include/yucsum.h)
    // can move every lane's window out of it: such a step stores no field (its
    // results are unspecified). In contract, lane 0's start is the step's lowest.
    const bool step_ok = !__any((int)(len > YU_MAX_TRANSPORT_LEN));
    const uint32_t lmax = sh + (uint32_t)(len < 60u ? len : 60u);  // bytes to load
    const uint64_t wo = (sa & ~3ull) - base;
    uint4 c[4];
    // the first 32 bytes, then the rest only for lanes whose header (IHL > 7
    // with the start offset) reaches past them: a 20-byte header costs one
    // 32-byte read (config 12 of tools/kbench: 55 -> 32.5 us)
#pragma unroll
    for (int k = 0; k < (TWO ? 2 : 4); ++k)
      c[k] = bld16(r, (16u * k < lmax && wo < kOOB) ? (uint32_t)wo + 16u * k : kOOB, NT != 0);
    const uint32_t hl = ipv4_hl(c[0].x, sh);
    if (TWO) {
      const uint32_t need = sh + (uint32_t)(len < hl ? len : hl);
#pragma unroll
      for (int k = 2; k < 4; ++k)
        c[k] = __any((int)(need > 32u))
                   ? bld16(r, (16u * k < need && wo < kOOB) ? (uint32_t)wo + 16u * k : kOOB, NT != 0)
                   : make_uint4(0u, 0u, 0u, 0u);
    }
    const uint32_t E = sh + (uint32_t)(len < hl ? len : hl);
    const bool fld = tx && sh + 12u <= E;  // Encode zeroes the field (network/ipv4/ipv4.go:85-94)
    const uint32_t f0 = fld ? sh + 10u : 0u, f1 = fld ? sh + 12u : 0u;
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t w[4] = {c[k].x, c[k].y, c[k].z, c[k].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t lo = 16u * k + 4u * j;
        const uint32_t m = byte_range_mask(lo, sh, E) & ~byte_range_mask(lo, f0, f1);
        acc = sad(w[j] & m, acc);
      }
    }
    if (act) {
      const uint32_t v = le_to_be(acc, (uint32_t)sa & 1u);
      Side sd;
      sd.a = sd.b = 0u;
      sd.i = 0;
      finish_packet(A, p, v, len, sd, step_ok ? fill_at(A, ext, s, len) : nullptr, E - sh);
    }
  }
}

// ---------------------------------------------------------------------
// k_seg<U, NT>: ragged batches as a segmented sum over one byte stream.
//
// The packets of a ragged batch tile [offsets[0], offsets[n]) back to back,
// so a chunk of 64 consecutive packets is one contiguous byte range. A wave
// takes a chunk (lane l owns packet 64c + l) and streams the range in tiles
// of 64 lanes x U x 16 bytes — every load a full, coalesced dwordx4 whatever
// the packet sizes — while keeping P(x), the running LE sum (v_sad_u16) of
// the chunk's bytes before position x. A packet's sum is P(end) - P(start):
// prefix differences are exact mod 2^32 and a packet's LE sum stays below
// 2^32 up to 131072 bytes (the LE-sum limit of the header comment). In TX
// modes the checksum field is two more points, P(s+f+2) - P(s+f), taken off.
//
// Per tile: each lane sums its U chunks, a DPP scan over the wave orders the
// chunk sums by address, and only if a packet boundary falls in the tile are
// the chunk bytes and their exclusive prefixes parked in LDS, where each lane
// whose point lies in the tile reads the one chunk it needs and adds the
// bytes before the point. Packets larger than a tile cost one scan per tile
// and no LDS traffic; small packets cost a few LDS reads each instead of a
// lane group per packet, so HBM sees the same byte stream for any mix.
//
// RAW packets longer than 131072 bytes need the reference's exact uint32
// accumulator (its wrap). A chunk holding one also keeps T(x), the plain byte
// sum (v_sad_u8): with A/B the sums of the bytes at even/odd addresses,
// L = A + 256 B and T = A + B (mod 2^32), so B = (L - T) * 255^-1 and A = T - B,
// and the big-endian word sum is 256 A + B (even start) or A + 256 B (odd
// start) — bit-exact mod 2^32 at any length.
//
// Pipelining: the loads of the next tile — of this chunk, or the first tile
// of the wave's next chunk, whose offsets and side data were read one chunk
// ahead — are issued before the current tile is summed.
// ---------------------------------------------------------------------
constexpr uint32_t kInv255 = 0xFEFEFEFFu;  // 255 * kInv255 == 1 (mod 2^32)

struct SegChunk {
  uint64_t ox, oy;  // this lane's packet [ox, oy) as offsets into data (lanes
                    // past the batch: the chunk end)
  uint64_t b0;      // floor4 address of the chunk's first byte (wave-uniform)
  uint64_t xe;      // chunk end relative to b0 (wave-uniform)
  Side sd;
};

// Loads only: the packet bounds and side data of the chunk starting at
// packet p0. Ragged: offsets[]; uniform: i*stride (packets may leave gaps,
// which are streamed but belong to no packet, or overlap).
// A chunk is CH packets, lane l < CH owning packet p0 + l; lanes past the
// chunk (l >= CH) or the batch sit at the chunk's end, so lane 63 always
// holds it.
template <int CH, bool SIDE = true>
__device__ __forceinline__ void seg_load(const BatchArgs &A, const SidePtrs &sp,
                                         uint64_t p0, uint32_t lane, SegChunk &k) {
  const uint64_t n = A.n;
  const uint64_t i = p0 + lane;
  const uint64_t ce = p0 < n ? (n - p0 < (uint64_t)CH ? n : p0 + CH) : n;  // chunk end (packets)
  const bool own = lane < (uint32_t)CH && i < n;
  // ragged: two (clamped) offset loads; uniform: arithmetic, with lanes past
  // the chunk at its end (its last packet's end)
  const uint64_t last = p0 < n ? ce - 1u : 0u;
  const uint64_t uy = (own ? i : last) * A.stride + A.len;
  const uint64_t *offs = A.offsets ? A.offsets : (const uint64_t *)g_side_zero;
  const uint64_t ry = offs[A.offsets ? (own ? i + 1 : ce) : 0];
  const uint64_t rx = offs[A.offsets ? (own ? i : ce) : 0];
  k.ox = A.offsets ? rx : (own ? i * A.stride : uy);
  k.oy = A.offsets ? ry : uy;
  if (SIDE) k.sd = load_side(sp, own ? i : n - 1);  // b0/xe: seg_geom
}


// Wave-uniform geometry of a loaded chunk starting at packet p0 (waits for
// its offsets). No such chunk: an empty range, so its loads are all masked.
// line128: the tiles start at the 128-byte line holding the chunk's first byte
// (the in-place writer's whole-line write-back, k_seg), unless that line begins
// before the batch; else at its dword. The bytes in front are loaded but lie
// before every point, and the line was fetched for the previous chunk anyway.
// (tests/seg_seams.py geometry() is this rule's test-side twin: the ledger's seam
// cases are planted with it, so a change of b0 here must change it there.)
//
// Out-of-contract chunks (device ragged batches, whose offsets the host never
// reads): a packet whose offsets decrease or whose length exceeds lim, the
// mode's limit (include/yucsum.h), or which ends past the batch's end
// (data + offsets[n], what the call may touch).
//  - The writing kinds (each = true: TX, TXW, DG) test every packet of the
//    chunk, wave-uniformly, on the offsets already loaded, and the chunk's end
//    against the batch's (in-chunk order then puts every packet before it). A
//    chunk holding such a packet gets xe = 0: it streams nothing (its results
//    are unspecified) and stores no field (k_seg's epilogue stores only for
//    xe > 0, which loses nothing: an in-contract chunk with xe == 0 holds only
//    empty packets).
//    Every other chunk lies back to back from its first offset, each packet
//    within the limit, so its positions are exact (< 64 x 65536 bytes: the
//    32-bit positions never wrap).
//  - The read-only kinds (plain, RX) only bound the chunk's span to what CH
//    in-contract packets can cover, so a chunk's time is bounded whatever the
//    offsets say (a decreasing chunk end would wrap xe); a packet out of
//    contract gets an unspecified result, its neighbours stay exact.
__device__ __forceinline__ void seg_geom(uint64_t data, uint64_t n, uint64_t p0, SegChunk &k,
                                         uint32_t, bool ragged, uint32_t lim, bool each, uint32_t ch,
                                         uint64_t end, bool line128 = false) {
  if (p0 >= n) {
    k.b0 = data & ~3ull;
    k.xe = 0;
    return;
  }
  const uint64_t s = data + readlane64(k.ox, 0);
  const uint64_t e = data + readlane64(k.oy, 63);  // lane 63's end = the chunk end
  const uint64_t l = s & ~127ull;
  k.b0 = line128 && l >= (data & ~3ull) ? l : s & ~3ull;
  k.xe = e - k.b0;
  // (lanes past the chunk sit at its end: length 0)
  if (ragged && (each ? (__any((int)(k.oy - k.ox > (uint64_t)lim)) != 0 || e > end)
                      : k.xe > (uint64_t)ch * lim + 131u))  // (+ b0's up to 131 bytes in front)
    k.xe = 0;
}

// The TX kind (UDP / TCP / ICMP fields: packets <= 65535 bytes, so a chunk spans
// < 4.2 MB) keeps a loaded chunk in fewer registers, which its in-place
// write-back needs: each lane holds only the low dword of its packet's end
// offset, and the chunk's first offset is one 8-byte value all lanes load alike
// (read to SGPRs by seg_geom). A lane's start is its left neighbour's end
// (ragged batches lie back to back) or i * stride (uniform); every position and
// length is a 32-bit difference from the first offset. Per chunk in flight: 3
// VGPRs instead of 4 (two 64-bit offsets).
struct SegChunk32 {
  uint32_t ey;  // low dword of this lane's packet end (lanes past the batch or
                // the chunk: the chunk end)
  uint32_t eh;  // its high dword (ragged; dead once seg_geom has checked the chunk)
  uint64_t s0;  // the chunk's first offset (ragged: offsets[p0]; uniform: p0 * stride)
  uint64_t b0;  // address the chunk's tiles start at (wave-uniform, see seg_geom)
  uint64_t xe;  // chunk end relative to b0 (wave-uniform)
  Side sd;
};

template <int CH, bool SIDE = true>
__device__ __forceinline__ void seg_load(const BatchArgs &A, const SidePtrs &sp,
                                         uint64_t p0, uint32_t lane, SegChunk32 &k) {
  const uint64_t n = A.n;
  const uint64_t i = p0 + lane;
  const uint64_t ce = p0 < n ? (n - p0 < (uint64_t)CH ? n : p0 + CH) : n;
  const bool own = lane < (uint32_t)CH && i < n;
  const uint64_t last = p0 < n ? ce - 1u : 0u;
  const uint64_t *offs = A.offsets ? A.offsets : (const uint64_t *)g_side_zero;
  const uint64_t ry = offs[A.offsets ? (own ? i + 1 : ce) : 0];
  const uint64_t r0 = offs[A.offsets ? (p0 < n ? p0 : n) : 0];
  k.ey = A.offsets ? (uint32_t)ry : (uint32_t)((own ? i : last) * A.stride + A.len);
  k.eh = (uint32_t)(ry >> 32);
  k.s0 = A.offsets ? r0 : (p0 < n ? p0 : 0u) * A.stride;
  if (SIDE) k.sd = load_side(sp, own ? i : n - 1);
}

// (the same checks, on the 64-bit ends: a lane's start is its left neighbour's
// end, lane 0's the chunk's first offset)
__device__ __forceinline__ void seg_geom(uint64_t data, uint64_t n, uint64_t p0, SegChunk32 &k,
                                         uint32_t lane, bool ragged, uint32_t lim, bool, uint32_t,
                                         uint64_t end, bool line128 = false) {
  if (p0 >= n) {
    k.b0 = data & ~3ull;
    k.xe = 0;
    k.s0 = 0;
    return;
  }
  const uint64_t s0 = uniform64(k.s0);
  k.s0 = s0;
  const uint64_t s = data + s0;
  const uint64_t l = s & ~127ull;
  k.b0 = line128 && l >= (data & ~3ull) ? l : s & ~3ull;
  k.xe = (uint64_t)((uint32_t)__builtin_amdgcn_readlane((int)k.ey, 63) - (uint32_t)s0) + (s - k.b0);
  if (ragged) {
    const uint64_t ye = ((uint64_t)k.eh << 32) | k.ey;
    const uint64_t yl = shfl64(ye, lane ? lane - 1u : 0u);
    const uint64_t c1 = readlane64(ye, 63);  // the chunk end
    if (__any((int)(ye - (lane ? yl : s0) > (uint64_t)lim)) || data + c1 > end) k.xe = 0;
  }
}

// This lane's packet as (position relative to b0, length).
template <int CH>
__device__ __forceinline__ void seg_xlen(const BatchArgs &A, const SegChunk &k, uint32_t,
                                         uint64_t, uint64_t &x, uint64_t &len) {
  x = (uint64_t)(uintptr_t)A.data + k.ox - k.b0;
  len = k.oy - k.ox;
}

template <int CH>
__device__ __forceinline__ void seg_xlen(const BatchArgs &A, const SegChunk32 &k, uint32_t lane,
                                         uint64_t p0, uint32_t &x, uint32_t &len) {
  const uint32_t h = (uint32_t)((uint64_t)(uintptr_t)A.data + k.s0 - k.b0);  // bytes before the chunk
  const uint32_t s0 = (uint32_t)k.s0;
  uint32_t ox;
  if (A.offsets) {  // back to back: the left neighbour's end
    const uint32_t l = (uint32_t)__shfl((int)k.ey, (int)(lane ? lane - 1u : 0u), 64);
    ox = lane ? l : s0;
  } else {  // lanes past the batch sit at the chunk end (ey)
    const bool own = lane < (uint32_t)CH && p0 + lane < A.n;
    ox = own ? (uint32_t)((p0 + lane) * A.stride) : k.ey;
  }
  x = ox - s0 + h;
  len = k.ey - ox;
}

// Loads of tile t (bytes [t*T, t*T + T) past b0) of a chunk ending xe past
// b0. One call site with selected arguments and a compile-time load policy:
// no load sits in a branch, so the next tile's loads stay in flight while the
// current one is summed. (The one 128-byte line two neighbouring chunks share
// is fetched by both: <= 2% of a chunk of 64 packets >= 40 bytes.)
template <int U, bool NTL>
__device__ __forceinline__ void seg_fetch(uint64_t b0, uint64_t xe, uint64_t t, uint32_t lane,
                                          uint64_t end, uint4 (&c)[U]) {
  constexpr uint32_t T = 64u * 16u * U;
  const uint64_t tb = t * T;
  const __amdgpu_buffer_rsrc_t r = rsrc_at(uniform64(b0 + tb), end);
  const uint64_t rem = xe > tb ? xe - tb : 0u;
  const uint32_t lim = rem < T ? (uint32_t)rem : T;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t cr = 16u * (lane + 64u * (uint32_t)u);
    c[u] = bld16(r, cr < lim ? cr : kOOB, NTL);
  }
}

// Sum of the first r (0..15) bytes of a 16-byte chunk: LE halves (sad_u16)
// or plain bytes (sad_u8).
template <bool BYTES>
__device__ __forceinline__ uint32_t seg_part(const uint4 &d, uint32_t r) {
  const uint32_t w = r >> 2;
  const uint32_t mk = (1u << (8u * (r & 3u))) - 1u;
  const uint32_t v[4] = {d.x, d.y, d.z, d.w};
  uint32_t acc = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t x = j < w ? v[j] : (j == w ? (v[j] & mk) : 0u);
    acc = BYTES ? __builtin_amdgcn_sad_u8(x, 0u, acc) : sad(x, acc);
  }
  return acc;
}

// P (or T, BYTES) at tile offset q from the parked tile: the exclusive prefix at
// q's 8-byte half chunk (pre2: two per 16-byte chunk, at its start and middle)
// plus the bytes of that half chunk before q. One 4-byte and one 8-byte LDS read
// and ~10 VALU (a 16-byte chunk prefix needed the 16 bytes and twice the VALU).
template <bool BYTES>
__device__ __forceinline__ uint32_t seg_point(const uint32_t *pre2, const uint2 *half, uint32_t q) {
  const uint32_t h = q >> 3, r = q & 7u;
  const uint2 d = half[h];
  const uint32_t mk = (1u << (8u * (r & 3u))) - 1u;
  const uint32_t lo = r >= 4u ? d.x : (d.x & mk);
  const uint32_t hi = r >= 4u ? (d.y & mk) : 0u;
  return BYTES ? __builtin_amdgcn_sad_u8(hi, 0u, __builtin_amdgcn_sad_u8(lo, 0u, pre2[h]))
               : sad(hi, sad(lo, pre2[h]));
}

// One point of a lane: position x (relative to b0), and P / T at x once the
// tile holding x has gone by.
template <typename Pos>
struct SegPt {
  Pos x;
  uint32_t p, t;
};

// RX verification (YU_MODE_VERIFY_RX): the IPv4 header of a received packet
// fixes two more points — the header end and the transport end — and the
// pseudo-header. Its first 20 bytes (up to 6 dwords from floor4(start)) are
// gathered from the tiles' LDS copies as they go by (a header may straddle
// two tiles), then parsed.
struct SegRx {
  uint32_t h[6];    // header window dwords
  uint32_t need;    // mask of the window dwords still to gather (0: parsed)
  uint32_t flags;   // YU_RX_* bits known at parse time
  uint32_t pseudo;  // LE-free big-endian word sum of src, dst, proto, length
  uint32_t proto;
  uint32_t ipf;     // TX_DATAGRAM: LE sum of the IPv4 checksum field's bytes
  uint32_t hl;      // TX_DATAGRAM: header length (0 outside the contract)
  uint32_t fo;      // TX_DATAGRAM: transport field offset in the packet (0: none)
  uint32_t h20;     // k_seg: the header is the plain 20 bytes (IHL 5) of a valid packet
  uint32_t hsum;    // k_seg: then the address-ordered LE sum of those 20 bytes
  uint32_t tnext;   // k_seg, ragged: TotalLength() == len, so the transport end is
                    // the next lane's start point (no point of its own)
};

// TX_DATAGRAM on a parsed header (rx_parse): the datagram is in contract when
// 20 <= HeaderLength() <= TotalLength() <= len; its transport field exists
// when the protocol is UDP / TCP / ICMP and the segment holds its header.
// Returns (and records in rx.fo) the transport field offset from the packet
// start (0: none), and records the IPv4 field's bytes 10 and 11 as the
// address-ordered LE sum they add to (byte 10 is a low byte when the packet
// starts at an even address) for subtraction.
__device__ __forceinline__ uint32_t dg_parse(SegRx &rx, uint32_t sh, uint32_t hl, uint32_t tl) {
  const bool ok = !(rx.flags & YU_RX_INVALID) && hl >= 20u;
  rx.hl = ok ? hl : 0u;
  const uint32_t w2 = __builtin_amdgcn_alignbyte(rx.h[3], rx.h[2], sh);  // bytes 8..11 (sh 0: h[2])
  const uint32_t f = w2 >> 16;
  rx.ipf = (sh & 1u) ? ((f >> 8) | ((f & 0xFFu) << 8)) : f;
  const uint32_t fo = l4_field(rx.proto);
  rx.fo = ok && fo && tl - hl >= l4_min(rx.proto) ? hl + fo : 0u;
  return rx.fo;
}

// A 16-bit field value stored big-endian (binary.BigEndian.PutUint16).
__device__ __forceinline__ void put_be16(uint8_t *q, uint32_t r) {
  if (((uintptr_t)q & 1u) == 0) {
    *(uint16_t *)q = (uint16_t)(((r >> 8) | (r << 8)) & 0xFFFFu);
  } else {
    q[0] = (uint8_t)(r >> 8);
    q[1] = (uint8_t)r;
  }
}

// The same for a field whose two bytes have an address each (they may lie in
// two views): one 16-bit store when they are adjacent at an even address.
__device__ __forceinline__ void put_be16_at(uint8_t *q0, uint8_t *q1, uint32_t r) {
  if (q1 == q0 + 1 && ((uintptr_t)q0 & 1u) == 0) {
    *(uint16_t *)q0 = (uint16_t)(((r >> 8) | (r << 8)) & 0xFFFFu);
  } else {
    *q0 = (uint8_t)(r >> 8);
    *q1 = (uint8_t)r;
  }
}

// Parse the gathered header of a packet of length len starting sh = start&3
// bytes into h[0] (header/ipv4.go:91-118,126-138). Returns the header and
// total lengths through hl/tl.
__device__ __forceinline__ void rx_parse(SegRx &rx, uint32_t sh, uint64_t len, uint32_t &hl,
                                         uint32_t &tl) {
  // bytes 4j..4j+3 of the header (v_alignbyte with sh 0 returns h[j] itself)
  uint32_t w[5];
#pragma unroll
  for (int j = 0; j < 5; ++j)
    if (j != 1) w[j] = __builtin_amdgcn_alignbyte(rx.h[j + 1], rx.h[j], sh);
  hl = (w[0] & 0xFu) * 4u;                                // HeaderLength()
  tl = ((w[0] >> 8) & 0xFF00u) | (w[0] >> 24);            // TotalLength(), BE
  const uint32_t proto = (w[2] >> 8) & 0xFFu;             // Protocol()
  const bool valid = hl <= tl && tl <= len;               // IsValid (len >= 20 checked)
  // The usual 20-byte header is wholly in registers: its sum in the order of
  // the stream's LE prefix sums (byte 0 is a low byte when the packet starts
  // at an even address), so k_seg needs no point at the header end.
  // Summed straight from the address-aligned window dwords, whose 16-bit halves
  // already weigh each byte by its address parity: dword 0 less the sh bytes
  // before the start, dword 5 only those sh bytes' counterparts past byte 20.
  const uint32_t head = (1u << (8u * sh)) - 1u;
  uint32_t hs = sad(rx.h[0] & ~head, 0u);
#pragma unroll
  for (int j = 1; j < 5; ++j) hs = sad(rx.h[j], hs);
  rx.hsum = sad(rx.h[5] & head, hs);
  rx.h20 = valid && hl == 20u;
  const bool l4 = valid && (proto == 6u || proto == 17u || proto == 1u);
  rx.flags = valid ? 0u : YU_RX_INVALID;
  if (l4) rx.flags |= YU_RX_L4;
  rx.proto = proto;
  // PseudoHeaderChecksum(proto, src, dst) + BE16(len(payload))
  // (checker/checker.go:80-88); ICMP has none (network/ipv4/icmp.go:36-45)
  uint32_t ph = sadperm(w[3], kSelSwap, 0u);
  ph = sadperm(w[4], kSelSwap, ph);
  rx.pseudo = proto == 1u ? 0u : ph + proto + ((tl - hl) & 0xFFFFu);
  if (!valid) hl = tl = 0;
}

// Waves that take part in a k_seg launch. The grid is sized for large
// packets (many tiles per 64-packet chunk). When a ragged batch's packets
// average under kSegSmallMean bytes, a chunk is one or two tiles, and a wave
// that handles a single chunk spends its life waiting on two dependent loads
// (offsets, then bytes). So only A.small_waves waves (3 blocks per CU) work,
// each streaming several chunks with the next chunk's loads in flight; the
// other waves exit at once. The mean comes from two scalar loads of the
// offsets, which the host cannot read without a device synchronisation.
// Measured (kbench, round 1): U{40..200} 33 -> 25.5 us, U{40..600} 61 -> 58 us,
// but U{40..1000} 91 -> 93 us and U{64..1500} 127 -> 131 us, so the cut is a
// 400-byte mean.
constexpr uint64_t kSegSmallMean = 400;

typedef const __attribute__((address_space(4))) uint64_t c_u64;

__device__ __forceinline__ uint64_t seg_waves(const BatchArgs &A) {
  const uint64_t all = (uint64_t)gridDim.x * (blockDim.x >> 6);
  if (!A.offsets || A.small_waves == 0 || A.small_waves >= all) return all;
  c_u64 *o = (c_u64 *)A.offsets;  // read-only here: scalar loads
  const uint64_t bytes = o[A.n] - o[0];
  return bytes < kSegSmallMean * A.n ? (uint64_t)A.small_waves : all;
}

// Kinds of k_seg by the points a lane evaluates (compile-time, so a kind
// carries no code or registers for the others): plain (RAW / VERIFY_TCP /
// VERIFY_UDP: start and end), TX (UDP / TCP / ICMP: + the checksum field's
// two ends), RX (VERIFY_RX: + header and transport ends), DG (TX_DATAGRAM:
// RX's points; the IPv4 field comes off the parsed header's registers and
// the transport field's two bytes are read from the tile that holds them).
constexpr int kSegPlain = 0, kSegTx = 1, kSegRx = 2, kSegDg = 3;
// TXW: the TX kind writing ragged batches in place with the whole-line write-back
// (32-bit chunk loads, the park fused into the scan: the registers the
// write-back needs; TX itself keeps the layout that serves its result-array
// form best, 26.1 vs 26.8 us on kbench 8)
constexpr int kSegTxW = 4;

// (the DG kind asks for at least 3 waves per SIMD, which it would otherwise
// miss by a few VGPRs; the other kinds are left alone)
template <int U, int NT, int K, int CH = 64>
__global__ __launch_bounds__(256, K == kSegDg ? 3 : 1) void k_seg(BatchArgs A) {
  constexpr bool DG = K == kSegDg;
  constexpr bool RX = K == kSegRx || DG;  // parses each packet's IPv4 header
  constexpr bool TXW = K == kSegTxW;
  constexpr bool tx = K == kSegTx || TXW;
  constexpr bool FB = tx || DG;                 // a field whose bytes are read from the tile
  constexpr bool FILLK = FB;                    // a kind that may write fields (seg_geom)
  constexpr int NP = K == kSegRx || DG ? 4 : 2;  // point slots in use
  constexpr uint32_t T = 64u * 16u * U;
  constexpr uint32_t NC = 64u * U;  // chunks per tile
  __shared__ uint4 s_data[4][NC];   // the tile's bytes
  // exclusive prefixes per 16-byte chunk (plain kind: L, then T) or per 8-byte half
  // chunk (the others, seg_point)
  __shared__ uint32_t s_pre[4][K == kSegPlain ? NC : 2 * NC];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t wave = grid_wave(A.xcd);
  const uint64_t nwave = seg_waves(A);
  const int mode = A.mode;
  const uint32_t fld = mode_field(mode);
  const SidePtrs sp = side_ptrs(A);
  const uint64_t data = (uint64_t)(uintptr_t)A.data;
  const uint64_t end = A.offsets ? data + A.offsets[A.n] : A.end;
  const uint32_t *s_dw = (const uint32_t *)s_data[wid];
  const bool contig = A.offsets != nullptr;  // ragged: packets back to back
  // TXW kind (writing a ragged batch in place): the fields go into the parked
  // last tile of each chunk and its whole 128-byte lines are stored back with
  // non-temporal stores. See the chunk epilogue.
  const bool wbk = TXW && A.fill && contig;
  // a packet's length limit (include/yucsum.h); a chunk holding a longer one is
  // out of contract (seg_geom). Only the plain kind takes RAW packets.
  const uint32_t lim = K == kSegPlain && mode == YU_MODE_RAW ? YU_MAX_RAW_LEN : YU_MAX_TRANSPORT_LEN;
  // Positions relative to the chunk's b0: 64-bit for the plain kind (RAW packets
  // up to YU_MAX_RAW_LEN), 32-bit for the TX / RX / DG kinds, whose packets are
  // at most 65535 bytes (include/yucsum.h), so a 64-packet chunk spans < 4.2 MB
  // (uniform batches with sparser strides take k_loop_rx, pick_uniform). Half the
  // VALU work on every point test and offset.
  using Pos = typename std::conditional<K == kSegPlain, uint64_t, uint32_t>::type;
  // CH < 64: lane CH holds no packet but sits at the chunk's end, so its start
  // point is the chunk's end point and every packet's end is its successor's start
  constexpr bool kMarker = CH < 64;
  // points from half-chunk prefixes (seg_point): the 32-bit kinds; the plain
  // kind's registers (exact path) leave no room for the halves' sums
  constexpr bool HP = K != kSegPlain;
  constexpr Pos kNoPt = ~(Pos)0;             // a point slot not in use

  uint64_t ch = wave;
  if (wave >= nwave || ch * CH >= A.n) return;
  using Chunk = typename std::conditional<TXW, SegChunk32, SegChunk>::type;
  Chunk cur, nxt;
  seg_load<CH, !RX>(A, sp, ch * CH, lane, cur);
  seg_load<CH, !RX>(A, sp, (ch + nwave) * CH, lane, nxt);
  seg_geom(data, A.n, ch * CH, cur, lane, contig, lim, FILLK, CH, end, wbk);

  // per-chunk state
  SegPt<Pos> pt[4];  // start, end, then (RX, DG) header and transport end
  SegRx rx;
  // A header window that starts 4-aligned and crosses two tiles never gathers
  // h[5] (its bytes lie past the 20-byte header), yet rx_parse reads it under a
  // zero mask: give it a defined value once, not per chunk.
#pragma unroll
  for (int j = 0; j < 6; ++j) rx.h[j] = 0u;
  // TX, DG: the checksum field's next unread byte (kNoPt: none or done; DG: the
  // transport field), the bytes of it still to read (2, or 1 when the field
  // straddles two tiles) and the address-ordered LE sum of those read:
  // P(field end) - P(field start) without two more point evaluations per tile
  Pos fx = 0;
  uint32_t fk = 0, fsum = 0;
  bool exact = false;
  uint32_t carry_l = 0, carry_t = 0;
  typename std::conditional<TXW, uint32_t, uint64_t>::type plen = 0;  // this lane's packet length
  auto begin_chunk = [&](const Chunk &k, uint64_t p0) __attribute__((always_inline)) {
    typename std::conditional<TXW, uint32_t, uint64_t>::type x64, len;
    seg_xlen<CH>(A, k, lane, p0, x64, len);
    plen = len;
    const Pos x = (Pos)x64;
    const Pos y = x + (Pos)len;
    pt[0].x = x;
    // ragged packets lie back to back: P(end) is the next lane's P(start), so
    // only lane 63 evaluates an end point (the chunk end); RX needs none
    pt[1].x = RX || (contig && (kMarker || lane != 63u)) ? kNoPt : y;
    if (tx) {  // the checksum field, when the packet holds it
      const bool f = fld + 2u <= len;
      fx = f ? x + fld : kNoPt;
      fk = f ? 2u : 0u;
      fsum = 0u;
    }
    if (RX) {  // header and transport ends, once the header is parsed
      const uint32_t sh = (uint32_t)x & 3u;
      rx.need = len >= 20u ? (1u << (((19u + sh) >> 2) + 1u)) - 1u : 0u;
      // an unparsed packet (len < 20) reports only these; rx_parse sets the rest
      rx.flags = YU_RX_INVALID;
      rx.hl = rx.fo = rx.tnext = 0u;
      pt[2].x = pt[3].x = kNoPt;
      if (DG) {
        pt[2].x = pt[3].x = fx = kNoPt;
        fk = fsum = 0u;
      }
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) pt[i].p = pt[i].t = 0u;
    exact = K == kSegPlain && mode == YU_MODE_RAW && __any((int)(len > kLEMax));
    carry_l = carry_t = 0u;
  };
  begin_chunk(cur, ch * CH);

  uint64_t t = 0;
  // One tile: issue the loads of the next item into cn, then sum c.
  // Returns true when the wave has no next item.
  auto step = [&](const uint4 (&c)[U], uint4 (&cn)[U]) __attribute__((always_inline)) -> bool {
    // the chunk's tiles cover [0, xe); a point at a tile's end (xe itself,
    // when tile-aligned) takes the running sums after that tile
    const bool last = t * T + T >= cur.xe;  // wave-uniform
    // The wave's next loads go out at raised priority, ahead of the other waves'
    // sums on its SIMD, so they are in flight sooner (small ragged RX 26.6 -> 26.3
    // us, U{64..1500} 129.0 -> 127.1; no gain for k_small, a loss for k_lane:
    // profiles/r04/kbench_ab_r04p_setprio.log)
    __builtin_amdgcn_s_setprio(2);
    Chunk nn;  // the chunk after next: its loads go out before this
                  // step's tile loads, so waiting on them never waits on those
    if (last) {
      seg_geom(data, A.n, (ch + nwave) * CH, nxt, lane, contig, lim, FILLK, CH, end, wbk);
      seg_load<CH, !RX>(A, sp, (ch + 2u * nwave) * CH, lane, nn);  // (RX, DG: no side data)
    }
    seg_fetch<U, NT != 0>(last ? nxt.b0 : cur.b0, last ? nxt.xe : cur.xe, last ? 0u : t + 1u, lane,
                          end, cn);
    __builtin_amdgcn_s_setprio(0);


    const Pos tb = (Pos)(t * T);
    bool here = false;  // a packet boundary (or header) lies in this tile
#pragma unroll
    for (int i = 0; i < NP; ++i)
      if (!(RX && i == 1)) here |= pt[i].x - tb < T;  // (RX and DG have no end point)
    if (FB) here |= fx - tb < T;
    if (RX) {  // a header window [floor4(start), +24) still being gathered
      const Pos hs = pt[0].x & ~(Pos)3;
      here |= rx.need != 0u && hs < tb + T && hs + 24u > tb;
    }
    const bool park = __any((int)here);
    // chunk sums, address-ordered exclusive prefixes (DPP scan per u). The TX
    // kind parks each column as its scan completes (FUSE: no prefix array
    // live across the scan, registers its in-place write-back needs); the
    // others after the scan
    constexpr bool FUSE = TXW;
    // chunk prefix; HP: also the chunk's first half's sum (half-chunk prefixes)
    uint32_t pl[U], ph[U], ptt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      ph[u] = sad(c[u].y, sad(c[u].x, 0u));
      const uint32_t s = sad(c[u].w, sad(c[u].z, ph[u]));
      const uint32_t inc = group_total<64>(s);
      pl[u] = carry_l + inc - s;
      carry_l += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
      if (FUSE && park) {
        s_data[wid][u * 64 + lane] = c[u];
        ((uint2 *)s_pre[wid])[u * 64 + lane] = make_uint2(pl[u], pl[u] + ph[u]);
      }
    }
    if (exact) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        uint32_t s = __builtin_amdgcn_sad_u8(c[u].x, 0u, 0u);
        s = __builtin_amdgcn_sad_u8(c[u].y, 0u, s);
        s = __builtin_amdgcn_sad_u8(c[u].z, 0u, s);
        s = __builtin_amdgcn_sad_u8(c[u].w, 0u, s);
        const uint32_t inc = group_total<64>(s);
        ptt[u] = carry_t + inc - s;
        carry_t += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
      }
    }
    if (park) {
      if (!FUSE) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          s_data[wid][u * 64 + lane] = c[u];
          if (HP)
            ((uint2 *)s_pre[wid])[u * 64 + lane] = make_uint2(pl[u], pl[u] + ph[u]);
          else
            s_pre[wid][u * 64 + lane] = pl[u];
        }
      }
      __builtin_amdgcn_wave_barrier();
      bool parsed = false;
      if (RX && rx.need) {  // gather header dwords held by this tile, parse
        const Pos q0 = (pt[0].x & ~(Pos)3) - tb;
        if (q0 <= (Pos)(T - 24u)) {
          // the whole 24-byte window lies in this tile (q0 wraps past T when
          // the window began in an earlier one): six reads, no bookkeeping
          const uint32_t d = (uint32_t)q0 >> 2;
#pragma unroll
          for (int j = 0; j < 6; ++j) rx.h[j] = s_dw[d + (uint32_t)j];
          rx.need = 0u;
        } else {  // a window across two tiles: the dwords this one holds
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            const Pos q = q0 + 4u * (uint32_t)j;
            if (((rx.need >> j) & 1u) && q < T) {
              rx.h[j] = s_dw[(uint32_t)q >> 2];
              rx.need &= ~(1u << j);
            }
          }
        }
        if (rx.need == 0u) {
          uint32_t hl, tl;
          rx_parse(rx, (uint32_t)pt[0].x & 3u, plen, hl, tl);
          // a well-formed datagram fills its packet: in a ragged chunk its
          // transport end is the next lane's start (the marker lane's, for the
          // chunk's last packet), already evaluated; when every lane's is, the
          // wave skips the transport-end slot altogether
          rx.tnext = contig && kMarker && tl == (uint32_t)plen ? 1u : 0u;
          if (DG) {
            // in contract HeaderLength() >= 20: every point lies at or past
            // byte 20, so never in a tile that has gone by
            const uint32_t fo = dg_parse(rx, (uint32_t)pt[0].x & 3u, hl, tl);
            if (rx.hl) {
              pt[2].x = rx.h20 ? kNoPt : pt[0].x + hl;
              pt[3].x = rx.tnext ? kNoPt : pt[0].x + tl;
            }
            if (fo) {
              fx = pt[0].x + fo;
              fk = 2u;
            }
          } else {
            pt[2].x = rx.h20 ? kNoPt : pt[0].x + hl;
            pt[3].x = rx.tnext ? kNoPt : pt[0].x + tl;
          }
          parsed = true;
        }
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const Pos q = pt[i].x - tb;
        if (!(RX && i == 1) && q < T) {
          if (HP) {
            pt[i].p = seg_point<false>(s_pre[wid], (const uint2 *)s_data[wid], (uint32_t)q);
          } else {
            const uint32_t k = (uint32_t)q >> 4;
            pt[i].p = s_pre[wid][k] + seg_part<false>(s_data[wid][k], (uint32_t)q & 15u);
          }
        }
      }
      if (FB) {  // the field's bytes, weighted by address parity
        const Pos q = fx - tb;
        if (q < T) {
          const uint8_t *sb = (const uint8_t *)s_data[wid];
          const uint32_t b = sb[q];
          fsum += (q & 1u) ? b << 8 : b;
          if (fk == 2u && q + 1u < T) {
            const uint32_t b1 = sb[q + 1u];
            fsum += (q & 1u) ? b1 : b1 << 8;
          }
          const bool split = fk == 2u && q + 1u == T;  // the field's second byte opens the next tile
          fk = split ? 1u : 0u;
          fx = split ? fx + 1u : kNoPt;
        }
      }
      if (RX && !DG && parsed) {
        // A header straddling two tiles is parsed in the second, but a header
        // or total length under 20 bytes (IsValid accepts IHL 0..4) can put
        // its point in the first, whose bytes have gone by. Such a point lies
        // inside the gathered 24-byte window: P(point) = P(start) + the LE sum
        // of the window bytes in between, taken from the registers.
        const uint32_t sh = (uint32_t)pt[0].x & 3u;
#pragma unroll
        for (int i = 2; i < 4; ++i) {
          if (pt[i].x < tb) {
            const uint32_t b = sh + (uint32_t)(pt[i].x - pt[0].x);  // < sh + 20
            uint32_t s = pt[0].p;
#pragma unroll
            for (int j = 0; j < 6; ++j)
              s = sad(rx.h[j] & byte_range_mask(4u * (uint32_t)j, sh, b), s);
            pt[i].p = s;
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      if (exact) {  // second pass, same buffer: the byte-sum prefixes
#pragma unroll
        for (int u = 0; u < U; ++u) s_pre[wid][u * 64 + lane] = ptt[u];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const Pos q = pt[i].x - tb;
          if (q < T) {
            const uint32_t k = (uint32_t)q >> 4;
            pt[i].t = s_pre[wid][k] + seg_part<true>(s_data[wid][k], (uint32_t)q & 15u);
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
#pragma unroll
    for (int i = 0; i < NP; ++i)
      if (!(RX && i == 1) && pt[i].x - tb == T) pt[i].p = carry_l;
    if (exact) {
#pragma unroll
      for (int i = 0; i < NP; ++i)
        if (pt[i].x - tb == T) pt[i].t = carry_t;
    }

    if (!last) {
      ++t;
      return false;
    }
    // end sums: the next lane's start (ragged), else this lane's end point
    const int nl = (int)(lane < 63u ? lane + 1u : 63u);
    const uint32_t nx_p = (uint32_t)__shfl((int)pt[0].p, nl, 64);
    const uint32_t nx_t = (uint32_t)__shfl((int)pt[0].t, nl, 64);
    const bool own_end = !contig || (!kMarker && lane == 63u);
    const uint32_t p3 = RX && rx.tnext ? nx_p : pt[3].p;  // P(transport end)
    const uint32_t pe = own_end ? pt[1].p : nx_p;
    const uint32_t te = own_end ? pt[1].t : nx_t;
    const uint64_t p = ch * CH + lane;
    // TX in place (wbk): this lane's field offset in the tile (wf: it has one),
    // its line when stored whole (64: not), its value
    Pos wq = 0;
    bool wf = false;
    uint32_t wl = 64u, wr = 0u;
    // an out-of-contract chunk (xe == 0, seg_geom) stores nothing: no field, no line
    const bool wr_ok = A.fill && cur.xe != 0u;
    const bool wbc = wbk && cur.xe != 0u;
    Pos x0 = 0;  // the chunk's start (wbk: the TX kind, 32-bit)
    if (wbc) x0 = (Pos)(uint32_t)__shfl((int)(uint32_t)pt[0].x, 0, 64);
    if (lane < (uint32_t)CH && p < A.n) {
      const uint32_t odd = (uint32_t)pt[0].x & 1u;
      if (DG) {
        // IPv4 header field: ^Checksum(b[:HeaderLength()]) with the field as 0
        // (network/ipv4/ipv4.go:85-94); transport field: the sender's value
        // over b[HeaderLength():TotalLength()] with its field as 0 and the
        // pseudo header + length from the datagram (sendUDP / sendTCP /
        // sendICMPv4, see include/yucsum.h)
        uint32_t ip = 0u, l4 = 0u;
        const uint32_t p2 = rx.h20 ? pt[0].p + rx.hsum : pt[2].p;  // P(header end)
        if (rx.hl) ip = ~fold32(le_to_be(p2 - pt[0].p - rx.ipf, odd)) & 0xFFFFu;
        if (rx.fo) l4 = ~fold32(le_to_be(p3 - p2 - fsum, odd) + rx.pseudo) & 0xFFFFu;
        if (A.out) {  // out[2p], out[2p + 1]: one 32-bit store when aligned
          if (((uintptr_t)A.out & 3u) == 0u) {
            ((uint32_t *)A.out)[p] = ip | (l4 << 16);
          } else {
            A.out[2u * p] = (uint16_t)ip;
            A.out[2u * p + 1u] = (uint16_t)l4;
          }
        }
        if (wr_ok) {
          uint8_t *pk = A.fill + (cur.b0 + pt[0].x - data);
          if (rx.hl) put_be16(pk + 10u, ip);
          if (rx.fo) put_be16(pk + rx.fo, l4);
        }
      } else if (RX) {
        // header: Checksum(b[:HeaderLength()]) in {0, 0xffff}; transport:
        // pseudo + BE16(len) + segment in {0, 0xffff} (checker/checker.go:32-35,80-92)
        uint32_t r = rx.flags;
        if (!(r & YU_RX_INVALID)) {
          const uint32_t p2 = rx.h20 ? pt[0].p + rx.hsum : pt[2].p;  // P(header end)
          const uint32_t ip = fold32(le_to_be(p2 - pt[0].p, odd));
          if (ip == 0u || ip == 0xFFFFu) r |= YU_RX_IP_OK;
          if (r & YU_RX_L4) {
            const uint32_t l4 = fold32(le_to_be(p3 - p2, odd) + rx.pseudo);
            if (l4 == 0u || l4 == 0xFFFFu) r |= YU_RX_L4_OK;
          }
        }
        if (A.out) A.out[p] = (uint16_t)r;
      } else {
        uint32_t v;
        if (exact) {
          const uint32_t L = pe - pt[0].p;
          const uint32_t S = te - pt[0].t;
          const uint32_t b = (L - S) * kInv255;  // odd-address bytes
          const uint32_t a = S - b;              // even-address bytes
          v = odd ? a + (b << 8) : (a << 8) + b;
        } else {
          v = le_to_be(pe - pt[0].p - (tx ? fsum : 0u), odd);
        }
        const uint64_t len = plen;
        uint8_t *pk = wr_ok ? A.fill + (cur.b0 + pt[0].x - data) : nullptr;
        if (tx && wbc && park && fld + 2u <= len) {
          // the field's offset in the parked (last) tile, wrapping below it;
          // its line is stored whole below when the field lies in one line of
          // this tile that holds no byte outside this chunk
          wq = pt[0].x + fld - tb;
          wf = true;
          const Pos ls = wq & ~(Pos)127;
          // (wq wraps for a field in an earlier tile: wq <= T - 2 keeps those out,
          // a field ending right at this tile's start included)
          if (wq <= T - 2u && (wq & 127u) != 127u && tb + ls >= x0 && tb + ls + 128u <= cur.xe) {
            wl = (uint32_t)wq >> 7;
            pk = nullptr;  // no 2-byte store
          }
        }
        const uint32_t r = packet_value(A, v, len, cur.sd);
        if (A.out) A.out[p] = (uint16_t)r;
        wr = r;
        if (pk) store_field(A, r, pk, (uint32_t)(len < 0xFFFFFFFFu ? len : 0xFFFFFFFFu));
      }
    }
    if (tx && wbc && park) {  // wave-uniform: the in-place write-back
      // 1. Every field byte that lies in the tile goes into its parked copy, the
      //    ones left to their 2-byte stores too (same bytes: a line stored whole
      //    that holds one stays right).
      uint8_t *sb = (uint8_t *)s_data[wid];
      if (wf && wq < T) sb[wq] = (uint8_t)(wr >> 8);
      if (wf && wq + 1u < T) sb[wq + 1u] = (uint8_t)wr;  // (wq + 1 == 0: a field from the tile before)
      // 2. The lines holding a field of their own, as a 64-bit mask (T / 128 <= 64 lines).
      const uint64_t m = (uint64_t)wave_or(wl < 32u ? 1u << wl : 0u) |
                         ((uint64_t)wave_or(wl >= 32u && wl < 64u ? 1u << (wl - 32u) : 0u) << 32);
      wave_lds_fence();
      // 3. Those lines from the tile copy, as full-line 16-byte stores (8 lanes
      //    per line, one contiguous KiB per instruction), non-temporal. Memory
      //    then sees whole lines, not one partial write per field.
      const __amdgpu_buffer_rsrc_t wr_r = __builtin_amdgcn_make_buffer_rsrc(
          (void *)(A.fill + (cur.b0 + tb - data)), (short)0, (int)T, 0x00020000);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t k = (uint32_t)u * 64u + lane;
        const uint4 d = s_data[wid][k];
        const uint32_t off = ((m >> (k >> 3)) & 1u) ? 16u * k : kOOB;
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{d.x, d.y, d.z, d.w}, wr_r, (int)off, 0, 2);  // nt
      }
    }
    if ((ch + nwave) * CH >= A.n) return true;
    cur = nxt;
    nxt = nn;
    ch += nwave;
    begin_chunk(cur, ch * CH);
    t = 0;
    return false;
  };

  // ping-pong: the loads of tile i+1 land in the buffer tile i-1 used, so
  // no register copy waits on them
  uint4 ca[U], cb[U];
  seg_fetch<U, NT != 0>(cur.b0, cur.xe, 0, lane, end, ca);
  for (;;) {
    if (step(ca, cb)) break;
    if (step(cb, ca)) break;
  }
}

// ---------------------------------------------------------------------
// k_loop_rx<U, NT>: VERIFY_RX for small bursts, a wave per datagram as in
// k_loop (k_seg's one wave per 64-packet chunk leaves a burst's GPU idle).
// Window 0 holds the header: the wave parses it from lanes 0-1's registers,
// then every dword counts toward the header sum [sh, sh+hl) or the transport
// sum [sh+hl, sh+tl) through byte masks (window coordinates, base floor4 of
// the start). Same checks and result bits as k_seg's RX kind.
// ---------------------------------------------------------------------
template <int U, int NT, bool DG = false>
__global__ __launch_bounds__(256) void k_loop_rx(BatchArgs A) {
  constexpr uint32_t W = 64u * 16u * U;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = grid_wave(A.xcd);
  const uint64_t nwave = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint64_t end = A.offsets ? (uint64_t)(uintptr_t)A.data + A.offsets[A.n] : A.end;
  const Extent ext = batch_extent(A);

  uint64_t p = wave;
  if (p >= A.n) return;
  LoopPkt cur, nxt;
  loop_pkt(A, p, false, cur);
  uint64_t pn = p + nwave;
  loop_pkt(A, pn, false, nxt);
  uint32_t wb = 0;
  uint4 c[U];
  loop_fetch<U, NT>(cur, 0, lane, end, c);
  uint32_t ah = 0, at = 0, hl = 0, tl = 0, fo = 0;
  SegRx rx;
  for (;;) {
    const bool last = wb + W >= cur.eload;  // wave-uniform
    const bool more = !last || pn < A.n;
    uint4 cn[U];
    loop_fetch<U, NT>(last ? nxt : cur, last ? 0u : wb + W, lane, end, cn);
    if (wb == 0) {  // header window dwords 0..5: lane 0's chunk, half of lane 1's
      rx.h[0] = (uint32_t)__builtin_amdgcn_readlane((int)c[0].x, 0);
      rx.h[1] = (uint32_t)__builtin_amdgcn_readlane((int)c[0].y, 0);
      rx.h[2] = (uint32_t)__builtin_amdgcn_readlane((int)c[0].z, 0);
      rx.h[3] = (uint32_t)__builtin_amdgcn_readlane((int)c[0].w, 0);
      rx.h[4] = (uint32_t)__builtin_amdgcn_readlane((int)c[0].x, 1);
      rx.h[5] = (uint32_t)__builtin_amdgcn_readlane((int)c[0].y, 1);
      rx.flags = YU_RX_INVALID;
      rx.pseudo = 0u;
      hl = tl = 0u;
      if (cur.len >= 20u) rx_parse(rx, cur.sh, cur.len, hl, tl);  // IsValid: minimum size
      if (DG) {  // TX_DATAGRAM: the two fields come off by byte masks
        rx.hl = 0u;
        fo = cur.len >= 20u ? dg_parse(rx, cur.sh, hl, tl) : 0u;
        if (!rx.hl) hl = tl = 0u;
      }
    }
    const uint32_t a = cur.sh, b = cur.sh + hl, e = cur.sh + tl;
    // DG: the IPv4 field [10, 12) and the transport field [fo, fo + 2) are
    // left out of the header and transport sums (empty ranges when absent)
    const uint32_t ia = DG && rx.hl ? cur.sh + 10u : 0u, ta = DG && fo ? cur.sh + fo : 0u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t w[4] = {c[u].x, c[u].y, c[u].z, c[u].w};
      const uint32_t base = wb + 16u * (lane + 64u * (uint32_t)u);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t lo = base + 4u * (uint32_t)j;
        if (DG) {
          ah = sad(w[j] & byte_range_mask(lo, a, b) & ~byte_range_mask(lo, ia, ia + (ia ? 2u : 0u)), ah);
          at = sad(w[j] & byte_range_mask(lo, b, e) & ~byte_range_mask(lo, ta, ta + (ta ? 2u : 0u)), at);
        } else {
          ah = sad(w[j] & byte_range_mask(lo, a, b), ah);
          at = sad(w[j] & byte_range_mask(lo, b, e), at);
        }
      }
    }
    if (last) {
      ah = group_total<64>(ah);
      at = group_total<64>(at);
      if (DG && lane == 63u) {  // TX_DATAGRAM: as k_seg's DG kind
        const uint32_t odd = cur.sh & 1u;
        const uint32_t ip = rx.hl ? ~fold32(le_to_be(ah, odd)) & 0xFFFFu : 0u;
        const uint32_t l4 = fo ? ~fold32(le_to_be(at, odd) + rx.pseudo) & 0xFFFFu : 0u;
        if (A.out) {
          A.out[2u * p] = (uint16_t)ip;
          A.out[2u * p + 1u] = (uint16_t)l4;
        }
        if (uint8_t *pk = fill_at(A, ext, cur.soff, cur.len)) {
          if (rx.hl) put_be16(pk + 10u, ip);
          if (fo) put_be16(pk + fo, l4);
        }
      } else if (lane == 63u) {
        // header: Checksum(b[:HeaderLength()]) in {0, 0xffff}; transport:
        // pseudo + BE16(len) + segment in {0, 0xffff} (checker/checker.go:32-35,80-92)
        uint32_t r = rx.flags;
        if (!(r & YU_RX_INVALID)) {
          const uint32_t odd = cur.sh & 1u;
          const uint32_t ip = fold32(le_to_be(ah, odd));
          if (ip == 0u || ip == 0xFFFFu) r |= YU_RX_IP_OK;
          if (r & YU_RX_L4) {
            const uint32_t l4 = fold32(le_to_be(at, odd) + rx.pseudo);
            if (l4 == 0u || l4 == 0xFFFFu) r |= YU_RX_L4_OK;
          }
        }
        if (A.out) A.out[p] = (uint16_t)r;
      }
      if (!more) break;
      p = pn;
      cur = nxt;
      pn = p + nwave;
      loop_pkt(A, pn, false, nxt);
      wb = 0;
      ah = at = 0u;
    } else {
      wb += W;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) c[u] = cn[u];
  }
}

// ---------------------------------------------------------------------
// The scatter-gather kernels (k_iov, k_pack, k_pack_dg below), one wave per
// packet, and the parts they share. The arithmetic, the walk over a packet's
// views and the load slots it cuts them into are yucsum_iov.h's; a step is U
// slots, so a 2-view MTU packet (header view, payload view) is one step.
// Everything a packet needs besides its bytes is fetched ahead of the walk:
// first_iov with scalar loads, issued at one point per packet (scalar loads
// return out of order, so using one waits for all of them); the packet's first
// 64 view records, one per lane, and its side data, by the lead lane, with
// loads whose idle lanes pass kOOB. The walk reads a record with v_readlane;
// only views past a packet's 64th are read as the walk reaches them. first_iov
// and those late records go through constant-address-space pointers, which is
// what makes a uniform load a scalar one whatever the kernel stores: no store
// of a call (out, the fields, the packed copy) may touch the tables.
// NT: 0 plain loads, 1 nt, 2 plain for a step's first slot (a short header
// view, whose line its neighbours share) and nt for the rest.
// ---------------------------------------------------------------------
#define YU_CONST_AS __attribute__((address_space(4)))
template <typename T>
__device__ __forceinline__ const YU_CONST_AS T *const_as(const T *p) {
  return (const YU_CONST_AS T *)(uintptr_t)p;
}

// A packet's place in the view table and its first 64 view records, one per
// lane (lanes past the packet's views hold an empty view).
struct IovRecs {
  uint64_t g0;      // index of the packet's first view
  uint32_t nv;      // its views (0 when first_iov decreases: out of contract)
  uint32_t blo, bhi, len;  // lane k: view g0 + k (a length past 32 bits is past every limit: clamped)
};

// first_iov[q], first_iov[q + 1] of packet q (none: an empty packet)
__device__ __forceinline__ void iov_first_pair(const YU_CONST_AS uint64_t *first, uint64_t n, uint64_t q,
                                               uint64_t &f0, uint64_t &f1) {
  f0 = f1 = 0;
  if (q < n) {
    f0 = first[q];
    f1 = first[q + 1];
  }
}

// The packet with views [f0, f1): lane k loads record f0 + k, lanes past the
// packet's views (and past 64 of them) nothing. (The pair by reference: see
// k_iov's packet, which keeps its own copy of this.)
__device__ __forceinline__ void iov_records(IovRecs &P, const yu_iovec *views, const uint64_t &f0,
                                            const uint64_t &f1, uint32_t lane) {
  const uint64_t nv = f1 >= f0 ? f1 - f0 : 0;
  P.g0 = f0;
  P.nv = nv < 0xFFFFFFFFull ? (uint32_t)nv : 0xFFFFFFFFu;
  const uint64_t base = uniform64((uint64_t)(uintptr_t)(views + f0));
  const __amdgpu_buffer_rsrc_t r = rsrc_at(base, base + 16u * (P.nv < 64u ? P.nv : 64u));
  const uint4 v = bld16(r, 16u * lane, false);
  P.blo = v.x;
  P.bhi = v.y;
  P.len = v.w ? 0xFFFFFFFFu : v.z;
}

// View k of packet P: a record the lanes hold, or, past the 64th, one read as it
// is needed (a scalar load: views points into the constant address space).
__device__ __forceinline__ void iov_record(const IovRecs &P, const YU_CONST_AS yu_iovec *views, uint32_t k,
                                           uint64_t &b, uint32_t &l) {
  if (k < 64u) {
    b = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)P.bhi, (int)k) << 32) |
        (uint32_t)__builtin_amdgcn_readlane((int)P.blo, (int)k);
    l = (uint32_t)__builtin_amdgcn_readlane((int)P.len, (int)k);
  } else {
    const uint64_t vl = views[P.g0 + k].len;
    b = (uint64_t)(uintptr_t)views[P.g0 + k].base;
    l = vl < 0xFFFFFFFFull ? (uint32_t)vl : 0xFFFFFFFFu;
  }
}

// A packet's side data, loaded by the lead lane alone (mine: lead lane of a
// packet of the batch; an absent array: nothing): the {src, dst} record, and
// initial_arr's entry or the scalar initial. Whether an array is there comes
// apart from its pointer, which k_pack (its own copy of this, see there) keeps
// in vector registers.
__device__ __forceinline__ void iov_side(uint32_t &sa, uint32_t &sb, uint32_t &si, const uint8_t *addrs,
                                         bool have_addrs, const uint16_t *initial_arr, bool have_initial,
                                         uint32_t initial, uint64_t q, bool mine) {
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  const uint32_t own = mine ? 0u : kOOB;
  const uint64_t ab = uniform64(have_addrs ? (uint64_t)(uintptr_t)(addrs + 8 * q) : 0ull);
  const uint64_t ib = uniform64(have_initial ? (uint64_t)(uintptr_t)(initial_arr + q) : 0ull);
  const __amdgpu_buffer_rsrc_t ra =
      __builtin_amdgcn_make_buffer_rsrc((void *)ab, (short)0, have_addrs ? 8 : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t ri =
      __builtin_amdgcn_make_buffer_rsrc((void *)ib, (short)0, have_initial ? 2 : 0, 0x00020000);
  const u32x2 sab = __builtin_amdgcn_raw_buffer_load_b64(ra, (int)own, 0, 0);
  const uint16_t sin = __builtin_amdgcn_raw_buffer_load_b16(ri, (int)own, 0, 0);
  sa = sab.x;
  sb = sab.y;
  si = have_initial ? (uint32_t)sin : initial;
}

// Datagrams: the header gather of packet P, whose records have arrived. The
// views are taken in order until they hold kIovHdr bytes (a wave-uniform loop
// without a load but for records past the 64th); lane j takes the address of
// packet byte j and loads it into hb. Lanes past the packet's bytes load its
// byte 0 again, so the load is unconditional for the lanes and touches nothing
// the packet does not hold; a packet without a byte loads nothing (a
// wave-uniform branch). have: min(len, yu::kIovHdr). Returns the lane's address.
__device__ __forceinline__ uint64_t iov_dg_gather(const IovRecs &P, const YU_CONST_AS yu_iovec *views,
                                                  uint32_t lane, uint32_t &have, uint32_t &hb) {
  uint32_t off = 0, k = 0;
  uint64_t ga = 0, a0 = 0;
  while (off < yu::kIovHdr && k < P.nv) {
    uint64_t b;
    uint32_t l;
    iov_record(P, views, k, b, l);
    l = l < 0x10000u ? l : 0x10000u;  // past every limit; keeps lane - off < l exact
    if (off == 0u) a0 = b;
    if (lane - off < l) ga = b + (lane - off);  // off <= lane < off + l
    off += l;
    ++k;
  }
  have = off < yu::kIovHdr ? off : yu::kIovHdr;
  ga = lane < have ? ga : a0;
  hb = 0u;
  if (have) hb = *(const __attribute__((address_space(1))) uint8_t *)(uintptr_t)ga;
  return ga;
}

// Datagrams: the header parsed from the gathered bytes (lane j < have holds
// packet byte j) and, in the lead lane, the header and pseudo-header sums.
__device__ __forceinline__ void iov_dg_header(yu::IovDg &D, uint32_t &dhs, uint32_t &dps, int mode, uint32_t have,
                                              uint32_t hb_, uint32_t lane) {
  const int hb = (int)hb_;
  yu::iov_dg_parse(D, mode, have, (uint32_t)__builtin_amdgcn_readlane(hb, 0),
                   (uint32_t)__builtin_amdgcn_readlane(hb, 2), (uint32_t)__builtin_amdgcn_readlane(hb, 3),
                   (uint32_t)__builtin_amdgcn_readlane(hb, 9));
  dhs = group_total<64>(yu::iov_dg_hdr_term(D.meta, mode, lane, hb_));
  dps = group_total<64>(yu::iov_dg_pseudo_term(lane, hb_));
}

// Slot u of a step: its load, 16 bytes per lane, lanes past the slot nothing.
template <int NT>
__device__ __forceinline__ uint4 iov_slot_load(const yu::IovSlot &S, uint32_t lane, int u) {
  const uint32_t lim = yu::iov_lim(S.info);
  const uint64_t base = uniform64(S.base);
  const __amdgpu_buffer_rsrc_t r = rsrc_at(base, base + lim);
  const uint32_t cr = 16u * lane;
  return bld16(r, cr < lim ? cr : kOOB, NT == 1 || (NT == 2 && u != 0));
}

// The lane's share of a slot's LE sum: a whole slot that does not begin its
// view as it is, any other dword by dword, cut to the view's bytes.
__device__ __forceinline__ uint32_t iov_slot_sum(const uint4 &c, uint32_t info, uint32_t lane) {
  const uint32_t lim = yu::iov_lim(info);
  if (lim >= yu::kIovSlot && !(info & yu::kIovFirst)) return sum_full<false>(c, 0u, 0u);
  const uint32_t hm = yu::iov_head_mask(info);
  const uint32_t cr = 16u * lane;
  uint32_t t = 0;
  t = yu::iov_add(yu::iov_dword(c.x, cr, lim, hm), t);
  t = yu::iov_add(yu::iov_dword(c.y, cr + 4u, lim, hm), t);
  t = yu::iov_add(yu::iov_dword(c.z, cr + 8u, lim, hm), t);
  t = yu::iov_add(yu::iov_dword(c.w, cr + 12u, lim, hm), t);
  return t;
}

// The field byte at slot byte q: the dword that holds it, from the lane that
// loaded it, and the byte's term in the slot's sum.
__device__ __forceinline__ uint32_t iov_field_byte(const uint4 &c, uint32_t q, uint32_t &word) {
  word = (uint32_t)__builtin_amdgcn_readlane((int)pick_dword(c, (q >> 2) & 3u), (int)(q >> 4));
  return yu::iov_field_term(word, q);
}

// A whole packet's value from its class sums, stored to out[p] (lead lane).
__device__ __forceinline__ uint32_t iov_finish(uint16_t *out, uint64_t p, int mode, uint32_t len, uint32_t sA,
                                               uint32_t sB, bool have_addrs, uint32_t sa, uint32_t sb, uint32_t si) {
  const uint32_t r = yu::iov_value(mode, yu::iov_residue(sA, sB), len, have_addrs, sa, sb, si);
  if (out) out[p] = (uint16_t)r;
  return r;
}

// A datagram's values, stored to out (lead lane): TX_DATAGRAM has two per packet.
__device__ __forceinline__ void iov_dg_out(uint16_t *out, uint64_t p, int mode, uint32_t r0, uint32_t r1) {
  if (!out) return;
  if (mode == YU_MODE_TX_DATAGRAM) {
    out[2 * p] = (uint16_t)r0;
    out[2 * p + 1] = (uint16_t)r1;
  } else {
    out[p] = (uint16_t)r0;
  }
}

// ---------------------------------------------------------------------
// k_iov<U, NT, FILL, DG>: scatter-gather packets (yu_csum_batch_iov /
// yu_csum_fill_iov; DG: yu_csum_batch_iov_datagram / yu_csum_fill_iov_datagram,
// whole IPv4 datagrams whose header is parsed out of the packet). The loads of
// the next step (of this packet or the next) are issued before the current one
// is summed. first_iov runs two packets ahead, the records and the side data one.
// DG (IPV4, VERIFY_IPV4, VERIFY_RX, TX_DATAGRAM): lane j < 60 also loads packet
// byte j, a packet ahead of the walk (iov_dg_gather), so the records run two
// packets ahead and first_iov three. When the walk reaches the packet its
// header is parsed and summed from those lanes (iov_dg_header), and the walk
// gets the window [HL, TL) and the packet's own field offset (yucsum_iov.h).
// The header-only modes get an empty window: their walk only counts the bytes.
// ---------------------------------------------------------------------
struct IovArgs {
  uint16_t *out;
  uint64_t n;
  uint32_t initial;
  int mode;
};

struct IovPkt : IovRecs {
  uint32_t sa, sb, si;  // lead lane: the {src, dst} record; initial_arr's entry or the scalar initial
  // DG: lane j < have holds packet byte j, loaded from address ga
  uint32_t have;
  uint32_t hb;
  uint64_t ga;
};

// What finishing a packet needs, taken when the walk leaves it. Only the lead
// lane uses it, so but for `last` it lives in that lane's vector registers.
struct IovFin {
  bool last;     // the step is its packet's last (wave-uniform)
  uint32_t len;  // the packet's bytes; bit 31: out of contract, no field store
  uint64_t fp0, fp1;
  uint32_t sa, sb, si;
  // DG: the parsed header (yu::IovDg), its sums and the addresses of bytes 10 and 11
  uint32_t tl, meta, f, hs, ps;
  uint64_t ip0, ip1;
};

template <int U, int NT, bool FILL, bool DG = false>
__global__ __launch_bounds__(256) void k_iov(const yu_iovec *views_, const uint64_t *first_,
                                             const uint16_t *initial_arr, const uint8_t *addrs_,
                                             IovArgs A) {
  const YU_CONST_AS yu_iovec *views = const_as(views_);
  const YU_CONST_AS uint64_t *first = const_as(first_);
  const uint32_t lane = threadIdx.x & 63u;
  const bool lead = lane == 63;
  const uint64_t wave = grid_wave(0u);
  const uint64_t nwave = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const int mode = A.mode;
  const uint32_t f = DG ? 0u : yu::iov_mode_field(mode);
  const bool tx = f != 0;  // == yu::iov_mode_tx(mode)
  const uint8_t *addrs = !DG && mode_has_pseudo(mode) ? addrs_ : nullptr;
  if (wave >= A.n) return;

  // Packet q's records and side data (DG: no side arrays, the datagram carries
  // its own). The record load is iov_records' text, kept here: through the
  // function (the pair by reference, as the packing kernels compile unchanged)
  // the fill kind's VGPRs go 85 -> 84, the datagram fill kind's 107 -> 109 and
  // the datagram kind's SGPR spills 8 -> 6; with the pair by value k_iov keeps
  // its lines and k_pack_dg's fill kind spills 12 SGPRs for 10.
  auto packet = [&](IovPkt &P, uint64_t q, uint64_t f0, uint64_t f1) __attribute__((always_inline)) {
    const uint64_t nv = f1 >= f0 ? f1 - f0 : 0;
    P.g0 = f0;
    P.nv = nv < 0xFFFFFFFFull ? (uint32_t)nv : 0xFFFFFFFFu;
    const uint64_t base = uniform64((uint64_t)(uintptr_t)(views_ + f0));
    const __amdgpu_buffer_rsrc_t r = rsrc_at(base, base + 16u * (P.nv < 64u ? P.nv : 64u));
    const uint4 v = bld16(r, 16u * lane, false);
    P.blo = v.x;
    P.bhi = v.y;
    P.len = v.w ? 0xFFFFFFFFu : v.z;
    P.have = P.hb = 0u;
    P.ga = 0ull;
    P.sa = P.sb = P.si = 0u;
    if constexpr (!DG)
      iov_side(P.sa, P.sb, P.si, addrs, addrs != nullptr, initial_arr, initial_arr != nullptr, A.initial, q,
               lead && q < A.n);
  };
  auto gather = [&](IovPkt &P) __attribute__((always_inline)) {
    P.ga = iov_dg_gather(P, views, lane, P.have, P.hb);
  };

  // The walk: packet wp, view vi of it; nx: packet wp + nwave; (ff0, ff1):
  // first_iov of packet wp + 2 nwave. DG: nx's header bytes are on their way too,
  // so the records run two packets ahead (nn: packet wp + 2 nwave) and first_iov
  // three.
  uint64_t wp = wave;
  uint64_t ff0, ff1;
  IovPkt cur, nx, nn;
  {
    uint64_t a0, a1, b0, b1;
    iov_first_pair(first, A.n, wp, a0, a1);
    iov_first_pair(first, A.n, wp + nwave, b0, b1);
    iov_first_pair(first, A.n, wp + 2 * nwave, ff0, ff1);
    packet(cur, wp, a0, a1);
    packet(nx, wp + nwave, b0, b1);
    if constexpr (DG) {
      packet(nn, wp + 2 * nwave, ff0, ff1);
      iov_first_pair(first, A.n, wp + 3 * nwave, ff0, ff1);
      gather(cur);
      gather(nx);
    }
  }
  yu::IovWalk W;
  yu::iov_walk_reset(W);
  uint32_t vi = 0;
  // DG: the current packet's parsed header and, in the lead lane, its sums
  yu::IovDg D = {0u, 0u, 0u, 0u, 0u};
  uint32_t dhs = 0, dps = 0;
  // (A lambda round the call: called at its two sites directly, the datagram
  // kind's VGPRs go 80 -> 77, SGPR spills 8 -> 6, the datagram fill kind's 107 -> 108.)
  auto parse = [&]() __attribute__((always_inline)) {
    iov_dg_header(D, dhs, dps, mode, cur.have, cur.hb, lane);
  };
  if constexpr (DG) parse();

  // Makes the walk's current view one with bytes left, if the packet has one.
  auto next_view = [&]() __attribute__((always_inline)) {
    while (yu::iov_walk_done(W) && vi < cur.nv) {
      uint64_t b;
      uint32_t l;
      iov_record(cur, views, vi, b, l);
      if constexpr (DG) {
        yu::iov_walk_view_win(W, b, l, D.lo, D.hi, D.f != 0u, D.f);
      } else {
        yu::iov_walk_view(W, b, l, tx, f);
      }
      ++vi;
    }
  };
  // The walk's next step: its slots' info words, their loads issued into c, and
  // what finishing needs when the step is its packet's last (the walk then
  // moves on to the next packet).
  auto produce = [&](uint32_t (&info)[U], uint4 (&c)[U], IovFin &fin) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      next_view();
      yu::IovSlot S;
      yu::iov_walk_slot(W, S);
      info[u] = S.info;
      c[u] = iov_slot_load<NT>(S, lane, u);
    }
    next_view();
    fin.last = yu::iov_walk_done(W) && vi >= cur.nv;
    if (fin.last) {
      fin.len = lead ? (W.off | (W.over << 31)) : 0u;
      fin.fp0 = lead ? W.fp[0] : 0ull;
      fin.fp1 = lead ? W.fp[1] : 0ull;
      fin.sa = cur.sa;
      fin.sb = cur.sb;
      fin.si = cur.si;
      if constexpr (DG) {
        fin.tl = lead ? D.tl : 0u;
        fin.meta = lead ? D.meta : 0u;
        fin.f = lead ? D.f : 0u;
        fin.hs = dhs;
        fin.ps = dps;
        fin.ip0 = lead ? readlane64(cur.ga, 10u) : 0ull;
        fin.ip1 = lead ? readlane64(cur.ga, 11u) : 0ull;
      }
      wp += nwave;
      cur = nx;
      if constexpr (DG) {  // nx's records came a packet ago: its header bytes set off now
        nx = nn;
        gather(nx);
        packet(nn, wp + 2 * nwave, ff0, ff1);
        iov_first_pair(first, A.n, wp + 3 * nwave, ff0, ff1);
        parse();
      } else {
        packet(nx, wp + nwave, ff0, ff1);
        iov_first_pair(first, A.n, wp + 2 * nwave, ff0, ff1);
      }
      yu::iov_walk_reset(W);
      vi = 0;
    }
  };

  uint64_t p = wave;  // the packet being summed
  uint32_t accA = 0, accB = 0;  // per lane: LE sums of the swapped / unswapped class
  uint32_t jA = 0, jB = 0;      // the field bytes' share of them (kept by the lead lane)
  // One step: issue the walk's next step into (in, cn, fn), then sum (ic, c) and
  // finish its packet if it ends one. false: the wave's last packet is done. The
  // loop alternates two sets of registers instead of copying (see k_small).
  auto step = [&](uint32_t (&ic)[U], uint4 (&c)[U], IovFin &fc, uint32_t (&in)[U], uint4 (&cn)[U],
                  IovFin &fn) __attribute__((always_inline)) -> bool {
    produce(in, cn, fn);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t info = ic[u];
      const uint32_t lim = yu::iov_lim(info);
      if (lim == 0) continue;  // an empty slot (wave-uniform): zeros came back
      const uint32_t t = iov_slot_sum(c[u], info, lane);
      const bool swap = (info & yu::kIovSwap) != 0;
      if (info & (yu::kIovF0 | yu::kIovF1)) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          if (yu::iov_has_field(info, k)) {
            uint32_t word;
            const uint32_t term = iov_field_byte(c[u], yu::iov_field_q(info, k), word);
            jA += (lead && swap) ? term : 0u;
            jB += (lead && !swap) ? term : 0u;
          }
        }
      }
      accA += swap ? t : 0u;
      accB += swap ? 0u : t;
    }
    if (!fc.last) return true;
    uint32_t sA = group_total<64>(accA), sB = group_total<64>(accB);
    if constexpr (DG) {
      if (lead) {
        const uint32_t len = fc.len & 0x7FFFFFFFu;
        const yu::IovDg d = {0u, 0u, fc.f, fc.tl, fc.meta};
        uint32_t r0, r1;
        bool st0, st1;
        yu::iov_dg_value(d, mode, len, fc.hs, fc.ps, sA - jA, sB - jB, r0, r1, st0, st1);
        iov_dg_out(A.out, p, mode, r0, r1);
        if (FILL && !(fc.len >> 31)) {  // binary.BigEndian.PutUint16 through the views
          if (st0) put_be16_at((uint8_t *)(uintptr_t)fc.ip0, (uint8_t *)(uintptr_t)fc.ip1, r0);
          if (st1) put_be16_at((uint8_t *)(uintptr_t)fc.fp0, (uint8_t *)(uintptr_t)fc.fp1, r1);
        }
      }
    } else if (lead) {
      const uint32_t len = fc.len & 0x7FFFFFFFu;
      const bool fld = tx && len >= f + 2u;  // the whole field lies in the packet
      if (fld) {
        sA -= jA;
        sB -= jB;
      }
      const uint32_t r = iov_finish(A.out, p, mode, len, sA, sB, addrs != nullptr, fc.sa, fc.sb, fc.si);
      if (FILL && fld && !(fc.len >> 31))  // binary.BigEndian.PutUint16 through the views
        put_be16_at((uint8_t *)(uintptr_t)fc.fp0, (uint8_t *)(uintptr_t)fc.fp1, r);
    }
    accA = accB = jA = jB = 0;
    p += nwave;
    return p < A.n;
  };

  uint32_t i0[U], i1[U];
  uint4 c0[U], c1[U];
  IovFin n0, n1;
  produce(i0, c0, n0);
  for (;;) {
    if (!step(i0, c0, n0, i1, c1, n1)) break;
    if (!step(i1, c1, n1, i0, c0, n0)) break;
  }
}

// ---------------------------------------------------------------------
// k_pack<U, NT, FILL>: scatter-gather packets summed and packed in one pass
// (yu_csum_pack_iov / yu_csum_pack_fill_iov). The walk, the prefetch, the slots,
// the sums and the value are k_iov's whole-packet kind (a step's loads are
// summed in the step itself, not one step later), here as text of its own and
// not through the shared functions above: through them every resource-usage
// line stayed but the code moved (17448 -> 17452 and 17504 -> 17516 bytes),
// and pack_fused measured 0.4 % (tcp1500) and 0.7 % (udp72) slower than the
// parent, outside the parent's own spread (profiles/r12/iov_refactor_ab_r12.log).
// A change to a shared part must be made here too. Its own is the store side
// (yucsum_iov_pack.h): as a slot is summed, its bytes are shifted to the
// destination's dword phase (v_alignbyte with the neighbour
// lane's last dword, one ds_bpermute; across a slot seam the previous slot's last
// dword, which lane 63 kept) and stored: whole dwords four at a time, the edge
// dwords of a view's span by 16-bit and byte stores, never a read-modify-write.
// The field's bytes are held back and stored once by the lead lane when the
// value is known: the value (FILL, in contract) or the bytes as read. Each
// packet's dst_offsets pair comes with its records, a packet ahead, as a vector
// load every lane makes (k_iov leaves no scalar registers for it), so where a
// packet goes and its room live in vector registers; every view's copy is cut
// to the room left in the packet's span.
// ---------------------------------------------------------------------
struct PackArgs {
  uint16_t *out;
  uint8_t *dst;
  const uint64_t *dst_offsets;
  uint64_t n;
  uint32_t initial;
  int mode;
};

struct PackPkt {
  uint64_t g0;
  uint32_t nv;
  uint32_t blo, bhi, len;
  uint32_t sa, sb, si;
  uint64_t o0, o1;  // every lane: dst_offsets[q], dst_offsets[q + 1] (a vector load: the scalar registers are full)
};

struct PackFin {
  bool last;
  uint32_t len;  // bit 31: out of contract (over kIovLimit, or more bytes than room)
  uint32_t sa, sb, si;
};

// The kernel's stores for yucsum_iov_pack.h (global memory; b128 needs 4-byte
// alignment only).
struct PackStore {
  typedef uint32_t __attribute__((ext_vector_type(4), aligned(4))) u32x4a;
#define YU_GLOBAL_AS __attribute__((address_space(1)))
  __device__ __forceinline__ void b8(uint64_t a, uint8_t v) const { *(YU_GLOBAL_AS uint8_t *)(uintptr_t)a = v; }
  __device__ __forceinline__ void b16(uint64_t a, uint16_t v) const { *(YU_GLOBAL_AS uint16_t *)(uintptr_t)a = v; }
  __device__ __forceinline__ void b32(uint64_t a, uint32_t v) const { *(YU_GLOBAL_AS uint32_t *)(uintptr_t)a = v; }
  __device__ __forceinline__ void b128(uint64_t a, uint32_t x, uint32_t y, uint32_t z, uint32_t w) const {
    u32x4a v = {x, y, z, w};
    *(YU_GLOBAL_AS u32x4a *)(uintptr_t)a = v;
  }
#undef YU_GLOBAL_AS
};

// Keeps a wave-uniform value in vector registers: k_iov's walk fills the scalar
// ones, and what only addresses a vector load or store needs none.
template <typename T>
__device__ __forceinline__ T in_vgpr(T x) {
  asm volatile("" : "+v"(x));
  return x;
}

// dst_offsets[q] in every lane (past the table, q > n: 0)
__device__ __forceinline__ uint64_t pack_dst_off(const uint64_t *dst_offsets, uint64_t n, uint64_t q) {
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  const uint64_t ob = uniform64((uint64_t)(uintptr_t)(dst_offsets + (q <= n ? q : 0)));
  const __amdgpu_buffer_rsrc_t ro =
      __builtin_amdgcn_make_buffer_rsrc((void *)ob, (short)0, q <= n ? 8 : 0, 0x00020000);
  const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(ro, 0, 0, 0);
  return ((uint64_t)v.y << 32) | v.x;
}

// Packet q's dst_offsets pair (past the batch: zeros).
__device__ __forceinline__ void pack_dst_pair(uint64_t &o0, uint64_t &o1, const uint64_t *dst_offsets, uint64_t n,
                                              uint64_t q) {
  o0 = pack_dst_off(dst_offsets, n, q < n ? q : n + 1);
  o1 = pack_dst_off(dst_offsets, n, q < n ? q + 1 : n + 1);
}

// Where the packet with the pair (o0, o1) goes, in every lane (doN: dst_offsets[n]).
__device__ __forceinline__ yu::IovPackDst pack_dst_of(const uint8_t *dst, uint64_t o0, uint64_t o1, uint64_t doN) {
  return {(uint64_t)(uintptr_t)dst + o0, yu::iov_pack_room(o0, o1, doN)};
}

template <int U, int NT, bool FILL>
__global__ __launch_bounds__(256) void k_pack(const yu_iovec *views_, const uint64_t *first_,
                                              const uint16_t *initial_arr_, const uint8_t *addrs_,
                                              PackArgs A_) {
  PackArgs A = A_;
  A.out = in_vgpr(A_.out);
  A.dst = in_vgpr(A_.dst);
  A.dst_offsets = in_vgpr(A_.dst_offsets);
  const uint16_t *initial_arr = in_vgpr(initial_arr_);
  const YU_CONST_AS yu_iovec *views = const_as(views_);
  const YU_CONST_AS uint64_t *first = const_as(first_);
  const uint32_t lane = threadIdx.x & 63u;
  const bool lead = lane == 63;
  const uint64_t wave = grid_wave(0u);
  const uint64_t nwave = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const int mode = A.mode;
  const uint32_t f = yu::iov_mode_field(mode);
  const bool tx = f != 0;
  const uint8_t *addrs = in_vgpr(mode_has_pseudo(mode) ? addrs_ : nullptr);
  const bool have_addrs = mode_has_pseudo(mode) && addrs_ != nullptr, have_initial = initial_arr_ != nullptr;
  if (wave >= A.n) return;
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  // dst_offsets[q] in every lane (past the table: 0)
  auto dst_off = [&](uint64_t q) __attribute__((always_inline)) -> uint64_t {
    const uint64_t ob = uniform64((uint64_t)(uintptr_t)(A.dst_offsets + (q <= A.n ? q : 0)));
    const __amdgpu_buffer_rsrc_t ro =
        __builtin_amdgcn_make_buffer_rsrc((void *)ob, (short)0, q <= A.n ? 8 : 0, 0x00020000);
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(ro, 0, 0, 0);
    return ((uint64_t)v.y << 32) | v.x;
  };
  const uint64_t doN = dst_off(A.n);

  struct Ahead {
    uint64_t f0, f1;
  };
  auto first_pair = [&](uint64_t q, Ahead &h) __attribute__((always_inline)) {
    h.f0 = h.f1 = 0;
    if (q < A.n) {
      h.f0 = first[q];
      h.f1 = first[q + 1];
    }
  };
  auto packet = [&](PackPkt &P, uint64_t q, const Ahead &h) __attribute__((always_inline)) {
    const uint64_t nv = h.f1 >= h.f0 ? h.f1 - h.f0 : 0;
    P.g0 = h.f0;
    P.nv = nv < 0xFFFFFFFFull ? (uint32_t)nv : 0xFFFFFFFFu;
    P.o0 = dst_off(q < A.n ? q : A.n + 1);
    P.o1 = dst_off(q < A.n ? q + 1 : A.n + 1);
    const uint64_t base = uniform64((uint64_t)(uintptr_t)(views_ + h.f0));
    const __amdgpu_buffer_rsrc_t r = rsrc_at(base, base + 16u * (P.nv < 64u ? P.nv : 64u));
    const uint4 v = bld16(r, 16u * lane, false);
    P.blo = v.x;
    P.bhi = v.y;
    P.len = v.w ? 0xFFFFFFFFu : v.z;
    const uint32_t own = lead && q < A.n ? 0u : kOOB;
    const uint64_t ab = uniform64(have_addrs ? (uint64_t)(uintptr_t)(addrs + 8 * q) : 0ull);
    const uint64_t ib = uniform64(have_initial ? (uint64_t)(uintptr_t)(initial_arr + q) : 0ull);
    const __amdgpu_buffer_rsrc_t ra =
        __builtin_amdgcn_make_buffer_rsrc((void *)ab, (short)0, have_addrs ? 8 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t ri =
        __builtin_amdgcn_make_buffer_rsrc((void *)ib, (short)0, have_initial ? 2 : 0, 0x00020000);
    const u32x2 sab = __builtin_amdgcn_raw_buffer_load_b64(ra, (int)own, 0, 0);
    const uint16_t sin = __builtin_amdgcn_raw_buffer_load_b16(ri, (int)own, 0, 0);
    P.sa = sab.x;
    P.sb = sab.y;
    P.si = have_initial ? (uint32_t)sin : A.initial;
  };
  // Where packet P goes, in every lane.
  auto dst_of = [&](const PackPkt &P) __attribute__((always_inline)) -> yu::IovPackDst {
    return {(uint64_t)(uintptr_t)A.dst + P.o0, yu::iov_pack_room(P.o0, P.o1, doN)};
  };

  uint64_t wp = wave;
  Ahead ff;
  PackPkt cur, nx;
  {
    Ahead a, b;
    first_pair(wp, a);
    first_pair(wp + nwave, b);
    first_pair(wp + 2 * nwave, ff);
    packet(cur, wp, a);
    packet(nx, wp + nwave, b);
  }
  yu::IovWalk W;
  yu::iov_walk_reset(W);
  uint32_t vi = 0;
  int32_t vpk = 0;  // yu::iov_pack_view of the walk's current view

  auto next_view = [&]() __attribute__((always_inline)) {
    while (yu::iov_walk_done(W) && vi < cur.nv) {
      uint64_t b;
      uint32_t l;
      if (vi < 64u) {
        b = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)cur.bhi, (int)vi) << 32) |
            (uint32_t)__builtin_amdgcn_readlane((int)cur.blo, (int)vi);
        l = (uint32_t)__builtin_amdgcn_readlane((int)cur.len, (int)vi);
      } else {
        const uint64_t vl = views[cur.g0 + vi].len;
        b = (uint64_t)(uintptr_t)views[cur.g0 + vi].base;
        l = vl < 0xFFFFFFFFull ? (uint32_t)vl : 0xFFFFFFFFu;
      }
      vpk = yu::iov_pack_view(b, W.off);
      yu::iov_walk_view(W, b, l, tx, f);
      ++vi;
    }
  };
  auto produce = [&](uint32_t (&info)[U], int32_t (&po)[U], yu::IovPackDst &D, uint4 (&c)[U], PackFin &fin)
                     __attribute__((always_inline)) {
    D = dst_of(cur);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      next_view();
      po[u] = yu::iov_pack_po(vpk, W.w, lane);
      yu::IovSlot S;
      yu::iov_walk_slot(W, S);
      info[u] = S.info;
      const uint32_t lim = yu::iov_lim(S.info);
      const uint64_t base = uniform64(S.base);
      const __amdgpu_buffer_rsrc_t r = rsrc_at(base, base + lim);
      const uint32_t cr = 16u * lane;
      c[u] = bld16(r, cr < lim ? cr : kOOB, NT == 1 || (NT == 2 && u != 0));
    }
    next_view();
    fin.last = yu::iov_walk_done(W) && vi >= cur.nv;
    if (fin.last) {
      const uint32_t bad = W.over | (W.off > D.room ? 1u : 0u);
      fin.len = lead ? (W.off | (bad << 31)) : 0u;
      fin.sa = cur.sa;
      fin.sb = cur.sb;
      fin.si = cur.si;
      wp += nwave;
      cur = nx;
      packet(nx, wp + nwave, ff);
      first_pair(wp + 2 * nwave, ff);
      yu::iov_walk_reset(W);
      vi = 0;
      vpk = 0;
    }
  };

  const PackStore st;
  uint64_t p = in_vgpr(wave);  // the packet being summed
  uint32_t accA = 0, accB = 0;
  uint32_t jA = 0, jB = 0;
  uint32_t cprev = 0;          // lane 63: the last source dword of the slot before
  uint64_t fa0 = 0, fa1 = 0;   // lead lane: where the held-back field bytes go (0: not held)
  uint32_t fb0 = 0, fb1 = 0;   // ... and the bytes as read
  // One step: issue its loads, then sum and store it and finish its packet if it
  // ends one (false: the wave's last packet is done). Unlike k_iov the next
  // step's loads are not in flight meanwhile: the second set of registers that
  // takes is what the store side lives in, and the other waves cover the wait.
  auto step = [&](uint32_t (&ic)[U], int32_t (&pc)[U], yu::IovPackDst &Dc, uint4 (&c)[U], PackFin &fc)
                  __attribute__((always_inline)) -> bool {
    produce(ic, pc, Dc, c, fc);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t info = ic[u];
      const uint32_t lim = yu::iov_lim(info);
      if (lim == 0) continue;
      uint32_t t = 0;
      if (lim >= yu::kIovSlot && !(info & yu::kIovFirst)) {
        t = sum_full<false>(c[u], 0u, 0u);
      } else {
        const uint32_t hm = yu::iov_head_mask(info);
        const uint32_t cr = 16u * lane;
        t = yu::iov_add(yu::iov_dword(c[u].x, cr, lim, hm), t);
        t = yu::iov_add(yu::iov_dword(c[u].y, cr + 4u, lim, hm), t);
        t = yu::iov_add(yu::iov_dword(c[u].z, cr + 8u, lim, hm), t);
        t = yu::iov_add(yu::iov_dword(c[u].w, cr + 12u, lim, hm), t);
      }
      const bool swap = (info & yu::kIovSwap) != 0;
      yu::IovPackPlan P;
      yu::iov_pack_plan(P, info, Dc, pc[u], lane);
      int32_t fq0 = -1, fq1 = -1;
      if (info & (yu::kIovF0 | yu::kIovF1)) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          if (yu::iov_has_field(info, k)) {
            const uint32_t q = yu::iov_field_q(info, k);
            const uint32_t word = (uint32_t)__builtin_amdgcn_readlane(
                (int)pick_dword(c[u], (q >> 2) & 3u), (int)(q >> 4));
            const uint32_t term = yu::iov_field_term(word, q);
            jA += (lead && swap) ? term : 0u;
            jB += (lead && !swap) ? term : 0u;
            // held back when it fits the room (the same answer in every lane)
            const bool held = yu::iov_pack_field_held(P, q, lane);
            const uint32_t byte = (word >> (8u * (q & 3u))) & 0xFFu;
            if (k == 0) {
              fq0 = held ? (int32_t)q : -1;
              fa0 = lead && held ? yu::iov_pack_field_addr(P, q, lane) : fa0;
              fb0 = byte;
            } else {
              fq1 = held ? (int32_t)q : -1;
              fa1 = lead && held ? yu::iov_pack_field_addr(P, q, lane) : fa1;
              fb1 = byte;
            }
          }
        }
      }
      // the source dword before the lane's own: the neighbour's last, and for lane 0
      // the last of the slot before, which lane 63 offers in place of its own
      const uint32_t prev = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4u * ((lane - 1u) & 63u)),
                                                                   (int)(lead ? cprev : c[u].w));
      yu::iov_pack_lane(st, P, lane, c[u].x, c[u].y, c[u].z, c[u].w, prev, fq0, fq1);
      cprev = c[u].w;
      accA += swap ? t : 0u;
      accB += swap ? 0u : t;
    }
    if (!fc.last) return true;
    uint32_t sA = group_total<64>(accA), sB = group_total<64>(accB);
    if (lead) {
      const uint32_t len = fc.len & 0x7FFFFFFFu;
      const bool fld = tx && len >= f + 2u;
      if (fld) {
        sA -= jA;
        sB -= jB;
      }
      const uint32_t r = yu::iov_value(mode, yu::iov_residue(sA, sB), len, have_addrs, fc.sa,
                                       fc.sb, fc.si);
      if (A.out) A.out[p] = (uint16_t)r;
      if (tx) {
        const bool put = FILL && fld && !(fc.len >> 31);  // binary.BigEndian.PutUint16 into the copy
        yu::iov_pack_field_store(st, fa0, fa1, put ? r >> 8 : fb0, put ? r & 0xFFu : fb1);
      }
    }
    accA = accB = jA = jB = 0;
    fa0 = fa1 = 0;
    p += nwave;
    return uniform64(p) < A.n;
  };

  uint32_t i0[U];
  int32_t p0[U];
  yu::IovPackDst d0;
  uint4 c0[U];
  PackFin n0;
  while (step(i0, p0, d0, c0, n0)) {
  }
}

// ---------------------------------------------------------------------
// k_pack_dg<U, NT, FILL>: whole IPv4 datagrams held as scatter-gather packets,
// verified or filled and packed in one pass (yu_csum_pack_iov_datagram /
// yu_csum_pack_fill_iov_datagram; named k_pack<4,dg> / k_pack<4,dg,fill>). A
// kernel of its own, so k_iov and k_pack compile as they did. The store side
// and the step are k_pack's, the prefetch pack_dst_pair and iov_records as
// there; the header comes by iov_dg_gather and iov_dg_header and the values
// leave by iov_dg_out as in k_iov's datagram kind. Where
// the two part (yucsum_iov_pack.h, last section): the walk is the plain one,
// since the copy wants every byte, and the window [HL, TL) is applied to the
// sum by each slot's place in the packet. FILL holds back bytes 10, 11 and the
// transport field's two bytes from the copy and stores them when the packet is
// done, because TL <= len is known only then: the value, or the byte as read.
// The plain form holds nothing back and copies all bytes as they come.
// Look-ahead: records one packet ahead (k_pack's depth; k_iov's datagram kind
// keeps two, which here would cost a third set of record registers), the
// header bytes of the next packet are loaded when the current one starts (its
// records came a packet ago), and a packet is parsed as its first step begins,
// a whole packet after its header bytes set off.
// ---------------------------------------------------------------------
struct PackDgPkt : IovRecs {
  uint64_t o0, o1;
  uint32_t have, hb;  // lane j < have holds packet byte j; have = min(len, yu::kIovHdr)
};

struct PackDgFin {
  bool last;
  uint32_t len;  // bit 31: out of contract
  uint32_t b10;  // lead lane: packet bytes 10 and 11 as read (byte 11 << 8)
};

template <int U, int NT, bool FILL>
__global__ __launch_bounds__(256) void k_pack_dg(const yu_iovec *views_, const uint64_t *first_, PackArgs A_) {
  PackArgs A = A_;
  A.out = in_vgpr(A_.out);
  A.dst = in_vgpr(A_.dst);
  A.dst_offsets = in_vgpr(A_.dst_offsets);
  const YU_CONST_AS yu_iovec *views = const_as(views_);
  const YU_CONST_AS uint64_t *first = const_as(first_);
  const uint32_t lane = threadIdx.x & 63u;
  const bool lead = lane == 63;
  const uint64_t wave = grid_wave(0u);
  const uint64_t nwave = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const int mode = A.mode;
  if (wave >= A.n) return;
  const uint64_t doN = pack_dst_off(A.dst_offsets, A.n, A.n);

  auto packet = [&](PackDgPkt &P, uint64_t q, uint64_t f0, uint64_t f1) __attribute__((always_inline)) {
    pack_dst_pair(P.o0, P.o1, A.dst_offsets, A.n, q);
    iov_records(P, views_, f0, f1, lane);
    P.have = P.hb = 0u;
  };
  auto gather = [&](PackDgPkt &P) __attribute__((always_inline)) {  // bytes 10, 11 go by offset: no address kept
    iov_dg_gather(P, views, lane, P.have, P.hb);
  };

  uint64_t wp = wave;
  uint64_t ff0, ff1;
  PackDgPkt cur, nx;
  {
    uint64_t a0, a1, b0, b1;
    iov_first_pair(first, A.n, wp, a0, a1);
    iov_first_pair(first, A.n, wp + nwave, b0, b1);
    iov_first_pair(first, A.n, wp + 2 * nwave, ff0, ff1);
    packet(cur, wp, a0, a1);
    packet(nx, wp + nwave, b0, b1);
    gather(cur);
  }
  yu::IovWalk W;
  yu::iov_walk_reset(W);
  uint32_t vi = 0;
  int32_t vpk = 0;
  bool fresh = true;  // the walk's next step is its packet's first
  // the current packet's parsed header (until the next one's first step) and, in
  // the lead lane, its sums
  yu::IovDg D = {0u, 0u, 0u, 0u, 0u};
  uint32_t dhs = 0, dps = 0;

  auto next_view = [&]() __attribute__((always_inline)) {
    while (yu::iov_walk_done(W) && vi < cur.nv) {
      uint64_t b;
      uint32_t l;
      iov_record(cur, views, vi, b, l);
      vpk = yu::iov_pack_view(b, W.off);
      yu::iov_walk_view(W, b, l, D.f != 0u, D.f);
      ++vi;
    }
  };
  auto produce = [&](uint32_t (&info)[U], int32_t (&po)[U], yu::IovPackDst &Dd, uint4 (&c)[U], PackDgFin &fin)
                     __attribute__((always_inline)) {
    if (fresh) {  // cur's header bytes set off a packet ago; nx's records came with cur's last step
      iov_dg_header(D, dhs, dps, mode, cur.have, cur.hb, lane);
      gather(nx);
      fresh = false;
    }
    Dd = pack_dst_of(A.dst, cur.o0, cur.o1, doN);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      next_view();
      po[u] = yu::iov_pack_po(vpk, W.w, lane);
      yu::IovSlot S;
      yu::iov_walk_slot(W, S);
      info[u] = S.info;
      c[u] = iov_slot_load<NT>(S, lane, u);
    }
    next_view();
    fin.last = yu::iov_walk_done(W) && vi >= cur.nv;
    if (fin.last) {
      const uint32_t bad = W.over | (W.off > Dd.room ? 1u : 0u);
      fin.len = lead ? (W.off | (bad << 31)) : 0u;
      fin.b10 = 0u;
      if constexpr (FILL) {
        const int hb = (int)cur.hb;
        fin.b10 = lead ? ((uint32_t)__builtin_amdgcn_readlane(hb, 10) |
                          ((uint32_t)__builtin_amdgcn_readlane(hb, 11) << 8))
                       : 0u;
      }
      wp += nwave;
      cur = nx;
      packet(nx, wp + nwave, ff0, ff1);
      iov_first_pair(first, A.n, wp + 2 * nwave, ff0, ff1);
      yu::iov_walk_reset(W);
      vi = 0;
      vpk = 0;
      fresh = true;
    }
  };

  const PackStore st;
  uint64_t p = in_vgpr(wave);
  uint32_t accA = 0, accB = 0;
  uint32_t jA = 0, jB = 0;
  uint32_t cprev = 0;
  uint32_t fb0 = 0, fb1 = 0;  // the transport field's bytes as read
  auto step = [&](uint32_t (&ic)[U], int32_t (&pc)[U], yu::IovPackDst &Dc, uint4 (&c)[U], PackDgFin &fc)
                  __attribute__((always_inline)) -> bool {
    produce(ic, pc, Dc, c, fc);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t info = ic[u];
      const uint32_t lim = yu::iov_lim(info);
      if (lim == 0) continue;
      const int32_t p0 = __builtin_amdgcn_readfirstlane(pc[u]);  // lane 0's: the slot's window byte 0
      const int span = yu::iov_pack_dg_span(info, p0, D.lo, D.hi);
      uint32_t t = 0;
      if (span == 1) {
        t = iov_slot_sum(c[u], info, lane);
      } else if (span == 2) {  // the slot straddles HL or TL: each dword's bytes by packet offset
        const uint32_t hm = yu::iov_head_mask(info);
        const uint32_t cr = 16u * lane;
        const int32_t x = pc[u];
        t = yu::iov_add(yu::iov_dword(c[u].x, cr, lim, hm) & yu::iov_win_mask(x, D.lo, D.hi), t);
        t = yu::iov_add(yu::iov_dword(c[u].y, cr + 4u, lim, hm) & yu::iov_win_mask(x + 4, D.lo, D.hi), t);
        t = yu::iov_add(yu::iov_dword(c[u].z, cr + 8u, lim, hm) & yu::iov_win_mask(x + 8, D.lo, D.hi), t);
        t = yu::iov_add(yu::iov_dword(c[u].w, cr + 12u, lim, hm) & yu::iov_win_mask(x + 12, D.lo, D.hi), t);
      }
      const bool swap = (info & yu::kIovSwap) != 0;
      yu::IovPackPlan P;
      yu::iov_pack_plan(P, info, Dc, pc[u], lane);
      int32_t fq0 = -1, fq1 = -1;
      if (info & (yu::kIovF0 | yu::kIovF1)) {  // TX_DATAGRAM: the transport field, inside the window
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          if (yu::iov_has_field(info, k)) {
            const uint32_t q = yu::iov_field_q7(info, k);
            uint32_t word;
            const uint32_t term = iov_field_byte(c[u], q, word);
            jA += (lead && swap) ? term : 0u;
            jB += (lead && !swap) ? term : 0u;
            if constexpr (FILL) {
              const bool held = yu::iov_pack_field_held(P, q, lane);
              const uint32_t byte = (word >> (8u * (q & 3u))) & 0xFFu;
              if (k == 0) {
                fq0 = held ? (int32_t)q : -1;
                fb0 = byte;
              } else {
                fq1 = held ? (int32_t)q : -1;
                fb1 = byte;
              }
            }
          }
        }
      }
      const uint32_t prev = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4u * ((lane - 1u) & 63u)),
                                                                   (int)(lead ? cprev : c[u].w));
      if (FILL && (info & yu::kIovFirst) && p0 <= 11) {  // the view's first slot reaches bytes 10, 11 (wave-uniform)
        const int32_t fq2 = yu::iov_pack_dg_held(P, info, p0, 10u, lane);
        const int32_t fq3 = yu::iov_pack_dg_held(P, info, p0, 11u, lane);
        yu::iov_pack_lane4(st, P, lane, c[u].x, c[u].y, c[u].z, c[u].w, prev, fq0, fq1, fq2, fq3);
      } else {
        yu::iov_pack_lane(st, P, lane, c[u].x, c[u].y, c[u].z, c[u].w, prev, fq0, fq1);
      }
      cprev = c[u].w;
      accA += swap ? t : 0u;
      accB += swap ? 0u : t;
    }
    if (!fc.last) return true;
    const uint32_t sA = group_total<64>(accA), sB = group_total<64>(accB);
    if (lead) {
      const uint32_t len = fc.len & 0x7FFFFFFFu;
      uint32_t r0, r1;
      bool st0, st1;
      yu::iov_dg_value(D, mode, len, dhs, dps, sA - jA, sB - jB, r0, r1, st0, st1);
      iov_dg_out(A.out, p, mode, r0, r1);
      if constexpr (FILL) {  // binary.BigEndian.PutUint16 into the copy, or the bytes as read
        const bool ok = !(fc.len >> 31);
        yu::iov_pack_dg_finish(st, Dc, len, D.f, ok && st0, ok && st1, r0, r1, fc.b10 & 0xFFu, fc.b10 >> 8, fb0,
                               fb1);
      }
    }
    accA = accB = jA = jB = 0;
    p += nwave;
    return uniform64(p) < A.n;
  };

  uint32_t i0[U];
  int32_t p0[U];
  yu::IovPackDst d0;
  uint4 c0[U];
  PackDgFin n0;
  while (step(i0, p0, d0, c0, n0)) {
  }
}

// ---------------------------------------------------------------------
// range_walk<U, NT>: the walk of a packet that is one source range, shared by
// k_build and k_split. The caller has positioned W on the range (iov_walk_view)
// and taken vpk from it; here the range goes by in steps of U 1-KiB slots, each
// summed (k_iov's slot sum) and stored through yucsum_iov_pack.h's plan, shift
// and masked stores with nothing held back, a lane's previous source dword from
// its neighbour by ds_bpermute (lane 0's from lane 63 of the slot before).
// Returns the lane's two class sums {swapped, plain}; the walk is handed back
// as it ends (k_build reads its `over`). The shape is the one the compiler
// follows most closely to the loop written out in each kernel: the walk on a
// local copy declared ahead of the sums, everything else by const value. By
// reference, or by value without the const, both kernels take one VGPR more;
// walking the caller's W in place lays k_build's loop out differently
// (profiles/r15/range_walk_isa_r15.txt).
// ---------------------------------------------------------------------
template <int U, int NT>
__device__ __forceinline__ uint2 range_walk(yu::IovWalk &walk, const int32_t vpk, const yu::IovPackDst D,
                                            const PackStore st, const uint32_t lane, const bool lead) {
  yu::IovWalk W = walk;
  uint32_t accA = 0, accB = 0;
  uint32_t cprev = 0;  // lane 63: the last source dword of the slot before
  while (!yu::iov_walk_done(W)) {
    uint32_t info[U];
    int32_t po[U];
    uint4 c[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      po[u] = yu::iov_pack_po(vpk, W.w, lane);
      yu::IovSlot S;
      yu::iov_walk_slot(W, S);
      info[u] = S.info;
      c[u] = iov_slot_load<NT>(S, lane, u);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (yu::iov_lim(info[u]) == 0) continue;  // an empty slot (wave-uniform)
      const uint32_t t = iov_slot_sum(c[u], info[u], lane);
      const bool swap = (info[u] & yu::kIovSwap) != 0;
      yu::IovPackPlan P;
      yu::iov_pack_plan(P, info[u], D, po[u], lane);
      const uint32_t prev = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4u * ((lane - 1u) & 63u)),
                                                                   (int)(lead ? cprev : c[u].w));
      yu::iov_pack_lane(st, P, lane, c[u].x, c[u].y, c[u].z, c[u].w, prev, -1, -1);
      cprev = c[u].w;
      accA += swap ? t : 0u;
      accB += swap ? 0u : t;
    }
  }
  walk = W;
  return make_uint2(accA, accB);
}

// ---------------------------------------------------------------------
// k_build<U, NT>: outgoing IPv4 datagrams built from a payload and one 32-byte
// record per packet (yu_tx_build_ragged; yucsum_build.h has the arithmetic). One
// wave per packet on the over-subscribed grid, as k_loop and k_iov. It is
// k_pack's store side fed by exactly one source range: the payload is a single
// view, walked from packet offset 20 + H by range_walk. There is no view table,
// no gather and no parse: the control data of a packet is its pay_offsets pair,
// its dst_offsets pair and its record (two 16-byte loads), all wave-uniform
// scalar loads through the constant address space (no store of the call may
// touch the tables) issued a packet ahead. The header's sums are arithmetic on the
// record; when the payload's class sums are known the header's 20 + H bytes are
// encoded with both fields in place and stored last, once: lane J < 11 owns
// destination dword J of the packet (source dwords J - 1 and J, the neighbour's
// by one DPP row shift), masked to the header's end and the packet's room and
// stored by the width rules of a payload dword.
// ---------------------------------------------------------------------
struct BuildArgs {
  uint8_t *dst;
  const uint64_t *dst_offsets;
  uint16_t *out;
  uint64_t n;
};

struct BuildPkt {
  uint64_t p0, p1;  // pay_offsets[q], pay_offsets[q + 1]
  uint64_t o0, o1;  // dst_offsets[q], dst_offsets[q + 1]
  yu::BuildRec R;
};

template <int U, int NT>
__global__ __launch_bounds__(256) void k_build(const uint8_t *payload, const uint64_t *pay_offsets_,
                                               const yu_tx_record *recs_, BuildArgs A) {
  const YU_CONST_AS uint64_t *pay_offsets = const_as(pay_offsets_);
  const YU_CONST_AS uint64_t *dst_offsets = const_as(A.dst_offsets);
  const YU_CONST_AS uint32_t *recs = const_as((const uint32_t *)recs_);
  const uint32_t lane = threadIdx.x & 63u;
  const bool lead = lane == 63;
  const uint64_t wave = grid_wave(0u);
  const uint64_t nwave = (uint64_t)gridDim.x * (blockDim.x >> 6);
  if (wave >= A.n) return;
  const uint64_t poN = pay_offsets[A.n], doN = dst_offsets[A.n];

  // Packet q's control data (past the batch: packet 0's again, never used).
  auto packet = [&](BuildPkt &P, uint64_t q) __attribute__((always_inline)) {
    const uint64_t i = q < A.n ? q : 0;
    P.p0 = pay_offsets[i];
    P.p1 = pay_offsets[i + 1];
    P.o0 = dst_offsets[i];
    P.o1 = dst_offsets[i + 1];
#pragma unroll
    for (int k = 0; k < 8; ++k) P.R.w[k] = recs[8 * i + k];
  };

  const PackStore st;
  BuildPkt cur, nx;
  packet(cur, wave);
  for (uint64_t p = wave; p < A.n; p += nwave) {
    packet(nx, p + nwave);
    const yu::BuildRec R = cur.R;
    const uint32_t H = yu::build_l4_len(yu::build_proto(R));
    // the payload, cut to payload[0, pay_offsets[n]) whatever its offsets say
    const bool ranged = cur.p0 <= cur.p1 && cur.p1 <= poN;
    const uint64_t pe = cur.p1 < poN ? cur.p1 : poN;
    const uint64_t plen = pe > cur.p0 ? pe - cur.p0 : 0;
    const uint64_t addr = (uint64_t)(uintptr_t)payload + (plen ? cur.p0 : 0);
    const yu::IovPackDst D = {(uint64_t)(uintptr_t)A.dst + cur.o0, yu::iov_pack_room(cur.o0, cur.o1, doN)};
    yu::IovWalk W;
    yu::iov_walk_reset(W);
    W.off = yu::kBuildIp + H;
    const int32_t vpk = yu::iov_pack_view(addr, W.off);
    yu::iov_walk_view(W, addr, plen, false, 0u);
    const uint32_t L = W.off - (yu::kBuildIp + H);  // the bytes taken: T <= 65535

    const uint2 acc = range_walk<U, NT>(W, vpk, D, st, lane, lead);
    const uint32_t sA = (uint32_t)__builtin_amdgcn_readlane((int)group_total<64>(acc.x), 63);
    const uint32_t sB = (uint32_t)__builtin_amdgcn_readlane((int)group_total<64>(acc.y), 63);
    uint32_t ipsum, xsum;
    yu::build_values(R, H, L, sA, sB, ipsum, xsum);

    // the header, stored last: lane J's destination dword J
    {
      const uint32_t hw = yu::build_hdr_src(R, H, L, ipsum, xsum, lane);
      const uint32_t hprev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hw, 0x111, 0xf, 0xf, true);  // row_shr:1
      yu::IovPackPlan P;
      yu::build_hdr_plan(P, D, H);
      const uint32_t m = lane < yu::kBuildHdrDwords ? yu::iov_pack_mask(P, lane) : 0u;
      if (m) yu::iov_pack_store(st, (P.pa & ~3ull) + 4u * lane, yu::build_hdr_dst(hw, hprev, P.delta), m);
    }
    if (lead && A.out) {
      const bool ok = yu::build_in_contract(R, ranged, W.over != 0u, L, D.room);
      A.out[2 * p] = (uint16_t)(ok ? ipsum : 0u);
      A.out[2 * p + 1] = (uint16_t)(ok ? xsum : 0u);
    }
    cur = nx;
  }
}

// ---------------------------------------------------------------------
// k_build_iov<U, NT> ("k_build<4,iov>"): k_build with the payload of packet i
// behind views[i] instead of payload[pay_offsets[i], pay_offsets[i + 1])
// (yu_tx_build_iov), so that datagrams are built straight from where their
// payloads lie, inside a received batch for instance. The view is one 16-byte
// wave-uniform load through the constant address space, issued a packet ahead
// like the record and the dst_offsets pair; it gives (addr, plen) as they
// stand, there is no batch end to cut it to. A packet whose destination span is
// empty is skipped (build_iov_skipped): a wave-uniform branch past the walk and
// the header, the view's base never used, the out pair {0, 0}. Everything after
// (addr, plen) is k_build's: range_walk, the header encode, the store rules.
// It is a kernel of its own, not a third template argument of k_build, so that
// k_build<4>'s code stays byte for byte what it was; it takes k_build's plan
// row (grid and load policy) and is no row of YU_WAVE_KERNELS.
// ---------------------------------------------------------------------
struct BuildIovPkt {
  uint64_t base, len;  // views[q]
  uint64_t o0, o1;     // dst_offsets[q], dst_offsets[q + 1]
  yu::BuildRec R;
};

template <int U, int NT>
__global__ __launch_bounds__(256) void k_build_iov(const yu_iovec *views_, const yu_tx_record *recs_, BuildArgs A) {
  static_assert(sizeof(yu_iovec) == 16 && offsetof(yu_iovec, len) == 8, "a view is {base, len}, 16 bytes");
  const YU_CONST_AS uint64_t *views = const_as((const uint64_t *)views_);
  const YU_CONST_AS uint64_t *dst_offsets = const_as(A.dst_offsets);
  const YU_CONST_AS uint32_t *recs = const_as((const uint32_t *)recs_);
  const uint32_t lane = threadIdx.x & 63u;
  const bool lead = lane == 63;
  const uint64_t wave = grid_wave(0u);
  const uint64_t nwave = (uint64_t)gridDim.x * (blockDim.x >> 6);
  if (wave >= A.n) return;
  const uint64_t doN = dst_offsets[A.n];

  // Packet q's control data (past the batch: packet 0's again, never used).
  auto packet = [&](BuildIovPkt &P, uint64_t q) __attribute__((always_inline)) {
    const uint64_t i = q < A.n ? q : 0;
    P.base = views[2 * i];
    P.len = views[2 * i + 1];
    P.o0 = dst_offsets[i];
    P.o1 = dst_offsets[i + 1];
#pragma unroll
    for (int k = 0; k < 8; ++k) P.R.w[k] = recs[8 * i + k];
  };

  const PackStore st;
  BuildIovPkt cur, nx;
  packet(cur, wave);
  for (uint64_t p = wave; p < A.n; p += nwave, cur = nx) {
    packet(nx, p + nwave);
    if (yu::build_iov_skipped(cur.o0, cur.o1)) {  // wave-uniform: both come from scalar loads
      if (lead && A.out) A.out[2 * p] = A.out[2 * p + 1] = 0;
      continue;
    }
    const yu::BuildRec R = cur.R;
    const uint32_t H = yu::build_l4_len(yu::build_proto(R));
    const uint64_t plen = cur.len, addr = cur.base;
    const yu::IovPackDst D = {(uint64_t)(uintptr_t)A.dst + cur.o0, yu::iov_pack_room(cur.o0, cur.o1, doN)};
    yu::IovWalk W;
    yu::iov_walk_reset(W);
    W.off = yu::kBuildIp + H;
    const int32_t vpk = yu::iov_pack_view(addr, W.off);
    yu::iov_walk_view(W, addr, plen, false, 0u);  // stops at the limit: W.over
    const uint32_t L = W.off - (yu::kBuildIp + H);  // the bytes taken: T <= 65535

    const uint2 acc = range_walk<U, NT>(W, vpk, D, st, lane, lead);
    const uint32_t sA = (uint32_t)__builtin_amdgcn_readlane((int)group_total<64>(acc.x), 63);
    const uint32_t sB = (uint32_t)__builtin_amdgcn_readlane((int)group_total<64>(acc.y), 63);
    uint32_t ipsum, xsum;
    yu::build_values(R, H, L, sA, sB, ipsum, xsum);

    // the header, stored last: lane J's destination dword J
    {
      const uint32_t hw = yu::build_hdr_src(R, H, L, ipsum, xsum, lane);
      const uint32_t hprev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hw, 0x111, 0xf, 0xf, true);  // row_shr:1
      yu::IovPackPlan P;
      yu::build_hdr_plan(P, D, H);
      const uint32_t m = lane < yu::kBuildHdrDwords ? yu::iov_pack_mask(P, lane) : 0u;
      if (m) yu::iov_pack_store(st, (P.pa & ~3ull) + 4u * lane, yu::build_hdr_dst(hw, hprev, P.delta), m);
    }
    if (lead && A.out) {
      const bool ok = yu::build_in_contract(R, true, W.over != 0u, L, D.room);
      A.out[2 * p] = (uint16_t)(ok ? ipsum : 0u);
      A.out[2 * p + 1] = (uint16_t)(ok ? xsum : 0u);
    }
  }
}

// ---------------------------------------------------------------------
// k_split<U, NT>: received IPv4 datagrams taken apart into a 32-byte record, a
// payload and VERIFY_RX's flags (yu_rx_split_ragged; yucsum_split.h has the
// arithmetic). k_build run backwards, on the same grid: one wave per packet.
// A packet is one source range, so there is no view table and no gather: lane
// j < 21 loads window dword j of the packet's first min(len, 80) bytes, a
// packet ahead of the walk, and one ds_bpermute plus one v_alignbyte turn that
// into packet dword k in lane k. The parse, the record and the reference's
// delivery tests read those lanes with v_readlane; the IPv4 header, the pseudo
// header's addresses and the H fixed transport bytes are summed from them.
// The payload [HL + H, TL) is the only thing walked, by range_walk. A packet
// that does not split is walked for its sum alone (no room: no store). The
// control data of a packet, its offsets pair and its pay_offsets pair, are
// wave-uniform scalar loads through the constant address space (no store of
// the call may touch the tables, which may be one array) issued two packets
// ahead, so that the header load of the next packet can be issued before the
// current one is walked. The record is stored by lanes 0..7, pay_len and out
// by the lead lane.
// ---------------------------------------------------------------------
struct SplitArgs {
  uint8_t *pay;
  const uint64_t *pay_offsets;
  uint32_t *recs;  // yu_tx_record as eight dwords
  uint32_t *pay_len;
  uint16_t *out;
  uint64_t n;
};

struct SplitPkt {
  uint64_t o0, o1;  // offsets[q], offsets[q + 1]
  uint64_t p0, p1;  // pay_offsets[q], pay_offsets[q + 1]
};

template <int U, int NT>
__global__ __launch_bounds__(256) void k_split(const uint8_t *data, const uint64_t *offsets_, SplitArgs A_) {
  SplitArgs A = A_;  // what only addresses a vector store needs no scalar registers
  A.pay = in_vgpr(A_.pay);
  A.recs = in_vgpr(A_.recs);
  A.pay_len = in_vgpr(A_.pay_len);
  A.out = in_vgpr(A_.out);
  const YU_CONST_AS uint64_t *offsets = const_as(offsets_);
  const YU_CONST_AS uint64_t *pay_offsets = const_as(A.pay_offsets);
  const uint32_t lane = threadIdx.x & 63u;
  const bool lead = lane == 63;
  const uint64_t wave = grid_wave(0u);
  const uint64_t nwave = (uint64_t)gridDim.x * (blockDim.x >> 6);
  if (wave >= A.n) return;
  const uint64_t oN = offsets[A.n], pN = pay_offsets[A.n];

  // Packet q's control data (past the batch: an empty packet, nothing is loaded).
  auto packet = [&](SplitPkt &P, uint64_t q) __attribute__((always_inline)) {
    const uint64_t i = q < A.n ? q : 0;
    P.o0 = offsets[i];
    P.o1 = q < A.n ? offsets[i + 1] : P.o0;
    P.p0 = pay_offsets[i];
    P.p1 = pay_offsets[i + 1];
  };
  // Its header load: lane j's window dword j.
  auto header = [&](const SplitPkt &P) __attribute__((always_inline)) -> uint32_t {
    uint64_t addr;
    uint32_t len;
    yu::split_src((uint64_t)(uintptr_t)data, P.o0, P.o1, oN, addr, len);
    const uint32_t lim = yu::split_hdr_lim(addr, len);
    const uint64_t base = uniform64(addr & ~3ull);
    const __amdgpu_buffer_rsrc_t r = rsrc_at(base, base + lim);
    return __builtin_amdgcn_raw_buffer_load_b32(r, (int)(4u * lane < lim ? 4u * lane : kOOB), 0, 0);
  };

  const PackStore st;
  SplitPkt cur, nx, nn;
  packet(cur, wave);
  packet(nx, wave + nwave);
  uint32_t hw = header(cur);
  for (uint64_t p = wave; p < A.n; p += nwave) {
    const uint32_t hwn = header(nx);
    packet(nn, p + 2 * nwave);
    uint64_t addr;
    uint32_t len;
    yu::split_src((uint64_t)(uintptr_t)data, cur.o0, cur.o1, oN, addr, len);
    // packet dword k in lane k (lanes past the header: zeros)
    const uint32_t up = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4u * ((lane + 1u) & 63u)), (int)hw);
    const int pd = (int)yu::split_pkt_dword(up, hw, (uint32_t)addr & 3u);
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane(pd, 0), d1 = (uint32_t)__builtin_amdgcn_readlane(pd, 1);
    const uint32_t d2 = (uint32_t)__builtin_amdgcn_readlane(pd, 2), d3 = (uint32_t)__builtin_amdgcn_readlane(pd, 3);
    const uint32_t d4 = (uint32_t)__builtin_amdgcn_readlane(pd, 4);
    const int q = (int)(d0 & 15u);  // IHL: the transport header's first dword
    const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane(pd, q), t1 = (uint32_t)__builtin_amdgcn_readlane(pd, q + 1);
    const uint32_t t2 = (uint32_t)__builtin_amdgcn_readlane(pd, q + 2);
    const uint32_t t3 = (uint32_t)__builtin_amdgcn_readlane(pd, q + 3);
    yu::SplitDg S;
    yu::split_parse(S, len, d0, d2, t1, t3);
    const uint32_t hs = group_total<64>(yu::split_ip_term(S, lane, (uint32_t)pd));
    const uint32_t xs = group_total<64>(yu::split_seg_term(S, lane, (uint32_t)pd));

    const yu::IovPackDst D = yu::split_dst(S, (uint64_t)(uintptr_t)A.pay, cur.p0, cur.p1, pN);
    yu::IovWalk W;
    const int32_t vpk = yu::split_walk(W, S, addr);
    const uint2 acc = range_walk<U, NT>(W, vpk, D, st, lane, lead);
    const uint32_t sA = group_total<64>(acc.x), sB = group_total<64>(acc.y);
    if (lead) {
      A.out[p] = (uint16_t)yu::split_value(S, len, hs, xs, sA, sB);
      A.pay_len[p] = S.L;
    }
    {
      yu::BuildRec R;
      yu::split_record(R, S, d0, d1, d2, d3, d4, t0, t1, t2, t3);
      uint32_t w = R.w[0];
#pragma unroll
      for (int k = 1; k < 8; ++k) w = lane == (uint32_t)k ? R.w[k] : w;
      if (lane < 8u) A.recs[8 * p + lane] = w;
    }
    cur = nx;
    nx = nn;
    hw = hwn;
  }
}

// ---------------------------------------------------------------------
// k_parse<VERIFY, NT>: received IPv4 datagrams parsed where they lie
// (yu_rx_parse_ragged; yucsum_parse.h has the arithmetic): k_split's record and
// YU_RX_SPLIT bit, and a yu_iovec onto the payload instead of a copy of it. The
// parse, the delivery tests and the record read at most a packet's first 80
// bytes, so this is a lane per packet, 64 packets per wave step, like k_hdr,
// and no payload byte is touched. A lane reads its own offsets pair as ordinary
// loads and cuts its own packet to the batch (split_src), so an out-of-contract
// packet changes no other lane's addresses; each of its window dwords is one
// global load, made only under parse_loads (inside the packet's own window, which
// split_src has already cut to data[0, offsets[n])) and zero otherwise. Window
// dwords 0 .. 9 serve IHL 5; the five past them are loaded only when some lane
// of the step has another IHL, at window index IHL + k: a second load, never a
// runtime index into the registers already held. The record leaves as two
// 16-byte stores per lane and the view as one, contiguous across the lanes.
// VERIFY: out[i] already holds VERIFY_RX's bits, stored by the launch before this
// one on the stream; the lane that owns packet i ORs YU_RX_SPLIT into it.
// Otherwise out[i] is stored here: YU_RX_INVALID and YU_RX_SPLIT.
// ---------------------------------------------------------------------
struct ParseArgs {
  uint8_t *recs;   // yu_tx_record, 32 bytes each, 8-byte aligned
  uint8_t *views;  // yu_iovec, 16 bytes each, 8-byte aligned
  uint16_t *out;
  uint64_t n;
};

// A 16-byte store to an 8-byte aligned address (the tables' contract).
typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));

// Window loads: global memory, 4-byte aligned, one, two or four dwords.
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
#define YU_GLOBAL_AS __attribute__((address_space(1)))

template <typename T, int NT>
__device__ __forceinline__ T parse_ld(uint64_t a) {
  const YU_GLOBAL_AS T *p = (const YU_GLOBAL_AS T *)(uintptr_t)a;
  return NT ? __builtin_nontemporal_load(p) : *p;
}

template <bool VERIFY, int NT>
__global__ __launch_bounds__(256) void k_parse(const uint8_t *data, const uint64_t *offsets, ParseArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = grid_wave(0u);
  const uint64_t nwave = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint64_t oN = offsets[A.n];
  for (uint64_t p0 = wave * yu::kParsePerWave; p0 < A.n; p0 += nwave * yu::kParsePerWave) {
    const uint64_t p = p0 + lane;
    const bool act = p < A.n;  // lanes past the batch: an empty packet, nothing is loaded
    const uint64_t o0 = offsets[act ? p : A.n], o1 = offsets[act ? p + 1 : A.n];
    uint32_t flags = 0;
    if (VERIFY && act) flags = A.out[p];
    uint64_t addr;
    uint32_t len;
    yu::split_src((uint64_t)(uintptr_t)data, o0, o1, oN, addr, len);
    const uint32_t lim = yu::split_hdr_lim(addr, len), s = (uint32_t)addr & 3u;
    const uint64_t base = addr & ~3ull;
    uint32_t w[yu::kParseFix];
    if (yu::parse_whole(lim)) {  // all ten: 16 + 16 + 8 bytes
      static_assert(yu::kParseFix == 10u, "window dwords 0 .. 9 as three loads");
      const u32x4_a4 a = parse_ld<u32x4_a4, NT>(base), b = parse_ld<u32x4_a4, NT>(base + 16u);
      const u32x2_a4 c = parse_ld<u32x2_a4, NT>(base + 32u);
      w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
      w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
      w[8] = c.x, w[9] = c.y;
    } else {
#pragma unroll
      for (uint32_t j = 0; j < yu::kParseFix; ++j)
        w[j] = yu::parse_loads(j, lim) ? parse_ld<uint32_t, NT>(base + 4u * j) : 0u;
    }
    yu::ParseHdr H;
    yu::parse_fixed(H, w, s);
    const bool opt = yu::parse_needs_opt(H, len);
    if (__any((int)opt)) {
      uint32_t x[yu::kParseOpt];
#pragma unroll
      for (uint32_t k = 0; k < yu::kParseOpt; ++k) {
        const uint32_t j = yu::parse_opt_dword(H, k);
        x[k] = opt && yu::parse_loads(j, lim) ? parse_ld<uint32_t, NT>(base + 4u * j) : 0u;
      }
      if (opt) yu::parse_opt(H, x, s);
    }
    yu::SplitDg S;
    yu::split_parse(S, len, H.d0, H.d2, H.t1, H.t3);
    yu::BuildRec R;
    yu::split_record(R, S, H.d0, H.d1, H.d2, H.d3, H.d4, H.t0, H.t1, H.t2, H.t3);
    const yu::ParseView V = yu::parse_view(S, addr);
    const uint32_t bits = yu::parse_hdr_bits(S, len);
    if (act) {
      u32x4_a8 r0, r1, v;
      r0.x = R.w[0], r0.y = R.w[1], r0.z = R.w[2], r0.w = R.w[3];
      r1.x = R.w[4], r1.y = R.w[5], r1.z = R.w[6], r1.w = R.w[7];
      v.x = (uint32_t)V.base, v.y = (uint32_t)(V.base >> 32), v.z = (uint32_t)V.len, v.w = (uint32_t)(V.len >> 32);
      *(u32x4_a8 *)(A.recs + 32u * p) = r0;
      *(u32x4_a8 *)(A.recs + 32u * p + 16u) = r1;
      *(u32x4_a8 *)(A.views + 16u * p) = v;
      A.out[p] = (uint16_t)(VERIFY ? (flags | (bits & yu::kSplitFlag)) : bits);
    }
  }
}

// ---------------------------------------------------------------------
// k_demux<FLAGS, COUNT, NT>: transport demultiplexing (yu_rx_demux;
// yucsum_demux.h has the arithmetic): which registered endpoint gets each
// received packet, from the records k_parse or k_split stored. A lane per
// packet, 64 per wave step. A lane loads its record's first 16 bytes (addresses,
// ports) and the dword holding proto, and with FLAGS its flags halfword: the
// record stream, under the NT policy. An eligible lane then runs the three
// lookups of deliverPacketLocked one after the other, leaving at the first hit;
// each probe is one 16-byte load of the slot at 16 * (index & (slots - 1)),
// always a plain load, because the table is what is reused. The probe loop and
// the lookups diverge per lane; no lane reads another lane's state, and lanes
// past n load nothing. `slots` and `m` are kernel arguments computed on the host
// from the caller's m, never read from the table, so whatever the table holds a
// probe stays inside it, a lookup ends after `slots` probes, and the index a
// lane ends with is below m or YU_DEMUX_NONE. ep[i] leaves as one dword store
// per lane, contiguous across the wave.
// COUNT: the lanes of a step are converged again after the lookups. While lanes
// remain uncounted, the first one's value is broadcast, the lanes holding it are
// balloted, and that first lane alone adds their number to the value's counter:
// one no-return atomic add per distinct endpoint of the step, at most 64, not
// one per lane.
// ---------------------------------------------------------------------
struct DemuxArgs {
  const uint8_t *recs;    // yu_tx_record, 32 bytes each, 8-byte aligned
  const uint16_t *flags;  // FLAGS only
  const uint8_t *table;   // slots x 16 bytes, 16-byte aligned
  uint32_t *ep;
  uint32_t *ep_count;     // COUNT only: m + 1 counters
  uint64_t n;
  uint32_t slots, m, need;
};

struct DemuxLd {
  const uint8_t *table;
  __device__ __forceinline__ yu::DemuxSlot operator()(uint32_t i) const {
    const u32x4 v = *(const u32x4 *)(table + (uint64_t)yu::kDemuxSlotBytes * i);
    return {v.x, v.y, v.z, v.w};
  }
};

template <bool FLAGS, bool COUNT, int NT>
__global__ __launch_bounds__(256) void k_demux(DemuxArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = grid_wave(0u);
  const uint64_t nwave = (uint64_t)gridDim.x * (blockDim.x >> 6);
  DemuxLd ld = {A.table};
  for (uint64_t p0 = wave * yu::kDemuxPerWave; p0 < A.n; p0 += nwave * yu::kDemuxPerWave) {
    const uint64_t p = p0 + lane;
    const bool act = p < A.n;
    uint32_t e = yu::kDemuxNone;
    if (act) {
      const uint64_t r = (uint64_t)(uintptr_t)A.recs + 32u * p;
      const u32x4_a8 a = parse_ld<u32x4_a8, NT>(r);
      const uint32_t proto = yu::demux_rec_proto(parse_ld<uint32_t, NT>(r + 24u));
      uint32_t fl = 0;
      if (FLAGS) fl = parse_ld<uint16_t, NT>((uint64_t)(uintptr_t)(A.flags + p));
      if (yu::demux_eligible(proto, FLAGS, fl, A.need)) e = yu::demux_deliver(ld, A.slots, A.m, a.x, a.y, a.z, proto);
      A.ep[p] = e;
    }
    if (COUNT) {
      uint64_t todo = __ballot((int)act);
      while (todo) {  // uniform: every lane of the wave runs the same iterations
        const uint32_t first = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)e, (int)first);
        const uint64_t same = __ballot((int)(act && e == v));
        if (lane == first) atomicAdd(A.ep_count + yu::demux_counter(v, A.m), (uint32_t)__popcll(same));
        todo &= ~same;  // `first` is in `same`: at most 64 iterations
      }
    }
  }
}

// ---------------------------------------------------------------------
// k_reply<FLAGS, NT>: which received packets are answered, and with what
// (yu_rx_reply; yucsum_reply.h has the arithmetic): the echo of
// sample/tun_udp_echo and of ipv4.handleICMP for a batch, from the records and
// views k_parse stored and the endpoints k_demux chose. A lane per packet, 64
// per wave step, like both. A lane loads its record as two 16-byte loads and its
// view's length (the record and view streams, under the NT policy), with FLAGS
// its flags halfword, as a UDP candidate its ep dword, and, where that index is
// below m and a table is given, one byte of ep_echo, always a plain load (the
// table is what is reused). It stores the reply record as two 16-byte stores,
// 32 zero bytes for no reply, and T, the reply's length or 0, as a uint64 into
// r_offsets[i]: the launches after this one scan that array in place. No lane
// reads another lane's state, lanes past n load and store nothing, and m is a
// kernel argument, so whatever ep holds the ep_echo index stays inside the
// table. No LDS, no atomics.
// ---------------------------------------------------------------------
struct ReplyArgs {
  const uint8_t *recs;     // yu_tx_record, 32 bytes each, 8-byte aligned
  const uint16_t *flags;   // FLAGS only
  const uint8_t *views;    // yu_iovec, 16 bytes each, 8-byte aligned
  const uint32_t *ep;      // NULL without YU_REPLY_UDP_ECHO
  const uint8_t *ep_echo;  // NULL, or m bytes
  uint8_t *r_recs;
  uint64_t *r_offsets;
  uint64_t n;
  uint32_t m, need, what;
};

template <bool FLAGS, int NT>
__global__ __launch_bounds__(256) void k_reply(ReplyArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = grid_wave(0u);
  const uint64_t nwave = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const bool have_echo = A.ep_echo != nullptr;
  for (uint64_t p0 = wave * yu::kReplyPerWave; p0 < A.n; p0 += nwave * yu::kReplyPerWave) {
    const uint64_t p = p0 + lane;
    if (p >= A.n) continue;
    const uint64_t r = (uint64_t)(uintptr_t)A.recs + 32u * p;
    const u32x4_a8 a = parse_ld<u32x4_a8, NT>(r), b = parse_ld<u32x4_a8, NT>(r + 16u);
    const uint64_t L = parse_ld<uint64_t, NT>((uint64_t)(uintptr_t)A.views + 16u * p + 8u);
    uint32_t fl = 0;
    if (FLAGS) fl = parse_ld<uint16_t, NT>((uint64_t)(uintptr_t)(A.flags + p));
    const yu::BuildRec in = {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
    const uint32_t kind = yu::reply_kind(A.what, yu::reply_gate(FLAGS, fl, A.need), yu::build_proto(in), in.w[2]);
    uint32_t e = yu::kDemuxNone, echo = 0;
    if (yu::reply_reads_ep(kind)) e = parse_ld<uint32_t, NT>((uint64_t)(uintptr_t)(A.ep + p));
    if (yu::reply_reads_echo(kind, have_echo, e, A.m)) echo = A.ep_echo[e];
    yu::BuildRec out;
    const uint64_t T = yu::reply_make(out, in, L, kind, have_echo, e, A.m, echo);
    u32x4_a8 r0, r1;
    r0.x = out.w[0], r0.y = out.w[1], r0.z = out.w[2], r0.w = out.w[3];
    r1.x = out.w[4], r1.y = out.w[5], r1.z = out.w[6], r1.w = out.w[7];
    *(u32x4_a8 *)(A.r_recs + 32u * p) = r0;
    *(u32x4_a8 *)(A.r_recs + 32u * p + 16u) = r1;
    A.r_offsets[p] = T;
  }
}

// ---------------------------------------------------------------------
// k_stream: receiver.handleRcvdSegment over every TCP endpoint's queue
// (yu_rx_stream; yucsum_stream.h has the rule and the walk, yu::stream_endpoint).
// A wave per endpoint on a grid-stride loop. A wave step is up to 64 queue
// entries, lane l the l-th: order[j], then the record's two 16-byte halves and
// the view, and the next step's loads are issued before the current step is
// processed. The plain run at the front of what is left is found by a prefix sum
// of the data lengths (__shfl_up) and a ballot; its lanes store their own
// delivered slot (the view and, into s_offsets[slot], its length: the launches
// after this one scan that array in place) and their status. Every other entry is
// broadcast (__shfl) and takes yu::stream_step, the same code and the same
// addresses on all 64 lanes: the heap is read and written in global memory with
// ordinary loads and stores, never held in registers. Then the wave stores,
// lane-strided, its empty slots, the pkt resets of its heap, the words of its state
// that a walk can change (a lane each; the state byte by lane 0) and its n_acks.
// The ACK records, which are a function of that state, and the tail of lanes
// (YU_SEG_NONE for order[first[m] .. n), the empty slots past first[m] + m * cap)
// are the launch after it, k_stream_fin, a lane per element: kept apart, they do
// not lengthen what every wave of the walk holds in scalar registers.
// Store order: the general step's heap and status stores are issued by all 64 lanes
// to one address with one value, and the epilogue's lane-strided stores (a pkt reset
// by lane i, a state word by lane k) land on bytes those wrote earlier. This relies on
// one wave's stores to one address being performed in issue order whichever lane
// issues them, which holds on gfx9-class hardware (vector memory instructions of a
// wave reach the cache in order); a target without that order needs a wait between.
// `first` is clamped to n and made monotone per endpoint,
// pend_count is clamped to cap, and every packet number, slot and heap index is
// compared with its bound before the access (in yucsum_stream.h, or here for the
// lanes' own stores). No LDS, no atomics, no wave waits for another.
// ---------------------------------------------------------------------
struct StreamArgs {
  const uint8_t *recs;    // yu_tx_record, 32 bytes each
  const uint8_t *views;   // yu_iovec, 16 bytes each
  const uint32_t *order;
  const uint64_t *first;  // m + 2
  uint8_t *st;            // yu_tcp_rcv, 40 bytes each
  uint8_t *heap;          // yu_tcp_seg, 32 bytes each, m * cap
  uint8_t *status;
  uint8_t *s_views;
  uint64_t *s_offsets;
  uint32_t *n_acks;       // NULL, or m
  uint32_t n, m, cap;
};

// The Wave and Io of yu::stream_endpoint for one endpoint.
struct StreamWave {
  const StreamArgs &A;
  const uint32_t lane;
  uint32_t e;  // the endpoint: its heap is found from A.heap at each access, one pointer less to hold
  yu::StreamSeg cur, nxt;
  uint32_t cur_pl;  // yu::stream_plain_len(cur), once per step: a value in a vector register, not lane masks

  __device__ __forceinline__ uint8_t *ent(uint32_t i) const { return A.heap + 32u * ((uint64_t)e * A.cap + i); }

  __device__ __forceinline__ void load(uint64_t j0, uint32_t cnt) {
    nxt = yu::StreamSeg{0u, 0u, yu::kDemuxNone, 0u, 0u};
    if (lane >= cnt) return;
    const uint32_t pkt = A.order[j0 + lane];
    nxt.pkt = pkt;
    if (pkt >= A.n) return;  // an entry without a record: not usable, and its status has no place
    const u32x4_a8 a = *(const u32x4_a8 *)(A.recs + 32u * (uint64_t)pkt);
    const u32x4_a8 b = *(const u32x4_a8 *)(A.recs + 32u * (uint64_t)pkt + 16u);
    const u32x4_a8 v = *(const u32x4_a8 *)(A.views + 16u * (uint64_t)pkt);
    nxt.seq = a.w, nxt.fdp = yu::stream_fdp(b.y >> 16, b.y >> 24, b.z);
    nxt.base = (uint64_t)v.x | (uint64_t)v.y << 32, nxt.vlen = v.w ? 0xFFFFFFFFu : v.z;
  }
  __device__ __forceinline__ void advance() {
    cur = nxt;
    cur_pl = yu::stream_plain_len(cur);
  }

  __device__ __forceinline__ uint32_t run(const yu::StreamSt &S, const yu::StreamCtx &C, uint32_t k0, uint32_t cnt,
                                          uint32_t &sum) {
    const bool in = lane >= k0 && lane < cnt;
    const uint32_t pl = in ? cur_pl : 0u;
    uint32_t incl = pl;
    for (uint32_t o = 1; o < 64u; o <<= 1) {
      // lane - o's value (ds_bpermute, the index wrapping below lane o) under lane >= o as an
      // all-ones word that the optimiser cannot see through: as compares (__shfl_up's too)
      // the six loop-invariant lane masks are hoisted out of the whole walk and each holds a
      // scalar register pair there, which spills
      const uint32_t u = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((lane - o) & 63u) << 2), (int)incl);
      uint32_t keep = (uint32_t)((int32_t)(o - 1u - lane) >> 31);
      asm volatile("" : "+v"(keep));
      incl += u & keep;
    }
    const uint64_t ballot = __ballot(in && yu::stream_in_run(cur, pl, S, incl - pl));
    const uint32_t r = yu::stream_run_len(ballot, k0, cnt);
    sum = 0;
    if (r == 0u) return 0u;
    sum = __builtin_amdgcn_readlane(incl, k0 + r - 1u);
    if (lane >= k0 && lane < k0 + r) {
      const uint64_t slot = C.slot_lo + S.slots + (lane - k0);
      if (slot < C.slot_hi) st_slot(slot, cur.base + (yu::seg_doff(cur) - 20u), pl);
      if (cur.pkt < C.n) st_status(cur.pkt, YU_SEG_CONSUMED);
    }
    return r;
  }
  __device__ __forceinline__ void fill(uint32_t k0, uint32_t cnt, uint32_t v) {
    if (lane >= k0 && lane < cnt && cur.pkt < A.n) st_status(cur.pkt, v);
  }
  // Lane k's entry for every lane: k is wave-uniform, so these are v_readlane and the
  // general step's values and branches are scalar.
  __device__ __forceinline__ yu::StreamSeg seg(uint32_t k) const {
    yu::StreamSeg s;
    const uint32_t b0 = __builtin_amdgcn_readlane((uint32_t)cur.base, k);
    const uint32_t b1 = __builtin_amdgcn_readlane((uint32_t)(cur.base >> 32), k);
    s.base = (uint64_t)b0 | (uint64_t)b1 << 32;
    s.vlen = __builtin_amdgcn_readlane(cur.vlen, k), s.pkt = __builtin_amdgcn_readlane(cur.pkt, k);
    s.seq = __builtin_amdgcn_readlane(cur.seq, k), s.fdp = __builtin_amdgcn_readlane(cur.fdp, k);
    return s;
  }

  __device__ __forceinline__ yu::StreamEnt ld_heap(uint32_t i) const {
    const u32x4_a8 a = *(const u32x4_a8 *)ent(i);
    const u32x4_a8 b = *(const u32x4_a8 *)(ent(i) + 16u);
    return yu::StreamEnt{(uint64_t)a.x | (uint64_t)a.y << 32, a.w ? 0xFFFFFFFFu : a.z, b.x, b.y, b.z & 0xFFu};
  }
  __device__ __forceinline__ uint32_t ld_heap_seq(uint32_t i) const {
    return *(const uint32_t *)(ent(i) + 16u);
  }
  __device__ __forceinline__ void mv_heap(uint32_t to, uint32_t from) const {
    const u32x4_a8 a = *(const u32x4_a8 *)ent(from);
    const u32x4_a8 b = *(const u32x4_a8 *)(ent(from) + 16u);
    *(u32x4_a8 *)ent(to) = a;
    *(u32x4_a8 *)(ent(to) + 16u) = b;
  }
  __device__ __forceinline__ void st_heap(uint32_t i, const yu::StreamEnt &x) const {
    u32x4_a8 a, b;
    a.x = (uint32_t)x.base, a.y = (uint32_t)(x.base >> 32), a.z = x.len, a.w = 0u;
    b.x = x.seq, b.y = x.pkt, b.z = x.flags & 0xFFu, b.w = 0u;
    *(u32x4_a8 *)ent(i) = a;
    *(u32x4_a8 *)(ent(i) + 16u) = b;
  }
  __device__ __forceinline__ void st_status(uint32_t pkt, uint32_t v) const { A.status[pkt] = (uint8_t)v; }
  __device__ __forceinline__ void st_slot(uint64_t slot, uint64_t base, uint32_t len) const {
    u32x4_a8 v;
    v.x = (uint32_t)base, v.y = (uint32_t)(base >> 32), v.z = len, v.w = 0u;
    *(u32x4_a8 *)(A.s_views + 16u * slot) = v;
    A.s_offsets[slot] = len;
  }
};

template <bool RUNS>
__global__ __launch_bounds__(256) void k_stream(StreamArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)grid_wave(0u);
  const uint32_t nwave = gridDim.x * (blockDim.x >> 6);
  StreamWave W = {A, lane, 0u, {}, {}, 0u};
  for (uint32_t e = wave; e < A.m; e += nwave) {
    const uint64_t f0 = A.first[e], f1 = A.first[e + 1u];
    const uint32_t lo = f0 < A.n ? (uint32_t)f0 : A.n;
    const uint32_t hi = f1 < lo ? lo : (f1 < A.n ? (uint32_t)f1 : A.n);
    const yu::StreamCtx C = {lo + (uint64_t)e * A.cap, hi + ((uint64_t)e + 1u) * A.cap, A.n, A.cap};
    yu::StreamSt S = {};
    bool touched = false;
    uint32_t *const st = (uint32_t *)(A.st + 4u * yu::kStreamStWords * (uint64_t)e);
    if (hi > lo) {
      uint32_t w[10];
#pragma unroll
      for (uint32_t k = 0; k < 10u; ++k) w[k] = st[k];
      yu::stream_unpack(S, w);
      if (S.pend_count > A.cap) S.pend_count = A.cap;
      touched = S.state == yu::kStreamOpen || S.state == yu::kStreamClosed;
      W.e = e;
      yu::stream_endpoint(W, C, S, lo, hi - lo, RUNS);
    }
    const uint64_t room = C.slot_hi - C.slot_lo;
    for (uint64_t slot = C.slot_lo + (S.slots < room ? S.slots : room) + lane; slot < C.slot_hi; slot += 64u)
      W.st_slot(slot, 0u, 0u);
    uint32_t ln = lane;  // the lane number again, opaque: the masks below are made here, not held from the start
    asm volatile("" : "+v"(ln));
    if (touched) {
      for (uint32_t i = ln; i < S.pend_count; i += 64u) *(uint32_t *)(W.ent(i) + 20u) = yu::kDemuxNone;
      if (yu::stream_word_changes(ln)) st[ln] = yu::stream_pack_word(S, ln);
      if (ln == 0u) ((uint8_t *)st)[yu::kStreamStateByte] = (uint8_t)S.state;
    }
    if (A.n_acks && ln == 0u) A.n_acks[e] = S.n_acks;
  }
}

// yu_rx_stream's second launch, a lane per element: the ACK record of every endpoint
// from the state k_stream left and its n_acks (32 zero bytes and an offset of 0
// where that is 0; 40 left in a_offsets[e] otherwise, scanned in place afterwards),
// YU_SEG_NONE for the packets without an endpoint, order[first[m] .. n), and the
// empty slots past first[m] + m * cap, their lengths into s_offsets.
struct StreamFinArgs {
  const uint32_t *order;
  const uint64_t *first;
  const uint32_t *ids;    // yu_endpoint_id, four dwords each; read only for an endpoint that sends an ACK
  const uint32_t *st;
  const uint32_t *n_acks;
  uint8_t *a_recs;        // NULL: no ACK outputs
  uint64_t *a_offsets;
  uint8_t *status;
  uint8_t *s_views;
  uint64_t *s_offsets;
  uint32_t n, m, cap;
};

__global__ __launch_bounds__(256) void k_stream_fin(StreamFinArgs A) {
  const uint64_t tid = (uint64_t)blockIdx.x * 256u + threadIdx.x, nthreads = (uint64_t)gridDim.x * 256u;
  if (A.a_recs)
    for (uint64_t e = tid; e < A.m; e += nthreads) {
      const uint32_t na = A.n_acks[e];
      uint32_t w[10] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, id0 = 0, id1 = 0, id2 = 0;
      if (na) {
#pragma unroll
        for (uint32_t k = 0; k < 10u; ++k) w[k] = A.st[yu::kStreamStWords * e + k];
        id0 = A.ids[4u * e], id1 = A.ids[4u * e + 1u], id2 = A.ids[4u * e + 2u];
      }
      u32x4_a8 r0, r1;
      r0.x = yu::stream_ack_word(w, na, id0, id1, id2, 0u), r0.y = yu::stream_ack_word(w, na, id0, id1, id2, 1u);
      r0.z = yu::stream_ack_word(w, na, id0, id1, id2, 2u), r0.w = yu::stream_ack_word(w, na, id0, id1, id2, 3u);
      r1.x = yu::stream_ack_word(w, na, id0, id1, id2, 4u), r1.y = yu::stream_ack_word(w, na, id0, id1, id2, 5u);
      r1.z = yu::stream_ack_word(w, na, id0, id1, id2, 6u), r1.w = yu::stream_ack_word(w, na, id0, id1, id2, 7u);
      *(u32x4_a8 *)(A.a_recs + 32u * e) = r0;
      *(u32x4_a8 *)(A.a_recs + 32u * e + 16u) = r1;
      A.a_offsets[e] = na ? (uint64_t)yu::kStreamAckBytes : 0u;
    }
  uint64_t d = A.first[A.m];
  if (d > A.n) d = A.n;
  for (uint64_t j = d + tid; j < A.n; j += nthreads) {
    const uint32_t pkt = A.order[j];
    if (pkt < A.n) A.status[pkt] = (uint8_t)YU_SEG_NONE;
  }
  const uint64_t N = A.n + (uint64_t)A.m * A.cap;
  const u32x4_a8 zero = {0u, 0u, 0u, 0u};
  for (uint64_t slot = d + (uint64_t)A.m * A.cap + tid; slot < N; slot += nthreads) {
    *(u32x4_a8 *)(A.s_views + 16u * slot) = zero;
    A.s_offsets[slot] = 0u;
  }
}

// ---------------------------------------------------------------------
// The kernels of yu_rx_group (yucsum_group.h has the arithmetic and the
// picture): the packet numbers grouped by endpoint, stable, as a
// least-significant-digit radix partition of (key, packet number), key =
// min(ep[i], m), and the scans that turn counts into `first` and the grouped
// view lengths into q_offsets. Planned by yu::plan_group.
//   k_group_hist<FIRST, COUNT>    one pass's digit counts per block, digit-major.
//   k_group_scatter<FIRST, LAST>  the pass's stable scatter to the scanned places.
//   k_group_scan_sums / _mid / _add   the device-wide exclusive scan.
//   k_group_first                 one pass only: `first` read off the scanned histogram.
//   k_group_views                 q_views[j] = views[order[j]], its length to q_offsets[j].
//   k_group_zero                  dwords set to zero (the key counts; n == 0).
// FIRST: the pass reads ep and the packet number is the position; otherwise it
// reads the (key, number) pairs the pass before stored. LAST: it stores `order`
// alone. No kernel waits for another block; every place a packet number or a
// view is stored at is compared with n first, and a packet number read back from
// `order` is compared with n before it indexes `views`, so when ep changes under
// the call (the histogram and the scatter then disagree) the results are wrong
// and nothing else happens.
// ---------------------------------------------------------------------
struct GroupArgs {
  const uint32_t *ep;   // FIRST
  const uint32_t *src;  // !FIRST: n keys, then n packet numbers
  uint32_t *dst;        // !LAST: n keys, then n packet numbers
  uint32_t *order;      // LAST
  uint32_t *hist;       // [1 << digit_bits][blocks]
  uint32_t *count;      // COUNT: m + 1 key counts, zero before the launch
  uint64_t n;
  uint32_t m, pass, digit_bits, tile, blocks;
};

template <bool FIRST>
__device__ __forceinline__ uint32_t group_ld_key(const GroupArgs &A, uint64_t i) {
  return FIRST ? yu::group_key(A.ep[i], A.m) : A.src[i];
}

// The lanes of the step that hold this lane's digit: one ballot per digit bit,
// among the active lanes. Every lane of the wave calls it.
__device__ __forceinline__ uint64_t group_match(bool act, uint32_t d) {
  uint64_t same = __ballot((int)act);
#pragma unroll
  for (uint32_t b = 0; b < 8u; ++b) {
    const bool bit = (d >> b) & 1u;
    const uint64_t set = __ballot((int)(act && bit));
    same &= bit ? set : ~set;
  }
  return same;
}

template <bool FIRST, bool COUNT>
__global__ __launch_bounds__(256) void k_group_hist(GroupArgs A) {
  __shared__ uint32_t h[yu::kGroupRadixMax];
  __shared__ uint32_t none;  // COUNT: the block's packets without an endpoint
  h[threadIdx.x] = 0;
  if (threadIdx.x == 0) none = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t begin = yu::group_wave_begin(blockIdx.x, w, A.tile);
  const uint32_t steps = yu::group_wave_steps(A.tile);
  for (uint32_t s = 0; s < steps && begin + 64u * s < A.n; ++s) {  // uniform per wave
    const uint64_t i = begin + 64u * s + lane;
    const bool act = i < A.n;
    uint32_t key = 0;
    if (act) {
      key = group_ld_key<FIRST>(A, i);
      atomicAdd(&h[yu::group_digit(key, A.pass, A.digit_bits)], 1u);
    }
    if (COUNT) {
      // the key m, "no endpoint", is the one every batch may pile up on (a port nobody
      // listens on): it is counted per block, in LDS, and added once at the end, so an
      // all-miss batch makes one add per block to count[m], not one per wave step.
      // Every other key: one add per distinct key of the step, as k_demux counts.
      const uint64_t miss = __ballot((int)(act && key == A.m));
      if (lane == 0 && miss) atomicAdd(&none, (uint32_t)__popcll(miss));
      uint64_t todo = __ballot((int)(act && key != A.m));
      while (todo) {
        const uint32_t first = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)first);
        const uint64_t same = __ballot((int)(act && key == v));
        if (lane == first) atomicAdd(A.count + v, (uint32_t)__popcll(same));  // v <= m: group_key
        todo &= ~same;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < (1u << A.digit_bits))
    A.hist[yu::group_hist_at(threadIdx.x, blockIdx.x, A.blocks)] = h[threadIdx.x];
  if (COUNT && threadIdx.x == 0 && none) atomicAdd(A.count + A.m, none);
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void k_group_scatter(GroupArgs A) {
  __shared__ uint32_t cnt[yu::kGroupWaves][yu::kGroupRadixMax];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  volatile uint32_t *mine = cnt[w];  // this wave's row: LDS accesses of one wave complete in order
  for (uint32_t k = 0; k < yu::kGroupRadixMax; k += 64u) mine[k + lane] = 0;
  const uint64_t begin = yu::group_wave_begin(blockIdx.x, w, A.tile);
  const uint32_t steps = yu::group_wave_steps(A.tile);
  // walk 1: this wave's count of every digit; the lowest lane of a digit's lanes adds them
  for (uint32_t s = 0; s < steps && begin + 64u * s < A.n; ++s) {
    const uint64_t i = begin + 64u * s + lane;
    const bool act = i < A.n;
    const uint32_t d = act ? yu::group_digit(group_ld_key<FIRST>(A, i), A.pass, A.digit_bits) : 0u;
    const uint64_t same = group_match(act, d);
    if (act && (same & (((uint64_t)1 << lane) - 1u)) == 0) mine[d] = mine[d] + (uint32_t)__popcll(same);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {  // counts to places: the scanned histogram, plus the earlier waves of this block
    const uint32_t d = threadIdx.x;
    uint32_t at = d < (1u << A.digit_bits) ? A.hist[yu::group_hist_at(d, blockIdx.x, A.blocks)] : 0u;
    for (uint32_t k = 0; k < yu::kGroupWaves; ++k) {
      const uint32_t c = cnt[k][d];
      cnt[k][d] = at;
      at += c;
    }
  }
  __syncthreads();
  // walk 2: place = the wave's running place of the digit + the lower lanes holding it
  for (uint32_t s = 0; s < steps && begin + 64u * s < A.n; ++s) {
    const uint64_t i = begin + 64u * s + lane;
    const bool act = i < A.n;
    const uint32_t key = act ? group_ld_key<FIRST>(A, i) : 0u;
    const uint32_t d = yu::group_digit(key, A.pass, A.digit_bits);
    const uint64_t same = group_match(act, d);
    const uint32_t rank = (uint32_t)__popcll(same & (((uint64_t)1 << lane) - 1u));
    uint32_t pos = 0;
    if (act) pos = mine[d] + rank;
    __builtin_amdgcn_wave_barrier();  // every lane has read before the lowest one writes
    if (act && rank == 0) mine[d] = pos + (uint32_t)__popcll(same);
    __builtin_amdgcn_wave_barrier();
    if (act && pos < A.n) {
      const uint32_t num = FIRST ? (uint32_t)i : A.src[A.n + i];
      if (LAST) {
        A.order[pos] = num;
      } else {
        A.dst[pos] = key;
        A.dst[A.n + pos] = num;
      }
    }
  }
}

// Exclusive prefix of v over the block's 256 threads in thread order, and the
// block's total: a shuffle scan per wave, the four wave totals through LDS.
__device__ __forceinline__ uint64_t group_block_scan(uint64_t v, uint64_t *wsum, uint64_t &total) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  unsigned long long incl = v;
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const unsigned long long u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63u) wsum[w] = incl;
  __syncthreads();
  uint64_t before = 0;
  total = 0;
  for (uint32_t k = 0; k < yu::kGroupWaves; ++k) {
    if (k < w) before += wsum[k];
    total += wsum[k];
  }
  return before + incl - v;
}

template <typename TIn>
__global__ __launch_bounds__(256) void k_group_scan_sums(const TIn *in, uint64_t n_in, uint64_t *sums) {
  __shared__ uint64_t wsum[yu::kGroupWaves];
  const uint64_t base = (uint64_t)blockIdx.x * yu::kGroupScanTile + threadIdx.x * yu::kGroupScanPer;
  uint64_t v = 0;
#pragma unroll
  for (uint32_t k = 0; k < yu::kGroupScanPer; ++k)
    if (base + k < n_in) v += in[base + k];
  uint64_t total;
  group_block_scan(v, wsum, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// One block: thread t takes the t-th run of the tile sums.
__global__ __launch_bounds__(256) void k_group_scan_mid(uint64_t *sums, uint64_t tiles) {
  __shared__ uint64_t wsum[yu::kGroupWaves];
  const uint64_t run = yu::group_scan_run(tiles);
  const uint64_t lo = threadIdx.x * run < tiles ? threadIdx.x * run : tiles;
  const uint64_t hi = lo + run < tiles ? lo + run : tiles;
  uint64_t v = 0;
  for (uint64_t i = lo; i < hi; ++i) v += sums[i];
  uint64_t total;
  uint64_t acc = group_block_scan(v, wsum, total);
  for (uint64_t i = lo; i < hi; ++i) {
    const uint64_t x = sums[i];
    sums[i] = acc;
    acc += x;
  }
}

// in == out is allowed: a thread loads its elements before the block's barrier and
// stores the same positions after it.
template <typename TIn, typename TOut>
__global__ __launch_bounds__(256) void k_group_scan_add(const TIn *in, uint64_t n_in, TOut *out, uint64_t n_out,
                                                        const uint64_t *sums) {
  __shared__ uint64_t wsum[yu::kGroupWaves];
  const uint64_t base = (uint64_t)blockIdx.x * yu::kGroupScanTile + threadIdx.x * yu::kGroupScanPer;
  uint64_t x[yu::kGroupScanPer];
  uint64_t v = 0;
#pragma unroll
  for (uint32_t k = 0; k < yu::kGroupScanPer; ++k) {
    x[k] = base + k < n_in ? (uint64_t)in[base + k] : 0u;
    v += x[k];
  }
  uint64_t total;
  uint64_t acc = group_block_scan(v, wsum, total) + sums[blockIdx.x];
#pragma unroll
  for (uint32_t k = 0; k < yu::kGroupScanPer; ++k) {
    if (base + k < n_out) out[base + k] = (TOut)acc;
    acc += x[k];
  }
}

// One pass: the digit is the whole key, so block 0's scanned count of digit e is the
// number of packets with a key below e.
__global__ __launch_bounds__(256) void k_group_first(const uint32_t *hist, uint32_t blocks, uint64_t n, uint32_t m,
                                                     uint64_t *first) {
  for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < (uint64_t)m + 2u; e += (uint64_t)gridDim.x * 256u)
    first[e] = e <= m ? (uint64_t)hist[yu::group_hist_at((uint32_t)e, 0u, blocks)] : n;
}

__global__ __launch_bounds__(256) void k_group_views(const uint32_t *order, const uint8_t *views,
                                                     const uint64_t *first, uint64_t n, uint32_t m, uint8_t *q_views,
                                                     uint64_t *q_offsets) {
  const uint64_t delivered = first[m];
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256u) {
    const uint32_t o = order[j];
    u32x4_a8 v = {0u, 0u, 0u, 0u};
    if (j < delivered && o < n) v = *(const u32x4_a8 *)(views + 16u * (uint64_t)o);
    *(u32x4_a8 *)(q_views + 16u * j) = v;
    q_offsets[j] = (uint64_t)v.z | (uint64_t)v.w << 32;  // scanned in place afterwards
  }
}

__global__ __launch_bounds__(256) void k_group_zero(uint32_t *p, uint64_t dwords, uint32_t *q, uint64_t q_dwords) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < dwords; i += (uint64_t)gridDim.x * 256u) p[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x < q_dwords) q[threadIdx.x] = 0;
}

// ---------------------------------------------------------------------
// Host side: launch. Which kernel, form, load policy and grid a batch gets is
// yu::plan's decision (yucsum_plan.cpp); here are the functions it names.
// ---------------------------------------------------------------------
typedef void (*KernelFn)(BatchArgs);

struct KernelFns {
  KernelFn fn[3];     // by load policy (bld16): plain, nt, hybrid; k_small: with runs
  KernelFn inter[3];  // k_small without runs (PR = 0), by load policy
  KernelFn fill;      // the in-place instantiation of a kernel that has its own
};

// One row per entry of YU_KERNELS (yucsum_plan.h), from each family's template
// arguments. Only k_small has a hybrid policy: elsewhere slot 2 repeats nt, and
// plain for k_hdr.
#define YU_FNS_Lane(U) {{k_lane<U, 0>, k_lane<U, 1>, k_lane<U, 1>}, {}, nullptr}
#define YU_TINY_FILL_true(G) k_tiny<G, 1, true>
#define YU_TINY_FILL_false(G) nullptr
#define YU_FNS_Tiny(G, OWN_FILL) \
  {{k_tiny<G, 0>, k_tiny<G, 1>, k_tiny<G, 1>}, {}, YU_TINY_FILL_##OWN_FILL(G)}
#define YU_FNS_Small(G, U)                                                                   \
  {{k_small<G, U, 0, yu::kSmallRun>, k_small<G, U, 1, yu::kSmallRun>,                        \
    k_small<G, U, 2, yu::kSmallRun>},                                                        \
   {k_small<G, U, 0, 0>, k_small<G, U, 1, 0>, k_small<G, U, 2, 0>}, nullptr}
#define YU_LOOP_loop_le(NT) k_loop<4, NT, false>
#define YU_LOOP_loop_be(NT) k_loop<4, NT, true>
#define YU_LOOP_loop_rx(NT) k_loop_rx<4, NT>
#define YU_LOOP_loop_dg(NT) k_loop_rx<4, NT, true>
#define YU_FNS_Loop(ID) {{YU_LOOP_##ID(0), YU_LOOP_##ID(1), YU_LOOP_##ID(1)}, {}, nullptr}
#define YU_FNS_Hdr() {{k_hdr<0>, k_hdr<1>, k_hdr<0>}, {}, nullptr}
#define YU_FNS_Seg(U, KIND, CH)                                                              \
  {{k_seg<U, 0, kSeg##KIND, CH>, k_seg<U, 1, kSeg##KIND, CH>, k_seg<U, 1, kSeg##KIND, CH>}, \
   {}, nullptr}
#define YU_X(id, name, family, window, G, ppw, run, grid, own_fill, fill_plain, tile, kind, \
             ragged_fill, targs)                                                           \
  YU_FNS_##family targs,
const KernelFns kFns[] = {YU_KERNELS(YU_X)};
#undef YU_X
static_assert(sizeof(kFns) / sizeof(kFns[0]) == yu::kKernelCount, "one row per kernel");

KernelFn kernel_fn(const yu::Plan &p) {
  const KernelFns &f = kFns[p.kernel];
  if (p.form == yu::Form::Fill) return f.fill;
  return p.form == yu::Form::Inter ? f.inter[p.policy] : f.fn[p.policy];
}

std::atomic<int> g_cu_count[64];

int cu_count(int dev) {
  if (dev < 0 || dev >= 64) return 256;
  int c = g_cu_count[dev].load(std::memory_order_relaxed);
  if (c > 0) return c;
  if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) !=
          hipSuccess ||
      c <= 0)
    c = 256;
  g_cu_count[dev].store(c, std::memory_order_relaxed);
  return c;
}

int hip_status(hipError_t e) {
  if (e == hipSuccess) return YU_OK;
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return YU_ENODEV;
  if (e == hipErrorOutOfMemory) return YU_ENOMEM;
  return YU_EHIP_BASE - (int)e;
}

int launch(const yu::Shape &s, const BatchArgs &A, hipStream_t stream) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_status(e);
  const yu::Plan p = yu::plan(s, cu_count(dev), yu::env_knobs());
  BatchArgs a = A;
  a.uf = p.uf;
  a.xcd = p.xcd;
  a.small_waves = p.small_waves;
  hipLaunchKernelGGL(kernel_fn(p), dim3(p.blocks), dim3(256), 0, stream, a);
  return hip_status(hipGetLastError());
}

// The yu_*_variant* calls: the plan's kernel name (no CU count enters that).
const char *variant_name(const yu::Shape &s) {
  return yu::plan(s, 256, yu::env_knobs()).name;
}

bool aligned(const void *p, uintptr_t a) {
  return ((uintptr_t)p & (a - 1)) == 0;
}

int check_common(int mode, const uint16_t *initial_arr, const uint8_t *addrs,
                 const uint16_t *out, bool fill, uint64_t n) {
  if (mode < 0 || mode >= YU_MODE_COUNT) return YU_EINVAL;  // EINVAL:mode
  if (!out && !fill && n) return YU_EINVAL;                // EINVAL:out (an empty batch may pass NULL)
  if (fill && !mode_fills(mode)) return YU_EINVAL;         // EINVAL:fill-mode
  if (initial_arr && !aligned(initial_arr, 2)) return YU_EINVAL;  // EINVAL:side-align
  if (addrs && !aligned(addrs, 4)) return YU_EINVAL;              // EINVAL:side-align
  if (out && !aligned(out, 2)) return YU_EINVAL;                  // EINVAL:side-align
  return YU_OK;
}

int batch_uniform(const uint8_t *data, uint8_t *fill, uint64_t stride,
                  uint32_t len, uint64_t n, int mode,
                  const uint16_t *initial_arr, uint16_t initial,
                  const uint8_t *addrs, uint16_t *out, void *stream) {
  int rc = check_common(mode, initial_arr, addrs, out, fill != nullptr, n);
  if (rc) return rc;
  if (n == 0) return YU_OK;
  if (!data) return YU_EINVAL;                                              // EINVAL:data
  if (mode != YU_MODE_RAW && len > YU_MAX_TRANSPORT_LEN) return YU_EINVAL;  // EINVAL:len-transport
  if (len < min_len(mode)) return YU_EINVAL;                                // EINVAL:len-min
  if (len > YU_MAX_RAW_LEN) return YU_EINVAL;  // EINVAL:len-raw (window offsets stay in uint32)
  // the batch [data, data + (n-1)*stride + len) must not wrap the address space
  if (n > 1 && stride > (UINT64_MAX - (uint64_t)(uintptr_t)data - len) / (n - 1))
    return YU_EINVAL;  // EINVAL:span
  // fill: packets must start 4-byte aligned. The uniform writers (k_tiny's and
  // k_lane's write-back, k_small) store whole dwords of each packet's window,
  // so no dword may hold bytes of two packets.
  if (fill && (((uintptr_t)data | stride) & 3u)) return YU_EINVAL;  // EINVAL:fill-align
  BatchArgs A;
  A.data = data;
  A.offsets = nullptr;
  A.initial_arr = initial_arr;
  A.addrs = addrs;
  A.out = out;
  A.fill = fill;
  A.stride = stride;
  A.n = n;
  A.end = (uint64_t)(uintptr_t)data + (n - 1) * stride + len;
  A.len = len;
  A.initial = initial;
  A.mode = mode;
  return launch({false, (uintptr_t)data, stride, len, n, mode, fill != nullptr}, A, (hipStream_t)stream);
}

int batch_ragged(const uint8_t *data, uint8_t *fill, const uint64_t *offsets,
                 uint64_t n, int mode, const uint16_t *initial_arr,
                 uint16_t initial, const uint8_t *addrs, uint16_t *out,
                 void *stream) {
  int rc = check_common(mode, initial_arr, addrs, out, fill != nullptr, n);
  if (rc) return rc;
  if (n == 0) return YU_OK;
  if (!offsets || !aligned(offsets, 8)) return YU_EINVAL;  // EINVAL:offsets
  if (!data) return YU_EINVAL;                             // EINVAL:data
  BatchArgs A;
  A.data = data;
  A.offsets = offsets;
  A.initial_arr = initial_arr;
  A.addrs = addrs;
  A.out = out;
  A.fill = fill;
  A.stride = 0;
  A.n = n;
  A.end = 0;
  A.len = 0;
  A.initial = initial;
  A.uf = 0;
  A.mode = mode;
  // k_seg streams the batch's bytes (exact BE recovery for chunks holding a
  // RAW packet > 131072 bytes); k_hdr takes the IPv4 header-only modes.
  return launch({true, 0, 0, 0, n, mode, fill != nullptr}, A, (hipStream_t)stream);
}

// The wave-per-packet kernels: one row per entry of YU_WAVE_KERNELS
// (yucsum_plan.h), by load policy, from each family's template arguments. The
// signatures differ (the packing forms add dst and dst_offsets, the datagram
// packing form takes no side arrays, k_build and k_split their own tables), so a
// row fills the member of its signature and leaves the others null.
struct WaveFns {
  void (*iov[3])(const yu_iovec *, const uint64_t *, const uint16_t *, const uint8_t *, IovArgs);
  void (*pack[3])(const yu_iovec *, const uint64_t *, const uint16_t *, const uint8_t *, PackArgs);
  void (*pack_dg[3])(const yu_iovec *, const uint64_t *, PackArgs);
  void (*build[3])(const uint8_t *, const uint64_t *, const yu_tx_record *, BuildArgs);
  void (*split[3])(const uint8_t *, const uint64_t *, SplitArgs);
};
#define YU_WFNS_Iov(U, FILL, DG) \
  {{k_iov<U, 0, FILL, DG>, k_iov<U, 1, FILL, DG>, k_iov<U, 2, FILL, DG>}, {}, {}, {}, {}}
#define YU_WFNS_Pack_false(U, FILL) \
  {{}, {k_pack<U, 0, FILL>, k_pack<U, 1, FILL>, k_pack<U, 2, FILL>}, {}, {}, {}}
#define YU_WFNS_Pack_true(U, FILL) \
  {{}, {}, {k_pack_dg<U, 0, FILL>, k_pack_dg<U, 1, FILL>, k_pack_dg<U, 2, FILL>}, {}, {}}
#define YU_WFNS_Pack(U, FILL, DG) YU_WFNS_Pack_##DG(U, FILL)
#define YU_WFNS_Build(U) {{}, {}, {}, {k_build<U, 0>, k_build<U, 1>, k_build<U, 2>}, {}}
#define YU_WFNS_Split(U) {{}, {}, {}, {}, {k_split<U, 0>, k_split<U, 1>, k_split<U, 2>}}
#define YU_X(id, name, family, dg, fill, targs) YU_WFNS_##family targs,
const WaveFns kWaveFns[] = {YU_WAVE_KERNELS(YU_X)};
#undef YU_X
static_assert(sizeof(kWaveFns) / sizeof(kWaveFns[0]) == yu::kWaveKernelCount, "one row per kernel");

// A wave-per-packet launch: the device's plan, then the plan's kernel, taken from
// the member `sig` of its row, with `args`.
template <typename Fn, typename... Args>
int launch_wave(Fn (WaveFns::*sig)[3], yu::WaveFamily family, uint64_t n, int mode, bool fill, void *stream,
                Args... args) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_status(e);
  const yu::WavePlan p = yu::plan_wave(family, n, mode, fill, cu_count(dev), yu::env_knobs());
  hipLaunchKernelGGL((kWaveFns[p.kernel].*sig)[p.policy], dim3(p.blocks), dim3(256), 0, (hipStream_t)stream,
                     args...);
  return hip_status(hipGetLastError());
}

// A scatter-gather device call. dg: the form for whole IPv4 datagrams, the modes
// that parse headers out of the packet, which takes no side arrays (initial_arr,
// addrs: null; initial: 0). pack: the packing form, with dst and dst_offsets
// (null otherwise).
struct IovCall {
  bool dg, pack;
  const yu_iovec *views;
  const uint64_t *first_iov;
  uint64_t n;
  int mode;
  const uint16_t *initial_arr;
  uint16_t initial;
  const uint8_t *addrs;
  uint8_t *dst;
  const uint64_t *dst_offsets;
  uint16_t *out;
  bool fill;
  void *stream;
};

// Its arguments. The tables are device memory and are not read here
// (include/yucsum.h, "Out of contract"); an empty batch passes before they are
// looked at.
int check_iov(const IovCall &c) {
  const int mode = c.mode;
  if (mode < 0 || mode >= YU_MODE_COUNT) return YU_EINVAL;      // EINVAL:mode
  if (c.dg && !yu::iov_dg_mode_ok(mode)) return YU_EINVAL;       // EINVAL:mode (a whole-packet sum: the whole-packet form takes it)
  if (c.fill && !(c.dg ? yu::iov_dg_mode_tx(mode) : yu::iov_mode_tx(mode)))
    return YU_EINVAL;  // EINVAL:fill-mode (no field: VERIFY_IPV4, VERIFY_RX store none; or a mode this form refuses)
  if (!c.dg && !yu::iov_mode_ok(mode)) return YU_EINVAL;         // EINVAL:mode (IPV4, VERIFY_IPV4, VERIFY_RX, TX_DATAGRAM parse headers)
  if (!c.out && !c.fill && c.n) return YU_EINVAL;                // EINVAL:out
  if (c.initial_arr && !aligned(c.initial_arr, 2)) return YU_EINVAL;  // EINVAL:side-align
  if (c.addrs && !aligned(c.addrs, 4)) return YU_EINVAL;              // EINVAL:side-align
  if (c.out && !aligned(c.out, 2)) return YU_EINVAL;                  // EINVAL:side-align
  if (c.n == 0) return YU_OK;
  if (!c.first_iov || !aligned(c.first_iov, 8) || !aligned(c.views, 8)) return YU_EINVAL;  // EINVAL:offsets
  if (c.pack && (!c.dst_offsets || !aligned(c.dst_offsets, 8))) return YU_EINVAL;         // EINVAL:offsets
  if (!c.views || (c.pack && !c.dst)) return YU_EINVAL;                                   // EINVAL:data
  return YU_OK;
}

// The call: checked, then the device's plan and its kernel's launch.
int call_iov(const IovCall &c) {
  const int rc = check_iov(c);
  if (rc != YU_OK || c.n == 0) return rc;
  if (!c.pack) {
    const IovArgs a = {c.out, c.n, c.initial, c.mode};
    return launch_wave(&WaveFns::iov, yu::WaveFamily::Iov, c.n, c.mode, c.fill, c.stream, c.views, c.first_iov,
                       c.initial_arr, c.addrs, a);
  }
  const PackArgs a = {c.out, c.dst, c.dst_offsets, c.n, c.initial, c.mode};
  if (c.dg)
    return launch_wave(&WaveFns::pack_dg, yu::WaveFamily::Pack, c.n, c.mode, c.fill, c.stream, c.views,
                       c.first_iov, a);
  return launch_wave(&WaveFns::pack, yu::WaveFamily::Pack, c.n, c.mode, c.fill, c.stream, c.views, c.first_iov,
                     c.initial_arr, c.addrs, a);
}

// The yu_iov*_variant_n calls: "" for a mode (or a fill) the form refuses.
const char *iov_variant(bool dg, bool pack, int mode, uint64_t n, int fill) {
  if (mode < 0 || mode >= YU_MODE_COUNT) return "";
  if (!(dg ? yu::iov_dg_mode_ok(mode) : yu::iov_mode_ok(mode))) return "";
  if (fill && !(dg ? yu::iov_dg_mode_tx(mode) : yu::iov_mode_tx(mode))) return "";
  const yu::WaveFamily family = pack ? yu::WaveFamily::Pack : yu::WaveFamily::Iov;
  return yu::plan_wave(family, n, mode, fill != 0, 256, yu::env_knobs()).name;
}

// yu_tx_build_ragged: the record as the kernel reads it (eight little-endian
// dwords, yu::BuildRec), its arguments, then the device's plan and the launch.
static_assert(sizeof(yu_tx_record) == 32, "yu_tx_record is 32 bytes");
static_assert(offsetof(yu_tx_record, src) == 0, "yu_tx_record.src");
static_assert(offsetof(yu_tx_record, dst) == 4, "yu_tx_record.dst");
static_assert(offsetof(yu_tx_record, sport) == 8, "yu_tx_record.sport");
static_assert(offsetof(yu_tx_record, dport) == 10, "yu_tx_record.dport");
static_assert(offsetof(yu_tx_record, seq) == 12, "yu_tx_record.seq");
static_assert(offsetof(yu_tx_record, ack) == 16, "yu_tx_record.ack");
static_assert(offsetof(yu_tx_record, window) == 20, "yu_tx_record.window");
static_assert(offsetof(yu_tx_record, flags) == 22, "yu_tx_record.flags");
static_assert(offsetof(yu_tx_record, doff) == 23, "yu_tx_record.doff");
static_assert(offsetof(yu_tx_record, proto) == 24, "yu_tx_record.proto");
static_assert(offsetof(yu_tx_record, ttl) == 25, "yu_tx_record.ttl");
static_assert(offsetof(yu_tx_record, ip_id) == 26, "yu_tx_record.ip_id");
static_assert(offsetof(yu_tx_record, tos) == 28, "yu_tx_record.tos");
static_assert(offsetof(yu_tx_record, reserved) == 29, "yu_tx_record.reserved");
static_assert(offsetof(yu_tx_record, frag) == 30, "yu_tx_record.frag");

int tx_build(const uint8_t *payload, const uint64_t *pay_offsets, const yu_tx_record *recs, uint64_t n,
             uint8_t *dst, const uint64_t *dst_offsets, uint16_t *out, void *stream) {
  if (out && !aligned(out, 2)) return YU_EINVAL;  // EINVAL:side-align
  if (n == 0) return YU_OK;
  if (!pay_offsets || !aligned(pay_offsets, 8) || !dst_offsets || !aligned(dst_offsets, 8) || !aligned(recs, 8))
    return YU_EINVAL;  // EINVAL:offsets
  if (!payload || !recs || !dst) return YU_EINVAL;  // EINVAL:data
  const BuildArgs a = {dst, dst_offsets, out, n};
  return launch_wave(&WaveFns::build, yu::WaveFamily::Build, n, 0, false, stream, payload, pay_offsets, recs, a);
}

// yu_tx_build_iov: its arguments, then k_build's plan row for the grid and the
// load policy, and this call's own kernel by that policy.
constexpr char kBuildIovName[] = "k_build<4,iov>";
int tx_build_iov(const yu_iovec *views, const yu_tx_record *recs, uint64_t n, uint8_t *dst,
                 const uint64_t *dst_offsets, uint16_t *out, void *stream) {
  if (out && !aligned(out, 2)) return YU_EINVAL;  // EINVAL:side-align
  if (n == 0) return YU_OK;
  if (!dst_offsets || !aligned(dst_offsets, 8) || !aligned(views, 8) || !aligned(recs, 8))
    return YU_EINVAL;  // EINVAL:offsets
  if (!views || !recs || !dst) return YU_EINVAL;  // EINVAL:data
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_status(e);
  const yu::WavePlan p = yu::plan_wave(yu::WaveFamily::Build, n, 0, false, cu_count(dev), yu::env_knobs());
  void (*const fn[3])(const yu_iovec *, const yu_tx_record *, BuildArgs) = {k_build_iov<4, 0>, k_build_iov<4, 1>,
                                                                            k_build_iov<4, 2>};
  const BuildArgs a = {dst, dst_offsets, out, n};
  hipLaunchKernelGGL(fn[p.policy], dim3(p.blocks), dim3(256), 0, (hipStream_t)stream, views, recs, a);
  return hip_status(hipGetLastError());
}

// yu_rx_split_ragged: its arguments, then the device's plan and the launch.
int rx_split(const uint8_t *data, const uint64_t *offsets, uint64_t n, uint8_t *pay, const uint64_t *pay_offsets,
             yu_tx_record *recs, uint32_t *pay_len, uint16_t *out, void *stream) {
  if (!aligned(out, 2) || !aligned(pay_len, 4)) return YU_EINVAL;  // EINVAL:side-align
  if (n == 0) return YU_OK;
  if (!out) return YU_EINVAL;  // EINVAL:out
  if (!offsets || !aligned(offsets, 8) || !pay_offsets || !aligned(pay_offsets, 8) || !aligned(recs, 8))
    return YU_EINVAL;  // EINVAL:offsets
  if (!data || !pay || !recs || !pay_len) return YU_EINVAL;  // EINVAL:data
  const SplitArgs a = {pay, pay_offsets, (uint32_t *)recs, pay_len, out, n};
  return launch_wave(&WaveFns::split, yu::WaveFamily::Split, n, 0, false, stream, data, offsets, a);
}

// yu_rx_parse_ragged: its arguments; with `verify` the VERIFY_RX launch exactly as
// yu_csum_batch_ragged makes it (yu::plan's kernel, which stores out), then
// k_parse on yu::plan_parse's grid, on the same stream.
int rx_parse(const uint8_t *data, const uint64_t *offsets, uint64_t n, int verify, yu_tx_record *recs,
             yu_iovec *pay_views, uint16_t *out, void *stream) {
  if (!aligned(out, 2)) return YU_EINVAL;  // EINVAL:side-align
  if (n == 0) return YU_OK;
  if (!out) return YU_EINVAL;  // EINVAL:out
  if (!offsets || !aligned(offsets, 8) || !aligned(recs, 8) || !aligned(pay_views, 8))
    return YU_EINVAL;  // EINVAL:offsets
  if (!data || !recs || !pay_views) return YU_EINVAL;  // EINVAL:data
  if (verify) {
    const int rc = batch_ragged(data, nullptr, offsets, n, YU_MODE_VERIFY_RX, nullptr, 0, nullptr, out, stream);
    if (rc != YU_OK) return rc;
  }
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_status(e);
  const yu::ParsePlan p = yu::plan_parse(n, cu_count(dev), yu::env_knobs());
  const ParseArgs a = {(uint8_t *)recs, (uint8_t *)pay_views, out, n};
  void (*const fn[2][2])(const uint8_t *, const uint64_t *, ParseArgs) = {{k_parse<false, 0>, k_parse<false, 1>},
                                                                          {k_parse<true, 0>, k_parse<true, 1>}};
  hipLaunchKernelGGL(fn[verify ? 1 : 0][p.policy], dim3(p.blocks), dim3(256), 0, (hipStream_t)stream, data, offsets,
                     a);
  return hip_status(hipGetLastError());
}

// yu_demux_table_fill: its checks, then yu::demux_fill (yucsum_demux.h). Host
// memory only; no HIP call.
int demux_table_fill(const yu_endpoint_id *ids, uint64_t m, void *h_table, uint64_t table_bytes, uint64_t *bad) {
  if (bad) *bad = m;
  if (m > yu::kDemuxMax || table_bytes != yu::demux_table_bytes(m)) return YU_EINVAL;  // EINVAL:data
  if (m > 0 && (!ids || !h_table)) return YU_EINVAL;                                   // EINVAL:data
  const uint64_t b = yu::demux_fill(ids, m, h_table);
  if (b > m) return YU_ENOMEM;
  if (bad) *bad = b;
  if (b < m) return YU_EINVAL;  // EINVAL:data
  return YU_OK;
}

// yu_rx_demux: its arguments, then k_demux on yu::plan_demux's grid. The slot
// count the kernel masks with comes from m here, never from the table.
int rx_demux(const yu_tx_record *recs, const uint16_t *flags, uint16_t need, uint64_t n, const void *table,
             uint64_t table_bytes, uint64_t m, uint32_t *ep, uint32_t *ep_count, void *stream) {
  if (!aligned(flags, 2) || !aligned(ep, 4) || !aligned(ep_count, 4)) return YU_EINVAL;  // EINVAL:side-align
  if (m > yu::kDemuxMax || table_bytes != yu::demux_table_bytes(m)) return YU_EINVAL;    // EINVAL:data
  if (n == 0) return YU_OK;
  if (!ep) return YU_EINVAL;                                     // EINVAL:out
  if (!aligned(recs, 8) || !aligned(table, 16)) return YU_EINVAL;  // EINVAL:offsets
  if (!recs || !table) return YU_EINVAL;                         // EINVAL:data
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_status(e);
  const yu::DemuxPlan p = yu::plan_demux(n, cu_count(dev), yu::env_knobs());
  const DemuxArgs a = {(const uint8_t *)recs, flags, (const uint8_t *)table, ep, ep_count, n,
                       yu::demux_slots(m), (uint32_t)m, need};
  void (*const fn[2][2][2])(DemuxArgs) = {
      {{k_demux<false, false, 0>, k_demux<false, false, 1>}, {k_demux<false, true, 0>, k_demux<false, true, 1>}},
      {{k_demux<true, false, 0>, k_demux<true, false, 1>}, {k_demux<true, true, 0>, k_demux<true, true, 1>}}};
  hipLaunchKernelGGL(fn[flags ? 1 : 0][ep_count ? 1 : 0][p.policy], dim3(p.blocks), dim3(256), 0, (hipStream_t)stream,
                     a);
  return hip_status(hipGetLastError());
}

// The device-wide exclusive scan of yu_rx_group: out[i] = the sum of in[0, i) for
// i < n_out, inputs at and past n_in taken as 0; `sums` holds one uint64 per tile of
// kGroupScanTile outputs. Three launches, none waiting for another block. in == out
// is allowed.
template <typename TIn, typename TOut>
void group_scan(const TIn *in, uint64_t n_in, TOut *out, uint64_t n_out, uint64_t *sums, hipStream_t stream) {
  const uint64_t tiles = yu::group_scan_tiles(n_out);
  hipLaunchKernelGGL(k_group_scan_sums<TIn>, dim3((uint32_t)tiles), dim3(256), 0, stream, in, n_in, sums);
  hipLaunchKernelGGL(k_group_scan_mid, dim3(1), dim3(256), 0, stream, sums, tiles);
  hipLaunchKernelGGL((k_group_scan_add<TIn, TOut>), dim3((uint32_t)tiles), dim3(256), 0, stream, in, n_in, out, n_out,
                     (const uint64_t *)sums);
}

// yu_rx_group: its arguments, then yu::plan_group's launches in the caller's
// workspace. The layout of `work` does not depend on the device.
int rx_group(const uint32_t *ep, uint64_t n, uint64_t m, const yu_iovec *views, uint32_t *order, uint64_t *first,
             yu_iovec *q_views, uint64_t *q_offsets, void *work, uint64_t work_bytes, void *stream_) {
  if (!aligned(first, 8) || !aligned(q_offsets, 8) || !aligned(views, 8) || !aligned(q_views, 8) ||
      !aligned(work, 16))
    return YU_EINVAL;                                              // EINVAL:offsets
  if (!aligned(ep, 4) || !aligned(order, 4)) return YU_EINVAL;     // EINVAL:side-align
  if (m > yu::kGroupMaxEndpoints || n >= (1ull << 32)) return YU_EINVAL;  // EINVAL:data
  if (!first) return YU_EINVAL;                                    // EINVAL:out
  hipStream_t stream = (hipStream_t)stream_;
  int dev = 0;
  if (n == 0) {  // the empty CSR is stored: no caller meets an undefined one
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_status(e);
    hipLaunchKernelGGL(k_group_zero, dim3((uint32_t)((2u * (m + 2u) + 255u) / 256u)), dim3(256), 0, stream,
                       (uint32_t *)first, 2u * (m + 2u), (uint32_t *)q_offsets, (uint64_t)(q_offsets ? 2u : 0u));
    return hip_status(hipGetLastError());
  }
  if (!order) return YU_EINVAL;                                    // EINVAL:out
  const yu::GroupPlan p0 = yu::plan_group(n, m, 256, yu::Knobs());
  if (!ep || !work || work_bytes < p0.bytes) return YU_EINVAL;     // EINVAL:data
  if ((views != nullptr) != (q_views != nullptr) || (views != nullptr) != (q_offsets != nullptr))
    return YU_EINVAL;                                              // EINVAL:data
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_status(e);
  const yu::GroupPlan p = yu::plan_group(n, m, cu_count(dev), yu::env_knobs());
  uint8_t *const w = (uint8_t *)work;
  uint32_t *const hist = (uint32_t *)(w + p.hist_off);
  uint64_t *const sums = (uint64_t *)(w + p.sums_off);
  uint32_t *const count = (uint32_t *)(w + p.count_off);
  uint32_t *const pair[2] = {(uint32_t *)(w + p.pair_off[0]), (uint32_t *)(w + p.pair_off[1])};
  if (p.passes > 1)
    hipLaunchKernelGGL(k_group_zero, dim3((uint32_t)((m + 256u) / 256u)), dim3(256), 0, stream, count, m + 1u,
                       (uint32_t *)nullptr, (uint64_t)0);
  for (uint32_t pass = 0; pass < p.passes; ++pass) {
    const bool head = pass == 0, last = pass + 1 == p.passes;
    const GroupArgs a = {ep, head ? nullptr : pair[(pass - 1u) & 1u], last ? nullptr : pair[pass & 1u], order, hist,
                         count, n, (uint32_t)m, pass, p.digit_bits, p.tile, p.blocks};
    void (*const hfn)(GroupArgs) = !head ? k_group_hist<false, false>
                                   : p.passes > 1 ? k_group_hist<true, true> : k_group_hist<true, false>;
    void (*const sfn[2][2])(GroupArgs) = {{k_group_scatter<false, false>, k_group_scatter<false, true>},
                                          {k_group_scatter<true, false>, k_group_scatter<true, true>}};
    const uint64_t cells = ((uint64_t)1 << p.digit_bits) * p.blocks;
    hipLaunchKernelGGL(hfn, dim3(p.blocks), dim3(256), 0, stream, a);
    group_scan<uint32_t, uint32_t>(hist, cells, hist, cells, sums, stream);
    hipLaunchKernelGGL(sfn[head ? 1 : 0][last ? 1 : 0], dim3(p.blocks), dim3(256), 0, stream, a);
  }
  if (p.passes == 1)
    hipLaunchKernelGGL(k_group_first, dim3((uint32_t)((m + 2u + 255u) / 256u)), dim3(256), 0, stream,
                       (const uint32_t *)hist, p.blocks, n, (uint32_t)m, first);
  else
    group_scan<uint32_t, uint64_t>(count, m + 1u, first, m + 2u, sums, stream);
  if (views) {
    hipLaunchKernelGGL(k_group_views, dim3(p.lane_blocks), dim3(256), 0, stream, (const uint32_t *)order,
                       (const uint8_t *)views, (const uint64_t *)first, n, (uint32_t)m, (uint8_t *)q_views, q_offsets);
    group_scan<uint64_t, uint64_t>(q_offsets, n, q_offsets, n + 1u, sums, stream);
  }
  return hip_status(hipGetLastError());
}

// yu_rx_reply: its arguments, then k_reply on yu::plan_reply's grid, which leaves
// T[i] in r_offsets[i], and the scan of yu_rx_group over n + 1 outputs in place,
// its tile sums in the caller's workspace. At n == 0 the one offset is stored.
int rx_reply(const yu_tx_record *recs, const uint16_t *flags, uint16_t need, const yu_iovec *views,
             const uint32_t *ep, uint64_t m, const uint8_t *ep_echo, uint32_t what, uint64_t n, yu_tx_record *r_recs,
             uint64_t *r_offsets, void *work, uint64_t work_bytes, void *stream_) {
  if (!aligned(recs, 8) || !aligned(views, 8) || !aligned(r_recs, 8) || !aligned(r_offsets, 8) ||
      !aligned(work, 16))
    return YU_EINVAL;                                            // EINVAL:offsets
  if (!aligned(flags, 2) || !aligned(ep, 4)) return YU_EINVAL;   // EINVAL:side-align
  if (m > yu::kDemuxMax || (what & ~yu::kReplyKnown)) return YU_EINVAL;  // EINVAL:data
  if (!r_offsets) return YU_EINVAL;                              // EINVAL:out
  hipStream_t stream = (hipStream_t)stream_;
  int dev = 0;
  if (n == 0) {  // the empty batch of replies is stored, as yu_rx_group stores its empty CSR
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_status(e);
    hipLaunchKernelGGL(k_group_zero, dim3(1), dim3(256), 0, stream, (uint32_t *)r_offsets, (uint64_t)2,
                       (uint32_t *)nullptr, (uint64_t)0);
    return hip_status(hipGetLastError());
  }
  if (!r_recs) return YU_EINVAL;                                 // EINVAL:out
  if (!recs || !views || !work || work_bytes < yu::reply_workspace_bytes(n)) return YU_EINVAL;  // EINVAL:data
  if (!ep && (what & yu::kReplyUdpEcho)) return YU_EINVAL;       // EINVAL:data
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_status(e);
  const yu::ReplyPlan p = yu::plan_reply(n, cu_count(dev), yu::env_knobs());
  const ReplyArgs a = {(const uint8_t *)recs, flags, (const uint8_t *)views, ep, ep_echo, (uint8_t *)r_recs,
                       r_offsets, n, (uint32_t)m, need, what};
  void (*const fn[2][2])(ReplyArgs) = {{k_reply<false, 0>, k_reply<false, 1>}, {k_reply<true, 0>, k_reply<true, 1>}};
  hipLaunchKernelGGL(fn[flags ? 1 : 0][p.policy], dim3(p.blocks), dim3(256), 0, stream, a);
  group_scan<uint64_t, uint64_t>(r_offsets, n, r_offsets, n + 1u, (uint64_t *)work, stream);
  return hip_status(hipGetLastError());
}

// yu_rx_stream: its arguments, then k_stream on yu::stream_blocks' grid, which
// leaves every slot's length in s_offsets[slot] and 40 or 0 in a_offsets[e], and
// the scan of yu_rx_group over both in place, one after the other, their tile
// sums in the caller's workspace. At n == 0 every output is zero and is stored so.
const char *stream_name(uint64_t n, uint64_t m, uint32_t cap) {
  if (yu::stream_workspace_bytes(n, m, cap) == 0u) return "none";
  return yu::env_knobs().stream_walk ? "k_stream<walk>" : "k_stream";
}

void stream_zero(void *p, uint64_t dwords, hipStream_t stream) {
  if (!p || !dwords) return;
  const uint64_t blocks = (dwords + 255u) / 256u;
  hipLaunchKernelGGL(k_group_zero, dim3((uint32_t)(blocks < 65536u ? blocks : 65536u)), dim3(256), 0, stream,
                     (uint32_t *)p, dwords, (uint32_t *)nullptr, (uint64_t)0);
}

int rx_stream(const yu_tx_record *recs, const yu_iovec *views, uint64_t n, const uint32_t *order,
              const uint64_t *first, uint64_t m, const yu_endpoint_id *ids, yu_tcp_rcv *st, yu_tcp_seg *heap,
              uint32_t cap, uint8_t *status, yu_iovec *s_views, uint64_t *s_offsets, yu_tx_record *a_recs,
              uint64_t *a_offsets, uint32_t *n_acks, void *work, uint64_t work_bytes, void *stream_) {
  if (!aligned(recs, 8) || !aligned(views, 8) || !aligned(first, 8) || !aligned(st, 8) || !aligned(heap, 8) ||
      !aligned(s_views, 8) || !aligned(s_offsets, 8) || !aligned(a_recs, 8) || !aligned(a_offsets, 8) ||
      !aligned(work, 16))
    return YU_EINVAL;                                                        // EINVAL:offsets
  if (!aligned(order, 4) || !aligned(ids, 4) || !aligned(n_acks, 4)) return YU_EINVAL;  // EINVAL:side-align
  if (m > yu::kDemuxMax || n >= (1ull << 32) || cap > yu::kStreamMaxCap) return YU_EINVAL;  // EINVAL:data
  if (m > 0 && !st) return YU_EINVAL;                                        // EINVAL:data
  if ((a_recs != nullptr) != (a_offsets != nullptr) || (a_recs != nullptr) != (n_acks != nullptr))
    return YU_EINVAL;                                                        // EINVAL:data
  const uint64_t N = n + m * cap;
  if (!s_offsets && (m > 0 || n > 0)) return YU_EINVAL;                      // EINVAL:out
  if (!s_views && N > 0) return YU_EINVAL;                                   // EINVAL:out
  hipStream_t stream = (hipStream_t)stream_;
  int dev = 0;
  if (n == 0) {  // the empty tables are stored; no state, no heap entry and no input is touched
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_status(e);
    stream_zero(s_views, 4u * N, stream);
    stream_zero(s_offsets, 2u * (N + 1u), stream);
    stream_zero(a_recs, 8u * m, stream);
    stream_zero(a_offsets, 2u * (m + 1u), stream);
    stream_zero(n_acks, m, stream);
    return hip_status(hipGetLastError());
  }
  if (!status) return YU_EINVAL;                                             // EINVAL:out
  if (!recs || !views || !order || !first || !work || work_bytes < yu::stream_workspace_bytes(n, m, cap))
    return YU_EINVAL;                                                        // EINVAL:data
  if ((!heap && m * cap > 0) || (!ids && a_recs && m > 0)) return YU_EINVAL;  // EINVAL:data
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_status(e);
  const yu::Knobs &k = yu::env_knobs();
  const StreamArgs a = {(const uint8_t *)recs, (const uint8_t *)views, order, first, (uint8_t *)st,
                        (uint8_t *)heap, status, (uint8_t *)s_views, s_offsets, n_acks,
                        (uint32_t)n, (uint32_t)m, cap};
  const uint32_t cus = (uint32_t)cu_count(dev);
  if (m)
    hipLaunchKernelGGL(k.stream_walk ? k_stream<false> : k_stream<true>,
                       dim3(yu::stream_blocks(0u, m, cus, k.blocks_per_cu)), dim3(256), 0, stream, a);
  const StreamFinArgs f = {order, first, (const uint32_t *)ids, (const uint32_t *)st, n_acks, (uint8_t *)a_recs,
                           a_offsets, status, (uint8_t *)s_views, s_offsets, (uint32_t)n, (uint32_t)m, cap};
  hipLaunchKernelGGL(k_stream_fin, dim3(yu::stream_blocks(n, (m + 63u) / 64u, cus, k.blocks_per_cu)), dim3(256), 0,
                     stream, f);
  group_scan<uint64_t, uint64_t>(s_offsets, N, s_offsets, N + 1u, (uint64_t *)work, stream);
  if (a_recs) group_scan<uint64_t, uint64_t>(a_offsets, m, a_offsets, m + 1u, (uint64_t *)work, stream);
  return hip_status(hipGetLastError());
}

// Completion signal for the host path's direct mode (yucsum_internal.h):
// stored after the work before it on the stream, with system-scope release,
// into coherent pinned host memory.
__global__ void k_signal(volatile uint32_t *flag, uint32_t value) {
  __threadfence_system();
  *flag = value;
  __threadfence_system();
}

}  // namespace

int yu_internal_signal(uint32_t *flag, uint32_t value, void *stream) {
  hipLaunchKernelGGL(k_signal, dim3(1), dim3(1), 0, (hipStream_t)stream, flag, value);
  return hip_status(hipGetLastError());
}

extern "C" {

int yu_csum_batch_uniform(const uint8_t *data, uint64_t stride, uint32_t len,
                          uint64_t n, int mode, const uint16_t *initial_arr,
                          uint16_t initial, const uint8_t *addrs,
                          uint16_t *out, void *stream) {
  return batch_uniform(data, nullptr, stride, len, n, mode, initial_arr,
                       initial, addrs, out, stream);
}

int yu_csum_batch_ragged(const uint8_t *data, const uint64_t *offsets,
                         uint64_t n, int mode, const uint16_t *initial_arr,
                         uint16_t initial, const uint8_t *addrs,
                         uint16_t *out, void *stream) {
  return batch_ragged(data, nullptr, offsets, n, mode, initial_arr, initial,
                      addrs, out, stream);
}

int yu_csum_fill_uniform(uint8_t *data, uint64_t stride, uint32_t len,
                         uint64_t n, int mode, const uint16_t *initial_arr,
                         uint16_t initial, const uint8_t *addrs, uint16_t *out,
                         void *stream) {
  if (n > 1 && stride < len) return YU_EINVAL;  // EINVAL:fill-overlap (overlapping packets)
  return batch_uniform(data, data, stride, len, n, mode, initial_arr, initial,
                       addrs, out, stream);
}

int yu_csum_fill_ragged(uint8_t *data, const uint64_t *offsets, uint64_t n,
                        int mode, const uint16_t *initial_arr,
                        uint16_t initial, const uint8_t *addrs, uint16_t *out,
                        void *stream) {
  // Any alignment (include/yucsum.h): the ragged writers store each field as one
  // 16-bit store (even address) or two byte stores, and the TXW kind's whole-line
  // write-back stores only 128-byte lines that lie inside its own chunk's packets.
  return batch_ragged(data, data, offsets, n, mode, initial_arr, initial,
                      addrs, out, stream);
}

int yu_csum_batch_iov(const yu_iovec *views, const uint64_t *first_iov, uint64_t n, int mode,
                      const uint16_t *initial_arr, uint16_t initial, const uint8_t *addrs,
                      uint16_t *out, void *stream) {
  return call_iov({false, false, views, first_iov, n, mode, initial_arr, initial, addrs, nullptr, nullptr, out,
                   false, stream});
}

int yu_csum_fill_iov(const yu_iovec *views, const uint64_t *first_iov, uint64_t n, int mode,
                     const uint16_t *initial_arr, uint16_t initial, const uint8_t *addrs,
                     uint16_t *out, void *stream) {
  return call_iov({false, false, views, first_iov, n, mode, initial_arr, initial, addrs, nullptr, nullptr, out,
                   true, stream});
}

const char *yu_iov_variant_n(int mode, uint64_t n, int fill) {
  return iov_variant(false, false, mode, n, fill);
}

int yu_csum_batch_iov_datagram(const yu_iovec *views, const uint64_t *first_iov, uint64_t n, int mode,
                               uint16_t *out, void *stream) {
  return call_iov({true, false, views, first_iov, n, mode, nullptr, 0, nullptr, nullptr, nullptr, out, false,
                   stream});
}

int yu_csum_fill_iov_datagram(const yu_iovec *views, const uint64_t *first_iov, uint64_t n, int mode,
                              uint16_t *out, void *stream) {
  return call_iov({true, false, views, first_iov, n, mode, nullptr, 0, nullptr, nullptr, nullptr, out, true,
                   stream});
}

const char *yu_iov_datagram_variant_n(int mode, uint64_t n, int fill) {
  return iov_variant(true, false, mode, n, fill);
}

int yu_csum_pack_iov(const yu_iovec *views, const uint64_t *first_iov, uint64_t n, int mode,
                     const uint16_t *initial_arr, uint16_t initial, const uint8_t *addrs, uint8_t *dst,
                     const uint64_t *dst_offsets, uint16_t *out, void *stream) {
  return call_iov({false, true, views, first_iov, n, mode, initial_arr, initial, addrs, dst, dst_offsets, out,
                   false, stream});
}

int yu_csum_pack_fill_iov(const yu_iovec *views, const uint64_t *first_iov, uint64_t n, int mode,
                          const uint16_t *initial_arr, uint16_t initial, const uint8_t *addrs, uint8_t *dst,
                          const uint64_t *dst_offsets, uint16_t *out, void *stream) {
  return call_iov({false, true, views, first_iov, n, mode, initial_arr, initial, addrs, dst, dst_offsets, out,
                   true, stream});
}

const char *yu_iov_pack_variant_n(int mode, uint64_t n, int fill) {
  return iov_variant(false, true, mode, n, fill);
}

int yu_csum_pack_iov_datagram(const yu_iovec *views, const uint64_t *first_iov, uint64_t n, int mode,
                              uint8_t *dst, const uint64_t *dst_offsets, uint16_t *out, void *stream) {
  return call_iov({true, true, views, first_iov, n, mode, nullptr, 0, nullptr, dst, dst_offsets, out, false,
                   stream});
}

int yu_csum_pack_fill_iov_datagram(const yu_iovec *views, const uint64_t *first_iov, uint64_t n, int mode,
                                   uint8_t *dst, const uint64_t *dst_offsets, uint16_t *out, void *stream) {
  return call_iov({true, true, views, first_iov, n, mode, nullptr, 0, nullptr, dst, dst_offsets, out, true,
                   stream});
}

const char *yu_iov_pack_datagram_variant_n(int mode, uint64_t n, int fill) {
  return iov_variant(true, true, mode, n, fill);
}

int yu_tx_build_ragged(const uint8_t *payload, const uint64_t *pay_offsets, const yu_tx_record *recs, uint64_t n,
                       uint8_t *dst, const uint64_t *dst_offsets, uint16_t *out, void *stream) {
  return tx_build(payload, pay_offsets, recs, n, dst, dst_offsets, out, stream);
}

const char *yu_tx_build_variant_n(uint64_t n) {
  return yu::plan_wave(yu::WaveFamily::Build, n, 0, false, 256, yu::env_knobs()).name;
}

int yu_tx_build_iov(const yu_iovec *views, const yu_tx_record *recs, uint64_t n, uint8_t *dst,
                    const uint64_t *dst_offsets, uint16_t *out, void *stream) {
  return tx_build_iov(views, recs, n, dst, dst_offsets, out, stream);
}

const char *yu_tx_build_iov_variant_n(uint64_t) { return kBuildIovName; }

int yu_rx_split_ragged(const uint8_t *data, const uint64_t *offsets, uint64_t n, uint8_t *pay,
                       const uint64_t *pay_offsets, yu_tx_record *recs, uint32_t *pay_len, uint16_t *out,
                       void *stream) {
  return rx_split(data, offsets, n, pay, pay_offsets, recs, pay_len, out, stream);
}

const char *yu_rx_split_variant_n(uint64_t n) {
  return yu::plan_wave(yu::WaveFamily::Split, n, 0, false, 256, yu::env_knobs()).name;
}

int yu_rx_parse_ragged(const uint8_t *data, const uint64_t *offsets, uint64_t n, int verify, yu_tx_record *recs,
                       yu_iovec *pay_views, uint16_t *out, void *stream) {
  return rx_parse(data, offsets, n, verify, recs, pay_views, out, stream);
}

const char *yu_rx_parse_variant_n(uint64_t n) {
  return yu::plan_parse(n, 256, yu::env_knobs()).name;
}

uint64_t yu_demux_table_bytes(uint64_t m) { return yu::demux_table_bytes(m); }

uint32_t yu_demux_hash(const yu_endpoint_id *id) { return yu::demux_hash(yu::demux_id_key(*id)); }

int yu_demux_table_fill(const yu_endpoint_id *ids, uint64_t m, void *h_table, uint64_t table_bytes, uint64_t *bad) {
  return demux_table_fill(ids, m, h_table, table_bytes, bad);
}

int yu_rx_demux(const yu_tx_record *recs, const uint16_t *flags, uint16_t need, uint64_t n, const void *table,
                uint64_t table_bytes, uint64_t m, uint32_t *ep, uint32_t *ep_count, void *stream) {
  return rx_demux(recs, flags, need, n, table, table_bytes, m, ep, ep_count, stream);
}

const char *yu_rx_demux_variant_n(uint64_t n) {
  return yu::plan_demux(n, 256, yu::env_knobs()).name;
}

uint64_t yu_rx_group_workspace_bytes(uint64_t n, uint64_t m) { return yu::plan_group(n, m, 256, yu::Knobs()).bytes; }

int yu_rx_group(const uint32_t *ep, uint64_t n, uint64_t m, const yu_iovec *views, uint32_t *order, uint64_t *first,
                yu_iovec *q_views, uint64_t *q_offsets, void *work, uint64_t work_bytes, void *stream) {
  return rx_group(ep, n, m, views, order, first, q_views, q_offsets, work, work_bytes, stream);
}

const char *yu_rx_group_variant_n(uint64_t n, uint64_t m) {
  return yu::plan_group(n, m, 256, yu::env_knobs()).name;
}

uint64_t yu_rx_reply_workspace_bytes(uint64_t n) { return yu::reply_workspace_bytes(n); }

int yu_rx_reply(const yu_tx_record *recs, const uint16_t *flags, uint16_t need, const yu_iovec *views,
                const uint32_t *ep, uint64_t m, const uint8_t *ep_echo, uint32_t what, uint64_t n,
                yu_tx_record *r_recs, uint64_t *r_offsets, void *work, uint64_t work_bytes, void *stream) {
  return rx_reply(recs, flags, need, views, ep, m, ep_echo, what, n, r_recs, r_offsets, work, work_bytes, stream);
}

const char *yu_rx_reply_variant_n(uint64_t n) {
  return yu::plan_reply(n, 256, yu::env_knobs()).name;
}

uint64_t yu_rx_stream_workspace_bytes(uint64_t n, uint64_t m, uint32_t cap) {
  return yu::stream_workspace_bytes(n, m, cap);
}

int yu_rx_stream(const yu_tx_record *recs, const yu_iovec *views, uint64_t n, const uint32_t *order,
                 const uint64_t *first, uint64_t m, const yu_endpoint_id *ids, yu_tcp_rcv *st, yu_tcp_seg *heap,
                 uint32_t cap, uint8_t *status, yu_iovec *s_views, uint64_t *s_offsets, yu_tx_record *a_recs,
                 uint64_t *a_offsets, uint32_t *n_acks, void *work, uint64_t work_bytes, void *stream) {
  return rx_stream(recs, views, n, order, first, m, ids, st, heap, cap, status, s_views, s_offsets, a_recs,
                   a_offsets, n_acks, work, work_bytes, stream);
}

const char *yu_rx_stream_variant_n(uint64_t n, uint64_t m, uint32_t cap) { return stream_name(n, m, cap); }

const char *yu_uniform_variant(uint64_t stride, uint32_t len, int mode,
                               uint64_t data_align16) {
  return variant_name({false, data_align16 & 15u, stride, len, 2, mode, false});
}

const char *yu_uniform_variant_n(uint64_t stride, uint32_t len, uint64_t n, int mode,
                                 uint64_t data_align16) {
  if (mode < 0 || mode >= YU_MODE_COUNT) return "";
  return variant_name({false, data_align16 & 15u, stride, len, n, mode, false});
}

const char *yu_ragged_variant(int mode) {
  if (mode < 0 || mode >= YU_MODE_COUNT) return "";
  return variant_name({true, 0, 0, 0, 1u << 20, mode, false});
}

const char *yu_ragged_variant_n(int mode, uint64_t n) {
  if (mode < 0 || mode >= YU_MODE_COUNT) return "";
  return variant_name({true, 0, 0, 0, n, mode, false});
}

const char *yu_ragged_fill_variant_n(int mode, uint64_t n) {
  if (mode < 0 || mode >= YU_MODE_COUNT) return "";
  return variant_name({true, 0, 0, 0, n, mode, true});
}

int yu_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c < 0 ? 0 : c;
}

}  // extern "C"
