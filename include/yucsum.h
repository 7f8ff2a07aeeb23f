/*
 * yucsum.h — C ABI of the MI355X-native Internet-checksum engine.
 *
 * This is the drop-in boundary for yustack's `checksum` package
 * (reference: /root/reference/checksum/checksum.go). The reference exposes
 * three package-level Go functions and nothing else; every caller
 * (header/ipv4.go:177-179, header/tcp.go:165-173, header/udp.go:67-75,
 * types/route.go:90-92, transport/udp/endpoint.go:175,
 * transport/tcp/connect.go:314,580, network/ipv4/icmp.go:42,
 * checker/checker.go:32,84-88) reaches the hot path through them.
 *
 * Two groups of entry points:
 *
 *  1. Scalar, Go-signature entry points (yu_checksum, yu_checksum_combine,
 *     yu_pseudo_header_checksum). These are what a cgo shim binds so that the
 *     reference's callers compile unchanged. They run on the
 *     calling host thread: a cgo call costs ~100 ns, a GPU round trip costs
 *     microseconds, so per-call offload would be a pessimisation. They are
 *     total functions (never fail), reentrant and allocation-free.
 *
 *  2. Batched device entry points (yu_csum_batch_uniform,
 *     yu_csum_batch_ragged, yu_csum_batch_iov and the yu_csum_fill_* forms).
 *     These are the GPU hot path: one launch computes the per-packet sums of a whole device-resident batch with hand-written
 *     gfx950 HIP kernels. They are asynchronous on the given HIP stream,
 *     perform no allocation and no synchronisation (graph-capturable), and
 *     return a status code. There is no CPU fallback: without a usable GPU
 *     they return a negative status.
 *
 *  3. Batched host entry points (yu_csum_batch_host_uniform / _ragged / _iov,
 *     and their _multi forms over several GPUs): the path that starts and
 *     ends in host memory (tun / link-layer buffers). Batches up to 4 MiB are
 *     read and answered in place over PCIe by the kernel (one launch, one
 *     synchronisation); larger ones are staged through library-owned pinned
 *     buffers with H2D copy, kernel and D2H copy overlapped on separate
 *     streams. Synchronous.
 *
 * All arithmetic is unsigned integer. Results are bit-identical to the
 * reference Go code on the same bytes, including the reference's uint32
 * wrap-around for buffers longer than 131072 bytes (RAW mode).
 */
#ifndef YUCSUM_H
#define YUCSUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YUCSUM_ABI_VERSION 1

/* ------------------------------------------------------------------ */
/* Status codes (batched entry points).                               */
/* ------------------------------------------------------------------ */
#define YU_OK 0
#define YU_EINVAL (-22)         /* bad argument (mode, NULL pointer, len) */
#define YU_ENODEV (-19)         /* no HIP device / device index out of range */
#define YU_ENOMEM (-12)         /* pinned/device staging allocation failed */
#define YU_EHIP_BASE (-1000)    /* -(1000 + hipError_t) for any other HIP error */

/* ------------------------------------------------------------------ */
/* Preconditions: every YU_EINVAL the batched calls return.            */
/* Each `return YU_EINVAL` in the library is tagged with one of these   */
/* names, and tests/test_abi.py checks that the tags and this list      */
/* agree. All are checked before any device work; a call that returns  */
/* YU_EINVAL has read no packet byte and written nothing.               */
/*                                                                      */
/*  [mode]          mode is not 0 .. YU_MODE_COUNT-1 (every call); the   */
/*                  scatter-gather device calls (yu_csum_*_iov, the      */
/*                  packing yu_csum_pack_*_iov included): also           */
/*                  IPV4, VERIFY_IPV4, VERIFY_RX and TX_DATAGRAM, which  */
/*                  parse headers out of the packet; the whole-datagram  */
/*                  calls (yu_csum_*_iov_datagram) take those four and   */
/*                  refuse every other mode.                             */
/*  [out]           out == NULL in a yu_csum_batch_* call, in            */
/*                  yu_rx_split_ragged or in yu_rx_parse_ragged, ep == NULL */
/*                  in yu_rx_demux, order == NULL in yu_rx_group, or h_out == */
/*                  NULL in a yu_csum_batch_host_* call, with n > 0 (the */
/*                  fill calls take NULL: no result array; an empty     */
/*                  batch, n == 0, is a no-op returning YU_OK);          */
/*                  yu_rx_group: first == NULL, with any n.              */
/*  [fill-mode]     a fill call (yu_csum_fill_*) with a mode that has no */
/*                  field to write: RAW, VERIFY_* (or no mode at all);   */
/*                  yu_csum_fill_iov and yu_csum_pack_fill_iov: any mode */
/*                  but UDP, TCP and ICMP;                               */
/*                  yu_csum_fill_iov_datagram: VERIFY_IPV4, VERIFY_RX.   */
/*  [side-align]    device calls: initial_arr not 2-byte aligned, addrs  */
/*                  not 4-byte aligned, out not 2-byte aligned           */
/*                  (yu_tx_build_ragged: out; yu_rx_split_ragged: out,   */
/*                  and pay_len not 4-byte aligned; yu_rx_parse_ragged:  */
/*                  out; yu_rx_demux: flags not 2-byte aligned, ep or    */
/*                  ep_count not 4-byte aligned; yu_rx_group: ep or      */
/*                  order not 4-byte aligned).                           */
/*  [data]          data == NULL with n > 0 (device calls), h_data ==    */
/*                  NULL while the packets hold bytes (host calls), iov  */
/*                  == NULL while first_iov names views; views == NULL  */
/*                  with n > 0 (yu_csum_*_iov); dst == NULL with n > 0   */
/*                  (yu_csum_pack_*_iov); payload, recs or dst == NULL   */
/*                  with n > 0 (yu_tx_build_ragged); data, pay, recs or  */
/*                  pay_len == NULL with n > 0 (yu_rx_split_ragged);     */
/*                  data, recs or pay_views == NULL with n > 0           */
/*                  (yu_rx_parse_ragged); recs or table == NULL with     */
/*                  n > 0, table_bytes != yu_demux_table_bytes(m) or m > */
/*                  YU_DEMUX_MAX_ENDPOINTS (yu_rx_demux); the same two,  */
/*                  ids or h_table == NULL with m > 0, a malformed id or */
/*                  one equal to an earlier id (yu_demux_table_fill);    */
/*                  yu_rx_group: m > YU_DEMUX_MAX_ENDPOINTS or n >= 2^32, */
/*                  and with n > 0: ep or work == NULL, work_bytes below */
/*                  yu_rx_group_workspace_bytes(n, m), or some but not   */
/*                  all of views, q_views and q_offsets given.           */
/*                  yu_rx_stream uses [data], [out], [offsets] and       */
/*                  [side-align] as the comment above it lists them.     */
/*  [len-transport] a packet of a mode other than RAW longer than        */
/*                  YU_MAX_TRANSPORT_LEN (uniform len; every host ragged */
/*                  or iov packet). Device ragged batches are not read   */
/*                  back on the host: see "Out of contract" below.       */
/*  [len-raw]       a RAW packet longer than YU_MAX_RAW_LEN (the same).  */
/*  [len-min]       uniform len below the mode's fixed header: UDP 8,    */
/*                  TCP 20, ICMP 4, IPV4 / VERIFY_IPV4 1 (the IHL byte). */
/*  [span]          uniform: data + (n-1)*stride + len wraps the address */
/*                  space.                                               */
/*  [offsets]       offsets == NULL, or (device) not 8-byte aligned, or  */
/*                  (host) decreasing; first_iov == NULL or decreasing;  */
/*                  yu_csum_*_iov (device tables): first_iov == NULL or  */
/*                  not 8-byte aligned, views not 8-byte aligned;        */
/*                  yu_csum_pack_*_iov: also dst_offsets == NULL or not  */
/*                  8-byte aligned; yu_tx_build_ragged: pay_offsets or   */
/*                  dst_offsets == NULL or not 8-byte aligned, recs not  */
/*                  8-byte aligned; yu_rx_split_ragged: offsets or       */
/*                  pay_offsets == NULL or not 8-byte aligned, recs not  */
/*                  8-byte aligned; yu_rx_parse_ragged: offsets == NULL  */
/*                  or not 8-byte aligned, recs or pay_views not 8-byte  */
/*                  aligned; yu_rx_demux: recs not 8-byte aligned, table */
/*                  not 16-byte aligned; yu_rx_group: first, q_offsets,  */
/*                  views or q_views not 8-byte aligned, work not        */
/*                  16-byte aligned.                                     */
/*  [iov-view]    a view with base == NULL and len > 0.                */
/*  [fill-align]    yu_csum_fill_uniform: data or stride not a multiple  */
/*                  of 4. The uniform writers store whole dwords of each */
/*                  packet's window, so no dword may hold bytes of two   */
/*                  packets.                                             */
/*  [fill-overlap]  yu_csum_fill_uniform: n > 1 and stride < len.        */
/*  [devices]       *_multi: devices == NULL, ndev < 1 or ndev > 64.     */
/*                  (A listed device that does not exist: YU_ENODEV.)    */
/*                                                                      */
/* Where the writers differ from the reference: Go's SetChecksum         */
/* (header/udp.go:60-62, header/tcp.go:156-158, header/ipv4.go:165-167,  */
/* header/icmpv4.go:46-48) has no alignment precondition, and neither do */
/* yu_csum_fill_ragged (device) and the yu_csum_fill_host_* calls: a     */
/* packed, unaligned tun burst (any data address, any offsets) is        */
/* written in place as it lies. Only the uniform device writer asks for  */
/* [fill-align]; an unaligned uniform batch goes through                 */
/* yu_csum_fill_ragged with offsets[i] = i * stride instead (same values,*/
/* same field stores). In the ragged writer a field at an even address   */
/* is one 16-bit store and one at an odd address two byte stores; from   */
/* 65536 packets on (the TXW kind, yu_ragged_fill_variant_n) the         */
/* 128-byte lines that lie wholly inside one 48-packet chunk's packets   */
/* and hold a field are stored whole from the bytes just read, the field */
/* patched in; a field straddling two lines keeps its byte stores.       */
/* Bytes outside the packets' fields are never changed.                  */
/*                                                                      */
/* Out of contract (device ragged batches only, whose offsets live in    */
/* device memory and are not checked here): a packet whose offsets       */
/* decrease, longer than the mode's limit (YU_MAX_TRANSPORT_LEN; RAW:    */
/* YU_MAX_RAW_LEN), or ending past offsets[n] (a call touches at most    */
/* data[0, offsets[n])). It gets an unspecified result, never a fault or */
/* a hang: every byte a ragged call reads or writes lies in the dwords   */
/* holding data[0, offsets[n]), whatever the other offsets say           */
/* (offsets[n] itself must be right, and data + offsets[i] must not wrap */
/* the address space). A kernel that takes a group of consecutive        */
/* packets at a time (k_seg's chunks                                    */
/* of 16 to 64 packets, k_hdr's steps of 64; yu_ragged_variant_n and    */
/* yu_ragged_fill_variant_n name the kernel) may give the other packets */
/* of the group holding one, [k*c, k*c + c) for group size c,           */
/* unspecified results too. A fill call never writes a byte outside the */
/* checksum fields of in-contract packets: no field of an out-of-       */
/* contract packet is stored, nor any field of its group. Every other   */
/* packet's result and field are exact. Validate first when the offsets */
/* come from outside (the host forms and the Python front end           */
/* batch.checksum_ragged(validate=True) do).                            */

/* ------------------------------------------------------------------ */
/* Scalar entry points (host CPU, Go-signature drop-ins).             */
/* ------------------------------------------------------------------ */

/* Replaces `func Checksum(buf []byte, initial uint16) uint16`
 * (checksum/checksum.go:4-18). Sum of big-endian 16-bit words of buf, odd
 * trailing byte as the high byte of a final word, plus `initial`, in a
 * uint32 accumulator that wraps mod 2^32, folded once by ChecksumCombine.
 * The result is NOT complemented. len==0 (buf may be NULL) returns
 * fold(initial) == initial. */
uint16_t yu_checksum(const uint8_t *buf, size_t len, uint16_t initial);

/* Replaces `func ChecksumCombine(a, b uint16) uint16`
 * (checksum/checksum.go:32-35): one end-around-carry add. */
uint16_t yu_checksum_combine(uint16_t a, uint16_t b);

/* Replaces `func PseudoHeaderChecksum(protocol uint32, srcAddr, dstAddr
 * string) uint16` (checksum/checksum.go:24-28). Go strings become
 * (pointer, length) pairs; the protocol is truncated to uint8 exactly as
 * `uint8(protocol)` does. The transport length is NOT included (callers add
 * it through {UDP,TCP}.CalculateChecksum, header/udp.go:67-75,
 * header/tcp.go:165-173). */
uint16_t yu_pseudo_header_checksum(uint32_t protocol,
                                   const uint8_t *src_addr, size_t src_len,
                                   const uint8_t *dst_addr, size_t dst_len);

/* ------------------------------------------------------------------ */
/* Batched modes. Each names the reference composition it reproduces.  */
/* "pseudo" = the per-packet pseudo-header partial sum: either the 8-byte */
/* {src[4], dst[4]} record from `addrs` (protocol fixed by the mode) or,  */
/* when addrs is NULL, the uint16 PseudoHeaderChecksum value from        */
/* `initial_arr[i]` (or the scalar `initial`).                           */
/* ------------------------------------------------------------------ */

/* out[i] = Checksum(pkt_i, initial_i)  — checksum/checksum.go:4-18.
 * Uncomplemented; exact for any length (uint32 wrap reproduced). */
#define YU_MODE_RAW 0
/* pkt_i = UDP header (8 B) + data. out[i] = the value sendUDP stores:
 * ^UDP.CalculateChecksum(Checksum(data, pseudo), len) with the header's
 * checksum field taken as 0 (Encode writes 0) —
 * transport/udp/endpoint.go:164-187, header/udp.go:67-83. Protocol 17. */
#define YU_MODE_UDP 1
/* pkt_i = TCP segment (header incl. options, then data). out[i] = the value
 * sendTCP stores: ^TCP.CalculateChecksum(Checksum(data, pseudo), len) with
 * the checksum field taken as 0 — transport/tcp/connect.go:556-586,
 * header/tcp.go:165-186. Protocol 6. As in every segment sendTCP encodes,
 * 20 <= DataOffset() <= len is required; other segments get an unspecified
 * value (never a fault). Data = the bytes past DataOffset() * 4. (Only
 * sendTCPWithOptions given options whose length is not a multiple of 4 —
 * no caller does: sendSynTCP passes 4 or 8, connect.go:266-284 — would sum
 * its header to the floored DataOffset() and leave the option bytes past it
 * out of the sum, a value the receiver's check rejects; this mode sums them
 * as data, as the receiver does. Measured by executing the reference,
 * DESIGN.md §2.) */
#define YU_MODE_TCP 2
/* pkt_i = IPv4 datagram. out[i] = ^IPv4.CalculateChecksum() over
 * b[:IHL*4] (clamped to len) with the header-checksum field taken as 0 —
 * network/ipv4/ipv4.go:80-97, header/ipv4.go:146-157,177-179. initial and
 * addrs are ignored. */
#define YU_MODE_IPV4 3
/* pkt_i = ICMPv4 message (4-byte header + data). out[i] =
 * ^Checksum(hdr, Checksum(data, 0)) with the checksum field taken as 0 —
 * network/ipv4/icmp.go:36-45. initial and addrs are ignored. */
#define YU_MODE_ICMP 4
/* Receive-side verification, checker semantics (checker/checker.go:25-40):
 * out[i] = Checksum(b[:IHL*4] clamped to len, 0) INCLUDING the stored field. The packet is
 * valid iff out[i] is 0x0000 or 0xFFFF. */
#define YU_MODE_VERIFY_IPV4 5
/* checker.TCP (checker/checker.go:71-99): out[i] = Checksum over
 * pseudo ‖ BE16(len) ‖ segment INCLUDING the stored field. Valid iff
 * out[i] ∈ {0, 0xFFFF}. Protocol 6. */
#define YU_MODE_VERIFY_TCP 6
/* The same verification for UDP datagrams (protocol 17). The reference
 * never verifies on receive (transport/udp/endpoint.go:191-229); this is
 * the checker.TCP formula applied to UDP. */
#define YU_MODE_VERIFY_UDP 7
/* Receive-side verification of whole IPv4 packets as a tun device delivers
 * them (link/tundev/tundev.go:78-114 -> network/ipv4/ipv4.go:62-77): the
 * composition of checker.IPv4 and checker.TCP's checksum test
 * (checker/checker.go:25-40,71-92), all inputs taken from the packet itself:
 *   valid  = len >= 20 && HeaderLength() <= TotalLength() <= len
 *            (IPv4.IsValid, header/ipv4.go:126-138)
 *   IP ok  = Checksum(b[:HeaderLength()], 0) in {0, 0xFFFF}
 *   L4     = valid && Protocol() in {6 TCP, 17 UDP, 1 ICMP}
 *   L4 ok  = Checksum(Payload(), Checksum(BE16(len(Payload())),
 *            PseudoHeaderChecksum(proto, src, dst))) in {0, 0xFFFF}, with
 *            Payload() = b[HeaderLength():TotalLength()]; ICMP without the
 *            pseudo-header and length (network/ipv4/icmp.go:36-45).
 * out[i] is a bit set of YU_RX_*. No side arrays; not a fill mode. */
#define YU_MODE_VERIFY_RX 8
/* Transmit side of whole IPv4 datagrams as the link endpoint writes them
 * (network/ipv4/ipv4.go:80-97 WritePacket after sendUDP
 * transport/udp/endpoint.go:164-187, sendTCP transport/tcp/connect.go:556-586
 * or sendICMPv4 network/ipv4/icmp.go:36-45; written out by
 * link/tundev/tundev.go:171-196): both checksum fields of a datagram in one
 * pass, all inputs taken from the datagram itself. TWO results per packet:
 *   out[2i]   = the IPv4 header checksum WritePacket stores: YU_MODE_IPV4's
 *               value, ^Checksum(b[:HeaderLength()]) with the field as 0;
 *   out[2i+1] = the transport checksum its sender stores, over the segment
 *               b[HeaderLength():TotalLength()] with the pseudo-header from
 *               the datagram's source, destination and protocol and the
 *               length TotalLength() - HeaderLength(): YU_MODE_UDP (17),
 *               YU_MODE_TCP (6) or YU_MODE_ICMP (1) on that segment, field as
 *               0; 0 when the protocol is another one or the segment is
 *               shorter than its header (8 / 20 / 4 bytes).
 * Datagrams must satisfy 20 <= HeaderLength() <= TotalLength() <= len (every
 * datagram WritePacket encodes: IHL 5); others get {0, 0} and, in place,
 * no write. TCP segments need 20 <= DataOffset() <= their length (as
 * YU_MODE_TCP). With fill, each field whose value is defined is stored
 * big-endian in place. No side arrays (initial / addrs are ignored). */
#define YU_MODE_TX_DATAGRAM 9
#define YU_MODE_COUNT 10

/* Results per packet in `out`: 2 for YU_MODE_TX_DATAGRAM, 1 otherwise. Every
 * out / h_out array below holds n * YU_MODE_OUTPUTS(mode) uint16 values. */
#define YU_MODE_OUTPUTS(mode) ((mode) == YU_MODE_TX_DATAGRAM ? 2 : 1)

#define YU_RX_IP_OK 1u   /* header checksum verifies */
#define YU_RX_L4 2u      /* transport (TCP/UDP/ICMP) present and checked */
#define YU_RX_L4_OK 4u   /* transport checksum verifies */
#define YU_RX_INVALID 8u /* IPv4.IsValid fails (nothing else is set) */
#define YU_RX_SPLIT 16u  /* yu_rx_split_ragged, yu_rx_parse_ragged: record and payload (pay_len, or the view) of this packet are defined */

/* Packets handed to the transport/IPv4/ICMP modes must be <= 65535 bytes
 * (the IPv4 total-length limit; the reference's uint16 length arithmetic is
 * only defined there). RAW packets may be up to YU_MAX_RAW_LEN bytes
 * (4 GiB - 64 KiB; the reference's uint32 wrap is reproduced throughout).
 * The uniform calls reject longer packets with YU_EINVAL; a ragged batch
 * is not read back on the host, so a longer ragged packet gets an
 * unspecified value (never a fault or a hang). */
#define YU_MAX_TRANSPORT_LEN 65535u
#define YU_MAX_RAW_LEN 0xFFFF0000u

/* ------------------------------------------------------------------ */
/* Batched device entry points (the GPU hot path).                     */
/* All pointers are device pointers (hipMalloc / torch CUDA tensors).   */
/* `stream` is a hipStream_t (NULL = legacy default stream).            */
/* Asynchronous: returns after enqueueing the kernel.                   */
/* ------------------------------------------------------------------ */

/* Uniform-stride batch: packet i occupies data[i*stride, i*stride + len).
 * Packets may overlap (stride < len) — they are only read.
 *  initial_arr: NULL or n uint16 (per-packet initial / pseudo partial)
 *  initial:     used when initial_arr == NULL
 *  addrs:       NULL or n*8 bytes {src[4], dst[4]} (UDP/TCP/VERIFY_TCP/UDP)
 *  out:         n * YU_MODE_OUTPUTS(mode) uint16 results, written in host
 *               byte order as numbers (store one big-endian into the packet
 *               to set its field). */
int yu_csum_batch_uniform(const uint8_t *data, uint64_t stride, uint32_t len,
                          uint64_t n, int mode,
                          const uint16_t *initial_arr, uint16_t initial,
                          const uint8_t *addrs, uint16_t *out, void *stream);

/* Ragged batch (tun-style back-to-back packets, any byte alignment):
 * packet i occupies data[offsets[i], offsets[i+1]); offsets is a device
 * array of n+1 non-decreasing uint64 (the layout of buffer.VectorisedView
 * flattened, buffer/view.go:37-46). */
int yu_csum_batch_ragged(const uint8_t *data, const uint64_t *offsets,
                         uint64_t n, int mode,
                         const uint16_t *initial_arr, uint16_t initial,
                         const uint8_t *addrs, uint16_t *out, void *stream);

/* In-place field writer (TX modes UDP/TCP/IPV4/ICMP/TX_DATAGRAM only):
 * computes the same value as the matching batch call and stores it
 * big-endian into the packet's checksum field (UDP.SetChecksum
 * header/udp.go:60-62, TCP.SetChecksum header/tcp.go:156-158,
 * IPv4.SetChecksum header/ipv4.go:165-167, ICMPv4.SetChecksum
 * header/icmpv4.go:46-48; both fields of a datagram in TX_DATAGRAM).
 * `out` may be NULL. `data` is written: the fields only (see Preconditions
 * above: [fill-mode]; the uniform form also [fill-align], [fill-overlap];
 * the ragged form takes any alignment). */
int yu_csum_fill_uniform(uint8_t *data, uint64_t stride, uint32_t len,
                         uint64_t n, int mode,
                         const uint16_t *initial_arr, uint16_t initial,
                         const uint8_t *addrs, uint16_t *out, void *stream);
int yu_csum_fill_ragged(uint8_t *data, const uint64_t *offsets, uint64_t n,
                        int mode, const uint16_t *initial_arr,
                        uint16_t initial, const uint8_t *addrs, uint16_t *out,
                        void *stream);

/* ------------------------------------------------------------------ */
/* Batched host entry point (host memory in, host memory out).         */
/* ------------------------------------------------------------------ */

/* Same contract as yu_csum_batch_uniform but every pointer is a HOST
 * pointer (pageable or pinned). The batch is cut into slices that are
 * staged through library-owned pinned buffers on `device` and pipelined
 * (H2D of slice k+1 overlaps the kernel of slice k and the D2H of slice
 * k-1). Synchronous: returns when h_out is complete. Thread-safe: each call
 * borrows one staging context of `device` from a bounded pool and returns it
 * (see yu_host_staging_bytes below). */
int yu_csum_batch_host_uniform(const uint8_t *h_data, uint64_t stride,
                               uint32_t len, uint64_t n, int mode,
                               const uint16_t *h_initial_arr,
                               uint16_t initial, const uint8_t *h_addrs,
                               uint16_t *h_out, int device);

/* The same for a ragged host batch: packet i = h_data[h_offsets[i],
 * h_offsets[i+1]) (a tun read burst packed back to back). The offsets are
 * host memory and are validated here (non-decreasing, packet lengths within
 * the mode's limit), then shipped rebased with each slice. */
int yu_csum_batch_host_ragged(const uint8_t *h_data, const uint64_t *h_offsets,
                              uint64_t n, int mode,
                              const uint16_t *h_initial_arr, uint16_t initial,
                              const uint8_t *h_addrs, uint16_t *h_out,
                              int device);

/* Scatter-gather packets, as the tun endpoint reads them into several views
 * (link/tundev/tundev.go:116-125; buffer.VectorisedView, buffer/view.go:
 * 37-46): packet i is the concatenation of iov[first_iov[i]] ..
 * iov[first_iov[i+1] - 1]. The views are gathered into the library's pinned
 * staging while earlier slices are on the GPU. Layout-compatible with
 * struct iovec. */
typedef struct yu_iovec {
  const void *base;
  uint64_t len;
} yu_iovec;

int yu_csum_batch_host_iov(const yu_iovec *iov, const uint64_t *first_iov,
                           uint64_t n, int mode, const uint16_t *h_initial_arr,
                           uint16_t initial, const uint8_t *h_addrs,
                           uint16_t *h_out, int device);

/* ------------------------------------------------------------------ */
/* Scatter-gather packets on the device.                               */
/* ------------------------------------------------------------------ */

/* The reference never holds an outgoing packet as one buffer: sendUDP
 * (transport/udp/endpoint.go:164-187), sendTCP (transport/tcp/connect.go:
 * 556-586) and sendICMPv4 (network/ipv4/icmp.go:36-45) build the transport
 * header in a buffer.Prependable, leave the payload in its own buffer.View and
 * sum the two separately; received packets are a VectorisedView of up to four
 * views (link/tundev/tundev.go:116-125). These calls take that layout where it
 * lies in device memory, without a packed copy: packet i is the concatenation
 * of views[first_iov[i]] .. views[first_iov[i+1] - 1], the CSR layout and the
 * yu_iovec of the host form above.
 *
 * `views`, `first_iov` (n + 1 entries), every `base`, the side arrays and `out`
 * are DEVICE pointers. Like the other device calls: asynchronous on `stream`,
 * no allocation, no synchronisation, graph-capturable, YU_ENODEV without a
 * device; n == 0 is a no-op returning YU_OK.
 *
 * Value: out[i] is exactly what yu_csum_batch_ragged returns for the same
 * bytes laid back to back, with the same side arguments.
 *
 * Modes: the whole-packet sums RAW, UDP, TCP, ICMP, VERIFY_TCP, VERIFY_UDP.
 * The TX modes take the checksum field as 0 wherever its two bytes lie, in two
 * different views included. IPV4, VERIFY_IPV4, VERIFY_RX and TX_DATAGRAM parse
 * headers out of the packet and are refused here with YU_EINVAL ([mode]):
 * yu_csum_batch_iov_datagram / yu_csum_fill_iov_datagram below take them. The
 * fill form takes UDP, TCP and ICMP ([fill-mode]).
 *
 * Views: any base address, any length (odd ones included), any number per
 * packet (0 included), in any address order, in any number of allocations. A
 * view with len == 0 may have any base, NULL included, and is skipped. The
 * read-only call may name the same view in many packets (a shared header
 * template, a shared payload). In a fill call the bytes that hold a field must
 * belong to one packet only; otherwise those field bytes, and nothing else,
 * are unspecified.
 *
 * Length: a packet's views total at most YU_MAX_TRANSPORT_LEN bytes in every
 * mode of this form, RAW included.
 *
 * Out of contract (the tables are device memory and are not read on the host;
 * compare "Out of contract" above): a packet whose views total more than the
 * limit, or at which first_iov decreases. It gets an unspecified value and no
 * field store, never a fault or a hang: the kernel stops adding view bytes at
 * the limit. Every other packet's value and field are exact. A call reads only
 * the dwords that hold the bytes of the views it names and writes, besides
 * out, only the two field bytes of in-contract packets: as one 16-bit store when both lie in one
 * view at an even address, as two byte stores otherwise. Pointers are trusted,
 * as `data` is in the other device calls.
 *
 * YU_EINVAL (Preconditions above): [mode], [out], [fill-mode], [side-align];
 * [data]: views == NULL with n > 0; [offsets]: first_iov == NULL or not 8-byte
 * aligned, or views not 8-byte aligned. */
int yu_csum_batch_iov(const yu_iovec *views, const uint64_t *first_iov,
                      uint64_t n, int mode, const uint16_t *initial_arr,
                      uint16_t initial, const uint8_t *addrs, uint16_t *out,
                      void *stream);
int yu_csum_fill_iov(const yu_iovec *views, const uint64_t *first_iov,
                     uint64_t n, int mode, const uint16_t *initial_arr,
                     uint16_t initial, const uint8_t *addrs, uint16_t *out,
                     void *stream);

/* Scatter-gather device batches of whole IPv4 datagrams: the four modes that
 * parse headers out of the packet, on the layout and call discipline of
 * yu_csum_batch_iov above (device CSR tables and bases, asynchronous on
 * `stream`, no allocation, no synchronisation, graph-capturable, YU_ENODEV
 * without a device, n == 0 a no-op returning YU_OK after the mode checks). A
 * received burst held as views is verified where it lies (VERIFY_RX), and an
 * outgoing datagram held as header view + payload view gets both of its fields
 * in one pass (TX_DATAGRAM). Every input is read from the datagram, so there
 * are no side arrays.
 *
 * Modes: IPV4, VERIFY_IPV4, VERIFY_RX, TX_DATAGRAM; every other mode is [mode]
 * (yu_csum_batch_iov takes those). The fill form takes IPV4 and TX_DATAGRAM
 * ([fill-mode]). `out` holds n * YU_MODE_OUTPUTS(mode) values and may be NULL
 * in the fill form.
 *
 * Value: out is exactly what yu_csum_batch_ragged returns for the same bytes
 * laid back to back, in every case that form defines: packets shorter than 20
 * bytes (0 included), any IHL (VERIFY_RX accepts HeaderLength() < 20,
 * TX_DATAGRAM answers {0, 0}), TotalLength() below, at or past the bytes
 * present, bytes past TotalLength() (left out of the transport sum), protocols
 * other than 1, 6 and 17, segments shorter than their fixed header. The header
 * may lie in any number of views, one-byte and empty ones included.
 *
 * Fill: exactly the fields yu_csum_fill_ragged stores. IPV4: bytes 10..11 iff
 * min(len, IHL*4) >= 12. TX_DATAGRAM: bytes 10..11 iff len >= 20 and 20 <=
 * HeaderLength() <= TotalLength() <= len, then the transport field at
 * HeaderLength() + {6 UDP, 16 TCP, 2 ICMP} iff the segment holds its fixed
 * header (8 / 20 / 4 bytes). Each field is stored through the views as
 * yu_csum_fill_iov stores its field: one 16-bit store when its two bytes are
 * adjacent in memory at an even address, two byte stores otherwise (two views
 * included). Nothing else is written.
 *
 * Views, length and "out of contract" are those of yu_csum_batch_iov: at most
 * YU_MAX_TRANSPORT_LEN bytes per packet; an over-limit packet, or one at which
 * first_iov decreases, gets an unspecified value and no field store, never a
 * fault or a hang, and every other packet stays exact. A call reads only
 * dwords that hold bytes of views it names: IPV4 and VERIFY_IPV4 only those of
 * the packet's first min(60, len) bytes, VERIFY_RX and TX_DATAGRAM those and
 * the bytes [HeaderLength(), TotalLength()) of a datagram they sum.
 *
 * YU_EINVAL (Preconditions above): [mode], [fill-mode], [out], [side-align]
 * (out), [offsets], [data], as for yu_csum_batch_iov. */
int yu_csum_batch_iov_datagram(const yu_iovec *views, const uint64_t *first_iov,
                               uint64_t n, int mode, uint16_t *out, void *stream);
int yu_csum_fill_iov_datagram(const yu_iovec *views, const uint64_t *first_iov,
                              uint64_t n, int mode, uint16_t *out, void *stream);

/* Scatter-gather device batches summed and packed in one pass (Linux's
 * csum_and_copy over a view list): the reference concatenates a received
 * VectorisedView with ToView() (buffer/view.go:93-102) before it hands the
 * bytes up, and writev gathers header and payload into one wire image
 * (link/tundev/tundev.go:171-196). These calls do what yu_csum_batch_iov does,
 * on its layout and call discipline (device CSR tables and bases, asynchronous
 * on `stream`, no allocation, no synchronisation, graph-capturable, YU_ENODEV
 * without a device, n == 0 a no-op returning YU_OK after the checks that do not
 * need n), and also store each packet's bytes in one piece: one read of the
 * views, one write of the copy.
 *
 * Copy: the bytes of packet i, the concatenation of its views, len_i of them,
 * are stored at dst[dst_offsets[i], dst_offsets[i] + len_i). `dst_offsets` holds
 * n + 1 DEVICE uint64 values, 8-byte aligned, as the `offsets` of the ragged
 * form; `dst` is a DEVICE pointer of any alignment. A packet may have slack,
 * len_i < dst_offsets[i+1] - dst_offsets[i]; slack bytes are never written.
 * When no packet has slack, (dst, dst_offsets) is exactly the ragged batch
 * yu_csum_batch_ragged takes. dst[0, dst_offsets[n]) must not overlap a byte of
 * any view named, the tables, the side arrays or `out`; this is not checked.
 *
 * Value: out[i] is exactly what yu_csum_batch_iov returns with the same side
 * arguments. Modes: RAW, UDP, TCP, ICMP, VERIFY_TCP, VERIFY_UDP; the TX modes
 * take the field as 0 wherever its two bytes lie.
 *
 * Field bytes in the copy: yu_csum_pack_iov copies them as they are.
 * yu_csum_pack_fill_iov (UDP, TCP, ICMP; `out` may be NULL) gives them the
 * value, big-endian, iff len_i >= f + 2 and the packet is in contract. Neither
 * call ever writes a source view, so views may be shared between packets in
 * both: a header template named by many packets gets its own field in each
 * copy, which yu_csum_fill_iov has to forbid. Every byte of dst is stored by
 * one store of the call, the field bytes included: they are held back until
 * the value is known.
 *
 * Out of contract: a packet with len_i > dst_offsets[i+1] - dst_offsets[i], at
 * which dst_offsets decreases, or out of yu_csum_batch_iov's contract (more
 * than YU_MAX_TRANSPORT_LEN bytes, first_iov decreasing). It gets an
 * unspecified value and unspecified bytes inside its own span
 * [dst_offsets[i], min(dst_offsets[i+1], dst_offsets[n])) (empty if that is no
 * range) and no field value; never a fault or a hang. No call writes a byte of
 * dst outside dst[0, dst_offsets[n]) or outside a packet's own span: each view's
 * copy is cut to the room left. Every other packet is exact in value and
 * bytes. Reads are those of yu_csum_batch_iov: only dwords that hold bytes of
 * the views named.
 *
 * YU_EINVAL (Preconditions above): [mode], [fill-mode], [out], [side-align] as
 * for yu_csum_batch_iov; [offsets]: also dst_offsets == NULL or not 8-byte
 * aligned; [data]: views == NULL or dst == NULL with n > 0.
 *
 * IPV4, VERIFY_IPV4, VERIFY_RX and TX_DATAGRAM are [mode] here:
 * yu_csum_pack_iov_datagram / yu_csum_pack_fill_iov_datagram below take them. */
int yu_csum_pack_iov(const yu_iovec *views, const uint64_t *first_iov,
                     uint64_t n, int mode, const uint16_t *initial_arr,
                     uint16_t initial, const uint8_t *addrs, uint8_t *dst,
                     const uint64_t *dst_offsets, uint16_t *out, void *stream);
int yu_csum_pack_fill_iov(const yu_iovec *views, const uint64_t *first_iov,
                          uint64_t n, int mode, const uint16_t *initial_arr,
                          uint16_t initial, const uint8_t *addrs, uint8_t *dst,
                          const uint64_t *dst_offsets, uint16_t *out, void *stream);

/* Scatter-gather device batches of whole IPv4 datagrams, verified or filled
 * and packed in one pass: what yu_csum_batch_iov_datagram does, and the copy of
 * yu_csum_pack_iov besides. The sending side hands writev a header view and a
 * payload view and needs both fields in the wire image (TX_DATAGRAM, fill); a
 * received VectorisedView is concatenated and then checked (VERIFY_RX). One
 * read of the views, one write of the copy.
 *
 * Call discipline, layout, tables, `dst`, `dst_offsets`, slack, room and "out
 * of contract" are yu_csum_pack_iov's, word for word: device CSR tables and
 * bases, `dst_offsets` n + 1 DEVICE uint64 values, 8-byte aligned, `dst` a
 * DEVICE pointer of any alignment that overlaps nothing the call reads;
 * asynchronous on `stream`, no allocation, no synchronisation,
 * graph-capturable, YU_ENODEV without a device, n == 0 a no-op returning YU_OK
 * after the mode checks. There are no side arrays.
 *
 * Modes: IPV4, VERIFY_IPV4, VERIFY_RX, TX_DATAGRAM; every other mode is [mode]
 * (yu_csum_pack_iov takes those). The fill form takes IPV4 and TX_DATAGRAM
 * ([fill-mode]). `out` holds n * YU_MODE_OUTPUTS(mode) values and may be NULL
 * in the fill form.
 *
 * Value: out is exactly yu_csum_batch_iov_datagram's, in every case that call
 * defines (packets shorter than 20 bytes, 0 included; any IHL; TotalLength()
 * below, at or past the bytes present; bytes past TotalLength(); other
 * protocols; segments shorter than their fixed header).
 *
 * Copy: all len_i bytes of packet i are stored at dst[dst_offsets[i], ...): the
 * header, bytes outside [HeaderLength(), TotalLength()) and bytes past
 * TotalLength() included, for invalid datagrams as for valid ones. The copy
 * does not depend on the parse.
 *
 * Field bytes in the copy: yu_csum_pack_iov_datagram copies them as read.
 * yu_csum_pack_fill_iov_datagram stores exactly the fields yu_csum_fill_ragged
 * would store on the packed copy (yu_csum_fill_iov_datagram's rule: bytes
 * 10..11, and the transport field at HeaderLength() + {6 UDP, 16 TCP, 2 ICMP}),
 * big-endian, iff the packet is in contract; every other byte, and the field
 * bytes of a datagram that gets no field, are copied as read. An out-of-contract
 * packet's field bytes are copied as read where they fit its room. No source
 * view is ever written, so views may be shared between packets: one header
 * template named by many packets gets its own fields in each copy. Every byte
 * of dst is stored by exactly one store of the call, never a
 * read-modify-write: the fill form holds bytes 10..11 and the transport
 * field's bytes back until the packet is done (TotalLength() <= len is known
 * only then) and stores them once, the value or the byte as read.
 *
 * Reads: only dwords that hold bytes of the views named (all of them: the copy
 * takes every byte).
 *
 * YU_EINVAL (Preconditions above): [mode], [fill-mode], [out], [side-align]
 * (out), [offsets] (first_iov, views, dst_offsets), [data] (views == NULL or
 * dst == NULL with n > 0), as for yu_csum_pack_iov. */
int yu_csum_pack_iov_datagram(const yu_iovec *views, const uint64_t *first_iov,
                              uint64_t n, int mode, uint8_t *dst,
                              const uint64_t *dst_offsets, uint16_t *out, void *stream);
int yu_csum_pack_fill_iov_datagram(const yu_iovec *views, const uint64_t *first_iov,
                                   uint64_t n, int mode, uint8_t *dst,
                                   const uint64_t *dst_offsets, uint16_t *out, void *stream);

/* Outgoing IPv4 datagrams built on the device. The reference's senders never
 * hold a packet whose headers somebody else encoded: sendUDP
 * (transport/udp/endpoint.go:164-187), sendTCP / sendTCPWithOptions
 * (transport/tcp/connect.go:556-586, 288-322) and sendICMPv4
 * (network/ipv4/icmp.go:36-45) are handed a payload and a few numbers, encode
 * the transport header into a zeroed Prependable, sum the payload, store the
 * transport field and call WritePacket (network/ipv4/ipv4.go:80-97), which
 * encodes and sums the IPv4 header; the link endpoint writes header and payload
 * as one wire image. yu_tx_build_ragged is that composition for a batch: it
 * takes the payloads and one fixed-size record per packet and writes whole
 * datagrams with both checksum fields. No header is read: there is no view
 * table, no header gather and no parse, the header sums are arithmetic on the
 * record, and each packet has exactly one source range.
 *
 * One outgoing datagram's header fields: 32 bytes, 8-byte aligned, DEVICE
 * memory. Numbers are host byte order (as `out` is); addresses are wire bytes. */
typedef struct yu_tx_record {
  uint8_t  src[4], dst[4];   /* IPv4Fields.SrcAddr / DstAddr                     */
  uint16_t sport, dport;     /* TCP/UDP ports. ICMP: sport = type << 8 | code,   */
                             /*                      dport ignored               */
  uint32_t seq, ack;         /* TCP only                                         */
  uint16_t window;           /* TCP only (the caller clamps, connect.go:559-561) */
  uint8_t  flags;            /* TCP only                                         */
  uint8_t  doff;             /* TCP only: header bytes incl. options, 20..60, %4 */
  uint8_t  proto;            /* 6, 17, 1; any other value: no transport header   */
  uint8_t  ttl;              /* WritePacket: 64                                  */
  uint16_t ip_id;            /* WritePacket: 0                                   */
  uint8_t  tos;              /* 0                                                */
  uint8_t  reserved;         /* 0                                                */
  uint16_t frag;             /* flags/fragment-offset word as a number; 0        */
} yu_tx_record;

/* Call discipline: that of the other device calls. Every pointer is a DEVICE
 * pointer; asynchronous on `stream`, no allocation, no synchronisation,
 * graph-capturable, YU_ENODEV without a device, n == 0 a no-op returning YU_OK
 * after the checks that do not need n.
 *
 * Input: payload i is payload[pay_offsets[i], pay_offsets[i+1]), the ragged
 * layout (n + 1 DEVICE uint64 offsets, 8-byte aligned), any byte alignment; L is
 * its length. For TCP the payload's first doff - 20 bytes are the option bytes,
 * as sendTCPWithOptions prepends them. `recs` holds n records.
 *
 * Output: datagram i is stored at dst[dst_offsets[i], dst_offsets[i] + T).
 * `dst`, `dst_offsets`, slack, room and "overlaps nothing the call reads" are
 * yu_csum_pack_iov's, word for word. With H the transport header's length (TCP
 * 20, UDP 8, ICMP 4, any other protocol 0), T = 20 + H + L, and the image is
 *   bytes 0..19 (IPv4.Encode, header/ipv4.go:146-157, IHL 5):
 *     0x45, tos, BE16(T), BE16(ip_id), BE16(frag), ttl, proto, BE16(ipsum), src, dst
 *   TCP (TCP.Encode, header/tcp.go:176-186): BE16 sport, BE16 dport, BE32 seq,
 *     BE32 ack, (doff / 4) << 4, flags, BE16 window, BE16 xsum, 0, 0, the payload
 *   UDP (header/udp.go:78-83): BE16 sport, BE16 dport, BE16(8 + L), BE16 xsum,
 *     the payload
 *   ICMP: sport >> 8, sport & 0xFF, BE16 xsum, the payload
 *   any other protocol: the payload follows the IPv4 header directly.
 * The two fields are defined by the image itself: ipsum is YU_MODE_IPV4's value,
 * xsum YU_MODE_TX_DATAGRAM's second value for this image with both fields taken
 * as 0. So with tight offsets yu_csum_fill_ragged(TX_DATAGRAM) on the result
 * changes no byte; a UDP sum of 0x0000 is stored as 0x0000 (no 0xFFFF
 * substitution) and an all-zero ICMP segment gets 0xFFFF, as in the reference.
 * `out` may be NULL; otherwise out[2i], out[2i+1] = {ipsum, xsum} as TX_DATAGRAM
 * gives them (other protocols: xsum 0).
 *
 * In contract: T <= 65535; T <= dst_offsets[i+1] - dst_offsets[i], offsets
 * non-decreasing on both sides; TCP: 20 <= doff <= 60, doff % 4 == 0 and
 * doff - 20 <= L. The tables are device memory and are not read on the host, so
 * an out-of-contract packet gets the pack calls' rule: its bytes are
 * unspecified inside its own span [dst_offsets[i], min(dst_offsets[i+1],
 * dst_offsets[n])) only and its out pair is unspecified; never a fault or a
 * hang. A TCP record whose only fault is doff gets every byte exact except the
 * two transport-field bytes. Every other packet is exact, and nothing outside
 * dst[0, dst_offsets[n]) is written.
 *
 * Reads and writes: every payload byte read lies in the dwords that hold
 * payload[0, pay_offsets[n]); record reads are recs[0, n). Every byte of a
 * datagram is stored by exactly one store, never a read-modify-write (with
 * tight packing the rest of a dword belongs to another wave's packet); slack is
 * never written. The header is stored last, once, with both fields in place.
 *
 * YU_EINVAL (Preconditions above): [data]: payload, recs or dst NULL with
 * n > 0; [offsets]: pay_offsets or dst_offsets NULL or not 8-byte aligned, recs
 * not 8-byte aligned; [side-align]: out not 2-byte aligned. */
int yu_tx_build_ragged(const uint8_t *payload, const uint64_t *pay_offsets,
                       const yu_tx_record *recs, uint64_t n,
                       uint8_t *dst, const uint64_t *dst_offsets,
                       uint16_t *out, void *stream);

/* Received IPv4 datagrams taken apart on the device: the inverse of
 * yu_tx_build_ragged. After its checksums (YU_MODE_VERIFY_RX) the reference
 * does four more things with a received datagram before the payload is queued:
 * ipv4.HandlePacket (network/ipv4/ipv4.go:62-77) checks IsValid and trims the
 * IPv4 header, Nic.DeliverTransportPacket (stack/nic.go:125-153) checks the
 * transport header's minimum size and reads the ports, segment.parse
 * (transport/tcp/segment.go:81-109) checks DataOffset, reads seq / ack / flags /
 * window and trims the header, udp.endpoint.HandlePacket
 * (transport/udp/endpoint.go:191-199) checks Length() and trims 8 bytes.
 * yu_rx_split_ragged is that composition for a batch, in one pass over it: per
 * packet VERIFY_RX's flags, the header fields as one yu_tx_record, and the
 * payload stored contiguously.
 *
 * Call discipline: that of yu_tx_build_ragged, word for word. Every pointer is
 * a DEVICE pointer; asynchronous on `stream`, no allocation, no
 * synchronisation, graph-capturable, YU_ENODEV without a device, n == 0 a no-op
 * returning YU_OK after the checks that do not need n.
 *
 * Input: the ragged batch yu_csum_batch_ragged takes, packet i =
 * data[offsets[i], offsets[i+1]) (n + 1 DEVICE uint64 offsets, 8-byte aligned),
 * at any byte alignment. `pay_offsets` holds n + 1 DEVICE uint64 values, 8-byte
 * aligned, and gives packet i the span pay[pay_offsets[i], pay_offsets[i+1]);
 * slack and room are yu_csum_pack_iov's dst_offsets rules. It may be the very
 * array `offsets` (a room of the packet's length always suffices): the tables
 * are only read. pay[0, pay_offsets[n]) overlaps nothing the call reads or
 * writes elsewhere (not checked).
 *
 * Per packet, with b its bytes, len its length, HL = HeaderLength(), TL =
 * TotalLength(), P = Protocol(), the segment S = b[HL:TL], slen = TL - HL and H
 * yu_tx_build_ragged's transport header length (TCP 20, UDP 8, ICMP 4, any other
 * protocol 0):
 *
 * out[i] is exactly the value yu_csum_batch_ragged(VERIFY_RX) gives the packet
 * (YU_RX_IP_OK, _L4, _L4_OK, _INVALID), plus YU_RX_SPLIT, which is set iff
 *   IsValid holds: len >= 20 && HL <= TL <= len;
 *   HL >= 20 (the address bytes are header bytes);
 *   slen >= H (stack/nic.go:133);
 *   TCP: 20 <= DataOffset() <= slen (segment.go:94-97);
 *   UDP: Length() <= slen (udp/endpoint.go:194).
 * Checksum outcomes do not enter YU_RX_SPLIT: the reference does not drop on
 * them (udp/endpoint.go:191-229), the caller combines the bits.
 *
 * With YU_RX_SPLIT, recs[i] holds the datagram's fields in yu_tx_record's
 * layout and byte-order rules: src = b[12:16], dst = b[16:20], proto = P, ttl =
 * b[8], ip_id = BE16(b[4:6]), tos = b[1], frag = BE16(b[6:8]), reserved = 0;
 * TCP: sport, dport, seq, ack, window, flags = S[13], doff = DataOffset(); UDP:
 * sport, dport (the TCP fields and doff are 0); ICMP: sport = type << 8 | code,
 * everything else 0; any other protocol: no transport fields. Not carried: the
 * IPv4 option bytes (HandlePacket trims them), TCP's urgent pointer, the low
 * nibble of TCP byte 12, and UDP's Length() when it is below slen. pay_len[i] =
 * L = slen - H, and the payload S[H:slen] is stored at pay[pay_offsets[i], +L).
 * For TCP it starts with the doff - 20 option bytes, the form
 * yu_tx_build_ragged takes it in. Bytes of b past TL are left out (VERIFY_RX's
 * reading of Payload()).
 * Without YU_RX_SPLIT, recs[i] is 32 zero bytes, pay_len[i] = 0 and no byte of
 * pay is stored.
 *
 * Stores and reads: every record, every pay_len and every out is stored by the
 * call (nothing needs pre-clearing). Every payload byte is stored by exactly one
 * store, never a read-modify-write (with tight pay_offsets the rest of a dword
 * belongs to another wave); slack, and anything outside pay[0, pay_offsets[n]),
 * is never written. Reads lie in the dwords holding data[0, offsets[n]).
 *
 * Round trip: for a datagram with IHL 5, TL == len, YU_RX_SPLIT set, UDP
 * Length() == slen, TCP urgent pointer 0 and data-offset low nibble 0, whose two
 * checksum fields hold the values YU_MODE_TX_DATAGRAM defines,
 * yu_tx_build_ragged over (pay, pay_offsets, recs) reproduces it byte for byte.
 *
 * Out of contract (the tables are device memory and are not read on the host):
 * a packet at which offsets decreases, one longer than YU_MAX_TRANSPORT_LEN or
 * one ending past offsets[n] gets four unspecified results, and unspecified
 * bytes inside its own pay span only. A packet whose L exceeds its room in pay,
 * or at which pay_offsets decreases, keeps exact out, recs and pay_len; only the
 * bytes inside its own span [pay_offsets[i], min(pay_offsets[i+1],
 * pay_offsets[n])) are unspecified. In both cases: never a fault or a hang,
 * every other packet is exact, and nothing outside spans is written.
 *
 * YU_EINVAL (Preconditions above): [data]: data, pay, recs or pay_len NULL with
 * n > 0; [out]: out NULL with n > 0; [offsets]: offsets or pay_offsets NULL or
 * not 8-byte aligned, recs not 8-byte aligned; [side-align]: out not 2-byte
 * aligned or pay_len not 4-byte aligned (checked without n). */
int yu_rx_split_ragged(const uint8_t *data, const uint64_t *offsets, uint64_t n,
                       uint8_t *pay, const uint64_t *pay_offsets,
                       yu_tx_record *recs, uint32_t *pay_len,
                       uint16_t *out, void *stream);

/* Received IPv4 datagrams parsed where they lie: yu_rx_split_ragged without the
 * payload copy, for a receiver that runs its state machine on the records and
 * consumes, gathers or drops the payloads later, or needs the headers only.
 * Instead of a copied payload and pay_len it stores one yu_iovec per packet that
 * points at the payload inside `data`.
 *
 * Call discipline: that of yu_rx_split_ragged, word for word. Every pointer is a
 * DEVICE pointer; asynchronous on `stream`, no allocation, no synchronisation,
 * graph-capturable, YU_ENODEV without a device, n == 0 a no-op returning YU_OK
 * after the checks that do not need n. Input: the ragged batch
 * yu_csum_batch_ragged takes (n + 1 DEVICE uint64 offsets, 8-byte aligned), at
 * any byte alignment.
 *
 * Per packet, with b, len, HL, TL, P, S, slen, H and L as for
 * yu_rx_split_ragged:
 *   recs[i]       exactly the record yu_rx_split_ragged stores: the header fields
 *                 with YU_RX_SPLIT, 32 zero bytes without it.
 *   pay_views[i]  with YU_RX_SPLIT {base = data + offsets[i] + HL + H, len = L},
 *                 the bytes yu_rx_split_ragged would have copied; without it
 *                 {NULL, 0}. n DEVICE yu_iovec, 8-byte aligned. With first_iov =
 *                 0, 1, .., n it is a view table the yu_csum_*_iov calls take as
 *                 it is, so "parse, decide, gather what was accepted" is this
 *                 call, the caller's decision and yu_csum_pack_iov.
 *   out[i]        verify != 0: exactly yu_rx_split_ragged's value, VERIFY_RX's
 *                 four bits plus YU_RX_SPLIT. verify == 0: that value &
 *                 (YU_RX_INVALID | YU_RX_SPLIT), the two bits the header alone
 *                 decides; no checksum is computed and no payload byte is read.
 *
 * Launches: with verify != 0 the VERIFY_RX launch of yu_csum_batch_ragged
 * (yu_ragged_variant_n(YU_MODE_VERIFY_RX, n) names its kernel), which stores
 * out, then the header pass (yu_rx_parse_variant_n) on the same stream, in which
 * the lane that owns packet i ORs YU_RX_SPLIT into out[i]. With verify == 0 the
 * header pass alone.
 *
 * Stores and reads: every record, every view and every out is stored by the call
 * (nothing needs pre-clearing); nothing else is written, `data` never. Reads lie
 * in the dwords holding data[0, offsets[n]); with verify == 0 only dwords holding
 * bytes of each packet's first min(len, 80) bytes are read.
 *
 * Out of contract (the tables are device memory and are not read on the host): a
 * packet at which offsets decreases, one longer than YU_MAX_TRANSPORT_LEN or one
 * ending past offsets[n] gets an unspecified record, view and out of its own,
 * never a fault or a hang. The record, the view and the YU_RX_SPLIT bit of every
 * other packet are exact (the header pass takes each packet by itself); the four
 * VERIFY_RX bits follow yu_csum_batch_ragged's group rule ("Out of contract"
 * above).
 *
 * YU_EINVAL (Preconditions above): [data]: data, recs or pay_views NULL with
 * n > 0; [out]: out NULL with n > 0; [offsets]: offsets NULL or not 8-byte
 * aligned, recs or pay_views not 8-byte aligned; [side-align]: out not 2-byte
 * aligned (checked without n). */
int yu_rx_parse_ragged(const uint8_t *data, const uint64_t *offsets, uint64_t n,
                       int verify, yu_tx_record *recs, yu_iovec *pay_views,
                       uint16_t *out, void *stream);

/* Transport demultiplexing on the device: which endpoint gets a received packet.
 * Once the ports are read, Nic.DeliverTransportPacket hands the packet to
 * transportDemuxer.deliverPacket, whose deliverPacketLocked looks the packet's
 * TransportEndpointId up three times, in a fixed order: the full 4-tuple (a
 * connection), the id with the remote part emptied (a listener bound to an
 * address), the id with the local address emptied as well (a listener on a
 * port). The first hit gets the packet; with none the packet is dropped. The
 * protocol is part of every key (the demuxer's first level). yu_rx_demux is that
 * function for a batch of records as yu_rx_parse_ragged / yu_rx_split_ragged
 * store them, against one table of registered ids. Endpoints, registration at
 * run time, locking, routes and the state machines stay with the caller. */
#define YU_DEMUX_NONE 0xFFFFFFFFu          /* no endpoint: the reference drops the packet */
#define YU_DEMUX_MAX_ENDPOINTS (1u << 24)

/* One registered types.TransportEndpointId plus its protocol: 16 bytes. `kind`
 * is explicit because Go's empty Address is not 0.0.0.0: a connection from
 * 0.0.0.0:0 and a listener are different keys. */
typedef struct yu_endpoint_id {
  uint8_t  local_addr[4];    /* wire bytes; zero when kind == 2                       */
  uint8_t  remote_addr[4];   /* wire bytes; zero when kind != 0                       */
  uint16_t local_port;       /* host byte order, as yu_tx_record's ports              */
  uint16_t remote_port;      /* zero when kind != 0                                   */
  uint8_t  proto;            /* 6 or 17                                               */
  uint8_t  kind;             /* 0: all four fields (a connection)                     */
                             /* 1: RemoteAddress "" and RemotePort 0 (listener on an address) */
                             /* 2: LocalAddress "" as well (listener on a port)       */
  uint16_t reserved;         /* 0 */
} yu_endpoint_id;

/* The table of m ids: an open-addressed hash table whose layout is the
 * library's own, yu_demux_table_bytes(m) bytes (16 bytes per slot; the slot
 * count is the power of two that is at least 16 and at least 2m). 0 when
 * m > YU_DEMUX_MAX_ENDPOINTS. No device needed. */
uint64_t yu_demux_table_bytes(uint64_t m);
/* The 32-bit hash of an id as the table uses it: an id's home slot is
 * yu_demux_hash(id) & (yu_demux_table_bytes(m) / 16 - 1), and ids with one home
 * slot follow each other from it on, wrapping at the table's end. Exported so
 * that colliding ids can be constructed. Fields the id's kind empties are
 * hashed as they stand. No device needed. */
uint32_t yu_demux_hash(const yu_endpoint_id *id);
/* Fills the HOST buffer h_table (table_bytes == yu_demux_table_bytes(m)) with
 * the table of ids[0, m); the caller copies it to the device, 16-byte aligned,
 * like every other buffer the device calls take. An endpoint's number is its
 * position in `ids`. m == 0 gives the empty table (16 empty slots). No device
 * needed.
 *
 * YU_EINVAL ([data], Preconditions above), before a byte of h_table is written:
 * ids or h_table NULL with m > 0; table_bytes != yu_demux_table_bytes(m); m >
 * YU_DEMUX_MAX_ENDPOINTS; an id that is malformed (proto not 6 or 17, kind > 2,
 * a field its kind empties not zero, reserved != 0) or that equals an earlier
 * one (the reference's ErrPortInUse, stack/transport_demuxer.go:69). *bad, where
 * bad != NULL, receives the index of the first such id, or m when the fault is
 * not an id; on YU_OK it receives m. YU_ENOMEM: no host memory for the working
 * copy (as large as the table). */
int yu_demux_table_fill(const yu_endpoint_id *ids, uint64_t m,
                        void *h_table, uint64_t table_bytes, uint64_t *bad);

/* Call discipline: that of the other device calls. Every pointer is a DEVICE
 * pointer; asynchronous on `stream`, no allocation, no synchronisation,
 * graph-capturable, YU_ENODEV without a device, n == 0 a no-op returning YU_OK
 * after the checks that do not need n.
 *
 * Input: `recs`, n records, 8-byte aligned; `flags`, NULL or n uint16, the `out`
 * of yu_rx_parse_ragged or yu_rx_split_ragged for these records; `table`, 16-byte
 * aligned, the bytes yu_demux_table_fill wrote for m ids, table_bytes ==
 * yu_demux_table_bytes(m).
 *
 * Packet i is eligible iff recs[i].proto is 6 or 17 and, with flags != NULL,
 * (flags[i] & (need | YU_RX_SPLIT)) == (need | YU_RX_SPLIT). A packet without
 * YU_RX_SPLIT has an all-zero record and is ineligible either way. need == 0 is
 * the reference, which does not drop on checksum outcomes at this point; need ==
 * YU_RX_IP_OK | YU_RX_L4_OK is a receiver that does. ICMP and every other
 * protocol are ineligible: DeliverTransportPacket finds no transport protocol
 * for them and drops (stack/nic.go:126-130).
 *
 * The id of an eligible packet is {LocalPort: dport, LocalAddress: dst,
 * RemotePort: sport, RemoteAddress: src} (stack/nic.go:144; on receive the
 * record's dst is local). It is looked up as kind 0 with all four fields, as
 * kind 1 with the remote fields zero, as kind 2 with the local address zero too,
 * each with the record's protocol.
 *   ep[i]        the index of the first hit; YU_DEMUX_NONE when all three miss or
 *                the packet is ineligible. n DEVICE uint32, every one stored.
 *   ep_count     NULL, or m + 1 DEVICE uint32 counters the call ADDS to (the
 *                caller zeroes them; accumulating over several batches is the
 *                caller's choice): ep_count[e] by the number of packets with
 *                ep[i] == e, ep_count[m] by the number with YU_DEMUX_NONE. Their
 *                exclusive sum is the CSR of a grouping by endpoint.
 *
 * One launch (yu_rx_demux_variant_n names its kernel). Reads: the records'
 * first 16 bytes and the dword holding proto, flags, and slots of the table.
 * Nothing but ep and ep_count is written.
 *
 * Out of contract (the table's contents are device memory and are not read on
 * the host): a table with other contents than yu_demux_table_fill's gives
 * unspecified ep values and counts, never a fault or a hang: every probe
 * address lies in table[0, table_bytes); a lookup makes at most table_bytes / 16
 * probes, even if no slot is empty; an index at or above m read from a slot is
 * taken as YU_DEMUX_NONE, so no counter outside ep_count[0, m] is touched.
 * Finite is not fast: on a table without an empty slot every miss walks all
 * table_bytes / 16 slots, three times per packet, one dependent load after the
 * other (at m = 2^24 up to about 10^8 probes per packet), so such a call can run
 * for seconds or, on a large batch, far longer. A table yu_demux_table_fill
 * wrote is at most half full and its chains are short.
 *
 * YU_EINVAL (Preconditions above): [data]: recs or table NULL with n > 0,
 * table_bytes != yu_demux_table_bytes(m), m > YU_DEMUX_MAX_ENDPOINTS (the last two
 * checked without n); [out]: ep NULL with n > 0; [offsets]: recs not 8-byte
 * aligned, table not 16-byte aligned (with n > 0); [side-align]: flags not
 * 2-byte aligned, ep or ep_count not 4-byte aligned (checked without n). */
int yu_rx_demux(const yu_tx_record *recs, const uint16_t *flags, uint16_t need,
                uint64_t n, const void *table, uint64_t table_bytes, uint64_t m,
                uint32_t *ep, uint32_t *ep_count, void *stream);

/* Grouping by endpoint on the device: the step between yu_rx_demux (decide) and
 * yu_csum_pack_iov (gather). deliverPacketLocked ends in ep.HandlePacket, which
 * appends the packet to that endpoint's queue in arrival order (rcvList.PushBack
 * in transport/udp/endpoint.go, segmentQueue.enqueue in transport/tcp/endpoint.go).
 * For a batch that is the stable grouping of the packet numbers by endpoint plus
 * the CSR saying where each endpoint's queue starts. All results are exact
 * integers.
 *
 * Call discipline: that of the other device calls. Every pointer is a DEVICE
 * pointer; asynchronous on `stream`, no allocation, no synchronisation,
 * graph-capturable, YU_ENODEV without a device. The scratch memory is therefore
 * the caller's: `work`, 16-byte aligned, work_bytes >=
 * yu_rx_group_workspace_bytes(n, m). NOT a no-op at n == 0, unlike every other
 * device call: the call then stores first[0 .. m+1] = 0 and, where q_offsets !=
 * NULL, q_offsets[0] = 0, so that no caller ever meets an undefined CSR; it
 * needs neither ep, order nor work for that, and it needs a device.
 *
 *   key(i)     ep[i] if ep[i] < m, else m: YU_DEMUX_NONE and every other value at
 *              or above m are "no endpoint". ep: n DEVICE uint32 (yu_rx_demux's).
 *   order[j]   j in [0, n): the packet numbers sorted by (key, i), the stable sort
 *              by key. n DEVICE uint32, every one stored.
 *   first[e]   e in [0, m+1]: the number of packets with key < e. m + 2 DEVICE
 *              uint64, 8-byte aligned, every one stored; first[0] = 0, first[m+1]
 *              = n. order[first[e] .. first[e+1]) is endpoint e's queue in arrival
 *              order, order[0 .. first[m]) every delivered packet. Derived from ep
 *              alone; yu_rx_demux's ep_count, which a caller may have accumulated
 *              over several batches, is not taken.
 *   views      NULL, or n yu_iovec, 8-byte aligned (yu_rx_parse_ragged's
 *              pay_views). Then q_views and q_offsets are required, else both
 *              must be NULL.
 *   q_views[j] views[order[j]] for j < first[m], {NULL, 0} for j >= first[m]; n
 *              yu_iovec, 8-byte aligned.
 *   q_offsets[j]  the sum of q_views[j'].len over j' < j, modulo 2^64; n + 1 DEVICE
 *              uint64, 8-byte aligned, q_offsets[0] = 0. (q_views, first_iov = 0,
 *              1, .., n, q_offsets) is exactly the input of yu_csum_pack_iov(...,
 *              n, YU_MODE_RAW, ..., dst, q_offsets, out, stream) over all n
 *              packets: dropped packets copy no byte, and endpoint e's payloads
 *              lie contiguous and in arrival order at dst[q_offsets[first[e]],
 *              q_offsets[first[e+1]]). The caller sizes dst on the host by an
 *              upper bound (the batch's offsets[n], say); nothing is read back.
 *
 * yu_rx_group_workspace_bytes(n, m) needs no device, is the same for every
 * device and is monotone in n; 0 when m > YU_DEMUX_MAX_ENDPOINTS or n >= 2^32
 * (order holds 32-bit packet numbers). With b = bitlen(m), P = max(1,
 * ceil(b / 8)) passes, D = max(1, ceil(b / P)) digit bits, B = min(ceil(n /
 * 1024), 8192) and r16(x) = x rounded up to a multiple of 16, it is
 *   r16(4 * 2^D * B)                                     the pass histogram
 * + r16(8 * ceil(max(2^D * B, m + 2, n + 1) / 2048))     the scan's tile sums
 * + (P > 1 ? r16(4 * (m + 1)) + r16(8 * n) : 0)          key counts, (key, number) pairs
 * + (P > 2 ? r16(8 * n) : 0)                             the second pair buffer.
 *
 * Launches: a stable least-significant-digit radix partition, P passes of a
 * block histogram, a device-wide exclusive scan (three launches, no block waits
 * for another) and a scatter; then `first` (read off the histogram when P == 1,
 * else the scan of the key counts) and, with views, the gather of the views and
 * the scan of their lengths. yu_rx_group_variant_n names the pass count.
 *
 * Writes: nothing but order, first, q_views, q_offsets and work[0,
 * yu_rx_group_workspace_bytes(n, m)). Reads: ep and views, which must not be
 * written while the call runs. ep holds arbitrary 32-bit values by the
 * definition of the key, so there is no out-of-contract ep; if ep changes under
 * the call the results are unspecified, but every scatter index is compared
 * with n before its store and no kernel waits for another block: never a
 * fault, a hang or a store outside the outputs. View lengths are summed as they
 * stand; yu_csum_pack_iov's own contract handles an oversized one.
 *
 * YU_EINVAL (Preconditions above): [offsets]: first, q_offsets, views or q_views
 * not 8-byte aligned, work not 16-byte aligned; [side-align]: ep or order not
 * 4-byte aligned; [data], checked without n: m > YU_DEMUX_MAX_ENDPOINTS, n >=
 * 2^32; [out]: first NULL (with any n), order NULL with n > 0; [data], each with
 * n > 0: ep or work NULL, work_bytes too small, some but not all of views,
 * q_views and q_offsets given. The alignments are checked without n. */
uint64_t yu_rx_group_workspace_bytes(uint64_t n, uint64_t m);
int yu_rx_group(const uint32_t *ep, uint64_t n, uint64_t m,
                const yu_iovec *views, uint32_t *order, uint64_t *first,
                yu_iovec *q_views, uint64_t *q_offsets,
                void *work, uint64_t work_bytes, void *stream);

/* Answering received datagrams on the device: the step that joins the receive
 * half (yu_rx_parse_ragged, yu_rx_demux) to the send half (yu_tx_build_iov
 * below). It is what the reference's samples do with a packet:
 * sample/tun_udp_echo is ep.Read followed by ep.Write(v, &fullAddr), which ends in
 * sendUDP(route, v, e.id.LocalPort, to.Port) with the addresses and ports turned
 * round (transport/udp/endpoint.go:138-187), and ipv4.handleICMP answers every
 * Echo with sendICMPv4(r, ICMPv4EchoReply, 0, v) once
 * vv.TrimFront(ICMPv4MinimumSize) has cut the ICMP header off
 * (network/ipv4/icmp.go:28-63). yu_rx_reply decides which packets of a batch are
 * answered, stores the replies' records and says where each reply will lie;
 * yu_tx_build_iov then builds the replies straight from the payload views. So
 * parse, demux, reply and build are four asynchronous calls on one stream with
 * no host read and no payload copy between them, and capture as one graph.
 *
 * Not modelled: the reply's source address is the request's destination, the
 * single-address case of FindRoute with an empty bindAddr (stack/stack.go:162; a
 * stack with several addresses or a bound endpoint may choose another); the UDP
 * endpoint's rcvBufSizeMax drop (transport/udp/endpoint.go:204: a full receive
 * queue drops the datagram before the sample reads it); and the TCP
 * state machine, so TCP segments get no reply here. Only Type() of an ICMP
 * message is tested, as icmp.go:57 does: the code is ignored, and no checksum
 * outcome is tested beyond `need`.
 *
 * Call discipline: that of yu_rx_group. Every pointer is a DEVICE pointer;
 * asynchronous on `stream`, no allocation, no synchronisation, graph-capturable,
 * YU_ENODEV without a device. The scratch memory is the caller's: `work`, 16-byte
 * aligned, work_bytes >= yu_rx_reply_workspace_bytes(n), which needs no device, is
 * monotone in n and is the tile sums of one scan over n + 1 outputs: 8 *
 * ceil((n + 1) / 2048) rounded up to a multiple of 16. NOT a no-op at n == 0: the
 * call then stores r_offsets[0] = 0, as yu_rx_group stores its empty CSR; it
 * needs nothing but r_offsets for that, and it needs a device.
 *
 * Input: `recs` (n records, 8-byte aligned), `flags` (NULL or n uint16) and
 * `views` (n yu_iovec, 8-byte aligned) are what yu_rx_parse_ragged stored; `ep`
 * (n uint32) is yu_rx_demux's output and m its endpoint count; `ep_echo` is NULL
 * or m bytes, non-zero meaning "this endpoint echoes" (NULL: every endpoint
 * does). `what` is a combination of the YU_REPLY_ bits. ep may be NULL without
 * YU_REPLY_UDP_ECHO.
 *
 * Per packet i, with the gate of yu_rx_demux (flags == NULL, or (flags[i] &
 * (need | YU_RX_SPLIT)) == (need | YU_RX_SPLIT)), L = views[i].len and H
 * yu_tx_build_ragged's transport header length:
 *   ICMP echo  what & YU_REPLY_ICMP_ECHO, the gate, recs[i].proto == 1 and
 *              recs[i].sport >> 8 == 8 (Echo). The reply record: src = recs[i].dst,
 *              dst = recs[i].src, sport = 0 (EchoReply, code 0), proto = 1, ttl =
 *              64, every other field 0. The payload is the view, S[4:slen].
 *   UDP echo   what & YU_REPLY_UDP_ECHO, the gate, recs[i].proto == 17, ep[i] < m
 *              and (ep_echo == NULL or ep_echo[ep[i]] != 0). The reply record:
 *              src = recs[i].dst, dst = recs[i].src, sport = recs[i].dport, dport =
 *              recs[i].sport, proto = 17, ttl = 64, every other field 0. The
 *              payload is the view, S[8:slen].
 *   no reply   everything else: TCP, other protocols, the all-zero record of a
 *              packet without YU_RX_SPLIT, and any L > 65535 - 20 - H.
 *   r_recs[i]  the reply record, or 32 zero bytes. n records, 8-byte aligned.
 *   T[i]       20 + H + L, or 0 when there is no reply.
 *   r_offsets[j]  the sum of T[i] over i < j, for j in [0, n]: n + 1 DEVICE uint64,
 *              8-byte aligned. The replies form a tight ragged batch in arrival
 *              order in which an unanswered packet is an empty entry:
 *              yu_tx_build_iov(views, r_recs, n, dst, r_offsets, out, stream)
 *              builds it, skipping the empty entries. The caller sizes dst on the
 *              host by an upper bound: a reply has IHL 5 and carries no byte past
 *              TotalLength, so T[i] is at most the received datagram's length and
 *              the batch's offsets[n] always suffices. Nothing is read back.
 *
 * Launches: k_reply (yu_rx_reply_variant_n), a lane per packet, which leaves T[i]
 * in r_offsets[i]; then yu_rx_group's device-wide exclusive scan in place (three
 * launches, no block waits for another).
 *
 * Writes: every r_recs[i] and every r_offsets[j] is stored (nothing needs
 * pre-clearing); nothing else is written except work[0,
 * yu_rx_reply_workspace_bytes(n)). Reads: recs, flags, views (the table, never
 * the payload bytes), ep and ep_echo, which must not be written while the call
 * runs and must not overlap what it writes. ep holds arbitrary 32-bit values (a
 * value at or above m is "no endpoint"), so the ep_echo index always lies in the
 * table: never a fault or a hang.
 *
 * YU_EINVAL (Preconditions above): [offsets]: recs, views, r_recs or r_offsets
 * not 8-byte aligned, work not 16-byte aligned; [side-align]: flags not 2-byte
 * aligned, ep not 4-byte aligned; [data], checked without n: m >
 * YU_DEMUX_MAX_ENDPOINTS, `what` with unknown bits; [out]: r_offsets NULL (with
 * any n), r_recs NULL with n > 0; [data], each with n > 0: recs, views or work
 * NULL, work_bytes too small, ep NULL with YU_REPLY_UDP_ECHO. The alignments are
 * checked without n. */
#define YU_REPLY_ICMP_ECHO 1u
#define YU_REPLY_UDP_ECHO  2u
uint64_t yu_rx_reply_workspace_bytes(uint64_t n);
int yu_rx_reply(const yu_tx_record *recs, const uint16_t *flags, uint16_t need,
                const yu_iovec *views, const uint32_t *ep, uint64_t m,
                const uint8_t *ep_echo, uint32_t what, uint64_t n,
                yu_tx_record *r_recs, uint64_t *r_offsets,
                void *work, uint64_t work_bytes, void *stream);

/* yu_tx_build_ragged with the payloads where they lie: the payload of packet i
 * is views[i] instead of payload[pay_offsets[i], pay_offsets[i+1]). Everything
 * else is yu_tx_build_ragged's, word for word: the call discipline (n == 0 a
 * no-op), recs, dst, dst_offsets, slack, room, the image, the two fields, `out`,
 * the store rules and the in-contract rules. Two differences:
 *
 * The views. n yu_iovec, 8-byte aligned, DEVICE memory; each at any base
 * alignment and of any length, {NULL, 0} an empty payload. Views may overlap
 * each other and several packets may name one view; no view may overlap dst
 * (not checked). Pointers are trusted, as in the scatter-gather calls: bytes are
 * read only in the dwords holding a view. A view longer than 65535 - 20 - H is
 * out of contract under the pack calls' rule: the walk stops at the limit,
 * unspecified bytes stay inside the packet's own span, its out pair is {0, 0};
 * never a fault or a hang.
 *
 * An empty destination span is a skipped packet. A packet with dst_offsets[i+1]
 * == dst_offsets[i] is skipped by definition, not out of contract: its view is
 * not dereferenced, its record is ignored, no byte is written and out[2i],
 * out[2i+1] = 0, 0. That is what lets yu_rx_reply's r_recs and r_offsets and
 * yu_rx_parse_ragged's view table be passed as they stand.
 *
 * One launch (yu_tx_build_iov_variant_n: "k_build<4,iov>"), on
 * yu_tx_build_ragged's grid.
 *
 * YU_EINVAL (Preconditions above): [data]: views, recs or dst NULL with n > 0;
 * [offsets]: dst_offsets NULL or not 8-byte aligned, views or recs not 8-byte
 * aligned; [side-align]: out not 2-byte aligned. */
int yu_tx_build_iov(const yu_iovec *views, const yu_tx_record *recs, uint64_t n,
                    uint8_t *dst, const uint64_t *dst_offsets,
                    uint16_t *out, void *stream);

/* TCP segments delivered in order on the device: the step between yu_rx_group
 * (each endpoint's packets in arrival order) and yu_csum_pack_iov (gather). A UDP
 * endpoint's queue is its data; a TCP endpoint does not deliver its queue, it runs
 * receiver.handleRcvdSegment over it (transport/tcp/rcv.go): the acceptability
 * test against the window, consumeSegment with its trim of bytes already
 * delivered, the heap of out-of-order segments bounded by pendingBufSize
 * (segment_heap.go, container/heap), the drain of that heap when a gap closes,
 * FIN, and an ACK (sendAck -> getSendParams) for everything that is not plain
 * in-order data. yu_rx_stream is that function for every TCP connection of a
 * batch at once, with the gates of handleSegments around it (RST, the ACK flag,
 * the final ACK check). It reads records and view tables only, never a payload
 * byte. So parse, demux, group, stream and gather, plus yu_tx_build_iov for the
 * ACKs, are asynchronous calls on one stream with no host read; they capture as
 * one graph that is replayed batch after batch while the connections' state
 * lives in device memory.
 *
 * Not modelled: the sender half (snd.handleRcvdSegment on the ack field,
 * retransmission, sendData); maxSegmentsPerWake (a batch is one wake-up); the
 * segment queue's own limit; one ACK datagram per sendAck (the batch coalesces:
 * one ACK per connection from the final state, n_acks says how many the
 * reference would have sent); handshakes and listeners (state 0). The one
 * departure inside the rule is `cap`, a fixed number of heap entries per endpoint:
 * a segment that would be parked while pend_count == cap is dropped and ACKed as
 * if the byte budget were full; cap == 0 is a receiver that keeps nothing out of
 * order.
 *
 * All sequence arithmetic is uint32 and wraps; lt(a, b) is (int32_t)(a - b) < 0
 * (seqnum.LessThan). Per-connection state, 40 bytes, 8-byte aligned, DEVICE
 * memory, read and written in place: */
typedef struct yu_tcp_rcv {
  uint32_t rcv_nxt, rcv_acc;      /* receiver.rcvNxt, rcvAcc                                 */
  uint32_t pend_used, pend_size;  /* pendingBufUsed, pendingBufSize                          */
  uint32_t buf_size, buf_used;    /* endpoint.rcvBufSize, rcvBufUsed (the caller lowers      */
                                  /* buf_used between calls when the application reads)      */
  uint32_t snd_nxt;               /* sender.sndNxt: the sequence number an ACK carries       */
  uint32_t max_sent_ack;          /* sender.maxSentAck                                       */
  uint32_t pend_count;            /* entries of this endpoint's heap in use                  */
  uint8_t  wnd_scale;             /* receiver.rcvWndScale                                    */
  uint8_t  state;                 /* 0 off (not a TCP connection this call serves),          */
                                  /* 1 open, 2 closed (FIN consumed), 3 reset (RST seen)     */
  uint16_t reserved;              /* 0 */
} yu_tcp_rcv;

typedef struct yu_tcp_seg {       /* 32 bytes, one pending segment */
  yu_iovec data;                  /* its data where it lies, options already cut off         */
  uint32_t seq;
  uint32_t pkt;                   /* packet number in the current batch, YU_DEMUX_NONE for   */
                                  /* a segment carried over from an earlier batch            */
  uint8_t  flags, reserved[7];
} yu_tcp_seg;

/* The verdict on one packet, status[i]. */
#define YU_SEG_NONE          0u  /* no endpoint, a state-0 endpoint, or no usable TCP record */
#define YU_SEG_CONSUMED      1u  /* in order: delivered (or a pure ACK on rcv_nxt)           */
#define YU_SEG_CONSUMED_LATE 2u  /* parked in this batch, delivered when the gap closed      */
#define YU_SEG_PENDING       3u  /* parked in the heap, still there                          */
#define YU_SEG_DUPLICATE     4u  /* parked in this batch, popped as already acknowledged     */
#define YU_SEG_DROPPED       5u  /* out of order and no room: byte budget or cap             */
#define YU_SEG_UNACCEPTABLE  6u  /* outside the window (RFC 793 p. 26): ACKed only           */
#define YU_SEG_NOOP          7u  /* a pure ACK off rcv_nxt                                   */
#define YU_SEG_IGNORED       8u  /* no ACK flag                                              */
#define YU_SEG_AFTER_CLOSE   9u  /* arrived after the FIN was consumed                       */
#define YU_SEG_RST           10u /* the RST that reset the connection                        */
#define YU_SEG_UNPROCESSED   11u /* queued behind an RST, or the connection was reset before */

/* Call discipline: that of yu_rx_group. Every pointer is a DEVICE pointer;
 * asynchronous on `stream`, no allocation, no synchronisation, graph-capturable,
 * YU_ENODEV without a device. The scratch memory is the caller's: `work`, 16-byte
 * aligned, work_bytes >= yu_rx_stream_workspace_bytes(n, m, cap), which needs no
 * device: with N = n + m * cap it is 8 * ceil((max(N, m) + 1) / 2048) rounded up to
 * a multiple of 16, the tile sums of the longer of the call's two scans; 0 when m >
 * YU_DEMUX_MAX_ENDPOINTS, n >= 2^32 or cap > 1024. NOT a no-op at n == 0: the empty
 * tables are stored (every slot {NULL, 0}, every offset 0, every a_recs zero, every
 * n_acks 0); no state and no heap entry is touched then, and `first` is not read.
 *
 * Input: `recs` (n records) and `views` (n yu_iovec) are yu_rx_parse_ragged's
 * outputs; `order` (n uint32) and `first` (m + 2 uint64) yu_rx_group's; `ids` a
 * device copy of the m ids yu_demux_table_fill was given (4-byte aligned); `st`, m
 * yu_tcp_rcv; `heap`, m * cap yu_tcp_seg, 8-byte aligned: endpoint e's heap is
 * heap[e * cap .. e * cap + st[e].pend_count), container/heap over segmentHeap
 * with lt on seq as the order (Push appends and sifts up; Pop swaps the first and
 * last entries, sifts down over the first n - 1 and removes the last), so the
 * array order is defined exactly and is part of the output.
 *
 * The walk for endpoint e goes over its queue order[first[e] .. first[e+1]) in
 * order; every field below is st[e]'s. An endpoint whose queue is empty is not
 * touched (the reference only runs on a wake-up); its slots and ACK outputs are
 * still stored empty. For packet i with record R and view V: opt = R.doff - 20,
 * dlen = V.len - opt, base = V.base + opt.
 *   1. state 0: every packet YU_SEG_NONE; st[e] and the heap are not touched.
 *   2. state 3 at entry: every packet YU_SEG_UNPROCESSED, no ACK, nothing touched.
 *   3. R.proto != 6, R.doff < 20, opt > V.len or V.len > 65535: YU_SEG_NONE.
 *   4. R.flags & 4 (RST): YU_SEG_RST, state = 3, every later packet of the queue
 *      YU_SEG_UNPROCESSED, no final ACK check (handleSegments returns false).
 *   5. !(R.flags & 16): YU_SEG_IGNORED.
 *   6. state == 2: YU_SEG_AFTER_CLOSE.
 *   7. wnd = rcv_acc - rcv_nxt. With wnd == 0 the segment is acceptable iff dlen ==
 *      0 && seq == rcv_nxt; else iff (seq - rcv_nxt) < wnd, or lt(rcv_nxt, seq +
 *      dlen) && lt(seq, rcv_acc). Not acceptable: ack(), YU_SEG_UNACCEPTABLE. A
 *      segment that overshoots rcv_acc is delivered whole; wnd then wraps to a huge
 *      value, as in the reference.
 *   8. consume(seq, dlen, base, flags). dlen > 0: fail unless (rcv_nxt - seq) <
 *      dlen; trim rcv_nxt - seq bytes off the front of seq, dlen and base; append
 *      {base, dlen} to the endpoint's delivered slots; buf_used += dlen. dlen == 0:
 *      fail unless seq == rcv_nxt. Then rcv_nxt = seq + dlen; with FIN rcv_nxt++,
 *      ack(), state = 2.
 *   9. consume failed: with dlen > 0 or FIN the segment is parked if pend_used <
 *      pend_size && pend_count < cap (pend_used += dlen + SYN + FIN,
 *      YU_SEG_PENDING, its heap entry holds {base, dlen}, seq, pkt = i, flags), else
 *      YU_SEG_DROPPED; ack() either way. A pure ACK off rcv_nxt: YU_SEG_NOOP.
 *  10. consume succeeded: YU_SEG_CONSUMED, then the drain: while state == 1 and
 *      pend_count > 0, with t the heap's first entry: if !lt(t.seq + t.len - 1,
 *      rcv_nxt) and consume(t) fails, stop; else pop t and pend_used -= its
 *      logical length AFTER consume's trim (the reference subtracts the trimmed
 *      length, so the budget can stay above zero). A popped entry with pkt !=
 *      YU_DEMUX_NONE gets YU_SEG_CONSUMED_LATE if consumed, YU_SEG_DUPLICATE if
 *      skipped as already acknowledged. (A parked FIN without data is popped as
 *      acknowledged when reached, t.seq - 1 being below rcv_nxt: the reference's
 *      behaviour.)
 *  11. end of the queue, state 1 or 2: if rcv_nxt != max_sent_ack, ack(). After a
 *      walk that touched the state every remaining heap entry gets pkt =
 *      YU_DEMUX_NONE.
 * ack(): n_acks++; avail = buf_used >= buf_size ? 0 : buf_size - buf_used; acc =
 * rcv_nxt + avail; if lt(rcv_acc, acc) rcv_acc = acc; max_sent_ack = rcv_nxt.
 *
 * Output, with N = n + m * cap:
 *   status     n bytes, every one stored; packets without an endpoint
 *              (order[first[m] .. n)) get YU_SEG_NONE.
 *   s_views    N yu_iovec, 8-byte aligned, every one stored. Endpoint e owns the
 *              slots [first[e] + e * cap, first[e+1] + (e + 1) * cap); its delivered
 *              views fill them from the front in delivery order, the rest and the
 *              slots from first[m] + m * cap on are {NULL, 0}.
 *   s_offsets  N + 1 uint64, the exclusive sum of the slot lengths. (s_views,
 *              first_iov = 0 .. N, s_offsets) is yu_csum_pack_iov(RAW)'s input as it
 *              stands; connection e's new in-order bytes lie at dst[s_offsets[lo],
 *              s_offsets[hi]) with [lo, hi) its slots.
 *   a_recs     m records: per endpoint with n_acks > 0 the ACK from the final state
 *              (sendTCP's fields): src, dst = ids[e].local_addr, remote_addr; sport,
 *              dport = local_port, remote_port; seq = snd_nxt; ack = rcv_nxt; window
 *              = min((rcv_acc - rcv_nxt) >> wnd_scale, 0xFFFF); flags 16, doff 20,
 *              proto 6, ttl 64, everything else 0. 32 zero bytes otherwise.
 *   a_offsets  m + 1 uint64: the exclusive sum of 40 per endpoint with an ACK.
 *              yu_tx_build_iov(zero_views, a_recs, m, dst, a_offsets, ..) builds the
 *              ACK datagrams from a zeroed m-entry view table the caller supplies.
 *   n_acks     m uint32, stored, not added to: the ACKs the reference would have sent.
 * a_recs, a_offsets and n_acks are all NULL or all given.
 *
 * Lifetime: a parked segment's view points into the batch it arrived in. The
 * caller keeps that memory until the segment has been delivered or the connection
 * is torn down. cap = 0 avoids it.
 *
 * Launches: k_stream (yu_rx_stream_variant_n), a wave per endpoint on a
 * grid-stride loop, 64 queue entries per wave step, a run of plain in-order
 * segments taken 64 at a time; then yu_rx_group's device-wide exclusive scan in
 * place over s_offsets and, with the ACK outputs, over a_offsets.
 *
 * Out of contract (the tables are device memory and are not read on the host),
 * with unspecified results for the endpoints concerned only: order values at or
 * above n, a `first` that is not monotone or exceeds n, pend_count > cap, a heap
 * that is not heap-ordered. Every index is compared with its bound before use and
 * every loop is bounded by the queue length or by cap: never a fault, a hang or a
 * store outside the outputs.
 *
 * YU_EINVAL (Preconditions above): [offsets]: recs, views, first, st, heap,
 * s_views, s_offsets, a_recs or a_offsets not 8-byte aligned, work not 16-byte
 * aligned; [side-align]: order, ids or n_acks not 4-byte aligned; [data], checked
 * without n: m > YU_DEMUX_MAX_ENDPOINTS, n >= 2^32, cap > 1024, st NULL with m > 0,
 * some but not all of a_recs, a_offsets and n_acks given; [out]: s_offsets NULL
 * with m > 0 (any n) or n > 0, status or s_views NULL with n > 0, s_views NULL
 * with m * cap > 0; [data], each with n > 0: recs, views, order, first or work
 * NULL, work_bytes too small, heap NULL with m * cap > 0, ids NULL with the ACK
 * outputs and m > 0. The alignments are checked without n. */
uint64_t yu_rx_stream_workspace_bytes(uint64_t n, uint64_t m, uint32_t cap);
int yu_rx_stream(const yu_tx_record *recs, const yu_iovec *views, uint64_t n,
                 const uint32_t *order, const uint64_t *first, uint64_t m,
                 const yu_endpoint_id *ids, yu_tcp_rcv *st, yu_tcp_seg *heap, uint32_t cap,
                 uint8_t *status, yu_iovec *s_views, uint64_t *s_offsets,
                 yu_tx_record *a_recs, uint64_t *a_offsets, uint32_t *n_acks,
                 void *work, uint64_t work_bytes, void *stream);

/* Host-memory field writer: the matching yu_csum_batch_host_* call (TX modes
 * UDP/TCP/IPV4/ICMP/TX_DATAGRAM only), then each result stored big-endian into the
 * packet's checksum field in host memory, as the device writer does
 * (yu_csum_fill_uniform). `h_out` may be NULL. The iov form writes through
 * the views (their `base` must be writable memory). Synchronous. */
int yu_csum_fill_host_uniform(uint8_t *h_data, uint64_t stride, uint32_t len,
                              uint64_t n, int mode,
                              const uint16_t *h_initial_arr, uint16_t initial,
                              const uint8_t *h_addrs, uint16_t *h_out,
                              int device);
int yu_csum_fill_host_ragged(uint8_t *h_data, const uint64_t *h_offsets,
                             uint64_t n, int mode,
                             const uint16_t *h_initial_arr, uint16_t initial,
                             const uint8_t *h_addrs, uint16_t *h_out,
                             int device);
int yu_csum_fill_host_iov(const yu_iovec *iov, const uint64_t *first_iov,
                          uint64_t n, int mode, const uint16_t *h_initial_arr,
                          uint16_t initial, const uint8_t *h_addrs,
                          uint16_t *h_out, int device);

/* Multi-GPU host path (SURVEY.md §8b `yu_csum_batch_host(..., ngpu)`, §8e):
 * the same three calls with the batch split into ndev contiguous shards, one
 * per entry of `devices` (a device may be listed more than once), each shard
 * run through the single-device pipeline on that device by a persistent
 * per-device worker thread, all at once. Packets are independent, so there
 * is no exchange: shard i writes h_out[first_i, first_i + n_i). Uniform and
 * iovec batches split by packet count, ragged batches on the packet boundary
 * nearest an even split of the bytes (balanced PCIe traffic). Synchronous;
 * returns the first failing shard's status (YU_EINVAL for ndev < 1 or > 64,
 * YU_ENODEV for a device index out of range). */
int yu_csum_batch_host_uniform_multi(const uint8_t *h_data, uint64_t stride,
                                     uint32_t len, uint64_t n, int mode,
                                     const uint16_t *h_initial_arr,
                                     uint16_t initial, const uint8_t *h_addrs,
                                     uint16_t *h_out, const int *devices,
                                     int ndev);
int yu_csum_batch_host_ragged_multi(const uint8_t *h_data,
                                    const uint64_t *h_offsets, uint64_t n,
                                    int mode, const uint16_t *h_initial_arr,
                                    uint16_t initial, const uint8_t *h_addrs,
                                    uint16_t *h_out, const int *devices,
                                    int ndev);
int yu_csum_batch_host_iov_multi(const yu_iovec *iov, const uint64_t *first_iov,
                                 uint64_t n, int mode,
                                 const uint16_t *h_initial_arr,
                                 uint16_t initial, const uint8_t *h_addrs,
                                 uint16_t *h_out, const int *devices, int ndev);

/* ------------------------------------------------------------------ */
/* Host-path staging (the yu_csum_batch_host_* / yu_csum_fill_host_*   */
/* calls, and each shard of the _multi forms).                          */
/* ------------------------------------------------------------------ */

/* A host call borrows one staging context of its device for its own length
 * and returns it; a caller that finds every context in use waits for one.
 * There are two pools per device: bulk contexts (3 pipeline slots) and burst
 * contexts (1 slot) for the calls that take the direct path (one slice of at
 * most 4 MiB: a tun read burst), so a burst never waits behind bulk batches
 * that hold every bulk context. Contexts are created on first need, up to
 * yu_host_contexts() per pool and device: YU_HOST_CONTEXTS in the environment
 * (1..64, default 4; a product setting, read without the YU_TUNING gate). So
 * the staging grows with the calls the pools let run at once, not with the
 * number of OS threads that ever called (the Go consumer calls from many
 * goroutines, which migrate across OS threads: transport/tcp/accept.go:238,
 * transport/tcp/endpoint.go:229, network/ipv4/icmp.go:30-34).
 *
 * A bulk context holds 3 pipeline slots of at most one slice each: up to
 * YU_HOST_SLICE_BYTES of packet bytes and YU_HOST_SLICE_PACKETS packets'
 * side arrays; a burst context one slot of at most 4 MiB and as many
 * packets. Between calls a device's staging is therefore at most
 * yu_host_contexts() * (YU_HOST_CONTEXT_PINNED_MAX +
 * YU_HOST_BURST_CONTEXT_PINNED_MAX) bytes of pinned host memory and
 * yu_host_contexts() * (YU_HOST_CONTEXT_DEVICE_MAX +
 * YU_HOST_BURST_CONTEXT_DEVICE_MAX) of device memory (a packet longer than a
 * slice gets a slice of its own for that call; the context gives the extra
 * back when the call returns). */
#define YU_HOST_SLICE_BYTES (32ull << 20)
#define YU_HOST_SLICE_PACKETS (1ull << 18)
#define YU_HOST_CONTEXT_PINNED_MAX \
  (3ull * (YU_HOST_SLICE_BYTES + 26ull * YU_HOST_SLICE_PACKETS + 72ull))
#define YU_HOST_CONTEXT_DEVICE_MAX \
  (3ull * (YU_HOST_SLICE_BYTES + 22ull * YU_HOST_SLICE_PACKETS + 8ull))
#define YU_HOST_BURST_CONTEXT_PINNED_MAX \
  ((4ull << 20) + 26ull * YU_HOST_SLICE_PACKETS + 72ull)
#define YU_HOST_BURST_CONTEXT_DEVICE_MAX \
  ((4ull << 20) + 22ull * YU_HOST_SLICE_PACKETS + 8ull)

/* The pool bound K (YU_HOST_CONTEXTS, clamped to 1..64), per pool. */
int yu_host_contexts(void);
/* Pinned host bytes the host-path staging of `device` holds now (idle and
 * lent contexts); the device bytes go to *dev_bytes when it is not NULL.
 * 0 for a device never used or out of range. Never fails. */
uint64_t yu_host_staging_bytes(int device, uint64_t *dev_bytes);
/* Frees the staging of every idle context of `device` (a later call
 * allocates again). YU_ENODEV for a device out of range. */
int yu_host_staging_trim(int device);

/* ------------------------------------------------------------------ */
/* Introspection.                                                      */
/* ------------------------------------------------------------------ */
int yu_abi_version(void);
const char *yu_strerror(int status);
/* Number of HIP devices (0 when none / no driver). Never fails. */
int yu_device_count(void);
/* Path of the HIP runtime (libamdhip64) this library's HIP calls are bound
 * to, as the dynamic loader resolved them (dladdr of the library's own
 * reference to hipGetDevice); NULL if it cannot be told. No device needed.
 * A process with two HIP runtimes (PyTorch-ROCm bundles one) must have this
 * library bound to the runtime the rest of the process uses: the Python
 * loader checks it ("One HIP runtime per process"). */
const char *yu_hip_runtime_path(void);
/* Name of the kernel variant the uniform path would launch for this shape
 * (for profiling and tests; no device needed). Returns a static string. */
const char *yu_uniform_variant(uint64_t stride, uint32_t len, int mode,
                               uint64_t data_align16);
/* The same for a batch of n packets (the choice above 3 KiB depends on n;
 * yu_uniform_variant answers for n = 2). */
const char *yu_uniform_variant_n(uint64_t stride, uint32_t len, uint64_t n,
                                 int mode, uint64_t data_align16);
/* Name of the kernel variant the ragged path launches for this mode (static
 * string; "" for a bad mode), for a large batch; _n: for a batch of n
 * packets (bursts of up to 4096 packets take a wave per packet). */
const char *yu_ragged_variant(int mode);
const char *yu_ragged_variant_n(int mode, uint64_t n);
/* The kernel variant yu_csum_fill_ragged launches for a batch of n packets (the
 * TX modes write in place through their own k_seg form). */
const char *yu_ragged_fill_variant_n(int mode, uint64_t n);
/* The kernel variant the scatter-gather device calls launch for a batch of n
 * packets (fill != 0: yu_csum_fill_iov); "" for a mode the form refuses. No
 * device needed. */
const char *yu_iov_variant_n(int mode, uint64_t n, int fill);
/* The same for the whole-datagram calls (fill != 0: yu_csum_fill_iov_datagram). */
const char *yu_iov_datagram_variant_n(int mode, uint64_t n, int fill);
/* The same for the packing calls (fill != 0: yu_csum_pack_fill_iov). */
const char *yu_iov_pack_variant_n(int mode, uint64_t n, int fill);
/* The same for the packing whole-datagram calls (fill != 0:
 * yu_csum_pack_fill_iov_datagram). */
const char *yu_iov_pack_datagram_variant_n(int mode, uint64_t n, int fill);
/* The kernel variant yu_tx_build_ragged launches for a batch of n packets. No
 * device needed. */
const char *yu_tx_build_variant_n(uint64_t n);
/* The same for yu_rx_split_ragged. */
const char *yu_rx_split_variant_n(uint64_t n);
/* The header pass of yu_rx_parse_ragged ("k_parse"). No device needed. */
const char *yu_rx_parse_variant_n(uint64_t n);
/* The kernel of yu_rx_demux ("k_demux"). No device needed. */
const char *yu_rx_demux_variant_n(uint64_t n);
/* The partition of yu_rx_group by its pass count: "k_group<1>" (m <= 255) ..
 * "k_group<4>" (m == 2^24); "none" where yu_rx_group_workspace_bytes is 0. No
 * device needed. */
const char *yu_rx_group_variant_n(uint64_t n, uint64_t m);
/* The kernel of yu_rx_reply ("k_reply"). No device needed. */
const char *yu_rx_reply_variant_n(uint64_t n);
/* The kernel of yu_rx_stream ("k_stream"; "k_stream<walk>" where the tuning value
 * YU_STREAM=walk forces the general step for every entry); "none" where
 * yu_rx_stream_workspace_bytes is 0. No device needed. */
const char *yu_rx_stream_variant_n(uint64_t n, uint64_t m, uint32_t cap);
/* The kernel of yu_tx_build_iov ("k_build<4,iov>"). No device needed. */
const char *yu_tx_build_iov_variant_n(uint64_t n);

#ifdef __cplusplus
}
#endif

#endif /* YUCSUM_H */
