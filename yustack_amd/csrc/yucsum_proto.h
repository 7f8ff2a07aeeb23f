// yucsum_proto.h — the protocol tables used by the kernels and by the host-side
// field writer (yucsum_hostgeom.h), so the two cannot disagree on which bytes a
// mode owns. No HIP call and no HIP header: a plain C++ compiler takes it too.
#ifndef YUCSUM_PROTO_H
#define YUCSUM_PROTO_H

#include <stdint.h>

#include "yucsum.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YU_PROTO_FN __host__ __device__ inline
#else
#define YU_PROTO_FN inline
#endif

namespace yu {

// Offset of the checksum field a single-field TX mode takes as zero
// (header/udp.go udpChecksum=6, header/tcp.go tcpChecksum=16,
//  header/ipv4.go ipChecksum=10, header/icmpv4.go checksum at 2); 0 otherwise.
YU_PROTO_FN uint32_t mode_field(int m) {
  switch (m) {
    case YU_MODE_UDP: return 6;
    case YU_MODE_TCP: return 16;
    case YU_MODE_IPV4: return 10;
    case YU_MODE_ICMP: return 2;
    default: return 0;
  }
}
YU_PROTO_FN bool mode_is_tx(int m) {
  return m == YU_MODE_UDP || m == YU_MODE_TCP || m == YU_MODE_IPV4 || m == YU_MODE_ICMP;
}
// Modes that may write in place (the single-field TX modes and TX_DATAGRAM).
YU_PROTO_FN bool mode_fills(int m) {
  return mode_is_tx(m) || m == YU_MODE_TX_DATAGRAM;
}
// Offset of the transport checksum field in a segment of IPv4 protocol
// `proto`, and the segment's minimum length (UDP 6/8, TCP 16/20, ICMP 2/4);
// 0 / 0 for other protocols.
YU_PROTO_FN uint32_t l4_field(uint32_t proto) {
  return proto == 17u ? 6u : (proto == 6u ? 16u : (proto == 1u ? 2u : 0u));
}
YU_PROTO_FN uint32_t l4_min(uint32_t proto) {
  return proto == 17u ? 8u : (proto == 6u ? 20u : (proto == 1u ? 4u : 0u));
}

}  // namespace yu

#endif  // YUCSUM_PROTO_H
