"""The reference's transport demultiplexer restated for the tests of yu_rx_demux:
restated, not executed (the Go-subset interpreter of tests/golden/goexec.py has no maps).
One dict per protocol, keyed by the TransportEndpointId ``(local_port, local_addr | None,
remote_port, remote_addr | None)`` with None for Go's empty Address; the three ``dict.get``
calls of deliverPacketLocked in their order; and the gate of DeliverTransportPacket (a
transport protocol exists for TCP and UDP only) with the receiver's choice of flag bits in
front of it. A plain module, like rxgen.py."""
import numpy as np

NONE = 0xFFFFFFFF  # YU_DEMUX_NONE
RX_SPLIT = 16      # YU_RX_SPLIT


class Demuxer:
    """``ids``: an array of packets.ENDPOINT_ID; an endpoint's number is its position."""

    def __init__(self, ids):
        self.protocol_ids = {6: {}, 17: {}}
        self.m = len(ids)
        for number, e in enumerate(ids):
            kind = int(e["kind"])
            key = (int(e["local_port"]), None if kind == 2 else bytes(e["local_addr"]),
                   int(e["remote_port"]) if kind == 0 else 0, bytes(e["remote_addr"]) if kind == 0 else None)
            eps = self.protocol_ids[int(e["proto"])]
            if key in eps:
                raise ValueError(f"id {number}: port in use")
            eps[key] = number

    def deliver_packet_locked(self, proto, local_port, local_addr, remote_port, remote_addr):
        eps = self.protocol_ids[proto]
        ep = eps.get((local_port, local_addr, remote_port, remote_addr))  # the full id
        if ep is None:
            ep = eps.get((local_port, local_addr, 0, None))               # the remote part emptied
        if ep is None:
            ep = eps.get((local_port, None, 0, None))                     # the local address emptied as well
        return NONE if ep is None else ep

    def deliver_transport_packet(self, rec, flags=None, need=0):
        """``rec``: one packets.TX_RECORD entry of a received packet (its dst is local)."""
        proto = int(rec["proto"])
        if proto not in self.protocol_ids:
            return NONE
        if flags is not None and (int(flags) & (need | RX_SPLIT)) != (need | RX_SPLIT):
            return NONE
        return self.deliver_packet_locked(proto, int(rec["dport"]), bytes(rec["dst"]), int(rec["sport"]),
                                          bytes(rec["src"]))


def demux(ids, recs, flags=None, need=0):
    """(ep, counts) as yu_rx_demux gives them on zeroed counters: uint32 arrays of
    len(recs) and len(ids) + 1 entries."""
    d = Demuxer(ids)
    ep = np.array([d.deliver_transport_packet(r, None if flags is None else flags[i], need)
                   for i, r in enumerate(recs)], dtype=np.uint32).reshape(len(recs))
    counts = np.bincount(np.where(ep == NONE, d.m, ep).astype(np.int64), minlength=d.m + 1).astype(np.uint32)
    return ep, counts
