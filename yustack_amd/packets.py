"""Scalar packet composition, mirroring the reference's send paths call for call.

These are the compositions the batched TX modes reproduce on the GPU; they run on
the host through the scalar C ABI, like the reference runs them per packet:

* :func:`send_udp`    transport/udp/endpoint.go:164-187 (sendUDP) + network/ipv4/ipv4.go:80-97
* :func:`send_tcp`    transport/tcp/connect.go:556-586 (sendTCP), :288-322 (with options)
* :func:`send_icmpv4` network/ipv4/icmp.go:36-45 (sendICMPv4)
* :func:`ipv4_write`  network/ipv4/ipv4.go:80-97 (endpoint.WritePacket)

and the test harnesses' inbound builders:

* :func:`tcp_test_packet` transport/tcp/testing/context/context.go:164-209 (SendPacket)
* :func:`udp_test_packet` transport/udp/udp_test.go:105-144 (sendPacket)

and the record layout of the device-side sender, ``batch.build_datagrams``:

* :data:`TX_RECORD`, :func:`tx_records`  struct yu_tx_record (include/yucsum.h)

which is also what the device-side receiver, ``batch.split_datagrams``, fills in:

* :data:`RX_SPLIT`, :func:`rx_records`   YU_RX_SPLIT and the records as ``TX_RECORD``

and the registered ids of the device-side demultiplexer, ``batch.demux_table``:

* :data:`ENDPOINT_ID`, :func:`endpoint_ids`  struct yu_endpoint_id (include/yucsum.h)
"""
from __future__ import annotations

import numpy as np

from .checksum import Checksum
from .header import (ICMPv4, ICMPv4MinimumSize, IPv4, IPv4MinimumSize, Route, TCP, TCPMinimumSize,
                     TCPProtocolNumber, UDP, UDPMinimumSize, UDPProtocolNumber, ICMPv4ProtocolNumber)


def ipv4_write(r: Route, transport_hdr: bytes, payload: bytes, protocol: int) -> bytearray:
    """network/ipv4/ipv4.go:80-97: prepend the IPv4 header (IHL 20, TTL 64, ID 0) and
    set its checksum."""
    b = bytearray(IPv4MinimumSize) + bytearray(transport_hdr) + bytearray(payload)
    ip = IPv4(b)
    ip.Encode(IHL=IPv4MinimumSize, TotalLength=len(b), ID=0, TTL=64, Protocol=protocol,
              SrcAddr=r.LocalAddress, DstAddr=r.RemoteAddress)
    ip.SetChecksum(~ip.CalculateChecksum() & 0xFFFF)
    return b


def send_udp(r: Route, data: bytes | None, local_port: int, remote_port: int) -> bytearray:
    """transport/udp/endpoint.go:164-187"""
    hdr = bytearray(UDPMinimumSize)
    udp = UDP(hdr)
    length = UDPMinimumSize
    xsum = r.PseudoHeaderChecksum(UDPProtocolNumber)
    if data is not None:
        length = (length + len(data)) & 0xFFFF
        xsum = Checksum(data, xsum)
    udp.Encode(SrcPort=local_port, DstPort=remote_port, Length=length)
    udp.SetChecksum(~udp.CalculateChecksum(xsum, length) & 0xFFFF)
    return ipv4_write(r, bytes(hdr), data or b"", UDPProtocolNumber)


def send_tcp(r: Route, local_port: int, remote_port: int, data: bytes | None, flags: int,
             seq: int, ack: int, rcv_wnd: int, options: bytes = b"") -> bytearray:
    """transport/tcp/connect.go:556-586 (options form: :288-322)"""
    hdr = bytearray(TCPMinimumSize + len(options))
    hdr[TCPMinimumSize:] = options
    rcv_wnd = min(rcv_wnd, 0xFFFF)
    tcp = TCP(hdr)
    tcp.Encode(SrcPort=local_port, DstPort=remote_port, SeqNum=seq, AckNum=ack,
               DataOffset=TCPMinimumSize + len(options), Flags=flags, WindowSize=rcv_wnd)
    length = len(hdr)
    xsum = r.PseudoHeaderChecksum(TCPProtocolNumber)
    if data is not None:
        length = (length + len(data)) & 0xFFFF
        xsum = Checksum(data, xsum)
    tcp.SetChecksum(~tcp.CalculateChecksum(xsum, length) & 0xFFFF)
    return ipv4_write(r, bytes(hdr), data or b"", TCPProtocolNumber)


def send_icmpv4(r: Route, typ: int, code: int, data: bytes) -> bytearray:
    """network/ipv4/icmp.go:36-45"""
    hdr = bytearray(ICMPv4MinimumSize)
    icmp = ICMPv4(hdr)
    icmp.SetType(typ)
    icmp.SetCode(code)
    icmp.SetChecksum(~Checksum(bytes(hdr), Checksum(data, 0)) & 0xFFFF)
    return ipv4_write(r, bytes(hdr), data, ICMPv4ProtocolNumber)


def tcp_test_packet(payload: bytes, src_port: int, dst_port: int, seq: int, ack: int, flags: int,
                    rcv_wnd: int, tcp_opts: bytes = b"",
                    test_addr: bytes = b"\x0a\x00\x00\x02",
                    stack_addr: bytes = b"\x0a\x00\x00\x01") -> bytearray:
    """transport/tcp/testing/context/context.go:164-209 (Context.SendPacket)"""
    buf = bytearray(TCPMinimumSize + IPv4MinimumSize + len(tcp_opts) + len(payload))
    buf[len(buf) - len(payload):] = payload
    buf[len(buf) - len(payload) - len(tcp_opts): len(buf) - len(payload)] = tcp_opts
    ip = IPv4(buf)
    ip.Encode(IHL=IPv4MinimumSize, TotalLength=len(buf), TTL=64, Protocol=TCPProtocolNumber,
              SrcAddr=test_addr, DstAddr=stack_addr)
    ip.SetChecksum(~ip.CalculateChecksum() & 0xFFFF)
    t = TCP(buf, IPv4MinimumSize)
    t.Encode(SrcPort=src_port, DstPort=dst_port, SeqNum=seq, AckNum=ack,
             DataOffset=TCPMinimumSize + len(tcp_opts), Flags=flags, WindowSize=rcv_wnd & 0xFFFF)
    xsum = Checksum(test_addr, 0)
    xsum = Checksum(stack_addr, xsum)
    xsum = Checksum(bytes([0, TCPProtocolNumber]), xsum)
    length = TCPMinimumSize + len(tcp_opts) + len(payload)
    xsum = Checksum(payload, xsum)
    t.SetChecksum(~t.CalculateChecksum(xsum, length) & 0xFFFF)
    return buf


def udp_test_packet(payload: bytes, src_port: int, dst_port: int,
                    test_addr: bytes = b"\x0a\x01\x00\x01",
                    stack_addr: bytes = b"\x0a\x01\x00\x02") -> bytearray:
    """transport/udp/udp_test.go:105-144 (testContext.sendPacket)"""
    buf = bytearray(UDPMinimumSize + IPv4MinimumSize + len(payload))
    buf[len(buf) - len(payload):] = payload
    ip = IPv4(buf)
    ip.Encode(IHL=IPv4MinimumSize, TotalLength=len(buf), TTL=64, Protocol=UDPProtocolNumber,
              SrcAddr=test_addr, DstAddr=stack_addr)
    ip.SetChecksum(~ip.CalculateChecksum() & 0xFFFF)
    u = UDP(buf, IPv4MinimumSize)
    u.Encode(SrcPort=src_port, DstPort=dst_port, Length=UDPMinimumSize + len(payload))
    xsum = Checksum(test_addr, 0)
    xsum = Checksum(stack_addr, xsum)
    xsum = Checksum(bytes([0, UDPProtocolNumber]), xsum)
    length = UDPMinimumSize + len(payload)
    xsum = Checksum(payload, xsum)
    u.SetChecksum(~u.CalculateChecksum(xsum, length) & 0xFFFF)
    return buf


# struct yu_tx_record (include/yucsum.h): one outgoing datagram's header fields for
# batch.build_datagrams. Numbers in host byte order, addresses as wire bytes.
TX_RECORD = np.dtype([("src", np.uint8, (4,)), ("dst", np.uint8, (4,)), ("sport", np.uint16), ("dport", np.uint16),
                      ("seq", np.uint32), ("ack", np.uint32), ("window", np.uint16), ("flags", np.uint8),
                      ("doff", np.uint8), ("proto", np.uint8), ("ttl", np.uint8), ("ip_id", np.uint16),
                      ("tos", np.uint8), ("reserved", np.uint8), ("frag", np.uint16)])
assert TX_RECORD.itemsize == 32


def tx_records(n: int, *, src=0, dst=0, sport=0, dport=0, seq=0, ack=0, window=0, flags=0, doff=20, proto=17,
               ttl=64, ip_id=0, tos=0, frag=0) -> np.ndarray:
    """n records of :data:`TX_RECORD`, each field from an array of n values or a scalar
    broadcast over the batch (``src`` / ``dst``: (n, 4) or (4,) wire bytes, or one
    address as a big-endian number). The defaults are WritePacket's
    (network/ipv4/ipv4.go:80-97): TTL 64, ID 0, TOS 0, no fragment word; ``doff`` 20 is
    a TCP header without options. ICMP: ``sport`` is ``type << 8 | code``. Upload with
    ``torch.from_numpy(recs.view(np.uint8).reshape(n, 32))``."""
    recs = np.zeros(n, dtype=TX_RECORD)
    for name, a in (("src", src), ("dst", dst)):
        a = np.asarray(a)
        if a.ndim == 0:  # 0x0A000001 is 10.0.0.1
            a = np.array([(int(a) >> s) & 0xFF for s in (24, 16, 8, 0)], dtype=np.uint8)
        recs[name] = np.broadcast_to(a, (n, 4))
    for name, a in (("sport", sport), ("dport", dport), ("seq", seq), ("ack", ack), ("window", window),
                    ("flags", flags), ("doff", doff), ("proto", proto), ("ttl", ttl), ("ip_id", ip_id),
                    ("tos", tos), ("frag", frag)):
        recs[name] = np.broadcast_to(np.asarray(a), (n,))
    return recs


# struct yu_endpoint_id (include/yucsum.h): one registered TransportEndpointId plus its
# protocol for batch.demux_table. Ports in host byte order, addresses as wire bytes.
ENDPOINT_ID = np.dtype([("local_addr", np.uint8, (4,)), ("remote_addr", np.uint8, (4,)), ("local_port", np.uint16),
                        ("remote_port", np.uint16), ("proto", np.uint8), ("kind", np.uint8), ("reserved", np.uint16)])
assert ENDPOINT_ID.itemsize == 16


def endpoint_ids(m: int, *, local_addr=0, remote_addr=0, local_port=0, remote_port=0, proto=6, kind=0) -> np.ndarray:
    """m ids of :data:`ENDPOINT_ID`, each field from an array of m values or a scalar
    broadcast over them (addresses as for :func:`tx_records`). ``kind`` 0 is a connection
    (all four fields), 1 a listener on an address (``remote_addr`` and ``remote_port``
    must be zero), 2 a listener on a port (``local_addr`` zero as well); nothing is
    zeroed here, ``batch.demux_table`` refuses an id whose emptied fields are not zero.
    An endpoint's number is its position in the array."""
    ids = np.zeros(m, dtype=ENDPOINT_ID)
    for name, a in (("local_addr", local_addr), ("remote_addr", remote_addr)):
        a = np.asarray(a)
        if a.ndim == 0:
            a = np.array([(int(a) >> s) & 0xFF for s in (24, 16, 8, 0)], dtype=np.uint8)
        ids[name] = np.broadcast_to(a, (m, 4))
    for name, a in (("local_port", local_port), ("remote_port", remote_port), ("proto", proto), ("kind", kind)):
        ids[name] = np.broadcast_to(np.asarray(a), (m,))
    return ids


# struct yu_tcp_rcv and struct yu_tcp_seg (include/yucsum.h): the per-connection receiver
# state and one pending segment of batch.stream_datagrams.
TCP_RCV = np.dtype([("rcv_nxt", np.uint32), ("rcv_acc", np.uint32), ("pend_used", np.uint32),
                    ("pend_size", np.uint32), ("buf_size", np.uint32), ("buf_used", np.uint32),
                    ("snd_nxt", np.uint32), ("max_sent_ack", np.uint32), ("pend_count", np.uint32),
                    ("wnd_scale", np.uint8), ("state", np.uint8), ("reserved", np.uint16)])
TCP_SEG = np.dtype([("base", np.uint64), ("len", np.uint64), ("seq", np.uint32), ("pkt", np.uint32),
                    ("flags", np.uint8), ("reserved", np.uint8, (7,))])
assert TCP_RCV.itemsize == 40 and TCP_SEG.itemsize == 32


def tcp_rcv(m: int, *, rcv_nxt=0, wnd=65535, snd_nxt=0, wnd_scale=0, state=1) -> np.ndarray:
    """m receivers of :data:`TCP_RCV` as newReceiver leaves them (transport/tcp/rcv.go:32-40):
    ``rcv_acc = rcv_nxt + wnd``, ``pend_size = buf_size = wnd``, nothing pending, nothing
    buffered, ``max_sent_ack = rcv_nxt``; each argument an array of m values or a scalar.
    ``state`` 0 marks an endpoint the stream call does not serve (UDP, a listener)."""
    st = np.zeros(m, dtype=TCP_RCV)
    nxt = np.broadcast_to(np.asarray(rcv_nxt, dtype=np.uint32), (m,))
    w = np.broadcast_to(np.asarray(wnd, dtype=np.uint32), (m,))
    st["rcv_nxt"], st["rcv_acc"], st["max_sent_ack"] = nxt, nxt + w, nxt
    st["pend_size"], st["buf_size"] = w, w
    st["snd_nxt"] = np.broadcast_to(np.asarray(snd_nxt, dtype=np.uint32), (m,))
    st["wnd_scale"] = np.broadcast_to(np.asarray(wnd_scale, dtype=np.uint8), (m,))
    st["state"] = np.broadcast_to(np.asarray(state, dtype=np.uint8), (m,))
    return st


# YU_RX_SPLIT (include/yucsum.h): the bit batch.split_datagrams adds to VERIFY_RX's flags
# when a packet's record, pay_len and payload are defined.
RX_SPLIT = 16


def rx_records(records) -> np.ndarray:
    """The ``records`` tensor of ``batch.split_datagrams`` (shape (n, 32) uint8, on any
    device) as a host array of n :data:`TX_RECORD` entries; a packet without
    :data:`RX_SPLIT` has an all-zero record."""
    raw = records.cpu().numpy() if hasattr(records, "cpu") else np.asarray(records)
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if raw.ndim != 2 or raw.shape[1] != TX_RECORD.itemsize:
        raise ValueError("records must have shape (n, 32)")
    return raw.view(TX_RECORD).reshape(raw.shape[0])
