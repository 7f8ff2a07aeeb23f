"""Batched Internet checksum on MI355X — the hot path.

Thin Python front end over the C ABI's batched entry points
(``yu_csum_batch_uniform`` / ``yu_csum_batch_ragged`` / ``yu_csum_batch_iov`` /
``yu_csum_batch_iov_datagram`` / ``yu_csum_pack_iov`` / ``yu_csum_pack_iov_datagram`` / ``yu_csum_fill_*`` /
``yu_tx_build_ragged`` / ``yu_rx_split_ragged`` / ``yu_rx_parse_ragged`` / ``yu_rx_demux`` /
``yu_rx_group`` / ``yu_csum_batch_host_uniform``,
include/yucsum.h). PyTorch is used only for device
memory and streams: the arithmetic happens in the hand-written gfx950 kernels of
``csrc/yucsum_kernels.hip``. There is no CPU fallback — without a HIP device every
entry point raises :class:`yustack_amd._lib.YuError`.

Modes (each reproduces one reference composition, see include/yucsum.h):

=============  =========================================================================
RAW            ``Checksum(pkt, initial)``                     checksum/checksum.go:4-18
UDP            field value of sendUDP                          transport/udp/endpoint.go:164-187
TCP            field value of sendTCP                          transport/tcp/connect.go:556-586
IPV4           field value of ipv4 WritePacket                 network/ipv4/ipv4.go:80-97
ICMP           field value of sendICMPv4                       network/ipv4/icmp.go:36-45
VERIFY_IPV4    checker.IPv4 sum (valid iff 0 or 0xFFFF)        checker/checker.go:25-40
VERIFY_TCP     checker.TCP sum                                 checker/checker.go:71-99
VERIFY_UDP     the checker.TCP formula for UDP
VERIFY_RX      whole received IPv4 packets: IsValid + checker.IPv4 + checker.TCP's
               test, inputs read from each packet; out = YU_RX_* bits
                                                               checker/checker.go:25-99
TX_DATAGRAM    whole outgoing IPv4 datagrams: both fields (IPv4 header and its
               sender's transport field), inputs read from each datagram; TWO
               results per packet, out[2i] / out[2i+1]     network/ipv4/ipv4.go:80-97
=============  =========================================================================
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._lib import YU_EINVAL, check, lib
from .packets import ENDPOINT_ID

RAW, UDP, TCP, IPV4, ICMP, VERIFY_IPV4, VERIFY_TCP, VERIFY_UDP, VERIFY_RX, TX_DATAGRAM = range(10)
MODES = {"raw": RAW, "udp": UDP, "tcp": TCP, "ipv4": IPV4, "icmp": ICMP,
         "verify_ipv4": VERIFY_IPV4, "verify_tcp": VERIFY_TCP, "verify_udp": VERIFY_UDP,
         "verify_rx": VERIFY_RX, "tx_datagram": TX_DATAGRAM}
# VERIFY_RX result bits (include/yucsum.h YU_RX_*)
RX_IP_OK, RX_L4, RX_L4_OK, RX_INVALID = 1, 2, 4, 8
RX_SPLIT = 16  # split_datagrams only (YU_RX_SPLIT): the packet's record, pay_len and payload are defined
TX_MODES = (UDP, TCP, IPV4, ICMP, TX_DATAGRAM)
MAX_TRANSPORT_LEN = 65535
MAX_RAW_LEN = 0xFFFF0000  # include/yucsum.h YU_MAX_RAW_LEN


def _mode(m) -> int:
    m = MODES[m] if isinstance(m, str) else int(m)
    if not 0 <= m < len(MODES):
        raise ValueError(f"bad mode {m}")
    return m


def outputs(mode) -> int:
    """Results per packet (include/yucsum.h YU_MODE_OUTPUTS): 2 for TX_DATAGRAM."""
    return 2 if _mode(mode) == TX_DATAGRAM else 1


def _dev_u8(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA (HIP) tensor")
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous uint8 tensor")
    return t


def _opt(t, dtype, numel, device, name):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
        raise TypeError(f"{name} must be a CUDA tensor on {device}")
    if t.dtype != dtype or not t.is_contiguous() or t.numel() < numel:
        raise TypeError(f"{name} must be a contiguous {dtype} tensor with >= {numel} elements")
    return t


def _result(out, count: int, device) -> torch.Tensor:
    """The uint16 result tensor of ``count`` entries: ``out`` checked, or a new one."""
    if out is None:
        return torch.empty(max(count, 1), dtype=torch.uint16, device=device)[:count]
    return _opt(out, torch.uint16, count, device, "out")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(device, stream):
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return s.cuda_stream


def checksum_uniform(data: torch.Tensor, stride: int, length: int, n: int, mode="raw", *,
                     initial: int = 0, initial_arr: torch.Tensor | None = None,
                     addrs: torch.Tensor | None = None, out: torch.Tensor | None = None,
                     stream: torch.cuda.Stream | None = None, fill: bool = False) -> torch.Tensor:
    """Per-packet sums of a uniform-stride device batch: packet i is
    ``data[i*stride : i*stride+length]``. Returns a uint16 tensor of n results (2n for TX_DATAGRAM)
    (allocated unless ``out`` is given). ``fill=True`` additionally stores each TX
    result big-endian into the packet's checksum field (in place)."""
    m = _mode(mode)
    _dev_u8(data, "data")
    if n < 0 or stride < 0 or not 0 <= length < 2 ** 32:
        raise ValueError("bad geometry")
    if n and (n - 1) * stride + length > data.numel():
        raise ValueError(f"batch needs {(n - 1) * stride + length} bytes, data has {data.numel()}")
    dev = data.device
    initial_arr = _opt(initial_arr, torch.uint16, n, dev, "initial_arr")
    addrs = _opt(addrs, torch.uint8, 8 * n, dev, "addrs")
    out = _result(out, n * outputs(m), dev)
    with torch.cuda.device(dev):
        f = lib().yu_csum_fill_uniform if fill else lib().yu_csum_batch_uniform
        rc = f(data.data_ptr(), stride, length, n, m, _ptr(initial_arr), initial & 0xFFFF,
               _ptr(addrs), out.data_ptr() if n else None, _stream(dev, stream))
    check(rc, "yu_csum_fill_uniform" if fill else "yu_csum_batch_uniform")
    return out


def checksum_ragged(data: torch.Tensor, offsets: torch.Tensor, mode="raw", *, initial: int = 0,
                    initial_arr: torch.Tensor | None = None, addrs: torch.Tensor | None = None,
                    out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None,
                    fill: bool = False, validate: bool = True) -> torch.Tensor:
    """Per-packet sums of a ragged device batch: packet i is
    ``data[offsets[i] : offsets[i+1]]`` (offsets: n+1 non-decreasing int64/uint64).
    ``validate`` checks the offsets against ``data`` on the device before launching
    (one small synchronisation); pass False only for offsets validated earlier."""
    m = _mode(mode)
    _dev_u8(data, "data")
    if not isinstance(offsets, torch.Tensor) or not offsets.is_cuda or offsets.device != data.device:
        raise TypeError("offsets must be a CUDA tensor on data's device")
    if offsets.dtype not in (torch.int64, torch.uint64) or not offsets.is_contiguous() or offsets.dim() != 1:
        raise TypeError("offsets must be a contiguous 1-D int64/uint64 tensor")
    n = offsets.numel() - 1
    if n < 0:
        raise ValueError("offsets must hold n+1 entries")
    if validate and n > 0:
        o = offsets.view(torch.int64)
        ok = bool(((o[1:] >= o[:-1]).all() & (o[0] >= 0) & (o[-1] <= data.numel())).item())
        if not ok:
            raise ValueError("offsets are not non-decreasing within data")
        cap = MAX_TRANSPORT_LEN if m != RAW else MAX_RAW_LEN
        if bool(((o[1:] - o[:-1]) > cap).any().item()):
            raise ValueError("transport/IPv4/ICMP packets must be <= 65535 bytes" if m != RAW
                             else f"RAW packets must be <= {MAX_RAW_LEN} bytes")
    dev = data.device
    initial_arr = _opt(initial_arr, torch.uint16, n, dev, "initial_arr")
    addrs = _opt(addrs, torch.uint8, 8 * n, dev, "addrs")
    out = _result(out, n * outputs(m), dev)
    with torch.cuda.device(dev):
        f = lib().yu_csum_fill_ragged if fill else lib().yu_csum_batch_ragged
        rc = f(data.data_ptr(), offsets.data_ptr(), n, m, _ptr(initial_arr), initial & 0xFFFF,
               _ptr(addrs), out.data_ptr() if n else None, _stream(dev, stream))
    check(rc, "yu_csum_fill_ragged" if fill else "yu_csum_batch_ragged")
    return out


IOV_MODES = (RAW, UDP, TCP, ICMP, VERIFY_TCP, VERIFY_UDP)
IOV_FILL_MODES = (UDP, TCP, ICMP)


def _dev_index(t, name: str, device, numel: int | None = None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
        raise TypeError(f"{name} must be a CUDA tensor on {device}")
    if t.dtype not in (torch.int32, torch.int64, torch.uint64) or t.dim() != 1:
        raise TypeError(f"{name} must be a 1-D int32/int64/uint64 tensor")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name} must hold {numel} entries")
    return (t.view(torch.int64) if t.dtype == torch.uint64 else t.to(torch.int64)).contiguous()


def _iov_table(pools, view_pool, view_off, view_len, first, validate: bool):
    """The device ``yu_iovec`` table of the scatter-gather calls, built with torch
    operations, and the checks ``validate`` asks for. Returns (device, table, first
    as int64, n)."""
    pools = list(pools)
    if not pools:
        raise ValueError("pools must hold at least one tensor")
    for k, pool in enumerate(pools):
        _dev_u8(pool, f"pools[{k}]")
    dev = pools[0].device
    if any(pool.device != dev for pool in pools):
        raise TypeError("pools must be on one device")
    vp = _dev_index(view_pool, "view_pool", dev)
    nviews = vp.numel()
    vo = _dev_index(view_off, "view_off", dev, nviews)
    vl = _dev_index(view_len, "view_len", dev, nviews)
    fi = _dev_index(first, "first", dev)
    n = fi.numel() - 1
    if n < 0:
        raise ValueError("first must hold n+1 entries")
    # base = pools[k].data_ptr() + off: one pass per pool, none per view
    base = torch.zeros_like(vo)
    size = torch.zeros_like(vo)
    for k, pool in enumerate(pools):
        sel = vp == k
        base = torch.where(sel, vo + pool.data_ptr(), base)
        size = torch.where(sel, torch.full_like(vo, pool.numel()), size)
    if validate and n > 0:
        ends = torch.zeros(nviews + 1, dtype=torch.int64, device=dev)
        ends[1:] = torch.cumsum(vl.clamp(min=0), 0)
        ok_first = (fi[1:] >= fi[:-1]).all() & (fi[0] >= 0) & (fi[-1] <= nviews)
        ok_view = ((vp >= 0) & (vp < len(pools)) & (vo >= 0) & (vl >= 0) & (vl <= size) &
                   (vo <= size - vl)).all()
        f = fi.clamp(0, nviews)
        ok_len = ((ends[f[1:]] - ends[f[:-1]]) <= MAX_TRANSPORT_LEN).all()
        okf, okv, okl = torch.stack((ok_first, ok_view, ok_len)).tolist()
        if not okf:
            raise ValueError("first is not non-decreasing within the view count")
        if not okv:
            raise ValueError("a view does not lie inside its pool")
        if not okl:
            raise ValueError("scatter-gather packets must be <= 65535 bytes")
    table = torch.stack((base, vl), dim=1).contiguous() if nviews else \
        torch.zeros((1, 2), dtype=torch.int64, device=dev)
    return dev, table, fi, n


IOV_DATAGRAM_MODES = (IPV4, VERIFY_IPV4, VERIFY_RX, TX_DATAGRAM)
IOV_DATAGRAM_FILL_MODES = (IPV4, TX_DATAGRAM)


def _iov_admit(who: str, m: int, datagram: bool, fill: bool) -> None:
    """The modes a scatter-gather function takes: the whole-packet ones, or the
    whole-datagram ones; with ``fill`` those of them that have a field to store."""
    if datagram:
        if m not in IOV_DATAGRAM_MODES:
            raise ValueError(f"{who} takes ipv4, verify_ipv4, verify_rx and tx_datagram")
        if fill and m not in IOV_DATAGRAM_FILL_MODES:
            raise ValueError("fill=True takes ipv4 or tx_datagram")
    else:
        if m not in IOV_MODES:
            raise ValueError(f"{who} takes the whole-packet modes: raw, udp, tcp, icmp, verify_tcp, verify_udp")
        if fill and m not in IOV_FILL_MODES:
            raise ValueError("fill=True takes udp, tcp or icmp")


def _iov(who: str, datagram: bool, pack: bool, pools, view_pool, view_off, view_len, first, mode, *, initial=0,
         initial_arr=None, addrs=None, dst=None, dst_offsets=None, out=None, stream=None, fill=False,
         validate=True):
    """The four scatter-gather functions: ``datagram`` picks the whole-datagram calls
    (no side arrays), ``pack`` the packing ones (``dst``, ``dst_offsets``; returns the
    triple). The call is enqueued on ``stream``; the table was built on the current one."""
    m = _mode(mode)
    _iov_admit(who, m, datagram, fill)
    pools = list(pools)
    dev, table, fi, n = _iov_table(pools, view_pool, view_off, view_len, first, validate)
    initial_arr = _opt(initial_arr, torch.uint16, n, dev, "initial_arr")
    addrs = _opt(addrs, torch.uint8, 8 * n, dev, "addrs")
    if pack:
        dst, do = _pack_dst(pools, dev, table, fi, n, dst, dst_offsets, validate)
    out = _result(out, n * outputs(m), dev)
    name = "yu_csum_" + (("pack_fill_" if fill else "pack_") if pack else ("fill_" if fill else "batch_")) + \
        ("iov_datagram" if datagram else "iov")
    args = [table.data_ptr(), fi.data_ptr(), n, m]
    if not datagram:
        args += [_ptr(initial_arr), initial & 0xFFFF, _ptr(addrs)]
    if pack:
        args += [dst.data_ptr(), do.data_ptr()]
    if stream is not None:
        if pack:
            do.record_stream(stream)
            dst.record_stream(stream)
        stream.wait_stream(torch.cuda.current_stream(dev))
        table.record_stream(stream)
        fi.record_stream(stream)
    with torch.cuda.device(dev):
        rc = getattr(lib(), name)(*args, out.data_ptr() if n else None, _stream(dev, stream))
    check(rc, name)
    if not pack:
        out.iov_table = (table, fi)
        return out
    out.iov_table = (table, fi, do)
    return out, dst, (do if dst_offsets is None else dst_offsets)


def checksum_iov(pools, view_pool: torch.Tensor, view_off: torch.Tensor, view_len: torch.Tensor,
                 first: torch.Tensor, mode="raw", *, initial: int = 0,
                 initial_arr: torch.Tensor | None = None, addrs: torch.Tensor | None = None,
                 out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None,
                 fill: bool = False, validate: bool = True) -> torch.Tensor:
    """Per-packet sums of scatter-gather device packets (yu_csum_batch_iov /
    yu_csum_fill_iov): view j is ``pools[view_pool[j]][view_off[j] : view_off[j] + view_len[j]]``
    and packet i the concatenation of views ``first[i] .. first[i+1]-1`` (``first``: n+1
    non-decreasing entries), e.g. a header pool and a payload pool. ``pools`` is a
    list of contiguous uint8 CUDA tensors on one device; the view arrays and
    ``first`` are CUDA integer tensors there. Each result is what
    :func:`checksum_ragged` gives for the same bytes laid back to back. Modes: RAW,
    UDP, TCP, ICMP, VERIFY_TCP, VERIFY_UDP; packets of at most 65535 bytes.
    ``fill=True`` (UDP, TCP, ICMP) also stores each result big-endian into the
    packet's checksum field where it lies in the pools, across two views if need be.

    The device ``yu_iovec`` table is built with torch operations (no host loop
    over views; capturable in a graph with ``validate=False``). ``validate`` checks
    on the device that every view lies inside its pool, that ``first`` is
    non-decreasing within the view count and that no packet is longer than 65535
    bytes (one small synchronisation). The returned tensor holds the table
    (``out.iov_table``), which must outlive the enqueued call."""
    return _iov("checksum_iov", False, False, pools, view_pool, view_off, view_len, first, mode, initial=initial,
                initial_arr=initial_arr, addrs=addrs, out=out, stream=stream, fill=fill, validate=validate)


def checksum_iov_datagrams(pools, view_pool: torch.Tensor, view_off: torch.Tensor, view_len: torch.Tensor,
                           first: torch.Tensor, mode="verify_rx", *, out: torch.Tensor | None = None,
                           stream: torch.cuda.Stream | None = None, fill: bool = False,
                           validate: bool = True) -> torch.Tensor:
    """Whole IPv4 datagrams held as scatter-gather device packets
    (yu_csum_batch_iov_datagram / yu_csum_fill_iov_datagram): the layout, the table,
    ``validate``, ``stream`` and ``out.iov_table`` are :func:`checksum_iov`'s. Modes:
    IPV4, VERIFY_IPV4, VERIFY_RX, TX_DATAGRAM, whose inputs are read from each
    datagram, so there are no side arrays. Returns ``n * outputs(mode)`` uint16
    results, each what :func:`checksum_ragged` gives for the same bytes laid back to
    back. ``fill=True`` (IPV4, TX_DATAGRAM) also stores the fields
    :func:`checksum_ragged` stores, where they lie in the pools."""
    return _iov("checksum_iov_datagrams", True, False, pools, view_pool, view_off, view_len, first, mode, out=out,
                stream=stream, fill=fill, validate=validate)


def _overlaps(a: torch.Tensor, b: torch.Tensor) -> bool:
    """The address ranges of two contiguous tensors share a byte."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    a1, b1 = a0 + a.numel() * a.element_size(), b0 + b.numel() * b.element_size()
    return a0 < b1 and b0 < a1


def _pack_dst(pools, dev, table, fi, n, dst, dst_offsets, validate: bool):
    """``dst`` and ``dst_offsets`` of the packing calls: the tight offsets and a new
    ``dst`` where they are not given, and the checks ``validate`` asks for. Returns
    (dst, the offsets as int64)."""
    if dst is not None:
        _dev_u8(dst, "dst")
        if dst.device != dev:
            raise TypeError(f"dst must be on {dev}")
        if any(_overlaps(dst, pool) for pool in pools):
            raise ValueError("dst overlaps a pool")
    need_len = dst_offsets is None or (validate and n > 0)
    if need_len:  # the packets' lengths: sums of their views' lengths
        nviews = table.shape[0]  # a table of no views holds one view of no bytes
        ends = torch.zeros(nviews + 1, dtype=torch.int64, device=dev)
        ends[1:] = torch.cumsum(table[:, 1].clamp(min=0), 0)
        f = fi.clamp(0, nviews)
        plen = (ends[f[1:]] - ends[f[:-1]]).clamp(min=0)
    if dst_offsets is None:
        do = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        do[1:] = torch.cumsum(plen, 0)
    else:
        do = _dev_index(dst_offsets, "dst_offsets", dev, n + 1)
        if do.data_ptr() % 8:
            raise TypeError("dst_offsets must be 8-byte aligned")
    if dst is None:
        dst = torch.empty(max(int(do[-1].item()), 1), dtype=torch.uint8, device=dev)
    if validate and n > 0:
        room = do[1:] - do[:-1]
        ok = torch.stack(((room >= 0).all() & (do[0] >= 0), (room >= plen).all(), do[-1] <= dst.numel())).tolist()
        if not ok[0]:
            raise ValueError("dst_offsets is not non-decreasing")
        if not ok[1]:
            raise ValueError("a packet has less room in dst than bytes")
        if not ok[2]:
            raise ValueError("dst_offsets run past dst")
    return dst, do


def pack_iov(pools, view_pool: torch.Tensor, view_off: torch.Tensor, view_len: torch.Tensor,
             first: torch.Tensor, mode="raw", *, initial: int = 0,
             initial_arr: torch.Tensor | None = None, addrs: torch.Tensor | None = None,
             dst: torch.Tensor | None = None, dst_offsets: torch.Tensor | None = None,
             out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None,
             fill: bool = False, validate: bool = True):
    """Scatter-gather device packets summed and packed into one buffer in one pass
    (yu_csum_pack_iov / yu_csum_pack_fill_iov): the layout, the table, the modes,
    the side arguments, ``stream`` and ``out.iov_table`` are :func:`checksum_iov`'s.
    Returns ``(out, dst, dst_offsets)``: packet i's bytes, the concatenation of its
    views, lie at ``dst[dst_offsets[i] : dst_offsets[i] + len_i]`` and ``out[i]`` is
    :func:`checksum_iov`'s value. With tight offsets ``(dst, dst_offsets)`` is the
    batch :func:`checksum_ragged` takes. ``fill=True`` (UDP, TCP, ICMP) stores each
    value big-endian into the field of the *copy*; the pools are never written, so
    views may be shared between packets (one header template for many).

    ``dst_offsets=None``: the tight offsets, an int64 cumsum of the packets' view
    lengths computed on the device. ``dst=None``: a new tensor of ``dst_offsets[-1]``
    bytes, which costs one synchronisation to learn that size. Given ``dst`` (a
    contiguous uint8 CUDA tensor), ``dst_offsets`` (n+1 int64/uint64 entries) and
    ``validate=False`` the call is capturable in a graph. ``validate`` also checks,
    on the device, that ``dst_offsets`` is non-decreasing, that every packet has
    room for its bytes and that ``dst_offsets[-1] <= dst.numel()``, and on the host
    that ``dst`` meets no pool. Slack bytes between packets are never written."""
    return _iov("pack_iov", False, True, pools, view_pool, view_off, view_len, first, mode, initial=initial,
                initial_arr=initial_arr, addrs=addrs, dst=dst, dst_offsets=dst_offsets, out=out, stream=stream,
                fill=fill, validate=validate)


def pack_iov_datagrams(pools, view_pool: torch.Tensor, view_off: torch.Tensor, view_len: torch.Tensor,
                       first: torch.Tensor, mode="verify_rx", *, dst: torch.Tensor | None = None,
                       dst_offsets: torch.Tensor | None = None, out: torch.Tensor | None = None,
                       stream: torch.cuda.Stream | None = None, fill: bool = False, validate: bool = True):
    """Whole IPv4 datagrams held as scatter-gather device packets, verified or filled
    and packed into one buffer in one pass (yu_csum_pack_iov_datagram /
    yu_csum_pack_fill_iov_datagram). The layout, the table, the modes and ``out`` are
    :func:`checksum_iov_datagrams`'s (IPV4, VERIFY_IPV4, VERIFY_RX, TX_DATAGRAM, no side
    arrays); ``dst``, ``dst_offsets``, ``validate`` and ``stream`` are :func:`pack_iov`'s.
    Returns ``(out, dst, dst_offsets)``: every byte of packet i lies at
    ``dst[dst_offsets[i] : dst_offsets[i] + len_i]``, whatever its header says, and
    ``out`` is :func:`checksum_iov_datagrams`'s. ``fill=True`` (IPV4, TX_DATAGRAM) gives
    the copy the fields :func:`checksum_ragged` with ``fill=True`` would store on it;
    the pools are never written, so one header template may serve many packets."""
    return _iov("pack_iov_datagrams", True, True, pools, view_pool, view_off, view_len, first, mode, dst=dst,
                dst_offsets=dst_offsets, out=out, stream=stream, fill=fill, validate=validate)


def build_datagrams(payload: torch.Tensor, pay_offsets: torch.Tensor, records: torch.Tensor, *,
                    dst: torch.Tensor | None = None, dst_offsets: torch.Tensor | None = None,
                    out: torch.Tensor | None = None, validate: bool = False,
                    stream: torch.cuda.Stream | None = None):
    """Outgoing IPv4 datagrams built on the device (yu_tx_build_ragged): what sendUDP,
    sendTCP / sendTCPWithOptions and sendICMPv4 do with a payload and a few numbers,
    WritePacket's IPv4 header included. Payload i is ``payload[pay_offsets[i] :
    pay_offsets[i+1]]`` (n+1 int64/uint64 offsets; for TCP its first ``doff - 20`` bytes
    are the option bytes); ``records`` is a device uint8 tensor of shape (n, 32), one
    ``yu_tx_record`` per packet (:func:`yustack_amd.packets.tx_records` fills them on the
    host). Returns ``(dst, dst_offsets, out)``: datagram i, 20 + H + L bytes with both
    checksum fields in place, lies at ``dst[dst_offsets[i]:]``, and ``out[2i], out[2i+1]``
    are its IPv4 and transport field values as ``tx_datagram`` gives them.

    ``dst_offsets=None``: the tight offsets, ``pay_offsets + exclusive_cumsum(20 + H)``
    with H from the records' proto column, computed on the device with no host read;
    ``(dst, dst_offsets)`` is then the batch :func:`checksum_ragged` takes. ``dst=None``:
    a new tensor of ``dst_offsets[-1]`` bytes (one synchronisation to learn the size).
    ``validate=True`` reads the tables back and raises ValueError for any packet out of
    the call's contract (include/yucsum.h). With ``dst``, ``dst_offsets`` and ``out``
    given the call is capturable in a graph."""
    _dev_u8(payload, "payload")
    dev = payload.device
    _dev_u8(records, "records")
    if records.device != dev:
        raise TypeError(f"records must be on {dev}")
    if records.dim() != 2 or records.shape[1] != 32:
        raise ValueError("records must have shape (n, 32)")
    n = records.shape[0]
    po = _dev_index(pay_offsets, "pay_offsets", dev, n + 1)
    if records.data_ptr() % 8 or po.data_ptr() % 8:
        raise TypeError("records and pay_offsets must be 8-byte aligned")
    if dst is not None:
        _dev_u8(dst, "dst")
        if dst.device != dev:
            raise TypeError(f"dst must be on {dev}")
        if _overlaps(dst, payload) or _overlaps(dst, records):
            raise ValueError("dst overlaps payload or records")
    need_len = dst_offsets is None or (validate and n > 0)
    if need_len:  # 20 + H per packet, from the proto column
        proto = records[:, 24].to(torch.int64)
        hdr = 20 + 20 * (proto == 6) + 8 * (proto == 17) + 4 * (proto == 1)
    if dst_offsets is None:
        do = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n:
            do[1:] = torch.cumsum(hdr, 0)
        do += po
    else:
        do = _dev_index(dst_offsets, "dst_offsets", dev, n + 1)
        if do.data_ptr() % 8:
            raise TypeError("dst_offsets must be 8-byte aligned")
    if dst is None:
        dst = torch.empty(max(int(do[-1].item()), 1), dtype=torch.uint8, device=dev)
    if validate and n > 0:
        plen = po[1:] - po[:-1]
        room = do[1:] - do[:-1]
        total = hdr + plen
        doff = records[:, 23].to(torch.int64)
        tcp_ok = (proto != 6) | ((doff >= 20) & (doff <= 60) & (doff % 4 == 0) & (doff - 20 <= plen))
        ok = torch.stack(((plen >= 0).all() & (po[0] >= 0) & (po[-1] <= payload.numel()),
                          (room >= 0).all() & (do[0] >= 0) & (do[-1] <= dst.numel()),
                          (total <= MAX_TRANSPORT_LEN).all(), (total <= room).all(), tcp_ok.all())).tolist()
        if not ok[0]:
            raise ValueError("pay_offsets is not non-decreasing within payload")
        if not ok[1]:
            raise ValueError("dst_offsets is not non-decreasing within dst")
        if not ok[2]:
            raise ValueError("datagrams must be <= 65535 bytes")
        if not ok[3]:
            raise ValueError("a datagram has less room in dst than bytes")
        if not ok[4]:
            raise ValueError("a TCP record's doff is not 20..60, a multiple of 4 and within its payload")
    out = _result(out, 2 * n, dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
        for t in (po, do, dst, out):
            t.record_stream(stream)
    with torch.cuda.device(dev):
        rc = lib().yu_tx_build_ragged(payload.data_ptr(), po.data_ptr(), records.data_ptr(), n, dst.data_ptr(),
                                      do.data_ptr(), out.data_ptr() if n else None, _stream(dev, stream))
    check(rc, "yu_tx_build_ragged")
    out.build_tables = (po, do)  # the kernel reads them asynchronously: keep them alive with the result
    return dst, (do if dst_offsets is None else dst_offsets), out


def split_datagrams(data: torch.Tensor, offsets: torch.Tensor, *, pay: torch.Tensor | None = None,
                    pay_offsets: torch.Tensor | None = None, records: torch.Tensor | None = None,
                    pay_len: torch.Tensor | None = None, out: torch.Tensor | None = None, validate: bool = False,
                    stream: torch.cuda.Stream | None = None):
    """Received IPv4 datagrams taken apart on the device (yu_rx_split_ragged), the inverse
    of :func:`build_datagrams`: what ipv4.HandlePacket, Nic.DeliverTransportPacket,
    segment.parse and udp.endpoint.HandlePacket do with a datagram once its checksums
    are known. Packet i is ``data[offsets[i] : offsets[i+1]]`` (n+1 int64/uint64 offsets,
    the batch :func:`checksum_ragged` takes). Returns ``(pay, pay_offsets, pay_len,
    records, out)``: ``out[i]`` is ``verify_rx``'s flags plus :data:`RX_SPLIT`; where that
    bit is set, ``records[i]`` (shape (n, 32) uint8, :func:`yustack_amd.packets.rx_records`
    views it as ``TX_RECORD``) holds the header fields, ``pay_len[i]`` (int32) the payload's
    length L and ``pay[pay_offsets[i] : pay_offsets[i] + L]`` the payload (for TCP it
    starts with the option bytes); where it is not, the record is zero, ``pay_len[i]`` is 0
    and nothing is stored in ``pay``.

    ``pay_offsets=None``: the ``offsets`` tensor itself (a packet's own length is always
    room enough), with no host read. ``pay=None``: a new tensor of ``max(data.numel(), 1)``
    bytes. ``validate=True`` reads the tables and the headers back and raises
    ValueError for offsets out of the call's contract (include/yucsum.h) or for a packet
    whose payload, by its own header, has less room in ``pay`` than bytes (room of the
    packet's length, as with ``pay_offsets=None``, always suffices). With every tensor
    given the call is capturable in a graph."""
    _dev_u8(data, "data")
    dev = data.device
    if not isinstance(offsets, torch.Tensor) or not offsets.is_cuda or offsets.device != dev:
        raise TypeError(f"offsets must be a CUDA tensor on {dev}")
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("offsets must hold n + 1 entries")
    n = offsets.numel() - 1
    o = _dev_index(offsets, "offsets", dev, n + 1)
    po = o if pay_offsets is None else _dev_index(pay_offsets, "pay_offsets", dev, n + 1)
    if o.data_ptr() % 8 or po.data_ptr() % 8:
        raise TypeError("offsets and pay_offsets must be 8-byte aligned")
    if pay is None:
        pay = torch.empty(max(data.numel(), 1), dtype=torch.uint8, device=dev)
    else:
        _dev_u8(pay, "pay")
        if pay.device != dev:
            raise TypeError(f"pay must be on {dev}")
        if _overlaps(pay, data):
            raise ValueError("pay overlaps data")
    if records is None:
        records = torch.empty((max(n, 1), 32), dtype=torch.uint8, device=dev)[:n]
    else:
        _dev_u8(records, "records")
        if records.device != dev:
            raise TypeError(f"records must be on {dev}")
        if records.dim() != 2 or records.shape != (n, 32):
            raise ValueError("records must have shape (n, 32)")
        if records.data_ptr() % 8:
            raise TypeError("records must be 8-byte aligned")
        if _overlaps(pay, records):
            raise ValueError("pay overlaps records")
    if pay_len is None:
        pay_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    else:
        pay_len = _opt(pay_len, torch.int32, n, dev, "pay_len")
    if validate and n > 0:
        plen = o[1:] - o[:-1]
        room = po[1:] - po[:-1]
        # what each header asks for: slen - H where IsValid holds and HL >= 20 (a packet
        # the delivery tests then refuse stores nothing and needs no room)
        byte = lambda k: data[(o[:-1] + k).clamp(0, data.numel() - 1)].to(torch.int64)  # noqa: E731
        hl, tl, proto = (byte(0) & 15) * 4, byte(2) * 256 + byte(3), byte(9)
        hdr = hl + 20 * (proto == 6) + 8 * (proto == 17) + 4 * (proto == 1)
        need = torch.where((plen >= 20) & (hl >= 20) & (hl <= tl) & (tl <= plen), (tl - hdr).clamp(min=0), 0)
        ok = torch.stack(((plen >= 0).all() & (o[0] >= 0) & (o[-1] <= data.numel()),
                          (plen <= MAX_TRANSPORT_LEN).all(),
                          (room >= 0).all() & (po[0] >= 0) & (po[-1] <= pay.numel()),
                          (room >= need).all())).tolist()
        if not ok[0]:
            raise ValueError("offsets is not non-decreasing within data")
        if not ok[1]:
            raise ValueError("datagrams must be <= 65535 bytes")
        if not ok[2]:
            raise ValueError("pay_offsets is not non-decreasing within pay")
        if not ok[3]:
            raise ValueError("a packet's payload has less room in pay than bytes")
    out = _result(out, n, dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
        for t in (o, po, pay, records, pay_len, out):
            t.record_stream(stream)
    with torch.cuda.device(dev):
        rc = lib().yu_rx_split_ragged(data.data_ptr(), o.data_ptr(), n, pay.data_ptr(), po.data_ptr(),
                                      records.data_ptr() if n else None, pay_len.data_ptr() if n else None,
                                      out.data_ptr() if n else None, _stream(dev, stream))
    check(rc, "yu_rx_split_ragged")
    out.split_tables = (o, po)  # the kernel reads them asynchronously: keep them alive with the result
    return pay, (offsets if pay_offsets is None else pay_offsets), pay_len, records, out


def parse_datagrams(data: torch.Tensor, offsets: torch.Tensor, *, verify: bool = True,
                    records: torch.Tensor | None = None, views: torch.Tensor | None = None,
                    out: torch.Tensor | None = None, validate: bool = False,
                    stream: torch.cuda.Stream | None = None):
    """Received IPv4 datagrams parsed where they lie (yu_rx_parse_ragged):
    :func:`split_datagrams` without the payload copy. Packet i is ``data[offsets[i] :
    offsets[i+1]]`` (n+1 int64/uint64 offsets). Returns ``(records, views, out)``:
    ``records`` (shape (n, 32) uint8) are :func:`split_datagrams`'s; ``views`` (shape
    (n, 2) int64) holds, where :data:`RX_SPLIT` is set, the payload's device address and
    its length L, and ``(0, 0)`` where it is not; ``out[i]`` is :func:`split_datagrams`'s
    value with ``verify=True`` (``verify_rx``'s flags plus :data:`RX_SPLIT`, two launches)
    and that value ``& (RX_INVALID | RX_SPLIT)`` with ``verify=False`` (the header pass
    alone: no checksum is computed and no payload byte is read).

    The payloads stay in ``data``: ``views[:, 0] - data.data_ptr()`` and ``views[:, 1]``
    are the ``view_off`` and ``view_len`` that ``batch.pack_iov([data], view_pool, view_off,
    view_len, first, ...)`` takes (``view_pool`` zeros, ``first = arange(n + 1)``, or fewer
    rows for the packets the receiver accepts), so gathering what was accepted is a
    composition of the two calls. In C the table is a ``yu_iovec`` array as it is.

    ``validate=True`` reads the offsets back and raises ValueError where they are out of
    the call's contract (include/yucsum.h). With every tensor given the call is capturable
    in a graph."""
    _dev_u8(data, "data")
    dev = data.device
    if not isinstance(offsets, torch.Tensor) or not offsets.is_cuda or offsets.device != dev:
        raise TypeError(f"offsets must be a CUDA tensor on {dev}")
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("offsets must hold n + 1 entries")
    n = offsets.numel() - 1
    o = _dev_index(offsets, "offsets", dev, n + 1)
    if o.data_ptr() % 8:
        raise TypeError("offsets must be 8-byte aligned")
    if records is None:
        records = torch.empty((max(n, 1), 32), dtype=torch.uint8, device=dev)[:n]
    else:
        _dev_u8(records, "records")
        if records.device != dev:
            raise TypeError(f"records must be on {dev}")
        if records.dim() != 2 or records.shape != (n, 32):
            raise ValueError("records must have shape (n, 32)")
        if records.data_ptr() % 8:
            raise TypeError("records must be 8-byte aligned")
        if _overlaps(records, data):
            raise ValueError("records overlaps data")
    if views is None:
        views = torch.empty((max(n, 1), 2), dtype=torch.int64, device=dev)[:n]
    else:
        if not isinstance(views, torch.Tensor) or not views.is_cuda or views.device != dev:
            raise TypeError(f"views must be a CUDA tensor on {dev}")
        if views.dtype != torch.int64 or not views.is_contiguous():
            raise TypeError("views must be a contiguous int64 tensor")
        if views.dim() != 2 or views.shape != (n, 2):
            raise ValueError("views must have shape (n, 2)")
        if _overlaps(views, data) or _overlaps(views, records):
            raise ValueError("views overlaps data or records")
    if validate and n > 0:
        plen = o[1:] - o[:-1]
        ok = torch.stack(((plen >= 0).all() & (o[0] >= 0) & (o[-1] <= data.numel()),
                          (plen <= MAX_TRANSPORT_LEN).all())).tolist()
        if not ok[0]:
            raise ValueError("offsets is not non-decreasing within data")
        if not ok[1]:
            raise ValueError("datagrams must be <= 65535 bytes")
    out = _result(out, n, dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
        for t in (o, records, views, out):
            t.record_stream(stream)
    with torch.cuda.device(dev):
        rc = lib().yu_rx_parse_ragged(data.data_ptr(), o.data_ptr(), n, 1 if verify else 0,
                                      records.data_ptr() if n else None, views.data_ptr() if n else None,
                                      out.data_ptr() if n else None, _stream(dev, stream))
    check(rc, "yu_rx_parse_ragged")
    out.parse_tables = (o, data)  # read asynchronously, and the views point into data: keep both alive
    return records, views, out


def parse_variant(n: int = 1 << 20) -> str:
    """Name of the kernel of :func:`parse_datagrams`'s header pass for a batch of n packets
    (with ``verify=True`` :func:`ragged_variant` ``("verify_rx", n)`` names the launch before it)."""
    return _wave_variant("rx_parse", n)


DEMUX_NONE = 0xFFFFFFFF  # YU_DEMUX_NONE: no endpoint, the reference drops the packet
DEMUX_MAX_ENDPOINTS = 1 << 24


def demux_table(ids, device):
    """The demultiplexer's table of the registered endpoint ids (yu_demux_table_fill):
    filled on the host and uploaded to ``device``. ``ids`` is an array of
    :data:`packets.ENDPOINT_ID` (``packets.endpoint_ids``), or its bytes as shape (m, 16)
    uint8; an endpoint's number is its position in it. Returns ``(table, m)``, what
    :func:`demux_datagrams` takes. Raises ValueError naming ``bad``, the index of the first
    refused id: a malformed one (``proto`` not 6 or 17, ``kind`` over 2, a field its kind
    empties not zero) or one equal to an earlier id (the reference's ErrPortInUse)."""
    ids = np.ascontiguousarray(ids)
    if ids.dtype == np.uint8 and ids.ndim == 2 and ids.shape[1] == ENDPOINT_ID.itemsize:
        ids = ids.view(ENDPOINT_ID).reshape(ids.shape[0])
    if ids.dtype != ENDPOINT_ID:
        raise TypeError("ids must be an array of packets.ENDPOINT_ID (or its bytes, shape (m, 16) uint8)")
    if ids.ndim != 1:
        raise ValueError("ids must be one-dimensional")
    device = torch.device(device)
    if device.type != "cuda":
        raise TypeError("device must be a CUDA (HIP) device")
    m = int(ids.shape[0])
    nbytes = int(lib().yu_demux_table_bytes(m))
    if nbytes == 0:
        raise ValueError(f"at most {DEMUX_MAX_ENDPOINTS} endpoint ids")
    host = np.empty(nbytes, dtype=np.uint8)
    bad = ctypes.c_uint64(m)
    rc = lib().yu_demux_table_fill(ids.ctypes.data if m else None, m, host.ctypes.data, nbytes, ctypes.byref(bad))
    if rc == YU_EINVAL:
        raise ValueError(f"endpoint id {bad.value} is malformed or equals an earlier id (bad = {bad.value})")
    check(rc, "yu_demux_table_fill")
    return torch.from_numpy(host).to(device), m


def _dev_u32(t, shape, dev, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev:
        raise TypeError(f"{name} must be a CUDA tensor on {dev}")
    if t.dtype not in (torch.uint32, torch.int32) or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous uint32 (or int32) tensor")
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} must have shape {shape}")
    return t


def demux_datagrams(records: torch.Tensor, table: torch.Tensor, m: int, *, flags: torch.Tensor | None = None,
                    need: int = 0, ep: torch.Tensor | None = None, counts: torch.Tensor | None = None,
                    group: bool = False, stream: torch.cuda.Stream | None = None):
    """Transport demultiplexing on the device (yu_rx_demux): which registered endpoint
    gets each received packet. ``records`` (shape (n, 32) uint8) are
    :func:`parse_datagrams`' or :func:`split_datagrams`'; ``table, m`` are
    :func:`demux_table`'s. A packet is eligible when its protocol is 6 or 17 and, with
    ``flags`` (the ``out`` of the call that stored the records), ``flags[i]`` has every
    bit of ``need | RX_SPLIT``: ``need=0`` is the reference, which does not drop on
    checksum outcomes here, ``need=RX_IP_OK | RX_L4_OK`` a receiver that does. Its id
    (local = the record's ``dst`` and ``dport``, remote = ``src`` and ``sport``) is looked
    up as a connection, then as a listener on the address, then as a listener on the port.

    Returns ``(ep, counts)``: ``ep[i]`` (uint32) is the first hit's endpoint number, or
    :data:`DEMUX_NONE` when all three miss or the packet is ineligible; ``counts``
    (m + 1 uint32) has the packets per endpoint and, at ``[m]``, those without one. The
    call *adds* to a ``counts`` it is given (to accumulate over batches) and zeroes one it
    allocates.

    ``group=True`` returns ``(ep, counts, order, first)``: ``order`` is the stable sort of
    the packet numbers by endpoint (packets without one last) and ``first`` (m + 2 int64)
    the exclusive sum of ``counts``, so ``order[first[e]:first[e+1]]`` are endpoint e's
    packets in arrival order and ``order[:first[m]]`` every delivered one. It needs counts
    that were zero before the call. :func:`group_datagrams` is the same grouping as one C-ABI
    call (yu_rx_group) that allocates nothing, and with ``views`` it also gives the gather below
    its table without a host read. Here the grouping is torch operations, not part of the C call;
    with ``stream`` they run on that stream, behind the kernel, and ``order`` and ``first`` are
    allocated on it: like ``ep``, they are ready when ``stream`` is, so wait for it before
    using them on another stream.

    Gathering each endpoint's payloads: with ``views`` from :func:`parse_datagrams` over
    ``data``, ``sel = order[:first[m]]`` and ``k = sel.numel()``, ::

        vl = views[sel, 1]
        do = torch.zeros(k + 1, dtype=torch.int64, device=dev); do[1:] = vl.cumsum(0)
        pack_iov([data], torch.zeros_like(vl), views[sel, 0] - data.data_ptr(), vl,
                 torch.arange(k + 1, device=dev), "raw", dst_offsets=do)

    leaves endpoint e's payloads contiguous and in arrival order from ``dst[do[first[e]]]``
    on: one packet stays one scatter-gather packet. An endpoint's whole queue must not be
    made a single scatter-gather packet, those calls stop at 65535 bytes per packet.

    With ``ep`` and ``counts`` given and ``group=False`` the call is capturable in a graph."""
    _dev_u8(records, "records")
    dev = records.device
    if records.dim() != 2 or records.shape[1] != 32:
        raise ValueError("records must have shape (n, 32)")
    n = records.shape[0]
    if records.data_ptr() % 8:
        raise TypeError("records must be 8-byte aligned")
    _dev_u8(table, "table")
    if table.device != dev:
        raise TypeError(f"table must be on {dev}")
    m = int(m)
    if not 0 <= m <= DEMUX_MAX_ENDPOINTS:
        raise ValueError(f"m must be 0 .. {DEMUX_MAX_ENDPOINTS}")
    if table.dim() != 1 or table.numel() != int(lib().yu_demux_table_bytes(m)):
        raise ValueError("table must hold the yu_demux_table_bytes(m) bytes demux_table returned")
    if table.data_ptr() % 16:
        raise TypeError("table must be 16-byte aligned")
    flags = _opt(flags, torch.uint16, n, dev, "flags")
    need = int(need)
    if not 0 <= need <= 0xFFFF:
        raise ValueError("need must be a combination of the RX_ bits")
    ep = torch.empty(max(n, 1), dtype=torch.uint32, device=dev)[:n] if ep is None else _dev_u32(ep, (n,), dev, "ep")
    if counts is None:
        counts = torch.zeros(m + 1, dtype=torch.uint32, device=dev)
    else:
        _dev_u32(counts, (m + 1,), dev, "counts")
    for k, t in enumerate((ep, counts)):
        if any(_overlaps(t, s) for s in (records, table, flags, ep)[:3 + k] if s is not None and s.numel()):
            raise ValueError("ep and counts must overlap nothing the call reads, nor each other")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
        for t in (records, table, ep, counts) + (() if flags is None else (flags,)):
            t.record_stream(stream)
    with torch.cuda.device(dev):
        rc = lib().yu_rx_demux(records.data_ptr() if n else None, _ptr(flags) if n else None, need, n,
                               table.data_ptr(), table.numel(), m, ep.data_ptr() if n else None, counts.data_ptr(),
                               _stream(dev, stream))
    check(rc, "yu_rx_demux")
    ep.demux_tables = (records, table, flags)  # read asynchronously: keep them alive
    if not group:
        return ep, counts
    # on the stream the kernel runs on, behind it: ep and counts are read where they were written
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        key = ep.view(torch.int32).to(torch.int64)
        order = torch.sort(torch.where(key < 0, m, key), stable=True).indices
        first = torch.zeros(m + 2, dtype=torch.int64, device=dev)
        first[1:] = torch.cumsum(counts.view(torch.int32).to(torch.int64), 0)
    return ep, counts, order, first


def demux_variant(n: int = 1 << 20) -> str:
    """Name of the kernel :func:`demux_datagrams` launches for a batch of n packets."""
    return _wave_variant("rx_demux", n)


def group_workspace_bytes(n: int, m: int) -> int:
    """Bytes of scratch memory :func:`group_datagrams` needs for n packets and m endpoints
    (yu_rx_group_workspace_bytes): the same on every device and monotone in n; 0 when
    ``m > DEMUX_MAX_ENDPOINTS`` or ``n >= 2**32``."""
    return int(lib().yu_rx_group_workspace_bytes(int(n), int(m)))


def group_variant(n: int = 1 << 20, m: int = 1) -> str:
    """Name of the partition :func:`group_datagrams` runs for n packets and m endpoints:
    ``k_group<P>`` with P passes (one up to m = 255, two up to 65535, four at 2**24)."""
    return lib().yu_rx_group_variant_n(int(n), int(m)).decode()


def _group_buf(t, dtypes, shape, dev, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev:
        raise TypeError(f"{name} must be a CUDA tensor on {dev}")
    if t.dtype not in dtypes or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous tensor of dtype {' or '.join(str(d) for d in dtypes)}")
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} must have shape {shape}")
    return t


def group_datagrams(ep: torch.Tensor, m: int, *, views: torch.Tensor | None = None,
                    order: torch.Tensor | None = None, first: torch.Tensor | None = None,
                    q_views: torch.Tensor | None = None, q_offsets: torch.Tensor | None = None,
                    work: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None):
    """The packets of a batch grouped by endpoint on the device (yu_rx_group): the step
    between :func:`demux_datagrams` and :func:`pack_iov`. ``ep`` (n uint32 or int32) is
    :func:`demux_datagrams`'; a value at or above ``m``, :data:`DEMUX_NONE` among them, is
    "no endpoint" and has the key ``m``.

    Returns ``(order, first)``: ``order`` (n int32) is the stable sort of the packet numbers
    by key and ``first`` (m + 2 int64) the number of packets with a key below e, so
    ``order[first[e]:first[e+1]]`` is endpoint e's queue in arrival order and
    ``order[:first[m]]`` every delivered packet: what ``demux_datagrams(group=True)``
    computes with torch operations. ``first`` comes from ``ep`` alone. With n = 0 the call
    still stores ``first`` (all zero) and ``q_offsets[0]``.

    With ``views`` (shape (n, 2) int64, :func:`parse_datagrams`') it returns ``(order, first,
    q_views, q_offsets)``: ``q_views[j] = views[order[j]]`` for ``j < first[m]`` and
    ``(0, 0)`` after, and ``q_offsets`` (n + 1 int64) the exclusive sum of ``q_views[:, 1]``.
    ``yu_csum_pack_iov(q_views, arange(n + 1), n, RAW, ..., dst, q_offsets, ...)`` over all n
    packets then leaves endpoint e's payloads contiguous and in arrival order at
    ``dst[q_offsets[first[e]] : q_offsets[first[e+1]]]``; dropped packets copy nothing, and
    ``dst`` is sized on the host by an upper bound such as the batch's ``offsets[n]``: no
    value is read back between the calls.

    ``work`` is the scratch memory, at least :func:`group_workspace_bytes` ``(n, m)`` uint8,
    16-byte aligned. Buffers not given are allocated; with every buffer given the call is
    capturable in a graph. ``stream`` as in :func:`demux_datagrams`. ``n >= 2**31`` raises
    ValueError (``order`` is int32, so that it indexes tensors as it is)."""
    if not isinstance(ep, torch.Tensor) or not ep.is_cuda:
        raise TypeError("ep must be a CUDA (HIP) tensor")
    dev = ep.device
    if ep.dim() != 1:
        raise ValueError("ep must be one-dimensional")
    n = ep.numel()
    _dev_u32(ep, (n,), dev, "ep")
    if n >= 1 << 31:
        raise ValueError("at most 2**31 - 1 packets: order holds int32 packet numbers")
    m = int(m)
    if not 0 <= m <= DEMUX_MAX_ENDPOINTS:
        raise ValueError(f"m must be 0 .. {DEMUX_MAX_ENDPOINTS}")
    with_views = views is not None
    if not with_views and (q_views is not None or q_offsets is not None):
        raise ValueError("q_views and q_offsets go with views")
    if with_views:
        _group_buf(views, (torch.int64,), (n, 2), dev, "views")
    need = group_workspace_bytes(n, m)
    if order is None:
        order = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    else:
        _group_buf(order, (torch.int32, torch.uint32), (n,), dev, "order")
        order = order.view(torch.int32)
    if first is None:
        first = torch.empty(m + 2, dtype=torch.int64, device=dev)
    else:
        _group_buf(first, (torch.int64, torch.uint64), (m + 2,), dev, "first")
        first = first.view(torch.int64)
    if with_views:
        if q_views is None:
            q_views = torch.empty((max(n, 1), 2), dtype=torch.int64, device=dev)[:n]
        else:
            _group_buf(q_views, (torch.int64,), (n, 2), dev, "q_views")
        if q_offsets is None:
            q_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        else:
            _group_buf(q_offsets, (torch.int64, torch.uint64), (n + 1,), dev, "q_offsets")
            q_offsets = q_offsets.view(torch.int64)
    if work is None:
        work = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    else:
        _dev_u8(work, "work")
        if work.device != dev:
            raise TypeError(f"work must be on {dev}")
        if work.dim() != 1 or work.numel() < need:
            raise ValueError(f"work must hold group_workspace_bytes(n, m) = {need} bytes")
        if work.data_ptr() % 16:
            raise TypeError("work must be 16-byte aligned")
    reads = tuple(t for t in (ep, views) if t is not None and t.numel())
    writes = tuple(t for t in (order, first, q_views, q_offsets, work) if t is not None and t.numel())
    for k, t in enumerate(writes):
        if any(_overlaps(t, s) for s in reads + writes[:k]):
            raise ValueError("order, first, q_views, q_offsets and work must overlap nothing the call reads, "
                             "nor each other")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
        for t in reads + writes:
            t.record_stream(stream)
    with torch.cuda.device(dev):
        rc = lib().yu_rx_group(ep.data_ptr() if n else None, n, m, _ptr(views) if n else None,
                               order.data_ptr() if n else None, first.data_ptr(),
                               _ptr(q_views) if n else None, _ptr(q_offsets), work.data_ptr(), work.numel(),
                               _stream(dev, stream))
    check(rc, "yu_rx_group")
    order.group_tables = (ep, views, work)  # read and written asynchronously: keep them alive
    if with_views:
        return order, first, q_views, q_offsets
    return order, first


REPLY_ICMP_ECHO, REPLY_UDP_ECHO = 1, 2  # YU_REPLY_ICMP_ECHO, YU_REPLY_UDP_ECHO


def reply_workspace_bytes(n: int) -> int:
    """Bytes of scratch memory :func:`reply_datagrams` needs for n packets
    (yu_rx_reply_workspace_bytes): the same on every device and monotone in n."""
    return int(lib().yu_rx_reply_workspace_bytes(int(n)))


def reply_variant(n: int = 1 << 20) -> str:
    """Name of the kernel :func:`reply_datagrams` launches for a batch of n packets."""
    return _wave_variant("rx_reply", n)


def build_iov_variant(n: int = 1 << 20) -> str:
    """Name of the kernel :func:`build_datagrams_iov` launches for a batch of n packets."""
    return _wave_variant("tx_build_iov", n)


def reply_datagrams(records: torch.Tensor, views: torch.Tensor, ep: torch.Tensor | None, m: int, *,
                    flags: torch.Tensor | None = None, need: int = 0,
                    what: int = REPLY_ICMP_ECHO | REPLY_UDP_ECHO, ep_echo: torch.Tensor | None = None,
                    r_records: torch.Tensor | None = None, r_offsets: torch.Tensor | None = None,
                    work: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None):
    """Which received packets are answered, and with what (yu_rx_reply): the echo of the
    reference's samples for a batch. ``records``, ``views`` and ``flags`` are
    :func:`parse_datagrams`' ``(records, views, out)``, ``ep`` and ``m`` :func:`demux_datagrams`'.
    A packet passes the gate when ``flags`` is None or ``flags[i]`` has every bit of
    ``need | RX_SPLIT``. With :data:`REPLY_ICMP_ECHO` in ``what`` a gated ICMP Echo request
    (type 8, any code) is answered with an Echo reply carrying the same bytes; with
    :data:`REPLY_UDP_ECHO` a gated UDP datagram whose ``ep[i] < m`` is answered with its
    payload, addresses and ports turned round, unless ``ep_echo`` (m uint8, non-zero: this
    endpoint echoes) says its endpoint does not. Everything else, TCP included, and any
    payload that would not fit a 65535-byte datagram, gets no reply. ``ep`` may be None
    without :data:`REPLY_UDP_ECHO`.

    Returns ``(r_records, r_offsets)``: ``r_records`` (shape (n, 32) uint8) holds the reply
    records, 32 zero bytes for an unanswered packet, and ``r_offsets`` (n + 1 int64) the
    exclusive sum of the replies' lengths, 0 for an unanswered packet, so
    ``build_datagrams_iov(views, r_records, r_offsets, dst)`` builds the replies as a tight
    ragged batch in arrival order. ``dst`` of the received batch's size always suffices.
    With n = 0 the call still stores ``r_offsets[0] = 0``.

    ``work`` is the scratch memory, at least :func:`reply_workspace_bytes` ``(n)`` uint8,
    16-byte aligned. Buffers not given are allocated; with every buffer given the call is
    capturable in a graph. ``stream`` as in :func:`demux_datagrams`."""
    _dev_u8(records, "records")
    dev = records.device
    if records.dim() != 2 or records.shape[1] != 32:
        raise ValueError("records must have shape (n, 32)")
    n = records.shape[0]
    if records.data_ptr() % 8:
        raise TypeError("records must be 8-byte aligned")
    _group_buf(views, (torch.int64,), (n, 2), dev, "views")
    what = int(what)
    if what & ~(REPLY_ICMP_ECHO | REPLY_UDP_ECHO) or what < 0:
        raise ValueError("what must be a combination of REPLY_ICMP_ECHO and REPLY_UDP_ECHO")
    if ep is None:
        if what & REPLY_UDP_ECHO:
            raise ValueError("REPLY_UDP_ECHO needs ep")
    else:
        _dev_u32(ep, (n,), dev, "ep")
    m = int(m)
    if not 0 <= m <= DEMUX_MAX_ENDPOINTS:
        raise ValueError(f"m must be 0 .. {DEMUX_MAX_ENDPOINTS}")
    flags = _opt(flags, torch.uint16, n, dev, "flags")
    need = int(need)
    if not 0 <= need <= 0xFFFF:
        raise ValueError("need must be a combination of the RX_ bits")
    if ep_echo is not None:
        _dev_u8(ep_echo, "ep_echo")
        if ep_echo.device != dev or ep_echo.dim() != 1 or ep_echo.numel() != m:
            raise ValueError(f"ep_echo must hold m uint8 values on {dev}")
    if r_records is None:
        r_records = torch.empty((max(n, 1), 32), dtype=torch.uint8, device=dev)[:n]
    else:
        _group_buf(r_records, (torch.uint8,), (n, 32), dev, "r_records")
        if r_records.data_ptr() % 8:
            raise TypeError("r_records must be 8-byte aligned")
    if r_offsets is None:
        r_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    else:
        _group_buf(r_offsets, (torch.int64, torch.uint64), (n + 1,), dev, "r_offsets")
        r_offsets = r_offsets.view(torch.int64)
    bytes_needed = reply_workspace_bytes(n)
    if work is None:
        work = torch.empty(max(bytes_needed, 16), dtype=torch.uint8, device=dev)
    else:
        _dev_u8(work, "work")
        if work.device != dev:
            raise TypeError(f"work must be on {dev}")
        if work.dim() != 1 or work.numel() < bytes_needed:
            raise ValueError(f"work must hold reply_workspace_bytes(n) = {bytes_needed} bytes")
        if work.data_ptr() % 16:
            raise TypeError("work must be 16-byte aligned")
    reads = tuple(t for t in (records, views, flags, ep, ep_echo) if t is not None and t.numel())
    writes = tuple(t for t in (r_records, r_offsets, work) if t.numel())
    for k, t in enumerate(writes):
        if any(_overlaps(t, s) for s in reads + writes[:k]):
            raise ValueError("r_records, r_offsets and work must overlap nothing the call reads, nor each other")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
        for t in reads + writes:
            t.record_stream(stream)
    with torch.cuda.device(dev):
        rc = lib().yu_rx_reply(records.data_ptr() if n else None, _ptr(flags) if n else None, need,
                               views.data_ptr() if n else None, _ptr(ep) if n else None, m,
                               _ptr(ep_echo) if n and m else None, what, n, r_records.data_ptr() if n else None,
                               r_offsets.data_ptr(), work.data_ptr(), work.numel(), _stream(dev, stream))
    check(rc, "yu_rx_reply")
    r_offsets.reply_tables = (records, views, flags, ep, ep_echo, work)  # read asynchronously: keep them alive
    return r_records, r_offsets


def build_datagrams_iov(views: torch.Tensor, records: torch.Tensor, dst_offsets: torch.Tensor,
                        dst: torch.Tensor | None = None, *, out: torch.Tensor | None = None,
                        stream: torch.cuda.Stream | None = None):
    """Outgoing IPv4 datagrams built on the device straight from payload views
    (yu_tx_build_iov): :func:`build_datagrams` with the payload of packet i at the device
    address ``views[i, 0]``, ``views[i, 1]`` bytes long (shape (n, 2) int64, the table
    :func:`parse_datagrams` returns, or any addresses of live device memory), so no payload is
    gathered first. ``records`` are :func:`build_datagrams`'; datagram i goes to
    ``dst[dst_offsets[i] : dst_offsets[i+1]]`` (n + 1 int64/uint64). A packet whose span is
    empty is skipped: its view is not read, its record is ignored and its ``out`` pair is 0,
    so :func:`reply_datagrams`' ``(r_records, r_offsets)`` are passed as they stand. Views may
    overlap each other; none may overlap ``dst``. The memory behind the views is the
    caller's to keep alive until the call has run.

    Returns ``(dst, dst_offsets, out)`` as :func:`build_datagrams`. ``dst=None`` reads
    ``dst_offsets[-1]`` back to size a new one; with every tensor given nothing is read back
    and the call is capturable in a graph."""
    _dev_u8(records, "records")
    dev = records.device
    if records.dim() != 2 or records.shape[1] != 32:
        raise ValueError("records must have shape (n, 32)")
    n = records.shape[0]
    _group_buf(views, (torch.int64,), (n, 2), dev, "views")
    if not isinstance(dst_offsets, torch.Tensor) or dst_offsets.dtype not in (torch.int64, torch.uint64) \
            or not dst_offsets.is_contiguous():
        raise TypeError("dst_offsets must be a contiguous int64 or uint64 tensor")
    do = _dev_index(dst_offsets, "dst_offsets", dev, n + 1)
    if records.data_ptr() % 8 or do.data_ptr() % 8:
        raise TypeError("records and dst_offsets must be 8-byte aligned")
    if dst is None:
        dst = torch.empty(max(int(do[-1].item()), 1), dtype=torch.uint8, device=dev)
    else:
        _dev_u8(dst, "dst")
        if dst.device != dev:
            raise TypeError(f"dst must be on {dev}")
        if _overlaps(dst, records) or _overlaps(dst, views) or _overlaps(dst, do):
            raise ValueError("dst overlaps records, views or dst_offsets")
    out = _result(out, 2 * n, dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
        for t in (views, records, do, dst, out):
            t.record_stream(stream)
    with torch.cuda.device(dev):
        rc = lib().yu_tx_build_iov(views.data_ptr() if n else None, records.data_ptr() if n else None, n,
                                   dst.data_ptr(), do.data_ptr(), out.data_ptr() if n else None,
                                   _stream(dev, stream))
    check(rc, "yu_tx_build_iov")
    out.build_tables = (views, records, do)  # the kernel reads them asynchronously: keep them alive with the result
    return dst, dst_offsets, out


def echo_datagrams(data: torch.Tensor, offsets: torch.Tensor, table: torch.Tensor, m: int, *, need: int = 0,
                   icmp: bool = True, ep_echo: torch.Tensor | None = None, dst: torch.Tensor | None = None,
                   stream: torch.cuda.Stream | None = None):
    """A batch of received IPv4 datagrams answered on the device: :func:`parse_datagrams`
    (with ``verify = need != 0``), yu_rx_demux against ``table, m`` (:func:`demux_table`'s),
    :func:`reply_datagrams` and :func:`build_datagrams_iov`, four asynchronous calls on one
    stream with no host read and no payload copy between them. Every UDP datagram that
    reaches a registered endpoint (one ``ep_echo`` does not switch off) is echoed to its
    sender, and with ``icmp`` every ICMP Echo request is answered; ``need`` is the gate
    (``0``: the reference, which does not drop on checksum outcomes; ``RX_IP_OK | RX_L4_OK``:
    a receiver that does).

    Returns ``(dst, r_offsets, out, flags, ep)``: reply i is ``dst[r_offsets[i] :
    r_offsets[i+1]]``, empty for a packet that got none, ``out`` its two checksum values,
    ``flags`` and ``ep`` the parse's and the demultiplexer's results. ``dst`` defaults to
    ``data.numel()`` bytes, which always suffices: a reply has IHL 5 and carries no byte past
    TotalLength, so it is never longer than the datagram it answers."""
    _dev_u8(data, "data")
    dev = data.device
    if dst is None:
        dst = torch.empty(max(data.numel(), 1), dtype=torch.uint8, device=dev)
    elif _overlaps(_dev_u8(dst, "dst"), data):
        raise ValueError("dst overlaps data")
    need = int(need)
    records, views, flags = parse_datagrams(data, offsets, verify=need != 0, stream=stream)
    n = records.shape[0]
    # the demultiplexer without its counters (demux_datagrams always counts)
    _dev_u8(table, "table")
    m = int(m)
    if not 0 <= m <= DEMUX_MAX_ENDPOINTS:
        raise ValueError(f"m must be 0 .. {DEMUX_MAX_ENDPOINTS}")
    if table.device != dev or table.dim() != 1 or table.numel() != int(lib().yu_demux_table_bytes(m)) \
            or table.data_ptr() % 16:
        raise ValueError("table must be the 16-byte aligned tensor demux_table returned for m ids")
    ep = torch.empty(max(n, 1), dtype=torch.uint32, device=dev)[:n]
    if stream is not None:
        table.record_stream(stream)
        ep.record_stream(stream)
    with torch.cuda.device(dev):
        rc = lib().yu_rx_demux(records.data_ptr() if n else None, flags.data_ptr() if n else None, need, n,
                               table.data_ptr(), table.numel(), m, ep.data_ptr() if n else None, None,
                               _stream(dev, stream))
    check(rc, "yu_rx_demux")
    what = REPLY_UDP_ECHO | (REPLY_ICMP_ECHO if icmp else 0)
    r_records, r_offsets = reply_datagrams(records, views, ep, m, flags=flags, need=need, what=what,
                                           ep_echo=ep_echo, stream=stream)
    dst, _, out = build_datagrams_iov(views, r_records, r_offsets, dst, stream=stream)
    out.echo_tables = (data, table, records, r_records, r_offsets)  # the views point into data: keep it alive
    return dst, r_offsets, out, flags, ep


STREAM_MAX_CAP = 1024
# YU_SEG_*: the verdict on one packet (include/yucsum.h)
SEG_NONE, SEG_CONSUMED, SEG_CONSUMED_LATE, SEG_PENDING, SEG_DUPLICATE, SEG_DROPPED, SEG_UNACCEPTABLE, SEG_NOOP, \
    SEG_IGNORED, SEG_AFTER_CLOSE, SEG_RST, SEG_UNPROCESSED = range(12)


def stream_workspace_bytes(n: int, m: int, cap: int) -> int:
    """Bytes of scratch memory :func:`stream_datagrams` needs for n packets, m endpoints and
    ``cap`` heap entries per endpoint (yu_rx_stream_workspace_bytes); 0 when
    ``m > DEMUX_MAX_ENDPOINTS``, ``n >= 2**32`` or ``cap > STREAM_MAX_CAP``."""
    return int(lib().yu_rx_stream_workspace_bytes(int(n), int(m), int(cap)))


def stream_variant(n: int = 1 << 20, m: int = 1, cap: int = 0) -> str:
    """Name of the kernel :func:`stream_datagrams` launches (``k_stream``)."""
    return lib().yu_rx_stream_variant_n(int(n), int(m), int(cap)).decode()


def tcp_receivers(m: int, cap: int, device, state=None):
    """The per-connection state of :func:`stream_datagrams` on the device: ``(st, heap)``,
    ``st`` of shape (m, 40) uint8 from the host array ``state`` (m entries of
    ``packets.TCP_RCV``, e.g. ``packets.tcp_rcv``; None: every endpoint in state 0) and
    ``heap`` of shape (m * cap, 32) uint8, zeroed. Both live across batches; the call
    updates them in place."""
    from .packets import TCP_RCV
    m, cap = int(m), int(cap)
    if not 0 <= m <= DEMUX_MAX_ENDPOINTS or not 0 <= cap <= STREAM_MAX_CAP:
        raise ValueError(f"m must be 0 .. {DEMUX_MAX_ENDPOINTS} and cap 0 .. {STREAM_MAX_CAP}")
    host = np.zeros(m, dtype=TCP_RCV) if state is None else np.ascontiguousarray(state, dtype=TCP_RCV)
    if host.shape != (m,):
        raise ValueError("state must hold m entries of packets.TCP_RCV")
    st = torch.zeros((max(m, 1), 40), dtype=torch.uint8, device=device)[:m]
    if m:
        st.copy_(torch.from_numpy(host.view(np.uint8).reshape(m, 40).copy()))
    heap = torch.zeros((max(m * cap, 1), 32), dtype=torch.uint8, device=device)[:m * cap]
    return st, heap


def stream_datagrams(records: torch.Tensor, views: torch.Tensor, order: torch.Tensor, first: torch.Tensor, m: int,
                     receivers, *, ids: torch.Tensor | None = None, acks: bool = False,
                     status: torch.Tensor | None = None, s_views: torch.Tensor | None = None,
                     s_offsets: torch.Tensor | None = None, a_records: torch.Tensor | None = None,
                     a_offsets: torch.Tensor | None = None, n_acks: torch.Tensor | None = None,
                     work: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None):
    """TCP segments delivered in order on the device (yu_rx_stream): the reference's
    receiver.handleRcvdSegment over every TCP connection's queue of a batch. ``records`` and
    ``views`` are :func:`parse_datagrams`', ``order`` and ``first`` :func:`group_datagrams`',
    ``receivers`` the ``(st, heap)`` pair of :func:`tcp_receivers`, updated in place; the
    heap's capacity per endpoint is ``heap.shape[0] // m``.

    Returns ``(status, s_views, s_offsets)``: ``status`` (n uint8) the :data:`SEG_NONE` ..
    :data:`SEG_UNPROCESSED` verdict per packet; ``s_views`` (shape (N, 2) int64, N = n + m *
    cap) the delivered payload views in stream order, trimmed, endpoint e's in the slots
    ``first[e] + e * cap .. first[e+1] + (e + 1) * cap`` from the front, ``(0, 0)`` elsewhere;
    ``s_offsets`` (N + 1 int64) the exclusive sum of their lengths, so yu_csum_pack_iov(RAW)
    over the N slots leaves each connection's new in-order bytes contiguous. With ``acks``
    (which needs ``ids``, shape (m, 16) uint8, the ids :func:`demux_table` was given) it also
    returns ``(a_records, a_offsets, n_acks)``: one ACK record per connection that owes one
    (32 zero bytes otherwise), the exclusive sum of 40 per ACK, which
    ``build_datagrams_iov(zero_views, a_records, a_offsets, dst)`` turns into datagrams, and
    the number of ACKs the reference would have sent.

    A segment parked out of order keeps a view into the batch it arrived in: keep that
    memory until it has been delivered. Buffers not given are allocated; with every buffer
    given the call is capturable in a graph."""
    _dev_u8(records, "records")
    dev = records.device
    if records.dim() != 2 or records.shape[1] != 32:
        raise ValueError("records must have shape (n, 32)")
    n = records.shape[0]
    if records.data_ptr() % 8:
        raise TypeError("records must be 8-byte aligned")
    _group_buf(views, (torch.int64,), (n, 2), dev, "views")
    m = int(m)
    if not 0 <= m <= DEMUX_MAX_ENDPOINTS:
        raise ValueError(f"m must be 0 .. {DEMUX_MAX_ENDPOINTS}")
    _group_buf(order, (torch.int32, torch.uint32), (n,), dev, "order")
    _group_buf(first, (torch.int64, torch.uint64), (m + 2,), dev, "first")
    st, heap = receivers
    _group_buf(st, (torch.uint8,), (m, 40), dev, "receivers[0]")
    if not isinstance(heap, torch.Tensor) or not heap.is_cuda or heap.device != dev or heap.dtype != torch.uint8 \
            or heap.dim() != 2 or heap.shape[1] != 32 or not heap.is_contiguous() \
            or (heap.shape[0] % m if m else heap.shape[0]):
        raise ValueError("receivers[1] must be the (m * cap, 32) uint8 tensor tcp_receivers returned")
    cap = heap.shape[0] // m if m else 0
    if cap > STREAM_MAX_CAP:
        raise ValueError(f"at most {STREAM_MAX_CAP} heap entries per endpoint")
    if st.data_ptr() % 8 or heap.data_ptr() % 8:
        raise TypeError("receivers must be 8-byte aligned")
    N = n + m * cap
    if acks:
        if ids is None:
            raise ValueError("acks needs ids")
        _group_buf(ids, (torch.uint8,), (m, 16), dev, "ids")
    elif a_records is not None or a_offsets is not None or n_acks is not None:
        raise ValueError("a_records, a_offsets and n_acks go with acks=True")

    def buf(t, shape, dtypes, name, align=8):
        if t is None:
            t = torch.empty((max(shape[0], 1),) + tuple(shape[1:]), dtype=dtypes[0], device=dev)[:shape[0]]
        else:
            _group_buf(t, dtypes, tuple(shape), dev, name)
            if t.data_ptr() % align:
                raise TypeError(f"{name} must be {align}-byte aligned")
        return t

    status = buf(status, (n,), (torch.uint8,), "status", 1)
    s_views = buf(s_views, (N, 2), (torch.int64,), "s_views")
    s_offsets = buf(s_offsets, (N + 1,), (torch.int64, torch.uint64), "s_offsets").view(torch.int64)
    if acks:
        a_records = buf(a_records, (m, 32), (torch.uint8,), "a_records")
        a_offsets = buf(a_offsets, (m + 1,), (torch.int64, torch.uint64), "a_offsets").view(torch.int64)
        n_acks = buf(n_acks, (m,), (torch.int32, torch.uint32), "n_acks", 4).view(torch.int32)
    need = stream_workspace_bytes(n, m, cap)
    if work is None:
        work = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    else:
        _dev_u8(work, "work")
        if work.device != dev:
            raise TypeError(f"work must be on {dev}")
        if work.dim() != 1 or work.numel() < need:
            raise ValueError(f"work must hold stream_workspace_bytes(n, m, cap) = {need} bytes")
        if work.data_ptr() % 16:
            raise TypeError("work must be 16-byte aligned")
    reads = tuple(t for t in (records, views, order, first, ids) if t is not None and t.numel())
    writes = tuple(t for t in (st, heap, status, s_views, s_offsets, a_records, a_offsets, n_acks, work)
                   if t is not None and t.numel())
    for k, t in enumerate(writes):
        if any(_overlaps(t, s) for s in reads + writes[:k]):
            raise ValueError("the receivers, the outputs and work must overlap nothing the call reads, nor each other")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
        for t in reads + writes:
            t.record_stream(stream)
    with torch.cuda.device(dev):
        rc = lib().yu_rx_stream(records.data_ptr() if n else None, views.data_ptr() if n else None, n,
                                order.data_ptr() if n else None, first.data_ptr(), m,
                                _ptr(ids) if acks and m else None, st.data_ptr() if m else None,
                                heap.data_ptr() if m * cap else None, cap, status.data_ptr() if n else None,
                                s_views.data_ptr() if N else None, s_offsets.data_ptr(),
                                # with m == 0 the two empty ACK outputs have no address of their own, yet the
                                # three are given together: a_offsets' stands in, nothing is stored there
                                (a_records.data_ptr() or a_offsets.data_ptr()) if acks else None, _ptr(a_offsets),
                                (n_acks.data_ptr() or a_offsets.data_ptr()) if acks else None,
                                work.data_ptr(), work.numel(), _stream(dev, stream))
    check(rc, "yu_rx_stream")
    # the launches read and write these asynchronously: they stay alive with the result, as the
    # sibling calls keep theirs (group_tables, reply_tables, build_tables)
    s_offsets.stream_tables = (records, views, order, first, ids, st, heap, work)
    if acks:
        return status, s_views, s_offsets, a_records, a_offsets, n_acks
    return status, s_views, s_offsets


def receive_datagrams(data: torch.Tensor, offsets: torch.Tensor, table: torch.Tensor, m: int, receivers, *,
                      need: int = 0, ids: torch.Tensor | None = None, acks: bool = False,
                      dst: torch.Tensor | None = None, ack_dst: torch.Tensor | None = None,
                      stream: torch.cuda.Stream | None = None):
    """A batch of received IPv4 datagrams turned into each TCP connection's in-order bytes on
    the device: :func:`parse_datagrams` (with ``verify = need != 0``), yu_rx_demux against
    ``table, m``, :func:`group_datagrams`, :func:`stream_datagrams` on ``receivers`` and
    yu_csum_pack_iov(RAW) over the delivered views, asynchronous calls on one stream with no
    host read between them. With ``acks`` (and ``ids``) the ACK datagrams are built too
    (:func:`build_datagrams_iov` from a zeroed view table).

    Returns a dict: ``dst`` (the gathered bytes; connection e's new bytes are
    ``dst[s_offsets[lo] : s_offsets[hi]]`` with ``lo, hi = first[e] + e * cap, first[e+1] + (e +
    1) * cap``), ``s_offsets``, ``s_views``, ``status``, ``first``, ``order``, ``ep``, ``flags``
    and, with ``acks``, ``ack_dst``, ``a_offsets``, ``a_records``, ``n_acks``; ``keep`` holds the
    tensors the asynchronous calls still read (the views point into ``data``): keep the dict
    until the stream has run.

    ``dst`` is sized by the caller: nothing is read back, so the call cannot check it against
    ``s_offsets[-1]``. ``data.numel()`` bytes hold everything this batch can deliver; a
    receiver with ``cap > 0`` may also deliver segments parked by earlier batches, up to
    ``pend_size`` bytes per connection, and the caller who configured the receivers knows that
    bound. So ``dst=None`` (a new tensor of ``data.numel()`` bytes) is accepted with ``cap ==
    0`` only. ``ack_dst`` holds at least 40 bytes per endpoint (the default)."""
    _dev_u8(data, "data")
    dev = data.device
    need = int(need)
    m = int(m)
    if not 0 <= m <= DEMUX_MAX_ENDPOINTS:
        raise ValueError(f"m must be 0 .. {DEMUX_MAX_ENDPOINTS}")
    # the destinations first: nothing is launched for a call that is refused
    heap = receivers[1]
    carried = heap.shape[0] if isinstance(heap, torch.Tensor) and heap.dim() == 2 else 0
    if dst is None:
        if carried:
            raise ValueError("with cap > 0 earlier batches' segments may be delivered too: give dst, sized for "
                             "data.numel() plus what the receivers may hold")
        dst = torch.empty(max(data.numel(), 1), dtype=torch.uint8, device=dev)
    elif _overlaps(_dev_u8(dst, "dst"), data):
        raise ValueError("dst overlaps data")
    elif dst.device != dev or dst.numel() < data.numel():
        raise ValueError("dst must be on the data's device and hold at least data.numel() bytes")
    if acks:
        if ack_dst is None:
            ack_dst = torch.empty(max(40 * m, 1), dtype=torch.uint8, device=dev)
        elif _dev_u8(ack_dst, "ack_dst").device != dev or ack_dst.numel() < 40 * m:
            raise ValueError("ack_dst must be on the data's device and hold 40 bytes per endpoint")
    records, views, flags = parse_datagrams(data, offsets, verify=need != 0, stream=stream)
    n = records.shape[0]
    _dev_u8(table, "table")
    if table.device != dev or table.dim() != 1 or table.numel() != int(lib().yu_demux_table_bytes(m)) \
            or table.data_ptr() % 16:
        raise ValueError("table must be the 16-byte aligned tensor demux_table returned for m ids")
    ep = torch.empty(max(n, 1), dtype=torch.uint32, device=dev)[:n]
    if stream is not None:
        table.record_stream(stream)
        ep.record_stream(stream)
    with torch.cuda.device(dev):
        rc = lib().yu_rx_demux(records.data_ptr() if n else None, flags.data_ptr() if n else None, need, n,
                               table.data_ptr(), table.numel(), m, ep.data_ptr() if n else None, None,
                               _stream(dev, stream))
    check(rc, "yu_rx_demux")
    order, first = group_datagrams(ep, m, stream=stream)
    res = stream_datagrams(records, views, order, first, m, receivers, ids=ids, acks=acks, stream=stream)
    status, s_views, s_offsets = res[:3]
    N = s_views.shape[0]
    fi = torch.arange(N + 1, dtype=torch.int64, device=dev)
    sums = torch.empty(max(N, 1), dtype=torch.uint16, device=dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))  # fi was made on the current stream
        for t in (fi, sums, dst):
            t.record_stream(stream)
    if N:
        with torch.cuda.device(dev):
            rc = lib().yu_csum_pack_iov(s_views.data_ptr(), fi.data_ptr(), N, RAW, None, 0, None, dst.data_ptr(),
                                        s_offsets.data_ptr(), sums.data_ptr(), _stream(dev, stream))
        check(rc, "yu_csum_pack_iov")
    out = dict(dst=dst, s_offsets=s_offsets, s_views=s_views, status=status, first=first, order=order, ep=ep,
               flags=flags, keep=(data, table, records, views, fi, sums))
    if acks:
        a_records, a_offsets, n_acks = res[3:]
        zero_views = torch.zeros((max(m, 1), 2), dtype=torch.int64, device=dev)[:m]
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream(dev))
            zero_views.record_stream(stream)
        ack_dst, _, _ = build_datagrams_iov(zero_views, a_records, a_offsets, ack_dst, stream=stream)
        out.update(ack_dst=ack_dst, a_offsets=a_offsets, a_records=a_records, n_acks=n_acks)
    return out


def split_variant(n: int = 1 << 20) -> str:
    """Name of the kernel :func:`split_datagrams` launches for a batch of n packets."""
    return _wave_variant("rx_split", n)


def _wave_variant(call: str, n: int, mode=None, fill: bool = False) -> str:
    """What ``yu_<call>_variant_n`` names: (mode, n, fill) for the scatter-gather
    calls, n alone for yu_tx_build_variant_n."""
    args = (n,) if mode is None else (_mode(mode), n, 1 if fill else 0)
    return getattr(lib(), f"yu_{call}_variant_n")(*args).decode()


def build_variant(n: int = 1 << 20) -> str:
    """Name of the kernel :func:`build_datagrams` launches for a batch of n packets."""
    return _wave_variant("tx_build", n)


def iov_pack_datagram_variant(mode="verify_rx", n: int = 1 << 20, fill: bool = False) -> str:
    """Name of the kernel the packing whole-datagram calls launch ("" for a mode
    they refuse)."""
    return _wave_variant("iov_pack_datagram", n, mode, fill)


def iov_pack_variant(mode="raw", n: int = 1 << 20, fill: bool = False) -> str:
    """Name of the kernel the packing scatter-gather calls launch ("" for a mode
    they refuse)."""
    return _wave_variant("iov_pack", n, mode, fill)


def iov_datagram_variant(mode="verify_rx", n: int = 1 << 20, fill: bool = False) -> str:
    """Name of the kernel the whole-datagram scatter-gather calls launch ("" for a
    mode they refuse)."""
    return _wave_variant("iov_datagram", n, mode, fill)


def iov_variant(mode="raw", n: int = 1 << 20, fill: bool = False) -> str:
    """Name of the kernel the scatter-gather device calls launch ("" for a mode
    they refuse)."""
    return _wave_variant("iov", n, mode, fill)


def _host_data(data, fill: bool):
    """Pointer and size of a host byte buffer; with ``fill`` the fields are written
    into it, so it must be the caller's own writable contiguous uint8 memory."""
    if isinstance(data, torch.Tensor):
        if data.is_cuda or data.dtype != torch.uint8 or not data.is_contiguous():
            raise TypeError("data must be a contiguous uint8 CPU tensor")
        return data, data.data_ptr(), data.numel()
    if fill:
        if not (isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.flags.c_contiguous
                and data.flags.writeable):
            raise TypeError("fill=True needs a writable C-contiguous uint8 numpy array")
    else:
        data = np.ascontiguousarray(data, dtype=np.uint8)
    return data, data.ctypes.data, data.size


def _fill_name(name: str, fill: bool, device) -> str:
    if not fill:
        return name
    if isinstance(device, (list, tuple)):
        raise ValueError("fill=True takes one device")
    return name.replace("_batch_", "_fill_")


def checksum_host_uniform(data: np.ndarray, stride: int, length: int, n: int, mode="raw", *,
                          initial: int = 0, initial_arr: np.ndarray | None = None,
                          addrs: np.ndarray | None = None, out: np.ndarray | None = None,
                          device: int | list[int] = 0, fill: bool = False) -> np.ndarray:
    """Host-memory batch in, host-memory results out (pinned staging + pipelined
    H2D/kernel/D2H inside the library). ``data`` may be a numpy array or a pinned
    torch CPU tensor (then the copy engine reads it directly). ``device`` may be a
    list of device indices: one shard per GPU, all at once. ``fill=True`` (TX modes)
    also stores each result into the packet's checksum field in ``data``
    (yu_csum_fill_host_uniform)."""
    m = _mode(mode)
    data, dptr, dlen = _host_data(data, fill)
    if n and (n - 1) * stride + length > dlen:
        raise ValueError("data too small for the batch geometry")
    ia = None if initial_arr is None else np.ascontiguousarray(initial_arr, dtype=np.uint16)
    ad = None if addrs is None else np.ascontiguousarray(addrs, dtype=np.uint8)
    if ia is not None and ia.size < n or ad is not None and ad.size < 8 * n:
        raise ValueError("side arrays too small")
    k = outputs(m)
    if out is None:
        out = np.empty(n * k, dtype=np.uint16)
    if isinstance(out, torch.Tensor):
        if out.element_size() != 2 or out.is_cuda or not out.is_contiguous() or out.numel() < n * k:
            raise ValueError("out must be a contiguous 16-bit CPU tensor of >= n results")
        optr = out.data_ptr()
    else:
        if out.dtype.itemsize != 2 or out.size < n * k or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous 16-bit array of >= n results")
        optr = out.ctypes.data
    args = (dptr, stride, length, n, m, None if ia is None else ia.ctypes.data, initial & 0xFFFF,
            None if ad is None else ad.ctypes.data, optr)
    _host_call(_fill_name("yu_csum_batch_host_uniform", fill, device), args, device)
    return out


def _host_call(name: str, args: tuple, device) -> None:
    """``device`` an int: the single-GPU host call. A sequence of ints: the
    ``_multi`` variant, the batch split into one shard per listed device
    (include/yucsum.h)."""
    import ctypes
    if isinstance(device, (list, tuple)):
        devs = (ctypes.c_int * max(1, len(device)))(*[int(d) for d in device])
        rc = getattr(lib(), name + "_multi")(*args, devs, len(device))
        check(rc, name + "_multi")
    else:
        check(getattr(lib(), name)(*args, int(device)), name)


def _host_side(n, initial_arr, addrs, out, k=1):
    ia = None if initial_arr is None else np.ascontiguousarray(initial_arr, dtype=np.uint16)
    ad = None if addrs is None else np.ascontiguousarray(addrs, dtype=np.uint8)
    if ia is not None and ia.size < n or ad is not None and ad.size < 8 * n:
        raise ValueError("side arrays too small")
    if out is None:
        out = np.empty(n * k, dtype=np.uint16)
    elif out.dtype != np.uint16 or out.size < n * k or not out.flags.c_contiguous:
        raise ValueError("out must be a contiguous uint16 array of >= n results")
    return ia, ad, out


def checksum_host_ragged(data, offsets, mode="raw", *, initial: int = 0, initial_arr=None,
                         addrs=None, out: np.ndarray | None = None,
                         device: int | list[int] = 0, fill: bool = False) -> np.ndarray:
    """Ragged host batch (packet i = data[offsets[i]:offsets[i+1]], e.g. a tun read
    burst) through the pinned, pipelined host path (yu_csum_batch_host_ragged).
    ``fill=True``: also the fields, in place (yu_csum_fill_host_ragged)."""
    m = _mode(mode)
    data, dptr, dlen = _host_data(data, fill)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = offs.size - 1
    if n < 0:
        raise ValueError("offsets must hold n+1 entries")
    if n and int(offs[-1]) > dlen:
        raise ValueError("offsets run past data")
    ia, ad, out = _host_side(n, initial_arr, addrs, out, outputs(m))
    args = (dptr, offs.ctypes.data, n, m, None if ia is None else ia.ctypes.data, initial & 0xFFFF,
            None if ad is None else ad.ctypes.data, out.ctypes.data)
    _host_call(_fill_name("yu_csum_batch_host_ragged", fill, device), args, device)
    return out


def checksum_host_iov(packets, mode="raw", *, initial: int = 0, initial_arr=None, addrs=None,
                      out: np.ndarray | None = None,
                      device: int | list[int] = 0, fill: bool = False) -> np.ndarray:
    """Scatter-gather host packets: ``packets[i]`` is a list of views (numpy uint8
    arrays / bytes) whose concatenation is packet i, as tundev's readv fills them
    (link/tundev/tundev.go:116-125). Gathered into pinned staging by the library.
    ``fill=True``: the fields are written through the views, which must then be
    writable contiguous uint8 numpy arrays or bytearrays (yu_csum_fill_host_iov)."""
    from ._lib import YuIovec
    m = _mode(mode)
    n = len(packets)
    keep, views = [], []
    first = np.zeros(n + 1, np.uint64)
    for i, pk in enumerate(packets):
        for v in pk:
            if fill:
                a = np.frombuffer(v, np.uint8) if isinstance(v, bytearray) else v
                if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags.c_contiguous
                        and a.flags.writeable):
                    raise TypeError("fill=True needs writable contiguous uint8 views")
            else:
                a = np.frombuffer(v, np.uint8) if isinstance(v, (bytes, bytearray)) else \
                    np.ascontiguousarray(v, dtype=np.uint8)
            keep.append(a)
            views.append((a.ctypes.data if a.size else None, a.size))
        first[i + 1] = len(views)
    iov = (YuIovec * max(1, len(views)))(*[YuIovec(b, l) for b, l in views])
    ia, ad, out = _host_side(n, initial_arr, addrs, out, outputs(m))
    args = (ctypes_addr(iov), first.ctypes.data, n, m, None if ia is None else ia.ctypes.data,
            initial & 0xFFFF, None if ad is None else ad.ctypes.data, out.ctypes.data)
    _host_call(_fill_name("yu_csum_batch_host_iov", fill, device), args, device)
    del keep
    return out


def ctypes_addr(obj) -> int:
    import ctypes
    return ctypes.addressof(obj)


def verified(sums: torch.Tensor) -> torch.Tensor:
    """checker semantics: a VERIFY_* sum is valid iff it is 0x0000 or 0xFFFF."""
    s = sums.view(torch.int16)
    return (s == 0) | (s == -1)


def rx_accepted(flags: torch.Tensor) -> torch.Tensor:
    """VERIFY_RX: the packet is well formed, its header checksum verifies and, when
    it carries TCP/UDP/ICMP, so does the transport checksum."""
    f = flags.to(torch.int32)
    ok_ip = (f & (RX_IP_OK | RX_INVALID)) == RX_IP_OK
    ok_l4 = ((f & RX_L4) == 0) | ((f & RX_L4_OK) != 0)
    return ok_ip & ok_l4


def ragged_variant(mode="raw", n: int = 1 << 20, fill: bool = False) -> str:
    """Name of the kernel the ragged path launches for this mode and batch size
    (bursts of up to 4096 packets take a wave per packet); ``fill``: the in-place
    form (yu_csum_fill_ragged)."""
    f = lib().yu_ragged_fill_variant_n if fill else lib().yu_ragged_variant_n
    return f(_mode(mode), n).decode()


def variant(stride: int, length: int, mode="raw", align16: int = 0, n: int = 2) -> str:
    """Name of the kernel the uniform path launches for this geometry (and batch
    size: dense packets above 3 KiB go to k_seg only in large batches)."""
    return lib().yu_uniform_variant_n(stride, length, n, _mode(mode), align16).decode()
