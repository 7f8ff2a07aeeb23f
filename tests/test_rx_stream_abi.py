"""yu_rx_stream at the C-ABI boundary (include/yucsum.h: yu_rx_stream_workspace_bytes,
yu_rx_stream, yu_rx_stream_variant_n): exported and declared, the two struct sizes, the
workspace formula of the header and its zeros, every documented YU_EINVAL returned before
any device work (those that do not need n also with n = 0), YU_ENODEV without a device for
what the header says is not an error, the variant name and its tuning value, and what the
Python front end refuses. CPU only: no call here reaches a device."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from yustack_amd import _lib, batch, packets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "yucsum.h")
NAMES = ("yu_rx_stream_workspace_bytes", "yu_rx_stream", "yu_rx_stream_variant_n")
E = _lib.YU_EINVAL
MAX_M = 1 << 24


def test_symbols_structs_and_constants():
    L = _lib.lib()
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert re.search(rf" T {name}$", nm, flags=re.M), name
        assert name in _lib.EXPORTS
    assert len(L.yu_rx_stream.argtypes) == 19
    assert packets.TCP_RCV.itemsize == 40 and packets.TCP_SEG.itemsize == 32
    # the structs as a C compiler lays them out
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "yucsum.h"\nint main(void){printf("%zu %zu %zu %zu %zu",'
            'sizeof(yu_tcp_rcv),sizeof(yu_tcp_seg),offsetof(yu_tcp_rcv,state),offsetof(yu_tcp_seg,pkt),'
            'offsetof(yu_tcp_seg,flags));return 0;}')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(prog)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", c, "-o", os.path.join(d, "s")],
                       check=True)
        out = subprocess.run([os.path.join(d, "s")], capture_output=True, text=True, check=True).stdout
    assert out.split() == ["40", "32", "37", "20", "24"]
    names = ("NONE", "CONSUMED", "CONSUMED_LATE", "PENDING", "DUPLICATE", "DROPPED", "UNACCEPTABLE", "NOOP", "IGNORED",
             "AFTER_CLOSE", "RST", "UNPROCESSED")
    for k, name in enumerate(names):
        assert re.search(rf"#define YU_SEG_{name}\s+{k}u", src), name
        assert getattr(batch, "SEG_" + name) == k
    doc = text[text.index("TCP segments delivered in order on the device"):text.index("uint64_t yu_rx_stream_workspace_bytes")]
    for word in ("sender half", "maxSegmentsPerWake", "segment queue", "one ACK datagram per sendAck", "handshakes",
                 "Lifetime", "cap == 0", "Out of contract"):
        assert word in doc, word


def header_formula(n, m, cap):
    if m > MAX_M or n >= 1 << 32 or cap > 1024:
        return 0
    N = n + m * cap
    return (8 * -(-(max(N, m) + 1) // 2048) + 15) & ~15


def test_workspace_bytes_is_the_header_formula():
    L = _lib.lib()
    for n in (0, 1, 63, 2047, 2048, 2049, 5 * 2048, 1 << 20, (1 << 32) - 1, 1 << 32):
        for m in (0, 1, 3, 70, 2048, 4097, MAX_M, MAX_M + 1):
            for cap in (0, 1, 4, 1024, 1025):
                got = L.yu_rx_stream_workspace_bytes(n, m, cap)
                assert got == header_formula(n, m, cap) == batch.stream_workspace_bytes(n, m, cap), (n, m, cap)
    assert L.yu_rx_stream_workspace_bytes(0, 0, 0) == 16
    assert L.yu_rx_stream_workspace_bytes(0, 5000, 0) == 32      # the ACK offsets are the longer scan
    assert L.yu_rx_stream_workspace_bytes(1 << 32, 1, 1) == 0
    assert L.yu_rx_stream_workspace_bytes(1, MAX_M + 1, 1) == 0
    assert L.yu_rx_stream_workspace_bytes(1, 1, 1025) == 0


@pytest.fixture
def bufs():
    def blk(n):
        b = (ctypes.c_uint8 * (n + 32))(*([0xA5] * (n + 32)))
        return b, (ctypes.addressof(b) + 15) & ~15
    keep, t = [], {}
    for name, size in (("recs", 32 * 8), ("views", 16 * 8), ("order", 4 * 8), ("first", 8 * 8), ("ids", 16 * 4),
                       ("st", 40 * 4), ("heap", 32 * 16), ("status", 8), ("s_views", 16 * 32), ("s_offsets", 8 * 33),
                       ("a_recs", 32 * 4), ("a_offsets", 8 * 5), ("n_acks", 4 * 4), ("work", 256)):
        b, a = blk(size)
        keep.append(b)
        t[name] = a
    t["untouched"] = lambda: all(bytes(b) == b"\xA5" * ctypes.sizeof(b) for b in keep)
    yield t
    del keep


def call(t, n=4, m=3, cap=4, work_bytes=256, **change):
    a = dict(t, **change)
    return _lib.lib().yu_rx_stream(a["recs"], a["views"], n, a["order"], a["first"], m, a["ids"], a["st"], a["heap"],
                                   cap, a["status"], a["s_views"], a["s_offsets"], a["a_recs"], a["a_offsets"],
                                   a["n_acks"], a["work"], work_bytes, None)


def test_every_einval_precedes_device_work(bufs):
    t = bufs
    need = _lib.lib().yu_rx_stream_workspace_bytes(4, 3, 4)
    assert 0 < need <= 256
    # [data], each with n > 0
    for name in ("recs", "views", "order", "first", "work", "heap", "ids"):
        assert call(t, **{name: None}) == E, name
    assert call(t, work_bytes=need - 1) == E and call(t, work_bytes=0) == E
    # [out], with n > 0
    assert call(t, status=None) == E and call(t, s_views=None) == E
    assert call(t, m=0, s_offsets=None) == E
    for n in (4, 0):
        # [data], checked without n
        assert call(t, n, m=MAX_M + 1) == E and call(t, n, cap=1025) == E
        assert call(t, n, st=None) == E
        for gone in (("a_recs",), ("a_offsets",), ("n_acks",), ("a_recs", "a_offsets"), ("a_offsets", "n_acks")):
            assert call(t, n, **{g: None for g in gone}) == E, gone
        # [out]: s_offsets with any n when m > 0; s_views once there are slots
        assert call(t, n, s_offsets=None) == E
        assert call(t, n, s_views=None) == E
        # [offsets]
        for name in ("recs", "views", "first", "st", "heap", "s_views", "s_offsets", "a_recs", "a_offsets"):
            assert call(t, n, **{name: t[name] + 4}) == E, name
        assert call(t, n, work=t["work"] + 8) == E
        # [side-align]
        for name in ("order", "ids", "n_acks"):
            assert call(t, n, **{name: t[name] + 2}) == E, name
    assert call(t, 1 << 32) == E
    assert t["untouched"]()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_valid_calls_fail_without_gpu(bufs):
    t = bufs
    nodev = _lib.YU_ENODEV
    assert call(t) == nodev
    assert call(t, a_recs=None, a_offsets=None, n_acks=None, ids=None) == nodev
    assert call(t, cap=0, heap=None) == nodev
    assert call(t, m=0, st=None, heap=None, ids=None) == nodev
    assert call(t, work_bytes=_lib.lib().yu_rx_stream_workspace_bytes(4, 3, 4)) == nodev
    assert call(t, status=t["status"] + 1) == nodev                      # status has no alignment
    # n == 0 is not a no-op: the empty tables are stored, which takes a device and no input
    assert call(t, 0) == nodev
    assert call(t, 0, recs=None, views=None, order=None, first=None, ids=None, heap=None, status=None, work=None,
                work_bytes=0) == nodev
    assert call(t, 0, m=0, cap=0, st=None, s_views=None, s_offsets=None, a_recs=None, a_offsets=None,
                n_acks=None) == nodev
    assert t["untouched"]()


def test_variant_name_and_tuning_value():
    L = _lib.lib()
    assert L.yu_rx_stream_variant_n(100, 3, 4) == b"k_stream" and batch.stream_variant(100, 3, 4) == "k_stream"
    assert L.yu_rx_stream_variant_n(1 << 32, 3, 4) == b"none" and L.yu_rx_stream_variant_n(1, 1, 1025) == b"none"
    code = "from yustack_amd import batch; print(batch.stream_variant(100, 3, 4))"

    def under(env):
        e = {k: v for k, v in os.environ.items() if not k.startswith("YU_")}
        e.update(env)
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return r.stdout.strip()
    assert under({"YU_STREAM": "walk"}) == "k_stream"                    # the gate is shut
    assert under({"YU_STREAM": "walk", "YU_TUNING": "1"}) == "k_stream<walk>"
    assert under({"YU_STREAM": "other", "YU_TUNING": "1"}) == "k_stream"


def test_python_front_end_refuses_before_the_library():
    z = torch.zeros
    with pytest.raises(TypeError):
        batch.stream_datagrams(z((4, 32), dtype=torch.uint8), z((4, 2), dtype=torch.int64), z(4, dtype=torch.int32),
                               z(5, dtype=torch.int64), 3, (z((3, 40), dtype=torch.uint8), z((12, 32), dtype=torch.uint8)))
    with pytest.raises(TypeError):
        batch.receive_datagrams(z(64, dtype=torch.uint8), z(2, dtype=torch.int64), z(256, dtype=torch.uint8), 1,
                                (z((1, 40), dtype=torch.uint8), z((0, 32), dtype=torch.uint8)))
    with pytest.raises(ValueError):
        batch.tcp_receivers(3, 1025, "cpu")
    with pytest.raises(ValueError):
        batch.tcp_receivers(3, 4, "cpu", state=packets.tcp_rcv(2))
    st, heap = batch.tcp_receivers(3, 4, "cpu", state=packets.tcp_rcv(3, rcv_nxt=[1, 2, 0xFFFFFFF0], wnd=100))
    assert st.shape == (3, 40) and heap.shape == (12, 32) and not heap.any()
    back = np.frombuffer(st.numpy().tobytes(), dtype=packets.TCP_RCV)
    assert list(back["rcv_nxt"]) == [1, 2, 0xFFFFFFF0] and list(back["rcv_acc"]) == [101, 102, 0x54]
    assert (back["state"] == 1).all() and (back["pend_size"] == 100).all()
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda:0")
    recs, views = z((4, 32), dtype=torch.uint8, device=dev), z((4, 2), dtype=torch.int64, device=dev)
    order, first = z(4, dtype=torch.int32, device=dev), z(5, dtype=torch.int64, device=dev)
    rc = batch.tcp_receivers(3, 4, dev)
    with pytest.raises(ValueError):
        batch.stream_datagrams(recs, views, order, first[:4], 3, rc)              # m + 2
    with pytest.raises(ValueError):
        batch.stream_datagrams(recs, views[:3], order, first, 3, rc)
    with pytest.raises(ValueError):
        batch.stream_datagrams(recs, views, order, first, 3, rc, acks=True)        # needs ids
    with pytest.raises(ValueError):
        batch.stream_datagrams(recs, views, order, first, 3, (rc[0], rc[1][:11]))  # not m * cap
    with pytest.raises(ValueError):
        batch.stream_datagrams(recs, views, order, first, 3, rc, work=z(8, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        batch.stream_datagrams(recs, views, order, first, 3, rc, n_acks=z(3, dtype=torch.int32, device=dev))
