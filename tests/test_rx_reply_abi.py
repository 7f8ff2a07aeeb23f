"""yu_rx_reply at the C-ABI boundary (include/yucsum.h: yu_rx_reply_workspace_bytes,
yu_rx_reply, yu_rx_reply_variant_n): exported and declared, the workspace formula of the
header and its monotonicity, every documented YU_EINVAL returned before any device work
(those that do not need n also with n = 0), YU_ENODEV without a device for the calls the
header says are not errors, the variant name, and what the Python front end refuses. CPU
only: no call here reaches a device: the arguments are refused first, or there is no
device. (A valid call with n = 0 is NOT among them where a device is present: it stores
r_offsets[0].)"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from yustack_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "yucsum.h")
NAMES = ("yu_rx_reply_workspace_bytes", "yu_rx_reply", "yu_rx_reply_variant_n")
E = _lib.YU_EINVAL
MAX_M = 1 << 24
ICMP, UDP = 1, 2


def test_symbols_exported_and_declared():
    L = _lib.lib()
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert re.search(rf" T {name}$", nm, flags=re.M), name
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None
    assert len(L.yu_rx_reply.argtypes) == 14
    assert re.search(r"#define YU_REPLY_ICMP_ECHO 1u", src) and re.search(r"#define YU_REPLY_UDP_ECHO\s+2u", src)
    assert (batch.REPLY_ICMP_ECHO, batch.REPLY_UDP_ECHO) == (ICMP, UDP)
    assert L.yu_abi_version() == 1
    # the header says what the reference does that the call does not model
    doc = text[text.index("Answering received datagrams on the device"):text.index("#define YU_REPLY_ICMP_ECHO")]
    for word in ("FindRoute", "bindAddr", "rcvBufSizeMax", "TCP", "state machine"):
        assert word in doc, word


def header_formula(n):
    """8 bytes per tile of 2048 of the n + 1 outputs, rounded up to a multiple of 16."""
    return (8 * -(-(n + 1) // 2048) + 15) & ~15


def test_workspace_bytes_is_the_header_formula_and_monotone():
    L = _lib.lib()
    ns = sorted({0, 1, 63, 64, 65, 2046, 2047, 2048, 2049, 4095, 4096, 3 * 2048 + 5, 1 << 20, (1 << 20) + 1,
                 (1 << 31) - 1, 1 << 32, 1 << 40} | set(range(0, 30000, 509)))
    sizes = [L.yu_rx_reply_workspace_bytes(n) for n in ns]
    for n, got in zip(ns, sizes):
        assert got == header_formula(n) == batch.reply_workspace_bytes(n), n
        assert got >= 16 and got % 16 == 0
    assert sizes == sorted(sizes)
    assert L.yu_rx_reply_workspace_bytes(0) == 16 and L.yu_rx_reply_workspace_bytes(2047) == 16
    assert L.yu_rx_reply_workspace_bytes(2048) == 16 and L.yu_rx_reply_workspace_bytes(2 * 2048) == 32


@pytest.fixture
def bufs():
    recs = (ctypes.c_uint8 * (32 * 8 + 8))()
    flags = (ctypes.c_uint16 * 9)()
    views = (_lib.YuIovec * 9)()
    ep = (ctypes.c_uint32 * 9)()
    echo = (ctypes.c_uint8 * 8)()
    r_recs = (ctypes.c_uint8 * (32 * 8 + 8))(*([0xA5] * (32 * 8 + 8)))
    r_offsets = (ctypes.c_uint64 * 10)(*([0xA5A5A5A5A5A5A5A5] * 10))
    work = (ctypes.c_uint8 * (256 + 32))(*([0xA5] * (256 + 32)))
    t = dict(recs=ctypes.addressof(recs), flags=ctypes.addressof(flags), views=ctypes.addressof(views),
             ep=ctypes.addressof(ep), ep_echo=ctypes.addressof(echo), r_recs=ctypes.addressof(r_recs),
             r_offsets=ctypes.addressof(r_offsets), work=(ctypes.addressof(work) + 15) & ~15)
    assert all(t[k] % 8 == 0 for k in ("recs", "views", "r_recs", "r_offsets"))

    def untouched():
        return all(bytes(b) == b"\xA5" * ctypes.sizeof(b) for b in (r_recs, r_offsets, work))
    t["untouched"] = untouched
    yield t
    del recs, flags, views, ep, echo, r_recs, r_offsets, work


def call(t, n=4, m=3, need=0, what=ICMP | UDP, work_bytes=256, **change):
    a = dict(t, **change)
    return _lib.lib().yu_rx_reply(a["recs"], a["flags"], need, a["views"], a["ep"], m, a["ep_echo"], what, n,
                                  a["r_recs"], a["r_offsets"], a["work"], work_bytes, None)


def test_every_einval_precedes_device_work(bufs):
    """Each refused argument returns YU_EINVAL, whether or not a device is present
    (nothing is launched: the pointers here are host memory), and stores nothing."""
    t = bufs
    need = _lib.lib().yu_rx_reply_workspace_bytes(4)
    assert 0 < need <= 256
    # [data], each with n > 0
    for name in ("recs", "views", "work"):
        assert call(t, **{name: None}) == E, name
    assert call(t, work_bytes=need - 1) == E
    assert call(t, work_bytes=0) == E
    assert call(t, ep=None) == E                       # YU_REPLY_UDP_ECHO needs ep
    assert call(t, ep=None, what=UDP) == E
    # [out], with n > 0
    assert call(t, r_recs=None) == E
    for n in (4, 0):
        # [data], checked without n
        assert call(t, n, m=MAX_M + 1) == E
        assert call(t, n, m=(1 << 64) - 1) == E
        for what in (4, 8, 7, 1 << 31, 0xFFFFFFFF):
            assert call(t, n, what=what) == E, what
        # [out]: r_offsets is always needed
        assert call(t, n, r_offsets=None) == E
        # [offsets]
        for name in ("recs", "views", "r_recs", "r_offsets"):
            assert call(t, n, **{name: t[name] + 4}) == E, name
        assert call(t, n, work=t["work"] + 8) == E
        # [side-align]
        assert call(t, n, flags=t["flags"] + 1) == E
        assert call(t, n, ep=t["ep"] + 2) == E
    assert t["untouched"]()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_valid_calls_fail_without_gpu(bufs):
    """What the header says is not an error gets past validation and stops at the
    missing device."""
    t = bufs
    nodev = _lib.YU_ENODEV
    assert call(t) == nodev
    assert call(t, flags=None) == nodev
    assert call(t, ep_echo=None) == nodev
    assert call(t, need=1 | 4) == nodev
    assert call(t, m=0) == nodev and call(t, m=MAX_M) == nodev
    assert call(t, what=0, ep=None) == nodev                   # ep may be NULL without YU_REPLY_UDP_ECHO
    assert call(t, what=ICMP, ep=None, ep_echo=None) == nodev
    assert call(t, work_bytes=_lib.lib().yu_rx_reply_workspace_bytes(4)) == nodev
    assert call(t, flags=t["flags"] + 2, ep=t["ep"] + 4, recs=t["recs"] + 8, views=t["views"] + 8,
                r_recs=t["r_recs"] + 8, r_offsets=t["r_offsets"] + 8, work=t["work"] + 16,
                work_bytes=256 - 16) == nodev
    # n == 0 is not a no-op: r_offsets[0] is stored, which takes a device and nothing but r_offsets
    assert call(t, 0) == nodev
    assert call(t, 0, recs=None, flags=None, views=None, ep=None, ep_echo=None, r_recs=None, work=None,
                work_bytes=0) == nodev
    assert t["untouched"]()


def test_variant_name():
    L = _lib.lib()
    for n in (0, 1, 64, 4097, 1 << 20):
        assert L.yu_rx_reply_variant_n(n) == b"k_reply" and batch.reply_variant(n) == "k_reply"
    assert batch.reply_variant() == "k_reply"


def test_python_front_end_refuses_before_the_library():
    cpu = torch.zeros((4, 32), dtype=torch.uint8)
    with pytest.raises(TypeError):
        batch.reply_datagrams(cpu, torch.zeros((4, 2), dtype=torch.int64), torch.zeros(4, dtype=torch.int32), 3)
    with pytest.raises(TypeError):
        batch.echo_datagrams(torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64),
                             torch.zeros(256, dtype=torch.uint8), 1)
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda:0")
    recs = torch.zeros((4, 32), dtype=torch.uint8, device=dev)
    views = torch.zeros((4, 2), dtype=torch.int64, device=dev)
    ep = torch.zeros(4, dtype=torch.uint32, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        batch.reply_datagrams(recs[:, :31].contiguous(), views, ep, 3)                    # shape
    with pytest.raises(ValueError):
        batch.reply_datagrams(recs, views[:3], ep, 3)
    with pytest.raises(TypeError):
        batch.reply_datagrams(recs, views.to(torch.int32), ep, 3)
    with pytest.raises(ValueError):
        batch.reply_datagrams(recs, views, None, 3)                                       # UDP echo needs ep
    with pytest.raises(ValueError):
        batch.reply_datagrams(recs, views, ep, 3, what=4)
    for m in (-1, MAX_M + 1):
        with pytest.raises(ValueError):
            batch.reply_datagrams(recs, views, ep, m)
    with pytest.raises(ValueError):
        batch.reply_datagrams(recs, views, ep, 3, need=1 << 16)
    with pytest.raises(ValueError):
        batch.reply_datagrams(recs, views, ep, 3, ep_echo=torch.zeros(4, dtype=torch.uint8, device=dev))  # m bytes
    with pytest.raises(ValueError):
        batch.reply_datagrams(recs, views, ep, 3, r_offsets=torch.zeros(4, **i64))       # n + 1
    with pytest.raises(ValueError):
        batch.reply_datagrams(recs, views, ep, 3, r_records=torch.zeros((3, 32), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        batch.reply_datagrams(recs, views, ep, 3, work=torch.zeros(8, dtype=torch.uint8, device=dev))  # too small
    big = torch.zeros(64 + 8, dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError):
        batch.reply_datagrams(recs, views, ep, 3, work=big[8:])                           # alignment
    with pytest.raises(ValueError):
        batch.reply_datagrams(recs, views, ep, 3, r_records=recs)                         # overlaps what is read
