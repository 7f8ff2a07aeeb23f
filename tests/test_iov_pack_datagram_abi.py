"""The packing whole-datagram scatter-gather calls at the C-ABI boundary
(include/yucsum.h, yu_csum_pack_iov_datagram / yu_csum_pack_fill_iov_datagram /
yu_iov_pack_datagram_variant_n): exported and declared, every documented YU_EINVAL
returned before any device work, YU_ENODEV without a device, the empty batch, the
kernels yu::plan_wave names for the four datagram modes (and the rows it keeps
for the others), and what the Python front end refuses. CPU only: no call here
reaches a device (the arguments are refused first, or there is no device)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import wave_plan
from yustack_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "yucsum.h")
NAMES = ("yu_csum_pack_iov_datagram", "yu_csum_pack_fill_iov_datagram", "yu_iov_pack_datagram_variant_n")
RAW, UDP, TCP, IPV4, ICMP, VERIFY_IPV4, VERIFY_TCP, VERIFY_UDP, VERIFY_RX, TX_DATAGRAM = range(10)
WHOLE_PACKET = (RAW, UDP, TCP, ICMP, VERIFY_TCP, VERIFY_UDP)
DATAGRAM = (IPV4, VERIFY_IPV4, VERIFY_RX, TX_DATAGRAM)
FILL = (IPV4, TX_DATAGRAM)


def test_symbols_exported_and_declared():
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert re.search(rf" T {name}$", nm, flags=re.M), name
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None
    assert L.yu_abi_version() == 1
    # the header no longer sends the datagram modes to a second call on the copy
    assert "not taken yet" not in open(HEADER).read()
    hpp = open(os.path.join(ROOT, "include", "yustack", "checksum.hpp")).read()
    assert "PackIovDatagram(" in hpp and "PackFillIovDatagram(" in hpp


@pytest.fixture
def tables():
    buf = (ctypes.c_uint8 * 256)()
    dst = (ctypes.c_uint8 * 256)()
    out = (ctypes.c_uint16 * 16)()
    p = ctypes.addressof(buf)
    iov = (_lib.YuIovec * 4)(*[_lib.YuIovec(p + 32 * i, 32) for i in range(4)])
    first = (ctypes.c_uint64 * 5)(0, 1, 2, 3, 4)
    doff = (ctypes.c_uint64 * 6)(0, 32, 64, 96, 128, 0)
    yield (ctypes.addressof(iov), ctypes.addressof(first), ctypes.addressof(dst), ctypes.addressof(doff),
           ctypes.addressof(out))
    del buf, dst, out, iov, first, doff


def test_every_einval_precedes_device_work(tables):
    """Each refused argument returns YU_EINVAL, whether or not a device is present
    (nothing is launched: the pointers here are host memory); the checks that do not
    need n for an empty batch too."""
    L = _lib.lib()
    v, f, d, do, o = tables
    E = _lib.YU_EINVAL
    both = (L.yu_csum_pack_iov_datagram, L.yu_csum_pack_fill_iov_datagram)
    for fn in both:
        for n in (4, 0):
            for bad in (-1, 10, 99) + WHOLE_PACKET:
                assert fn(v, f, n, bad, d, do, o, None) == E  # [mode]
    for m in (VERIFY_IPV4, VERIFY_RX):
        for n in (4, 0):
            assert L.yu_csum_pack_fill_iov_datagram(v, f, n, m, d, do, o, None) == E  # [fill-mode]
    for m in DATAGRAM:
        assert L.yu_csum_pack_iov_datagram(v, f, 4, m, d, do, None, None) == E  # [out]
    for fn, modes in ((both[0], DATAGRAM), (both[1], FILL)):
        for m in modes:
            for n in (4, 0):
                assert fn(v, f, n, m, d, do, o + 1, None) == E   # [side-align] out
            assert fn(None, f, 4, m, d, do, o, None) == E     # [data] views
            assert fn(v, f, 4, m, None, do, o, None) == E     # [data] dst
            assert fn(v, None, 4, m, d, do, o, None) == E     # [offsets]
            assert fn(v, f + 4, 4, m, d, do, o, None) == E    # [offsets] first_iov alignment
            assert fn(v + 4, f, 4, m, d, do, o, None) == E    # [offsets] views alignment
            assert fn(v, f, 4, m, d, None, o, None) == E      # [offsets] dst_offsets
            assert fn(v, f, 4, m, d, do + 4, o, None) == E    # [offsets] dst_offsets alignment
    assert bytes(ctypes.string_at(d, 256)) == bytes(256)


def test_empty_batch_is_a_no_op(tables):
    L = _lib.lib()
    v, f, d, do, o = tables
    for m in DATAGRAM:
        assert L.yu_csum_pack_iov_datagram(v, f, 0, m, d, do, o, None) == _lib.YU_OK
        assert L.yu_csum_pack_iov_datagram(None, None, 0, m, None, None, None, None) == _lib.YU_OK
    for m in FILL:
        assert L.yu_csum_pack_fill_iov_datagram(None, None, 0, m, None, None, None, None) == _lib.YU_OK
    assert bytes(ctypes.string_at(d, 256)) == bytes(256)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_valid_calls_fail_without_gpu(tables):
    L = _lib.lib()
    v, f, d, do, o = tables
    for m in DATAGRAM:
        assert L.yu_csum_pack_iov_datagram(v, f, 4, m, d + 1, do, o, None) == _lib.YU_ENODEV  # any dst alignment
    for m in FILL:
        assert L.yu_csum_pack_fill_iov_datagram(v, f, 4, m, d, do, None, None) == _lib.YU_ENODEV  # NULL out is fine


def test_variant_names():
    L = _lib.lib()
    for n in (1, 64, 4097, 1 << 20):
        for m in DATAGRAM:
            assert L.yu_iov_pack_datagram_variant_n(m, n, 0) == b"k_pack<4,dg>"
            assert batch.iov_pack_datagram_variant(m, n) == "k_pack<4,dg>"
            assert L.yu_iov_datagram_variant_n(m, n, 0) == b"k_iov<4,dg>"  # the in-place calls keep theirs
            assert L.yu_iov_pack_variant_n(m, n, 0) == b"" and L.yu_iov_pack_variant_n(m, n, 1) == b""
        for m in FILL:
            assert L.yu_iov_pack_datagram_variant_n(m, n, 1) == b"k_pack<4,dg,fill>"
            assert batch.iov_pack_datagram_variant(m, n, fill=True) == "k_pack<4,dg,fill>"
        for m in (VERIFY_IPV4, VERIFY_RX):
            assert L.yu_iov_pack_datagram_variant_n(m, n, 1) == b""
        for m in WHOLE_PACKET + (-1, 10, 99):
            assert L.yu_iov_pack_datagram_variant_n(m, n, 0) == b""
            assert L.yu_iov_pack_datagram_variant_n(m, n, 1) == b""


def test_python_front_end_refuses_before_the_library():
    cpu = torch.zeros(64, dtype=torch.uint8)
    idx = torch.zeros(1, dtype=torch.int64)
    for mode in ("raw", "udp", "tcp", "icmp", "verify_tcp", "verify_udp"):
        with pytest.raises(ValueError):
            batch.pack_iov_datagrams([cpu], idx, idx, idx, idx, mode)
    for mode in ("verify_ipv4", "verify_rx"):
        with pytest.raises(ValueError):
            batch.pack_iov_datagrams([cpu], idx, idx, idx, idx, mode, fill=True)
    with pytest.raises(TypeError):
        batch.pack_iov_datagrams([cpu], idx, idx, idx, torch.zeros(2, dtype=torch.int64), "verify_rx")  # CPU tensors
    with pytest.raises(ValueError):
        batch.pack_iov_datagrams([], idx, idx, idx, idx, "tx_datagram")
    for mode in ("ipv4", "verify_ipv4", "verify_rx", "tx_datagram"):  # pack_iov still refuses them
        with pytest.raises(ValueError):
            batch.pack_iov([cpu], idx, idx, idx, idx, mode)


@pytest.fixture(scope="module")
def pack_plan():
    return lambda cases, env=None: (wave_plan.pack_and_iov(cases, env), wave_plan.enum())


def test_enum_values_keep_their_meaning(pack_plan):
    _, enum = pack_plan([])
    assert enum[:8] == [0, 1, 2, 3, 4, 5, 6, 7]
    assert enum[8:] == [8, 9, 10]  # k_build4, k_split4, then the count


def test_plan_rows_for_the_datagram_modes(pack_plan):
    for m in DATAGRAM:
        for fill in ((0, 1) if m in FILL else (0,)):
            rows, _ = pack_plan([(n, m, fill, cus) for n in (1, 4, 5, 4097, 1 << 20) for cus in (64, 256, 304)])
            for pack, iov in rows:
                assert iov[0] == 2 + fill and iov[1] == 2 and iov[3] == ("k_iov<4,dg,fill>" if fill else "k_iov<4,dg>")
                assert pack[0] == 6 + fill and pack[3] == ("k_pack<4,dg,fill>" if fill else "k_pack<4,dg>")
                assert pack[1:3] == iov[1:3]  # the in-place calls' load policy and grid
            assert [p[2] for p, _ in rows[-3:]] == [64 * 64, 256 * 64, 304 * 64]
            assert [p[2] for p, _ in rows[0:12:3]] == [1, 1, 2, 1025]  # a wave per packet, four per block
    # the whole-packet modes keep their rows
    rows, _ = pack_plan([(1 << 20, m, 0, 256) for m in WHOLE_PACKET] + [(1 << 20, TCP, 1, 256)])
    assert [p[0] for p, _ in rows] == [4] * 6 + [5]
    assert [p[3] for p, _ in rows] == ["k_pack<4>"] * 6 + ["k_pack<4,fill>"]


def test_plan_honours_the_knobs_behind_the_gate(pack_plan):
    case = [(1 << 20, TX_DATAGRAM, 1, 256)]
    (k, pol, blocks, name), _ = pack_plan(case)[0][0]
    assert pack_plan(case, {"YU_NT": "0", "YU_BLOCKS_PER_CU": "1"})[0][0][0] == (k, pol, blocks, name)  # gate closed
    tuned, _ = pack_plan(case, {"YU_TUNING": "1", "YU_NT": "0", "YU_BLOCKS_PER_CU": "1"})[0][0]
    assert tuned == (k, 0, 256, name)
