"""The whole-datagram scatter-gather device calls at the C-ABI boundary (include/yucsum.h,
yu_csum_batch_iov_datagram / yu_csum_fill_iov_datagram / yu_iov_datagram_variant_n):
exported and declared, every documented YU_EINVAL returned before any device work, the
kernels yu::plan_wave names for the four datagram modes, and unchanged rows for the six
whole-packet modes. CPU only: no call here reaches a device (the arguments are refused
first, or there is no device)."""
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
NAMES = ("yu_csum_batch_iov_datagram", "yu_csum_fill_iov_datagram", "yu_iov_datagram_variant_n")
RAW, UDP, TCP, IPV4, ICMP, VERIFY_IPV4, VERIFY_TCP, VERIFY_UDP, VERIFY_RX, TX_DATAGRAM = range(10)
DATAGRAM = (IPV4, VERIFY_IPV4, VERIFY_RX, TX_DATAGRAM)
FILL = (IPV4, TX_DATAGRAM)
WHOLE_PACKET = (RAW, UDP, TCP, ICMP, VERIFY_TCP, VERIFY_UDP)


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


@pytest.fixture
def tables():
    buf = (ctypes.c_uint8 * 256)()
    out = (ctypes.c_uint16 * 16)()
    p = ctypes.addressof(buf)
    iov = (_lib.YuIovec * 4)(*[_lib.YuIovec(p + 32 * i, 32) for i in range(4)])
    first = (ctypes.c_uint64 * 5)(0, 1, 2, 3, 4)
    yield ctypes.addressof(iov), ctypes.addressof(first), p, ctypes.addressof(out)
    del buf, out, iov, first


def test_every_einval_precedes_device_work(tables):
    """Each refused argument returns YU_EINVAL, whether or not a device is present
    (nothing is launched: the pointers here are host memory), for an empty batch too."""
    L = _lib.lib()
    v, f, p, o = tables
    E = _lib.YU_EINVAL
    both = (L.yu_csum_batch_iov_datagram, L.yu_csum_fill_iov_datagram)
    for fn in both:
        for n in (4, 0):
            for bad in (-1, 10, 99) + WHOLE_PACKET:
                assert fn(v, f, n, bad, o, None) == E  # [mode]
    for m in (VERIFY_IPV4, VERIFY_RX):
        for n in (4, 0):
            assert L.yu_csum_fill_iov_datagram(v, f, n, m, o, None) == E  # [fill-mode]
    for m in DATAGRAM:
        assert L.yu_csum_batch_iov_datagram(v, f, 4, m, None, None) == E  # [out]
    for fn, modes in ((both[0], DATAGRAM), (both[1], FILL)):
        for m in modes:
            assert fn(v, f, 4, m, o + 1, None) == E      # [side-align] out
            assert fn(v, f, 0, m, o + 1, None) == E      # ... for an empty batch too
            assert fn(None, f, 4, m, o, None) == E       # [data]
            assert fn(v, None, 4, m, o, None) == E       # [offsets]
            assert fn(v, f + 4, 4, m, o, None) == E      # [offsets] first_iov alignment
            assert fn(v + 4, f, 4, m, o, None) == E      # [offsets] views alignment


def test_empty_batch_is_a_no_op(tables):
    L = _lib.lib()
    v, f, p, o = tables
    for m in DATAGRAM:
        assert L.yu_csum_batch_iov_datagram(v, f, 0, m, o, None) == _lib.YU_OK
        assert L.yu_csum_batch_iov_datagram(None, None, 0, m, None, None) == _lib.YU_OK
    for m in FILL:
        assert L.yu_csum_fill_iov_datagram(None, None, 0, m, None, None) == _lib.YU_OK


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_valid_calls_fail_without_gpu(tables):
    L = _lib.lib()
    v, f, p, o = tables
    for m in DATAGRAM:
        assert L.yu_csum_batch_iov_datagram(v, f, 4, m, o, None) == _lib.YU_ENODEV
    for m in FILL:
        assert L.yu_csum_fill_iov_datagram(v, f, 4, m, None, None) == _lib.YU_ENODEV  # NULL out is fine


def test_variant_names():
    L = _lib.lib()
    for n in (1, 64, 4097, 1 << 20):
        for m in DATAGRAM:
            name = L.yu_iov_datagram_variant_n(m, n, 0).decode()
            assert name.startswith("k_iov<") and "dg" in name and "fill" not in name
            assert batch.iov_datagram_variant(m, n) == name
            assert L.yu_iov_variant_n(m, n, 0) == b""  # the whole-packet calls still refuse the mode
        for m in FILL:
            name = L.yu_iov_datagram_variant_n(m, n, 1).decode()
            assert name.startswith("k_iov<") and "dg" in name and "fill" in name
            assert batch.iov_datagram_variant(m, n, fill=True) == name
        for m in (VERIFY_IPV4, VERIFY_RX):
            assert L.yu_iov_datagram_variant_n(m, n, 1) == b""
        for m in WHOLE_PACKET + (-1, 10, 99):
            assert L.yu_iov_datagram_variant_n(m, n, 0) == b"" and L.yu_iov_datagram_variant_n(m, n, 1) == b""


def test_python_front_end_refuses_before_the_library():
    cpu = torch.zeros(64, dtype=torch.uint8)
    idx = torch.zeros(1, dtype=torch.int64)
    for mode in ("raw", "udp", "tcp", "icmp", "verify_tcp", "verify_udp"):
        with pytest.raises(ValueError):
            batch.checksum_iov_datagrams([cpu], idx, idx, idx, idx, mode)
    for mode in ("verify_ipv4", "verify_rx"):
        with pytest.raises(ValueError):
            batch.checksum_iov_datagrams([cpu], idx, idx, idx, idx, mode, fill=True)
    with pytest.raises(TypeError):
        batch.checksum_iov_datagrams([cpu], idx, idx, idx, torch.zeros(2, dtype=torch.int64), "verify_rx")
    with pytest.raises(ValueError):
        batch.checksum_iov_datagrams([], idx, idx, idx, idx, "tx_datagram")
    # the whole-packet front end is as it was
    with pytest.raises(ValueError):
        batch.checksum_iov([cpu], idx, idx, idx, idx, "verify_rx")


@pytest.fixture(scope="module")
def iov_plan():
    return lambda cases, env=None: wave_plan.plans("iov", cases, env)


def test_plan_iov_names_the_datagram_kernels(iov_plan):
    old = iov_plan([(1 << 20, m, fill, 256) for m in WHOLE_PACKET for fill in (0, 1)])
    assert {row[3] for row in old} == {"k_iov<4>", "k_iov<4,fill>"}
    for (k, pol, blocks, name), fill in zip(old, [0, 1] * len(WHOLE_PACKET)):
        # the rows of the six whole-packet modes: kernel, policy and blocks as before
        assert (k, pol, blocks, name) == (fill, 2, 256 * 64, "k_iov<4,fill>" if fill else "k_iov<4>")
    for m in DATAGRAM:
        for fill in ((0, 1) if m in FILL else (0,)):
            big = iov_plan([(1 << 20, m, fill, cus) for cus in (64, 256, 304)])
            assert len({(k, pol, name) for k, pol, _, name in big}) == 1
            assert big[0][0] == 2 + fill and big[0][1] == 2
            assert big[0][3] == ("k_iov<4,dg,fill>" if fill else "k_iov<4,dg>")
            assert big[0][3] == _lib.lib().yu_iov_datagram_variant_n(m, 1 << 20, fill).decode()
            assert [row[2] for row in big] == [64 * 64, 256 * 64, 304 * 64]  # k_iov's grid
    for m in DATAGRAM:  # a wave per packet, four waves per block
        assert [row[2] for row in iov_plan([(n, m, 0, 256) for n in (1, 4, 5, 4097)])] == [1, 1, 2, 1025]
        assert iov_plan([(n, m, 0, 256) for n in (1, 5, 4097)]) != iov_plan([(n, RAW, 0, 256) for n in (1, 5, 4097)])
        assert [r[1:3] for r in iov_plan([(n, m, 0, 256) for n in (1, 5, 4097)])] == \
            [r[1:3] for r in iov_plan([(n, RAW, 0, 256) for n in (1, 5, 4097)])]


def test_plan_iov_honours_the_knobs_behind_the_gate(iov_plan):
    case = [(1 << 20, VERIFY_RX, 0, 256)]
    k, pol, blocks, _ = iov_plan(case)[0]
    assert iov_plan(case, {"YU_NT": "0", "YU_BLOCKS_PER_CU": "1"})[0][:3] == (k, pol, blocks)  # gate closed
    tuned = iov_plan(case, {"YU_TUNING": "1", "YU_NT": "0", "YU_BLOCKS_PER_CU": "1"})[0]
    assert tuned[1] == 0 and tuned[2] == 256 and tuned[0] == k
    assert iov_plan(case, {"YU_TUNING": "1", "YU_NT": "1"})[0][1] == 1
