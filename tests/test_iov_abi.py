"""The scatter-gather device calls at the C-ABI boundary (include/yucsum.h,
yu_csum_batch_iov / yu_csum_fill_iov / yu_iov_variant_n): exported and declared, every
documented YU_EINVAL returned before any device work, the kernel yu::plan_wave names,
and the build-level bounds of the k_iov instantiations. CPU only: no call here
reaches a device (the arguments are refused first, or there is no device)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import wave_plan
from test_build import resource_usage  # noqa: F401 - the module-scoped compile fixture
from yustack_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "yucsum.h")
NAMES = ("yu_csum_batch_iov", "yu_csum_fill_iov", "yu_iov_variant_n")
RAW, UDP, TCP, IPV4, ICMP, VERIFY_IPV4, VERIFY_TCP, VERIFY_UDP, VERIFY_RX, TX_DATAGRAM = range(10)
SUPPORTED = (RAW, UDP, TCP, ICMP, VERIFY_TCP, VERIFY_UDP)
REFUSED = (IPV4, VERIFY_IPV4, VERIFY_RX, TX_DATAGRAM)


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
    out = (ctypes.c_uint16 * 8)()
    p = ctypes.addressof(buf)
    iov = (_lib.YuIovec * 4)(*[_lib.YuIovec(p + 32 * i, 32) for i in range(4)])
    first = (ctypes.c_uint64 * 5)(0, 1, 2, 3, 4)
    yield ctypes.addressof(iov), ctypes.addressof(first), p, ctypes.addressof(out)
    del buf, out, iov, first


def test_every_einval_precedes_device_work(tables):
    """The table of the header: each refused argument returns YU_EINVAL, whether or
    not a device is present (nothing is launched: the pointers here are host memory)."""
    L = _lib.lib()
    v, f, p, o = tables
    E = _lib.YU_EINVAL
    for fn in (L.yu_csum_batch_iov, L.yu_csum_fill_iov):
        for bad in (-1, 10, 99):
            assert fn(v, f, 4, bad, None, 0, None, o, None) == E  # [mode]
    for m in REFUSED:
        assert L.yu_csum_batch_iov(v, f, 4, m, None, 0, None, o, None) == E  # [mode]
        assert L.yu_csum_fill_iov(v, f, 4, m, None, 0, None, o, None) == E   # [fill-mode]
    assert L.yu_csum_batch_iov(v, f, 4, RAW, None, 0, None, None, None) == E  # [out]
    for m in (RAW, VERIFY_TCP, VERIFY_UDP):
        assert L.yu_csum_fill_iov(v, f, 4, m, None, 0, None, o, None) == E  # [fill-mode]
    for fn, m in ((L.yu_csum_batch_iov, RAW), (L.yu_csum_fill_iov, UDP)):
        assert fn(v, f, 4, m, p + 1, 0, None, o, None) == E   # [side-align] initial_arr
        assert fn(v, f, 4, m, None, 0, p + 2, o, None) == E   # [side-align] addrs
        assert fn(v, f, 4, m, None, 0, None, o + 1, None) == E  # [side-align] out
        assert fn(None, f, 4, m, None, 0, None, o, None) == E  # [data]
        assert fn(v, None, 4, m, None, 0, None, o, None) == E  # [offsets]
        assert fn(v, f + 4, 4, m, None, 0, None, o, None) == E  # [offsets] first_iov alignment
        assert fn(v + 4, f, 4, m, None, 0, None, o, None) == E  # [offsets] views alignment
    # refused even for an empty batch
    assert L.yu_csum_batch_iov(v, f, 0, IPV4, None, 0, None, o, None) == E
    assert L.yu_csum_fill_iov(v, f, 0, RAW, None, 0, None, o, None) == E


def test_empty_batch_is_a_no_op(tables):
    L = _lib.lib()
    v, f, p, o = tables
    for m in SUPPORTED:
        assert L.yu_csum_batch_iov(v, f, 0, m, None, 0, None, o, None) == _lib.YU_OK
        assert L.yu_csum_batch_iov(None, None, 0, m, None, 0, None, None, None) == _lib.YU_OK
    for m in (UDP, TCP, ICMP):
        assert L.yu_csum_fill_iov(None, None, 0, m, None, 0, None, None, None) == _lib.YU_OK


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_valid_calls_fail_without_gpu(tables):
    L = _lib.lib()
    v, f, p, o = tables
    for m in SUPPORTED:
        assert L.yu_csum_batch_iov(v, f, 4, m, None, 0, None, o, None) == _lib.YU_ENODEV
    for m in (UDP, TCP, ICMP):
        assert L.yu_csum_fill_iov(v, f, 4, m, None, 0, None, None, None) == _lib.YU_ENODEV  # NULL out is fine


def test_variant_names():
    L = _lib.lib()
    for n in (1, 64, 4097, 1 << 20):
        for m in SUPPORTED:
            assert L.yu_iov_variant_n(m, n, 0).decode().startswith("k_iov<")
            assert batch.iov_variant(m, n) == L.yu_iov_variant_n(m, n, 0).decode()
        for m in (UDP, TCP, ICMP):
            name = L.yu_iov_variant_n(m, n, 1).decode()
            assert name.startswith("k_iov<") and "fill" in name
            assert batch.iov_variant(m, n, fill=True) == name
        for m in (RAW, VERIFY_TCP, VERIFY_UDP):
            assert L.yu_iov_variant_n(m, n, 1) == b""
        for m in REFUSED + (-1, 10, 99):
            assert L.yu_iov_variant_n(m, n, 0) == b"" and L.yu_iov_variant_n(m, n, 1) == b""


def test_python_front_end_refuses_before_the_library():
    cpu = torch.zeros(64, dtype=torch.uint8)
    idx = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(TypeError):
        batch.checksum_iov([cpu], idx, idx, idx, torch.zeros(2, dtype=torch.int64), "raw")
    with pytest.raises(ValueError):
        batch.checksum_iov([cpu], idx, idx, idx, idx, "ipv4")
    with pytest.raises(ValueError):
        batch.checksum_iov([cpu], idx, idx, idx, idx, "raw", fill=True)
    with pytest.raises(ValueError):
        batch.checksum_iov([], idx, idx, idx, idx, "raw")


@pytest.fixture(scope="module")
def iov_plan():
    return lambda cases, env=None: wave_plan.plans("iov", cases, env)


def test_plan_iov_scales_with_the_cu_count(iov_plan):
    for m in SUPPORTED:
        for fill in ((0, 1) if m in (UDP, TCP, ICMP) else (0,)):
            big = iov_plan([(1 << 20, m, fill, cus) for cus in (64, 256, 304)])
            assert len({(k, pol, name) for k, pol, _, name in big}) == 1  # the same kernel everywhere
            assert big[0][3] == _lib.lib().yu_iov_variant_n(m, 1 << 20, fill).decode()
            b64, b256, b304 = (row[2] for row in big)
            assert b256 == 4 * b64 and b304 * 64 == 304 * b64 and b64 % 64 == 0  # blocks per CU
    # a wave per packet, four waves per block: a small batch gets no more blocks than that
    assert [row[2] for row in iov_plan([(n, RAW, 0, 256) for n in (1, 4, 5, 4097)])] == [1, 1, 2, 1025]


def test_plan_iov_honours_the_knobs_behind_the_gate(iov_plan):
    case = [(1 << 20, TCP, 0, 256)]
    k, pol, blocks, _ = iov_plan(case)[0]
    assert iov_plan(case, {"YU_NT": "0", "YU_BLOCKS_PER_CU": "1"})[0][:3] == (k, pol, blocks)  # gate closed
    tuned = iov_plan(case, {"YU_TUNING": "1", "YU_NT": "0", "YU_BLOCKS_PER_CU": "1"})[0]
    assert tuned[1] == 0 and tuned[2] == 256 and tuned[0] == k
    assert iov_plan(case, {"YU_TUNING": "1", "YU_NT": "1"})[0][1] == 1


def test_k_iov_build_bounds(resource_usage):  # noqa: F811
    """The bounds tests/test_build.py holds every kernel to, asserted for k_iov by
    name: it is compiled, uses no scratch, spills no vector register and at most 13
    scalar ones, and keeps at least 4 waves per SIMD."""
    mine = {name: ru for name, ru in resource_usage.items() if "k_iov" in name}
    assert len(mine) >= 2, sorted(resource_usage)
    for name, ru in mine.items():
        assert ru.get("ScratchSize [bytes/lane]") == "0", (name, ru)
        assert ru.get("VGPRs Spill") == "0", (name, ru)
        assert int(ru.get("SGPRs Spill", "99")) <= 13, (name, ru)
        assert int(ru.get("Occupancy [waves/SIMD]", "0")) >= 4, (name, ru)
