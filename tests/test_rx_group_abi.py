"""yu_rx_group at the C-ABI boundary (include/yucsum.h: yu_rx_group_workspace_bytes,
yu_rx_group, yu_rx_group_variant_n): exported and declared, the workspace formula of the
header, yu::plan_group's passes, digits and regions, every documented YU_EINVAL returned
before any device work (those that do not need n also with n = 0), YU_ENODEV without a
device, the variant name, and what the Python front end refuses. CPU only: no call here
reaches a device: the arguments are refused first, or there is no device. (A valid call
with n = 0 is NOT among them where a device is present: it stores the empty CSR.)"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import group_plan
from yustack_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "yucsum.h")
NAMES = ("yu_rx_group_workspace_bytes", "yu_rx_group", "yu_rx_group_variant_n")
E = _lib.YU_EINVAL
MAX_M = 1 << 24


def test_symbols_exported_and_declared():
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert re.search(rf" T {name}$", nm, flags=re.M), name
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None
    assert len(L.yu_rx_group.argtypes) == 11
    assert L.yu_abi_version() == 1


def r16(x):
    return (x + 15) & ~15


def header_formula(n, m):
    """The formula in yu_rx_group's header comment."""
    if m > MAX_M or n >= 1 << 32:
        return 0
    b = m.bit_length()
    passes = max(1, -(-b // 8))
    d = max(1, -(-b // passes))
    blocks = min(-(-n // 1024), 8192)
    total = r16(4 * (1 << d) * blocks) + r16(8 * -(-max((1 << d) * blocks, m + 2, n + 1) // 2048))
    if passes > 1:
        total += r16(4 * (m + 1)) + r16(8 * n)
    if passes > 2:
        total += r16(8 * n)
    return total


NS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2051, 9189, 4095, 4096, 4097, 1 << 20, (1 << 23) - 1, 1 << 23,
      (1 << 23) + 1, 1 << 24, (1 << 31) - 1, (1 << 32) - 1)
MS = (0, 1, 255, 256, 65535, 65536, MAX_M - 1, MAX_M)


def test_workspace_bytes_is_the_header_formula_and_the_plan():
    L = _lib.lib()
    cases = [(n, m) for n in NS for m in MS]
    plans = group_plan.plans([(n, m, 256) for n, m in cases])
    for (n, m), p in zip(cases, plans):
        got = L.yu_rx_group_workspace_bytes(n, m)
        assert got == header_formula(n, m) == p.bytes == batch.group_workspace_bytes(n, m), (n, m)
        assert got > 0 and got % 16 == 0


def test_workspace_bytes_is_monotone_in_n_and_zero_where_refused():
    L = _lib.lib()
    fine = sorted(set(NS) | {k * (1 << 23) + d for k in range(1, 40) for d in (-1, 0, 1)} | set(range(0, 20000, 997)))
    for m in MS:
        sizes = [L.yu_rx_group_workspace_bytes(n, m) for n in fine]
        assert sizes == sorted(sizes), m
    for n in (0, 5, 1 << 20):
        assert L.yu_rx_group_workspace_bytes(n, MAX_M + 1) == 0
        assert L.yu_rx_group_workspace_bytes(n, (1 << 64) - 1) == 0
    for m in (0, 5, MAX_M):
        assert L.yu_rx_group_workspace_bytes(1 << 32, m) == 0
        assert L.yu_rx_group_workspace_bytes((1 << 64) - 1, m) == 0


def test_plan_passes_and_digit_bits():
    """Keys are 0 .. m: ceil(bitlen(m) / 8) passes on digits of equal width."""
    ms = (0, 255, 256, 65535, 65536, MAX_M - 1, MAX_M)
    rows = group_plan.plans([(1 << 20, m, 256) for m in ms])
    assert [(p.passes, p.digit_bits) for p in rows] == [(1, 1), (1, 8), (2, 5), (2, 8), (3, 6), (3, 8), (4, 7)]
    assert [p.name for p in rows] == ["k_group<1>", "k_group<1>", "k_group<2>", "k_group<2>", "k_group<3>",
                                      "k_group<3>", "k_group<4>"]
    for p, m in zip(rows, ms):
        assert p.passes * p.digit_bits >= m.bit_length() and p.digit_bits <= 8
    refused = group_plan.plans([(1 << 20, MAX_M + 1, 256), (1 << 32, 5, 256)])
    assert all(p.passes == 0 and p.bytes == 0 and p.name == "none" for p in refused)


def test_plan_tiles_and_grids():
    rows = group_plan.plans([(n, 1, 256) for n in (1, 1024, 1025, 1 << 23, (1 << 23) + 1, (1 << 32) - 1)])
    assert [(p.tile, p.blocks) for p in rows] == [(1024, 1), (1024, 1), (1024, 2), (1024, 8192), (2048, 4097),
                                                  (1024 * 512, 8192)]
    for p in rows:
        assert p.tile % 256 == 0 and 1 <= p.blocks <= 8192
    # only the lane-per-element grid depends on the device and, behind the gate, on the knobs
    a, b = group_plan.plans([(1 << 20, 300, 64), (1 << 20, 300, 304)])
    assert a.lane_blocks == 64 * 8 and b.lane_blocks == 304 * 8
    assert a._replace(lane_blocks=0) == b._replace(lane_blocks=0)
    env = {"YU_TUNING": "1", "YU_BLOCKS_PER_CU": "2"}
    c = group_plan.plans([(1 << 20, 300, 64)], env)[0]
    assert c.lane_blocks == 128 and c._replace(lane_blocks=0) == a._replace(lane_blocks=0)
    assert group_plan.plans([(1 << 20, 300, 64)], {"YU_BLOCKS_PER_CU": "2"})[0] == a   # gate closed


def test_plan_regions_are_disjoint_aligned_and_inside():
    cases = [(n, m, 256) for n in NS for m in MS]
    for (n, m, _), p in zip(cases, group_plan.plans(cases)):
        regions = [r for r in (p.hist, p.sums, p.count, p.pair0, p.pair1) if r[1]]
        end = 0
        for off, size in sorted(regions):
            assert off % 16 == 0 and off >= end, (n, m)
            end = off + size
        assert end <= p.bytes, (n, m)
        radix = 1 << p.digit_bits
        assert p.hist[1] >= 4 * radix * p.blocks                       # the grid's histogram fits
        assert p.sums[1] >= 8 * -(-max(radix * p.blocks, m + 2, n + 1) // 2048)
        assert p.count[1] >= (4 * (m + 1) if p.passes > 1 else 0)
        assert p.pair0[1] >= (8 * n if p.passes > 1 else 0) and p.pair1[1] >= (8 * n if p.passes > 2 else 0)


@pytest.fixture
def bufs():
    ep = (ctypes.c_uint32 * 8)()
    views = (_lib.YuIovec * 8)()
    order = (ctypes.c_uint32 * 8)(*([0xA5A5A5A5] * 8))
    first = (ctypes.c_uint64 * 8)(*([0xA5A5A5A5A5A5A5A5] * 8))
    q_views = (ctypes.c_uint64 * 16)(*([0xA5A5A5A5A5A5A5A5] * 16))
    q_offsets = (ctypes.c_uint64 * 9)(*([0xA5A5A5A5A5A5A5A5] * 9))
    work = (ctypes.c_uint8 * (4096 + 32))(*([0xA5] * (4096 + 32)))
    t = dict(ep=ctypes.addressof(ep), views=ctypes.addressof(views), order=ctypes.addressof(order),
             first=ctypes.addressof(first), q_views=ctypes.addressof(q_views), q_offsets=ctypes.addressof(q_offsets),
             work=(ctypes.addressof(work) + 15) & ~15)

    def untouched():
        return all(bytes(b) == b"\xA5" * ctypes.sizeof(b) for b in (order, first, q_views, q_offsets, work))
    t["untouched"] = untouched
    yield t
    del ep, views, order, first, q_views, q_offsets, work


def call(t, n=4, m=3, work_bytes=4096, **change):
    a = dict(t, **change)
    return _lib.lib().yu_rx_group(a["ep"], n, m, a["views"], a["order"], a["first"], a["q_views"], a["q_offsets"],
                                  a["work"], work_bytes, None)


def test_every_einval_precedes_device_work(bufs):
    """Each refused argument returns YU_EINVAL, whether or not a device is present
    (nothing is launched: the pointers here are host memory), and stores nothing."""
    t = bufs
    need = _lib.lib().yu_rx_group_workspace_bytes(4, 3)
    assert 0 < need <= 4096
    # [data], each with n > 0
    assert call(t, ep=None) == E
    assert call(t, work=None) == E
    assert call(t, work_bytes=need - 1) == E
    assert call(t, work_bytes=0) == E
    for missing in ("views", "q_views", "q_offsets"):                    # one of the three missing
        assert call(t, **{missing: None}) == E, missing
    for given in ("views", "q_views", "q_offsets"):                      # one of the three alone
        assert call(t, **{k: None for k in ("views", "q_views", "q_offsets") if k != given}) == E, given
    for n in (4, 0):
        # [data], checked without n
        assert call(t, n, m=MAX_M + 1) == E
        assert call(t, n, m=(1 << 64) - 1) == E
        # [out]: first is always needed
        assert call(t, n, first=None) == E
        assert call(t, n, first=None, views=None, q_views=None, q_offsets=None) == E
        # [offsets]
        for name in ("first", "q_offsets", "views", "q_views"):
            assert call(t, n, **{name: t[name] + 4}) == E, name
        assert call(t, n, work=t["work"] + 8) == E
        # [side-align]
        assert call(t, n, ep=t["ep"] + 2) == E
        assert call(t, n, order=t["order"] + 2) == E
    for n in (1 << 32, (1 << 64) - 1):                                   # [data]: order holds 32-bit numbers
        assert call(t, n, work_bytes=(1 << 64) - 1) == E
    assert call(t, order=None) == E                                      # [out], with n > 0
    assert t["untouched"]()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_valid_calls_fail_without_gpu(bufs):
    t = bufs
    none = dict(views=None, q_views=None, q_offsets=None)
    assert call(t) == _lib.YU_ENODEV
    assert call(t, **none) == _lib.YU_ENODEV
    assert call(t, m=0) == _lib.YU_ENODEV
    assert call(t, ep=t["ep"] + 4, order=t["order"] + 4, first=t["first"] + 8, work=t["work"] + 16,
                work_bytes=4096 - 16) == _lib.YU_ENODEV
    # n == 0 is not a no-op: the empty CSR is stored, which takes a device
    assert call(t, 0) == _lib.YU_ENODEV
    assert call(t, 0, ep=None, order=None, work=None, work_bytes=0, **none) == _lib.YU_ENODEV
    assert t["untouched"]()


def test_variant_name_is_the_plan():
    L = _lib.lib()
    cases = [(n, m) for n in (0, 1, 4097, 1 << 20) for m in (0, 1, 255, 256, 65535, 65536, MAX_M)]
    for (n, m), p in zip(cases, group_plan.plans([(n, m, 256) for n, m in cases])):
        assert L.yu_rx_group_variant_n(n, m).decode() == p.name == batch.group_variant(n, m) == f"k_group<{p.passes}>"
    assert L.yu_rx_group_variant_n(5, MAX_M + 1) == b"none" and L.yu_rx_group_variant_n(1 << 32, 5) == b"none"
    assert batch.group_variant() == "k_group<1>"


def test_python_front_end_refuses_before_the_library():
    with pytest.raises(TypeError):
        batch.group_datagrams(torch.zeros(4, dtype=torch.int32), 3)                      # a CPU tensor
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda:0")
    ep = torch.zeros(4, dtype=torch.uint32, device=dev)
    views = torch.zeros((4, 2), dtype=torch.int64, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    with pytest.raises(TypeError):
        batch.group_datagrams(ep.view(torch.uint8), 3)                                   # dtype
    with pytest.raises(ValueError):
        batch.group_datagrams(ep.reshape(2, 2), 3)                                       # shape
    for m in (-1, MAX_M + 1):
        with pytest.raises(ValueError):
            batch.group_datagrams(ep, m)
    with pytest.raises(ValueError):
        batch.group_datagrams(ep, 3, q_offsets=torch.zeros(5, **i64))                    # goes with views
    with pytest.raises(ValueError):
        batch.group_datagrams(ep, 3, views=views[:3])
    with pytest.raises(TypeError):
        batch.group_datagrams(ep, 3, views=views.to(torch.int32))
    with pytest.raises(TypeError):
        batch.group_datagrams(ep, 3, order=torch.zeros(4, **i64))
    with pytest.raises(ValueError):
        batch.group_datagrams(ep, 3, order=torch.zeros(5, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        batch.group_datagrams(ep, 3, first=torch.zeros(4, **i64))                        # m + 2
    with pytest.raises(TypeError):
        batch.group_datagrams(ep, 3, first=torch.zeros(5, dtype=torch.int64))            # a CPU tensor
    with pytest.raises(ValueError):
        batch.group_datagrams(ep, 3, views=views, q_views=torch.zeros((4, 3), **i64))
    with pytest.raises(ValueError):
        batch.group_datagrams(ep, 3, views=views, q_offsets=torch.zeros(4, **i64))       # n + 1
    with pytest.raises(ValueError):
        batch.group_datagrams(ep, 3, work=torch.zeros(16, dtype=torch.uint8, device=dev))  # too small
    big = torch.zeros(8192 + 8, dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError):
        batch.group_datagrams(ep, 3, work=big[8:])                                       # alignment
    with pytest.raises(ValueError):
        batch.group_datagrams(ep, 3, order=ep.view(torch.int32))                         # overlaps ep
    both = torch.zeros(12, **i64)
    with pytest.raises(ValueError):
        batch.group_datagrams(ep, 3, first=both[:5], views=views, q_offsets=both[4:9])   # overlap each other
