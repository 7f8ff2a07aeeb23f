"""The in-place receiver at the C-ABI boundary (include/yucsum.h, yu_rx_parse_ragged /
yu_rx_parse_variant_n): exported and declared, every documented YU_EINVAL returned
before any device work with the output arrays untouched, the empty batch, YU_ENODEV
without a device, the variant name, yu::plan_parse's grid and its knobs behind the gate,
and what the Python front end refuses. CPU only: no call here reaches a device (the
arguments are refused first, or there is no device)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import parse_plan
from yustack_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "yucsum.h")
NAMES = ("yu_rx_parse_ragged", "yu_rx_parse_variant_n")


def test_symbols_exported_and_declared():
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert re.search(rf" T {name}$", nm, flags=re.M), name
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None
    assert len(L.yu_rx_parse_ragged.argtypes) == 8
    assert ctypes.sizeof(_lib.YuIovec) == 16  # one view per packet: base, len


@pytest.fixture
def tables():
    data = (ctypes.c_uint8 * 256)()
    out = (ctypes.c_uint16 * 16)(*([0xA5A5] * 16))
    recs = (_lib.YuTxRecord * 5)()
    views = (_lib.YuIovec * 5)()
    ctypes.memset(recs, 0xA5, ctypes.sizeof(recs))
    ctypes.memset(views, 0xA5, ctypes.sizeof(views))
    offs = (ctypes.c_uint64 * 6)(0, 64, 128, 192, 256, 0)
    t = dict(data=ctypes.addressof(data), offs=ctypes.addressof(offs), recs=ctypes.addressof(recs),
             views=ctypes.addressof(views), out=ctypes.addressof(out))

    def untouched():
        return bytes(out) == b"\xA5" * 32 and bytes(recs) == b"\xA5" * 160 and bytes(views) == b"\xA5" * 80
    t["untouched"] = untouched
    yield t
    del data, out, recs, views, offs


def call(t, n=4, verify=1, **change):
    a = dict(t, **change)
    return _lib.lib().yu_rx_parse_ragged(a["data"], a["offs"], n, verify, a["recs"], a["views"], a["out"], None)


@pytest.mark.parametrize("verify", (1, 0))
def test_every_einval_precedes_device_work(tables, verify):
    """Each refused argument returns YU_EINVAL, whether or not a device is present
    (nothing is launched: the pointers here are host memory), and stores nothing."""
    t, E = tables, _lib.YU_EINVAL
    for name in ("data", "recs", "views"):           # [data]
        assert call(t, 4, verify, **{name: None}) == E, name
    assert call(t, 4, verify, out=None) == E         # [out]
    assert call(t, 4, verify, offs=None) == E        # [offsets]
    assert call(t, 4, verify, offs=t["offs"] + 4) == E
    assert call(t, 4, verify, recs=t["recs"] + 4) == E    # [offsets] recs alignment
    assert call(t, 4, verify, views=t["views"] + 4) == E  # [offsets] pay_views alignment
    for n in (4, 0):                                 # [side-align], checked without n
        assert call(t, n, verify, out=t["out"] + 1) == E
    assert t["untouched"]()


def test_empty_batch_is_a_no_op(tables):
    t = tables
    for verify in (1, 0):
        assert call(t, 0, verify) == _lib.YU_OK
        assert call(t, 0, verify, offs=t["offs"] + 4, recs=t["recs"] + 4, views=None) == _lib.YU_OK  # checked with n only
        assert _lib.lib().yu_rx_parse_ragged(None, None, 0, verify, None, None, None, None) == _lib.YU_OK
    assert t["untouched"]()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_valid_calls_fail_without_gpu(tables):
    t = tables
    for verify in (1, 0, 7):
        assert call(t, 4, verify) == _lib.YU_ENODEV
        assert call(t, 4, verify, data=t["data"] + 1) == _lib.YU_ENODEV  # any byte alignment
        assert call(t, 4, verify, recs=t["recs"] + 8, views=t["views"] + 8) == _lib.YU_ENODEV  # 8-byte aligned tables
    assert t["untouched"]()


def test_variant_name():
    L = _lib.lib()
    for n in (0, 1, 64, 4097, 1 << 20):
        assert L.yu_rx_parse_variant_n(n) == b"k_parse"
        assert batch.parse_variant(n) == "k_parse"
    assert batch.parse_variant() == "k_parse"


def test_plan_rows():
    """A lane per packet: 256 packets per block, 8 blocks per CU, plain loads."""
    ns = (1, 256, 257, 4097, 1 << 20, 1 << 24)
    rows = parse_plan.plans([(n, cus) for n in ns for cus in (64, 256, 304)])
    assert all(r[0] == 0 and r[2] == "k_parse" for r in rows)
    assert [r[1] for r in rows[0:12:3]] == [1, 1, 2, 17]                  # ceil(n / 256)
    assert [r[1] for r in rows[12:15]] == [64 * 8, 256 * 8, 304 * 8]      # 1M packets: the cap
    assert [r[1] for r in rows[15:18]] == [64 * 8, 256 * 8, 304 * 8]


def test_plan_honours_the_knobs_behind_the_gate():
    case = [(1 << 20, 256)]
    plain = parse_plan.plans(case)[0]
    assert plain == (0, 256 * 8, "k_parse")
    assert parse_plan.plans(case, {"YU_NT": "1", "YU_BLOCKS_PER_CU": "1"})[0] == plain  # gate closed
    tuned = parse_plan.plans(case, {"YU_TUNING": "1", "YU_NT": "1", "YU_BLOCKS_PER_CU": "1"})[0]
    assert tuned == (1, 256, "k_parse")
    # one load policy besides plain: YU_NT=2 (the wave kernels' hybrid) stays plain
    assert parse_plan.plans(case, {"YU_TUNING": "1", "YU_NT": "2"})[0] == plain
    assert parse_plan.plans(case, {"YU_TUNING": "1", "YU_BLOCKS_PER_CU": "3"})[0] == (0, 768, "k_parse")


def test_python_front_end_refuses_before_the_library():
    data = torch.zeros(64, dtype=torch.uint8)
    offs = torch.tensor([0, 64], dtype=torch.int64)
    with pytest.raises(TypeError):
        batch.parse_datagrams(data, offs)  # CPU tensors
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda:0")
    data, offs = data.to(dev), offs.to(dev)
    with pytest.raises(TypeError):
        batch.parse_datagrams(data.to(torch.int8), offs)                    # dtype
    with pytest.raises(TypeError):
        batch.parse_datagrams(data, offs.to(torch.float32))                 # dtype
    with pytest.raises(TypeError):
        batch.parse_datagrams(data, offs.cpu())                             # device
    with pytest.raises(ValueError):
        batch.parse_datagrams(data, torch.zeros(0, dtype=torch.int64, device=dev))                   # n + 1
    with pytest.raises(ValueError):
        batch.parse_datagrams(data, offs, records=torch.zeros((1, 16), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        batch.parse_datagrams(data, offs, records=torch.zeros(32, dtype=torch.uint8, device=dev))    # shape
    with pytest.raises(TypeError):
        batch.parse_datagrams(data, offs, records=torch.zeros((1, 32), dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        batch.parse_datagrams(data, offs, views=torch.zeros((1, 2), dtype=torch.int32, device=dev))  # dtype
    with pytest.raises(ValueError):
        batch.parse_datagrams(data, offs, views=torch.zeros(2, dtype=torch.int64, device=dev))       # shape
    with pytest.raises(TypeError):
        batch.parse_datagrams(data, offs, views=torch.zeros((1, 2), dtype=torch.int64))              # CPU views
    with pytest.raises(ValueError):
        batch.parse_datagrams(data, offs, records=data[:32].view(1, 32))                             # overlaps data
    with pytest.raises(TypeError):
        batch.parse_datagrams(data, offs, out=torch.zeros(1, dtype=torch.int32, device=dev))         # dtype
    with pytest.raises(ValueError):
        batch.parse_datagrams(data, torch.tensor([0, 65], device=dev), validate=True)                # past data
    with pytest.raises(ValueError):
        batch.parse_datagrams(data, torch.tensor([9, 8], device=dev), validate=True)                 # decreasing
