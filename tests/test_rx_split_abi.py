"""The device-side receiver at the C-ABI boundary (include/yucsum.h, yu_rx_split_ragged /
yu_rx_split_variant_n / YU_RX_SPLIT): exported and declared, every documented YU_EINVAL
returned before any device work with the output arrays untouched, the empty batch,
YU_ENODEV without a device, the kernel yu::plan_wave names, its grid and its knobs
behind the gate, what the Python front end refuses and what packets.rx_records views.
CPU only: no call here reaches a device (the arguments are refused first, or there is no
device)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import wave_plan
from yustack_amd import _lib, batch, packets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "yucsum.h")
NAMES = ("yu_rx_split_ragged", "yu_rx_split_variant_n")


def test_symbols_exported_and_declared():
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert re.search(rf" T {name}$", nm, flags=re.M), name
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None
    assert re.search(r"#define\s+YU_RX_SPLIT\s+16u", src)
    assert batch.RX_SPLIT == packets.RX_SPLIT == 16
    assert batch.RX_SPLIT & (batch.RX_IP_OK | batch.RX_L4 | batch.RX_L4_OK | batch.RX_INVALID) == 0


@pytest.fixture
def tables():
    data = (ctypes.c_uint8 * 256)()
    pay = (ctypes.c_uint8 * 256)(*([0xA5] * 256))
    out = (ctypes.c_uint16 * 16)(*([0xA5A5] * 16))
    plen = (ctypes.c_uint32 * 16)(*([0xA5A5A5A5] * 16))
    recs = (_lib.YuTxRecord * 4)()
    ctypes.memset(recs, 0xA5, ctypes.sizeof(recs))
    offs = (ctypes.c_uint64 * 6)(0, 64, 128, 192, 256, 0)
    po = (ctypes.c_uint64 * 6)(0, 64, 128, 192, 256, 0)
    t = dict(data=ctypes.addressof(data), offs=ctypes.addressof(offs), pay=ctypes.addressof(pay),
             po=ctypes.addressof(po), recs=ctypes.addressof(recs), plen=ctypes.addressof(plen),
             out=ctypes.addressof(out))

    def untouched():
        return (bytes(pay) == b"\xA5" * 256 and bytes(out) == b"\xA5" * 32 and bytes(plen) == b"\xA5" * 64
                and bytes(recs) == b"\xA5" * 128)
    t["untouched"] = untouched
    yield t
    del data, pay, out, plen, recs, offs, po


def call(t, n=4, **change):
    a = dict(t, **change)
    return _lib.lib().yu_rx_split_ragged(a["data"], a["offs"], n, a["pay"], a["po"], a["recs"], a["plen"], a["out"],
                                         None)


def test_every_einval_precedes_device_work(tables):
    """Each refused argument returns YU_EINVAL, whether or not a device is present
    (nothing is launched: the pointers here are host memory), and stores nothing."""
    t, E = tables, _lib.YU_EINVAL
    for name in ("data", "pay", "recs", "plen"):     # [data]
        assert call(t, **{name: None}) == E, name
    assert call(t, out=None) == E                    # [out]
    for name in ("offs", "po"):                      # [offsets]
        assert call(t, **{name: None}) == E, name
        assert call(t, **{name: t[name] + 4}) == E, name
    assert call(t, recs=t["recs"] + 4) == E          # [offsets] recs alignment
    for n in (4, 0):                                 # [side-align], checked without n
        assert call(t, n, out=t["out"] + 1) == E
        assert call(t, n, plen=t["plen"] + 2) == E
    assert t["untouched"]()


def test_empty_batch_is_a_no_op(tables):
    t = tables
    assert call(t, 0) == _lib.YU_OK
    assert _lib.lib().yu_rx_split_ragged(None, None, 0, None, None, None, None, None, None) == _lib.YU_OK
    assert t["untouched"]()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_valid_calls_fail_without_gpu(tables):
    t = tables
    assert call(t) == _lib.YU_ENODEV
    assert call(t, data=t["data"] + 1, pay=t["pay"] + 3) == _lib.YU_ENODEV  # any byte alignment
    assert call(t, po=t["offs"]) == _lib.YU_ENODEV                           # pay_offsets may be offsets itself
    assert t["untouched"]()


def test_variant_name():
    L = _lib.lib()
    for n in (0, 1, 64, 4097, 1 << 20):
        assert L.yu_rx_split_variant_n(n) == b"k_split<4>"
        assert batch.split_variant(n) == "k_split<4>"
    assert batch.split_variant() == "k_split<4>"


def split_plans(cases, env=None):
    """[(kernel, policy, blocks, name)] for the (n, cus) cases."""
    return wave_plan.plans("split", [(n, 0, 0, cus) for n, cus in cases], env)


def test_plan_rows():
    rows = split_plans([(n, cus) for n in (1, 4, 5, 4097, 1 << 20) for cus in (64, 256, 304)])
    assert all(r[0] == 9 and r[1] == 2 and r[3] == "k_split<4>" for r in rows)
    assert [r[2] for r in rows[-3:]] == [64 * 64, 256 * 64, 304 * 64]   # 64 blocks per CU
    assert [r[2] for r in rows[0:12:3]] == [1, 1, 2, 1025]              # a wave per packet, four per block


def test_plan_honours_the_knobs_behind_the_gate():
    case = [(1 << 20, 256)]
    plain = split_plans(case)[0]
    assert plain[1:] == (2, 256 * 64, "k_split<4>")
    assert split_plans(case, {"YU_NT": "0", "YU_BLOCKS_PER_CU": "1"})[0] == plain  # gate closed
    tuned = split_plans(case, {"YU_TUNING": "1", "YU_NT": "0", "YU_BLOCKS_PER_CU": "1"})[0]
    assert tuned[1:] == (0, 256, "k_split<4>")


def test_python_front_end_refuses_before_the_library():
    data = torch.zeros(64, dtype=torch.uint8)
    offs = torch.tensor([0, 64], dtype=torch.int64)
    with pytest.raises(TypeError):
        batch.split_datagrams(data, offs)  # CPU tensors
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda:0")
    data, offs = data.to(dev), offs.to(dev)
    with pytest.raises(TypeError):
        batch.split_datagrams(data.to(torch.int8), offs)                    # dtype
    with pytest.raises(TypeError):
        batch.split_datagrams(data, offs.to(torch.float32))                 # dtype
    with pytest.raises(TypeError):
        batch.split_datagrams(data, offs.cpu())                             # device
    with pytest.raises(ValueError):
        batch.split_datagrams(data, offs, pay_offsets=torch.zeros(3, dtype=torch.int64, device=dev))  # n + 1
    with pytest.raises(ValueError):
        batch.split_datagrams(data, offs, records=torch.zeros((1, 16), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        batch.split_datagrams(data, offs, records=torch.zeros(32, dtype=torch.uint8, device=dev))    # shape
    with pytest.raises(TypeError):
        batch.split_datagrams(data, offs, records=torch.zeros((1, 32), dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        batch.split_datagrams(data, offs, pay_len=torch.zeros(1, dtype=torch.int64, device=dev))     # dtype
    with pytest.raises(TypeError):
        batch.split_datagrams(data, offs, pay=torch.zeros(64, dtype=torch.uint8))                    # CPU pay
    with pytest.raises(ValueError):
        batch.split_datagrams(data, offs, pay=data[8:])                                              # pay overlaps data
    with pytest.raises(ValueError):
        batch.split_datagrams(data, torch.tensor([0, 65], device=dev), validate=True)                # past data
    data[0], data[3], data[9] = 0x45, 64, 17  # a 64-byte UDP datagram: a 36-byte payload
    with pytest.raises(ValueError):
        batch.split_datagrams(data, offs, pay_offsets=torch.tensor([0, 35], device=dev), validate=True)  # room < L
    with pytest.raises(ValueError):
        batch.split_datagrams(data, offs, pay_offsets=torch.tensor([40, 39], device=dev), validate=True)  # decreasing


def test_rx_records_views_the_record_layout():
    raw = np.zeros((2, 32), dtype=np.uint8)
    rec = packets.tx_records(1, src=[10, 0, 0, 1], dst=0x0A000002, sport=7, dport=80, proto=6, seq=0xFFFFFFFE,
                             flags=0x18, window=0xFFFF, doff=24, ttl=3, ip_id=0x1234, tos=9, frag=0x4000)
    raw[1] = rec.view(np.uint8)
    r = packets.rx_records(torch.from_numpy(raw))
    assert r.dtype == packets.TX_RECORD and r.shape == (2,)
    assert r[1] == rec[0] and not raw[0].any() and r[0]["proto"] == 0
    assert (r["seq"][1], r["doff"][1], r["ip_id"][1], r["frag"][1]) == (0xFFFFFFFE, 24, 0x1234, 0x4000)
    with pytest.raises(ValueError):
        packets.rx_records(np.zeros((2, 16), dtype=np.uint8))
