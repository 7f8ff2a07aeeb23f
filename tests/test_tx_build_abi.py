"""The device-side sender at the C-ABI boundary (include/yucsum.h, yu_tx_build_ragged /
yu_tx_build_variant_n / struct yu_tx_record): exported and declared, the record's
layout, every documented YU_EINVAL returned before any device work, the empty batch,
YU_ENODEV without a device, the kernel yu::plan_wave names and its knobs behind the
gate, what the Python front end refuses and what packets.tx_records fills in. CPU only:
no call here reaches a device (the arguments are refused first, or there is no device)."""
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
CSRC = os.path.join(ROOT, "yustack_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "yucsum.h")
NAMES = ("yu_tx_build_ragged", "yu_tx_build_variant_n")
# field, offset, size: struct yu_tx_record as include/yucsum.h lays it out
LAYOUT = (("src", 0, 4), ("dst", 4, 4), ("sport", 8, 2), ("dport", 10, 2), ("seq", 12, 4), ("ack", 16, 4),
          ("window", 20, 2), ("flags", 22, 1), ("doff", 23, 1), ("proto", 24, 1), ("ttl", 25, 1), ("ip_id", 26, 2),
          ("tos", 28, 1), ("reserved", 29, 1), ("frag", 30, 2))


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
    assert "typedef struct yu_tx_record" in src


def test_record_layout():
    assert ctypes.sizeof(_lib.YuTxRecord) == 32
    assert packets.TX_RECORD.itemsize == 32
    assert [f[0] for f in _lib.YuTxRecord._fields_] == [f[0] for f in LAYOUT] == list(packets.TX_RECORD.names)
    for name, off, size in LAYOUT:
        fld = getattr(_lib.YuTxRecord, name)
        assert (fld.offset, fld.size) == (off, size), name
        dt, npoff = packets.TX_RECORD.fields[name][:2]
        assert (npoff, dt.itemsize) == (off, size), name
    # the library asserts the same offsets at compile time
    hip = open(os.path.join(CSRC, "yucsum_kernels.hip")).read()
    assert "static_assert(sizeof(yu_tx_record) == 32" in hip
    for name, off, _ in LAYOUT:
        assert f"static_assert(offsetof(yu_tx_record, {name}) == {off}," in hip, name


@pytest.fixture
def tables():
    pay = (ctypes.c_uint8 * 256)()
    dst = (ctypes.c_uint8 * 512)()
    out = (ctypes.c_uint16 * 16)()
    recs = (_lib.YuTxRecord * 4)()
    for r in recs:
        r.proto, r.doff, r.ttl = 17, 20, 64
    po = (ctypes.c_uint64 * 6)(0, 64, 128, 192, 256, 0)
    do = (ctypes.c_uint64 * 6)(0, 92, 184, 276, 368, 0)
    yield (ctypes.addressof(pay), ctypes.addressof(po), ctypes.addressof(recs), ctypes.addressof(dst),
           ctypes.addressof(do), ctypes.addressof(out))
    del pay, dst, out, recs, po, do


def test_every_einval_precedes_device_work(tables):
    """Each refused argument returns YU_EINVAL, whether or not a device is present
    (nothing is launched: the pointers here are host memory)."""
    f = _lib.lib().yu_tx_build_ragged
    p, po, r, d, do, o = tables
    E = _lib.YU_EINVAL
    assert f(None, po, r, 4, d, do, o, None) == E      # [data] payload
    assert f(p, po, None, 4, d, do, o, None) == E      # [data] recs
    assert f(p, po, r, 4, None, do, o, None) == E      # [data] dst
    assert f(p, None, r, 4, d, do, o, None) == E       # [offsets] pay_offsets
    assert f(p, po + 4, r, 4, d, do, o, None) == E     # [offsets] pay_offsets alignment
    assert f(p, po, r, 4, d, None, o, None) == E       # [offsets] dst_offsets
    assert f(p, po, r, 4, d, do + 4, o, None) == E     # [offsets] dst_offsets alignment
    assert f(p, po, r + 4, 4, d, do, o, None) == E     # [offsets] recs alignment
    for n in (4, 0):
        assert f(p, po, r, n, d, do, o + 1, None) == E  # [side-align] out, checked without n
    assert bytes(ctypes.string_at(d, 512)) == bytes(512)


def test_empty_batch_is_a_no_op(tables):
    f = _lib.lib().yu_tx_build_ragged
    p, po, r, d, do, o = tables
    assert f(p, po, r, 0, d, do, o, None) == _lib.YU_OK
    assert f(None, None, None, 0, None, None, None, None) == _lib.YU_OK
    assert bytes(ctypes.string_at(d, 512)) == bytes(512)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_valid_calls_fail_without_gpu(tables):
    f = _lib.lib().yu_tx_build_ragged
    p, po, r, d, do, o = tables
    assert f(p, po, r, 4, d, do, o, None) == _lib.YU_ENODEV
    assert f(p + 1, po, r, 4, d + 3, do, None, None) == _lib.YU_ENODEV  # any byte alignment, NULL out


def test_variant_name():
    L = _lib.lib()
    for n in (0, 1, 64, 4097, 1 << 20):
        assert L.yu_tx_build_variant_n(n) == b"k_build<4>"
        assert batch.build_variant(n) == "k_build<4>"
    assert batch.build_variant() != ""


@pytest.fixture(scope="module")
def build_plan():
    return lambda cases, env=None: wave_plan.plans("build", [(n, 0, 0, cus) for n, cus in cases], env)


def test_plan_rows(build_plan):
    rows = build_plan([(n, cus) for n in (1, 4, 5, 4097, 1 << 20) for cus in (64, 256, 304)])
    assert all(r[0] == 8 and r[1] == 2 and r[3] == "k_build<4>" for r in rows)
    assert [r[2] for r in rows[-3:]] == [64 * 64, 256 * 64, 304 * 64]   # 64 blocks per CU
    assert [r[2] for r in rows[0:12:3]] == [1, 1, 2, 1025]              # a wave per packet, four per block


def test_plan_honours_the_knobs_behind_the_gate(build_plan):
    case = [(1 << 20, 256)]
    plain = build_plan(case)[0]
    assert build_plan(case, {"YU_NT": "0", "YU_BLOCKS_PER_CU": "1"})[0] == plain  # gate closed
    assert build_plan(case, {"YU_TUNING": "1", "YU_NT": "0", "YU_BLOCKS_PER_CU": "1"})[0] == (8, 0, 256, "k_build<4>")


def test_python_front_end_refuses_before_the_library():
    pay = torch.zeros(64, dtype=torch.uint8)
    po = torch.tensor([0, 64], dtype=torch.int64)
    recs = torch.zeros((1, 32), dtype=torch.uint8)
    with pytest.raises(TypeError):
        batch.build_datagrams(pay, po, recs)  # CPU tensors
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda:0")
    pay, po, recs = pay.to(dev), po.to(dev), recs.to(dev)
    with pytest.raises(TypeError):
        batch.build_datagrams(pay.to(torch.int8), po, recs)            # dtype
    with pytest.raises(TypeError):
        batch.build_datagrams(pay, po.to(torch.float32), recs)         # dtype
    with pytest.raises(TypeError):
        batch.build_datagrams(pay, po, recs.to(torch.int32))           # dtype
    with pytest.raises(ValueError):
        batch.build_datagrams(pay, po, recs.reshape(32))               # shape
    with pytest.raises(ValueError):
        batch.build_datagrams(pay, po, torch.zeros((1, 16), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        batch.build_datagrams(pay, torch.zeros(3, dtype=torch.int64, device=dev), recs)  # n + 1 offsets
    with pytest.raises(ValueError):
        batch.build_datagrams(pay, po, recs, dst=pay)                  # dst overlaps payload
    with pytest.raises(TypeError):
        batch.build_datagrams(pay, po, recs, dst=torch.zeros(128, dtype=torch.uint8))  # CPU dst


def test_tx_records_defaults_and_broadcast():
    r = packets.tx_records(3)
    assert r.dtype == packets.TX_RECORD and r.shape == (3,)
    assert (r["ttl"] == 64).all() and (r["ip_id"] == 0).all() and (r["tos"] == 0).all()
    assert (r["frag"] == 0).all() and (r["doff"] == 20).all() and (r["reserved"] == 0).all()
    r = packets.tx_records(3, src=[10, 0, 0, 1], dst=0x0A000002, sport=np.array([1, 2, 3]), dport=80, proto=6,
                           seq=[7, 8, 0xFFFFFFFF], flags=0x18, window=0xFFFF, doff=24)
    assert r["src"].tolist() == [[10, 0, 0, 1]] * 3 and r["dst"].tolist() == [[10, 0, 0, 2]] * 3
    assert r["sport"].tolist() == [1, 2, 3] and r["dport"].tolist() == [80] * 3
    assert r["seq"].tolist() == [7, 8, 0xFFFFFFFF] and (r["proto"] == 6).all() and (r["doff"] == 24).all()
    raw = r.view(np.uint8).reshape(3, 32)
    assert raw[2, 12:16].tolist() == [0xFF] * 4 and raw[1, 8] == 2 and raw[0, 24] == 6 and raw[0, 25] == 64
    c = _lib.YuTxRecord.from_buffer_copy(raw[1].tobytes())
    assert (c.sport, c.dport, c.seq, c.flags, c.window, c.doff, c.proto, c.ttl) == (2, 80, 8, 0x18, 0xFFFF, 24, 6, 64)
    assert bytes(c.src) == bytes([10, 0, 0, 1]) and bytes(c.dst) == bytes([10, 0, 0, 2])
