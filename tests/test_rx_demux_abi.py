"""The demultiplexer at the C-ABI boundary (include/yucsum.h: yu_demux_table_bytes,
yu_demux_hash, yu_demux_table_fill, yu_rx_demux, yu_rx_demux_variant_n): exported and
declared, the table's size, a round trip through the fill in which a Python walk of the
filled bytes finds every id, each refusal of the fill with its `bad` and the buffer
untouched, every documented YU_EINVAL of yu_rx_demux returned before any device work,
the empty batch, YU_ENODEV without a device, the variant name, yu::plan_demux's grid and
its knobs behind the gate, and what the Python front end refuses. CPU only: no call here
reaches a device (the arguments are refused first, or there is no device)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import demux_plan
import parse_plan
from yustack_amd import _lib, batch, packets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "yucsum.h")
NAMES = ("yu_demux_table_bytes", "yu_demux_hash", "yu_demux_table_fill", "yu_rx_demux", "yu_rx_demux_variant_n")
E = _lib.YU_EINVAL


def test_symbols_exported_and_declared():
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert re.search(rf" T {name}$", nm, flags=re.M), name
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None
    assert len(L.yu_rx_demux.argtypes) == 10 and len(L.yu_demux_table_fill.argtypes) == 5
    assert ctypes.sizeof(_lib.YuEndpointId) == 16 == packets.ENDPOINT_ID.itemsize
    for name, _ in _lib.YuEndpointId._fields_:
        assert getattr(_lib.YuEndpointId, name).offset == packets.ENDPOINT_ID.fields[name][1], name
    assert re.search(r"#define YU_DEMUX_NONE 0xFFFFFFFFu", src) and batch.DEMUX_NONE == 0xFFFFFFFF
    assert re.search(r"#define YU_DEMUX_MAX_ENDPOINTS \(1u << 24\)", src) and batch.DEMUX_MAX_ENDPOINTS == 1 << 24


def test_table_bytes():
    """16 bytes per slot; the slots are the power of two that is at least 16 and at least 2m."""
    L = _lib.lib()
    got = [L.yu_demux_table_bytes(m) for m in (0, 1, 8, 9, 1 << 24, (1 << 24) + 1)]
    assert got == [256, 256, 256, 512, 16 << 25, 0]
    assert L.yu_demux_table_bytes(1 << 63) == 0 and L.yu_demux_table_bytes((1 << 64) - 1) == 0


def mixed_ids(m, seed=5):
    """m distinct well-formed ids of all three kinds and both protocols."""
    rng = np.random.default_rng(seed)
    ids, seen = packets.endpoint_ids(m), set()
    k = 0
    while k < m:
        kind, proto = int(rng.integers(0, 3)), (6, 17)[int(rng.integers(0, 2))]
        la = rng.integers(0, 256, 4, dtype=np.uint8) if kind != 2 else np.zeros(4, np.uint8)
        ra = rng.integers(0, 4, 4, dtype=np.uint8) if kind == 0 else np.zeros(4, np.uint8)  # 0.0.0.0 is among them
        lp, rp = int(rng.integers(0, 65536)), int(rng.integers(0, 3)) if kind == 0 else 0
        key = (kind, proto, bytes(la), bytes(ra), lp, rp)
        if key in seen:
            continue
        seen.add(key)
        ids[k] = (la, ra, lp, rp, proto, kind, 0)
        k += 1
    return ids


def fill(ids, m=None, table_bytes=None, buf=None, null_ids=False, null_table=False):
    """(status, bad, the buffer's bytes) of one yu_demux_table_fill call on a buffer of 0xA5."""
    L = _lib.lib()
    m = len(ids) if m is None else m
    nbytes = L.yu_demux_table_bytes(len(ids)) if table_bytes is None else table_bytes
    buf = np.full(max(nbytes, 16) if buf is None else buf, 0xA5, dtype=np.uint8)
    ids = np.ascontiguousarray(ids)
    bad = ctypes.c_uint64(0xDEAD)
    rc = L.yu_demux_table_fill(None if null_ids else ids.ctypes.data, m, None if null_table else buf.ctypes.data,
                               nbytes, ctypes.byref(bad))
    return rc, bad.value, buf


def walk(table, ident, number):
    """Finds `ident` in the filled bytes: from its home slot on, over taken slots only."""
    L = _lib.lib()
    slots = table.size // 16
    words = table.view(np.uint32).reshape(slots, 4)
    want = [int(ident["local_addr"].view(np.uint32)[0]), int(ident["remote_addr"].view(np.uint32)[0]),
            int(ident["local_port"]) | int(ident["remote_port"]) << 16,
            number << 8 | int(ident["kind"]) << 4 | (2 if ident["proto"] == 17 else 1)]
    one = np.array([ident], dtype=packets.ENDPOINT_ID)
    i = L.yu_demux_hash(one.ctypes.data) & (slots - 1)
    for _ in range(slots):
        if words[i].tolist() == want:
            return True
        if words[i, 3] == 0:
            return False
        i = (i + 1) & (slots - 1)
    return False


@pytest.mark.parametrize("m", (0, 1, 8, 9, 1000))
def test_fill_round_trip(m):
    ids = mixed_ids(m)
    rc, bad, table = fill(ids)
    assert rc == _lib.YU_OK and bad == m
    assert table.size == _lib.lib().yu_demux_table_bytes(m)
    words = table.view(np.uint32).reshape(-1, 4)
    assert int((words[:, 3] != 0).sum()) == m                      # every other slot is empty ...
    assert not words[words[:, 3] == 0].any()                        # ... and all zero
    assert all(walk(table, ids[j], j) for j in range(m))
    assert not walk(table, mixed_ids(1, seed=77)[0], 0)


def test_hash_is_the_home_slot():
    """A table of one id holds it in slot yu_demux_hash & 15; and the hash tells kinds,
    protocols and each key word apart."""
    L = _lib.lib()
    ids = mixed_ids(64, seed=9)
    hashes = set()
    for j in range(64):
        one = np.ascontiguousarray(ids[j:j + 1])
        rc, bad, table = fill(one)
        assert rc == _lib.YU_OK
        taken = np.flatnonzero(table.view(np.uint32).reshape(16, 4)[:, 3])
        h = L.yu_demux_hash(one.ctypes.data)
        assert taken.tolist() == [h & 15]
        hashes.add(h)
    assert len(hashes) == 64
    base = packets.endpoint_ids(1, local_addr=0x0A000001, local_port=80, remote_addr=0x0A000002, remote_port=9)
    variants = [base.copy() for _ in range(5)]
    variants[1]["proto"], variants[2]["local_port"], variants[3]["remote_port"] = 17, 81, 10
    variants[4]["remote_addr"] = (10, 0, 0, 3)
    assert len({L.yu_demux_hash(v.ctypes.data) for v in variants}) == 5


def test_fill_refuses_each_malformed_id_and_names_it():
    good = mixed_ids(8)

    def with_id(at, **fields):
        ids = good.copy()
        ids[at] = packets.endpoint_ids(1, **{"local_addr": 0x0A000001, "local_port": 80, **fields})[0]
        return ids

    cases = [
        (3, with_id(3, proto=1)),
        (0, with_id(0, proto=0)),
        (7, with_id(7, kind=3)),
        (2, with_id(2, kind=1, remote_addr=0x0A000002)),           # a listener with a remote address
        (4, with_id(4, kind=1, remote_port=5)),                    # ... with a remote port
        (5, with_id(5, kind=2)),                                   # a port listener with a local address
        (1, with_id(1, kind=2, local_addr=0, remote_port=1)),
    ]
    reserved = good.copy()
    reserved["reserved"][6] = 1
    cases.append((6, reserved))
    for at, ids in cases:
        rc, bad, buf = fill(ids)
        assert (rc, bad) == (E, at), (at, rc, bad)
        assert (buf == 0xA5).all()
    # the same ids with their fields emptied go in
    rc, bad, _ = fill(with_id(5, kind=2, local_addr=0))
    assert (rc, bad) == (_lib.YU_OK, 8)


def test_fill_refuses_a_duplicate_at_its_index():
    good = mixed_ids(8)
    dup = good.copy()
    dup[5] = dup[2]
    rc, bad, buf = fill(dup)
    assert (rc, bad) == (E, 5) and (buf == 0xA5).all()
    both = dup.copy()
    both["proto"][4] = 99                   # the first offending id is named, whatever its fault
    assert fill(both)[:2] == (E, 4)
    both[4], both[1] = good[4], good[0]
    assert fill(both)[:2] == (E, 1)
    # Go's empty Address is not 0.0.0.0: a connection from 0.0.0.0:0 and a listener on the same
    # local pair are two ids, and so is one 4-tuple under the two protocols
    ids = packets.endpoint_ids(4, local_addr=0x0A000001, local_port=80, kind=[0, 1, 0, 1], proto=[6, 6, 17, 17])
    rc, bad, table = fill(ids)
    assert (rc, bad) == (_lib.YU_OK, 4) and all(walk(table, ids[j], j) for j in range(4))


def test_fill_refuses_sizes_and_nulls():
    ids = mixed_ids(9)
    right = _lib.lib().yu_demux_table_bytes(9)
    for wrong in (0, right - 16, right + 16, 256):
        rc, bad, buf = fill(ids, table_bytes=wrong, buf=right + 16)
        assert (rc, bad) == (E, 9) and (buf == 0xA5).all()
    rc, bad, buf = fill(ids, null_ids=True)
    assert (rc, bad) == (E, 9) and (buf == 0xA5).all()
    assert fill(ids, null_table=True)[:2] == (E, 9)
    over = (1 << 24) + 1                     # over the limit: refused before an id is read
    rc, bad, buf = fill(ids, m=over, table_bytes=0)
    assert (rc, bad) == (E, over) and (buf == 0xA5).all()
    assert fill(ids, m=over, table_bytes=16 << 25, buf=64)[:2] == (E, over)
    # m == 0: the empty table, 16 zero slots; bad may be NULL
    rc, bad, buf = fill(ids[:0])
    assert (rc, bad) == (_lib.YU_OK, 0) and buf.size == 256 and not buf.any()
    buf = np.full(256, 0xA5, dtype=np.uint8)
    assert _lib.lib().yu_demux_table_fill(None, 0, buf.ctypes.data, 256, None) == _lib.YU_OK and not buf.any()
    assert _lib.lib().yu_demux_table_fill(ids.ctypes.data, 9, None, right, None) == E


@pytest.fixture
def tables():
    recs = (_lib.YuTxRecord * 5)()
    flags = (ctypes.c_uint16 * 8)()
    table = (ctypes.c_uint8 * (256 + 32))()
    ep = (ctypes.c_uint32 * 8)(*([0xA5A5A5A5] * 8))
    count = (ctypes.c_uint32 * 8)(*([0xA5A5A5A5] * 8))
    t = dict(recs=ctypes.addressof(recs), flags=ctypes.addressof(flags),
             table=(ctypes.addressof(table) + 15) & ~15, ep=ctypes.addressof(ep), count=ctypes.addressof(count))

    def untouched():
        return bytes(ep) == b"\xA5" * 32 and bytes(count) == b"\xA5" * 32
    t["untouched"] = untouched
    yield t
    del recs, flags, table, ep, count


def call(t, n=4, need=0, table_bytes=256, m=3, **change):
    a = dict(t, **change)
    return _lib.lib().yu_rx_demux(a["recs"], a["flags"], need, n, a["table"], table_bytes, m, a["ep"], a["count"], None)


def test_every_einval_precedes_device_work(tables):
    """Each refused argument returns YU_EINVAL, whether or not a device is present
    (nothing is launched: the pointers here are host memory), and stores nothing."""
    t = tables
    for name in ("recs", "table"):                       # [data]
        assert call(t, **{name: None}) == E, name
    for n in (4, 0):                                     # [data], checked without n
        assert call(t, n, table_bytes=512) == E
        assert call(t, n, table_bytes=0) == E
        assert call(t, n, m=9) == E                      # 9 ids take 512 bytes
        assert call(t, n, m=(1 << 24) + 1, table_bytes=0) == E
        assert call(t, n, m=(1 << 24) + 1, table_bytes=16 << 25) == E
    assert call(t, ep=None) == E                         # [out]
    assert call(t, recs=t["recs"] + 4) == E              # [offsets]
    assert call(t, table=t["table"] + 8) == E
    for n in (4, 0):                                     # [side-align], checked without n
        assert call(t, n, flags=t["flags"] + 1) == E
        assert call(t, n, ep=t["ep"] + 2) == E
        assert call(t, n, count=t["count"] + 2) == E
    assert t["untouched"]()


def test_empty_batch_is_a_no_op(tables):
    t = tables
    assert call(t, 0) == _lib.YU_OK
    assert call(t, 0, recs=t["recs"] + 4, table=t["table"] + 8, ep=None) == _lib.YU_OK  # checked with n only
    assert _lib.lib().yu_rx_demux(None, None, 0, 0, None, 256, 0, None, None, None) == _lib.YU_OK
    assert t["untouched"]()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_valid_calls_fail_without_gpu(tables):
    t = tables
    for need in (0, 5, 0xFFFF):
        assert call(t, 4, need) == _lib.YU_ENODEV
        assert call(t, 4, need, flags=None, count=None) == _lib.YU_ENODEV
        assert call(t, 4, need, recs=t["recs"] + 8, flags=t["flags"] + 2, ep=t["ep"] + 4) == _lib.YU_ENODEV
        assert call(t, 4, need, m=0) == _lib.YU_ENODEV
    assert t["untouched"]()


def test_variant_name():
    L = _lib.lib()
    for n in (0, 1, 64, 4097, 1 << 20):
        assert L.yu_rx_demux_variant_n(n) == b"k_demux"
        assert batch.demux_variant(n) == "k_demux"
    assert batch.demux_variant() == "k_demux"


def test_plan_rows():
    """A lane per packet: 256 packets per block, 8 blocks per CU, plain loads: the rule of
    yu::plan_parse, one function behind both."""
    cases = [(n, cus) for n in (1, 256, 257, 4097, 1 << 20, 1 << 24) for cus in (64, 256, 304)]
    rows = demux_plan.plans(cases)
    assert all(r[0] == 0 and r[2] == "k_demux" for r in rows)
    assert [r[1] for r in rows[0:12:3]] == [1, 1, 2, 17]                  # ceil(n / 256)
    assert [r[1] for r in rows[12:15]] == [64 * 8, 256 * 8, 304 * 8]      # 1M packets: the cap
    assert [r[:2] for r in rows] == [r[:2] for r in parse_plan.plans(cases)]


def test_plan_honours_the_knobs_behind_the_gate():
    case = [(1 << 20, 256)]
    plain = demux_plan.plans(case)[0]
    assert plain == (0, 256 * 8, "k_demux")
    assert demux_plan.plans(case, {"YU_NT": "1", "YU_BLOCKS_PER_CU": "1"})[0] == plain  # gate closed
    env = {"YU_TUNING": "1", "YU_NT": "1", "YU_BLOCKS_PER_CU": "1"}
    assert demux_plan.plans(case, env)[0] == (1, 256, "k_demux")
    assert demux_plan.plans(case, env)[0][:2] == parse_plan.plans(case, env)[0][:2]
    assert demux_plan.plans(case, {"YU_TUNING": "1", "YU_BLOCKS_PER_CU": "3"})[0] == (0, 768, "k_demux")


def test_endpoint_ids_broadcast():
    ids = packets.endpoint_ids(3, local_addr=0x0A000001, local_port=[1, 2, 3], proto=17, kind=1)
    assert ids["local_addr"].tolist() == [[10, 0, 0, 1]] * 3 and ids["local_port"].tolist() == [1, 2, 3]
    assert ids["proto"].tolist() == [17] * 3 and ids["kind"].tolist() == [1] * 3 and not ids["reserved"].any()
    assert ids.view(np.uint8).reshape(3, 16)[1].tolist() == [10, 0, 0, 1, 0, 0, 0, 0, 2, 0, 0, 0, 17, 1, 0, 0]


def test_python_front_end_refuses_before_the_library():
    ids = mixed_ids(8)
    with pytest.raises(TypeError):
        batch.demux_table(ids, "cpu")                                      # no device table on a CPU
    with pytest.raises(TypeError):
        batch.demux_table(np.zeros(8, dtype=np.uint32), "cuda:0")          # not ids
    with pytest.raises(ValueError):
        batch.demux_table(ids.reshape(2, 4), "cuda:0")
    dup = ids.copy()
    dup[6] = dup[1]
    with pytest.raises(ValueError, match="bad = 6"):                       # refused on the host, before any upload
        batch.demux_table(dup, "cuda:0")
    dup["kind"][3] = 7
    with pytest.raises(ValueError, match="bad = 3"):
        batch.demux_table(dup.view(np.uint8).reshape(8, 16), "cuda:0")
    recs, table = torch.zeros((4, 32), dtype=torch.uint8), torch.zeros(256, dtype=torch.uint8)
    with pytest.raises(TypeError):
        batch.demux_datagrams(recs, table, 0)                              # CPU tensors
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda:0")
    recs, table = recs.to(dev), table.to(dev)
    u32 = dict(dtype=torch.uint32, device=dev)
    with pytest.raises(TypeError):
        batch.demux_datagrams(recs, table.cpu(), 0)                        # device
    with pytest.raises(TypeError):
        batch.demux_datagrams(recs.to(torch.int8), table, 0)               # dtype
    with pytest.raises(ValueError):
        batch.demux_datagrams(recs.reshape(8, 16), table, 0)               # shape
    with pytest.raises(ValueError):
        batch.demux_datagrams(recs.reshape(-1), table, 0)
    with pytest.raises(ValueError):
        batch.demux_datagrams(recs, table, 9)                              # 9 ids take 512 bytes
    with pytest.raises(ValueError):
        batch.demux_datagrams(recs, table, (1 << 24) + 1)
    with pytest.raises(ValueError):
        batch.demux_datagrams(recs, table.reshape(16, 16), 0)
    with pytest.raises(TypeError):
        batch.demux_datagrams(recs, torch.zeros(272, dtype=torch.uint8, device=dev)[8:264], 0)   # table alignment
    with pytest.raises(TypeError):
        batch.demux_datagrams(torch.zeros(132, dtype=torch.uint8, device=dev)[4:].view(4, 32), table, 0)
    with pytest.raises(TypeError):
        batch.demux_datagrams(recs, table, 0, flags=torch.zeros(4, dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        batch.demux_datagrams(recs, table, 0, flags=torch.zeros(3, dtype=torch.uint16, device=dev))  # too few
    with pytest.raises(ValueError):
        batch.demux_datagrams(recs, table, 0, need=1 << 16)
    with pytest.raises(TypeError):
        batch.demux_datagrams(recs, table, 0, ep=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        batch.demux_datagrams(recs, table, 0, ep=torch.zeros(5, **u32))
    with pytest.raises(TypeError):
        batch.demux_datagrams(recs, table, 0, ep=torch.zeros(4, dtype=torch.uint32))                 # CPU ep
    with pytest.raises(ValueError):
        batch.demux_datagrams(recs, table, 3, counts=torch.zeros(3, **u32))                          # m + 1
    with pytest.raises(ValueError):
        batch.demux_datagrams(recs, table, 0, ep=table[:16].view(torch.uint32))                     # overlaps the table
    both = torch.zeros(5, **u32)
    with pytest.raises(ValueError):
        batch.demux_datagrams(recs, table, 0, ep=both[:4], counts=both[3:4])                        # overlap each other
