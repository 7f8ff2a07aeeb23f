"""Whole IPv4 datagrams held as scatter-gather device packets (yu_csum_batch_iov_datagram /
yu_csum_fill_iov_datagram through batch.checksum_iov_datagrams) on the GPU: IPV4,
VERIFY_IPV4, VERIFY_RX and TX_DATAGRAM.

Every result is compared bit for bit with the C oracle's ragged batch over the same
bytes laid back to back, and no packet is filtered out: the oracle defines all four
modes at every length, 0 included. In place, every byte of every pool (guard bytes
included) is compared with the pools the field rule of include/yucsum.h gives
(tests/test_gpu_contract.py::_fields restates it on the packed bytes), and `out`'s
guard is untouched. Datagrams come from tests/rxgen.py, which keeps the one input
condition YU_MODE_TCP makes (20 <= DataOffset <= segment length inside a valid
datagram)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rxgen
from iov_layout import Layout, general_layout, two_view_layout
from oracle import oracle as O
from test_gpu_contract import _fields
from test_oracle import refexec_mode_batch
from yustack_amd import _lib, batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (O.MODE_IPV4, O.MODE_VERIFY_IPV4, O.MODE_VERIFY_RX, O.MODE_TX_DATAGRAM)
FILL = (O.MODE_IPV4, O.MODE_TX_DATAGRAM)


@pytest.fixture(scope="module")
def rng():
    return np.random.default_rng(20261020)


def put_packets(lay, packets):
    """Writes the packets' bytes where the layout's views lie; the layout's lengths
    must be theirs."""
    assert [len(p) for p in packets] == list(lay.lens)
    blob = np.frombuffer(b"".join(bytes(p) for p in packets), np.uint8)
    if blob.size:
        lay.put(np.arange(blob.size), blob)
    return lay


def build(packets, views, rng, npools=2):
    """packets[i] cut into views[i] = [(pool, address mod 16, length), ...]."""
    return put_packets(general_layout(views, rng, npools=npools), packets)


def random_cuts(rng, ln, nv, npools=2):
    """ln bytes in nv views (some empty), each in a random pool at a random alignment."""
    c = np.sort(rng.integers(0, ln + 1, nv - 1)) if nv > 1 else np.zeros(0, np.int64)
    edges = np.concatenate(([0], c, [ln]))
    return [(int(rng.integers(0, npools)), int(rng.integers(0, 16)), int(b - a)) for a, b in zip(edges[:-1], edges[1:])]


def expected_pools(lay, mode, blob, want, skip=()):
    pools = [p.copy() for p in lay.pools]
    offs = lay.offsets.astype(np.int64)
    g, v = [], []
    for i in range(lay.n):
        if i in skip:
            continue
        for at, val in _fields(mode, blob, int(offs[i]), int(offs[i + 1]), [int(x) for x in want[i]]):
            g.append(at)
            v.append(val & 0xFF)
    if g:
        lay.put(g, np.asarray(v, np.uint8), pools)
    return pools


def check(lay, mode, dev, oracle_c, fill=False, with_out=True):
    """One call on every packet of `lay`."""
    k = 2 if mode == O.MODE_TX_DATAGRAM else 1
    blob = lay.blob()
    want = oracle_c.batch(blob, mode, offsets=lay.offsets, threads=8).reshape(lay.n, k)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    guard = 64  # around an `out` that is 2-byte but not 4-byte aligned, as the ABI allows
    out = torch.full((1 + lay.n * k + guard,), 0xA5A5, dtype=torch.uint16, device=dev)
    got = batch.checksum_iov_datagrams(views, vp, vo, vl, first, mode, fill=fill,
                                       out=out[1:1 + lay.n * k] if with_out else None)
    assert got.numel() == lay.n * k
    res = got.cpu().numpy().reshape(lay.n, k)
    bad = np.flatnonzero((res != want).any(1))
    assert bad.size == 0, (mode, fill, bad[:8], lay.lens[bad[:8]], res[bad[:8]], want[bad[:8]])
    assert int(out[0]) == 0xA5A5 and (out[1 + lay.n * k:].cpu().numpy() == 0xA5A5).all()
    expect = expected_pools(lay, mode, blob, want) if fill else lay.pools
    for q, (a, e) in enumerate(zip(pools, expect)):
        diff = np.flatnonzero(a.cpu().numpy() != e)
        assert diff.size == 0, (mode, fill, q, diff[:8])
    return want


def check_all(lay, dev, oracle_c, fills=True):
    for mode in MODES:
        check(lay, mode, dev, oracle_c)
    if fills:
        for mode in FILL:
            check(lay, mode, dev, oracle_c, fill=True)
            check(lay, mode, dev, oracle_c, fill=True, with_out=False)


def datagram(rng, ihl, proto, seg):
    """A datagram with a `seg`-byte segment: built as the senders build it where the
    segment holds its fixed header, else a bare header and random segment bytes."""
    if seg >= {6: 20, 17: 8, 1: 4}.get(proto, 0):
        return rxgen.make_packet(rng, seg, proto=proto, ihl=ihl)
    hl = 4 * ihl
    pkt = bytearray(rng.integers(0, 256, hl + seg, dtype=np.uint8).tobytes())
    pkt[0] = 0x40 | ihl
    pkt[2], pkt[3] = (hl + seg) >> 8, (hl + seg) & 0xFF
    pkt[9] = proto
    return pkt


# ---- 1. header splits ---------------------------------------------------------------
@pytest.fixture(scope="module")
def split_layout(rng):
    """IHL 5, 6, 15; segments of 0, 1, 7, 8, 64 and 1480 bytes of each protocol; two
    views split at every position 0..HL+20. The first view's address takes every
    value mod 16 and the second's every value mod 4 over the splits of each datagram,
    rotated from one datagram to the next, so bytes 10|11 and the transport field's
    two bytes fall into different views at odd addresses."""
    pk, cuts, a1, a2 = [], [], [], []
    k = 0
    for ihl in (5, 6, 15):
        for seg in (0, 1, 7, 8, 64, 1480):
            for proto in (6, 17, 1, 47):
                d = datagram(rng, ihl, proto, seg)
                for c in range(min(4 * ihl + 20, len(d)) + 1):
                    pk.append(d)
                    cuts.append(c)
                    a1.append((c + k) % 16)
                    a2.append((c // 16 + c // 2 + k // 16) % 4)
                k += 5
    return put_packets(two_view_layout([len(p) for p in pk], cuts, a1, a2, rng), pk)


@pytest.mark.parametrize("mode", MODES)
def test_header_splits(split_layout, mode, dev, oracle_c):
    check(split_layout, mode, dev, oracle_c)


@pytest.mark.parametrize("mode", FILL)
def test_header_splits_in_place(split_layout, mode, dev, oracle_c):
    check(split_layout, mode, dev, oracle_c, fill=True)
    check(split_layout, mode, dev, oracle_c, fill=True, with_out=False)


def test_fill_without_out_at_the_abi(dev, rng, oracle_c):
    """out == NULL in the fill form: the fields are stored all the same."""
    pk = [rxgen.tx_packet(rng, 40 + i, proto=(6, 17, 1)[i % 3]) for i in range(30)]
    lay = build(pk, [[(0, i % 16, 11), (1, i % 4, len(p) - 11)] for i, p in enumerate(pk)], rng)
    blob = lay.blob()
    want = oracle_c.batch(blob, O.MODE_TX_DATAGRAM, offsets=lay.offsets).reshape(lay.n, 2)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    base = torch.where(vp == 0, vo + views[0].data_ptr(), vo + views[1].data_ptr())
    table = torch.stack((base, vl), 1).contiguous()
    rc = _lib.lib().yu_csum_fill_iov_datagram(table.data_ptr(), first.data_ptr(), lay.n, O.MODE_TX_DATAGRAM, None,
                                              torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for a, e in zip(pools, expected_pools(lay, O.MODE_TX_DATAGRAM, blob, want)):
        assert np.array_equal(a.cpu().numpy(), e)


# ---- 2. one-byte and empty views ------------------------------------------------------
def test_one_byte_and_empty_views(dev, rng, oracle_c):
    pk, vw = [], []
    for proto in (6, 17, 1):
        for ihl in (5, 15):
            d = rxgen.make_packet(rng, 100, proto=proto, ihl=ihl)
            pk.append(d)  # the first 80 views hold one byte each
            vw.append([(i % 2, (3 * i) % 16, 1) for i in range(80)] + [(1, 3, len(d) - 80)])
            pk.append(d)  # an empty view between every two header bytes
            vw.append([v for i in range(4 * ihl + 20) for v in ((i % 2, (5 * i) % 16, 1), (1, 0, 0))] +
                      [(0, 1, len(d) - 4 * ihl - 20)])
            pk.append(d)  # 70 empty views first: the header lies past the records the lanes hold
            vw.append([(0, 0, 0)] * 70 + [(0, 7, 9), (1, 2, 4 * ihl), (0, 0, 0), (1, 1, len(d) - 9 - 4 * ihl)])
    pk.append(bytearray())
    vw.append([(0, 0, 0)] * 3)
    pk.append(bytearray())
    vw.append([])
    check_all(build(pk, vw, rng), dev, oracle_c)


def test_null_base_empty_views(dev, rng, oracle_c):
    """A yu_iovec table written by hand: 70 empty views with base NULL (and one wild
    base) in front of the header, which so lies past the 64 records the lanes hold."""
    d = np.frombuffer(bytes(rxgen.make_packet(rng, 300, proto=6, ihl=6)), np.uint8)
    a = torch.from_numpy(np.concatenate((np.zeros(3, np.uint8), d[:13]))).to(dev)
    b = torch.from_numpy(np.concatenate((np.zeros(1, np.uint8), d[13:]))).to(dev)
    recs = [(0, 0)] * 35 + [(0xDEAD0001, 0)] + [(0, 0)] * 34 + [(a.data_ptr() + 3, 13), (0, 0),
                                                              (b.data_ptr() + 1, len(d) - 13), (0, 0)]
    recs += [(0, 0)]                                           # packet 1: one empty view
    recs += [(a.data_ptr() + 3, 13), (b.data_ptr() + 1, 50)]   # packet 2: TotalLength past the bytes
    first = [0, 74, 75, 77]
    table = torch.tensor(recs, dtype=torch.int64, device=dev)
    fi = torch.tensor(first, dtype=torch.int64, device=dev)
    pk = [d, d[:0], d[:63]]
    offs = np.concatenate(([0], np.cumsum([len(x) for x in pk]))).astype(np.uint64)
    blob = np.concatenate(pk + [np.zeros(1, np.uint8)])
    for mode in MODES:
        k = 2 if mode == O.MODE_TX_DATAGRAM else 1
        out = torch.zeros(3 * k, dtype=torch.uint16, device=dev)
        rc = _lib.lib().yu_csum_batch_iov_datagram(table.data_ptr(), fi.data_ptr(), 3, mode, out.data_ptr(),
                                                   torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
        assert np.array_equal(out.cpu().numpy(), oracle_c.batch(blob, mode, offsets=offs).reshape(-1)), mode


# ---- 3. window seams --------------------------------------------------------------------
def test_window_seams(dev, rng, oracle_c):
    pk, vw = [], []
    for proto in (6, 17, 1):
        for ihl in (5, 7):
            hl = 4 * ihl
            d = rxgen.make_packet(rng, 200, proto=proto, ihl=ihl)
            tl = len(d)
            tail = bytes(rng.integers(0, 256, 37, dtype=np.uint8))
            for al in (0, 1, 2, 3):
                # TL == len: the header end on a view boundary and mid-view
                pk.append(d); vw.append([(0, al, hl), (1, al + 1, tl - hl)])
                pk.append(d); vw.append([(0, al, hl - 3), (1, 5 - al, tl - hl + 3)])
                pk.append(d); vw.append([(0, al, hl + 5), (1, 2 + al, tl - hl - 5)])
                # TL < len: the trailing bytes in the same view, in a later view, as whole extra views
                pk.append(d + tail); vw.append([(0, al, hl), (1, 3 - al, tl - hl + 37)])
                pk.append(d + tail); vw.append([(0, al, hl), (1, al, tl - hl), (0, 9 + al, 37)])
                pk.append(d + tail); vw.append([(0, al, tl), (1, al, 30), (0, 0, 0), (1, 3 + al, 7)])
                # TL one byte before, on and one byte past a view boundary
                for e in (-1, 0, 1):
                    pk.append(d + tail); vw.append([(0, al, hl + 11), (1, al + 8, tl - hl - 11 + e), (0, al + 1, 37 - e)])
    # slot seams and step seams (a step is 4 slots of 1 KiB) in 1, 2 and 5 views
    for i, seg in enumerate((1023, 1024, 1025, 4095, 4096, 4097, 9000)):
        proto = (6, 17, 1)[i % 3]
        d = rxgen.make_packet(rng, seg, proto=proto, ihl=5 + i % 3)
        hl = (d[0] & 15) * 4
        pk.append(d); vw.append([(0, 3 + i, len(d))])
        pk.append(d); vw.append([(0, i, hl), (1, i + 1, seg)])
        pk.append(d); vw.append([(0, 2 * i, hl + 1)] + [(1 - j % 2, i + 3 * j, (seg - 1) // 4) for j in range(3)] +
                                [(1, 5, seg - 1 - 3 * ((seg - 1) // 4))])
        pk.append(d + bytes(50)); vw.append(random_cuts(rng, len(d) + 50, 5))
    d = rxgen.make_packet(rng, 65535 - 20, proto=17, ihl=5)
    pk.append(d); vw.append([(0, 1, 20), (1, 3, 65515)])
    d = rxgen.make_packet(rng, 65535 - 60, proto=6, ihl=15)
    pk.append(d); vw.append([(1, 2, 65535)])
    check_all(build(pk, vw, rng), dev, oracle_c)


# ---- 4. malformed -------------------------------------------------------------------------
def cut_batch(rng, blob, offs, npools=2, nvmax=4):
    offs = offs.astype(np.int64)
    pk = [blob[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    return pk, [random_cuts(rng, len(p), int(rng.integers(1, nvmax + 1)), npools) for p in pk]


def test_malformed(dev, rng, oracle_c):
    pk, vw = cut_batch(rng, *rxgen.rx_batch(rng, 600, hi=300, bad=0.5))
    p2, v2 = cut_batch(rng, *rxgen.tx_batch(rng, 600, hi=300, bad=0.3))
    p3 = [bytes(rxgen.short_header_packet(rng, int(rng.integers(20, 90)))) for _ in range(300)]
    v3 = [random_cuts(rng, len(p), int(rng.integers(1, 5))) for p in p3]
    p4 = []  # len < 20, HL > TL, TL > len, segments shorter than their header, protocol 47
    for proto in (6, 17, 1, 47):
        for ihl in (0, 3, 5, 9, 15):
            d = bytearray(rxgen.make_packet(rng, 64, proto=proto, ihl=max(ihl, 5)))
            d[0] = 0x40 | ihl
            hl = 4 * ihl
            for tl in (0, hl - 1, hl, hl + 1, hl + 3, hl + 7, hl + 19, len(d) - 1, len(d), len(d) + 1, 65535):
                if tl < 0:
                    continue
                e = bytearray(d)
                e[2], e[3] = tl >> 8, tl & 0xFF
                e = rxgen.tcp_contract(e)
                for ln in sorted({0, 1, 11, 12, 19, 20, hl, len(e)}):
                    if ln <= len(e):
                        p4.append(bytes(e[:ln]))
    v4 = [random_cuts(rng, len(p), int(rng.integers(1, 5))) for p in p4]
    lay = build(pk + p2 + p3 + p4, vw + v2 + v3 + v4, rng)
    want = check(lay, O.MODE_VERIFY_RX, dev, oracle_c)
    assert {0, 1, 2, 3, 6, 7, 8} <= set(int(x) for x in want[:, 0])  # every YU_RX_* outcome occurs
    for mode in (O.MODE_IPV4, O.MODE_VERIFY_IPV4, O.MODE_TX_DATAGRAM):
        check(lay, mode, dev, oracle_c)
    for mode in FILL:
        check(lay, mode, dev, oracle_c, fill=True)


# ---- 5. zero poles ------------------------------------------------------------------------
def test_zero_poles(dev, rng, oracle_c):
    pk, vw = [], []
    tags = []
    for seg in (4, 8, 63, 64, 1480):
        for fillbyte, tag in ((0x00, "zero"), (0xFF, "multiple")):
            d = bytearray(rxgen.make_packet(rng, seg, proto=1, ihl=5))
            d[20:] = bytes([fillbyte]) * seg  # all 0xFF, an even length: the words sum to a multiple of 65535
            for c in (0, 1, 20, 21, 22, 23, 24, len(d) // 2):
                pk.append(bytes(d)); vw.append([(0, c % 16, c), (1, (c + 1) % 4, len(d) - c)])
                tags.append("other" if fillbyte and seg % 2 else tag)
    # VERIFY_RX: an all-zero header (IHL 0: the header sum is over no byte) and an
    # empty segment (TotalLength 0): both sums are 0x0000; the usual ones are 0xFFFF
    for proto in (1, 6, 17):
        z = bytearray(24)
        z[9] = proto
        pk.append(bytes(z)); vw.append([(0, 3, 9), (1, 1, 15)]); tags.append("rx")
        z[3] = 24
        pk.append(bytes(z)); vw.append([(0, 2, 24)]); tags.append("rx")
        pk.append(bytes(rxgen.make_packet(rng, 40, proto=proto, ihl=5))); vw.append([(0, 1, 20), (1, 2, 40)])
        tags.append("rx")
    lay = build(pk, vw, rng)
    want = check(lay, O.MODE_TX_DATAGRAM, dev, oracle_c)
    tags = np.array(tags)
    assert (want[tags == "zero", 1] == 0xFFFF).all() and (tags == "zero").sum() >= 8
    assert (want[tags == "multiple", 1] == 0x0000).all() and (tags == "multiple").sum() >= 8
    check(lay, O.MODE_TX_DATAGRAM, dev, oracle_c, fill=True)
    rx = check(lay, O.MODE_VERIFY_RX, dev, oracle_c)
    assert (rx[tags == "rx", 0] & 1).all()
    check(lay, O.MODE_IPV4, dev, oracle_c)
    check(lay, O.MODE_VERIFY_IPV4, dev, oracle_c)


# ---- 6. counts ------------------------------------------------------------------------------
def count_layout(n, rng):
    a, oa = rxgen.rx_batch(rng, n - n // 2, hi=120, bad=0.3)
    b, ob = rxgen.tx_batch(rng, n // 2, hi=120, bad=0.2)
    pk, vw = cut_batch(rng, a, oa)
    p2, v2 = cut_batch(rng, b, ob)
    return build(pk + p2, vw + v2, rng)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_counts(n, dev, rng, oracle_c):
    lay = count_layout(n, rng)
    check(lay, O.MODE_VERIFY_RX, dev, oracle_c)
    check(lay, O.MODE_VERIFY_IPV4, dev, oracle_c)
    check(lay, O.MODE_TX_DATAGRAM, dev, oracle_c, fill=True)
    check(lay, O.MODE_IPV4, dev, oracle_c, fill=True)


_SECOND_PASS = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np, torch
import rxgen
from oracle import oracle as O
from yustack_amd import batch
dev = torch.device("cuda:0")
cus = torch.cuda.get_device_properties(dev).multi_processor_count
n = cus * 4 + 37          # one block per CU, four waves each: every wave takes a second, partial pass
rng = np.random.default_rng(5)
pk = [bytes(rxgen.make_packet(rng, 44, proto=(6, 17, 1)[i %% 3], ihl=5)) for i in range(64)]
pk = [pk[i %% 64] for i in range(n)]
hdr = np.zeros((n, 64), np.uint8)
pay = np.zeros((n, 44), np.uint8)
for i, p in enumerate(pk):
    hdr[i, :20] = np.frombuffer(p[:20], np.uint8)
    pay[i] = np.frombuffer(p[20:], np.uint8)
ar = torch.arange(n, device=dev)
vp = torch.stack((torch.zeros_like(ar), torch.ones_like(ar)), 1).reshape(-1)
vo = torch.stack((ar * 64, ar * 44), 1).reshape(-1)
vl = torch.tensor([20, 44], device=dev).repeat(n)
first = 2 * torch.arange(n + 1, device=dev)
pools = [torch.from_numpy(hdr).to(dev).reshape(-1), torch.from_numpy(pay).to(dev).reshape(-1)]
blob = np.frombuffer(b"".join(pk), np.uint8)
same = True
for mode in (O.MODE_VERIFY_RX, O.MODE_TX_DATAGRAM, O.MODE_IPV4, O.MODE_VERIFY_IPV4):
    got = batch.checksum_iov_datagrams(pools, vp, vo, vl, first, mode).cpu().numpy()
    want = O.C().batch(blob, mode, stride=64, length=64, n=n).reshape(-1)
    same = same and bool(np.array_equal(got, want))
print("same", same, n)
"""


def test_second_partial_pass_on_a_one_block_per_cu_grid():
    env = dict(os.environ, YU_TUNING="1", YU_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", _SECOND_PASS % (ROOT, os.path.join(ROOT, "tests"))],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split()[:2] == ["same", "True"], r.stdout
    assert "YU_BLOCKS_PER_CU=1" in r.stderr  # the knob was read


# ---- 7. out of contract -------------------------------------------------------------------
def run_unvalidated(lay, first, mode, fill, dev, oracle_c, bad):
    """A call with validate=False whose packets `bad` are out of contract: every other
    result and field exact, no field of the bad ones stored, and the run completes."""
    k = 2 if mode == O.MODE_TX_DATAGRAM else 1
    blob = lay.blob()
    want = oracle_c.batch(blob, mode, offsets=lay.offsets, threads=8).reshape(lay.n, k)
    pools, views, (vp, vo, vl, _) = lay.device(dev)
    got = batch.checksum_iov_datagrams(views, vp, vo, vl, first.to(dev), mode, fill=fill, validate=False)
    torch.cuda.synchronize()  # the call returns
    clean = np.setdiff1d(np.arange(lay.n), bad)
    assert np.array_equal(got.cpu().numpy().reshape(lay.n, k)[clean], want[clean]), (mode, fill)
    expect = expected_pools(lay, mode, blob, want, skip=set(bad)) if fill else lay.pools
    for a, e in zip(pools, expect):
        assert np.array_equal(a.cpu().numpy(), e), (mode, fill)
    return views, vp, vo, vl


@pytest.mark.parametrize("fill", (False, True))
def test_one_packet_over_the_limit(dev, rng, oracle_c, fill):
    pk = [bytes(rxgen.tx_packet(rng, 40 + i, proto=(6, 17, 1, 47)[i % 4])) for i in range(200)]
    vw = [[(0, i % 16, 20), (1, i % 4, len(p) - 20)] for i, p in enumerate(pk)]
    # 70000 bytes of valid memory that begin as a well-formed UDP datagram of 65535
    long = bytes(rxgen.tx_packet(rng, 65515, proto=17, ihl=5)) + bytes(rng.integers(0, 256, 4465, dtype=np.uint8))
    pk.insert(100, long)
    vw.insert(100, [(0, 2, 20), (1, 1, 30000), (1, 3, 39980)])
    lay = build(pk, vw, rng)
    for mode in (FILL if fill else MODES):
        views, vp, vo, vl = run_unvalidated(lay, torch.from_numpy(lay.first), mode, fill, dev, oracle_c, [100])
    with pytest.raises(ValueError):
        batch.checksum_iov_datagrams(views, vp, vo, vl, torch.from_numpy(lay.first).to(dev), "verify_rx")


@pytest.mark.parametrize("fill", (False, True))
def test_decreasing_first_is_out_of_contract_for_that_packet_only(dev, rng, oracle_c, fill):
    pk = [bytes(rxgen.tx_packet(rng, 40 + i, proto=(6, 17, 1, 47)[i % 4])) for i in range(50)]
    lay = build(pk, [[(0, i % 16, 20), (1, i % 4, len(p) - 20)] for i, p in enumerate(pk)], rng)
    bad = torch.from_numpy(lay.first.copy())
    bad[50] = 90  # first decreases at the last packet (views 98 .. 89): no other packet changes
    for mode in (FILL if fill else MODES):
        views, vp, vo, vl = run_unvalidated(lay, bad, mode, fill, dev, oracle_c, [49])
    with pytest.raises(ValueError):
        batch.checksum_iov_datagrams(views, vp, vo, vl, bad.to(dev), "verify_rx")
    if not fill:  # in the middle too, where the next packet takes other packets' views: read-only
        mid = torch.from_numpy(lay.first.copy())
        mid[21] = 30
        got = batch.checksum_iov_datagrams(views, vp, vo, vl, mid.to(dev), "verify_rx", validate=False)
        torch.cuda.synchronize()
        want = oracle_c.batch(lay.blob(), O.MODE_VERIFY_RX, offsets=lay.offsets)
        keep = np.delete(np.arange(50), (20, 21))
        assert np.array_equal(got.cpu().numpy()[keep], want[keep])


# ---- 8. shared views ------------------------------------------------------------------------
def test_shared_header_template(dev, rng, oracle_c):
    """Read-only: 64 packets name one header view (IP + UDP header), each with its own
    payload view; the header's sums verify for none or one of them, as the oracle says."""
    d = rxgen.make_packet(rng, 8 + 64, proto=17, ihl=5)
    pay = [(1 + i % 2, (5 * i) % 16, 64) for i in range(64)]
    lay = general_layout([[(0, 6, 28)]] + [[p] for p in pay], rng, npools=3)
    order = np.arange(64, 0, -1)
    vp = np.stack((np.full(64, lay.vp[0]), lay.vp[order]), 1).reshape(-1)
    vo = np.stack((np.full(64, lay.vo[0]), lay.vo[order]), 1).reshape(-1)
    vl = np.stack((np.full(64, 28), lay.vl[order]), 1).reshape(-1)
    shared = Layout(lay.pools, vp, vo, vl, 2 * np.arange(65))
    shared.put(np.arange(28), np.frombuffer(bytes(d[:28]), np.uint8))
    shared.put(np.arange(28, 92), np.frombuffer(bytes(d[28:]), np.uint8))  # packet 0 carries the summed payload
    for mode in MODES:
        check(shared, mode, dev, oracle_c)


def test_own_headers_shared_payload_in_place(dev, rng, oracle_c):
    """In place: each packet has its own header view (IP + transport header, where
    both fields lie) and all name one payload view."""
    hdrs = [rxgen.tx_packet(rng, 20 + 300, proto=(6, 17, 1)[i % 3], ihl=5 + i % 4) for i in range(48)]
    for h in hdrs:
        if h[9] == 6:
            h[4 * (h[0] & 15) + 12] = 0x50
    cut = [4 * (h[0] & 15) + 20 for h in hdrs]
    lay = general_layout([[(0, (3 * i) % 16, c)] for i, c in enumerate(cut)] + [[(1, 5, 300)]], rng)
    vp = np.stack((lay.vp[:48], np.full(48, 1)), 1).reshape(-1)
    vo = np.stack((lay.vo[:48], np.full(48, lay.vo[48])), 1).reshape(-1)
    vl = np.stack((lay.vl[:48], np.full(48, 300)), 1).reshape(-1)
    own = Layout(lay.pools, vp, vo, vl, 2 * np.arange(49))
    for i, (h, c) in enumerate(zip(hdrs, cut)):
        own.put(int(own.offsets[i]) + np.arange(c), np.frombuffer(bytes(h[:c]), np.uint8))
    for mode in MODES:
        check(own, mode, dev, oracle_c)
    for mode in FILL:
        check(own, mode, dev, oracle_c, fill=True)


# ---- 9. seeded fuzz ---------------------------------------------------------------------------
def test_fuzz(dev, oracle_c):
    rng = np.random.default_rng(78)
    for it in range(6):
        n = 500
        a, oa = rxgen.rx_batch(rng, n // 2, hi=int(rng.choice([60, 400, 1480])), bad=0.4)
        b, ob = rxgen.tx_batch(rng, n // 2, hi=int(rng.choice([60, 400, 1480])), bad=0.3)
        pk, vw = cut_batch(rng, a, oa, npools=3, nvmax=6)
        p2, v2 = cut_batch(rng, b, ob, npools=3, nvmax=6)
        pk, vw = pk + p2, vw + v2
        perm = rng.permutation(len(pk))
        pk, vw = [pk[i] for i in perm], [vw[i] for i in perm]
        lay = build(pk, vw, rng, npools=3)
        if it % 2:  # the packets in descending address order
            rev = np.arange(lay.n)[::-1]
            lay = lay.select(rev)
            assert (np.diff(lay.vo[lay.first[:-1][lay.lens > 0]]) < 0).sum() > lay.n // 2
        check_all(lay, dev, oracle_c)


# ---- 10. graph capture ------------------------------------------------------------------------
def test_graph_capture(dev, rng, oracle_c):
    lay = count_layout(500, rng)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    out = torch.zeros(500, dtype=torch.uint16, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        batch.checksum_iov_datagrams(views, vp, vo, vl, first, "verify_rx", out=out)  # warm up, validated
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            batch.checksum_iov_datagrams(views, vp, vo, vl, first, "verify_rx", out=out, validate=False)
    torch.cuda.current_stream(dev).wait_stream(s)
    for rep in range(2):
        blob = lay.blob()  # other bytes in the same views: damage 200 of them
        flip = rng.integers(0, blob.size - 1, 200)
        lay.put(flip, blob[flip] ^ 0x10)
        for k, p in enumerate(pools):
            p.copy_(torch.from_numpy(lay.pools[k]))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = oracle_c.batch(lay.blob(), O.MODE_VERIFY_RX, offsets=lay.offsets)
        assert np.array_equal(out.cpu().numpy(), want), rep


# ---- 11. known answers --------------------------------------------------------------------------
def test_known_answers(dev):
    """tests/golden/refexec.json (values recorded by executing the reference): whole
    datagrams, each split into a header view (the IPv4 header, as far as the packet
    holds it) and a payload view."""
    vecs = json.load(open(os.path.join(ROOT, "tests", "golden", "refexec.json")))["modes"]
    for mode in MODES:
        data, offs, _, _, want = refexec_mode_batch(vecs[str(mode)], mode)
        offs = offs.astype(np.int64)
        lens = np.diff(offs)
        n = len(lens)
        assert n >= 10
        hl = np.array([(int(data[offs[i]]) & 15) * 4 if lens[i] else 0 for i in range(n)])
        hl = np.minimum(hl, lens)
        hdr = np.zeros((n, 64), np.uint8)
        for i in range(n):
            hdr[i, :hl[i]] = data[offs[i]:offs[i] + hl[i]]
        pl = lens - hl
        po = np.concatenate(([0], np.cumsum(pl)))
        pay = np.zeros(int(po[-1]) + 1, np.uint8)
        for i in range(n):
            pay[po[i]:po[i + 1]] = data[offs[i] + hl[i]:offs[i + 1]]
        vp = torch.tensor([0, 1] * n, device=dev)
        vo = torch.from_numpy(np.stack((np.arange(n) * 64, po[:-1]), 1).reshape(-1)).to(dev)
        vl = torch.from_numpy(np.stack((hl, pl), 1).reshape(-1)).to(dev)
        got = batch.checksum_iov_datagrams([torch.from_numpy(hdr.reshape(-1)).to(dev), torch.from_numpy(pay).to(dev)],
                                           vp, vo, vl, 2 * torch.arange(n + 1, device=dev), mode)
        assert np.array_equal(got.cpu().numpy(), want), mode
