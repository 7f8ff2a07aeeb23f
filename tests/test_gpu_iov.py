"""Scatter-gather device batches (yu_csum_batch_iov / yu_csum_fill_iov through
batch.checksum_iov) on the GPU. Every result is compared bit for bit with the C
oracle's ragged batch over the same bytes laid back to back; the in-place form also
with every byte of every pool, guard bytes included.

The oracle's TX compositions index the fixed transport header (oracle/csum_oracle.c
or_packet: UDP 8, TCP 20, ICMP 4 bytes), so packets shorter than that are given to
the modes that define them (RAW, VERIFY_*) only, as in tests/test_gpu_parity.py. TCP
packets carry DataOffset 5 (byte 12 = 0x50), as every segment sendTCP encodes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from iov_layout import GUARD, Layout, general_layout, two_view_layout  # noqa: F401 - shared with the kernel ledger
from oracle import oracle as O
from test_oracle import refexec_mode_batch
from yustack_amd import batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (O.MODE_RAW, O.MODE_UDP, O.MODE_TCP, O.MODE_ICMP, O.MODE_VERIFY_TCP, O.MODE_VERIFY_UDP)
TX = (O.MODE_UDP, O.MODE_TCP, O.MODE_ICMP)
MIN_LEN = {O.MODE_UDP: 8, O.MODE_TCP: 20, O.MODE_ICMP: 4}
PSEUDO = (O.MODE_UDP, O.MODE_TCP, O.MODE_VERIFY_TCP, O.MODE_VERIFY_UDP)


def side_args(mode, kind, n, rng, dev):
    """(oracle kwargs, checksum_iov kwargs) with the side data given as `kind`."""
    if kind == "addrs" and mode in PSEUDO:
        a = rng.integers(0, 256, 8 * n, dtype=np.uint8)
        return {"addrs": a}, {"addrs": torch.from_numpy(a).to(dev)}
    if kind == "initial_arr" or kind == "addrs":
        ia = rng.integers(0, 65536, n, dtype=np.uint16)
        ia[: min(n, 4)] = (0, 0xFFFF, 1, 0xFFFE)[: min(n, 4)]
        return {"initial_arr": ia}, {"initial_arr": torch.from_numpy(ia).to(dev)}
    init = int(rng.integers(0, 65536)) if kind == "initial" else int(kind)
    return {"initial": init}, {"initial": init}


def check(lay, mode, kind, dev, rng, oracle_c, fill=False, with_out=True, min_len=None):
    """One call on the packets of `lay` the oracle defines for `mode`."""
    lay = lay.at_least(MIN_LEN.get(mode, 0) if min_len is None else min_len)
    blob = lay.blob()
    okw, gkw = side_args(mode, kind, lay.n, rng, dev)
    want = oracle_c.batch(blob, mode, offsets=lay.offsets, threads=8, **okw)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    guard = 64
    out = torch.full((lay.n + guard,), 0xA5A5, dtype=torch.uint16, device=dev)
    got = batch.checksum_iov(views, vp, vo, vl, first, mode, fill=fill, out=out[:lay.n] if with_out else None,
                             **gkw)
    if fill and not with_out:
        assert got.numel() == lay.n
    res = got.cpu().numpy()
    bad = np.flatnonzero(res != want)
    assert bad.size == 0, (mode, kind, fill, bad[:8], lay.lens[bad[:8]], res[bad[:8]], want[bad[:8]])
    assert (out[lay.n:].cpu().numpy() == 0xA5A5).all()
    after = [p.cpu().numpy() for p in pools]
    expect = lay.filled(mode, want) if fill else lay.pools
    for k, (a, e) in enumerate(zip(after, expect)):
        diff = np.flatnonzero(a != e)
        assert diff.size == 0, (mode, kind, fill, k, diff[:8])
    return lay


@pytest.fixture(scope="module")
def rng():
    return np.random.default_rng(20261019)


# ---- 1. splits (and 8: the same in place) -------------------------------------
def split_cases():
    """Lengths 0..130, 255..257, 1023..1025 and 1500, split at every position. Up to
    40 bytes every (first view mod 16, second view mod 4) pair; above, every split
    takes each first-view alignment once with the second view's alignment cycling, so
    each length still sees all 64 pairs and every pair both split parities (the
    kernel's arithmetic treats the two views independently: each view's sum depends on
    its own address mod 4, its length and the parity of its offset in the packet)."""
    L, C, A1, A2 = [], [], [], []
    for ln in list(range(131)) + [255, 256, 257, 1023, 1024, 1025, 1500]:
        c = np.arange(ln + 1)
        if ln <= 40:
            cc, a1, a2 = np.meshgrid(c, np.arange(16), np.arange(4), indexing="ij")
        elif ln <= 130:
            cc, a1 = np.meshgrid(c, np.arange(16), indexing="ij")
            a2 = (cc // 2 + a1) % 4
        else:  # one placement per split, cycling through the 64 pairs
            cc = c
            a1 = c % 16
            a2 = (c // 16 + c // 2) % 4
        L.append(np.full(cc.size, ln))
        C.append(cc.reshape(-1))
        A1.append(np.asarray(a1).reshape(-1))
        A2.append(np.asarray(a2).reshape(-1))
    return tuple(np.concatenate(x) for x in (L, C, A1, A2))


@pytest.fixture(scope="module")
def split_layout(rng):
    return two_view_layout(*split_cases(), rng)


SIDE_OF = {O.MODE_RAW: ("initial_arr", "initial", 0xFFFF), O.MODE_UDP: ("addrs", "initial"),
           O.MODE_TCP: ("addrs", "initial_arr"), O.MODE_ICMP: ("initial",),
           O.MODE_VERIFY_TCP: ("addrs", "initial_arr", "initial"), O.MODE_VERIFY_UDP: ("addrs", 0)}


@pytest.mark.parametrize("mode", MODES)
def test_splits(split_layout, mode, dev, rng, oracle_c):
    for kind in SIDE_OF[mode]:
        check(split_layout, mode, kind, dev, rng, oracle_c)


@pytest.mark.parametrize("mode", TX)
def test_splits_in_place(split_layout, mode, dev, rng, oracle_c):
    check(split_layout, mode, "addrs", dev, rng, oracle_c, fill=True)
    check(split_layout, mode, "initial", dev, rng, oracle_c, fill=True, with_out=False)


# ---- 2. the field across views ---------------------------------------------------
def field_packets():
    pk = []
    for al in range(4):
        for cut in (6, 7, 8, 16, 17, 18, 2, 3, 4):
            pk.append([(0, al, cut), (1, (al + cut) % 4, 60 - cut)])
            pk.append([(1, al, cut), (1, 3 - al, 41 - cut)])
        pk.append([(al % 2, (al + i) % 16, 1) for i in range(40)])              # forty 1-byte views
        pk.append([(0, 0, 0), (0, al, 5), (1, 0, 0), (1, 0, 0), (1, al, 33), (0, 0, 0)])  # empty views around
        pk.append([(0, 0, 0), (0, 0, 0)])
    return pk


@pytest.mark.parametrize("fill", (False, True))
def test_field_across_views(dev, rng, oracle_c, fill):
    lay = general_layout(field_packets(), rng)  # (NULL bases: test_null_base_empty_views)
    for mode in (TX if fill else MODES):
        for kind in ("addrs", "initial"):
            check(lay, mode, kind, dev, rng, oracle_c, fill=fill)


def test_null_base_empty_views(dev, rng, oracle_c):
    """yu_iovec tables written by hand: empty views with base NULL (and a wild
    base) before, between and after the others."""
    from yustack_amd import _lib
    a = torch.from_numpy(rng.integers(0, 256, 300, dtype=np.uint8)).to(dev)
    b = torch.from_numpy(rng.integers(0, 256, 300, dtype=np.uint8)).to(dev)
    a[12 + 3] = 0x50
    recs = [(0, 0), (a.data_ptr() + 3, 20), (0, 0), (0xDEAD0001, 0), (b.data_ptr() + 1, 77), (0, 0),  # packet 0
            (0, 0),                                                                                  # packet 1: empty
            (b.data_ptr() + 100, 9), (0, 0), (a.data_ptr() + 64, 64)]                                 # packet 2
    first = [0, 6, 7, 10]
    table = torch.tensor(recs, dtype=torch.int64, device=dev)
    fi = torch.tensor(first, dtype=torch.int64, device=dev)
    ha, hb = a.cpu().numpy(), b.cpu().numpy()
    pk = [np.concatenate((ha[3:23], hb[1:78])), np.zeros(0, np.uint8), np.concatenate((hb[100:109], ha[64:128]))]
    offs = np.concatenate(([0], np.cumsum([len(x) for x in pk]))).astype(np.uint64)
    blob = np.concatenate(pk + [np.zeros(1, np.uint8)])
    for mode in (O.MODE_RAW, O.MODE_VERIFY_TCP, O.MODE_VERIFY_UDP):
        out = torch.zeros(3, dtype=torch.uint16, device=dev)
        rc = _lib.lib().yu_csum_batch_iov(table.data_ptr(), fi.data_ptr(), 3, mode, None, 0x1234, None,
                                          out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
        want = oracle_c.batch(blob, mode, offsets=offs, initial=0x1234)
        assert np.array_equal(out.cpu().numpy(), want), mode


# ---- 3. long views and many views -------------------------------------------------
@pytest.mark.parametrize("fill", (False, True))
def test_long_and_many_views(dev, rng, oracle_c, fill):
    pk = [[(0, 5, n)] for n in (4096, 4097, 9001, 65535)]
    pk.append([(1, 3, 1), (0, 7, 65533), (1, 2, 1)])
    pk.append([(i % 2, (3 * i) % 16, 7) for i in range(200)])
    pk.append([(1, 1, 20), (0, 9, 1480)])
    lay = general_layout(pk, rng)
    for mode in (TX if fill else MODES):
        check(lay, mode, "addrs", dev, rng, oracle_c, fill=fill)
        check(lay, mode, "initial", dev, rng, oracle_c, fill=fill)


# ---- 4. zero-ness -------------------------------------------------------------------
def test_zero_ness(dev, rng, oracle_c):
    """TCP needs DataOffset >= 5 in byte 12, which an all-zero packet cannot carry:
    all-0xFF segments (DataOffset 15) of at least 60 bytes take it, the others the
    five remaining modes."""
    not_tcp = tuple(m for m in MODES if m != O.MODE_TCP)
    for fillbyte in (0x00, 0xFF):
        pk = []
        for ln in (0, 1, 2, 20, 21, 64, 1025, 1500):
            for cut in sorted({0, 1, 2, 7, 8, ln // 2, ln} & set(range(ln + 1))):
                pk.append([(0, cut % 16, cut), (1, (cut + 1) % 4, ln - cut)])
        lay = general_layout(pk, rng, fillbyte=fillbyte)
        for mode in not_tcp:
            for kind in (0, 0xFFFF):
                check(lay, mode, kind, dev, rng, oracle_c)
        if fillbyte == 0xFF:
            check(lay, O.MODE_TCP, 0xFFFF, dev, rng, oracle_c, min_len=60)
    # the only nonzero byte is the last byte of the last view
    pk = [[(0, a, 20), (1, a % 4, ln), (0, 0, 0), (1, 3, 1)] for a in range(8) for ln in (0, 1, 43, 1480)]
    lay = general_layout(pk, rng, fillbyte=0x00)
    last = lay.offsets[1:].astype(np.int64) - 1
    for q, p in enumerate(lay.pools):
        sel = lay.bpool[last] == q
        p[lay.bpos[last][sel]] = 0x01
    for mode in not_tcp:
        check(lay, mode, 0, dev, rng, oracle_c)


# ---- 5. sharing and order ---------------------------------------------------------
def test_shared_header_descending_order_three_pools(dev, rng, oracle_c):
    # 64 packets share one 20-byte header view, each with its own payload, the
    # payloads listed in descending address order, over three allocations
    pay = [(1 + i % 2, (5 * i) % 16, 30 + 23 * i) for i in range(64)]
    lay = general_layout([[(0, 6, 20)]] + [[p] for p in pay], rng, npools=3)
    hdr = (lay.vp[0], lay.vo[0], lay.vl[0])
    order = np.arange(64, 0, -1)  # views 64..1: descending addresses within each pool
    vp = np.stack((np.full(64, hdr[0]), lay.vp[order]), 1).reshape(-1)
    vo = np.stack((np.full(64, hdr[1]), lay.vo[order]), 1).reshape(-1)
    vl = np.stack((np.full(64, hdr[2]), lay.vl[order]), 1).reshape(-1)
    shared = Layout(lay.pools, vp, vo, vl, 2 * np.arange(65))
    assert (np.diff(shared.vo[1::2][shared.vp[1::2] == 1]) < 0).all()
    for mode in MODES:
        check(shared, mode, "addrs", dev, rng, oracle_c)
    # a payload before its header in memory, and both views in one pool
    pk = [[(0, 3, 0)], [(0, 9, 1000)], [(0, 1, 20)]]
    lay = general_layout(pk, rng, npools=1)
    rev = Layout(lay.pools, [0, 0], [lay.vo[2], lay.vo[1]], [20, 1000], [0, 2])
    for mode in MODES:
        check(rev, mode, "initial", dev, rng, oracle_c)


def test_own_headers_in_place(dev, rng, oracle_c):
    # 64 packets, each with its own header in a 64-byte-pitch header pool and its
    # payload in another allocation
    pk = [[(0, 0, 20), (1 + i % 2, (7 * i) % 16, 30 + 23 * i)] for i in range(64)]
    lay = general_layout(pk, rng, npools=3)
    for mode in TX:
        check(lay, mode, "addrs", dev, rng, oracle_c, fill=True)
        check(lay, mode, "initial_arr", dev, rng, oracle_c, fill=True, with_out=False)


# ---- 6. counts ----------------------------------------------------------------------
def count_layout(n, rng):
    ln = rng.integers(20, 200, n)
    return two_view_layout(ln, rng.integers(0, ln + 1), rng.integers(0, 16, n), rng.integers(0, 4, n), rng)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_counts(n, dev, rng, oracle_c):
    lay = count_layout(n, rng)
    check(lay, O.MODE_RAW, "initial_arr", dev, rng, oracle_c)
    check(lay, O.MODE_TCP, "addrs", dev, rng, oracle_c, fill=True)


_SECOND_PASS = r"""
import sys
sys.path.insert(0, %r)
import numpy as np, torch
from oracle import oracle as O
from yustack_amd import batch
dev = torch.device("cuda:0")
cus = torch.cuda.get_device_properties(dev).multi_processor_count
n = cus * 4 + 37          # one block per CU, four waves each: every wave takes a second, partial pass
rng = np.random.default_rng(5)
hdr = rng.integers(0, 256, (n, 64), dtype=np.uint8)
hdr[:, 12] = 0x50
pay = rng.integers(0, 256, (n, 44), dtype=np.uint8)
ar = torch.arange(n, device=dev)
vp = torch.stack((torch.zeros_like(ar), torch.ones_like(ar)), 1).reshape(-1)
vo = torch.stack((ar * 64, ar * 44), 1).reshape(-1)
vl = torch.tensor([20, 44], device=dev).repeat(n)
first = 2 * torch.arange(n + 1, device=dev)
addrs = rng.integers(0, 256, 8 * n, dtype=np.uint8)
got = batch.checksum_iov([torch.from_numpy(hdr).to(dev).reshape(-1), torch.from_numpy(pay).to(dev).reshape(-1)],
                         vp, vo, vl, first, "tcp", addrs=torch.from_numpy(addrs).to(dev)).cpu().numpy()
blob = np.concatenate((hdr[:, :20], pay), 1).reshape(-1)
want = O.C().batch(blob, O.MODE_TCP, stride=64, length=64, n=n, addrs=addrs)
print("same", bool(np.array_equal(got, want)), n)
"""


def test_second_partial_pass_on_a_one_block_per_cu_grid():
    env = dict(os.environ, YU_TUNING="1", YU_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", _SECOND_PASS % ROOT], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split()[:2] == ["same", "True"], r.stdout
    assert "YU_BLOCKS_PER_CU=1" in r.stderr  # the knob was read


# ---- 7. known answers ---------------------------------------------------------------
def test_known_answers(dev):
    """tests/golden/refexec.json (values recorded by executing the reference), each
    packet split where the reference's sender splits it: after the transport header."""
    vecs = json.load(open(os.path.join(ROOT, "tests", "golden", "refexec.json")))["modes"]
    for mode in (O.MODE_UDP, O.MODE_TCP, O.MODE_ICMP, O.MODE_VERIFY_TCP):
        data, offs, addrs, init, want = refexec_mode_batch(vecs[str(mode)], mode)
        offs = offs.astype(np.int64)
        lens = np.diff(offs)
        if mode in (O.MODE_TCP, O.MODE_VERIFY_TCP):
            hl = (data[offs[:-1] + 12] >> 4).astype(np.int64) * 4
        else:
            hl = np.full(len(lens), 8 if mode == O.MODE_UDP else 4)
        hl = np.minimum(hl, lens)
        n = len(lens)
        # headers in one tensor at a 64-byte pitch, payloads packed in another
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
        got = batch.checksum_iov([torch.from_numpy(hdr.reshape(-1)).to(dev), torch.from_numpy(pay).to(dev)],
                                 vp, vo, vl, 2 * torch.arange(n + 1, device=dev), mode,
                                 addrs=None if addrs is None else torch.from_numpy(addrs).to(dev))
        assert np.array_equal(got.cpu().numpy(), want), mode


# ---- 9. out of contract ---------------------------------------------------------------
@pytest.mark.parametrize("fill", (False, True))
def test_one_packet_over_the_limit(dev, rng, oracle_c, fill):
    pk = [[(0, i % 16, 20), (1, i % 4, 40 + i)] for i in range(200)]
    pk.insert(100, [(0, 2, 20), (1, 1, 30000), (1, 3, 39980)])  # 70000 bytes of valid memory
    lay = general_layout(pk, rng)
    clean = np.delete(np.arange(201), 100)
    mode = O.MODE_TCP
    sub = lay.select(clean)
    addrs = rng.integers(0, 256, 8 * 201, dtype=np.uint8)
    want = oracle_c.batch(sub.blob(), mode, offsets=sub.offsets, addrs=addrs.reshape(201, 8)[clean].reshape(-1))
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    with pytest.raises(ValueError):
        batch.checksum_iov(views, vp, vo, vl, first, mode, addrs=torch.from_numpy(addrs).to(dev))
    got = batch.checksum_iov(views, vp, vo, vl, first, mode, addrs=torch.from_numpy(addrs).to(dev), fill=fill,
                             validate=False)
    torch.cuda.synchronize()  # the call returns
    assert np.array_equal(got.cpu().numpy()[clean], want)
    expect = sub.filled(mode, want) if fill else lay.pools  # no byte of the long packet is written
    for a, e in zip(pools, expect):
        assert np.array_equal(a.cpu().numpy(), e)


def test_decreasing_first_is_out_of_contract_for_that_packet_only(dev, rng, oracle_c):
    pk = [[(0, i % 16, 20), (1, i % 4, 40 + i)] for i in range(50)]
    lay = general_layout(pk, rng)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    bad = first.clone()
    bad[21] = 30  # first decreases at packet 20 (views 40 .. 29); packet 21 becomes views 30 .. 43
    got = batch.checksum_iov(views, vp, vo, vl, bad, O.MODE_RAW, initial=7, validate=False)
    torch.cuda.synchronize()
    want = oracle_c.batch(lay.blob(), O.MODE_RAW, offsets=lay.offsets, initial=7)
    keep = np.delete(np.arange(50), (20, 21))
    assert np.array_equal(got.cpu().numpy()[keep], want[keep])
    with pytest.raises(ValueError):
        batch.checksum_iov(views, vp, vo, vl, bad, O.MODE_RAW, initial=7)


# ---- 10. seeded fuzz --------------------------------------------------------------------
def test_fuzz(dev, oracle_c):
    rng = np.random.default_rng(77)
    for it in range(200):
        n = int(rng.integers(1, 301))
        npools = int(rng.integers(1, 4))
        pk = []
        for _ in range(n):
            nv = int(rng.integers(0, 7))
            lens = rng.integers(0, 2001, nv) * (rng.random(nv) < 0.8)
            if rng.random() < 0.5:
                lens = lens % 80
            pk.append([(int(rng.integers(0, npools)), int(rng.integers(0, 16)), int(x)) for x in lens])
        lay = general_layout(pk, rng, npools=npools)
        mode = MODES[int(rng.integers(0, len(MODES)))]
        fill = mode in TX and rng.random() < 0.5
        kind = ("addrs", "initial_arr", "initial")[int(rng.integers(0, 3))]
        check(lay, mode, kind, dev, rng, oracle_c, fill=fill, with_out=bool(rng.random() < 0.8) or not fill)


# ---- 11. graph capture --------------------------------------------------------------------
def test_graph_capture(dev, rng, oracle_c):
    lay = count_layout(500, rng)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    addrs = torch.from_numpy(rng.integers(0, 256, 8 * 500, dtype=np.uint8)).to(dev)
    out = torch.zeros(500, dtype=torch.uint16, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        batch.checksum_iov(views, vp, vo, vl, first, "verify_tcp", addrs=addrs, out=out)  # warm up, validated
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            batch.checksum_iov(views, vp, vo, vl, first, "verify_tcp", addrs=addrs, out=out, validate=False)
    torch.cuda.current_stream(dev).wait_stream(s)
    for rep in range(2):
        for k, p in enumerate(pools):
            lay.pools[k] = rng.integers(0, 256, p.numel(), dtype=np.uint8)
            p.copy_(torch.from_numpy(lay.pools[k]))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = oracle_c.batch(lay.blob(), O.MODE_VERIFY_TCP, offsets=lay.offsets, addrs=addrs.cpu().numpy())
        assert np.array_equal(out.cpu().numpy(), want), rep


# ---- 12. Python validation --------------------------------------------------------------
def test_python_validation(dev, rng):
    lay = count_layout(10, rng)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    past = vl.clone()
    past[3] = views[int(vp[3])].numel() - int(vo[3]) + 1  # one byte past its pool
    with pytest.raises(ValueError, match="pool"):
        batch.checksum_iov(views, vp, vo, past, first, "raw")
    dec = first.clone()
    dec[4] = 2
    with pytest.raises(ValueError, match="first"):
        batch.checksum_iov(views, vp, vo, vl, dec, "raw")
    far = first.clone()
    far[-1] = 21
    with pytest.raises(ValueError, match="first"):
        batch.checksum_iov(views, vp, vo, vl, far, "raw")
    wrong = vp.clone()
    wrong[0] = 2
    with pytest.raises(ValueError, match="pool"):
        batch.checksum_iov(views, wrong, vo, vl, first, "raw")
    assert batch.checksum_iov(views, vp, vo, vl, first, "raw").numel() == 10
