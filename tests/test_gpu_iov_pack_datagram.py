"""Whole IPv4 datagrams held as scatter-gather device packets, verified or filled
and packed in one pass (yu_csum_pack_iov_datagram / yu_csum_pack_fill_iov_datagram
through batch.pack_iov_datagrams) on the GPU: IPV4, VERIFY_IPV4, VERIFY_RX and
TX_DATAGRAM.

Per call: every result against the C oracle's ragged batch over the same bytes laid
back to back; ALL of dst, with 128-byte guards on both sides and every slack byte
(prefilled 0xA5), against the expected image (tests/test_gpu_iov_pack.py's `image`,
plus, in the fill form, the fields tests/test_gpu_contract.py::_fields gives);
every pool unchanged byte for byte; out's guard. No packet is filtered: the oracle
defines the four modes at every length. Datagrams come from tests/rxgen.py, which
keeps the one input condition YU_MODE_TCP makes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rxgen
from iov_layout import GUARD, Layout, general_layout, two_view_layout
from oracle import oracle as O
from test_gpu_contract import _fields
from test_gpu_iov_datagram import FILL, MODES, build, count_layout, cut_batch, datagram, put_packets, random_cuts
from test_gpu_iov_pack import image, slack_offsets, tight
from test_oracle import refexec_mode_batch
from yustack_amd import _lib, batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rng():
    return np.random.default_rng(20261020)


def dg_image(lay, blob, do, total, base, mode=None, want=None, skip=()):
    """pack's image; with `want` (the fill form) the fields of the packed copy."""
    exp = image(lay, blob, do, total, base, skip=skip)
    if want is not None:
        offs = lay.offsets.astype(np.int64)
        for i in range(lay.n):
            if i in skip:
                continue
            for at, val in _fields(mode, blob, int(offs[i]), int(offs[i + 1]), [int(x) for x in want[i]]):
                exp[GUARD + base + int(do[i]) + at - int(offs[i])] = val & 0xFF
    return exp


_base = [0]


def pcheck(lay, mode, dev, oracle_c, fill=False, with_out=True, offsets=tight):
    """One packing call on every packet of `lay`; the dst base offset cycles 0..15
    from call to call. Returns (want, buf, base, do)."""
    k = 2 if mode == O.MODE_TX_DATAGRAM else 1
    blob = lay.blob()
    want = oracle_c.batch(blob, mode, offsets=lay.offsets, threads=8).reshape(lay.n, k)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    base = _base[0] = (_base[0] + 1) % 16
    do = offsets(lay)
    total = GUARD + base + int(do[-1]) + GUARD
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    dst = buf[GUARD + base:GUARD + base + int(do[-1])]
    dofs = torch.from_numpy(do).to(dev)
    out = torch.full((1 + lay.n * k + 64,), 0xA5A5, dtype=torch.uint16, device=dev)  # 2- but not 4-byte aligned
    got, d2, o2 = batch.pack_iov_datagrams(views, vp, vo, vl, first, mode, fill=fill, dst=dst, dst_offsets=dofs,
                                           out=out[1:1 + lay.n * k] if with_out else None)
    assert d2 is dst and o2 is dofs and got.numel() == lay.n * k
    res = got.cpu().numpy().reshape(lay.n, k)
    bad = np.flatnonzero((res != want).any(1))
    assert bad.size == 0, (mode, fill, bad[:8], lay.lens[bad[:8]], res[bad[:8]], want[bad[:8]])
    assert int(out[0]) == 0xA5A5 and (out[1 + lay.n * k:].cpu().numpy() == 0xA5A5).all()
    exp = dg_image(lay, blob, do, total, base, mode, want if fill else None)
    diff = np.flatnonzero(buf.cpu().numpy() != exp)
    assert diff.size == 0, (mode, fill, base, diff[:8] - GUARD - base)
    for q, (a, e) in enumerate(zip(pools, lay.pools)):
        assert np.array_equal(a.cpu().numpy(), e), (mode, fill, q)  # the sources are never written
    return want, buf, base, do


def pcheck_all(lay, dev, oracle_c, offsets=(tight, slack_offsets)):
    for off in offsets:
        for mode in MODES:
            pcheck(lay, mode, dev, oracle_c, offsets=off)
        for mode in FILL:
            pcheck(lay, mode, dev, oracle_c, fill=True, offsets=off)
    pcheck(lay, O.MODE_TX_DATAGRAM, dev, oracle_c, fill=True, with_out=False)


# ---- 1. header splits ---------------------------------------------------------------
@pytest.fixture(scope="module")
def split_layout(rng):
    """tests/test_gpu_iov_datagram.py's grid: IHL 5, 6, 15; segments of 0, 1, 7, 8, 64
    and 1480 bytes of each protocol; two views split at every position 0..HL+20, the
    views' addresses rotating through every value mod 16 / mod 4."""
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


def test_slack_offsets_take_every_start(split_layout):
    assert set(slack_offsets(split_layout)[:-1] % 16) == set(range(16))
    assert set(tight(split_layout)[:-1] % 16) == set(range(16))


@pytest.mark.parametrize("offsets", (tight, slack_offsets))
@pytest.mark.parametrize("mode", MODES)
def test_header_splits(split_layout, mode, offsets, dev, oracle_c):
    pcheck(split_layout, mode, dev, oracle_c, offsets=offsets)


@pytest.mark.parametrize("offsets", (tight, slack_offsets))
@pytest.mark.parametrize("mode", FILL)
def test_header_splits_fill(split_layout, mode, offsets, dev, oracle_c):
    pcheck(split_layout, mode, dev, oracle_c, fill=True, offsets=offsets)
    pcheck(split_layout, mode, dev, oracle_c, fill=True, with_out=False, offsets=offsets)


def test_fill_without_out_at_the_abi(dev, rng, oracle_c):
    """out == NULL in the fill form: the fields are stored all the same."""
    pk = [rxgen.tx_packet(rng, 40 + i, proto=(6, 17, 1)[i % 3]) for i in range(30)]
    lay = build(pk, [[(0, i % 16, 11), (1, i % 4, len(p) - 11)] for i, p in enumerate(pk)], rng)
    blob = lay.blob()
    want = oracle_c.batch(blob, O.MODE_TX_DATAGRAM, offsets=lay.offsets).reshape(lay.n, 2)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    vbase = torch.where(vp == 0, vo + views[0].data_ptr(), vo + views[1].data_ptr())
    table = torch.stack((vbase, vl), 1).contiguous()
    do = tight(lay)
    total = int(do[-1]) + 2 * GUARD
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    dofs = torch.from_numpy(do).to(dev)
    rc = _lib.lib().yu_csum_pack_fill_iov_datagram(table.data_ptr(), first.data_ptr(), lay.n, O.MODE_TX_DATAGRAM,
                                                   buf.data_ptr() + GUARD, dofs.data_ptr(), None,
                                                   torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), dg_image(lay, blob, do, total, 0, O.MODE_TX_DATAGRAM, want))


# ---- 2. field bytes across views and parities -----------------------------------------
def test_field_bytes_across_views(dev, rng, oracle_c):
    """Bytes 10|11 and the transport field's two bytes in different views, one-byte
    and empty views around them; tight and slack offsets and the moving base put each
    at even and odd destination addresses."""
    pk, vw = [], []
    for proto in (6, 17, 1):
        for ihl in (5, 6, 15):
            d = rxgen.tx_packet(rng, 60, proto=proto, ihl=ihl)
            f = 4 * ihl + {6: 16, 17: 6, 1: 2}[proto]
            rest = len(d) - f - 2
            for al in range(4):
                # a cut between 10 and 11, and between the field's bytes
                pk.append(d); vw.append([(0, al, 11), (1, al + 1, f - 10), (0, 2 * al, rest + 1)])
                # each of the four bytes alone in a one-byte view, empty views between
                pk.append(d); vw.append([(0, al, 10), (1, al, 1), (0, 0, 0), (1, al + 2, 1), (0, al + 1, f - 12),
                                         (1, 3 - al, 1), (0, 0, 0), (0, al, 1), (1, al, rest)])
                # both pairs inside one view that starts right at them
                pk.append(d); vw.append([(1, al, 10), (0, al + 5, f - 10), (1, al + 9, rest + 2)])
    # 70 empty or one-byte views: the header lies past the 64 records the lanes hold
    for proto in (6, 17, 1):
        d = rxgen.tx_packet(rng, 100, proto=proto, ihl=5)
        pk.append(d); vw.append([(0, 0, 0)] * 70 + [(0, 7, 9), (1, 2, 20), (0, 0, 0), (1, 1, len(d) - 29)])
        pk.append(d); vw.append([(i % 2, (3 * i) % 16, 1) for i in range(70)] + [(1, 3, len(d) - 70)])
        pk.append(d); vw.append([v for i in range(40) for v in ((i % 2, (5 * i) % 16, 1), (1, 0, 0))] +
                                [(0, 1, len(d) - 40)])
    pk.append(bytearray()); vw.append([(0, 0, 0)] * 3)
    pk.append(bytearray()); vw.append([])
    lay = build(pk, vw, rng)
    pcheck_all(lay, dev, oracle_c)
    pcheck_all(lay, dev, oracle_c)  # the base has moved on by an odd count: the other parity


# ---- 3. window seams --------------------------------------------------------------------
def test_window_seams(dev, rng, oracle_c):
    pk, vw = [], []
    for proto in (6, 17, 1):
        hl = 20
        d = rxgen.make_packet(rng, 200, proto=proto, ihl=5)
        tl = len(d)
        tail = bytes(rng.integers(0, 256, 37, dtype=np.uint8))
        for al in (0, 1, 2, 3):
            # HL at, one before and one after a view boundary
            for e in (-1, 0, 1):
                pk.append(d); vw.append([(0, al, hl + e), (1, al + 1, tl - hl - e)])
            # TL < len: trailing bytes (copied, not summed) in the same view, a later view;
            # TL one before, at and one after a view boundary
            pk.append(d + tail); vw.append([(0, al, hl), (1, 3 - al, tl - hl + 37)])
            for e in (-1, 0, 1):
                pk.append(d + tail); vw.append([(0, al, hl + 11), (1, al + 8, tl - hl - 11 + e), (0, al + 1, 37 - e)])
            # TL > len: the datagram is cut short
            pk.append(d[:tl - 1]); vw.append([(0, al, hl), (1, al + 2, tl - hl - 1)])
            pk.append(d[:hl + 3]); vw.append([(0, al, hl + 3)])
    # HL and TL at, one before and one after a 1024-byte slot boundary: one view whose
    # window starts at its address mod 4, and a header view in front of the segment
    for i, proto in enumerate((6, 17, 1)):
        for seg in (1024 - 20 - 1, 1024 - 20, 1024 - 20 + 1, 1023, 1024, 1025, 2047, 2048, 2049, 4097):
            d = rxgen.make_packet(rng, seg, proto=proto, ihl=5)
            for al in (0, 1, 3):
                pk.append(d + bytes(5)); vw.append([(0, al, len(d) + 5)])
                pk.append(d + b"\x01\x02\x03"); vw.append([(0, al + 4, 20), (1, al, seg + 3)])
        for ihl in (5, 6):  # HL next to the seam: 1004..1028 bytes of one-byte-shifted views in front
            d = rxgen.make_packet(rng, 1100, proto=proto, ihl=ihl)
            for c in (4 * ihl - 1, 4 * ihl, 4 * ihl + 1, 4 * ihl + 1023, 4 * ihl + 1024, 4 * ihl + 1025):
                pk.append(d); vw.append([(0, i, c), (1, i + 1, len(d) - c)])
    lay = build(pk, vw, rng)
    pcheck_all(lay, dev, oracle_c)


# ---- 4. malformed and zero poles --------------------------------------------------------
def test_malformed(dev, rng, oracle_c):
    pk, vw = cut_batch(rng, *rxgen.rx_batch(rng, 500, hi=300, bad=0.5))
    p2, v2 = cut_batch(rng, *rxgen.tx_batch(rng, 500, hi=300, bad=0.3))
    p3 = [bytes(rxgen.short_header_packet(rng, int(rng.integers(20, 90)))) for _ in range(200)]
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
    want, *_ = pcheck(lay, O.MODE_VERIFY_RX, dev, oracle_c, offsets=slack_offsets)
    assert {0, 1, 2, 3, 6, 7, 8} <= set(int(x) for x in want[:, 0])  # every YU_RX_* outcome occurs
    for mode in (O.MODE_IPV4, O.MODE_VERIFY_IPV4, O.MODE_TX_DATAGRAM):
        pcheck(lay, mode, dev, oracle_c)
    for mode in FILL:
        pcheck(lay, mode, dev, oracle_c, fill=True)
        pcheck(lay, mode, dev, oracle_c, fill=True, offsets=slack_offsets)


def test_zero_poles(dev, rng, oracle_c):
    pk, vw, tags = [], [], []
    for seg in (4, 8, 63, 64, 1480):
        for fillbyte, tag in ((0x00, "zero"), (0xFF, "multiple")):
            d = bytearray(rxgen.make_packet(rng, seg, proto=1, ihl=5))
            d[20:] = bytes([fillbyte]) * seg  # all 0xFF, an even length: the words sum to a multiple of 65535
            for c in (0, 1, 20, 21, 22, 23, 24, len(d) // 2):
                pk.append(bytes(d)); vw.append([(0, c % 16, c), (1, (c + 1) % 4, len(d) - c)])
                tags.append("other" if fillbyte and seg % 2 else tag)
    for proto in (1, 6, 17):
        z = bytearray(24)
        z[9] = proto
        pk.append(bytes(z)); vw.append([(0, 3, 9), (1, 1, 15)]); tags.append("rx")
        z[3] = 24
        pk.append(bytes(z)); vw.append([(0, 2, 24)]); tags.append("rx")
        pk.append(bytes(rxgen.make_packet(rng, 40, proto=proto, ihl=5))); vw.append([(0, 1, 20), (1, 2, 40)])
        tags.append("rx")
    lay = build(pk, vw, rng)
    want, *_ = pcheck(lay, O.MODE_TX_DATAGRAM, dev, oracle_c)
    tags = np.array(tags)
    assert (want[tags == "zero", 1] == 0xFFFF).all() and (tags == "zero").sum() >= 8
    assert (want[tags == "multiple", 1] == 0x0000).all() and (tags == "multiple").sum() >= 8
    pcheck(lay, O.MODE_TX_DATAGRAM, dev, oracle_c, fill=True, offsets=slack_offsets)
    rx, *_ = pcheck(lay, O.MODE_VERIFY_RX, dev, oracle_c)
    assert (rx[tags == "rx", 0] & 1).all()
    pcheck(lay, O.MODE_IPV4, dev, oracle_c, fill=True)
    pcheck(lay, O.MODE_VERIFY_IPV4, dev, oracle_c)


# ---- 5. length ------------------------------------------------------------------------------
def test_longest_datagram(dev, rng, oracle_c):
    d = rxgen.make_packet(rng, 65535 - 20, proto=17, ihl=5)
    e = rxgen.make_packet(rng, 65535 - 60, proto=6, ihl=15)
    lay = build([d, d, e], [[(1, 2, 65535)], [(0, 1, 20), (1, 3, 30000), (0, 2, 35515)], [(0, 3, 60), (1, 1, 65475)]], rng)
    for mode in (O.MODE_VERIFY_RX, O.MODE_VERIFY_IPV4):
        pcheck(lay, mode, dev, oracle_c)
    for mode in FILL:
        pcheck(lay, mode, dev, oracle_c, fill=True, offsets=slack_offsets)


# ---- 6. shared template -----------------------------------------------------------------------
def test_shared_header_template(dev, rng, oracle_c):
    """64 packets name one 40-byte IP + TCP header view, each with its own payload of
    equal length: under fill every copy gets both of its fields (the transport values
    differ with the payloads) and the template stays as it is."""
    plen = 100
    d = rxgen.tx_packet(rng, 20 + plen, proto=6, ihl=5)
    pay = [(1, (5 * i) % 16, plen) for i in range(64)]
    lay = general_layout([[(0, 6, 40)]] + [[p] for p in pay], rng)
    vp = np.stack((np.full(64, lay.vp[0]), lay.vp[1:]), 1).reshape(-1)
    vo = np.stack((np.full(64, lay.vo[0]), lay.vo[1:]), 1).reshape(-1)
    vl = np.stack((np.full(64, 40), lay.vl[1:]), 1).reshape(-1)
    shared = Layout(lay.pools, vp, vo, vl, 2 * np.arange(65))
    shared.put(np.arange(40), np.frombuffer(bytes(d[:40]), np.uint8))
    for mode in MODES:
        pcheck(shared, mode, dev, oracle_c)
    want, *_ = pcheck(shared, O.MODE_TX_DATAGRAM, dev, oracle_c, fill=True)
    assert len(set(want[:, 0].tolist())) == 1 and len(set(want[:, 1].tolist())) > 32
    pcheck(shared, O.MODE_TX_DATAGRAM, dev, oracle_c, fill=True, offsets=slack_offsets)
    pcheck(shared, O.MODE_IPV4, dev, oracle_c, fill=True)


# ---- 7. counts ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 4, 5, 4097))
def test_counts(n, dev, rng, oracle_c):
    lay = count_layout(n, rng)
    pcheck(lay, O.MODE_VERIFY_RX, dev, oracle_c)
    pcheck(lay, O.MODE_VERIFY_IPV4, dev, oracle_c, offsets=slack_offsets)
    pcheck(lay, O.MODE_TX_DATAGRAM, dev, oracle_c, fill=True, offsets=slack_offsets)
    pcheck(lay, O.MODE_IPV4, dev, oracle_c, fill=True)


def test_second_pass_of_the_grid(dev, rng, oracle_c):
    """70000 packets: the grid holds at most 65536 waves, so some take a second packet."""
    n = 70000
    src = [rxgen.tx_packet(rng, 20 + int(s), proto=(6, 17, 1)[i % 3]) for i, s in enumerate(rng.integers(20, 61, 256))]
    pk = [src[i % 256] for i in range(n)]
    ln = np.array([len(p) for p in pk])
    lay = put_packets(two_view_layout(ln, rng.integers(0, ln + 1), rng.integers(0, 16, n), rng.integers(0, 4, n), rng), pk)
    pcheck(lay, O.MODE_TX_DATAGRAM, dev, oracle_c, fill=True)
    pcheck(lay, O.MODE_VERIFY_RX, dev, oracle_c)


_FEW_WAVES = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np, torch
import rxgen
from oracle import oracle as O
from iov_layout import GUARD
from test_gpu_iov_datagram import build
from test_gpu_iov_pack_datagram import pcheck
from test_gpu_iov_pack import slack_offsets
dev = torch.device("cuda:0")
cus = torch.cuda.get_device_properties(dev).multi_processor_count
n = cus * 4 * 2 + 37      # one block per CU, four waves each: two full passes and a partial third
rng = np.random.default_rng(5)
src = [bytes(rxgen.tx_packet(rng, 64, proto=(6, 17, 1)[i %% 3], ihl=5)) for i in range(64)]
pk = [src[i %% 64] for i in range(n)]
lay = build(pk, [[(0, i %% 16, 20), (1, i %% 4, len(p) - 20)] for i, p in enumerate(pk)], rng)
for mode, fill in ((O.MODE_VERIFY_RX, False), (O.MODE_TX_DATAGRAM, True), (O.MODE_IPV4, True), (O.MODE_VERIFY_IPV4, False)):
    pcheck(lay, mode, dev, O.C(), fill=fill, offsets=slack_offsets)
print("same", True, n)
"""


def test_three_packets_per_wave_on_a_one_block_per_cu_grid():
    """A child process with YU_TUNING=1 YU_BLOCKS_PER_CU=1: every wave takes three
    packets (the last pass partial), so the look-ahead runs past the table's end."""
    env = dict(os.environ, YU_TUNING="1", YU_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", _FEW_WAVES % (ROOT, os.path.join(ROOT, "tests"))],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split()[:2] == ["same", "True"], r.stdout
    assert "YU_BLOCKS_PER_CU=1" in r.stderr  # the knob was read


# ---- 8. out of contract -----------------------------------------------------------------
@pytest.mark.parametrize("fill", (False, True))
def test_out_of_contract_packets_stay_inside_their_span(dev, rng, oracle_c, fill):
    """Room one byte short (packet 3), room 0 (6), dst_offsets decreasing (9), a packet
    over 65535 bytes (12) and first_iov decreasing at the last packet (15); all pointers
    valid. Every other packet is exact in value and bytes, nothing outside the
    offenders' spans is written, and the field bytes of the short-room packet keep the
    bytes of its source."""
    pk = [bytes(rxgen.tx_packet(rng, 60 + i, proto=(6, 17, 1)[i % 3])) for i in range(16)]
    vw = [[(0, i % 16, 20), (1, i % 4, len(p) - 20)] for i, p in enumerate(pk)]
    pk[12] = bytes(rxgen.tx_packet(rng, 65515, proto=17, ihl=5)) + bytes(rng.integers(0, 256, 4465, dtype=np.uint8))
    vw[12] = [(0, 2, 20), (1, 1, 30000), (1, 3, 39980)]  # 70000 bytes of valid memory
    lay = build(pk, vw, rng)
    off = (3, 6, 9, 12, 15)
    mode = O.MODE_TX_DATAGRAM if fill else O.MODE_VERIFY_RX
    k = 2 if fill else 1
    blob = lay.blob()
    lens = lay.lens.astype(np.int64)
    room = lens.copy()
    room[3] -= 1
    room[6] = 0
    room[12] = 65535
    do = np.concatenate(([0], np.cumsum(room)))
    do[9] = do[-1]  # decreases at 9: packet 8 has slack up to the end, packet 9 no span
    first = lay.first.copy()
    first[16] = first[15] - 3  # packet 15: no views
    want = oracle_c.batch(blob, mode, offsets=lay.offsets).reshape(16, k)
    pools, views, (vp, vo, vl, _) = lay.device(dev)
    base = 5
    total = GUARD + base + int(do[-1]) + GUARD
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    dst = buf[GUARD + base:GUARD + base + int(do[-1])]
    dofs = torch.from_numpy(do).to(dev)
    fi = torch.from_numpy(first).to(dev)
    with pytest.raises(ValueError):
        batch.pack_iov_datagrams(views, vp, vo, vl, fi, mode, dst=dst, dst_offsets=dofs)
    got, _, _ = batch.pack_iov_datagrams(views, vp, vo, vl, fi, mode, dst=dst, dst_offsets=dofs, fill=fill,
                                         validate=False)
    torch.cuda.synchronize()  # the call returns
    clean = np.delete(np.arange(16), off)
    assert np.array_equal(got.cpu().numpy().reshape(16, k)[clean], want[clean])
    exp = dg_image(lay, blob, do, total, base, mode, want if fill else None, skip=off)
    after = buf.cpu().numpy()
    mask = np.ones(total, bool)
    for i in off:  # the offending packets' own spans: unspecified bytes
        lo, hi = int(do[i]), int(min(do[i + 1], do[-1]))
        if hi > lo:
            mask[GUARD + base + lo:GUARD + base + hi] = False
    assert np.array_equal(after[mask], exp[mask])
    # the short-room packet: no field value; what fits its room is the source's bytes
    p3, s3 = GUARD + base + int(do[3]), int(lay.offsets[3])
    assert np.array_equal(after[p3:p3 + lens[3] - 1], blob[s3:s3 + lens[3] - 1])
    for x, e in zip(pools, lay.pools):
        assert np.array_equal(x.cpu().numpy(), e)


# ---- 9. equivalence ----------------------------------------------------------------------------
def test_equivalence_with_the_ragged_calls_on_the_copy(dev, rng, oracle_c):
    lay = count_layout(3000, rng)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    for mode in MODES:
        out, dst, do = batch.pack_iov_datagrams(views, vp, vo, vl, first, mode)  # dst and offsets allocated
        assert np.array_equal(do.cpu().numpy(), tight(lay)) and dst.numel() == max(int(lay.offsets[-1]), 1)
        assert torch.equal(batch.checksum_ragged(dst, do, mode), out)
    raw, copy, do = batch.pack_iov(views, vp, vo, vl, first, "raw")
    for mode in FILL:
        out, dst, _ = batch.pack_iov_datagrams(views, vp, vo, vl, first, mode, fill=True)
        ref = copy.clone()
        again = batch.checksum_ragged(ref, do, mode, fill=True)
        assert torch.equal(again, out) and torch.equal(ref, dst)
    # a filled TX_DATAGRAM copy verifies wherever the datagram was valid
    tx, dst, _ = batch.pack_iov_datagrams(views, vp, vo, vl, first, "tx_datagram", fill=True)
    rx = batch.checksum_ragged(dst, do, "verify_rx").cpu().numpy()
    before = batch.checksum_iov_datagrams(views, vp, vo, vl, first, "verify_rx").cpu().numpy()
    hl = np.array([(int(b) & 15) * 4 for b in lay.blob()[lay.offsets[:-1].astype(np.int64)]])
    ok = (before != 8) & (hl >= 20) & (lay.lens > 0)
    assert ok.sum() > 1000 and (rx[ok] & 1).all()  # the IPv4 header of every copy now verifies


# ---- 10. graph capture ------------------------------------------------------------------------
def test_graph_capture(dev, rng, oracle_c):
    lay = count_layout(500, rng)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    out = torch.zeros(1000, dtype=torch.uint16, device=dev)
    do = tight(lay)
    dofs = torch.from_numpy(do).to(dev)
    total = int(do[-1]) + 2 * GUARD
    buf = torch.zeros(total, dtype=torch.uint8, device=dev)
    dst = buf[GUARD:GUARD + int(do[-1])]
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    kw = dict(out=out, dst=dst, dst_offsets=dofs, fill=True)
    with torch.cuda.stream(s):
        batch.pack_iov_datagrams(views, vp, vo, vl, first, "tx_datagram", **kw)  # warm up, validated
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            batch.pack_iov_datagrams(views, vp, vo, vl, first, "tx_datagram", validate=False, **kw)
    torch.cuda.current_stream(dev).wait_stream(s)
    for rep in range(2):
        blob = lay.blob()  # other bytes in the same views: damage 200 of them
        flip = rng.integers(0, blob.size - 1, 200)
        lay.put(flip, blob[flip] ^ 0x10)
        for k, p in enumerate(pools):
            p.copy_(torch.from_numpy(lay.pools[k]))
        out.zero_()
        buf.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        blob = lay.blob()
        want = oracle_c.batch(blob, O.MODE_TX_DATAGRAM, offsets=lay.offsets).reshape(500, 2)
        assert np.array_equal(out.cpu().numpy().reshape(500, 2), want), rep
        assert np.array_equal(buf.cpu().numpy(), dg_image(lay, blob, do, total, 0, O.MODE_TX_DATAGRAM, want)), rep


# ---- 11. known answers --------------------------------------------------------------------------
def test_known_answers(dev):
    """tests/golden/refexec.json (values recorded by executing the reference): whole
    datagrams, each split where the senders split, into a header view (the IPv4
    header, as far as the packet holds it) and a payload view; the copy is the
    datagram, in the fill form with the recorded values in its fields."""
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
        pools = [torch.from_numpy(hdr.reshape(-1)).to(dev), torch.from_numpy(pay).to(dev)]
        k = 2 if mode == O.MODE_TX_DATAGRAM else 1
        for fill in ((False, True) if mode in FILL else (False,)):
            got, dst, _ = batch.pack_iov_datagrams(pools, vp, vo, vl, 2 * torch.arange(n + 1, device=dev), mode,
                                                   fill=fill)
            assert np.array_equal(got.cpu().numpy(), want), mode
            img = data[:offs[-1]].copy()
            if fill:
                w = np.asarray(want).reshape(n, k)
                for i in range(n):
                    for at, val in _fields(mode, data, int(offs[i]), int(offs[i + 1]), [int(x) for x in w[i]]):
                        img[at] = val & 0xFF
            assert np.array_equal(dst.cpu().numpy()[:offs[-1]], img), (mode, fill)


# ---- Python validation -----------------------------------------------------------------
def test_python_validation(dev, rng):
    lay = count_layout(10, rng)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    do = torch.from_numpy(tight(lay)).to(dev)
    dst = torch.zeros(int(lay.offsets[-1]), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="overlaps"):
        batch.pack_iov_datagrams(views, vp, vo, vl, first, "verify_rx", dst=views[0][4:], dst_offsets=do)
    with pytest.raises(ValueError, match="past dst"):
        batch.pack_iov_datagrams(views, vp, vo, vl, first, "verify_rx", dst=dst[:-1], dst_offsets=do)
    short = do.clone()
    short[5:] -= 1
    with pytest.raises(ValueError, match="room|non-decreasing"):
        batch.pack_iov_datagrams(views, vp, vo, vl, first, "verify_rx", dst=dst, dst_offsets=short)
    with pytest.raises(ValueError):
        batch.pack_iov_datagrams(views, vp, vo, vl, first, "tcp")
    with pytest.raises(ValueError):
        batch.pack_iov_datagrams(views, vp, vo, vl, first, "verify_rx", fill=True)
    out, d, o = batch.pack_iov_datagrams(views, vp, vo, vl, first, "tx_datagram")
    assert out.numel() == 20 and d.numel() == int(lay.offsets[-1]) and o.numel() == 11
    assert batch.iov_pack_datagram_variant("tx_datagram", 10, True) == "k_pack<4,dg,fill>"
