"""Scatter-gather device packets summed and packed in one pass (yu_csum_pack_iov /
yu_csum_pack_fill_iov through batch.pack_iov) on the GPU. Per call: every value
against the C oracle's ragged batch over the same bytes laid back to back; ALL of
dst, with 128-byte guards on both sides and every slack byte (prefilled 0xA5),
against the expected image; every pool, unchanged byte for byte; out's guard.

No result is filtered. The only input selection is the modes' own input condition
(tests/test_gpu_iov.py: UDP 8, TCP 20, ICMP 4 bytes, TCP's byte 12 = 0x50)."""
import numpy as np
import pytest
import torch

from iov_layout import FIELD, GUARD, Layout, general_layout, two_view_layout
from oracle import oracle as O
from test_gpu_iov import MIN_LEN, MODES, SIDE_OF, TX, count_layout, field_packets, side_args, split_cases
from yustack_amd import batch

pytestmark = pytest.mark.gpu


def tight(lay):
    return lay.offsets.astype(np.int64)


def slack_offsets(lay):
    """dst_offsets with packet i starting at i mod 16 and 1..19 bytes of slack."""
    lens = lay.lens.astype(np.int64)
    slack = 1 + (-lens) % 16                      # len + slack = 1 mod 16
    slack[(slack <= 3) & (np.arange(lay.n) % 32 < 16)] += 16  # 17..19 for some (a multiple of 16 more)
    return np.concatenate(([0], np.cumsum(lens + slack)))


def image(lay, blob, do, total, base, values=None, mode=None, skip=()):
    """The buffer the call leaves: 0xA5 everywhere, packet i's bytes at do[i]; with
    `values` the field of every packet that holds it. `skip`: packets left out."""
    exp = np.full(total, 0xA5, np.uint8)
    lens = lay.lens.astype(np.int64)
    src0 = lay.offsets[:-1].astype(np.int64)
    keep = np.ones(lay.n, bool)
    keep[np.asarray(list(skip), dtype=np.int64)] = False
    ln = np.where(keep, lens, 0)
    rel = np.arange(ln.sum()) - np.repeat(np.cumsum(ln) - ln, ln)
    exp[GUARD + base + np.repeat(do[:-1], ln) + rel] = blob[np.repeat(src0, ln) + rel]
    if values is not None:
        f = FIELD[mode]
        pk = np.flatnonzero((lens >= f + 2) & keep)
        exp[GUARD + base + do[pk] + f] = values[pk] >> 8
        exp[GUARD + base + do[pk] + f + 1] = values[pk] & 0xFF
    return exp


_base = [0]


def pcheck(lay, mode, kind, dev, rng, oracle_c, fill=False, with_out=True, offsets=tight, min_len=None):
    """One packing call on the packets of `lay` the oracle defines for `mode`; the dst
    base offset cycles 0..15 from call to call. Returns (lay, dst, dst_offsets, want)."""
    lay = lay.at_least(MIN_LEN.get(mode, 0) if min_len is None else min_len)
    blob = lay.blob()
    okw, gkw = side_args(mode, kind, lay.n, rng, dev)
    want = oracle_c.batch(blob, mode, offsets=lay.offsets, threads=8, **okw)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    base = _base[0] = (_base[0] + 1) % 16
    do = offsets(lay)
    total = GUARD + base + int(do[-1]) + GUARD
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    dst = buf[GUARD + base:GUARD + base + int(do[-1])]
    dofs = torch.from_numpy(do).to(dev)
    out = torch.full((lay.n + 64,), 0xA5A5, dtype=torch.uint16, device=dev)
    got, d2, o2 = batch.pack_iov(views, vp, vo, vl, first, mode, fill=fill, dst=dst, dst_offsets=dofs,
                                 out=out[:lay.n] if with_out else None, **gkw)
    assert d2 is dst and o2 is dofs and got.numel() == lay.n
    res = got.cpu().numpy()
    bad = np.flatnonzero(res != want)
    assert bad.size == 0, (mode, kind, fill, bad[:8], lay.lens[bad[:8]], res[bad[:8]], want[bad[:8]])
    assert (out[lay.n:].cpu().numpy() == 0xA5A5).all()
    exp = image(lay, blob, do, total, base, want if fill else None, mode)
    diff = np.flatnonzero(buf.cpu().numpy() != exp)
    assert diff.size == 0, (mode, kind, fill, base, diff[:8] - GUARD - base)
    for k, (a, e) in enumerate(zip(pools, lay.pools)):
        assert np.array_equal(a.cpu().numpy(), e), (mode, kind, fill, k)  # the sources are never written
    return lay, dst, dofs, want


@pytest.fixture(scope="module")
def rng():
    return np.random.default_rng(20261020)


@pytest.fixture(scope="module")
def split_layout(rng):
    return two_view_layout(*split_cases(), rng)


# ---- 1. splits x shifts ------------------------------------------------------------
@pytest.mark.parametrize("offsets", (tight, slack_offsets))
@pytest.mark.parametrize("mode", MODES)
def test_splits(split_layout, mode, offsets, dev, rng, oracle_c):
    for kind in SIDE_OF[mode]:
        pcheck(split_layout, mode, kind, dev, rng, oracle_c, offsets=offsets)


@pytest.mark.parametrize("offsets", (tight, slack_offsets))
@pytest.mark.parametrize("mode", TX)
def test_splits_fill(split_layout, mode, offsets, dev, rng, oracle_c):
    pcheck(split_layout, mode, "addrs", dev, rng, oracle_c, fill=True, offsets=offsets)
    pcheck(split_layout, mode, "initial", dev, rng, oracle_c, fill=True, with_out=False, offsets=offsets)


def test_slack_offsets_take_every_start():
    lay = count_layout(64, np.random.default_rng(1))
    do = slack_offsets(lay)
    slack = np.diff(do) - lay.lens
    assert set(do[:-1] % 16) == set(range(16)) and slack.min() >= 1 and slack.max() <= 19


# ---- 2. the field across views, at even and odd destination addresses ---------------
@pytest.mark.parametrize("fill", (False, True))
def test_field_across_views(dev, rng, oracle_c, fill):
    lay = general_layout(field_packets(), rng)
    for mode in (TX if fill else MODES):
        for kind in ("addrs", "initial"):  # two calls: the base offset moves on, both parities
            pcheck(lay, mode, kind, dev, rng, oracle_c, fill=fill)
            pcheck(lay, mode, kind, dev, rng, oracle_c, fill=fill, offsets=slack_offsets)


# ---- 3. long and many views ----------------------------------------------------------
@pytest.mark.parametrize("fill", (False, True))
def test_long_and_many_views(dev, rng, oracle_c, fill):
    pk = [[(0, 5, 65535)], [(1, 3, 1), (0, 7, 65533), (1, 2, 1)], [(1, 1, 30000), (0, 2, 5535), (1, 3, 30000)]]
    pk.append([(i % 2, (3 * i) % 16, 1 + i % 3) for i in range(70)])  # past the 64 lane-held records
    for sh in range(4):
        for ln in (1023, 1024, 1025):
            pk.append([(0, sh, 20), (1, (sh + ln) % 16, ln), (0, 3 - sh, ln)])
    lay = general_layout(pk, rng)
    for mode in (TX if fill else MODES):
        for off in (tight, slack_offsets):
            pcheck(lay, mode, "addrs", dev, rng, oracle_c, fill=fill, offsets=off)


# ---- 4. shared views -----------------------------------------------------------------
def test_shared_header_template(dev, rng, oracle_c):
    """One 20-byte header named by 64 packets with their own payloads: every copy gets
    its own field and the template stays as it is (yu_csum_fill_iov cannot)."""
    pay = [(1, (5 * i) % 16, 30 + 23 * i) for i in range(64)]
    lay = general_layout([[(0, 6, 20)]] + [[p] for p in pay], rng)
    vp = np.stack((np.full(64, lay.vp[0]), lay.vp[1:]), 1).reshape(-1)
    vo = np.stack((np.full(64, lay.vo[0]), lay.vo[1:]), 1).reshape(-1)
    vl = np.stack((np.full(64, lay.vl[0]), lay.vl[1:]), 1).reshape(-1)
    shared = Layout(lay.pools, vp, vo, vl, 2 * np.arange(65))
    for mode in TX:
        _, dst, _, want = pcheck(shared, mode, "addrs", dev, rng, oracle_c, fill=True)
        assert len(set(want.tolist())) > 32  # the copies' fields differ


# ---- 5. counts -------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 4, 5, 4097))
def test_counts(n, dev, rng, oracle_c):
    lay = count_layout(n, rng)
    pcheck(lay, O.MODE_RAW, "initial_arr", dev, rng, oracle_c)
    pcheck(lay, O.MODE_TCP, "addrs", dev, rng, oracle_c, fill=True, offsets=slack_offsets)


def test_second_pass_of_the_grid(dev, rng, oracle_c):
    """70000 packets: the grid holds at most 65536 waves, so some take a second packet."""
    n = 70000
    ln = rng.integers(40, 81, n)
    lay = two_view_layout(ln, rng.integers(0, ln + 1), rng.integers(0, 16, n), rng.integers(0, 4, n), rng)
    pcheck(lay, O.MODE_UDP, "addrs", dev, rng, oracle_c, fill=True)


# ---- 6. round trip -------------------------------------------------------------------
def test_round_trip(dev, rng, oracle_c):
    lay = count_layout(3000, rng)
    for mode, vmode in ((O.MODE_TCP, O.MODE_VERIFY_TCP), (O.MODE_UDP, O.MODE_VERIFY_UDP)):
        addrs = rng.integers(0, 256, 8 * lay.n, dtype=np.uint8)
        a = torch.from_numpy(addrs).to(dev)
        pools, views, (vp, vo, vl, first) = lay.device(dev)
        out, dst, do = batch.pack_iov(views, vp, vo, vl, first, mode, addrs=a)  # dst and offsets allocated
        assert np.array_equal(do.cpu().numpy(), tight(lay)) and dst.numel() == int(lay.offsets[-1])
        again = batch.checksum_ragged(dst, do, mode, addrs=a)
        assert torch.equal(again, out)
        out2, dst2, _ = batch.pack_iov(views, vp, vo, vl, first, mode, addrs=a, fill=True)
        assert torch.equal(out2, out)
        v = batch.checksum_ragged(dst2, do, vmode, addrs=a)
        assert bool(batch.verified(v).all())
        assert np.array_equal(out.cpu().numpy(), oracle_c.batch(lay.blob(), mode, offsets=lay.offsets, addrs=addrs))


# ---- 7. out of contract ----------------------------------------------------------------
@pytest.mark.parametrize("fill", (False, True))
def test_out_of_contract_packets_stay_inside_their_span(dev, rng, oracle_c, fill):
    """Room one byte short (packet 3), room 0 (6), dst_offsets decreasing (9) and a
    packet over 65535 bytes (12); all pointers valid. Every other packet is exact in
    value and bytes, nothing outside the four spans is written, and the field of the
    short-room packet keeps the bytes of its source."""
    pk = [[(0, i % 16, 20), (1, i % 4, 40 + i)] for i in range(16)]
    pk[12] = [(0, 2, 20), (1, 1, 30000), (1, 3, 39980)]  # 70000 bytes of valid memory
    lay = general_layout(pk, rng)
    off = (3, 6, 9, 12)
    mode = O.MODE_TCP
    blob = lay.blob()
    lens = lay.lens.astype(np.int64)
    room = lens.copy()
    room[3] -= 1
    room[6] = 0
    room[12] = 65535
    do = np.concatenate(([0], np.cumsum(room)))
    do[9] = do[-1]  # decreases at 9: packet 8 has slack up to the end, packet 9 no span
    clean = np.delete(np.arange(16), off)
    sub = lay.select(clean)
    addrs = rng.integers(0, 256, 8 * 16, dtype=np.uint8)
    want = oracle_c.batch(sub.blob(), mode, offsets=sub.offsets, addrs=addrs.reshape(16, 8)[clean].reshape(-1))
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    base = 5
    total = GUARD + base + int(do[-1]) + GUARD
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    dst = buf[GUARD + base:GUARD + base + int(do[-1])]
    dofs = torch.from_numpy(do).to(dev)
    a = torch.from_numpy(addrs).to(dev)
    with pytest.raises(ValueError):
        batch.pack_iov(views, vp, vo, vl, first, mode, addrs=a, dst=dst, dst_offsets=dofs)
    got, _, _ = batch.pack_iov(views, vp, vo, vl, first, mode, addrs=a, dst=dst, dst_offsets=dofs, fill=fill,
                               validate=False)
    torch.cuda.synchronize()  # the call returns
    res = got.cpu().numpy()
    assert np.array_equal(res[clean], want)
    full = np.zeros(16, np.uint16)
    full[clean] = want
    exp = image(lay, blob, do, total, base, full if fill else None, mode, skip=off)
    after = buf.cpu().numpy()
    mask = np.ones(total, bool)
    for i in off:  # the offending packets' own spans: unspecified bytes
        lo, hi = int(do[i]), int(min(do[i + 1], do[-1]))
        if hi > lo:
            mask[GUARD + base + lo:GUARD + base + hi] = False
    assert not mask[GUARD + base + do[3]:GUARD + base + do[4]].any() and mask.sum() == total - (lens[3] - 1) - 65535
    assert np.array_equal(after[mask], exp[mask])
    p3 = GUARD + base + int(do[3])
    assert np.array_equal(after[p3 + 16:p3 + 18], blob[int(lay.offsets[3]) + 16:int(lay.offsets[3]) + 18])
    for x, e in zip(pools, lay.pools):
        assert np.array_equal(x.cpu().numpy(), e)


# ---- 8. seeded fuzz ------------------------------------------------------------------
def test_fuzz(dev, oracle_c):
    rng = np.random.default_rng(78)
    for it in range(12):
        n = int(rng.integers(100, 250))
        npools = int(rng.integers(1, 4))
        pk = []
        for _ in range(n):
            nv = int(rng.integers(0, 7))
            lens = rng.integers(0, 2001, nv) * (rng.random(nv) < 0.8)
            if rng.random() < 0.5:
                lens = lens % 80
            pk.append([(int(rng.integers(0, npools)), int(rng.integers(0, 16)), int(x)) for x in lens])
        lay = general_layout(pk, rng, npools=npools)
        mode = MODES[it % len(MODES)]
        fill = mode in TX and it >= 6

        def offsets(lay):
            return np.concatenate(([0], np.cumsum(lay.lens.astype(np.int64) + rng.integers(0, 20, lay.n) * (it % 2))))
        kind = ("addrs", "initial_arr", "initial")[int(rng.integers(0, 3))]
        pcheck(lay, mode, kind, dev, rng, oracle_c, fill=fill, with_out=bool(rng.random() < 0.8) or not fill,
               offsets=offsets)


# ---- 9. graph capture ------------------------------------------------------------------
def test_graph_capture(dev, rng, oracle_c):
    lay = count_layout(500, rng)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    addrs = torch.from_numpy(rng.integers(0, 256, 8 * 500, dtype=np.uint8)).to(dev)
    out = torch.zeros(500, dtype=torch.uint16, device=dev)
    do = tight(lay)
    dofs = torch.from_numpy(do).to(dev)
    total = int(do[-1]) + 2 * GUARD
    buf = torch.zeros(total, dtype=torch.uint8, device=dev)
    dst = buf[GUARD:GUARD + int(do[-1])]
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    kw = dict(addrs=addrs, out=out, dst=dst, dst_offsets=dofs, fill=True)
    with torch.cuda.stream(s):
        batch.pack_iov(views, vp, vo, vl, first, "tcp", **kw)  # warm up, validated
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            batch.pack_iov(views, vp, vo, vl, first, "tcp", validate=False, **kw)
    torch.cuda.current_stream(dev).wait_stream(s)
    for rep in range(2):
        for k, p in enumerate(pools):
            lay.pools[k] = rng.integers(0, 256, p.numel(), dtype=np.uint8)
        lay.put(lay.offsets[:-1].astype(np.int64) + 12, 0x50)
        for k, p in enumerate(pools):
            p.copy_(torch.from_numpy(lay.pools[k]))
        out.zero_()
        buf.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        blob = lay.blob()
        want = oracle_c.batch(blob, O.MODE_TCP, offsets=lay.offsets, addrs=addrs.cpu().numpy())
        assert np.array_equal(out.cpu().numpy(), want), rep
        assert np.array_equal(buf.cpu().numpy(), image(lay, blob, do, total, 0, want, O.MODE_TCP)), rep


# ---- Python validation -----------------------------------------------------------------
def test_python_validation(dev, rng):
    lay = count_layout(10, rng)
    pools, views, (vp, vo, vl, first) = lay.device(dev)
    do = torch.from_numpy(tight(lay)).to(dev)
    dst = torch.zeros(int(lay.offsets[-1]), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="overlaps"):
        batch.pack_iov(views, vp, vo, vl, first, "raw", dst=views[0][4:], dst_offsets=do)
    with pytest.raises(ValueError, match="past dst"):
        batch.pack_iov(views, vp, vo, vl, first, "raw", dst=dst[:-1], dst_offsets=do)
    short = do.clone()
    short[5:] -= 1
    with pytest.raises(ValueError, match="room"):
        batch.pack_iov(views, vp, vo, vl, first, "raw", dst=dst, dst_offsets=short)
    dec = do.clone()
    dec[4] = dec[-1]
    with pytest.raises(ValueError, match="non-decreasing"):
        batch.pack_iov(views, vp, vo, vl, first, "raw", dst=torch.zeros(4096, dtype=torch.uint8, device=dev),
                       dst_offsets=dec)
    with pytest.raises(ValueError):
        batch.pack_iov(views, vp, vo, vl, first, "verify_rx")
    with pytest.raises(ValueError):
        batch.pack_iov(views, vp, vo, vl, first, "raw", fill=True)
    out, d, o = batch.pack_iov(views, vp, vo, vl, first, "raw")
    assert out.numel() == 10 and d.numel() == int(lay.offsets[-1]) and o.numel() == 11
    assert batch.iov_pack_variant("tcp", 10, True) == "k_pack<4,fill>"
