"""yu_rx_parse_ragged on the MI355X (k_parse): received IPv4 datagrams parsed where they
lie into yu_rx_split_ragged's record, one yu_iovec onto the payload, and out: VERIFY_RX's
flags plus YU_RX_SPLIT with verify, the two header bits without.

1. the 198 datagrams the reference's own senders produced (tests/golden/refexec.json) and
   the 110 the Linux kernel verified or built (tests/golden/kernel_verified.npz);
2. seeded received batches (tests/rxgen.py), half of them damaged, at data byte phases
   0..3 and n = 1, 63, 64, 65, 257 (the lane, wave and block seams), and one wave that
   mixes short-header, IHL 5, IHL 6 and IHL 15 datagrams;
3. a last packet of 20..79 bytes with nothing behind `data` but the guard;
4. more packets than twice the grid's lanes, compared with yu_rx_split_ragged too;
5. batch.pack_iov over the returned views reproduces yu_rx_split_ragged's pay;
6. the contract batch: out-of-contract packets change no other packet's results;
7. the C call with data at an odd address and 8-byte aligned tables, and one graph
   capture and replay of the two-launch form.

The flags' low four bits come from the C oracle's ragged VERIFY_RX; YU_RX_SPLIT, the
record and the payload range from the reference restatement `decode` of
tests/test_gpu_rx_split.py. Records, views and out sit between 256-byte guards of 0xA5
that are checked after every call. Every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

import parse_plan
import rxgen
from oracle import oracle as O
from test_gpu_rx_split import ALL_OK, FIELD_AT, H_OF, Want, delivery_faults, ragged
from yustack_amd import _lib, batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
HDR_BITS = batch.RX_INVALID | batch.RX_SPLIT


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def oracle_c():
    return O.C()


def pay_at(want):
    """Packet offset of each payload, HL + H (0 where the packet does not split)."""
    return np.array([(p[0] & 15) * 4 + H_OF.get(p[9], 0) if s else 0 for p, s in zip(want.pkts, want.split)],
                    dtype=np.int64)


def guarded(dev, nbytes):
    return torch.full((GUARD + max(nbytes, 1) + 8 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)


class Run:
    """One call on the device. The data at byte phase `dphase` between 0xA5 guards, so
    that nothing but guard bytes lies behind its last byte; records, views and out between
    guards too, the two tables `tshift` (0 or 8) bytes further on. offs: the table the
    device gets."""

    def __init__(self, dev, blob, offs, verify, dphase=0, tshift=0, via_c=False, validate=False, launch=True):
        self.n = n = len(offs) - 1
        self.offs = offs = np.asarray(offs).astype(np.int64)
        size = max(len(blob), 1)
        self.whole = torch.full((GUARD + dphase + size + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.data = self.whole[GUARD + dphase:GUARD + dphase + size]
        self.data[:len(blob)] = torch.from_numpy(blob).to(dev)
        self.ot = torch.from_numpy(offs).to(dev)
        self.verify, self.tshift, self.dev = verify, tshift, dev
        self.recbuf, self.viewbuf, self.outbuf = guarded(dev, 32 * n), guarded(dev, 16 * n), guarded(dev, 2 * n)
        at = GUARD + tshift
        self.recs = self.recbuf[at:at + 32 * n].view(n, 32)
        self.views = self.viewbuf[at:at + 16 * n].view(torch.int64).view(n, 2)
        self.out = self.outbuf[GUARD:GUARD + 2 * n].view(torch.uint16)
        assert self.data.data_ptr() % 4 == dphase and self.recs.data_ptr() % 16 == tshift
        if not launch:
            return
        if via_c:
            rc = _lib.lib().yu_rx_parse_ragged(self.data.data_ptr(), self.ot.data_ptr(), n, 1 if verify else 0,
                                               self.recs.data_ptr(), self.views.data_ptr(), self.out.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream)
            assert rc == _lib.YU_OK
        else:
            got = self.call(validate)
            assert got[0] is self.recs and got[1] is self.views and got[2] is self.out
        torch.cuda.synchronize(dev)  # raises if the stream did not finish cleanly

    def call(self, validate=False):
        return batch.parse_datagrams(self.data, self.ot, verify=self.verify, records=self.recs, views=self.views,
                                     out=self.out, validate=validate)

    def results(self):
        n, at = self.n, GUARD + self.tshift
        out, recs, views = self.outbuf.cpu().numpy(), self.recbuf.cpu().numpy(), self.viewbuf.cpu().numpy()
        for name, buf, lo, size in (("out", out, GUARD, 2 * n), ("records", recs, at, 32 * n),
                                    ("views", views, at, 16 * n)):
            assert (buf[:lo] == 0xA5).all() and (buf[lo + size:] == 0xA5).all(), f"{name}: guard written"
        return (out[GUARD:GUARD + 2 * n].view(np.uint16), recs[at:at + 32 * n].reshape(n, 32),
                views[at:at + 16 * n].view(np.int64).reshape(n, 2))

    def check(self, want, skip_all=(), loose_flags=()):
        """Everything equals `want` but for the packets in skip_all (every result
        unspecified) and, with verify, the VERIFY_RX bits of those in loose_flags (the
        group mates of an out-of-contract packet); every guard byte is still 0xA5."""
        n = self.n
        keep = np.ones(n, dtype=bool)
        keep[list(skip_all)] = False
        got_out, got_rec, got_view = self.results()
        want_out = want.out if self.verify else want.out & HDR_BITS
        mask = np.full(n, 0xFFFF, dtype=np.uint16)
        if self.verify:
            mask[list(loose_flags)] = batch.RX_SPLIT
        bad = np.nonzero(((got_out ^ want_out) & mask != 0) & keep)[0]
        assert bad.size == 0, f"out differs at {bad[:8]}: {got_out[bad[:8]]} want {want_out[bad[:8]]}"
        bad = np.nonzero((got_rec != want.recs).any(1) & keep)[0]
        assert bad.size == 0, f"records differ at {bad[:8]}"
        base = np.where(want.split, self.data.data_ptr() + self.offs[:-1] + pay_at(want), 0)
        length = np.where(want.split, want.L, 0)
        bad = np.nonzero(((got_view[:, 0] != base) | (got_view[:, 1] != length)) & keep)[0]
        assert bad.size == 0, f"views differ at {bad[:8]}: {got_view[bad[:8]]}"
        assert (self.whole[:GUARD].cpu().numpy() == 0xA5).all() and (self.whole[-GUARD:].cpu().numpy() == 0xA5).all()
        return got_out


def both(dev, blob, offs, want, **kw):
    """The batch with verify and without; out(verify=0) == out(verify=1) & (INVALID | SPLIT)."""
    o1 = Run(dev, blob, offs, True, **kw).check(want)
    o0 = Run(dev, blob, offs, False, **kw).check(want)
    assert (o0 == o1 & HDR_BITS).all()


# ---- 1. the fixture datagrams ---------------------------------------------------------------
def test_executed_reference_datagrams(dev, oracle_c):
    vecs = [v for v in json.load(open(os.path.join(ROOT, "tests", "golden", "refexec.json")))["modes"]["9"]
            if v.get("src") == "exec"]
    assert len(vecs) == 198
    pkts = []
    for v in vecs:
        b = bytearray.fromhex(v["hex"])
        sums = [int(x) for x in v["want"]]
        b[10:12] = sums[0].to_bytes(2, "big")  # the two fields as the senders stored them
        f = FIELD_AT.get(b[9])
        if f is not None:
            b[20 + f:22 + f] = sums[1].to_bytes(2, "big")
        pkts.append(bytes(b))
    blob, offs = ragged(pkts)
    want = Want(blob, offs, oracle_c)
    assert (want.out == ALL_OK).all()
    both(dev, blob, offs, want, validate=True)


def test_kernel_verified_datagrams(dev, oracle_c):
    f = np.load(os.path.join(ROOT, "tests", "golden", "kernel_verified.npz"))
    pkts = [bytes(b[int(s):int(e)]) for b, o in ((f["sent_blob"], f["sent_offs"]), (f["kernel_blob"], f["kernel_offs"]))
            for s, e in zip(o[:-1], o[1:])]
    assert len(pkts) == 110
    blob, offs = ragged(pkts)
    want = Want(blob, offs, oracle_c)
    assert (want.out == ALL_OK).all()
    both(dev, blob, offs, want, dphase=1, validate=True)


# ---- 2. seeded batches ----------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_received_batches_at_the_seams(dev, oracle_c, n):
    """rxgen.rx_batch(rng, n, 0, 200, bad=0.5): payloads short enough that many packets
    end inside the 80-byte window, IHL 5..15, half of them damaged."""
    rng = np.random.default_rng(16000 + n)
    blob, offs = rxgen.rx_batch(rng, n, 0, 200, bad=0.5)
    want = Want(blob, offs, oracle_c)
    if n >= 63:
        assert want.split.any() and not want.split.all()
    for dphase in range(4):
        both(dev, blob, offs, want, dphase=dphase)


def test_lanes_diverge_on_the_option_path(dev, oracle_c):
    """One wave (and a second, partial one) whose lanes hold short-header datagrams, IHL
    5, 6 and 15, and datagrams that pass IsValid and fail a delivery test: the second
    load is taken by some lanes of the step only."""
    rng = np.random.default_rng(16002)
    pkts = []
    for i in range(80):
        kind = i % 5
        if kind == 0:
            pkts.append(bytes(rxgen.short_header_packet(rng, int(rng.integers(20, 81)))))
        else:
            pkts.append(bytes(rxgen.make_packet(rng, int(rng.integers(0, 90)), ihl=(5, 6, 15, 5)[kind - 1])))
    pkts += delivery_faults(rng)
    order = rng.permutation(len(pkts))
    blob, offs = ragged([pkts[i] for i in order])
    want = Want(blob, offs, oracle_c)
    ihl = np.array([p[0] & 15 for p in want.pkts])
    assert all((ihl[:64] == v).sum() >= 5 for v in (5, 6, 15)) and (ihl[:64] < 5).sum() >= 5
    assert want.split.sum() >= 40 and (~want.split).sum() >= 20
    for dphase in (0, 3):
        both(dev, blob, offs, want, dphase=dphase)


# ---- 3. the last packet ---------------------------------------------------------------------
def test_short_last_packet_at_the_batch_end(dev, oracle_c):
    """The last packet is 20..79 bytes long, shorter than the 80-byte window, and behind
    it lies only the 0xA5 guard: a window load past the packet would read guard bytes
    into the record. Its length also moves the data's end through every byte phase."""
    rng = np.random.default_rng(16003)
    for last in range(20, 80):
        pkts = [bytes(rxgen.make_packet(rng, int(rng.integers(0, 40)))) for _ in range(2)]
        p = bytearray(rxgen.make_packet(rng, 60, proto=(6, 17, 1, 47)[last % 4], ihl=(5, 6, 15)[last % 3]))[:last]
        p[2:4] = last.to_bytes(2, "big")  # TL = len: valid, and splits where the transport header fits
        pkts.append(bytes(p))
        blob, offs = ragged(pkts)
        want = Want(blob, offs, oracle_c)
        Run(dev, blob, offs, bool(last % 2), dphase=last % 4).check(want)


# ---- 4. grid stride -------------------------------------------------------------------------
def test_more_packets_than_twice_the_lanes(dev, oracle_c):
    """2 x blocks x 256 + 5 datagrams of 20..60 bytes, where blocks is yu::plan_parse's cap
    for this device: every lane takes more than one packet. The batch is 4099 seeded
    datagrams repeated (4099 is odd, so a repeat lands on other lanes and byte phases);
    a packet's results depend on its own bytes only, so the expected values repeat too,
    the view bases aside. yu_rx_split_ragged on the same batch gives the same out and
    records, and its pay_len is the views' length column."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    (_, blocks, name), = parse_plan.plans([(1 << 26, cus)])
    assert name == "k_parse" and blocks == 8 * cus
    n = 2 * blocks * 256 + 5
    rng = np.random.default_rng(16004)
    base = []
    for _ in range(4099):
        proto = int(rng.choice([6, 17, 1, 47]))
        base.append(bytes(rxgen.make_packet(rng, int(rng.integers(H_OF.get(proto, 0), 41)), proto=proto, ihl=5)))
    bblob, boffs = ragged(base)
    bwant = Want(bblob, boffs, oracle_c)
    assert bwant.split.all() and 20 <= min(map(len, base)) and max(map(len, base)) <= 60
    reps = -(-n // 4099)
    lens = np.tile(np.diff(boffs.astype(np.int64)), reps)[:n]
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    blob = np.tile(bblob, reps)[:offs[-1]]
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:n]  # noqa: E731
    want_out, want_rec, want_L, want_at = tile(bwant.out), tile(bwant.recs), tile(bwant.L), tile(pay_at(bwant))
    for verify in (True, False):
        r = Run(dev, blob, offs, verify, dphase=3)
        got_out, got_rec, got_view = r.results()
        assert np.array_equal(got_out, want_out if verify else want_out & HDR_BITS)
        assert np.array_equal(got_rec, want_rec)
        assert np.array_equal(got_view[:, 0], r.data.data_ptr() + offs[:-1] + want_at)
        assert np.array_equal(got_view[:, 1], want_L)
    _, _, pay_len, recs, out = batch.split_datagrams(r.data, r.ot)
    torch.cuda.synchronize(dev)
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(recs.cpu().numpy(), want_rec)
    assert np.array_equal(pay_len.cpu().numpy(), got_view[:, 1])


# ---- 5. composition -------------------------------------------------------------------------
def test_pack_iov_over_the_views_is_rx_split(dev, oracle_c):
    """parse, then gather: batch.pack_iov([data], ...) in raw mode over the returned views
    with tight offsets gives yu_rx_split_ragged's pay byte for byte, and so does
    yu_csum_pack_iov on the view table as the call stored it."""
    rng = np.random.default_rng(16005)
    blob, offs = rxgen.rx_batch(rng, 300, 0, 300, bad=0.4)
    want = Want(blob, offs, oracle_c)
    n = want.n
    r = Run(dev, blob, offs, False, dphase=1)
    r.check(want)
    po = np.zeros(n + 1, dtype=np.int64)
    po[1:] = np.cumsum(np.where(want.split, want.L, 0))
    pot = torch.from_numpy(po).to(dev)
    total = int(po[-1])
    pay = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=dev)
    batch.split_datagrams(r.data, r.ot, pay=pay, pay_offsets=pot)
    view_len = r.views[:, 1].contiguous()
    view_off = torch.where(view_len > 0, r.views[:, 0] - r.data.data_ptr(), 0)
    first = torch.arange(n + 1, dtype=torch.int64, device=dev)
    dst = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=dev)
    _, dst, do = batch.pack_iov([r.data], torch.zeros(n, dtype=torch.int64, device=dev), view_off, view_len, first,
                                "raw", dst=dst, validate=True)
    torch.cuda.synchronize(dev)
    assert do.cpu().numpy().tolist() == po.tolist()
    assert total > 10000 and np.array_equal(dst.cpu().numpy(), pay.cpu().numpy())
    dst2 = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=dev)
    sums = torch.zeros(n, dtype=torch.uint16, device=dev)
    rc = _lib.lib().yu_csum_pack_iov(r.views.data_ptr(), first.data_ptr(), n, batch.RAW, None, 0, None,
                                     dst2.data_ptr(), pot.data_ptr(), sums.data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream)
    assert rc == _lib.YU_OK
    torch.cuda.synchronize(dev)
    assert np.array_equal(dst2.cpu().numpy(), pay.cpu().numpy())


# ---- 6. the contract ------------------------------------------------------------------------
def test_out_of_contract_packets_change_no_other_packet(dev, oracle_c):
    """196 good packets and four out of contract: a 65536-byte packet (20), offsets
    decreasing (45; and again at the last packet, 199) and a packet ending past offsets[n]
    (198). tests/cpp/rx_parse.cpp runs the same cases on a CPU; none faults. Record, view
    and YU_RX_SPLIT of every other packet are exact; VERIFY_RX's four bits are compared
    outside the 64-packet groups [0, 64) and [192, 200) that hold the four (the group rule
    of yu_csum_batch_ragged; without verify the header bits of every other packet are
    exact). The guards are intact."""
    rng = np.random.default_rng(16006)
    n = 200
    bad = {"over": 20, "dec": 45, "past": 198, "tail": 199}
    pkts = [bytes(rxgen.make_packet(rng, int(rng.integers(0, 131)))) for _ in range(n)]
    pkts[bad["over"]] = bytes(rxgen.make_packet(rng, 65536 - 20, proto=17, ihl=5))
    assert len(pkts[bad["over"]]) == 65536
    blob, o = ragged(pkts)
    want = Want(blob, o, oracle_c)  # what each packet's own bytes give
    o = o.astype(np.int64)
    unspecified = tuple(bad.values())
    assert want.split[[i for i in range(n) if i not in unspecified]].all()
    # the device's table. Packet 45's start moves 7 bytes past its end: offsets decreases at it, and packet 44
    # ends there, with packet 45's bytes and 7 more as trailing bytes past its TotalLength (the same results).
    # offsets[n] moves 5 bytes before packet 198's end: that packet ends past it, and packet 199 decreases.
    t = o.copy()
    t[bad["dec"]] = o[bad["dec"] + 1] + 7
    t[n] = o[n - 1] - 5
    with pytest.raises(ValueError):
        Run(dev, blob, t, True, launch=False).call(validate=True)
    group_mates = [i for i in range(n) if i < 64 or i >= 192]
    for verify in (True, False):
        r = Run(dev, blob, t, verify, dphase=2)  # YU_OK, and the stream synchronises cleanly
        r.offs = o  # the expected views: each packet's own start (packet 45's is not compared)
        r.check(want, skip_all=unspecified, loose_flags=group_mates)


# ---- 7. the C call and a graph --------------------------------------------------------------
def test_c_call_at_odd_addresses(dev, oracle_c):
    """data at an odd address; records and views 8 bytes off a 16-byte boundary, which the
    contract allows and the 16-byte stores must take."""
    rng = np.random.default_rng(16007)
    blob, offs = rxgen.rx_batch(rng, 130, 0, 300, bad=0.3)
    want = Want(blob, offs, oracle_c)
    for dphase, tshift, verify in ((1, 8, True), (3, 0, True), (3, 8, False)):
        Run(dev, blob, offs, verify, dphase=dphase, tshift=tshift, via_c=True).check(want)


def test_graph_capture_of_the_two_launches(dev, oracle_c):
    rng = np.random.default_rng(16008)
    blob, offs = rxgen.rx_batch(rng, 500, 0, 400, bad=0.5)
    want = Want(blob, offs, oracle_c)
    r = Run(dev, blob, offs, True, dphase=1, launch=False)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        r.call(validate=True)  # warm up, validated
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            r.call()
    torch.cuda.current_stream(dev).wait_stream(s)
    r.check(want)
    for buf in (r.recbuf, r.viewbuf, r.outbuf):
        buf.fill_(0xA5)
    g.replay()
    torch.cuda.synchronize(dev)
    r.check(want)
