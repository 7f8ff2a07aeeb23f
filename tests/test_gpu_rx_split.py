"""yu_rx_split_ragged on the MI355X (k_split<4>): received IPv4 datagrams taken apart on
the device into VERIFY_RX's flags plus YU_RX_SPLIT, one 32-byte record, the payload's
length and the payload.

1. the 198 datagrams the reference's own senders produced when executed end to end
   (tests/golden/refexec.json), split in one launch and rebuilt by yu_tx_build_ragged
   byte for byte;
2. the 110 datagrams the Linux kernel verified or built (tests/golden/kernel_verified.npz);
3. seeded received batches (tests/rxgen.py), half of them damaged, at every data and pay
   byte phase, and short-header datagrams;
4. 70000 datagrams: more packets than waves, tight pay_offsets and the offsets tensor
   itself;
5. n = 1, 4, 5 and one 65535-byte datagram;
6. the contract batch: out-of-contract packets stay inside their own spans;
7. the C call with data and pay at odd addresses.

The flags' low four bits come from the C oracle's ragged VERIFY_RX; YU_RX_SPLIT, the
record, pay_len and the payload from a restatement of ipv4.HandlePacket,
Nic.DeliverTransportPacket, segment.parse and udp.endpoint.HandlePacket written here
(`decode`). Every output buffer sits between 256-byte guards of 0xA5 that are checked
after every call. Every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

import rxgen
from oracle import oracle as O
from yustack_amd import _lib, batch, packets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
H_OF = {6: 20, 17: 8, 1: 4}
FIELD_AT = {6: 16, 17: 6, 1: 2}
ALL_OK = batch.RX_IP_OK | batch.RX_L4 | batch.RX_L4_OK | batch.RX_SPLIT
# the seeds of the received batches of test 3 (payloads 0..1480 and 0..96): chosen on a CPU
# so that `census` finds every outcome often enough in each batch
SEEDS = {1480: 14005, 96: 14002}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def oracle_c():
    return O.C()


def decode(b: bytes):
    """What the reference does with the received datagram b once its checksums are
    known: (why, record, payload). why is None when the packet is delivered
    (YU_RX_SPLIT), else the first test it fails; record is one packets.TX_RECORD."""
    rec = np.zeros(1, dtype=packets.TX_RECORD)[0]
    n = len(b)
    if n < 20:                                   # IsValid, header/ipv4.go:126-138
        return "invalid", rec, b""
    hl, tl = (b[0] & 15) * 4, (b[2] << 8) | b[3]
    if hl > tl or tl > n:
        return "invalid", rec, b""
    if hl < 20:                                  # the address bytes are not header bytes
        return "short header", rec, b""
    seg = b[hl:tl]                               # ipv4.HandlePacket trims the header (and what follows TL)
    proto = b[9]
    H = H_OF.get(proto, 0)
    if len(seg) < H:                             # stack/nic.go:133
        return "slen < H", rec, b""
    num = lambda at, size=2: int.from_bytes(seg[at:at + size], "big")  # noqa: E731
    tcp = {}
    if proto == 6:                               # segment.parse, transport/tcp/segment.go:81-109
        doff = (seg[12] >> 4) * 4
        if doff < 20 or doff > len(seg):
            return "data offset", rec, b""
        tcp = dict(sport=num(0), dport=num(2), seq=num(4, 4), ack=num(8, 4), flags=seg[13], window=num(14), doff=doff)
    elif proto == 17:                            # udp.endpoint.HandlePacket, transport/udp/endpoint.go:191-199
        if num(4) > len(seg):
            return "udp length", rec, b""
        tcp = dict(sport=num(0), dport=num(2))
    elif proto == 1:
        tcp = dict(sport=num(0))
    rec["src"], rec["dst"] = list(b[12:16]), list(b[16:20])
    rec["proto"], rec["ttl"], rec["tos"] = proto, b[8], b[1]
    rec["ip_id"], rec["frag"] = (b[4] << 8) | b[5], (b[6] << 8) | b[7]
    for k, v in tcp.items():
        rec[k] = v
    return None, rec, bytes(seg[H:])


class Want:
    """The expected results of a batch, computed once: the oracle's flags, `decode`."""

    def __init__(self, blob, offs, oracle_c):
        offs = np.asarray(offs, dtype=np.uint64)
        self.n = n = len(offs) - 1
        raw = blob.tobytes()
        o = offs.astype(np.int64)
        self.pkts = [raw[o[i]:o[i + 1]] for i in range(n)]
        self.why, recs, self.pays = zip(*(decode(p) for p in self.pkts)) if n else ((), (), ())
        self.recs = np.array(list(recs), dtype=packets.TX_RECORD).view(np.uint8).reshape(n, 32)
        self.split = np.array([w is None for w in self.why], dtype=bool)
        self.L = np.array([len(p) for p in self.pays], dtype=np.int64)
        self.flags = oracle_c.batch(blob, O.MODE_VERIFY_RX, offsets=offs).astype(np.uint16)
        self.out = self.flags | np.where(self.split, batch.RX_SPLIT, 0).astype(np.uint16)
        self.proto = np.array([p[9] if len(p) > 9 else 0 for p in self.pkts])

    def census(self):
        c = {k: int((self.split & (self.proto == v)).sum()) for k, v in (("tcp", 6), ("udp", 17), ("icmp", 1))}
        c["other"] = int((self.split & ~np.isin(self.proto, (6, 17, 1))).sum())
        for why in ("invalid", "slen < H", "data offset"):
            c[why] = sum(1 for w in self.why if w == why)
        return c


def guarded(dev, nbytes):
    buf = torch.full((GUARD + max(nbytes, 1) + 3 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    return buf


class Run:
    """One call on the device. The data at byte phase `dphase`; pay at byte phase `pphase`
    between guards, laid out by `po` (host offsets; None: tight, from want.L; "same": the
    offsets tensor itself is passed, by leaving pay_offsets out); records, pay_len and out
    between guards too."""

    def __init__(self, dev, blob, offs, want, po=None, dphase=0, pphase=0, validate=False, via_c=False):
        n = self.n = want.n
        offs = np.asarray(offs).astype(np.int64)
        whole = torch.from_numpy(np.concatenate((np.zeros(dphase, np.uint8), blob, np.zeros(4, np.uint8)))).to(dev)
        data = whole[dphase:dphase + max(len(blob), 1)]
        ot = torch.from_numpy(offs).to(dev)
        same = isinstance(po, str)
        if po is None:
            po = np.zeros(n + 1, dtype=np.int64)
            po[1:] = np.cumsum(want.L)
        self.po = po = offs if same else np.asarray(po, dtype=np.int64)
        size = int(po[-1])
        self.paybuf = guarded(dev, size)
        pay = self.paybuf[GUARD + pphase:GUARD + pphase + max(size, 1)]
        self.pay_at = GUARD + pphase
        self.recbuf, self.lenbuf, self.outbuf = guarded(dev, 32 * n), guarded(dev, 4 * n), guarded(dev, 2 * n)
        recs = self.recbuf[GUARD:GUARD + 32 * n].view(n, 32)
        plen = self.lenbuf[GUARD:GUARD + 4 * n].view(torch.int32)
        out = self.outbuf[GUARD:GUARD + 2 * n].view(torch.uint16)
        assert data.data_ptr() % 4 == dphase and pay.data_ptr() % 4 == pphase
        pt = None if same else torch.from_numpy(po).to(dev)
        if via_c:
            rc = _lib.lib().yu_rx_split_ragged(data.data_ptr(), ot.data_ptr(), n, pay.data_ptr(),
                                               (ot if same else pt).data_ptr(), recs.data_ptr(), plen.data_ptr(),
                                               out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            assert rc == _lib.YU_OK
        else:
            got = batch.split_datagrams(data, ot, pay=pay, pay_offsets=pt, records=recs, pay_len=plen, out=out,
                                        validate=validate)
            assert got[0] is pay and got[1] is (ot if same else pt) and got[3] is recs
        torch.cuda.synchronize(dev)  # raises if the stream did not finish cleanly
        self.keep = (whole, ot, pt)

    def check(self, want, skip_all=(), skip_pay=()):
        """Everything equals `want` but for the packets in skip_all (every result
        unspecified) and skip_pay (only the bytes of their own pay span); every other
        byte of the four buffers, guards and slack included, is still 0xA5."""
        n, po = self.n, self.po
        keep = np.ones(n, dtype=bool)
        keep[list(skip_all)] = False
        out = self.outbuf.cpu().numpy()
        lens = self.lenbuf.cpu().numpy()
        recs = self.recbuf.cpu().numpy()
        for name, buf, size in (("out", out, 2 * n), ("pay_len", lens, 4 * n), ("records", recs, 32 * n)):
            assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + size:] == 0xA5).all(), f"{name}: guard written"
        got_out = out[GUARD:GUARD + 2 * n].view(np.uint16)
        got_len = lens[GUARD:GUARD + 4 * n].view(np.int32)
        got_rec = recs[GUARD:GUARD + 32 * n].reshape(n, 32)
        bad = np.nonzero((got_out != want.out) & keep)[0]
        assert bad.size == 0, f"out differs at {bad[:8]}: {got_out[bad[:8]]} want {want.out[bad[:8]]}"
        bad = np.nonzero((got_len != np.where(want.split, want.L, 0)) & keep)[0]
        assert bad.size == 0, f"pay_len differs at {bad[:8]}"
        bad = np.nonzero((got_rec != want.recs).any(1) & keep)[0]
        assert bad.size == 0, f"records differ at {bad[:8]}"
        got = self.paybuf.cpu().numpy()
        exp = np.full_like(got, 0xA5)
        known = np.ones(len(got), dtype=bool)
        for i in range(n):
            a = self.pay_at + int(po[i])
            if i in skip_all or i in skip_pay:
                known[a:self.pay_at + max(int(po[i]), min(int(po[i + 1]), int(po[-1])))] = False
            elif want.split[i] and want.L[i]:
                exp[a:a + int(want.L[i])] = np.frombuffer(want.pays[i], dtype=np.uint8)
        bad = np.nonzero((got != exp) & known)[0]
        assert bad.size == 0, f"{bad.size} pay bytes differ, first at pay byte {bad[0] - self.pay_at}"


def ragged(pkts):
    offs = np.zeros(len(pkts) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p) for p in pkts])
    return np.frombuffer(b"".join(bytes(p) for p in pkts), dtype=np.uint8).copy(), offs


# ---- 1. the executed reference ----------------------------------------------------------
def test_executed_reference_datagrams_split_and_rebuild(dev, oracle_c):
    vecs = [v for v in json.load(open(os.path.join(ROOT, "tests", "golden", "refexec.json")))["modes"]["9"]
            if v.get("src") == "exec"]
    assert len(vecs) == 198
    pkts = []
    for v in vecs:
        b = bytearray.fromhex(v["hex"])
        want = [int(x) for x in v["want"]]
        b[10:12] = want[0].to_bytes(2, "big")  # the two fields as the senders stored them
        f = FIELD_AT.get(b[9])
        if f is not None:
            b[20 + f:22 + f] = want[1].to_bytes(2, "big")
        pkts.append(bytes(b))
    blob, offs = ragged(pkts)
    want = Want(blob, offs, oracle_c)
    assert (want.out == ALL_OK).all()
    r = Run(dev, blob, offs, want, validate=True)  # one launch, tight pay_offsets
    r.check(want)
    # build(split(x)) == x
    n = want.n
    pay = r.paybuf[GUARD:GUARD + max(int(r.po[-1]), 1)]
    recs = r.recbuf[GUARD:GUARD + 32 * n].view(n, 32)
    dst, do, _ = batch.build_datagrams(pay, torch.from_numpy(r.po).to(dev), recs, validate=True)
    assert do.cpu().numpy().tolist() == offs.astype(np.int64).tolist()
    assert np.array_equal(dst.cpu().numpy(), blob)


# ---- 2. the Linux-verified datagrams --------------------------------------------------------
def test_kernel_verified_datagrams(dev, oracle_c):
    f = np.load(os.path.join(ROOT, "tests", "golden", "kernel_verified.npz"))
    pkts = [bytes(b[int(s):int(e)]) for b, o in ((f["sent_blob"], f["sent_offs"]), (f["kernel_blob"], f["kernel_offs"]))
            for s, e in zip(o[:-1], o[1:])]
    assert len(pkts) == 110
    blob, offs = ragged(pkts)
    want = Want(blob, offs, oracle_c)
    assert (want.out == ALL_OK).all()
    Run(dev, blob, offs, want, validate=True).check(want)


# ---- 3. seeded received batches ----------------------------------------------------------------
def delivery_faults(rng):
    """16 datagrams that pass IsValid and fail a delivery test: 8 whose segment is shorter
    than the transport header (TotalLength pulled in, the cut bytes left as trailing
    bytes), 8 TCP ones whose DataOffset is under 20 or past the segment. rxgen's own
    damage almost never produces either (a flipped header bit has to hit the IHL, the
    TotalLength or the data-offset nibble): about one of each in a batch of 600."""
    pkts = []
    for i in range(8):
        proto = (6, 17, 1, 6)[i % 4]
        p = rxgen.make_packet(rng, int(rng.integers(0, 40)), proto=proto)
        hl = (p[0] & 15) * 4
        tl = hl + int(rng.integers(0, H_OF[proto]))
        p[2:4] = tl.to_bytes(2, "big")
        pkts.append(bytes(p))
    for i in range(8):
        p = rxgen.make_packet(rng, int(rng.integers(0, 30)), proto=6)
        hl, slen = (p[0] & 15) * 4, len(p) - (p[0] & 15) * 4
        nib = int(rng.integers(0, 5)) if i % 2 else slen // 4 + 1  # slen < 60: the nibble holds it
        p[hl + 12] = (nib << 4) | (p[hl + 12] & 15)
        pkts.append(bytes(p))
    return pkts


@pytest.mark.parametrize("hi", (1480, 96))
def test_received_batches_at_every_phase(dev, oracle_c, hi):
    """rxgen.rx_batch(rng, 600, 0, hi, bad=0.5), with delivery_faults' 16 datagrams after
    them: no seed of rx_batch alone holds five packets with slen < H and five with a bad
    DataOffset (400 seeds tried on a CPU: at most one of each), so those are added; the
    600 are as rx_batch gives them."""
    rng = np.random.default_rng(SEEDS[hi])
    blob, offs = rxgen.rx_batch(rng, 600, 0, hi, bad=0.5)
    o = offs.astype(np.int64)
    blob, offs = ragged([blob.tobytes()[o[i]:o[i + 1]] for i in range(600)] + delivery_faults(rng))
    want = Want(blob, offs, oracle_c)
    c = want.census()
    assert min(c[k] for k in ("tcp", "udp", "icmp", "other")) >= 20, c
    assert min(c[k] for k in ("invalid", "slen < H", "data offset")) >= 5, c
    slack = np.zeros(want.n + 1, dtype=np.int64)
    slack[1:] = np.cumsum(want.L + (np.arange(want.n) % 6))  # slack 0..5 after each payload
    for dphase in range(4):
        for pphase in range(4):
            Run(dev, blob, offs, want, po=slack, dphase=dphase, pphase=pphase).check(want)


def test_short_header_datagrams_never_split(dev, oracle_c):
    rng = np.random.default_rng(200)
    blob, offs = ragged([rxgen.short_header_packet(rng, int(rng.integers(20, 81))) for _ in range(200)])
    want = Want(blob, offs, oracle_c)
    assert not want.split.any() and set(want.why) <= {"invalid", "short header"}
    r = Run(dev, blob, offs, want, po="same", dphase=1, pphase=2)
    r.check(want)
    assert (r.outbuf[GUARD:GUARD + 2 * want.n].view(torch.uint16).cpu().numpy() == want.flags).all()


# ---- 4. grid-stride and prefetch ---------------------------------------------------------------
@pytest.fixture(scope="module")
def many(oracle_c):
    rng = np.random.default_rng(70000)
    n = 70000
    protos = rng.choice([6, 17, 1, 47], n)
    pkts = [rxgen.make_packet(rng, int(L), proto=int(p), ihl=5) for L, p in zip(rng.integers(0, 65, n), protos)]
    blob, offs = ragged(pkts)
    return blob, offs, Want(blob, offs, oracle_c)


@pytest.mark.parametrize("po", (None, "same"))
def test_more_packets_than_waves(dev, many, po):
    blob, offs, want = many
    assert want.n == 70000 and want.n > 304 * 64 * 4 // 2 and want.split.all()
    Run(dev, blob, offs, want, po=po, dphase=3, pphase=1).check(want)


# ---- 5. limits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 4, 5))
def test_few_packets(dev, oracle_c, n):
    rng = np.random.default_rng(n)
    blob, offs = ragged([rxgen.make_packet(rng, int(rng.integers(0, 3000))) for _ in range(n)])
    want = Want(blob, offs, oracle_c)
    assert want.split.all()
    Run(dev, blob, offs, want, dphase=2, pphase=3, validate=True).check(want)
    assert batch.split_variant(n) == "k_split<4>"


def test_the_largest_datagram(dev, oracle_c):
    rng = np.random.default_rng(65535)
    pkt = rxgen.make_packet(rng, 65535 - 20, proto=6, ihl=5)
    assert len(pkt) == 65535
    blob, offs = ragged([pkt])
    want = Want(blob, offs, oracle_c)
    assert want.out[0] == ALL_OK and want.L[0] == 65535 - 40
    Run(dev, blob, offs, want, dphase=1, pphase=3, validate=True).check(want)


# ---- 6. the contract --------------------------------------------------------------------------------
def test_out_of_contract_packets_stay_inside_their_span(dev, oracle_c):
    """131 good packets and five out of contract: a 65536-byte packet (20), offsets
    decreasing (45; and again at the last packet, 135), a packet ending past offsets[n]
    (134), room 3 short (70) and pay_offsets decreasing (100). tests/cpp/rx_split.cpp runs
    the same cases on a CPU; none faults. Every other packet is exact; the two room cases
    keep exact out, records and pay_len; no byte outside the offending packets' own spans
    differs from 0xA5 or its expected value."""
    rng = np.random.default_rng(6)
    n = 136
    bad = {"over": 20, "dec": 45, "short": 70, "pdec": 100, "past": 134, "tail": 135}
    pkts = [bytes(rxgen.make_packet(rng, int(rng.integers(0, 131)))) for _ in range(n)]
    pkts[bad["over"]] = bytes(rxgen.make_packet(rng, 65536 - 20, proto=17, ihl=5))
    pkts[bad["short"]] = bytes(rxgen.make_packet(rng, 708, proto=17, ihl=5))
    assert len(pkts[bad["over"]]) == 65536
    blob, o = ragged(pkts)
    want = Want(blob, o, oracle_c)  # what each packet's own bytes give
    o = o.astype(np.int64)
    unspecified = (bad["over"], bad["dec"], bad["past"], bad["tail"])
    assert want.split[[i for i in range(n) if i not in unspecified]].all() and want.L[bad["short"]] == 700
    # the device's table. Packet 45's start moves 7 bytes past its end: offsets decreases at it, and packet 44
    # ends there, with packet 45's bytes and 7 more as trailing bytes past its TotalLength (the same results).
    # offsets[n] moves 5 bytes before packet 134's end: that packet ends past it, and packet 135 decreases.
    t = o.copy()
    t[bad["dec"]] = o[bad["dec"] + 1] + 7
    t[n] = o[n - 1] - 5
    # pay: tight, but packet 70 three short, and pay_offsets decreasing at 100 (packet 99 has slack up to the
    # end, packet 100 no span)
    room = want.L.copy()
    room[bad["short"]] -= 3
    room[bad["over"]] = 100
    po = np.zeros(n + 1, dtype=np.int64)
    po[1:] = np.cumsum(room)
    po[bad["pdec"]] = po[-1]
    with pytest.raises(ValueError):
        batch.split_datagrams(torch.from_numpy(blob).to(dev), torch.from_numpy(t).to(dev), validate=True)
    r = Run(dev, blob, t, want, po=po, dphase=2, pphase=1)  # YU_OK, and the stream synchronises cleanly
    r.check(want, skip_all=unspecified, skip_pay=(bad["short"], bad["pdec"]))


# ---- 7. the C call -----------------------------------------------------------------------------------
def test_c_call_at_odd_addresses(dev, oracle_c):
    rng = np.random.default_rng(7)
    blob, offs = rxgen.rx_batch(rng, 64, 0, 300, bad=0.3)
    want = Want(blob, offs, oracle_c)
    for dphase, pphase in ((1, 3), (3, 1)):
        Run(dev, blob, offs, want, dphase=dphase, pphase=pphase, via_c=True).check(want)
