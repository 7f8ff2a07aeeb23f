"""yu_tx_build_ragged on the MI355X (k_build<4>): whole outgoing IPv4 datagrams built on
the device from payloads and 32-byte records.

1. the 198 datagrams the reference's own senders produced when executed end to end
   (tests/golden/refexec.json), rebuilt in one launch from the fields in their own
   headers plus their payloads, byte for byte;
2. seeded mixed-protocol batches against a numpy header encoder plus the C oracle's
   ragged TX_DATAGRAM, at every payload and destination byte phase;
3. bounds: guards, a leading gap, slack, and the C call with out == NULL;
4. the round trip through VERIFY_RX;
5. the limit T = 65535;
6. the contract batch: out-of-contract packets stay inside their own spans.

Every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from yustack_amd import _lib, batch, packets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
H_OF = {6: 20, 17: 8, 1: 4}
FIELD_AT = {6: 36, 17: 26, 1: 22}  # the transport field's offset in the image (IHL 5)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def oracle_c():
    return O.C()


def be16(x):
    return [(int(x) >> 8) & 0xFF, int(x) & 0xFF]


def be32(x):
    return be16(int(x) >> 16) + be16(int(x) & 0xFFFF)


def encode_zero(rec, pay: np.ndarray) -> np.ndarray:
    """The image of include/yucsum.h with both checksum fields zero (numpy, byte by byte)."""
    proto = int(rec["proto"])
    H = H_OF.get(proto, 0)
    T = 20 + H + len(pay)
    b = [0x45, int(rec["tos"])] + be16(T) + be16(rec["ip_id"]) + be16(rec["frag"]) + [int(rec["ttl"]), proto, 0, 0]
    b += rec["src"].tolist() + rec["dst"].tolist()
    if proto == 6:
        b += be16(rec["sport"]) + be16(rec["dport"]) + be32(rec["seq"]) + be32(rec["ack"])
        b += [((int(rec["doff"]) // 4) << 4) & 0xFF, int(rec["flags"])] + be16(rec["window"]) + [0, 0, 0, 0]
    elif proto == 17:
        b += be16(rec["sport"]) + be16(rec["dport"]) + be16(8 + len(pay)) + [0, 0]
    elif proto == 1:
        b += be16(rec["sport"]) + [0, 0]
    return np.concatenate((np.array(b, dtype=np.uint8), pay))


def expected(recs, pays, oracle_c):
    """(images with both fields in place, out): the numpy encoder's zero-field images,
    the fields by the C oracle's ragged TX_DATAGRAM over them."""
    imgs = [encode_zero(r, p) for r, p in zip(recs, pays)]
    offs = np.zeros(len(imgs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(i) for i in imgs])
    want = oracle_c.batch(np.concatenate(imgs), O.MODE_TX_DATAGRAM, offsets=offs).reshape(-1, 2)
    for img, r, w in zip(imgs, recs, want):
        img[10:12] = be16(w[0])
        f = FIELD_AT.get(int(r["proto"]))
        if f is not None:
            img[f:f + 2] = be16(w[1])
        else:
            assert w[1] == 0
    return imgs, want.reshape(-1)


class Placed:
    """A batch on the device: the payloads at byte phase `pphase`, dst inside guards of
    0xA5 at byte phase `dphase` with `lead` bytes before the first packet and `room[i]`
    bytes per packet."""

    def __init__(self, dev, recs, pays, room, pphase=0, dphase=0, lead=0):
        n = len(pays)
        self.n, self.lead, self.room = n, lead, np.asarray(room, dtype=np.int64)
        po = np.zeros(n + 1, dtype=np.int64)
        po[1:] = np.cumsum([len(p) for p in pays])
        blob = np.concatenate([np.zeros(pphase, np.uint8)] + list(pays) + [np.zeros(1, np.uint8)])
        self.pay_all = torch.from_numpy(blob).to(dev)
        self.payload = self.pay_all[pphase:pphase + int(po[-1])] if po[-1] else self.pay_all[pphase:pphase + 1]
        self.po = torch.from_numpy(po).to(dev)
        self.recs = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(n, 32).copy()).to(dev)
        do = np.zeros(n + 1, dtype=np.int64)
        do[0] = lead
        do[1:] = lead + np.cumsum(self.room)
        self.do_host = do
        self.size = int(do[-1])
        self.buf = torch.full((GUARD + dphase + self.size + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.dst = self.buf[GUARD + dphase:GUARD + dphase + self.size]
        self.do = torch.from_numpy(do).to(dev)
        assert self.payload.data_ptr() % 4 == pphase and self.dst.data_ptr() % 4 == dphase

    def check(self, imgs, skip=()):
        """dst holds imgs[i] at its offset for every i not in `skip`; every other byte of
        the buffer outside the skipped packets' spans (guards, the leading gap, slack) is
        still 0xA5."""
        got = self.buf.cpu().numpy()
        want = np.full_like(got, 0xA5)
        known = np.ones(len(got), dtype=bool)
        base = self.dst.data_ptr() - self.buf.data_ptr()
        for i in range(self.n):
            a = base + int(self.do_host[i])
            if i in skip:
                e = base + max(int(self.do_host[i]), min(int(self.do_host[i + 1]), int(self.do_host[-1])))
                known[a:e] = False
            else:
                want[a:a + len(imgs[i])] = imgs[i]
        bad = np.nonzero((got != want) & known)[0]
        assert bad.size == 0, f"{bad.size} bytes differ, first at buffer byte {bad[0]} (dst byte {bad[0] - base})"


def random_records(rng, n, lens, protos=(6, 17, 1, 47)):
    recs = packets.tx_records(
        n, src=rng.integers(0, 256, (n, 4), dtype=np.uint8), dst=rng.integers(0, 256, (n, 4), dtype=np.uint8),
        sport=rng.integers(0, 65536, n), dport=rng.integers(0, 65536, n), seq=rng.integers(0, 2 ** 32, n),
        ack=rng.integers(0, 2 ** 32, n), window=rng.integers(0, 65536, n), flags=rng.integers(0, 256, n),
        proto=rng.choice(protos, n), ttl=rng.integers(0, 256, n), ip_id=rng.integers(0, 65536, n),
        tos=rng.integers(0, 256, n), frag=rng.integers(0, 65536, n))
    # TCP: any option length the payload can hold
    most = np.minimum(60, 20 + (np.asarray(lens) // 4) * 4)
    recs["doff"] = 20 + 4 * (rng.integers(0, 11, n) % ((most - 20) // 4 + 1))
    return recs


def draw_lengths(rng, n):
    pool = np.concatenate((np.arange(0, 131), np.arange(1020, 1031), np.arange(1459, 1462), [4099]))
    short = rng.integers(0, 131, n)
    lens = np.where(rng.random(n) < 0.7, short, rng.choice(pool, n))
    lens[rng.integers(0, n)] = 4099  # past one step of four slots
    return lens


# ---- 1. the executed reference ----------------------------------------------------------
def test_executed_reference_datagrams(dev):
    vecs = [v for v in json.load(open(os.path.join(ROOT, "tests", "golden", "refexec.json")))["modes"]["9"]
            if v.get("src") == "exec"]
    assert len(vecs) == 198
    recs = np.zeros(len(vecs), dtype=packets.TX_RECORD)
    pays, imgs, wants, kinds, left_out = [], [], [], set(), 0
    for r, v in zip(recs, vecs):
        b = np.frombuffer(bytes.fromhex(v["hex"]), dtype=np.uint8).copy()
        want = [int(x) for x in v["want"]]
        proto = int(b[9])
        H = H_OF.get(proto, 0)
        if b[0] != 0x45 or len(b) != ((int(b[2]) << 8) | int(b[3])) or len(b) < 20 + H:
            left_out += 1
            continue
        b[10:12] = be16(want[0])  # the two fields as the senders stored them
        if proto in FIELD_AT:
            b[FIELD_AT[proto]:FIELD_AT[proto] + 2] = be16(want[1])
        raw = bytes(b)

        def num(at, size=2):
            return int.from_bytes(raw[at:at + size], "big")
        r["tos"], r["ip_id"], r["frag"], r["ttl"], r["proto"] = raw[1], num(4), num(6), raw[8], proto
        r["src"], r["dst"], r["doff"] = b[12:16], b[16:20], 20
        if proto in (6, 17):
            r["sport"], r["dport"] = num(20), num(22)
        if proto == 6:
            r["seq"], r["ack"] = num(24, 4), num(28, 4)
            r["doff"], r["flags"], r["window"] = (raw[32] >> 4) * 4, raw[33], num(34)
            kinds.add("tcp" if r["doff"] == 20 else "tcp+options")
        elif proto == 17:
            kinds.add("udp")
        elif proto == 1:
            r["sport"] = num(20)
            kinds.add("icmp")
        pays.append(b[20 + H:].copy())
        imgs.append(b)
        wants += want
    assert left_out == 0 and len(imgs) == 198
    assert kinds == {"udp", "icmp", "tcp", "tcp+options"}
    payload = torch.from_numpy(np.concatenate(pays)).to(dev)
    po = np.zeros(199, dtype=np.int64)
    po[1:] = np.cumsum([len(p) for p in pays])
    rt = torch.from_numpy(recs.view(np.uint8).reshape(198, 32).copy()).to(dev)
    dst, do, out = batch.build_datagrams(payload, torch.from_numpy(po).to(dev), rt, validate=True)  # one launch, tight
    whole = np.concatenate(imgs)
    assert do[-1].item() == len(whole) and dst.numel() == len(whole)
    assert np.array_equal(dst.cpu().numpy(), whole)
    assert out.cpu().numpy().tolist() == wants
    # six of the UDP datagrams sum to 0xFFFF and keep 0x0000 in the field
    assert sum(1 for i, b in enumerate(imgs) if b[9] == 17 and wants[2 * i + 1] == 0) == 6
    # yu_csum_fill_ragged(TX_DATAGRAM) on the result changes no byte
    again = dst.clone()
    batch.checksum_ragged(again, do, "tx_datagram", fill=True)
    assert torch.equal(again, dst)


# ---- 2. the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 300))
def test_mixed_batches_match_the_oracle(dev, oracle_c, n):
    rng = np.random.default_rng(1300 + n)
    for pphase in range(4):
        for dphase in range(4):
            lens = draw_lengths(rng, n)
            recs = random_records(rng, n, lens)
            pays = [rng.integers(0, 256, int(L), dtype=np.uint8) for L in lens]
            imgs, want = expected(recs, pays, oracle_c)
            p = Placed(dev, recs, pays, [len(i) for i in imgs], pphase, dphase)
            _, _, out = batch.build_datagrams(p.payload, p.po, p.recs, dst=p.dst, dst_offsets=p.do, validate=True)
            assert np.array_equal(out.cpu().numpy(), want), (pphase, dphase)
            p.check(imgs)


def test_tight_offsets_are_computed_on_the_device(dev, oracle_c):
    rng = np.random.default_rng(77)
    n = 40
    lens = draw_lengths(rng, n)
    recs = random_records(rng, n, lens)
    pays = [rng.integers(0, 256, int(L), dtype=np.uint8) for L in lens]
    imgs, want = expected(recs, pays, oracle_c)
    p = Placed(dev, recs, pays, [len(i) for i in imgs])
    dst, do, out = batch.build_datagrams(p.payload, p.po, p.recs)
    assert do.cpu().numpy().tolist() == (p.do_host - p.lead).tolist()
    assert np.array_equal(dst.cpu().numpy(), np.concatenate(imgs)) and np.array_equal(out.cpu().numpy(), want)
    assert batch.build_variant(n) == "k_build<4>"


# ---- 3. bounds -----------------------------------------------------------------------------
@pytest.mark.parametrize("dphase", range(4))
def test_guards_gap_and_slack_are_never_written(dev, oracle_c, dphase):
    rng = np.random.default_rng(31 + dphase)
    n = 70
    lens = draw_lengths(rng, n)
    recs = random_records(rng, n, lens)
    pays = [rng.integers(0, 256, int(L), dtype=np.uint8) for L in lens]
    imgs, want = expected(recs, pays, oracle_c)
    room = np.array([len(i) for i in imgs]) + rng.integers(0, 8, n)
    p = Placed(dev, recs, pays, room, pphase=(dphase + 1) % 4, dphase=dphase, lead=13)
    assert int(p.do_host[0]) > 0
    _, _, out = batch.build_datagrams(p.payload, p.po, p.recs, dst=p.dst, dst_offsets=p.do, validate=True)
    assert np.array_equal(out.cpu().numpy(), want)
    p.check(imgs)
    # the C call with out == NULL: the same image
    p.buf.fill_(0xA5)
    rc = _lib.lib().yu_tx_build_ragged(p.payload.data_ptr(), p.po.data_ptr(), p.recs.data_ptr(), n, p.dst.data_ptr(),
                                       p.do.data_ptr(), None, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == _lib.YU_OK
    torch.cuda.synchronize(dev)
    p.check(imgs)


# ---- 4. the round trip -----------------------------------------------------------------------
def test_built_datagrams_verify_as_received(dev):
    rng = np.random.default_rng(404)
    n = 96
    lens = draw_lengths(rng, n)
    recs = random_records(rng, n, lens)
    recs["proto"] = np.array([1, 6, 17, 47])[np.arange(n) % 4]
    pays = [rng.integers(0, 256, int(L), dtype=np.uint8) for L in lens]
    p = Placed(dev, recs, pays, [20 + H_OF.get(int(r["proto"]), 0) + len(q) for r, q in zip(recs, pays)])
    dst, do, out = batch.build_datagrams(p.payload, p.po, p.recs)
    flags = batch.checksum_ragged(dst, do, "verify_rx").cpu().numpy()
    o = out.cpu().numpy().reshape(n, 2)
    l4 = recs["proto"] != 47
    assert (flags[l4] == (batch.RX_IP_OK | batch.RX_L4 | batch.RX_L4_OK)).all()
    assert (flags[~l4] == batch.RX_IP_OK).all() and (o[~l4, 1] == 0).all()


# ---- 5. the limit ------------------------------------------------------------------------------
def test_the_largest_datagram(dev, oracle_c):
    rng = np.random.default_rng(65535)
    recs = random_records(rng, 1, [65507], protos=(17,))
    pays = [rng.integers(0, 256, 65507, dtype=np.uint8)]
    imgs, want = expected(recs, pays, oracle_c)
    assert len(imgs[0]) == 65535
    p = Placed(dev, recs, pays, [65535], pphase=1, dphase=3)
    _, _, out = batch.build_datagrams(p.payload, p.po, p.recs, dst=p.dst, dst_offsets=p.do, validate=True)
    assert np.array_equal(out.cpu().numpy(), want)
    p.check(imgs)


# ---- 6. the contract ---------------------------------------------------------------------------
def test_out_of_contract_packets_stay_inside_their_span(dev, oracle_c):
    """130 good packets and four out of contract: T = 65536 (packet 20), room short by 3
    (50), dst_offsets decreasing (80) and a TCP record with doff 24 and L = 2 (110).
    tests/cpp/tx_build.cpp runs the same four cases on a CPU; none faults. Every good
    packet is exact, guards and the other packets' spans are untouched, and the doff
    packet differs from its expected image in at most its two field bytes."""
    rng = np.random.default_rng(6)
    n = 134
    bad = {"over": 20, "short": 50, "dec": 80, "doff": 110}
    lens = rng.integers(0, 131, n)
    lens[bad["over"]], lens[bad["doff"]] = 65508, 2
    recs = random_records(rng, n, lens)
    recs["proto"][bad["over"]] = 17
    recs["proto"][bad["doff"]], recs["doff"][bad["doff"]] = 6, 24
    recs["proto"][bad["short"]] = 6  # a cut inside the payload's first dwords
    pays = [rng.integers(0, 256, int(L), dtype=np.uint8) for L in lens]
    good = [i for i in range(n) if i not in (bad["over"], bad["short"], bad["dec"])]
    gi, gw = expected(recs[good], [pays[i] for i in good], oracle_c)  # the doff packet: by the same formulas
    imgs, want = [None] * n, np.zeros((n, 2), dtype=np.uint16)
    for k, i in enumerate(good):
        imgs[i], want[i] = gi[k], gw[2 * k:2 * k + 2]
    room = np.array([20 + H_OF.get(int(r["proto"]), 0) + len(q) for r, q in zip(recs, pays)], dtype=np.int64)
    room[bad["over"]] = 65536
    room[bad["short"]] -= 3
    p = Placed(dev, recs, pays, room, pphase=2, dphase=1, lead=5)
    do = p.do_host.copy()
    do[bad["dec"]] = do[-1]  # decreases at 80: packet 79 has slack up to the end, packet 80 no span
    p.do_host, p.do = do, torch.from_numpy(do).to(dev)
    with pytest.raises(ValueError):
        batch.build_datagrams(p.payload, p.po, p.recs, dst=p.dst, dst_offsets=p.do, validate=True)
    _, _, out = batch.build_datagrams(p.payload, p.po, p.recs, dst=p.dst, dst_offsets=p.do)
    torch.cuda.synchronize(dev)
    # the doff packet: every byte but the two field bytes
    got = p.dst.cpu().numpy()
    a = int(do[bad["doff"]])
    img = imgs[bad["doff"]]
    diff = np.nonzero(got[a:a + len(img)] != img)[0]
    assert set(diff.tolist()) <= {36, 37}
    p.check(imgs, skip=(bad["over"], bad["short"], bad["dec"], bad["doff"]))
    # (the span the decreasing pair left empty, [old offset of 80, offset of 81), is "known": still 0xA5)
    clean = [i for i in good if i != bad["doff"]]
    assert np.array_equal(out.cpu().numpy().reshape(n, 2)[clean], want[clean])
