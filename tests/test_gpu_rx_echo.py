"""Received datagrams answered on the MI355X: yu_rx_reply (k_reply and the scan) and the
chain parse -> demux -> reply -> build_iov (batch.echo_datagrams).

1. every UDP datagram the reference's sendUDP produced when executed
   (tests/golden/refexec.json): the request is that datagram with addresses and ports
   turned round, and the echo must reproduce the datagram byte for byte;
2. the ICMP Echo replies the reference's sendICMPv4 produced when executed
   (tests/golden/echo_icmp.json): type-8 requests carrying the same bytes, some with a
   non-zero code, must be answered with exactly those datagrams;
3. a seeded mixed batch of 3 * 2048 + 5 received packets, half of them damaged, against a
   numpy restatement of which packets are answered and with which record; the reply images
   against a numpy header encoder and the C oracle's ragged TX_DATAGRAM, and VERIFY_RX
   accepts every reply; need = 0 and IP_OK | L4_OK, ep_echo mixed;
4. the seams n = 0, 1, 63, 64, 65, 2047, 2048, 2049;
5. writes: the inputs are unchanged and the workspace is written only inside
   yu_rx_reply_workspace_bytes(n);
6. the four calls captured as one graph and replayed on a second batch.

Every pointer is valid device memory and every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

import demux_ref
import rxgen
from oracle import oracle as O
from test_gpu_rx_demux import table_from
from test_gpu_tx_build import expected
from yustack_amd import batch, packets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
OK_BITS = batch.RX_IP_OK | batch.RX_L4_OK
ACCEPTED = batch.RX_IP_OK | batch.RX_L4 | batch.RX_L4_OK
N_BIG = 3 * 2048 + 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def oracle_c():
    return O.C()


def ragged(pkts):
    offs = np.zeros(len(pkts) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(p) for p in pkts])
    return np.frombuffer(b"".join(bytes(p) for p in pkts) + b"\0", dtype=np.uint8).copy(), offs


def upload(dev, pkts):
    blob, offs = ragged(pkts)
    return torch.from_numpy(blob).to(dev), torch.from_numpy(offs).to(dev)


def replies(dst, r_offsets):
    d, o = dst.cpu().numpy(), r_offsets.cpu().numpy()
    return [bytes(d[int(a):int(b)]) for a, b in zip(o[:-1], o[1:])]


def build_requests(dev, recs, pays):
    """The requests as yu_tx_build_ragged builds them from records and payloads."""
    po = np.zeros(len(pays) + 1, dtype=np.int64)
    po[1:] = np.cumsum([len(p) for p in pays])
    payload = torch.from_numpy(np.concatenate(list(pays) + [np.zeros(1, np.uint8)])).to(dev)
    rt = torch.from_numpy(recs.view(np.uint8).reshape(len(pays), 32).copy()).to(dev)
    data, offs, _ = batch.build_datagrams(payload, torch.from_numpy(po).to(dev), rt, validate=True)
    return data, offs


# ---- 1. the executed UDP senders -----------------------------------------------------------
def test_executed_udp_datagrams_are_echoed(dev):
    vecs = [v for v in json.load(open(os.path.join(ROOT, "tests", "golden", "refexec.json")))["modes"]["9"]
            if v.get("src") == "exec"]
    want = []
    for v in vecs:
        b = bytearray.fromhex(v["hex"])
        if b[9] != 17:
            continue
        b[10:12] = int(v["want"][0]).to_bytes(2, "big")  # the two fields as sendUDP and WritePacket stored them
        b[26:28] = int(v["want"][1]).to_bytes(2, "big")
        want.append(bytes(b))
    n = len(want)
    assert n == 76 and all(d[0] == 0x45 and len(d) == int.from_bytes(d[2:4], "big") for d in want)
    num = lambda d, at: int.from_bytes(d[at:at + 2], "big")  # noqa: E731
    # the request: D with addresses and ports turned round
    recs = packets.tx_records(n, src=np.array([list(d[16:20]) for d in want], dtype=np.uint8),
                              dst=np.array([list(d[12:16]) for d in want], dtype=np.uint8),
                              sport=[num(d, 22) for d in want], dport=[num(d, 20) for d in want], proto=17,
                              ttl=np.arange(n) % 200 + 1, ip_id=np.arange(n) * 7)  # nothing of these is echoed
    data, offs = build_requests(dev, recs, [np.frombuffer(d[28:], dtype=np.uint8) for d in want])
    ports = sorted({num(d, 20) for d in want})
    ids = packets.endpoint_ids(len(ports), local_port=ports, proto=17, kind=2)
    table, m = batch.demux_table(ids, dev)
    dst, r_offsets, out, flags, ep = batch.echo_datagrams(data, offs, table, m)
    torch.cuda.synchronize(dev)
    assert (ep.cpu().numpy() < m).all() and (flags.cpu().numpy() & batch.RX_SPLIT).all()
    assert replies(dst, r_offsets) == want
    o = out.cpu().numpy().reshape(n, 2)
    assert o[:, 0].tolist() == [num(d, 10) for d in want] and o[:, 1].tolist() == [num(d, 26) for d in want]
    assert int(r_offsets[-1]) == int(offs[-1])  # a reply is exactly as long as its request
    # a receiver that drops on checksum outcomes answers the same: every request verifies
    dst2, ro2, _, _, _ = batch.echo_datagrams(data, offs, table, m, need=OK_BITS)
    assert replies(dst2, ro2) == want
    # no listener: nothing is answered
    empty, m0 = batch.demux_table(packets.endpoint_ids(0), dev)
    _, ro3, out3, _, ep3 = batch.echo_datagrams(data, offs, empty, m0)
    assert (ro3 == 0).all() and (out3 == 0).all() and (ep3.cpu().numpy() == NONE).all()


# ---- 2. the executed ICMP replies -------------------------------------------------------------
def test_executed_icmp_echo_replies(dev):
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "echo_icmp.json")))["icmp_echo_reply"]
    assert len(fx) == 13 and all(v["executed"] is True for v in fx)
    assert [len(v["data"]) // 2 for v in fx] == [0, 1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 1472]
    want = [bytes.fromhex(v["reply"]) for v in fx]
    n = len(fx)
    code = np.where(np.arange(n) % 3 == 1, 0, np.arange(n) * 19 % 256)  # some requests carry a code
    assert (code != 0).any() and (code == 0).any()
    recs = packets.tx_records(n, src=np.array([list(bytes.fromhex(v["dst"])) for v in fx], dtype=np.uint8),
                              dst=np.array([list(bytes.fromhex(v["src"])) for v in fx], dtype=np.uint8),
                              sport=(8 << 8) | code, proto=1, ttl=np.arange(n) + 3, ip_id=np.arange(n) + 100)
    data, offs = build_requests(dev, recs, [np.frombuffer(bytes.fromhex(v["data"]), dtype=np.uint8) for v in fx])
    table, m = batch.demux_table(packets.endpoint_ids(0), dev)
    dst, r_offsets, out, flags, _ = batch.echo_datagrams(data, offs, table, m, need=OK_BITS)
    torch.cuda.synchronize(dev)
    assert (flags.cpu().numpy() == (ACCEPTED | batch.RX_SPLIT)).all()
    assert replies(dst, r_offsets) == want
    o = out.cpu().numpy().reshape(n, 2)
    assert o[:, 0].tolist() == [int.from_bytes(d[10:12], "big") for d in want]
    assert o[:, 1].tolist() == [int.from_bytes(d[22:24], "big") for d in want]
    _, ro, _, _, _ = batch.echo_datagrams(data, offs, table, m, icmp=False)
    assert (ro == 0).all()


# ---- 3. the seeded mixed batch -------------------------------------------------------------------
def fix_icmp(p):
    """Every ICMP packet whose header parses becomes an Echo request (a valid sum again)."""
    if len(p) < 20:
        return p
    hl, tl = (p[0] & 15) * 4, (p[2] << 8) | p[3]
    if not (20 <= hl <= tl <= len(p)) or p[9] != 1 or tl - hl < 4:
        return p
    p = bytearray(p)
    p[hl], p[hl + 2], p[hl + 3] = 8, 0, 0
    p[hl + 2:hl + 4] = (~O.checksum(bytes(p[hl:tl]), 0) & 0xFFFF).to_bytes(2, "big")
    return bytes(p)


class Mixed:
    """The batch, parsed once on the device; its table; what a numpy restatement expects."""

    def __init__(self, dev, seed, n=N_BIG):
        rng = np.random.default_rng(seed)
        blob, offs = rxgen.rx_batch(rng, n, lo=0, hi=160, bad=0.5)
        pkts = [bytes(blob[int(a):int(b)]) for a, b in zip(offs[:-1], offs[1:])]
        self.pkts = [fix_icmp(p) if k % 3 else p for k, p in enumerate(pkts)]  # two ICMP packets in three
        self.n, self.dev = n, dev
        self.data, self.offs = upload(dev, self.pkts)
        recs, _, _ = batch.parse_datagrams(self.data, self.offs, verify=False)
        self.ids = table_from(packets.rx_records(recs), rng)
        self.table, self.m = batch.demux_table(self.ids, dev)
        self.echo = rng.integers(0, 3, self.m).astype(np.uint8) * 85  # a third of the endpoints do not echo
        self.echo_t = torch.from_numpy(self.echo).to(dev)

    def head(self, k):
        """The first k packets as a batch of their own, with the same table."""
        h = object.__new__(Mixed)
        h.__dict__.update(self.__dict__)
        h.n, h.pkts = k, self.pkts[:k]
        h.data, h.offs = upload(self.dev, h.pkts)
        return h

    def stages(self, need, echo, what=3):
        """parse, demux, reply as separate calls: everything on the host."""
        recs, views, flags = batch.parse_datagrams(self.data, self.offs, verify=need != 0)
        ep, _ = batch.demux_datagrams(recs, self.table, self.m, flags=flags, need=need)
        r_recs, r_offsets = batch.reply_datagrams(recs, views, ep, self.m, flags=flags, need=need, what=what,
                                                  ep_echo=self.echo_t if echo else None)
        torch.cuda.synchronize(self.dev)
        return (packets.rx_records(recs), views.cpu().numpy(), flags.cpu().numpy(), ep.cpu().numpy(),
                packets.rx_records(r_recs), r_offsets.cpu().numpy())

    def restated(self, recs, views, flags, need, echo, what=3):
        """(reply records, T) by the rules of include/yucsum.h, in numpy; ep by the
        restated demultiplexer of demux_ref."""
        ep, _ = demux_ref.demux(self.ids, recs, flags, need)
        gate = (flags & (need | batch.RX_SPLIT)) == (need | batch.RX_SPLIT)
        L = views[:, 1]
        icmp = gate & (recs["proto"] == 1) & ((recs["sport"] >> 8) == 8) & (L <= 65535 - 24) & bool(what & 1)
        reach = ep < self.m
        if echo:
            reach &= self.echo[np.where(ep < self.m, ep, 0)] != 0
        udp = gate & (recs["proto"] == 17) & reach & (L <= 65535 - 28) & bool(what & 2)
        want = np.zeros(len(recs), dtype=packets.TX_RECORD)
        for mask, proto in ((icmp, 1), (udp, 17)):
            want["src"][mask], want["dst"][mask] = recs["dst"][mask], recs["src"][mask]
            want["proto"][mask], want["ttl"][mask] = proto, 64
        want["sport"][udp], want["dport"][udp] = recs["dport"][udp], recs["sport"][udp]
        T = np.where(icmp, 24 + L, 0) + np.where(udp, 28 + L, 0)
        return ep, want, T, icmp, udp


@pytest.fixture(scope="module")
def mixed(dev):
    return Mixed(dev, 19003)


@pytest.mark.parametrize("need,echo", ((0, False), (OK_BITS, True), (0, True)))
def test_mixed_batch_against_the_restatement(dev, oracle_c, mixed, need, echo):
    recs, views, flags, ep, r_recs, r_offsets = mixed.stages(need, echo)
    want_ep, want, T, icmp, udp = mixed.restated(recs, views, flags, need, echo)
    assert np.array_equal(ep, want_ep)
    # the batch exercises every branch
    assert icmp.sum() >= 100 and udp.sum() >= 100 and (~(icmp | udp) & (recs["proto"] == 17)).sum() >= 50
    assert (recs["proto"] == 6).sum() >= 100 and ((flags & batch.RX_SPLIT) == 0).sum() >= 100
    assert ((recs["proto"] == 1) & ~icmp).sum() >= 50
    assert np.array_equal(r_recs.view(np.uint8), want.view(np.uint8))  # zero records where there is no reply
    off = np.zeros(mixed.n + 1, dtype=np.int64)
    off[1:] = np.cumsum(T)
    assert np.array_equal(r_offsets, off)
    # the whole chain in one call: the same offsets, and the images
    dst, ro, out, fl, ep2 = batch.echo_datagrams(mixed.data, mixed.offs, mixed.table, mixed.m, need=need,
                                                 ep_echo=mixed.echo_t if echo else None)
    torch.cuda.synchronize(dev)
    assert np.array_equal(ro.cpu().numpy(), off) and np.array_equal(ep2.cpu().numpy(), ep)
    assert np.array_equal(fl.cpu().numpy(), flags)
    ans = np.flatnonzero(icmp | udp)
    base = mixed.data.data_ptr()
    host = mixed.data.cpu().numpy()
    pays = [host[int(views[i, 0]) - base:int(views[i, 0]) - base + int(views[i, 1])] for i in ans]
    imgs, vals = expected(want[ans], pays, oracle_c)  # the header encoder; both fields by the oracle's TX_DATAGRAM
    got = replies(dst, ro)
    assert [got[i] for i in ans] == [bytes(x) for x in imgs]
    assert all(len(got[i]) == 0 for i in np.flatnonzero(~(icmp | udp)))
    o = out.cpu().numpy().reshape(mixed.n, 2)
    assert np.array_equal(o[ans].reshape(-1), vals) and (o[~(icmp | udp)] == 0).all()
    # VERIFY_RX accepts every reply (the empty entries are left out of this batch)
    tight = torch.from_numpy(np.concatenate((off[ans], off[-1:]))).to(dev)
    rx = batch.checksum_ragged(dst, tight, "verify_rx").cpu().numpy()
    assert (rx == ACCEPTED).all()
    if need == 0 and not echo:
        # each bit of `what` alone
        for what, mask in ((1, icmp), (2, udp), (0, np.zeros_like(icmp))):
            r = mixed.stages(need, echo, what)
            assert np.array_equal(r[5][1:] - r[5][:-1], np.where(mask, T, 0)), what


# ---- 4. the seams ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 2047, 2048, 2049))
def test_seams(dev, mixed, n):
    h = mixed.head(n)
    recs, views, flags, ep, r_recs, r_offsets = h.stages(OK_BITS, True)
    _, want, T, _, _ = h.restated(recs, views, flags, OK_BITS, True)
    assert np.array_equal(r_recs.view(np.uint8), want.view(np.uint8))
    assert r_offsets[0] == 0 and np.array_equal(r_offsets[1:], np.cumsum(T))
    # r_offsets pre-filled: every entry is stored, r_offsets[0] at n == 0 too
    ro = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    dev_recs, dev_views, dev_flags = batch.parse_datagrams(h.data, h.offs, verify=True)
    dev_ep, _ = batch.demux_datagrams(dev_recs, h.table, h.m, flags=dev_flags, need=OK_BITS)
    batch.reply_datagrams(dev_recs, dev_views, dev_ep, h.m, flags=dev_flags, need=OK_BITS, ep_echo=h.echo_t,
                          r_offsets=ro)
    assert np.array_equal(ro.cpu().numpy(), r_offsets)
    dst, ro2, out, _, _ = batch.echo_datagrams(h.data, h.offs, h.table, h.m, need=OK_BITS, ep_echo=h.echo_t)
    assert np.array_equal(ro2.cpu().numpy(), r_offsets) and out.numel() == 2 * n


# ---- 5. writes ------------------------------------------------------------------------------------------
def test_inputs_unchanged_and_workspace_bounded(dev, mixed):
    h = mixed.head(2049)
    n = h.n
    recs, views, flags = batch.parse_datagrams(h.data, h.offs, verify=True)
    ep, _ = batch.demux_datagrams(recs, h.table, h.m, flags=flags, need=0)
    torch.cuda.synchronize(dev)
    before = [t.clone() for t in (recs, views, flags, ep, h.data, h.echo_t)]
    need_bytes = batch.reply_workspace_bytes(n)
    assert need_bytes == 16  # two tile sums of the scan over n + 1 = 2050 outputs: every byte of it is used
    G = 256
    wbuf = torch.full((G + need_bytes + G,), 0xA5, dtype=torch.uint8, device=dev)
    rbuf = torch.full((G + 32 * n + G,), 0xA5, dtype=torch.uint8, device=dev)
    obuf = torch.full((G // 8 + n + 1 + G // 8,), -1, dtype=torch.int64, device=dev)
    assert wbuf.data_ptr() % 16 == 0
    r_recs, r_offsets = batch.reply_datagrams(recs, views, ep, h.m, flags=flags, ep_echo=h.echo_t,
                                              r_records=rbuf[G:G + 32 * n].view(n, 32),
                                              r_offsets=obuf[G // 8:G // 8 + n + 1], work=wbuf[G:G + need_bytes])
    dst = torch.full((h.data.numel() + 2 * G,), 0xA5, dtype=torch.uint8, device=dev)
    batch.build_datagrams_iov(views, r_recs, r_offsets, dst[G:-G])
    torch.cuda.synchronize(dev)
    for t, b in zip((recs, views, flags, ep, h.data, h.echo_t), before):
        assert torch.equal(t, b)
    for buf in (wbuf, rbuf, dst):
        assert (buf[:G] == 0xA5).all() and (buf[-G:] == 0xA5).all()
    assert (obuf[:G // 8] == -1).all() and (obuf[-(G // 8):] == -1).all()
    total = int(r_offsets[-1])
    assert 0 < total <= h.data.numel() and (dst[G + total:] == 0xA5).all()  # nothing past the last reply
    want = h.stages(0, True)
    assert np.array_equal(r_offsets.cpu().numpy(), want[5])
    assert np.array_equal(packets.rx_records(r_recs).view(np.uint8), want[4].view(np.uint8))


# ---- 6. one graph ---------------------------------------------------------------------------------------
def test_four_calls_captured_as_one_graph(dev, mixed):
    one, two = mixed.head(700), Mixed(dev, 19006, 700)
    two.ids, two.table, two.m, two.echo, two.echo_t = one.ids, one.table, one.m, one.echo, one.echo_t
    n = 700
    size = max(one.data.numel(), two.data.numel())
    data = torch.zeros(size, dtype=torch.uint8, device=dev)
    offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    recs, views = torch.zeros((n, 32), **u8), torch.zeros((n, 2), dtype=torch.int64, device=dev)
    flags, ep = torch.zeros(n, dtype=torch.uint16, device=dev), torch.zeros(n, dtype=torch.uint32, device=dev)
    counts = torch.zeros(one.m + 1, dtype=torch.uint32, device=dev)
    r_recs, r_offsets = torch.zeros((n, 32), **u8), torch.zeros(n + 1, dtype=torch.int64, device=dev)
    work = torch.zeros(batch.reply_workspace_bytes(n), **u8)
    dst, out = torch.zeros(size, **u8), torch.zeros(2 * n, dtype=torch.uint16, device=dev)

    def load(b):
        data[:b.data.numel()] = b.data
        offs.copy_(b.offs)

    def calls():
        batch.parse_datagrams(data, offs, verify=True, records=recs, views=views, out=flags)
        batch.demux_datagrams(recs, one.table, one.m, flags=flags, need=OK_BITS, ep=ep, counts=counts)
        batch.reply_datagrams(recs, views, ep, one.m, flags=flags, need=OK_BITS, ep_echo=one.echo_t,
                              r_records=r_recs, r_offsets=r_offsets, work=work)
        batch.build_datagrams_iov(views, r_recs, r_offsets, dst, out=out)

    def check(b):
        want_dst, want_ro, want_out, _, _ = batch.echo_datagrams(b.data, b.offs, b.table, b.m, need=OK_BITS,
                                                                 ep_echo=b.echo_t)
        torch.cuda.synchronize(dev)
        total = int(want_ro[-1])
        assert total > 0 and torch.equal(r_offsets, want_ro) and torch.equal(out, want_out)
        assert torch.equal(dst[:total], want_dst[:total])
        return total

    load(one)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        calls()  # warm up
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            calls()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)
    first = check(one)
    load(two)  # the inputs rewritten in place
    dst.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    assert check(two) != first
