"""yu_rx_demux on the MI355X (k_demux): which registered endpoint gets each received
packet, and the per-endpoint counters.

1. hand-built cases (every subset of the three kinds on one port, a connection from
   0.0.0.0:0 beside a listener, one 4-tuple under both protocols, ICMP, protocol 47 and a
   zero record, every need against every flag combination) at n = 1, 63, 64, 65, 257 (the
   lane, wave and block seams);
2. end to end: the 198 datagrams the reference's senders produced and the 110 the Linux
   kernel verified or built go through parse_datagrams and are demultiplexed against a
   table of some of their own 4-tuples, some of their listeners and ids that match
   nothing, with need = 0 and, on a copy with damaged checksums, need = IP_OK | L4_OK;
3. eight ids sharing home slot 15 of 16: the probe chain wraps past the table's end;
4. the counters: a wave holding 1, 2, 3 and 64 distinct endpoints, a wave without any, a
   second call accumulating into the first one's counters, and no counters at all;
5. more records than twice the grid's lanes;
6. out of contract: a table of random bytes, a table without an empty slot and slots
   whose index is at or above m all end cleanly, and a valid table gives exact results
   on the same batch afterwards (well-defined inputs the contract says cannot fault);
7. group=True against numpy's stable argsort, the docstring's pack_iov recipe, and the
   grouping on a side stream that is still busy when the call returns;
8. the C call with recs 8 bytes off a 16-byte boundary, and a graph capture and replay.

The expected values come from tests/demux_ref.py, the reference's three map lookups
restated (not executed). ep and counts sit between 256-byte guards of 0xA5 that are
checked after every call. Every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

import demux_plan
import demux_ref
import rxgen
from test_gpu_rx_split import FIELD_AT, ragged
from yustack_amd import _lib, batch, packets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
NONE = batch.DEMUX_NONE
OK_BITS = batch.RX_IP_OK | batch.RX_L4_OK
A, B, R, S, Z = (10, 0, 0, 1), (10, 0, 0, 2), (192, 168, 1, 7), (192, 168, 1, 8), (0, 0, 0, 0)
ADDRS = (A, B, R, Z)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def guarded(dev, nbytes):
    return torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)


def records(rows, seed=0):
    """TX_RECORD entries of received packets: rows of (proto, local addr, local port,
    remote addr, remote port); what is not part of the key is random."""
    rng = np.random.default_rng(seed)
    n = len(rows)
    return packets.tx_records(n, src=np.array([r[3] for r in rows], dtype=np.uint8).reshape(n, 4),
                              dst=np.array([r[1] for r in rows], dtype=np.uint8).reshape(n, 4),
                              sport=[r[4] for r in rows], dport=[r[2] for r in rows], proto=[r[0] for r in rows],
                              seq=rng.integers(0, 1 << 32, n), ack=rng.integers(0, 1 << 32, n),
                              window=rng.integers(0, 1 << 16, n), flags=rng.integers(0, 256, n),
                              ttl=rng.integers(0, 256, n), ip_id=rng.integers(0, 1 << 16, n))


def ids_of(rows):
    """ENDPOINT_ID entries: rows of (kind, proto, local addr, local port, remote addr, remote port)."""
    m = len(rows)
    return packets.endpoint_ids(m, kind=[r[0] for r in rows], proto=[r[1] for r in rows],
                                local_addr=np.array([r[2] for r in rows], dtype=np.uint8).reshape(m, 4),
                                local_port=[r[3] for r in rows],
                                remote_addr=np.array([r[4] for r in rows], dtype=np.uint8).reshape(m, 4),
                                remote_port=[r[5] for r in rows])


class Run:
    """One call on the device: the records `rshift` (0 or 8) bytes off a 16-byte boundary,
    ep and counts between 0xA5 guards, the counters zeroed unless `counts` carries an
    earlier run's."""

    def __init__(self, dev, recs, table, m, flags=None, need=0, counts=True, rshift=0, via_c=False, launch=True):
        raw = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 32)
        self.n, self.m, self.dev, self.need, self.table = raw.shape[0], m, dev, need, table
        n = self.n
        self.recbuf = torch.zeros(32 * n + 32, dtype=torch.uint8, device=dev)
        self.recs = self.recbuf[rshift:rshift + 32 * n].view(n, 32)
        self.recs.copy_(torch.from_numpy(raw.copy()).to(dev))
        assert self.recs.data_ptr() % 16 == rshift and table.data_ptr() % 16 == 0
        self.flags = None if flags is None else torch.from_numpy(np.asarray(flags, dtype=np.uint16).copy()).to(dev)
        self.epbuf = guarded(dev, 4 * n)
        self.ep = self.epbuf[GUARD:GUARD + 4 * n].view(torch.uint32)
        if isinstance(counts, Run):
            self.cbuf, self.counts = counts.cbuf, counts.counts
        elif counts:
            self.cbuf = guarded(dev, 4 * (m + 1))
            self.cbuf[GUARD:GUARD + 4 * (m + 1)] = 0
            self.counts = self.cbuf[GUARD:GUARD + 4 * (m + 1)].view(torch.uint32)
        else:
            self.cbuf = self.counts = None
        if not launch:
            return
        if via_c or self.counts is None:  # the front end always passes counters
            rc = _lib.lib().yu_rx_demux(self.recs.data_ptr(), None if self.flags is None else self.flags.data_ptr(),
                                        need, n, table.data_ptr(), table.numel(), m, self.ep.data_ptr(),
                                        None if self.counts is None else self.counts.data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream)
            assert rc == _lib.YU_OK
        else:
            got = self.call()
            assert got[0] is self.ep and got[1] is self.counts
        torch.cuda.synchronize(dev)  # raises if the stream did not finish cleanly

    def call(self, **kw):
        return batch.demux_datagrams(self.recs, self.table, self.m, flags=self.flags, need=self.need, ep=self.ep,
                                     counts=self.counts, **kw)

    def results(self):
        n, m = self.n, self.m
        ep = self.epbuf.cpu().numpy()
        assert (ep[:GUARD] == 0xA5).all() and (ep[GUARD + 4 * n:] == 0xA5).all(), "ep: guard written"
        counts = None
        if self.cbuf is not None:
            c = self.cbuf.cpu().numpy()
            assert (c[:GUARD] == 0xA5).all() and (c[GUARD + 4 * (m + 1):] == 0xA5).all(), "counts: guard written"
            counts = c[GUARD:GUARD + 4 * (m + 1)].view(np.uint32)
        return ep[GUARD:GUARD + 4 * n].view(np.uint32), counts

    def check(self, want_ep, want_counts=None):
        ep, counts = self.results()
        bad = np.nonzero(ep != want_ep)[0]
        assert bad.size == 0, f"ep differs at {bad[:8]}: {ep[bad[:8]]} want {want_ep[bad[:8]]}"
        if want_counts is not None:
            assert np.array_equal(counts, want_counts), (counts[:16], want_counts[:16])
        return ep, counts


def checked(dev, ids, recs, flags=None, need=0, **kw):
    """One run against demux_ref; returns the expected (ep, counts)."""
    table, m = batch.demux_table(ids, dev)
    want = demux_ref.demux(ids, recs, flags, need)
    Run(dev, recs, table, m, flags, need, **kw).check(*want)
    return want


# ---- 1. hand-built cases --------------------------------------------------------------------
def hand_cases():
    """(ids, record rows, flags): the ids hold, on ports 8000 .. 8007, every subset of the
    three kinds; on 8100 a connection from 0.0.0.0:0 beside a listener on the address; on
    8200 one 4-tuple under both protocols; on port 0 listeners a zero record would match."""
    ids, rows = [], []
    for sub in range(8):
        port = 8000 + sub
        ids += [(kind, 6, Z if kind == 2 else A, port, R if kind == 0 else Z, 40000 if kind == 0 else 0)
                for kind in range(3) if sub >> kind & 1]
        rows += [(6, A, port, R, 40000), (6, A, port, S, 40000), (6, B, port, R, 40000), (17, A, port, R, 40000)]
    ids += [(0, 6, A, 8100, Z, 0), (1, 6, A, 8100, Z, 0)]
    rows += [(6, A, 8100, Z, 0), (6, A, 8100, R, 40000), (6, A, 8100, Z, 1)]
    ids += [(0, 6, A, 8200, R, 40000), (0, 17, A, 8200, R, 40000)]
    rows += [(6, A, 8200, R, 40000), (17, A, 8200, R, 40000), (6, A, 8200, R, 40001), (6, A, 8201, R, 40000)]
    ids += [(2, 6, Z, 0, Z, 0), (2, 17, Z, 0, Z, 0)]
    rows += [(1, A, 0, R, 0x0800), (47, A, 8007, R, 40000), (0, Z, 0, Z, 0), (1, A, 8007, R, 40000)]
    return ids_of(ids), rows


@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_hand_built_cases_at_the_seams(dev, n):
    ids, rows = hand_cases()
    recs = records([rows[(i + n) % len(rows)] for i in range(n)], seed=n)
    zero = [i for i in range(n) if rows[(i + n) % len(rows)][0] == 0]
    recs.view(np.uint8).reshape(n, 32)[zero] = 0  # the record of a packet without YU_RX_SPLIT
    want, _ = checked(dev, ids, recs)
    if n >= 63:
        hit = want[want != NONE]
        assert set(ids["kind"][hit].tolist()) == {0, 1, 2} and (want == NONE).sum() >= 10
        conn0 = int(np.flatnonzero((ids["local_port"] == 8100) & (ids["kind"] == 0))[0])
        for i in range(n):  # the connection from 0.0.0.0:0 and the listener each catch only their own packets
            row = rows[(i + n) % len(rows)]
            if row[2] == 8100:
                assert want[i] == (conn0 if row[3:] == (Z, 0) else conn0 + 1)
    # every need against every flag combination, the flags cycling over the records
    for need in range(8):
        flags = (np.arange(n) * 7 + need) % 32
        got, _ = checked(dev, ids, recs, flags.astype(np.uint16), need)
        passing = (flags & (need | 16)) == (need | 16)
        assert (got[~passing] == NONE).all() and np.array_equal(got[passing], want[passing])
    checked(dev, ids, recs, np.full(n, 0xFFFF, dtype=np.uint16), 0xFFEF)   # every bit asked for and present
    assert (checked(dev, ids, recs, np.full(n, 0xFFEF, dtype=np.uint16), 0)[0] == NONE).all()  # no YU_RX_SPLIT


# ---- 2. end to end --------------------------------------------------------------------------
def fixture_datagrams():
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
    f = np.load(os.path.join(ROOT, "tests", "golden", "kernel_verified.npz"))
    more = [bytes(b[int(s):int(e)]) for b, o in ((f["sent_blob"], f["sent_offs"]), (f["kernel_blob"], f["kernel_offs"]))
            for s, e in zip(o[:-1], o[1:])]
    assert len(more) == 110
    return pkts + more


def table_from(recs, rng, strangers=20):
    """Ids out of received records: every third distinct 4-tuple as a connection, every
    second distinct local pair as a listener on the address, every second distinct port as
    a listener on the port, and `strangers` ids no record matches."""
    l4 = recs[(recs["proto"] == 6) | (recs["proto"] == 17)]
    tup = sorted({(int(r["proto"]), tuple(r["dst"]), int(r["dport"]), tuple(r["src"]), int(r["sport"])) for r in l4})
    pair = sorted({t[:3] for t in tup})
    port = sorted({(t[0], t[2]) for t in tup})
    rows = [(0, p, la, lp, ra, rp) for p, la, lp, ra, rp in tup[::3]]
    rows += [(1, p, la, lp, Z, 0) for p, la, lp in pair[1::2]]
    rows += [(2, p, Z, lp, Z, 0) for p, lp in port[::2]]
    rows += [(0, 6, (172, 16, 0, k), 50000 + k, (172, 16, 1, k), k) for k in range(strangers)]
    return ids_of([rows[i] for i in rng.permutation(len(rows))])


def parse(dev, pkts):
    blob, offs = ragged(pkts)
    recs, _, out = batch.parse_datagrams(torch.from_numpy(blob).to(dev),
                                         torch.from_numpy(offs.astype(np.int64)).to(dev), verify=True)
    torch.cuda.synchronize(dev)
    return packets.rx_records(recs), out.cpu().numpy()


def test_end_to_end_on_the_fixture_datagrams(dev):
    pkts = fixture_datagrams()
    recs, flags = parse(dev, pkts)
    assert (flags & batch.RX_SPLIT).all()
    ids = table_from(recs, np.random.default_rng(17002))
    want, counts = checked(dev, ids, recs, flags, 0)
    hit = want[want != NONE]
    assert set(ids["kind"][hit].tolist()) == {0, 1, 2} and (want == NONE).any() and (counts[:-1] == 0).any()
    assert np.array_equal(checked(dev, ids, recs)[0], want)             # no flags array: the same
    assert np.array_equal(checked(dev, ids, recs, flags, OK_BITS)[0], want)  # every checksum verifies
    # a copy with damaged checksums: a receiver that drops on them delivers fewer
    rng = np.random.default_rng(17003)
    hurt = []
    for k, p in enumerate(pkts):
        p = bytearray(p)
        if k % 2:
            hl = (p[0] & 15) * 4
            i = int(rng.integers(hl, len(p))) if k % 4 == 1 and len(p) > hl else 10  # a payload byte, or the IPv4 field
            p[i] ^= 0x40
        hurt.append(bytes(p))
    hurt += [bytes(rxgen.damage(rng, bytearray(p))) for p in pkts[:60]] + [pkts[0][:10]]  # the last one cannot split
    recs, flags = parse(dev, hurt)
    split = (flags & batch.RX_SPLIT) != 0
    assert (split & ((flags & OK_BITS) != OK_BITS)).sum() >= 50 and (~split).any()
    lax, _ = checked(dev, ids, recs, flags, 0)
    strict, _ = checked(dev, ids, recs, flags, OK_BITS)
    assert ((lax != NONE) & (strict == NONE)).sum() >= 20 and (strict != NONE).sum() >= 20
    assert np.array_equal(strict[strict != NONE], lax[strict != NONE])


# ---- 3. the wrapped chain -------------------------------------------------------------------
def test_collision_chain_wraps_past_the_table_end(dev):
    L = _lib.lib()
    ports = []
    for port in range(1, 65536):
        one = ids_of([(2, 6, Z, port, Z, 0)])
        if L.yu_demux_hash(one.ctypes.data) & 15 == 15:
            ports.append(port)
            if len(ports) == 9:
                break
    ids = ids_of([(2, 6, Z, p, Z, 0) for p in ports[:8]])
    table, m = batch.demux_table(ids, dev)
    tags = table.cpu().numpy().view(np.uint32).reshape(16, 4)[:, 3]
    assert m == 8 and [int(t) >> 8 for t in tags[[15, 0, 1, 2, 3, 4, 5, 6]]] == list(range(8)) and not tags[7:15].any()
    recs = records([(6, A, p, R, 40000 + k) for k, p in enumerate(ports)] + [(17, A, ports[0], R, 40000)])
    want = np.array(list(range(8)) + [NONE, NONE], dtype=np.uint32)
    assert np.array_equal(demux_ref.demux(ids, recs)[0], want)
    Run(dev, recs, table, m).check(want, np.array([1] * 8 + [2], dtype=np.uint32))


# ---- 4. the counters ------------------------------------------------------------------------
def test_counters_of_one_wave(dev):
    ids = ids_of([(2, 17, Z, 1000 + k, Z, 0) for k in range(64)])
    table, m = batch.demux_table(ids, dev)
    for distinct in (1, 2, 3, 64):
        recs = records([(17, A, 1000 + (5 * i) % distinct, R, i) for i in range(64)], seed=distinct)
        want_ep, want_counts = demux_ref.demux(ids, recs)
        assert (want_counts != 0).sum() == distinct and want_counts[m] == 0 and want_counts.sum() == 64
        first = Run(dev, recs, table, m)
        first.check(want_ep, want_counts)
        Run(dev, recs, table, m, counts=first).check(want_ep, 2 * want_counts)   # the call adds
        Run(dev, recs[:37], table, m, counts=first).check(want_ep[:37], 2 * want_counts +
                                                          demux_ref.demux(ids, recs[:37])[1])
        ep, counts = Run(dev, recs, table, m, counts=False).check(want_ep)        # ep_count == NULL
        assert counts is None
    nobody = records([(17, A, 2000 + i, R, i) for i in range(64)])
    Run(dev, nobody, table, m).check(np.full(64, NONE, dtype=np.uint32),
                                     np.array([0] * 64 + [64], dtype=np.uint32))
    mixed = records([(17, A, 1000 + i if i % 3 else 3000, R, i) for i in range(64)])  # endpoints and none in one wave
    Run(dev, mixed, table, m).check(*demux_ref.demux(ids, mixed))


# ---- 5. grid stride, and 6. out of contract -------------------------------------------------
def pool_ids(rng, m):
    rows, seen = [], set()
    while len(rows) < m:
        kind, proto = int(rng.integers(0, 3)), (6, 17)[int(rng.integers(0, 2))]
        row = (kind, proto, Z if kind == 2 else ADDRS[int(rng.integers(0, 4))], 1000 + int(rng.integers(0, 200)),
               ADDRS[int(rng.integers(0, 4))] if kind == 0 else Z, int(rng.integers(0, 8)) if kind == 0 else 0)
        if row not in seen:
            seen.add(row)
            rows.append(row)
    return ids_of(rows)


def pool_records(rng, n):
    protos = (6, 17, 6, 17, 6, 1, 47)
    return records([(protos[int(rng.integers(0, 7))], ADDRS[int(rng.integers(0, 4))], 1000 + int(rng.integers(0, 210)),
                     ADDRS[int(rng.integers(0, 4))], int(rng.integers(0, 9))) for _ in range(n)], seed=n)


@pytest.fixture(scope="module")
def pool():
    """1000 ids and 4099 records from small pools, their flags, and what the restatement
    gives for them with need = IP_OK | L4_OK: computed once."""
    rng = np.random.default_rng(17005)
    ids, recs = pool_ids(rng, 1000), pool_records(rng, 4099)
    flags = np.where(rng.random(4099) < 0.8, 0x17, rng.integers(0, 32, 4099)).astype(np.uint16)
    ep, counts = demux_ref.demux(ids, recs, flags, OK_BITS)
    hit = ep[ep != NONE]
    assert set(ids["kind"][hit].tolist()) == {0, 1, 2} and 1000 < hit.size < 3500
    return ids, recs, flags, ep, counts


def test_more_records_than_twice_the_lanes(dev, pool):
    """2 x blocks x 256 + 5 records, where blocks is yu::plan_demux's cap for this device:
    every lane takes more than one record. The batch is the 4099 seeded records repeated
    (4099 is odd, so a repeat lands on other lanes); a record's result depends on itself
    only, so the expected values repeat too."""
    ids, recs, flags, ep, _ = pool
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    (_, blocks, name), = demux_plan.plans([(1 << 26, cus)])
    assert name == "k_demux" and blocks == 8 * cus
    n = 2 * blocks * 256 + 5
    reps = -(-n // 4099)
    big, big_flags, want = np.tile(recs, reps)[:n], np.tile(flags, reps)[:n], np.tile(ep, reps)[:n]
    counts = np.bincount(np.where(want == NONE, 1000, want).astype(np.int64), minlength=1001).astype(np.uint32)
    table, m = batch.demux_table(ids, dev)
    Run(dev, big, table, m, big_flags, OK_BITS).check(want, counts)


def test_tables_out_of_contract_end_cleanly(dev, pool):
    """Contents yu_demux_table_fill did not write: ep and the counters are unspecified but
    lie in range (an endpoint below m or none; the counters add up to n), the guards are
    intact and the stream finishes. The valid table then gives the exact results."""
    ids, recs, flags, ep, counts = pool
    table, m = batch.demux_table(ids, dev)
    host = table.cpu().numpy()
    rng = np.random.default_rng(17006)
    noise = rng.integers(0, 256, host.size, dtype=np.uint8)
    full = host.copy().view(np.uint32).reshape(-1, 4)
    empty = full[:, 3] == 0
    full[empty] = rng.integers(1, 1 << 32, (int(empty.sum()), 4), dtype=np.uint32) | 0x80  # no code has bit 7
    for other in (noise, full.view(np.uint8).reshape(-1)):
        r = Run(dev, recs, torch.from_numpy(other.copy()).to(dev), m, flags, OK_BITS)
        got_ep, got_counts = r.results()
        assert ((got_ep < m) | (got_ep == NONE)).all() and int(got_counts.sum()) == r.n
        assert np.array_equal(got_counts, np.bincount(np.where(got_ep == NONE, m, got_ep).astype(np.int64),
                                                      minlength=m + 1))
    r.check(ep, counts)  # the full table still holds every id: the bound only ends the misses
    # indices at or above m: the even endpoints' slots get index + m, or 2^24 - 1
    moved = host.copy().view(np.uint32).reshape(-1, 4)
    index, code = moved[:, 3] >> 8, moved[:, 3] & 0xFF
    even = (moved[:, 3] != 0) & (index % 2 == 0)
    moved[even, 3] = np.where(index[even] % 4 == 0, index[even] + m, (1 << 24) - 1) << 8 | code[even]
    want = np.where((ep != NONE) & (ep % 2 == 0), NONE, ep).astype(np.uint32)
    Run(dev, recs, torch.from_numpy(moved.view(np.uint8).reshape(-1).copy()).to(dev), m, flags, OK_BITS).check(
        want, np.bincount(np.where(want == NONE, m, want).astype(np.int64), minlength=m + 1).astype(np.uint32))
    Run(dev, recs, table, m, flags, OK_BITS).check(ep, counts)


# ---- 7. grouping ----------------------------------------------------------------------------
def test_grouping_and_the_gather_recipe(dev):
    rng = np.random.default_rng(17007)
    blob, offs = rxgen.rx_batch(rng, 300, 0, 300, bad=0.3)
    data = torch.from_numpy(blob).to(dev)
    recs_t, views, out = batch.parse_datagrams(data, torch.from_numpy(offs.astype(np.int64)).to(dev), verify=False)
    recs = packets.rx_records(recs_t)
    # few addresses, so that endpoints get several packets each
    recs["dst"], recs["src"] = [ADDRS[i % 2] for i in range(300)], [ADDRS[2 + i % 2] for i in range(300)]
    recs["dport"], recs["sport"] = np.arange(300) % 5 + 80, np.arange(300) % 3
    ids = table_from(recs, rng, strangers=5)
    table, m = batch.demux_table(ids, dev)
    recs_t = torch.from_numpy(recs.view(np.uint8).reshape(300, 32).copy()).to(dev)
    ep, counts, order, first = batch.demux_datagrams(recs_t, table, m, flags=out, group=True)
    torch.cuda.synchronize(dev)
    want_ep, want_counts = demux_ref.demux(ids, recs, out.cpu().numpy(), 0)
    assert np.array_equal(ep.cpu().numpy(), want_ep) and np.array_equal(counts.cpu().numpy(), want_counts)
    key = np.where(want_ep == NONE, m, want_ep).astype(np.int64)
    assert np.array_equal(order.cpu().numpy(), np.argsort(key, kind="stable"))
    want_first = np.zeros(m + 2, dtype=np.int64)
    want_first[1:] = np.cumsum(want_counts)
    assert np.array_equal(first.cpu().numpy(), want_first) and want_first[-1] == 300
    assert (want_counts[:m] >= 3).sum() >= 5 and want_counts[m] > 0
    # the docstring's recipe
    sel = order[:first[m]]
    k = sel.numel()
    vl = views[sel, 1].contiguous()
    do = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    do[1:] = vl.cumsum(0)
    _, dst, _ = batch.pack_iov([data], torch.zeros_like(vl), (views[sel, 0] - data.data_ptr()).contiguous(), vl,
                               torch.arange(k + 1, device=dev), "raw", dst_offsets=do)
    torch.cuda.synchronize(dev)
    dst, do, v = dst.cpu().numpy(), do.cpu().numpy(), views.cpu().numpy()
    at = v[:, 0] - data.data_ptr()
    for e in range(m):
        mine = np.flatnonzero(want_ep == e)  # arrival order
        queue = np.concatenate([blob[at[i]:at[i] + v[i, 1]] for i in mine]) if mine.size else np.zeros(0, np.uint8)
        assert np.array_equal(dst[do[want_first[e]]:do[want_first[e + 1]]], queue), e
    assert do[-1] == dst.size > 5000


def test_grouping_on_a_side_stream(dev, pool):
    """group=True with stream=s: the kernel runs on s, behind work already queued there,
    and the sort and the exclusive sum must run behind the kernel, not on the current
    stream, where ep (preset to none) and the counters (zero) are not written yet."""
    ids, recs, flags, ep, counts = pool
    table, m = batch.demux_table(ids, dev)
    r = Run(dev, recs, table, m, flags, OK_BITS, launch=False)
    r.epbuf[GUARD:GUARD + 4 * r.n] = 0xFF
    busy = torch.rand((4096, 4096), device=dev) / 4096
    s = torch.cuda.Stream(dev)
    for queued in (False, True):  # the first round only warms the allocator and the GEMM, so the second never
        torch.cuda.synchronize(dev)  # makes the host wait
        with torch.cuda.stream(s):
            x = busy
            for _ in range(20):
                x = x @ busy  # queued: keeps s occupied while the host runs on
    assert queued and not s.query()  # s is still at work when the call is made
    with torch.cuda.stream(torch.cuda.Stream(dev)):  # the caller's current stream: not the null stream, which may
        got = r.call(group=True, stream=s)           # wait for every other stream by itself
    assert got[0] is r.ep and got[1] is r.counts
    s.synchronize()
    order, first = got[2].cpu().numpy(), got[3].cpu().numpy()
    r.check(ep, counts)
    key = np.where(ep == NONE, m, ep).astype(np.int64)
    assert np.array_equal(order, np.argsort(key, kind="stable"))
    assert first[0] == 0 and np.array_equal(first[1:], np.cumsum(counts.astype(np.int64)))


# ---- 8. the C call and a graph --------------------------------------------------------------
def test_c_call_with_records_off_a_16_byte_boundary(dev, pool):
    ids, recs, flags, ep, counts = pool
    table, m = batch.demux_table(ids, dev)
    Run(dev, recs, table, m, flags, OK_BITS, rshift=8, via_c=True).check(ep, counts)
    lax = demux_ref.demux(ids, recs[:130])
    Run(dev, recs[:130], table, m, None, 0, rshift=8, via_c=True).check(*lax)
    Run(dev, recs[:130], table, m, None, 0, counts=False, via_c=True).check(lax[0])


def test_graph_capture_and_replay(dev, pool):
    ids, recs, flags, ep, counts = pool
    table, m = batch.demux_table(ids, dev)
    r = Run(dev, recs, table, m, flags, OK_BITS, launch=False)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        r.call()  # warm up
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            r.call()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)
    r.check(ep, counts)  # capturing launches nothing
    r.epbuf.fill_(0xA5)
    g.replay()
    torch.cuda.synchronize(dev)
    r.check(ep, 2 * counts)
