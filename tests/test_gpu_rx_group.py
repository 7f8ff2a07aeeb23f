"""yu_rx_group on the device (include/yucsum.h; the kernels k_group_* of
yustack_amd/csrc/yucsum_kernels.hip): the packet numbers grouped by endpoint, the CSR,
the grouped view table and its offsets, all exact integers.

1. the grid of the CPU model (tests/cpp/rx_group.cpp): n x m x key patterns, and m = 2^24
   once (four passes), against numpy's stable argsort, searchsorted and a gather with a
   cumsum; a batch over 2^23 packets, whose tile is grown;
2. the records of test_gpu_rx_demux.py's grouping case, rebuilt here: order and first equal
   what demux_datagrams(group=True) returns;
3. every output and the workspace (exactly yu_rx_group_workspace_bytes long) between 0xA5
   guards, ep and views unchanged: checked in every call of 1;
4. a second call gives identical bytes: in every call of 1 at two of the sizes;
5. parse, demux, group and pack_iov on one side stream without a host read between them;
6. the same chain captured in a graph and replayed on a second batch;
7. n = 0 stores the empty CSR."""
import numpy as np
import pytest
import torch

import demux_ref
import rxgen
from yustack_amd import _lib, batch, packets

pytestmark = pytest.mark.gpu

GUARD = 256
NONE = batch.DEMUX_NONE
TILE = 1024
NS = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 9 * TILE - 27)
A, B, R, S, Z = (10, 0, 0, 1), (10, 0, 0, 2), (192, 168, 1, 7), (192, 168, 1, 8), (0, 0, 0, 0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def fill(rng, n, m, pattern):
    """The key patterns of tests/cpp/rx_group.cpp."""
    bits = int(m).bit_length()
    if pattern == 0:
        ep = np.full(n, max(m - 1, 0))                                   # all equal
    elif pattern == 1:
        ep = np.full(n, NONE)                                            # all none
    elif pattern == 2:
        ep = np.arange(n)[::-1]                                          # distinct, descending
    elif pattern == 3:
        ep = (np.arange(n) & 1) << (bits - 1) if bits else np.zeros(n)   # the top digit alone differs
    elif pattern == 4:                                                   # m, m + 1, 0x7FFFFFFF mixed in
        odd = np.stack((np.full(n, m), np.full(n, m + 1), np.full(n, 0x7FFFFFFF), rng.integers(0, max(m, 1), n)))
        ep = odd[rng.integers(0, 4, n), np.arange(n)]
    else:
        ep = rng.integers(0, m + 2, n)                                   # random
    return np.ascontiguousarray(ep).astype(np.uint32)


class Guarded:
    """`nbytes` bytes between two 0xA5 guards, all of it 0xA5 before the call."""

    def __init__(self, dev, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def body(self, dtype):
        return self.buf[GUARD:GUARD + self.nbytes].cpu().numpy().view(dtype)

    def guards_intact(self):
        edge = torch.cat((self.buf[:GUARD], self.buf[GUARD + self.nbytes:]))
        return bool((edge == 0xA5).all())


def expect(ep, m, views=None):
    """(order, first, q_views, q_offsets) from numpy."""
    n = ep.size
    key = np.minimum(ep.astype(np.int64), m)
    order = np.argsort(key, kind="stable")
    first = np.searchsorted(key[order], np.arange(m + 2), side="left")
    if views is None:
        return order, first, None, None
    qv = views[order].copy()
    qv[first[m]:] = 0
    qo = np.zeros(n + 1, dtype=np.uint64)
    qo[1:] = np.cumsum(qv[:, 1].astype(np.uint64), dtype=np.uint64)      # modulo 2^64
    return order, first, qv, qo


class Run:
    """One yu_rx_group call through the C ABI on guarded buffers."""

    def __init__(self, dev, ep, m, views=None):
        self.dev, self.n, self.m, self.ep_host, self.views_host = dev, ep.size, m, ep, views
        n = self.n
        self.ep = torch.from_numpy(ep.view(np.int32).copy()).to(dev)
        self.views = None if views is None else torch.from_numpy(views.copy()).to(dev)
        self.need = batch.group_workspace_bytes(n, m)
        assert self.need > 0 and self.need % 16 == 0
        self.order, self.first = Guarded(dev, 4 * n), Guarded(dev, 8 * (m + 2))
        self.q_views = Guarded(dev, 16 * n) if views is not None else None
        self.q_offsets = Guarded(dev, 8 * (n + 1)) if views is not None else None
        self.work = Guarded(dev, self.need)

    def call(self):
        n, v = self.n, self.views is not None
        rc = _lib.lib().yu_rx_group(self.ep.data_ptr() if n else None, n, self.m,
                                    self.views.data_ptr() if v and n else None, self.order.ptr if n else None,
                                    self.first.ptr, self.q_views.ptr if v and n else None,
                                    self.q_offsets.ptr if v else None, self.work.ptr, self.need,
                                    torch.cuda.current_stream(self.dev).cuda_stream)
        assert rc == _lib.YU_OK, rc
        torch.cuda.synchronize(self.dev)

    def outputs(self):
        out = [self.order.body(np.uint32), self.first.body(np.uint64)]
        if self.views is not None:
            out += [self.q_views.body(np.int64).reshape(-1, 2), self.q_offsets.body(np.uint64)]
        return out

    def check(self):
        got = self.outputs()
        want = expect(self.ep_host, self.m, self.views_host)
        for name, g, w in zip(("order", "first", "q_views", "q_offsets"), got, want):
            assert np.array_equal(g.astype(np.uint64), np.asarray(w).astype(np.uint64)), (name, self.n, self.m)
        assert got[1][0] == 0 and got[1][-1] == self.n
        for b in (self.order, self.first, self.q_views, self.q_offsets, self.work):
            assert b is None or b.guards_intact(), (self.n, self.m)
        assert np.array_equal(self.ep.cpu().numpy().view(np.uint32), self.ep_host)        # the inputs are only read
        assert self.views is None or np.array_equal(self.views.cpu().numpy(), self.views_host)
        return got


def some_views(rng, n):
    """n views as a parser might leave them: any address, lengths up to 1500, some empty."""
    v = np.empty((n, 2), dtype=np.int64)
    v[:, 0] = rng.integers(1 << 20, 1 << 40, n)
    v[:, 1] = rng.integers(0, 1501, n) * (rng.random(n) < 0.9)
    return v


# ---- 1, 3, 4. the model's grid, the guards and the second call ------------------------------
@pytest.mark.parametrize("m", (0, 1, 255, 256, 65535, 65536))
def test_grid_of_the_model(dev, m):
    rng = np.random.default_rng(18000 + m)
    for n in NS:
        for pattern in range(6):
            r = Run(dev, fill(rng, n, m, pattern), m, some_views(rng, n) if pattern != 1 or n == TILE else None)
            r.call()
            got = r.check()
            if n in (65, 2 * TILE + 3):  # once more on the same inputs: the same bytes
                r.call()
                again = r.outputs()
                assert all(np.array_equal(a, b) for a, b in zip(got, again)), (n, m, pattern)
                r.check()


def test_sums_of_lengths_wrap_at_2_to_the_64(dev):
    rng = np.random.default_rng(18001)
    ep = fill(rng, 300, 7, 5)
    views = some_views(rng, 300)
    views[np.flatnonzero(ep < 7)[:3], 1] = -256                          # 2^64 - 256 as an unsigned length
    r = Run(dev, ep, 7, views)
    r.call()
    r.check()


def test_four_passes(dev):
    """m = 2^24: keys of 25 bits, four passes on 7-bit digits, a `first` of 128 MiB."""
    m = 1 << 24
    assert batch.group_variant(300, m) == "k_group<4>"
    rng = np.random.default_rng(18002)
    ep = fill(rng, 300, m, 5)
    ep[:8] = (0, m - 1, m, m + 1, NONE, 0, m - 1, 1 << 23)
    r = Run(dev, ep, m, some_views(rng, 300))
    r.call()
    r.check()


def test_a_grown_tile(dev):
    """Over 2^23 packets a block's tile is 2048 packets: 8 steps per wave."""
    n = (1 << 23) + 4099
    rng = np.random.default_rng(18003)
    ep = rng.integers(0, 5, n).astype(np.uint32)                         # m = 3: keys 0 .. 3, a quarter dropped
    r = Run(dev, ep, 3)
    r.call()
    r.check()


# ---- 2. the grouping case of the demultiplexer's tests --------------------------------------
def ids_of(rows):
    """ENDPOINT_ID entries: rows of (kind, proto, local addr, local port, remote addr, remote port)."""
    m = len(rows)
    return packets.endpoint_ids(m, kind=[r[0] for r in rows], proto=[r[1] for r in rows],
                                local_addr=np.array([r[2] for r in rows], dtype=np.uint8).reshape(m, 4),
                                local_port=[r[3] for r in rows],
                                remote_addr=np.array([r[4] for r in rows], dtype=np.uint8).reshape(m, 4),
                                remote_port=[r[5] for r in rows])


def table_from(recs, rng, strangers):
    """Every third distinct 4-tuple of the records as a connection, every second local pair
    as a listener on the address, every second port as a listener on the port, and ids no
    record matches, shuffled."""
    l4 = recs[(recs["proto"] == 6) | (recs["proto"] == 17)]
    tup = sorted({(int(r["proto"]), tuple(r["dst"]), int(r["dport"]), tuple(r["src"]), int(r["sport"])) for r in l4})
    pair = sorted({t[:3] for t in tup})
    port = sorted({(t[0], t[2]) for t in tup})
    rows = [(0, p, la, lp, ra, rp) for p, la, lp, ra, rp in tup[::3]]
    rows += [(1, p, la, lp, Z, 0) for p, la, lp in pair[1::2]]
    rows += [(2, p, Z, lp, Z, 0) for p, lp in port[::2]]
    rows += [(0, 6, (172, 16, 0, k), 50000 + k, (172, 16, 1, k), k) for k in range(strangers)]
    return ids_of([rows[i] for i in rng.permutation(len(rows))])


def test_equals_the_torch_grouping_of_demux_datagrams(dev):
    rng = np.random.default_rng(17007)
    blob, offs = rxgen.rx_batch(rng, 300, 0, 300, bad=0.3)
    data = torch.from_numpy(blob).to(dev)
    recs_t, views, out = batch.parse_datagrams(data, torch.from_numpy(offs.astype(np.int64)).to(dev), verify=False)
    recs = packets.rx_records(recs_t)
    recs["dst"], recs["src"] = [(A, B, R, Z)[i % 2] for i in range(300)], [(A, B, R, Z)[2 + i % 2] for i in range(300)]
    recs["dport"], recs["sport"] = np.arange(300) % 5 + 80, np.arange(300) % 3
    ids = table_from(recs, rng, strangers=5)
    table, m = batch.demux_table(ids, dev)
    recs_t = torch.from_numpy(recs.view(np.uint8).reshape(300, 32).copy()).to(dev)
    ep, counts, t_order, t_first = batch.demux_datagrams(recs_t, table, m, flags=out, group=True)
    want_ep, want_counts = demux_ref.demux(ids, recs, out.cpu().numpy(), 0)
    assert np.array_equal(ep.cpu().numpy(), want_ep)
    assert (want_counts[:m] >= 3).sum() >= 5 and want_counts[m] > 0
    order, first, q_views, q_offsets = batch.group_datagrams(ep, m, views=views)
    torch.cuda.synchronize(dev)
    assert order.dtype == torch.int32 and first.dtype == torch.int64 and q_offsets.dtype == torch.int64
    assert np.array_equal(order.cpu().numpy(), t_order.cpu().numpy())
    assert np.array_equal(first.cpu().numpy(), t_first.cpu().numpy())
    # both index tensors as they are, and the docstring's recipe of demux_datagrams gives the same table
    sel = order[:first[m]]
    assert np.array_equal(q_views[:sel.numel()].cpu().numpy(), views[sel].cpu().numpy())
    assert not q_views[sel.numel():].any()
    assert np.array_equal(q_offsets[1:sel.numel() + 1].cpu().numpy(), views[sel, 1].cumsum(0).cpu().numpy())
    # without views, buffers given, on a side stream
    s = torch.cuda.Stream(dev)
    o2 = torch.empty(300, dtype=torch.int32, device=dev)
    f2 = torch.empty(m + 2, dtype=torch.int64, device=dev)
    work = torch.empty(batch.group_workspace_bytes(300, m), dtype=torch.uint8, device=dev)
    got = batch.group_datagrams(ep, m, order=o2, first=f2, work=work, stream=s)
    s.synchronize()
    assert len(got) == 2 and got[0].data_ptr() == o2.data_ptr() and got[1].data_ptr() == f2.data_ptr()
    assert torch.equal(o2, order) and torch.equal(f2, first)


# ---- 5, 6. the pipeline without a host read --------------------------------------------------
PIPE_N = 300
PIPE_IDS = ids_of([(0, 6, A, 80, R, 1), (0, 17, A, 80, R, 1), (0, 6, B, 81, S, 2), (1, 6, A, 80, Z, 0),
                   (1, 17, B, 82, Z, 0), (1, 6, B, 84, Z, 0), (2, 6, Z, 83, Z, 0), (2, 17, Z, 83, Z, 0),
                   (2, 17, Z, 81, Z, 0), (0, 6, (172, 16, 0, 1), 50000, (172, 16, 1, 1), 7)])


def pipe_batch(seed):
    """About 300 mixed TCP / UDP / ICMP / other datagrams, a share of them damaged, from
    few addresses and ports, so that endpoints get several packets each. Checksums are not
    kept: the pipeline parses with verify=False and demultiplexes with need = 0."""
    rng = np.random.default_rng(seed)
    blob, offs = rxgen.rx_batch(rng, PIPE_N, 0, 300, bad=0.3)
    blob = blob.copy()
    for i in range(PIPE_N):
        p = blob[int(offs[i]):int(offs[i + 1])]
        hl = 4 * (int(p[0]) & 15) if p.size else 0
        if p.size >= 20:
            p[12:16], p[16:20] = (R, S)[i % 2], (A, B)[(i // 2) % 2]
        if hl >= 20 and p.size >= hl + 4:
            p[hl:hl + 2] = (0, i % 3)                                    # source port 0 .. 2
            p[hl + 2:hl + 4] = (0, 80 + i % 5)                           # destination port 80 .. 84
    return blob, offs.astype(np.int64)


class Pipe:
    """Every buffer of the four calls, allocated once: what a graph needs."""

    def __init__(self, dev, room):
        n, self.dev = PIPE_N, dev
        self.table, self.m = batch.demux_table(PIPE_IDS, dev)
        m = self.m
        u8 = dict(dtype=torch.uint8, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        self.data, self.offs = torch.zeros(room, **u8), torch.zeros(n + 1, **i64)
        self.recs, self.views = torch.zeros((n, 32), **u8), torch.zeros((n, 2), **i64)
        self.out = torch.zeros(n, dtype=torch.uint16, device=dev)
        self.ep = torch.zeros(n, dtype=torch.uint32, device=dev)
        self.counts = torch.zeros(m + 1, dtype=torch.uint32, device=dev)
        self.order, self.first = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(m + 2, **i64)
        self.q_views, self.q_offsets = torch.zeros((n, 2), **i64), torch.zeros(n + 1, **i64)
        self.work = torch.zeros(batch.group_workspace_bytes(n, m), **u8)
        self.iota = torch.arange(n + 1, **i64)
        self.dst = torch.zeros(room, **u8)                               # an upper bound: the batch itself
        self.sums = torch.zeros(n, dtype=torch.uint16, device=dev)

    def load(self, blob, offs):
        self.blob = blob
        self.data[:blob.size] = torch.from_numpy(blob).to(self.dev)
        self.offs.copy_(torch.from_numpy(offs).to(self.dev))
        self.dst.fill_(0xA5)

    def calls(self, stream):
        """The four calls on `stream` (None: the current one); nothing is read back."""
        n, m = PIPE_N, self.m
        batch.parse_datagrams(self.data, self.offs, verify=False, records=self.recs, views=self.views, out=self.out,
                              stream=stream)
        batch.demux_datagrams(self.recs, self.table, m, flags=self.out, ep=self.ep, counts=self.counts, stream=stream)
        batch.group_datagrams(self.ep, m, views=self.views, order=self.order, first=self.first, q_views=self.q_views,
                              q_offsets=self.q_offsets, work=self.work, stream=stream)
        s = stream if stream is not None else torch.cuda.current_stream(self.dev)
        rc = _lib.lib().yu_csum_pack_iov(self.q_views.data_ptr(), self.iota.data_ptr(), n, batch.RAW, None, 0, None,
                                         self.dst.data_ptr(), self.q_offsets.data_ptr(), self.sums.data_ptr(),
                                         s.cuda_stream)
        assert rc == _lib.YU_OK, rc

    def check(self):
        """After one synchronise: every endpoint's byte range of dst is its packets'
        payloads in arrival order."""
        n, m, blob = PIPE_N, self.m, self.blob
        flags = self.out.cpu().numpy()
        recs = packets.rx_records(self.recs)
        want_ep, want_counts = demux_ref.demux(PIPE_IDS, recs, flags, 0)
        assert np.array_equal(self.ep.cpu().numpy(), want_ep)
        assert (want_counts[:m] >= 3).sum() >= 5 and want_counts[m] >= 20 and (flags & batch.RX_SPLIT == 0).any()
        assert {int(p) for p in recs["proto"][want_ep == NONE]} >= {1, 6, 17}         # ICMP, and unregistered ports
        views = self.views.cpu().numpy()
        order, first, qv, qo = expect(want_ep, m, views)
        assert np.array_equal(self.order.cpu().numpy(), order) and np.array_equal(self.first.cpu().numpy(), first)
        assert np.array_equal(self.q_views.cpu().numpy(), qv)
        assert np.array_equal(self.q_offsets.cpu().numpy().view(np.uint64), qo)
        dst, at = self.dst.cpu().numpy(), views[:, 0] - self.data.data_ptr()
        for e in range(m):
            mine = np.flatnonzero(want_ep == e)                          # arrival order
            queue = np.concatenate([blob[at[i]:at[i] + views[i, 1]] for i in mine]) if mine.size else blob[:0]
            assert np.array_equal(dst[int(qo[first[e]]):int(qo[first[e + 1]])], queue), e
        assert int(qo[n]) == int(qo[first[m]]) > 5000 and (dst[int(qo[n]):] == 0xA5).all()
        sums = self.sums.cpu().numpy()
        assert not sums[first[m]:].any()                                 # dropped packets copy, and sum, no byte
        return int(qo[n])


def test_pipeline_on_a_side_stream_without_a_host_read(dev):
    blob, offs = pipe_batch(18005)
    p = Pipe(dev, blob.size + 4096)
    p.load(blob, offs)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    p.calls(s)
    s.synchronize()
    p.check()


def test_pipeline_captured_in_a_graph_and_replayed_on_a_second_batch(dev):
    one, two = pipe_batch(18006), pipe_batch(18007)
    p = Pipe(dev, max(one[0].size, two[0].size) + 4096)
    p.load(*one)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        p.calls(None)  # warm up
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            p.calls(None)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)
    bytes_one = p.check()  # capturing launches nothing: the warm-up's results
    p.load(*two)
    for t in (p.ep, p.order, p.first, p.q_views, p.q_offsets):
        t.view(torch.uint8).fill_(0xA5)
    g.replay()
    torch.cuda.synchronize(dev)
    assert p.check() != bytes_one


# ---- 7. the empty batch ---------------------------------------------------------------------
def test_empty_batch_stores_the_empty_csr(dev):
    ep = torch.empty(0, dtype=torch.uint32, device=dev)
    first = torch.full((7,), -1, dtype=torch.int64, device=dev)
    q_offsets = torch.full((1,), -1, dtype=torch.int64, device=dev)
    got = batch.group_datagrams(ep, 5, views=torch.empty((0, 2), dtype=torch.int64, device=dev), first=first,
                                q_offsets=q_offsets)
    torch.cuda.synchronize(dev)
    assert len(got) == 4 and got[0].numel() == 0 and got[2].numel() == 0
    assert not first.any() and not q_offsets.any()
    order, first = batch.group_datagrams(ep, 70000)                      # no views: first alone
    torch.cuda.synchronize(dev)
    assert order.numel() == 0 and first.shape == (70002,) and not first.any()
    r = Run(dev, np.zeros(0, dtype=np.uint32), 3, np.zeros((0, 2), dtype=np.int64))
    r.call()
    r.check()
