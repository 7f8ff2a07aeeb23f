"""yu_tx_build_iov on the MI355X ("k_build<4,iov>"): outgoing IPv4 datagrams built straight
from payload views.

1. differential against yu_tx_build_ragged: the same records and payloads, the payloads
   left scattered behind views, at every payload and destination byte phase, inside 0xA5
   guards with a leading gap and slack: dst and out identical;
2. skipped packets (an empty destination span) between built ones, their views {0, 0} or
   valid memory whose contents would show in the result if it were read;
3. one view named by three packets;
4. T = 65535, and an over-limit view confined to its own span;
5. the C call with out == NULL.

Every pointer is valid device memory and every comparison is exact. The contiguous
builder itself is held against the reference and the oracle in test_gpu_tx_build.py."""
import numpy as np
import pytest
import torch

from test_gpu_tx_build import GUARD, Placed, random_records
from yustack_amd import _lib, batch

pytestmark = pytest.mark.gpu

H_OF = {6: 20, 17: 8, 1: 4}
LENGTHS = list(range(0, 6)) + list(range(1019, 1026)) + list(range(4091, 4098))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Scattered:
    """The payloads in one pool in reverse order with filler between them, payload i at
    byte phase (pphase + i) % 4; `views` is the (n, 2) int64 table onto them."""

    def __init__(self, dev, rng, pays, pphase=0):
        parts, at, where = [], 0, [0] * len(pays)
        for i in reversed(range(len(pays))):
            pad = 4 + (pphase + i - at) % 4 + 4 * int(rng.integers(0, 3))
            pad += (pphase + i - (at + pad)) % 4
            parts.append(rng.integers(1, 256, pad, dtype=np.uint8))
            at += pad
            where[i] = at
            parts.append(pays[i])
            at += len(pays[i])
        parts.append(rng.integers(1, 256, 8, dtype=np.uint8))
        self.host = np.concatenate(parts)
        self.pool = torch.from_numpy(self.host).to(dev)
        assert self.pool.data_ptr() % 4 == 0
        v = np.array([[self.pool.data_ptr() + w, len(p)] for w, p in zip(where, pays)], dtype=np.int64).reshape(-1, 2)
        assert all((int(a) % 4) == (pphase + i) % 4 for i, a in enumerate(v[:, 0]))
        self.views_host = v
        self.views = torch.from_numpy(v).to(dev)


def rooms(recs, pays, slack=None):
    r = np.array([20 + H_OF.get(int(x["proto"]), 0) + len(p) for x, p in zip(recs, pays)], dtype=np.int64)
    return r if slack is None else r + slack


def both(dev, rng, recs, pays, room, pphase, dphase, lead):
    """The contiguous call and the view call over the same records, payloads and layout:
    (reference Placed, its out, view-call Placed, its out, the scattered pool)."""
    ref = Placed(dev, recs, pays, room, pphase, dphase, lead)
    _, _, want = batch.build_datagrams(ref.payload, ref.po, ref.recs, dst=ref.dst, dst_offsets=ref.do)
    got = Placed(dev, recs, pays, room, pphase, dphase, lead)
    sc = Scattered(dev, rng, pays, pphase)
    _, _, out = batch.build_datagrams_iov(sc.views, got.recs, got.do, got.dst)
    torch.cuda.synchronize(dev)
    assert np.array_equal(sc.pool.cpu().numpy(), sc.host), "a view was written"
    return ref, want, got, out, sc


# ---- 1. differential ------------------------------------------------------------------------
@pytest.mark.parametrize("pphase", range(4))
def test_identical_to_the_contiguous_builder(dev, pphase):
    rng = np.random.default_rng(1900 + pphase)
    for dphase in range(4):
        lens = np.array(LENGTHS + [int(x) for x in rng.integers(0, 131, 50)])
        rng.shuffle(lens)
        n = len(lens)
        recs = random_records(rng, n, lens)
        pays = [rng.integers(0, 256, int(L), dtype=np.uint8) for L in lens]
        room = rooms(recs, pays, rng.integers(0, 8, n))
        ref, want, got, out, _ = both(dev, rng, recs, pays, room, pphase, dphase, lead=13)
        assert torch.equal(got.buf, ref.buf), (pphase, dphase)
        assert torch.equal(out, want), (pphase, dphase)
        assert (want.cpu().numpy().reshape(n, 2)[:, 0] != 0).any()  # the reference call was in contract
    assert batch.build_iov_variant(n) == "k_build<4,iov>"


# ---- 2. skipped packets ----------------------------------------------------------------------
@pytest.mark.parametrize("null_views", (True, False))
def test_skipped_packets_store_nothing(dev, null_views):
    rng = np.random.default_rng(1902 + null_views)
    n = 150
    lens = rng.choice(np.array(LENGTHS + list(range(6, 131))), n)
    recs = random_records(rng, n, lens)
    pays = [rng.integers(0, 256, int(L), dtype=np.uint8) for L in lens]
    skip = rng.random(n) < 0.4
    skip[[0, 1, 64, n - 1]] = True   # the first two, a wave's first and the last
    skip[[2, 63, 65, n - 2]] = False
    room = np.where(skip, 0, rooms(recs, pays, rng.integers(0, 5, n)))
    keep = np.flatnonzero(~skip)
    # the contiguous call over the packets that are built, at the same offsets
    ref = Placed(dev, recs[keep], [pays[i] for i in keep], room[keep], pphase=1, dphase=2, lead=7)
    _, _, want = batch.build_datagrams(ref.payload, ref.po, ref.recs, dst=ref.dst, dst_offsets=ref.do)
    got = Placed(dev, recs, pays, room, pphase=1, dphase=2, lead=7)
    assert got.size == ref.size
    sc = Scattered(dev, rng, pays, pphase=1)
    views = sc.views.clone()
    if null_views:
        views[torch.from_numpy(skip).to(dev)] = 0
    else:
        assert all(len(pays[i]) == 0 or sc.host[sc.views_host[i, 0] - sc.pool.data_ptr()] == pays[i][0]
                   for i in np.flatnonzero(skip))  # a skipped view points at its payload: valid memory
    out = torch.full((2 * n,), 0xA5A5, dtype=torch.uint16, device=dev)
    batch.build_datagrams_iov(views, got.recs, got.do, got.dst, out=out)
    torch.cuda.synchronize(dev)
    assert torch.equal(got.buf, ref.buf)  # guards, gap, slack and neighbours included
    o = out.cpu().numpy().reshape(n, 2)
    assert np.array_equal(o[keep].reshape(-1), want.cpu().numpy())
    assert (o[skip] == 0).all()


# ---- 3. one view, three packets ----------------------------------------------------------------
def test_three_packets_name_one_view(dev):
    rng = np.random.default_rng(1903)
    L = 1021
    pay = rng.integers(0, 256, L, dtype=np.uint8)
    recs = random_records(rng, 5, [L] * 5, protos=(17, 1, 6))
    pays = [pay, rng.integers(0, 256, 40, dtype=np.uint8), pay, pay, rng.integers(0, 256, 3, dtype=np.uint8)]
    room = rooms(recs, pays)
    ref = Placed(dev, recs, pays, room, pphase=3, dphase=1, lead=3)
    _, _, want = batch.build_datagrams(ref.payload, ref.po, ref.recs, dst=ref.dst, dst_offsets=ref.do)
    got = Placed(dev, recs, pays, room, pphase=3, dphase=1, lead=3)
    sc = Scattered(dev, rng, pays, pphase=3)
    views = sc.views.clone()
    views[2] = views[0]
    views[3] = views[0]
    _, _, out = batch.build_datagrams_iov(views, got.recs, got.do, got.dst)
    assert torch.equal(got.buf, ref.buf) and torch.equal(out, want)


# ---- 4. the limit --------------------------------------------------------------------------------
def test_the_largest_datagram_and_an_over_limit_view(dev):
    rng = np.random.default_rng(1904)
    lens = [700, 65507, 33, 65508, 9]
    recs = random_records(rng, 5, lens, protos=(17,))
    pays = [rng.integers(0, 256, L, dtype=np.uint8) for L in lens]
    room = rooms(recs, pays)
    assert room[1] == 65535 and room[3] == 65536
    ref, want, got, out, _ = both(dev, rng, recs, pays, room, pphase=1, dphase=3, lead=5)
    w, o = want.cpu().numpy().reshape(5, 2), out.cpu().numpy().reshape(5, 2)
    good = [0, 1, 2, 4]
    assert np.array_equal(o[good], w[good]) and (w[good, 0] != 0).all()
    assert (o[3] == 0).all()                   # out of contract: the pair is {0, 0}
    a, b = ref.buf.cpu().numpy(), got.buf.cpu().numpy()
    base = got.dst.data_ptr() - got.buf.data_ptr()
    lo, hi = base + int(got.do_host[3]), base + int(got.do_host[4])
    assert np.array_equal(a[:lo], b[:lo]) and np.array_equal(a[hi:], b[hi:])  # T = 65535 exact; neighbours, guards
    assert (b[:GUARD] == 0xA5).all() and (b[-GUARD:] == 0xA5).all()


# ---- 5. out == NULL -------------------------------------------------------------------------------
def test_c_call_without_out(dev):
    rng = np.random.default_rng(1905)
    n = 70
    lens = rng.choice(np.array(LENGTHS + list(range(6, 131))), n)
    recs = random_records(rng, n, lens)
    pays = [rng.integers(0, 256, int(L), dtype=np.uint8) for L in lens]
    room = rooms(recs, pays, rng.integers(0, 8, n))
    room[[5, 66]] = 0
    _, _, got, _, sc = both(dev, rng, recs, pays, room, pphase=2, dphase=0, lead=13)
    first = got.buf.clone()
    assert (first != 0xA5).any()
    got.buf.fill_(0xA5)
    rc = _lib.lib().yu_tx_build_iov(sc.views.data_ptr(), got.recs.data_ptr(), n, got.dst.data_ptr(), got.do.data_ptr(),
                                    None, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == _lib.YU_OK
    torch.cuda.synchronize(dev)
    assert torch.equal(got.buf, first)
