"""One yu_rx_stream call on the device against tests/stream_ref.py, for
tests/test_gpu_rx_stream.py: a batch assembled from endpoints (state, carried heap, queue
of segments), UDP endpoints in state 0 and packets of no endpoint mixed in by a random merge
that keeps each queue's arrival order; every output between guard bytes; every output
compared byte for byte with the model's. A plain module, like seg_seams.py.

Run as a program it walks the case grid once and prints "<variant> <cases> ok": the test of
the forced general step starts it under YU_TUNING=1 YU_STREAM=walk."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import stream_cases as C  # noqa: E402
import stream_ref as R  # noqa: E402
from yustack_amd import batch, packets  # noqa: E402

GUARD = 64


def guarded(shape, dtype, dev):
    """A tensor of `shape` between two guards of 64 bytes of 0xA5, itself filled with 0x5A."""
    count = int(np.prod(shape)) if shape else 1
    item = torch.empty(0, dtype=dtype).element_size()
    raw = torch.full((2 * GUARD + count * item,), 0xA5, dtype=torch.uint8, device=dev)
    raw[GUARD:GUARD + count * item] = 0x5A
    return raw, raw[GUARD:GUARD + count * item].view(dtype).view(shape)


def guards_intact(raw):
    r = raw.cpu().numpy()
    return (r[:GUARD] == 0xA5).all() and (r[-GUARD:] == 0xA5).all()


def run(eps, cap, dev, rng, nobody=0, payload=None):
    """eps: a list of (st, heap, segs) as stream_cases.scenario returns them. Runs the call
    and compares; returns what it stored (numpy) for further checks."""
    m = len(eps)
    owner = [e for e, ep in enumerate(eps) for _ in ep[2]] + [m] * nobody
    left = [len(ep[2]) for ep in eps] + [nobody]
    n = len(owner)
    # a random merge: packet numbers in arrival order, each queue's own order kept
    ep_of = np.empty(n, dtype=np.int64)
    for i in range(n):
        e = int(rng.integers(0, m + 1))
        while left[e] == 0:
            e = (e + 1) % (m + 1)
        left[e] -= 1
        ep_of[i] = e
    order = np.argsort(ep_of, kind="stable").astype(np.int32)
    first = np.searchsorted(ep_of[order], np.arange(m + 2)).astype(np.int64)
    if payload is None:
        payload = torch.zeros(16, dtype=torch.uint8, device=dev)  # addresses only: no payload byte is read
    origin = payload.data_ptr()
    recs = packets.tx_records(max(n, 1), proto=17)[:n]
    views = np.zeros((n, 2), dtype=np.int64)
    queues = []
    for e, (st, heap, segs) in enumerate(eps):
        pk = np.flatnonzero(ep_of == e)
        q = C.place(segs, pk, origin)
        queues.append(q)
        for s in q:
            r = recs[s["pkt"]]
            r["proto"], r["doff"], r["flags"], r["seq"] = s["proto"], s["doff"], s["flags"], s["seq"]
            r["ack"], r["window"] = 7, 1000
            views[s["pkt"]] = (s["base"], s["vlen"])
    st_in = np.zeros(m, dtype=packets.TCP_RCV)
    heap_in = np.zeros(m * cap, dtype=packets.TCP_SEG)
    heaps = []
    for e, (st, heap, segs) in enumerate(eps):
        for k in R.ST_FIELDS:
            st_in[e][k] = st[k]
        st_in[e]["reserved"] = 0x1234 + e
        h = [dict(t, base=t["base"] + origin) for t in heap]
        heaps.append(h)
        for i, t in enumerate(h):
            x = heap_in[e * cap + i]
            x["base"], x["len"], x["seq"], x["pkt"], x["flags"] = t["base"], t["len"], t["seq"], t["pkt"], t["flags"]
    ids = packets.endpoint_ids(max(m, 1), local_addr=[10, 0, 0, 1], local_port=80, proto=6)[:m]
    ids["remote_addr"] = rng.integers(1, 255, (m, 4))
    ids["remote_port"] = rng.integers(1024, 65535, m)

    def up(a, shape=None):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
        return t if shape is None else t.view(shape)
    N = n + m * cap
    d_recs = up(recs, (n, 32)) if n else torch.zeros((0, 32), dtype=torch.uint8, device=dev)
    d_views = torch.from_numpy(views).to(dev)
    d_order, d_first = torch.from_numpy(order).to(dev), torch.from_numpy(first).to(dev)
    d_ids = up(ids, (m, 16)) if m else torch.zeros((0, 16), dtype=torch.uint8, device=dev)
    g = {}
    g["st"] = guarded((m, 40), torch.uint8, dev)
    g["heap"] = guarded((m * cap, 32), torch.uint8, dev)
    if m:
        g["st"][1].copy_(up(st_in, (m, 40)))
    if m * cap:
        g["heap"][1].copy_(up(heap_in, (m * cap, 32)))
    g["status"] = guarded((n,), torch.uint8, dev)
    g["s_views"] = guarded((N, 2), torch.int64, dev)
    g["s_offsets"] = guarded((N + 1,), torch.int64, dev)
    g["a_records"] = guarded((m, 32), torch.uint8, dev)
    g["a_offsets"] = guarded((m + 1,), torch.int64, dev)
    g["n_acks"] = guarded((m,), torch.int32, dev)
    batch.stream_datagrams(d_recs, d_views, d_order, d_first, m, (g["st"][1], g["heap"][1]), ids=d_ids, acks=True,
                           status=g["status"][1], s_views=g["s_views"][1], s_offsets=g["s_offsets"][1],
                           a_records=g["a_records"][1], a_offsets=g["a_offsets"][1], n_acks=g["n_acks"][1])
    torch.cuda.synchronize()
    got = {k: v[1].cpu().numpy() for k, v in g.items()}
    for k, v in g.items():
        assert guards_intact(v[0]), f"guard bytes around {k}"

    # the model
    w_status = np.zeros(n, dtype=np.uint8)
    w_views = np.zeros((N, 2), dtype=np.int64)
    w_st, w_heap = st_in.copy(), heap_in.copy()
    w_arecs = np.zeros(m, dtype=packets.TX_RECORD)
    w_nacks = np.zeros(m, dtype=np.int32)
    for e, (st, heap, segs) in enumerate(eps):
        want = R.walk(st, heaps[e], cap, queues[e])
        for p, v in want["status"].items():
            w_status[p] = v
        lo = int(first[e]) + e * cap
        for k, (b, ln) in enumerate(want["delivered"]):
            w_views[lo + k] = (b, ln)
        if queues[e] and st["state"] in (R.OPEN, R.CLOSED):
            for k in R.ST_FIELDS:
                w_st[e][k] = want["st"][k]
            for i, t in enumerate(want["heap"]):
                x = w_heap[e * cap + i]
                x["base"], x["len"], x["seq"], x["pkt"], x["flags"] = t["base"], t["len"], t["seq"], t["pkt"], t["flags"]
                x["reserved"] = 0
        w_nacks[e] = want["n_acks"]
        if want["ack"]:
            a = w_arecs[e]
            a["src"], a["dst"] = ids[e]["local_addr"], ids[e]["remote_addr"]
            a["sport"], a["dport"] = ids[e]["local_port"], ids[e]["remote_port"]
            a["seq"], a["ack"], a["window"] = want["ack"]
            a["flags"], a["doff"], a["proto"], a["ttl"] = 16, 20, 6, 64
    w_off = np.concatenate(([0], np.cumsum(w_views[:, 1]))).astype(np.int64)
    w_aoff = np.concatenate(([0], np.cumsum(np.where(w_nacks > 0, 40, 0)))).astype(np.int64)
    assert np.array_equal(got["status"], w_status), ("status", np.flatnonzero(got["status"] != w_status)[:8],
                                                     got["status"][:16], w_status[:16])
    assert np.array_equal(got["s_views"], w_views), "s_views"
    assert np.array_equal(got["s_offsets"], w_off), "s_offsets"
    assert np.array_equal(got["st"].reshape(-1), w_st.view(np.uint8).reshape(-1)), \
        ("st", np.frombuffer(got["st"].tobytes(), dtype=packets.TCP_RCV), w_st)
    g_heap = np.frombuffer(got["heap"].tobytes(), dtype=packets.TCP_SEG)
    for e in range(m):
        pc = int(w_st[e]["pend_count"])
        assert pc <= cap
        assert g_heap[e * cap:e * cap + pc].tobytes() == w_heap[e * cap:e * cap + pc].tobytes(), ("heap", e)
    assert got["a_records"].tobytes() == w_arecs.tobytes(), "a_recs"
    assert np.array_equal(got["a_offsets"], w_aoff), "a_offsets"
    assert np.array_equal(got["n_acks"], w_nacks), "n_acks"
    got.update(first=first, order=order, ids=ids, tensors=g, views=d_views, want_status=w_status)
    return got


def grid_batches(dev, seed=20261021):
    """The case grid as a few batches: per capacity, every (kind, length) case an endpoint of
    one call, state-0 UDP endpoints and packets of no endpoint mixed in; then m = 0, 1, 3, 70."""
    rng = np.random.default_rng(seed)
    cases = 0
    by_cap = {cap: [] for cap in C.CAPS}
    for name, cap, st, heap, segs in C.grid(seed):
        by_cap[cap].append((st, heap, segs))
    for cap, eps in by_cap.items():
        mixed = []
        for k, ep in enumerate(eps):
            mixed.append(ep)
            if k % 9 == 0:  # a UDP endpoint: state 0, its queue records of protocol 17
                udp = [dict(C.seg(0, 30), proto=17, doff=0) for _ in range(int(rng.integers(0, 70)))]
                mixed.append((R.new_state(state=R.OFF), [], udp))
        run(mixed, cap, dev, rng, nobody=77)
        cases += len(eps)
    for m in (0, 1, 3, 70):
        for cap in C.CAPS:
            eps = [C.scenario(C.KINDS[(7 * e + cap) % len(C.KINDS)], C.LENS[(e + cap) % 7], cap, rng) for e in range(m)]
            run(eps, cap, dev, rng, nobody=0 if cap == 1 else 5)
            cases += 1
    # n == 0: the empty tables are stored
    run([C.scenario("in_order", 0, 4, rng) for _ in range(3)], 4, dev, rng)
    run([], 0, dev, rng)
    return cases + 2


if __name__ == "__main__":
    print(batch.stream_variant(100, 3, 4), grid_batches(torch.device("cuda:0")), "ok")
