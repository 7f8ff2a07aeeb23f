"""yu_rx_stream on the device (include/yucsum.h) against tests/stream_ref.py, the Python
restatement of the rule. tests/stream_gpu.py assembles the batches and compares every output
byte for byte: status, s_views, s_offsets, st, heap[0, pend_count) per endpoint, a_recs,
a_offsets and n_acks, with guard bytes around each.

* the case grid of tests/stream_cases.py (26 cases x queue lengths 0, 1, 2, 63, 64, 65, 130 x
  cap 0, 1, 4), every case an endpoint of one call per capacity, UDP endpoints in state 0 and
  packets without an endpoint mixed in; m = 0, 1, 3, 70; n = 0;
* the golden vectors of tests/golden/tcp_stream.json, and their ACK datagrams built by
  yu_tx_build_iov from the ACK records;
* the forced general step (YU_TUNING=1 YU_STREAM=walk, a process of its own because the
  tuning values are read once) gives the same outputs: both equal the model's;
* two batches in sequence: a segment parked in the first is delivered in the second, its view
  pointing into the first batch's memory, and the bytes yu_csum_pack_iov gathers are the stream;
* the whole pipeline from datagrams: batch.receive_datagrams (parse, demux, group, stream,
  gather, and the ACKs built and verified)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stream_cases as C
import stream_gpu as G
import stream_ref as R
from yustack_amd import _lib, batch, packets

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def test_case_grid(dev):
    assert batch.stream_variant(100, 3, 4) == "k_stream"
    assert G.grid_batches(dev) == len(C.KINDS) * len(C.LENS) * len(C.CAPS) + 4 * 3 + 2


def gather(s_views, s_offsets, size, dev):
    N = s_views.shape[0]
    fi = torch.arange(N + 1, dtype=torch.int64, device=dev)
    dst = torch.zeros(size, dtype=torch.uint8, device=dev)
    out = torch.empty(max(N, 1), dtype=torch.uint16, device=dev)
    rc = _lib.lib().yu_csum_pack_iov(s_views.data_ptr(), fi.data_ptr(), N, 0, None, 0, None, dst.data_ptr(),
                                     s_offsets.data_ptr(), out.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def test_golden_vectors(dev):
    with open(os.path.join(HERE, "golden", "tcp_stream.json")) as f:
        g = json.load(f)
    rng = np.random.default_rng(5)
    for cap in sorted({v["cap"] for v in g["vectors"]}):
        vs = [v for v in g["vectors"] if v["cap"] == cap]
        got = G.run([(v["st"], v["heap"], v["segs"]) for v in vs], cap, dev, rng, nobody=3)
        for e, v in enumerate(vs):
            pk = got["order"][got["first"][e]:got["first"][e + 1]]
            assert [int(got["status"][p]) for p in pk] == v["status"], v["name"]
            assert int(got["n_acks"][e]) == v["n_acks"], v["name"]
            lo = int(got["first"][e]) + e * cap
            lens = [int(x) for x in got["s_views"][lo:lo + len(v["delivered"]), 1]]
            assert lens == [d[1] for d in v["delivered"]], v["name"]
            st = np.frombuffer(got["st"][e].tobytes(), dtype=packets.TCP_RCV)[0]
            for k in R.ST_FIELDS:
                assert int(st[k]) == v["st_out"][k], (v["name"], k)
        # the ACK datagrams: yu_tx_build_iov over the ACK records, against sendTCP's bytes for the
        # vectors' endpoint (addresses and ports of the fixture in place of the batch's ids)
        m = len(vs)
        t = got["tensors"]
        a_recs = t["a_records"][1].clone()
        rec = np.frombuffer(a_recs.cpu().numpy().tobytes(), dtype=packets.TX_RECORD).copy()
        for e, v in enumerate(vs):
            if v["ack"]:
                rec[e]["src"], rec[e]["dst"] = g["local"], g["remote"]
                rec[e]["sport"], rec[e]["dport"] = g["local_port"], g["remote_port"]
        a_recs.copy_(torch.from_numpy(rec.view(np.uint8).reshape(m, 32).copy()))
        zero_views = torch.zeros((m, 2), dtype=torch.int64, device=dev)
        dst, _, _ = batch.build_datagrams_iov(zero_views, a_recs, t["a_offsets"][1])
        torch.cuda.synchronize()
        img, off = dst.cpu().numpy(), got["a_offsets"]
        for e, v in enumerate(vs):
            want = bytes.fromhex(v.get("ack_datagram", ""))
            assert img[off[e]:off[e + 1]].tobytes() == want, v["name"]


def test_forced_general_step_gives_identical_outputs(dev):
    env = dict(os.environ, YU_TUNING="1", YU_STREAM="walk", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(HERE, "stream_gpu.py")], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    variant, cases, ok = r.stdout.split()[-3:]
    assert variant == "k_stream<walk>" and ok == "ok"
    assert int(cases) == len(C.KINDS) * len(C.LENS) * len(C.CAPS) + 4 * 3 + 2


def test_two_batches_in_sequence(dev):
    """[1000, 1100) in order and [1200, 1300) parked in the first batch; [1100, 1200) in the
    second closes the gap, and the parked segment is delivered from the first batch's memory."""
    rng = np.random.default_rng(11)
    stream_bytes = rng.integers(0, 256, 300, dtype=np.uint8)
    cap, P = 4, C.PITCH
    rc = batch.tcp_receivers(1, cap, dev, packets.tcp_rcv(1, rcv_nxt=1000, wnd=65535, snd_nxt=77))
    ids = torch.from_numpy(packets.endpoint_ids(1, local_addr=[10, 0, 0, 1], remote_addr=[10, 0, 0, 2], local_port=80,
                                                remote_port=4000).view(np.uint8).reshape(1, 16).copy()).to(dev)

    def one(segs):
        """segs: (seq, bytes). Returns the batch's memory and the call's outputs."""
        n = len(segs)
        mem = np.zeros(n * P, dtype=np.uint8)
        recs = packets.tx_records(n, proto=6, flags=R.ACK, doff=20, seq=[s for s, _ in segs])
        views = np.zeros((n, 2), dtype=np.int64)
        for k, (_, b) in enumerate(segs):
            mem[k * P:k * P + len(b)] = b
        d_mem = torch.from_numpy(mem).to(dev)
        for k, (_, b) in enumerate(segs):
            views[k] = (d_mem.data_ptr() + k * P, len(b))
        order = torch.arange(n, dtype=torch.int32, device=dev)
        first = torch.tensor([0, n, n], dtype=torch.int64, device=dev)
        res = batch.stream_datagrams(torch.from_numpy(recs.view(np.uint8).reshape(n, 32).copy()).to(dev),
                                     torch.from_numpy(views).to(dev), order, first, 1, rc, ids=ids, acks=True)
        torch.cuda.synchronize()
        return d_mem, res

    mem1, (status, s_views, s_offsets, a_recs, a_off, n_acks) = one([(1000, stream_bytes[:100]),
                                                                      (1200, stream_bytes[200:])])
    assert status.cpu().tolist() == [R.CONSUMED, R.PENDING]
    assert n_acks.cpu().tolist() == [1] and a_off.cpu().tolist() == [0, 40]
    off = s_offsets.cpu().numpy()
    assert off[-1] == 100
    assert np.array_equal(gather(s_views, s_offsets, 400, dev)[:100], stream_bytes[:100])
    st = np.frombuffer(rc[0].cpu().numpy().tobytes(), dtype=packets.TCP_RCV)[0]
    assert (st["rcv_nxt"], st["pend_count"], st["pend_used"], st["buf_used"]) == (1100, 1, 100, 100)
    heap = np.frombuffer(rc[1].cpu().numpy().tobytes(), dtype=packets.TCP_SEG)
    assert heap[0]["base"] == mem1.data_ptr() + P and heap[0]["len"] == 100 and heap[0]["seq"] == 1200
    assert heap[0]["pkt"] == 0xFFFFFFFF                        # carried over: no packet of a later batch
    a = np.frombuffer(a_recs.cpu().numpy().tobytes(), dtype=packets.TX_RECORD)[0]
    assert (a["seq"], a["ack"], a["flags"], a["doff"], a["proto"], a["ttl"]) == (77, 1100, 16, 20, 6, 64)

    mem2, (status, s_views, s_offsets, a_recs, a_off, n_acks) = one([(1100, stream_bytes[100:200])])
    assert status.cpu().tolist() == [R.CONSUMED]
    sv = s_views.cpu().numpy()
    assert sv[0].tolist() == [mem2.data_ptr(), 100] and sv[1].tolist() == [mem1.data_ptr() + P, 100]
    assert s_offsets.cpu().numpy()[-1] == 200
    assert np.array_equal(gather(s_views, s_offsets, 400, dev)[:200], stream_bytes[100:])
    st = np.frombuffer(rc[0].cpu().numpy().tobytes(), dtype=packets.TCP_RCV)[0]
    assert (st["rcv_nxt"], st["pend_count"], st["pend_used"], st["buf_used"]) == (1300, 0, 0, 300)
    assert n_acks.cpu().tolist() == [1]                       # the final check: rcv_nxt moved past max_sent_ack


def test_full_pipeline_from_datagrams(dev):
    """Two TCP connections (one in order, one with its segments swapped), a UDP listener and
    a segment for nobody, as IPv4 datagrams: parse, demux, group, stream, gather, ACKs."""
    rng = np.random.default_rng(13)
    A = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
    Bs = rng.integers(0, 256, 500, dtype=np.uint8).tobytes()
    opts = bytes([1, 1, 8, 10, 0, 0, 0, 1, 0, 0, 0, 2])      # NOP NOP timestamp: doff 32
    pk = [packets.tcp_test_packet(A[:300], 4000, 80, 1000, 1, R.ACK, 1000),
          packets.tcp_test_packet(Bs[200:], 4001, 80, (0xFFFFFFF0 + 200) & 0xFFFFFFFF, 1, R.ACK | R.PSH, 1000),
          packets.udp_test_packet(b"x" * 50, 999, 53, test_addr=bytes([10, 0, 0, 2]), stack_addr=bytes([10, 0, 0, 1])),
          packets.tcp_test_packet(A[300:], 4000, 80, 1300, 1, R.ACK, 1000, tcp_opts=opts),
          packets.tcp_test_packet(b"nobody", 4009, 81, 5, 1, R.ACK, 1000),
          packets.tcp_test_packet(Bs[:200], 4001, 80, 0xFFFFFFF0, 1, R.ACK, 1000)]
    offs = np.concatenate(([0], np.cumsum([len(p) for p in pk]))).astype(np.int64)
    data = torch.from_numpy(np.frombuffer(b"".join(bytes(p) for p in pk), dtype=np.uint8).copy()).to(dev)
    ids = packets.endpoint_ids(3, local_addr=[10, 0, 0, 1], remote_addr=[10, 0, 0, 2], local_port=80, proto=6)
    ids["remote_port"] = [4000, 4001, 0]
    ids[2]["proto"], ids[2]["kind"], ids[2]["local_port"], ids[2]["local_addr"], ids[2]["remote_addr"] = 17, 2, 53, 0, 0
    table, m = batch.demux_table(ids, dev)
    cap = 2
    state = packets.tcp_rcv(3, rcv_nxt=[1000, 0xFFFFFFF0, 0], wnd=65535, snd_nxt=[1, 2, 0], state=[1, 1, 0])
    rcv = batch.tcp_receivers(m, cap, dev, state)
    d_ids = torch.from_numpy(ids.view(np.uint8).reshape(3, 16).copy()).to(dev)
    res = batch.receive_datagrams(data, torch.from_numpy(offs).to(dev), table, m, rcv,
                                  need=batch.RX_IP_OK | batch.RX_L4_OK, ids=d_ids, acks=True,
                                  dst=torch.empty(data.numel() + cap * m * 1460, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    assert res["ep"].cpu().tolist() == [0, 1, 2, 0, 0xFFFFFFFF, 1]
    assert res["status"].cpu().tolist() == [R.CONSUMED, R.CONSUMED_LATE, R.NONE, R.CONSUMED, R.NONE, R.CONSUMED]
    first, so, dst = res["first"].cpu().numpy(), res["s_offsets"].cpu().numpy(), res["dst"].cpu().numpy()
    got = [dst[so[first[e] + e * cap]:so[first[e + 1] + (e + 1) * cap]].tobytes() for e in range(3)]
    assert got == [A, Bs, b""]
    st = np.frombuffer(rcv[0].cpu().numpy().tobytes(), dtype=packets.TCP_RCV)
    assert st["rcv_nxt"].tolist() == [1700, (0xFFFFFFF0 + 500) & 0xFFFFFFFF, 0] and st["pend_count"].tolist() == [0, 0, 0]
    assert res["n_acks"].cpu().tolist() == [1, 2, 0] and res["a_offsets"].cpu().tolist() == [0, 40, 80, 80]
    flags = batch.checksum_ragged(res["ack_dst"], res["a_offsets"], "verify_rx").cpu().numpy()
    assert (flags[:2] == (batch.RX_IP_OK | batch.RX_L4 | batch.RX_L4_OK)).all()
    ack = res["ack_dst"].cpu().numpy()
    for e, (port, snd, nxt) in enumerate(((4000, 1, 1700), (4001, 2, (0xFFFFFFF0 + 500) & 0xFFFFFFFF))):
        want = packets.send_tcp(packets.Route(bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])), 80, port, None, R.ACK, snd,
                                nxt, min((int(st["rcv_acc"][e]) - nxt) & 0xFFFFFFFF, 0xFFFF))
        assert ack[40 * e:40 * e + 40].tobytes() == bytes(want), e


# ---- group, stream, gather and the ACK build captured as one graph -----------------------------
G_N, G_M, G_CAP = 8, 3, 2
NOBODY = 0xFFFFFFFF


def graph_batches(mem):
    """Two batches of 8 packets for connections 0 and 1 (TCP) and endpoint 2 (UDP, state 0):
    (endpoint, seq, flags, bytes) per packet, the payload of packet p of batch b at
    mem[b][p * PITCH]. Batch 1 leaves connection 0's segment 1200 parked; batch 2 closes the gap,
    so it is delivered from batch 1's memory, and connection 1 takes a FIN."""
    rng = np.random.default_rng(17)
    A = rng.integers(0, 256, 400, dtype=np.uint8)
    B = rng.integers(0, 256, 400, dtype=np.uint8)
    u = np.full(30, 0x55, dtype=np.uint8)
    one = [(0, 1000, R.ACK, A[:100]), (1, 5200, R.ACK, B[200:300]), (2, 0, 0, u), (0, 1200, R.ACK, A[200:300]),
           (NOBODY, 9, R.ACK, u), (1, 5000, R.ACK | R.PSH, B[:200]), (0, 1100, R.ACK, A[100:150]), (2, 0, 0, u)]
    two = [(0, 1150, R.ACK, A[150:200]), (1, 5300, R.ACK | R.FIN, B[300:310]), (NOBODY, 9, R.ACK, u), (2, 0, 0, u),
           (0, 1300, R.ACK, A[300:320]), (1, 5311, R.ACK, B[311:316]), (0, 1000, R.ACK, A[:50]), (2, 0, 0, u)]
    want_streams = [(A[:150].tobytes(), B[:300].tobytes()), (A[150:320].tobytes(), B[300:310].tobytes())]
    out = []
    for b, pk in enumerate((one, two)):
        img = np.zeros(G_N * C.PITCH, dtype=np.uint8)
        recs = packets.tx_records(G_N, proto=[6 if e != 2 else 17 for e, *_ in pk], doff=20,
                                  flags=[f for _, _, f, _ in pk], seq=[s for _, s, _, _ in pk])
        views = np.zeros((G_N, 2), dtype=np.int64)
        for p, (e, s, f, data) in enumerate(pk):
            img[p * C.PITCH:p * C.PITCH + len(data)] = data
            views[p] = (mem[b].data_ptr() + p * C.PITCH, len(data))
        out.append(dict(k=b, img=img, recs=recs, views=views, ep=np.array([e for e, *_ in pk], dtype=np.uint32),
                        streams=want_streams[b]))
    return out


def test_group_stream_gather_and_acks_captured_in_one_graph_and_replayed(dev):
    """yu_rx_group, yu_rx_stream, yu_csum_pack_iov and yu_tx_build_iov with every buffer given,
    captured once and replayed over two batches written into the same input buffers while st and
    the heap stay in device memory: every output equals tests/stream_ref.py's after each replay,
    a segment parked in replay 1 is delivered in replay 2, and the n == 0 branch captures too."""
    n, m, cap = G_N, G_M, G_CAP
    N = n + m * cap
    mem = [torch.zeros(n * C.PITCH, dtype=torch.uint8, device=dev) for _ in range(2)]
    batches = graph_batches(mem)
    ids = packets.endpoint_ids(m, local_addr=[10, 0, 0, 1], remote_addr=[10, 0, 0, 2], local_port=80, proto=6)
    ids["remote_port"] = [4000, 4001, 4002]
    d_ids = torch.from_numpy(ids.view(np.uint8).reshape(m, 16).copy()).to(dev)
    st0 = packets.tcp_rcv(m, rcv_nxt=[1000, 5000, 0], wnd=65535, snd_nxt=[11, 22, 0], state=[1, 1, 0])
    st, heap = batch.tcp_receivers(m, cap, dev, st0)
    st_keep = st.clone()
    z = dict(device=dev)
    recs = torch.zeros((n, 32), dtype=torch.uint8, **z)
    views = torch.zeros((n, 2), dtype=torch.int64, **z)
    ep = torch.zeros(n, dtype=torch.uint32, **z)
    order, first = torch.empty(n, dtype=torch.int32, **z), torch.empty(m + 2, dtype=torch.int64, **z)
    g_work = torch.empty(max(batch.group_workspace_bytes(n, m), 16), dtype=torch.uint8, **z)
    status = torch.empty(n, dtype=torch.uint8, **z)
    s_views, s_offsets = torch.empty((N, 2), dtype=torch.int64, **z), torch.empty(N + 1, dtype=torch.int64, **z)
    a_recs, a_offsets = torch.empty((m, 32), dtype=torch.uint8, **z), torch.empty(m + 1, dtype=torch.int64, **z)
    n_acks = torch.empty(m, dtype=torch.int32, **z)
    s_work = torch.empty(max(batch.stream_workspace_bytes(n, m, cap), 16), dtype=torch.uint8, **z)
    fi = torch.arange(N + 1, dtype=torch.int64, **z)
    dst, sums = torch.empty(4096, dtype=torch.uint8, **z), torch.empty(N, dtype=torch.uint16, **z)
    zero_views = torch.zeros((m, 2), dtype=torch.int64, **z)
    ack_dst, ack_out = torch.empty(40 * m, dtype=torch.uint8, **z), torch.empty(2 * m, dtype=torch.uint16, **z)
    # the empty batch beside it: its outputs are stored by the captured zeroing launches
    e_views, e_offsets = torch.empty((m * cap, 2), dtype=torch.int64, **z), torch.empty(m * cap + 1, dtype=torch.int64, **z)
    e_first = torch.zeros(m + 2, dtype=torch.int64, **z)
    e_in = (torch.empty((0, 32), dtype=torch.uint8, **z), torch.empty((0, 2), dtype=torch.int64, **z),
            torch.empty(0, dtype=torch.int32, **z))
    e_st, e_heap = batch.tcp_receivers(m, cap, dev, st0)

    def load(b):
        mem[b["k"]].copy_(torch.from_numpy(b["img"]))
        recs.copy_(torch.from_numpy(b["recs"].view(np.uint8).reshape(n, 32).copy()))
        views.copy_(torch.from_numpy(b["views"]))
        ep.copy_(torch.from_numpy(b["ep"]))

    def calls():
        batch.group_datagrams(ep, m, order=order, first=first, work=g_work)
        batch.stream_datagrams(recs, views, order, first, m, (st, heap), ids=d_ids, acks=True, status=status,
                               s_views=s_views, s_offsets=s_offsets, a_records=a_recs, a_offsets=a_offsets,
                               n_acks=n_acks, work=s_work)
        rc = _lib.lib().yu_csum_pack_iov(s_views.data_ptr(), fi.data_ptr(), N, 0, None, 0, None, dst.data_ptr(),
                                         s_offsets.data_ptr(), sums.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
        batch.build_datagrams_iov(zero_views, a_recs, a_offsets, ack_dst, out=ack_out)
        batch.stream_datagrams(e_in[0], e_in[1], e_in[2], e_first, m, (e_st, e_heap), s_views=e_views,
                               s_offsets=e_offsets, work=s_work)

    load(batches[0])
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        calls()  # warm up; it advances the receivers, which are put back below
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            calls()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)
    st.copy_(st_keep)
    heap.zero_()

    model_st = [{k: int(st0[e][k]) for k in R.ST_FIELDS} for e in range(m)]
    model_heap = [[] for _ in range(m)]
    seen = set()
    for b in batches:
        load(b)
        for t in (order, first, status, s_views, s_offsets, a_recs, a_offsets, n_acks, dst, ack_dst, e_views, e_offsets):
            t.view(torch.uint8).fill_(0xA5)
        g.replay()
        torch.cuda.synchronize(dev)
        want_order = np.argsort(np.minimum(b["ep"], m), kind="stable")
        want_first = np.searchsorted(np.minimum(b["ep"], m)[want_order], np.arange(m + 2))
        assert np.array_equal(order.cpu().numpy(), want_order) and np.array_equal(first.cpu().numpy(), want_first)
        w_status, w_views = np.zeros(n, dtype=np.uint8), np.zeros((N, 2), dtype=np.int64)
        w_nacks, w_st = np.zeros(m, dtype=np.int32), []
        for e in range(m):
            pk = [int(p) for p in np.flatnonzero(b["ep"] == e)]
            q = [dict(pkt=p, proto=int(b["recs"][p]["proto"]), doff=20, flags=int(b["recs"][p]["flags"]),
                      seq=int(b["recs"][p]["seq"]), base=int(b["views"][p][0]), vlen=int(b["views"][p][1])) for p in pk]
            want = R.walk(model_st[e], model_heap[e], cap, q)
            model_st[e], model_heap[e] = want["st"], want["heap"]
            for p, v in want["status"].items():
                w_status[p] = v
            for k, d in enumerate(want["delivered"]):
                w_views[want_first[e] + e * cap + k] = d
            w_nacks[e] = want["n_acks"]
            w_st.append(want["st"])
        seen |= set(w_status.tolist())
        assert np.array_equal(status.cpu().numpy(), w_status), (status.cpu().numpy(), w_status)
        assert np.array_equal(s_views.cpu().numpy(), w_views)
        so = s_offsets.cpu().numpy()
        assert np.array_equal(so, np.concatenate(([0], np.cumsum(w_views[:, 1]))))
        assert np.array_equal(n_acks.cpu().numpy(), w_nacks)
        assert np.array_equal(a_offsets.cpu().numpy(), np.concatenate(([0], np.cumsum(np.where(w_nacks > 0, 40, 0)))))
        got_st = np.frombuffer(st.cpu().numpy().tobytes(), dtype=packets.TCP_RCV)
        g_heap = np.frombuffer(heap.cpu().numpy().tobytes(), dtype=packets.TCP_SEG)
        for e in range(m):
            for k in R.ST_FIELDS:
                assert int(got_st[e][k]) == w_st[e][k], (e, k)
            for i, t in enumerate(model_heap[e]):
                x = g_heap[e * cap + i]
                assert (int(x["base"]), int(x["len"]), int(x["seq"]), int(x["pkt"]), int(x["flags"])) == \
                    (t["base"], t["len"], t["seq"], t["pkt"], t["flags"]), (e, i)
        # the gathered bytes are each connection's new in-order bytes; the ACKs are sendTCP's datagrams
        img, ack, ao = dst.cpu().numpy(), ack_dst.cpu().numpy(), a_offsets.cpu().numpy()
        for e in range(2):
            lo, hi = so[want_first[e] + e * cap], so[want_first[e + 1] + (e + 1) * cap]
            assert img[lo:hi].tobytes() == b["streams"][e], e
            assert w_nacks[e] > 0
            w = min((w_st[e]["rcv_acc"] - w_st[e]["rcv_nxt"]) & 0xFFFFFFFF, 0xFFFF)
            want = packets.send_tcp(packets.Route(bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])), 80, 4000 + e, None, R.ACK,
                                    w_st[e]["snd_nxt"], w_st[e]["rcv_nxt"], w)
            assert ack[ao[e]:ao[e + 1]].tobytes() == bytes(want), e
        assert (img[so[-1]:] == 0xA5).all() and (ack[ao[-1]:] == 0xA5).all()
        assert not e_views.any() and not e_offsets.any()                  # n == 0: the empty tables, stored
        assert torch.equal(e_st, st_keep) and not e_heap.any()            # and no state touched
        if b is batches[0]:
            assert model_st[0]["pend_count"] == 1 and model_heap[0][0]["seq"] == 1200
            assert model_heap[0][0]["base"] == mem[0].data_ptr() + 3 * C.PITCH
    assert model_st[0]["pend_count"] == 0 and model_st[0]["rcv_nxt"] == 1320 and model_st[1]["state"] == R.CLOSED
    assert {R.CONSUMED, R.CONSUMED_LATE, R.PENDING, R.AFTER_CLOSE, R.UNACCEPTABLE, R.NONE} <= seen
    sv = s_views.cpu().numpy()
    assert [mem[0].data_ptr() + 3 * C.PITCH, 100] in sv.tolist()          # delivered from the first batch's memory
