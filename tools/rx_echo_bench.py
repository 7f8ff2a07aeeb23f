#!/usr/bin/env python3
"""The device echo (yu_rx_reply + yu_tx_build_iov) against the route it replaces
(measurement only).

Three workloads of --n received datagrams each, built on the device by yu_tx_build_ragged:

  udp1500  1500-byte UDP datagrams (1472-byte payloads) to one listener on a port
  udp72    72-byte UDP datagrams (44-byte payloads) to the same listener
  icmp56   ICMP Echo requests with 56-byte payloads (84-byte datagrams)

Every packet is answered. Per workload, alternated launch by launch within one process,
each timed with HIP events, medians over --launches launches:

  (a) echo        batch.echo_datagrams end to end (need = --need, 0 by default: the
                  reference's gate, so the parse is the header pass alone)
      parse, demux, reply, build_iov   each of its four C calls alone, on preallocated buffers
  (b) replaced    the same parse and demux calls, then what a caller had to do before: the
                  reply records and both offset tables with torch operations (where, the
                  field swaps, two cumsums), yu_csum_pack_iov(RAW) of the answered views into
                  a contiguous buffer, and yu_tx_build_ragged
      torch, pack, build_ragged        its three parts alone
  (c) copy        a plain device copy of the reply bytes
  (d) build_iov against build_ragged on the same payloads laid contiguously (the views
      point into the buffer (b) packed), five repeats of --launches launches each: the
      medians of the repeats and their spread; then the same five with the two calls'
      destination buffers exchanged, which tells a difference between the kernels from one
      between the buffers

Before timing, the replies of (a) are compared with (b)'s byte for byte, VERIFY_RX must
accept every one, and (d)'s two outputs must be equal.

Prints one JSON line per workload. The library's knobs apply (YU_TUNING=1 YU_BLOCKS_PER_CU,
YU_NT).

  python tools/rx_echo_bench.py [--n 1048576] [--launches 10] [--need 0] [--workloads udp1500,udp72,icmp56]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yustack_amd import _lib, batch, packets  # noqa: E402

WORKLOADS = {"udp1500": (17, 1472), "udp72": (17, 44), "icmp56": (1, 56)}
H_OF = {17: 8, 1: 4}
RAW = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--need", type=int, default=0)
    ap.add_argument("--workloads", default="udp1500,udp72,icmp56")
    a = ap.parse_args()
    n, need, dev = a.n, a.need, torch.device("cuda:0")
    rng = np.random.default_rng(19)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    i64 = dict(dtype=torch.int64, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    ids = packets.endpoint_ids(1, local_port=7, proto=17, kind=2)
    table, m = batch.demux_table(ids, dev)
    arange = torch.arange(n + 1, **i64)

    def ck(rc, what):
        _lib.check(rc, what)

    for name in a.workloads.split(","):
        proto, pl = WORKLOADS[name]
        T = 20 + H_OF[proto] + pl
        # the received batch: built on the device from random payloads and records
        recs_h = packets.tx_records(n, src=rng.integers(1, 255, (n, 4), dtype=np.uint8), dst=[10, 0, 0, 1],
                                    sport=rng.integers(1024, 65536, n) if proto == 17 else 8 << 8, dport=7,
                                    proto=proto)
        src_pay = torch.randint(0, 256, (n * pl,), **u8)
        data, offs, _ = batch.build_datagrams(src_pay, arange * pl,
                                              torch.from_numpy(recs_h.view(np.uint8).reshape(n, 32).copy()).to(dev))
        del src_pay
        size = data.numel()
        assert size == n * T

        # buffers of the C calls
        recs, views = torch.zeros((n, 32), **u8), torch.zeros((n, 2), **i64)
        flags, ep = torch.zeros(n, dtype=torch.uint16, device=dev), torch.zeros(n, dtype=torch.uint32, device=dev)
        r_recs, r_offs = torch.zeros((n, 32), **u8), torch.zeros(n + 1, **i64)
        work = torch.zeros(batch.reply_workspace_bytes(n), **u8)
        dst_a, dst_b, dst_c = torch.zeros(size, **u8), torch.zeros(size, **u8), torch.zeros(size, **u8)
        out_a, out_b = (torch.zeros(2 * n, dtype=torch.uint16, device=dev) for _ in range(2))
        out_p = torch.zeros(n, dtype=torch.uint16, device=dev)
        paybuf = torch.zeros(n * pl + 8, **u8)
        state = {}

        def parse(_):
            ck(L.yu_rx_parse_ragged(data.data_ptr(), offs.data_ptr(), n, 1 if need else 0, recs.data_ptr(),
                                    views.data_ptr(), flags.data_ptr(), stream), "yu_rx_parse_ragged")

        def demux(_):
            ck(L.yu_rx_demux(recs.data_ptr(), flags.data_ptr(), need, n, table.data_ptr(), table.numel(), m,
                             ep.data_ptr(), None, stream), "yu_rx_demux")

        def reply(_):
            ck(L.yu_rx_reply(recs.data_ptr(), flags.data_ptr(), need, views.data_ptr(), ep.data_ptr(), m, None, 3, n,
                             r_recs.data_ptr(), r_offs.data_ptr(), work.data_ptr(), work.numel(), stream),
               "yu_rx_reply")

        def build_iov(_):
            ck(L.yu_tx_build_iov(views.data_ptr(), r_recs.data_ptr(), n, dst_a.data_ptr(), r_offs.data_ptr(),
                                 out_a.data_ptr(), stream), "yu_tx_build_iov")

        def echo(_):
            state["echo"] = batch.echo_datagrams(data, offs, table, m, need=need, dst=dst_a)

        def torch_part(_):
            """The reply records and the two offset tables with torch operations."""
            w = recs.view(torch.int32)
            pr = recs[:, 24]
            gate = (flags.view(torch.int16) & (need | batch.RX_SPLIT)) == (need | batch.RX_SPLIT)
            e = ep.view(torch.int32)
            udp = gate & (pr == 17) & (e >= 0) & (e < m)
            icmp = gate & (pr == 1) & (recs[:, 9] == 8)
            ans = udp | icmp
            r = torch.zeros_like(w)
            r[:, 0], r[:, 1] = w[:, 1], w[:, 0]
            r[:, 2] = torch.where(udp, ((w[:, 2] >> 16) & 0xFFFF) | (w[:, 2] << 16), 0)
            r[:, 6] = pr.to(torch.int32) | (64 << 8)
            r = torch.where(ans[:, None], r, 0)
            ln = torch.where(ans, views[:, 1], 0)
            tot = torch.where(ans, 20 + torch.where(udp, 8, 4) + ln, 0)
            po, do = torch.zeros(n + 1, **i64), torch.zeros(n + 1, **i64)
            po[1:], do[1:] = torch.cumsum(ln, 0), torch.cumsum(tot, 0)
            v = views.clone()
            v[:, 1] = ln
            state["b"] = (r.view(torch.uint8), po, do, v)

        def pack(_):
            r, po, do, v = state["b"]
            ck(L.yu_csum_pack_iov(v.data_ptr(), arange.data_ptr(), n, RAW, None, 0, None, paybuf.data_ptr(),
                                  po.data_ptr(), out_p.data_ptr(), stream), "yu_csum_pack_iov")

        def build_ragged(_):
            r, po, do, v = state["b"]
            ck(L.yu_tx_build_ragged(paybuf.data_ptr(), po.data_ptr(), r.data_ptr(), n, dst_b.data_ptr(),
                                    do.data_ptr(), out_b.data_ptr(), stream), "yu_tx_build_ragged")

        def replaced(it):
            parse(it), demux(it), torch_part(it), pack(it), build_ragged(it)

        def copy(_):
            dst_c.copy_(dst_a)

        # both routes once, compared over the whole batch
        echo(0)
        replaced(0)
        torch.cuda.synchronize()
        _, r_o, e_out, _, _ = state["echo"]
        assert int(r_o[-1]) == size and torch.equal(r_o, state["b"][2]), f"{name}: offsets"
        assert torch.equal(dst_a, dst_b) and torch.equal(e_out, out_b), f"{name}: the two routes differ"
        rx = batch.checksum_ragged(dst_a, r_o, "verify_rx")
        assert (rx == (batch.RX_IP_OK | batch.RX_L4 | batch.RX_L4_OK)).all(), f"{name}: VERIFY_RX"
        reply(0)  # r_recs and r_offs of the C call, for build_iov alone
        torch.cuda.synchronize()

        alts = {"echo": echo, "parse": parse, "demux": demux, "reply": reply, "build_iov": build_iov,
                "replaced": replaced, "torch": torch_part, "pack": pack, "build_ragged": build_ragged, "copy": copy}
        ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in alts}
        times = {k: [] for k in alts}
        for it in range(a.launches + 2):
            for k, fn in alts.items():
                ev[k][0].record()
                fn(it)
                ev[k][1].record()
            torch.cuda.synchronize()
            if it >= 2:  # warm-up launches are not recorded
                for k in alts:
                    times[k].append(ev[k][0].elapsed_time(ev[k][1]) * 1e3)
        med = {k: statistics.median(t) for k, t in times.items()}

        # (d) the two builders on the same contiguous payloads
        r, po, do, _ = state["b"]
        cviews = torch.stack((paybuf.data_ptr() + po[:-1], po[1:] - po[:-1]), 1).contiguous()

        def d_iov(dst, out):
            ck(L.yu_tx_build_iov(cviews.data_ptr(), r.data_ptr(), n, dst.data_ptr(), do.data_ptr(), out.data_ptr(),
                                 stream), "yu_tx_build_iov")

        def d_ragged(dst, out):
            ck(L.yu_tx_build_ragged(paybuf.data_ptr(), po.data_ptr(), r.data_ptr(), n, dst.data_ptr(), do.data_ptr(),
                                    out.data_ptr(), stream), "yu_tx_build_ragged")

        d_iov(dst_a, out_a), d_ragged(dst_b, out_b)
        torch.cuda.synchronize()
        assert torch.equal(dst_a, dst_b) and torch.equal(out_a, out_b), f"{name}: (d) outputs differ"
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def five(iov_to, ragged_to):
            """Five repeats of --launches alternated launches: the median of each repeat."""
            reps = {"iov": [], "ragged": []}
            for _ in range(5):
                t = {"iov": [], "ragged": []}
                for it in range(a.launches + 1):
                    for k, fn, to in (("iov", d_iov, iov_to), ("ragged", d_ragged, ragged_to)):
                        e0.record()
                        fn(*to)
                        e1.record()
                        torch.cuda.synchronize()
                        if it >= 1:
                            t[k].append(e0.elapsed_time(e1) * 1e3)
                for k in reps:
                    reps[k].append(round(statistics.median(t[k]), 2))
            return reps

        reps = five((dst_a, out_a), (dst_b, out_b))
        swapped = five((dst_b, out_b), (dst_a, out_a))  # the two destination buffers exchanged
        spread = max(reps["ragged"]) - min(reps["ragged"])
        gap = statistics.median(reps["iov"]) - statistics.median(reps["ragged"])
        gap_swapped = statistics.median(swapped["iov"]) - statistics.median(swapped["ragged"])
        print(json.dumps({
            "workload": name, "n": n, "datagram_bytes": T, "reply_bytes": size, "need": need, "launches": a.launches,
            "variants": {"parse": batch.parse_variant(n), "demux": batch.demux_variant(n),
                         "reply": batch.reply_variant(n), "build_iov": batch.build_iov_variant(n),
                         "build_ragged": batch.build_variant(n), "pack": batch.iov_pack_variant("raw", n)},
            "knobs": {k: v for k, v in os.environ.items() if k.startswith("YU_")},
            "us": {k: round(v, 2) for k, v in med.items()},
            "us_min": {k: round(min(t), 2) for k, t in times.items()},
            "us_max": {k: round(max(t), 2) for k, t in times.items()},
            "echo_vs_replaced": round(med["echo"] / med["replaced"], 3),
            "echo_vs_copy": round(med["echo"] / med["copy"], 3),
            "four_calls_sum_us": round(med["parse"] + med["demux"] + med["reply"] + med["build_iov"], 2),
            "d_build_us": reps, "d_ragged_spread_us": round(spread, 2), "d_iov_minus_ragged_us": round(gap, 2),
            "d_build_swapped_us": swapped, "d_swapped_iov_minus_ragged_us": round(gap_swapped, 2),
        }), flush=True)
        del data, recs, views, flags, ep, r_recs, r_offs, work, dst_a, dst_b, dst_c, out_a, out_b, paybuf, cviews
        state.clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
