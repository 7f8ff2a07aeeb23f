#!/usr/bin/env python3
"""yu_rx_demux against a plain read of its records (measurement only).

Input: n records as yu_rx_parse_ragged(verify=0) leaves them for rx_parse_bench.py's
tcp1460 workload (n received 1500-byte TCP datagrams built on the device by
yu_tx_build_ragged, every one to 10.0.0.1:443 from its own remote address and port).
The tables:

  one      m = 1, a listener on port 443 (kind 2): every packet takes all three lookups
           and lands on one endpoint, the worst case for the counters
  conn64k  m = 65536 connections (kind 0), a 2 MiB table: every packet hits on the first
           lookup. Its records are the parsed records of the first 65536 packets, each 16
           times, shuffled
  conn1m   m = n connections (kind 0), a 32 MiB table at n = 1M: the parsed records as
           they are
  miss     conn64k's table against the parsed records with another destination port:
           every packet takes all three lookups and misses

Per table, alternated launch by launch within one process, each timed with HIP events,
medians over --launches launches:

  demux        yu_rx_demux with ep_count = NULL
  demux_count  yu_rx_demux with ep_count (the counters are not cleared between launches)
  read         a plain read of the record array: torch's sum over it as int64 words
  parse0       yu_rx_parse_ragged(verify=0) on the datagrams, the call that produced the
               records

Before timing, ep and the counters of each table's first 4099 records are checked against
tests/demux_ref.py, the reference's three map lookups restated in Python.

The record arrays rotate over --rsets copies (32 MiB each at 1M), the datagram batches
over --sets. Prints one JSON line per table. The library's knobs apply (YU_TUNING=1
YU_NT=0|1, YU_BLOCKS_PER_CU).

  python tools/rx_demux_bench.py [--n 1048576] [--launches 30] [--sets 2] [--rsets 8] [--tables one,conn64k,conn1m,miss]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import demux_ref  # noqa: E402
from yustack_amd import _lib, batch, packets  # noqa: E402

SAMPLE = 4099
LOCAL, PORT = (10, 0, 0, 1), 443


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--rsets", type=int, default=8)
    ap.add_argument("--tables", default="one,conn64k,conn1m,miss")
    a = ap.parse_args()
    n, dev = a.n, torch.device("cuda:0")
    pl, T = 1460, 1500
    rng = np.random.default_rng(17)
    g = torch.Generator(device=dev).manual_seed(17)
    remote = np.unique(rng.integers(0, 1 << 48, 2 * n, dtype=np.int64))  # distinct (address, port) pairs
    remote = rng.permutation(remote)[:n]
    src = np.stack([(remote >> s) & 0xFF for s in (40, 32, 24, 16)], 1).astype(np.uint8)
    recs_h = packets.tx_records(n, src=src, dst=LOCAL, sport=remote & 0xFFFF, dport=PORT,
                                seq=rng.integers(0, 2 ** 32, n), ack=rng.integers(0, 2 ** 32, n),
                                window=rng.integers(0, 65536, n), flags=0x18, proto=6)
    recs_in = torch.from_numpy(recs_h.view(np.uint8).reshape(n, 32).copy()).to(dev)
    po = torch.arange(n + 1, device=dev) * pl
    offs = torch.arange(n + 1, device=dev) * T
    datas = []
    for k in range(a.sets):
        p = torch.randint(0, 256, (n * pl,), dtype=torch.uint8, device=dev, generator=g)
        datas.append(batch.build_datagrams(p, po, recs_in, dst_offsets=offs)[0])
    del p
    parsed, pviews, pout = batch.parse_datagrams(datas[0], offs, verify=False)
    torch.cuda.synchronize()
    assert bool((pout == batch.RX_SPLIT).all())
    assert np.array_equal(packets.rx_records(parsed).view(np.uint8), recs_h.view(np.uint8)), "parsed records"

    c64 = min(65536, n)
    conn = packets.endpoint_ids(n, local_addr=LOCAL, local_port=PORT, remote_addr=src, remote_port=remote & 0xFFFF,
                                proto=6, kind=0)
    again = torch.from_numpy(rng.permutation(n) % c64).to(dev)
    other_port = parsed.clone()
    other_port[:, 10] += 1  # dport's low byte
    # table name -> (ids, the records it is run against)
    cases = {"one": (packets.endpoint_ids(1, local_port=PORT, proto=6, kind=2), parsed),
             "conn64k": (conn[:c64], parsed[again].contiguous()),
             "conn1m": (conn, parsed),
             "miss": (conn[:c64], other_port)}
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(4)]
    for name in a.tables.split(","):
        ids, recs0 = cases[name]
        table, m = batch.demux_table(ids, dev)
        # the sample against the restatement
        ep_s, counts_s = batch.demux_datagrams(recs0[:SAMPLE].contiguous(), table, m, flags=pout[:SAMPLE].contiguous())
        want_ep, want_counts = demux_ref.demux(ids, packets.rx_records(recs0[:SAMPLE]), pout[:SAMPLE].cpu().numpy(), 0)
        assert np.array_equal(ep_s.cpu().numpy(), want_ep), f"{name}: ep"
        assert np.array_equal(counts_s.cpu().numpy(), want_counts), f"{name}: counts"
        hits = int((want_ep != demux_ref.NONE).sum())
        assert hits == (0 if name == "miss" else min(SAMPLE, n)), f"{name}: {hits} hits in the sample"
        del ep_s, counts_s

        rsets = [recs0] + [recs0.clone() for _ in range(a.rsets - 1)]
        words = [r.view(torch.int64) for r in rsets]
        ep = torch.zeros(n, dtype=torch.uint32, device=dev)
        counts = torch.zeros(m + 1, dtype=torch.uint32, device=dev)
        recs_out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        views = torch.zeros((n, 2), dtype=torch.int64, device=dev)
        out = torch.zeros(n, dtype=torch.uint16, device=dev)
        sink = []

        def demux(with_counts):
            def fn(it):
                _lib.check(L.yu_rx_demux(rsets[it % len(rsets)].data_ptr(), pout.data_ptr(), 0, n, table.data_ptr(),
                                         table.numel(), m, ep.data_ptr(), counts.data_ptr() if with_counts else None,
                                         stream), "yu_rx_demux")
            return fn

        def read(it):
            sink[:] = [words[it % len(words)].sum()]

        def parse0(it):
            _lib.check(L.yu_rx_parse_ragged(datas[it % len(datas)].data_ptr(), offs.data_ptr(), n, 0,
                                            recs_out.data_ptr(), views.data_ptr(), out.data_ptr(), stream),
                       "yu_rx_parse_ragged")

        alts = {"demux": demux(False), "demux_count": demux(True), "read": read, "parse0": parse0}
        times = {k: [] for k in alts}
        for it in range(a.launches + 3):
            for (k, fn), (e0, e1) in zip(alts.items(), ev):
                timed(lambda: fn(it), e0, e1)
            torch.cuda.synchronize()
            if it >= 3:  # warm-up launches are not recorded
                for k, (e0, e1) in zip(alts, ev):
                    times[k].append(e0.elapsed_time(e1) * 1e3)
        med = {k: statistics.median(t) for k, t in times.items()}
        print(json.dumps({
            "table": name, "n": n, "m": m, "table_bytes": table.numel(), "launches": a.launches, "rsets": len(rsets),
            "sets": len(datas), "variant": batch.demux_variant(n), "sample_hits": hits,
            "knobs": {k: v for k, v in os.environ.items() if k.startswith("YU_")},
            "us": {k: round(v, 2) for k, v in med.items()},
            "us_min": {k: round(min(t), 2) for k, t in times.items()},
            "us_max": {k: round(max(t), 2) for k, t in times.items()},
            "demux_vs_read": round(med["demux"] / med["read"], 3),
            "demux_count_vs_read": round(med["demux_count"] / med["read"], 3),
            "demux_count_vs_demux": round(med["demux_count"] / med["demux"], 3),
            "demux_vs_parse0": round(med["demux"] / med["parse0"], 3),
            "record_bytes": 32 * n,
        }), flush=True)
        del rsets, words, table, ep, counts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
