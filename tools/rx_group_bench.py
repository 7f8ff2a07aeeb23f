#!/usr/bin/env python3
"""yu_rx_group against the torch grouping of demux_datagrams(group=True) (measurement only).

Input: ep, n endpoint numbers as yu_rx_demux stores them, and n payload views of 1460
bytes at a 1500-byte pitch (never dereferenced here). The shapes:

  one      m = 1, a single listener: every packet has the key 0 (one pass)
  conn64k  m = 65536 connections: the keys are a shuffle of 0 .. 65535, each 16 times at
           n = 1M (three passes)
  conn1m   m = n connections: the keys are a permutation of 0 .. n - 1 (three passes)
  miss     m = 65536, every ep is YU_DEMUX_NONE: every packet has the key m

Per shape, alternated launch by launch within one process, each timed with HIP events,
medians over --launches launches:

  group        yu_rx_group without views: order and first
  group_views  yu_rx_group with views: also q_views and q_offsets
  torch        what demux_datagrams(group=True) runs after the kernel: where, a stable
               sort of int64 keys, and the cumsum of the counts into first (the counts
               are given: yu_rx_demux's ep_count)
  read         a plain read of ep: torch's sum over it as int64 words

Before timing, order and first of the call are compared with the torch grouping's, and
q_views and q_offsets with a gather and a cumsum, over the whole batch.

ep rotates over --rsets copies. Prints one JSON line per shape. The library's knobs
apply (YU_TUNING=1 YU_BLOCKS_PER_CU).

  python tools/rx_group_bench.py [--n 1048576] [--launches 30] [--rsets 8] [--shapes one,conn64k,conn1m,miss]
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
from yustack_amd import _lib, batch  # noqa: E402


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--rsets", type=int, default=8)
    ap.add_argument("--shapes", default="one,conn64k,conn1m,miss")
    a = ap.parse_args()
    n, dev = a.n, torch.device("cuda:0")
    rng = np.random.default_rng(18)
    c64 = min(65536, n)
    shapes = {"one": (1, np.zeros(n, dtype=np.uint32)),
              "conn64k": (c64, (rng.permutation(n) % c64).astype(np.uint32)),
              "conn1m": (n, rng.permutation(n).astype(np.uint32)),
              "miss": (c64, np.full(n, batch.DEMUX_NONE, dtype=np.uint32))}
    i64 = dict(dtype=torch.int64, device=dev)
    views = torch.stack((0x7000_0000_0000 + 40 + 1500 * torch.arange(n, **i64), torch.full((n,), 1460, **i64)), 1)
    views = views.contiguous()
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(4)]
    for name in a.shapes.split(","):
        m, ep_h = shapes[name]
        eps = [torch.from_numpy(ep_h.view(np.int32)).to(dev).view(torch.uint32) for _ in range(a.rsets)]
        words = [e.view(torch.int64) for e in eps]
        key_h = np.minimum(ep_h.astype(np.int64), m)
        counts = torch.from_numpy(np.bincount(key_h, minlength=m + 1).astype(np.int32)).to(dev).view(torch.uint32)
        order = torch.zeros(n, dtype=torch.int32, device=dev)
        first = torch.zeros(m + 2, **i64)
        q_views, q_offsets = torch.zeros((n, 2), **i64), torch.zeros(n + 1, **i64)
        work = torch.zeros(batch.group_workspace_bytes(n, m), dtype=torch.uint8, device=dev)
        sink = []

        def group(with_views):
            def fn(it):
                v = with_views
                _lib.check(L.yu_rx_group(eps[it % len(eps)].data_ptr(), n, m, views.data_ptr() if v else None,
                                         order.data_ptr(), first.data_ptr(), q_views.data_ptr() if v else None,
                                         q_offsets.data_ptr() if v else None, work.data_ptr(), work.numel(), stream),
                           "yu_rx_group")
            return fn

        def torch_grouping(it):  # batch.demux_datagrams, group=True, after its kernel
            ep = eps[it % len(eps)]
            key = ep.view(torch.int32).to(torch.int64)
            t_order = torch.sort(torch.where(key < 0, m, key), stable=True).indices
            t_first = torch.zeros(m + 2, dtype=torch.int64, device=dev)
            t_first[1:] = torch.cumsum(counts.view(torch.int32).to(torch.int64), 0)
            sink[:] = [t_order, t_first]

        def read(it):
            sink[:] = [words[it % len(words)].sum()]

        # the whole batch against the torch grouping before timing
        group(True)(0)
        torch_grouping(0)
        t_order, t_first = sink
        torch.cuda.synchronize()
        assert torch.equal(order.long(), t_order), f"{name}: order"
        assert torch.equal(first, t_first), f"{name}: first"
        kept = int(t_first[m])
        want_v = views[t_order].clone()
        want_v[kept:] = 0
        assert torch.equal(q_views, want_v), f"{name}: q_views"
        assert torch.equal(q_offsets[1:], want_v[:, 1].cumsum(0)) and int(q_offsets[0]) == 0, f"{name}: q_offsets"
        del t_order, t_first, want_v
        sink.clear()

        alts = {"group": group(False), "group_views": group(True), "torch": torch_grouping, "read": read}
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
            "shape": name, "n": n, "m": m, "delivered": kept, "work_bytes": work.numel(), "launches": a.launches,
            "rsets": len(eps), "variant": batch.group_variant(n, m),
            "knobs": {k: v for k, v in os.environ.items() if k.startswith("YU_")},
            "us": {k: round(v, 2) for k, v in med.items()},
            "us_min": {k: round(min(t), 2) for k, t in times.items()},
            "us_max": {k: round(max(t), 2) for k, t in times.items()},
            "group_vs_torch": round(med["group"] / med["torch"], 3),
            "group_views_vs_torch": round(med["group_views"] / med["torch"], 3),
            "group_vs_read": round(med["group"] / med["read"], 3),
            "group_views_vs_group": round(med["group_views"] / med["group"], 3),
        }), flush=True)
        del eps, words, counts, order, first, q_views, q_offsets, work
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
