#!/usr/bin/env python3
"""yu_rx_split_ragged against what it replaces (measurement only).

Workload: n received datagrams of one protocol and one payload length, packed back to
back (built on the device by yu_tx_build_ragged from random payloads and records, so
both checksums hold). The alternatives, alternated launch by launch within one process,
each timed with HIP events, medians over --launches launches:

  split       yu_rx_split_ragged: flags, records, pay_len and the payloads in one pass
  two_launch  yu_csum_batch_ragged(VERIFY_RX), then yu_csum_pack_iov(RAW) over a view
              table of the payload ranges (one view per packet): the route a caller had
              before. Building that table (which needs the parsed headers) and decoding
              the header fields are not timed, which favours this route; it produces no
              records at all.
  copy        a plain device copy of L bytes per packet: the floor

Before timing, split's flags, lengths, records and payloads are checked against the
batch's construction, and two_launch must leave the same flags and payload bytes.

The batches rotate over --sets copies, so no launch finds its bytes in the Infinity
Cache (the small workload takes at least 16). Prints one JSON line per workload. The
library's knobs apply (YU_TUNING=1 YU_NT=0|1|2, YU_BLOCKS_PER_CU).

  python tools/rx_split_bench.py [--n 1048576] [--launches 30] [--sets 2] [--workloads tcp1460,udp64]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yustack_amd import _lib, batch, packets  # noqa: E402

PEAK = 8.0e12  # HBM bytes/s
WORKLOADS = {"tcp1460": (6, 20, 1460), "udp64": (17, 8, 64)}  # proto, H, L


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()


def run(name, n, launches, sets, dev):
    proto, H, pl = WORKLOADS[name]
    hl, T = 20 + H, 20 + H + pl
    g = torch.Generator(device=dev).manual_seed(14)
    rng = np.random.default_rng(14)
    recs_h = packets.tx_records(
        n, src=rng.integers(0, 256, (n, 4), dtype=np.uint8), dst=rng.integers(0, 256, (n, 4), dtype=np.uint8),
        sport=rng.integers(0, 65536, n), dport=rng.integers(0, 65536, n), seq=rng.integers(0, 2 ** 32, n),
        ack=rng.integers(0, 2 ** 32, n), window=rng.integers(0, 65536, n), flags=0x18, proto=proto)
    recs_in = torch.from_numpy(recs_h.view(np.uint8).reshape(n, 32).copy()).to(dev)
    po = torch.arange(n + 1, device=dev) * pl
    offs = torch.arange(n + 1, device=dev) * T
    datas = []
    for k in range(sets):  # received batches: datagrams the sender side built
        p = torch.randint(0, 256, (n * pl,), dtype=torch.uint8, device=dev, generator=g)
        d, _, _ = batch.build_datagrams(p, po, recs_in, dst_offsets=offs)
        datas.append(d)
        if k == 0:
            pay0 = p
    srcs = [torch.randint(0, 256, (n * pl,), dtype=torch.uint8, device=dev, generator=g) for _ in range(sets)]
    pay = torch.zeros(n * pl, dtype=torch.uint8, device=dev)
    pay2 = torch.zeros(n * pl, dtype=torch.uint8, device=dev)
    pay3 = torch.zeros(n * pl, dtype=torch.uint8, device=dev)
    recs = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    plen = torch.zeros(n, dtype=torch.int32, device=dev)
    out = torch.zeros(n, dtype=torch.uint16, device=dev)
    out2 = torch.zeros(n, dtype=torch.uint16, device=dev)
    out3 = torch.zeros(n, dtype=torch.uint16, device=dev)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rx, raw = batch.MODES["verify_rx"], batch.MODES["raw"]

    def split(k):
        _lib.check(L.yu_rx_split_ragged(datas[k].data_ptr(), offs.data_ptr(), n, pay.data_ptr(), po.data_ptr(),
                                        recs.data_ptr(), plen.data_ptr(), out.data_ptr(), stream), "yu_rx_split_ragged")

    # the view table of the old route: one view per packet, its payload range
    ar = torch.arange(n, device=dev)
    first = torch.arange(n + 1, device=dev)
    tables = [torch.stack((ar * T + hl + d.data_ptr(), torch.full_like(ar, pl)), 1).contiguous() for d in datas]

    def two_launch(k):
        _lib.check(L.yu_csum_batch_ragged(datas[k].data_ptr(), offs.data_ptr(), n, rx, None, 0, None, out2.data_ptr(),
                                          stream), "yu_csum_batch_ragged")
        _lib.check(L.yu_csum_pack_iov(tables[k].data_ptr(), first.data_ptr(), n, raw, None, 0, None, pay2.data_ptr(),
                                      po.data_ptr(), out3.data_ptr(), stream), "yu_csum_pack_iov")

    def copy(k):
        pay3.copy_(srcs[k])

    alts = {"split": split, "two_launch": two_launch, "copy": copy}
    split(0)
    two_launch(0)
    torch.cuda.synchronize()
    ok = batch.RX_IP_OK | batch.RX_L4 | batch.RX_L4_OK
    assert bool((out == (ok | batch.RX_SPLIT)).all()), "split: flags"
    assert bool((out2 == ok).all()), "two_launch: flags"
    assert bool((plen == pl).all()), "split: pay_len"
    assert torch.equal(pay, pay0), "split: payload bytes"
    assert torch.equal(pay2, pay0), "two_launch: payload bytes"
    got = packets.rx_records(recs)
    want = recs_h.copy()
    if proto != 6:
        for f in ("seq", "ack", "window", "flags", "doff"):
            want[f] = 0
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), "split: records"
    del got, want

    times = {a: [] for a in alts}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in alts]
    for it in range(launches + 3):
        k = it % sets
        for (a, fn), (e0, e1) in zip(alts.items(), ev):
            timed(lambda: fn(k), e0, e1)
        torch.cuda.synchronize()
        if it >= 3:  # warm-up launches are not recorded
            for a, (e0, e1) in zip(alts, ev):
                times[a].append(e0.elapsed_time(e1) * 1e3)
    med = {a: statistics.median(t) for a, t in times.items()}
    alg = n * (T + pl + 32 + 4 + 2 + 16)  # T read, L written, the record, pay_len, out, two offset entries
    res = {
        "workload": name, "n": n, "launches": launches, "sets": sets, "proto": proto, "L": pl, "T": T,
        "variant": batch.split_variant(n),
        "two_launch_variants": [batch.ragged_variant("verify_rx", n), batch.iov_pack_variant("raw", n)],
        "knobs": {k: v for k, v in os.environ.items() if k.startswith("YU_")},
        "us": {a: round(v, 2) for a, v in med.items()},
        "us_min": {a: round(min(t), 2) for a, t in times.items()},
        "us_max": {a: round(max(t), 2) for a, t in times.items()},
        "split_vs_two_launch": round(med["split"] / med["two_launch"], 3),
        "split_vs_copy": round(med["split"] / med["copy"], 3),
        "two_launch_vs_copy": round(med["two_launch"] / med["copy"], 3),
        "split_algorithmic_bytes": alg,
        "split_fraction_of_hbm_peak": round(alg / (med["split"] * 1e-6) / PEAK, 3),
        "copy_fraction_of_hbm_peak": round(2 * n * pl / (med["copy"] * 1e-6) / PEAK, 3),
    }
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--workloads", default="tcp1460,udp64")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for w in a.workloads.split(","):
        # the small workload needs more copies to leave the Infinity Cache behind
        sets = a.sets if WORKLOADS[w][2] > 1000 else max(a.sets, 16)
        run(w, a.n, a.launches, sets, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
