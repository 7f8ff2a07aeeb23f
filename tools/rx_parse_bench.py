#!/usr/bin/env python3
"""yu_rx_parse_ragged against its neighbours (measurement only).

Workload: tools/rx_split_bench.py's, built the same way: n received datagrams of one
protocol and one payload length, packed back to back (built on the device by
yu_tx_build_ragged from random payloads and records, so both checksums hold). The
alternatives, alternated launch by launch within one process, each timed with HIP
events, medians over --launches launches:

  parse1  yu_rx_parse_ragged(verify=1): VERIFY_RX's launch, then the header pass
  parse0  yu_rx_parse_ragged(verify=0): the header pass alone
  split   yu_rx_split_ragged: the same flags and records, and the payloads copied out
  verify  yu_csum_batch_ragged(VERIFY_RX) alone: what parse1's first launch costs
  read    a plain read of the batch: torch's sum over its bytes as int64 words

Before timing, parse1's and parse0's flags, records and views are checked against the
batch's construction, and split must leave the same flags and records.

The batches rotate over --sets copies, so no launch finds its bytes in the Infinity
Cache (the small workload takes at least 16). Prints one JSON line per workload. The
library's knobs apply (YU_TUNING=1 YU_NT=0|1, YU_BLOCKS_PER_CU).

  python tools/rx_parse_bench.py [--n 1048576] [--launches 30] [--sets 2] [--workloads tcp1460,udp64]
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
    g = torch.Generator(device=dev).manual_seed(16)
    rng = np.random.default_rng(16)
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
    del p
    assert (n * T) % 8 == 0
    words = [d.view(torch.int64) for d in datas]
    pay = torch.zeros(n * pl, dtype=torch.uint8, device=dev)
    recs = {a: torch.zeros((n, 32), dtype=torch.uint8, device=dev) for a in ("parse1", "parse0", "split")}
    views = {a: torch.zeros((n, 2), dtype=torch.int64, device=dev) for a in ("parse1", "parse0")}
    outs = {a: torch.zeros(n, dtype=torch.uint16, device=dev) for a in ("parse1", "parse0", "split", "verify")}
    plen = torch.zeros(n, dtype=torch.int32, device=dev)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rx = batch.MODES["verify_rx"]

    def parse(a, verify):
        def fn(k):
            _lib.check(L.yu_rx_parse_ragged(datas[k].data_ptr(), offs.data_ptr(), n, verify, recs[a].data_ptr(),
                                            views[a].data_ptr(), outs[a].data_ptr(), stream), "yu_rx_parse_ragged")
        return fn

    def split(k):
        _lib.check(L.yu_rx_split_ragged(datas[k].data_ptr(), offs.data_ptr(), n, pay.data_ptr(), po.data_ptr(),
                                        recs["split"].data_ptr(), plen.data_ptr(), outs["split"].data_ptr(), stream),
                   "yu_rx_split_ragged")

    def verify(k):
        _lib.check(L.yu_csum_batch_ragged(datas[k].data_ptr(), offs.data_ptr(), n, rx, None, 0, None,
                                          outs["verify"].data_ptr(), stream), "yu_csum_batch_ragged")

    sink = []

    def read(k):
        sink[:] = [words[k].sum()]

    alts = {"parse1": parse("parse1", 1), "parse0": parse("parse0", 0), "split": split, "verify": verify,
            "read": read}
    for fn in alts.values():
        fn(0)
    torch.cuda.synchronize()
    ok = batch.RX_IP_OK | batch.RX_L4 | batch.RX_L4_OK
    assert bool((outs["parse1"] == (ok | batch.RX_SPLIT)).all()), "parse1: flags"
    assert bool((outs["parse0"] == batch.RX_SPLIT).all()), "parse0: flags"
    assert bool((outs["split"] == (ok | batch.RX_SPLIT)).all()), "split: flags"
    assert bool((outs["verify"] == ok).all()), "verify: flags"
    want = recs_h.copy()
    if proto != 6:
        for f in ("seq", "ack", "window", "flags", "doff"):
            want[f] = 0
    want_views = torch.stack((offs[:-1] + hl + datas[0].data_ptr(), torch.full_like(offs[:-1], pl)), 1)
    for a in ("parse1", "parse0", "split"):
        assert np.array_equal(packets.rx_records(recs[a]).view(np.uint8), want.view(np.uint8)), f"{a}: records"
    for a in ("parse1", "parse0"):
        assert torch.equal(views[a], want_views), f"{a}: views"
    del want, want_views

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
    hdr = n * (32 + 16 + 2 + 16)  # the record, the view, out, two offset entries
    res = {
        "workload": name, "n": n, "launches": launches, "sets": sets, "proto": proto, "L": pl, "T": T,
        "variant": batch.parse_variant(n),
        "verify_variant": batch.ragged_variant("verify_rx", n), "split_variant": batch.split_variant(n),
        "knobs": {k: v for k, v in os.environ.items() if k.startswith("YU_")},
        "us": {a: round(v, 2) for a, v in med.items()},
        "us_min": {a: round(min(t), 2) for a, t in times.items()},
        "us_max": {a: round(max(t), 2) for a, t in times.items()},
        "parse1_vs_split": round(med["parse1"] / med["split"], 3),
        "parse1_vs_verify": round(med["parse1"] / med["verify"], 3),
        "parse1_minus_verify_us": round(med["parse1"] - med["verify"], 2),
        "parse0_vs_read": round(med["parse0"] / med["read"], 3),
        "parse0_stored_bytes": hdr,
        "read_fraction_of_hbm_peak": round(n * T / (med["read"] * 1e-6) / PEAK, 3),
        "verify_fraction_of_hbm_peak": round(n * T / (med["verify"] * 1e-6) / PEAK, 3),
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
