#!/usr/bin/env python3
"""yu_tx_build_ragged against what it replaces (measurement only).

Workload: n outgoing datagrams of one protocol and one payload length, the payloads
packed back to back in a payload pool, one 32-byte record per packet (random
addresses, ports, sequence numbers, flags, windows, TTL 64). The alternatives,
alternated launch by launch within one process, each timed with HIP events, medians
over --launches launches:

  build      yu_tx_build_ragged: payloads + records -> whole datagrams, both fields
  pack_fill  yu_csum_pack_fill_iov_datagram(TX_DATAGRAM) over a pre-encoded header pool
             (20 + H header bytes per packet at a 64-byte pitch) plus the same payload
             pool, two views per packet: the route a caller had before. Encoding the
             headers and uploading them is not timed, which favours this route.
  copy       a plain device copy of T bytes per packet: the floor

Before timing, build's datagrams and values are checked against the C oracle's
TX_DATAGRAM over the built bytes, and pack_fill must leave the same bytes and values.

The payload pools rotate over --sets copies, so no launch finds its bytes in the
Infinity Cache (the small workload takes at least 16). Prints one JSON line per
workload. The library's knobs apply (YU_TUNING=1 YU_NT=0|1|2, YU_BLOCKS_PER_CU).

  python tools/tx_build_bench.py [--n 1048576] [--launches 30] [--sets 2] [--workloads tcp1460,udp64]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O  # noqa: E402
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
    g = torch.Generator(device=dev).manual_seed(13)
    pays = [torch.randint(0, 256, (n * pl,), dtype=torch.uint8, device=dev, generator=g) for _ in range(sets)]
    srcs = [torch.randint(0, 256, (n * T,), dtype=torch.uint8, device=dev, generator=g) for _ in range(sets)]
    rng = np.random.default_rng(13)
    recs_h = packets.tx_records(
        n, src=rng.integers(0, 256, (n, 4), dtype=np.uint8), dst=rng.integers(0, 256, (n, 4), dtype=np.uint8),
        sport=rng.integers(0, 65536, n), dport=rng.integers(0, 65536, n), seq=rng.integers(0, 2 ** 32, n),
        ack=rng.integers(0, 2 ** 32, n), window=rng.integers(0, 65536, n), flags=0x18, proto=proto)
    recs = torch.from_numpy(recs_h.view(np.uint8).reshape(n, 32).copy()).to(dev)
    po = torch.arange(n + 1, device=dev) * pl
    do = torch.arange(n + 1, device=dev) * T
    dst = torch.zeros(n * T, dtype=torch.uint8, device=dev)
    dst2 = torch.zeros(n * T, dtype=torch.uint8, device=dev)
    dst3 = torch.zeros(n * T, dtype=torch.uint8, device=dev)
    out = torch.zeros(2 * n, dtype=torch.uint16, device=dev)
    out2 = torch.zeros(2 * n, dtype=torch.uint16, device=dev)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def build(k):
        _lib.check(L.yu_tx_build_ragged(pays[k].data_ptr(), po.data_ptr(), recs.data_ptr(), n, dst.data_ptr(),
                                        do.data_ptr(), out.data_ptr(), stream), "yu_tx_build_ragged")

    # the header pool of the old route: the headers build encodes, which do not depend
    # on the payload set but for the two fields, and those the old route fills itself
    build(0)
    hdr = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    hdr[:, :hl] = dst.view(n, T)[:, :hl]
    ar = torch.arange(n, device=dev)
    vo = torch.stack((ar * 64, ar * pl), 1).reshape(-1)
    vl = torch.tensor([hl, pl], device=dev).repeat(n)
    first = 2 * torch.arange(n + 1, device=dev)
    sel = (torch.arange(2 * n, device=dev) & 1) == 0
    tables = [torch.stack((torch.where(sel, vo + hdr.data_ptr(), vo + p.data_ptr()), vl), 1).contiguous() for p in pays]
    m = batch.MODES["tx_datagram"]

    def pack_fill(k):
        _lib.check(L.yu_csum_pack_fill_iov_datagram(tables[k].data_ptr(), first.data_ptr(), n, m, dst2.data_ptr(),
                                                    do.data_ptr(), out2.data_ptr(), stream), "pack_fill_iov_datagram")

    def copy(k):
        dst3.copy_(srcs[k])

    alts = {"build": build, "pack_fill": pack_fill, "copy": copy}
    pack_fill(0)
    torch.cuda.synchronize()
    built = dst.cpu().numpy()
    want = O.C().batch(built, m, stride=T, length=T, n=n, threads=16).reshape(-1)
    assert np.array_equal(out.cpu().numpy(), want), "build: values differ from the oracle's"
    img = built.reshape(n, T)
    f = {6: 36, 17: 26}[proto]
    w = want.reshape(n, 2)
    assert np.array_equal(img[:, 10], w[:, 0] >> 8) and np.array_equal(img[:, 11], w[:, 0] & 0xFF), "build: IPv4 field"
    assert np.array_equal(img[:, f], w[:, 1] >> 8) and np.array_equal(img[:, f + 1], w[:, 1] & 0xFF), "build: field"
    assert np.array_equal(img[:, hl:].reshape(-1), pays[0].cpu().numpy()), "build: payload bytes"
    assert torch.equal(dst, dst2) and torch.equal(out, out2), "build and pack_fill leave different datagrams"
    del built, img

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
    alg = n * (pl + T + 32 + 32)  # L read, T written, the record, two offset pairs' share and the results
    res = {
        "workload": name, "n": n, "launches": launches, "sets": sets, "proto": proto, "L": pl, "T": T,
        "variant": batch.build_variant(n), "pack_fill_variant": batch.iov_pack_datagram_variant("tx_datagram", n, True),
        "knobs": {k: v for k, v in os.environ.items() if k.startswith("YU_")},
        "us": {a: round(v, 2) for a, v in med.items()},
        "us_min": {a: round(min(t), 2) for a, t in times.items()},
        "us_max": {a: round(max(t), 2) for a, t in times.items()},
        "build_vs_pack_fill": round(med["build"] / med["pack_fill"], 3),
        "build_vs_copy": round(med["build"] / med["copy"], 3),
        "pack_fill_vs_copy": round(med["pack_fill"] / med["copy"], 3),
        "build_algorithmic_bytes": alg,
        "build_fraction_of_hbm_peak": round(alg / (med["build"] * 1e-6) / PEAK, 3),
        "copy_fraction_of_hbm_peak": round(2 * n * T / (med["copy"] * 1e-6) / PEAK, 3),
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
