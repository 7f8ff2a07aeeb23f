#!/usr/bin/env python3
"""Scatter-gather device batches against what they replace (measurement only).

Workload: n packets, each a header view (hdr bytes, in a header pool with a 64-byte
pitch) and a payload view (pay bytes, in a payload pool), TCP or UDP with `addrs`.
The alternatives, alternated launch by launch within one process, each timed with
HIP events, medians over --launches launches:

  iov         yu_csum_batch_iov on a prebuilt device table (the call a C user makes)
  iov_py      batch.checksum_iov(validate=False): the same plus building the table
  pack+sum    the two pools packed into one contiguous buffer (torch.cat of the strided
              header slice and the payload), then checksum_uniform: what the caller
              had to do before
  packed      checksum_uniform on bytes already packed: the floor
  pack_fused  yu_csum_pack_iov on the same table into a preallocated dst and offsets:
              the sums and the packed copy in one launch (what pack+sum delivers in
              two); its dst and values are checked against the oracle before timing

Whole-datagram workloads (yu_csum_batch_iov_datagram / yu_csum_fill_iov_datagram): n
1500-byte TCP datagrams, each a 40-byte header view (IPv4 + TCP header) and a 1460-byte
payload view; rx1500 is VERIFY_RX, tx1500 TX_DATAGRAM in place. The alternatives are the
same four, with the ragged-form modes on the packed copy (tx1500's pack+sum leaves its
fields in the copy: scattering them back to the views is not charged to it), and two that
deliver the packed datagrams as well as the results:

  pack_fused        yu_csum_pack_iov_datagram / yu_csum_pack_fill_iov_datagram into a
                    preallocated dst: one launch
  pack_then_ragged  yu_csum_pack_iov(RAW) into a preallocated dst, then yu_csum_batch_ragged /
                    yu_csum_fill_ragged on the copy: what took two launches before

Their results and dst bytes are asserted equal before timing.

The pools rotate over --sets copies (more than 2 GiB in all for the MTU workload), so
no launch finds its bytes in the Infinity Cache. Prints one JSON line per workload.
The library's knobs apply (YU_TUNING=1 YU_NT=0|1|2, YU_BLOCKS_PER_CU): run it once
per setting to compare load policies and grids.

  python tools/iov_bench.py [--n 1048576] [--launches 30] [--sets 2] [--workloads tcp1500,udp72,rx1500,tx1500]
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
from yustack_amd import _lib, batch  # noqa: E402

PEAK = 8.0e12  # HBM bytes/s
WORKLOADS = {"tcp1500": ("tcp", 20, 1480), "udp72": ("udp", 8, 64)}
DATAGRAM_WORKLOADS = {"rx1500": ("verify_rx", 40, 1460, False), "tx1500": ("tx_datagram", 40, 1460, True)}


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()


def run(name, n, launches, sets, dev):
    mode, hl, pl = WORKLOADS[name]
    g = torch.Generator(device=dev).manual_seed(1)
    hdrs = [torch.randint(0, 256, (n, 64), dtype=torch.uint8, device=dev, generator=g) for _ in range(sets)]
    pays = [torch.randint(0, 256, (n, pl), dtype=torch.uint8, device=dev, generator=g) for _ in range(sets)]
    for h in hdrs:
        h[:, 12] = 0x50
    packed = [torch.cat((h[:, :hl], p), 1).contiguous() for h, p in zip(hdrs, pays)]
    addrs = torch.randint(0, 256, (8 * n,), dtype=torch.uint8, device=dev, generator=g)
    ar = torch.arange(n, device=dev)
    vp = torch.stack((torch.zeros_like(ar), torch.ones_like(ar)), 1).reshape(-1)
    vo = torch.stack((ar * 64, ar * pl), 1).reshape(-1)
    vl = torch.tensor([hl, pl], device=dev).repeat(n)
    first = 2 * torch.arange(n + 1, device=dev)
    tables = [torch.stack((torch.where(vp == 0, vo + h.data_ptr(), vo + p.data_ptr()), vl), 1).contiguous()
              for h, p in zip(hdrs, pays)]
    out = torch.zeros(n, dtype=torch.uint16, device=dev)
    L, m = _lib.lib(), batch.MODES[mode]
    stream = torch.cuda.current_stream(dev).cuda_stream
    ln = hl + pl
    dst = torch.zeros(n * ln, dtype=torch.uint8, device=dev)
    dst_offsets = torch.arange(n + 1, device=dev) * ln

    def iov(k):
        _lib.check(L.yu_csum_batch_iov(tables[k].data_ptr(), first.data_ptr(), n, m, None, 0, addrs.data_ptr(),
                                       out.data_ptr(), stream), "yu_csum_batch_iov")

    def iov_py(k):
        batch.checksum_iov([hdrs[k].view(-1), pays[k].view(-1)], vp, vo, vl, first, mode, addrs=addrs, out=out,
                           validate=False)

    def pack_sum(k):
        buf = torch.cat((hdrs[k][:, :hl], pays[k]), 1)
        batch.checksum_uniform(buf.view(-1), ln, ln, n, mode, addrs=addrs, out=out)

    def floor(k):
        batch.checksum_uniform(packed[k].view(-1), ln, ln, n, mode, addrs=addrs, out=out)

    def pack_fused(k):
        _lib.check(L.yu_csum_pack_iov(tables[k].data_ptr(), first.data_ptr(), n, m, None, 0, addrs.data_ptr(),
                                      dst.data_ptr(), dst_offsets.data_ptr(), out.data_ptr(), stream),
                   "yu_csum_pack_iov")

    alts = {"iov": iov, "iov_py": iov_py, "pack+sum": pack_sum, "packed": floor, "pack_fused": pack_fused}
    # every alternative computes the same values, and they are the oracle's
    want = None
    for a, fn in alts.items():
        out.zero_()
        fn(0)
        got = out.cpu().numpy().copy()
        if want is None:
            want = O.C().batch(packed[0].cpu().numpy().reshape(-1), m, stride=ln, length=ln, n=n,
                               addrs=addrs.cpu().numpy(), threads=16)
        assert np.array_equal(got, want), a
    assert torch.equal(dst, packed[0].view(-1)), "pack_fused: dst is not the packed bytes"
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
    alg = n * (ln + 2 * 16 + 8 + 8 + 2)  # packet bytes, two view records, first_iov, addrs, result
    res = {
        "workload": name, "n": n, "launches": launches, "sets": sets,
        "pool_bytes": sets * n * (64 + pl),
        "variant": batch.iov_variant(mode, n), "floor_variant": batch.variant(ln, ln, mode, 0, n),
        "knobs": {k: v for k, v in os.environ.items() if k.startswith("YU_")},
        "us": {a: round(v, 2) for a, v in med.items()},
        "us_min": {a: round(min(t), 2) for a, t in times.items()},
        "iov_vs_pack_sum": round(med["iov"] / med["pack+sum"], 3),
        "iov_vs_floor": round(med["iov"] / med["packed"], 3),
        "pack_variant": batch.iov_pack_variant(mode, n),
        "pack_fused_vs_pack_sum": round(med["pack_fused"] / med["pack+sum"], 3),
        "pack_fused_vs_floor": round(med["pack_fused"] / med["packed"], 3),
        "iov_algorithmic_bytes": alg,
        "iov_fraction_of_hbm_peak": round(alg / (med["iov"] * 1e-6) / PEAK, 3),
        "floor_fraction_of_hbm_peak": round(n * (ln + 8 + 2) / (med["packed"] * 1e-6) / PEAK, 3),
        # one read of the views and tables, one write of the copy
        "pack_fused_fraction_of_hbm_peak": round((alg + n * (ln + 16)) / (med["pack_fused"] * 1e-6) / PEAK, 3),
    }
    print(json.dumps(res), flush=True)
    return res


def run_datagram(name, n, launches, sets, dev):
    mode, hl, pl, fill = DATAGRAM_WORKLOADS[name]
    ln = hl + pl
    g = torch.Generator(device=dev).manual_seed(2)
    hdrs = [torch.randint(0, 256, (n, 64), dtype=torch.uint8, device=dev, generator=g) for _ in range(sets)]
    pays = [torch.randint(0, 256, (n, pl), dtype=torch.uint8, device=dev, generator=g) for _ in range(sets)]
    for h in hdrs:  # IHL 5, TotalLength = ln, TCP, DataOffset 5
        h[:, 0], h[:, 2], h[:, 3], h[:, 9], h[:, 32] = 0x45, ln >> 8, ln & 0xFF, 6, 0x50
    packed = [torch.cat((h[:, :hl], p), 1).contiguous() for h, p in zip(hdrs, pays)]
    ar = torch.arange(n, device=dev)
    vp = torch.stack((torch.zeros_like(ar), torch.ones_like(ar)), 1).reshape(-1)
    vo = torch.stack((ar * 64, ar * pl), 1).reshape(-1)
    vl = torch.tensor([hl, pl], device=dev).repeat(n)
    first = 2 * torch.arange(n + 1, device=dev)
    tables = [torch.stack((torch.where(vp == 0, vo + h.data_ptr(), vo + p.data_ptr()), vl), 1).contiguous()
              for h, p in zip(hdrs, pays)]
    L, m = _lib.lib(), batch.MODES[mode]
    k_out = batch.outputs(m)
    out = torch.zeros(n * k_out, dtype=torch.uint16, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    call = L.yu_csum_fill_iov_datagram if fill else L.yu_csum_batch_iov_datagram

    def iov(k):
        _lib.check(call(tables[k].data_ptr(), first.data_ptr(), n, m, out.data_ptr(), stream), "iov_datagram")

    def iov_py(k):
        batch.checksum_iov_datagrams([hdrs[k].view(-1), pays[k].view(-1)], vp, vo, vl, first, mode, out=out,
                                     fill=fill, validate=False)

    def pack_sum(k):
        buf = torch.cat((hdrs[k][:, :hl], pays[k]), 1)
        batch.checksum_uniform(buf.view(-1), ln, ln, n, mode, out=out, fill=fill)

    def floor(k):
        batch.checksum_uniform(packed[k].view(-1), ln, ln, n, mode, out=out, fill=fill)

    dst = torch.zeros(n * ln, dtype=torch.uint8, device=dev)
    dst2 = torch.zeros(n * ln, dtype=torch.uint8, device=dev)
    dst_offsets = torch.arange(n + 1, device=dev) * ln
    raw = torch.zeros(n, dtype=torch.uint16, device=dev)
    pack_call = L.yu_csum_pack_fill_iov_datagram if fill else L.yu_csum_pack_iov_datagram
    ragged_call = L.yu_csum_fill_ragged if fill else L.yu_csum_batch_ragged

    def pack_fused(k):
        _lib.check(pack_call(tables[k].data_ptr(), first.data_ptr(), n, m, dst.data_ptr(), dst_offsets.data_ptr(),
                             out.data_ptr(), stream), "pack_iov_datagram")

    def pack_then_ragged(k):
        _lib.check(L.yu_csum_pack_iov(tables[k].data_ptr(), first.data_ptr(), n, batch.MODES["raw"], None, 0, None,
                                      dst2.data_ptr(), dst_offsets.data_ptr(), raw.data_ptr(), stream),
                   "yu_csum_pack_iov")
        _lib.check(ragged_call(dst2.data_ptr(), dst_offsets.data_ptr(), n, m, None, 0, None, out.data_ptr(), stream),
                   "ragged on the copy")

    alts = {"iov": iov, "iov_py": iov_py, "pack+sum": pack_sum, "packed": floor, "pack_fused": pack_fused,
            "pack_then_ragged": pack_then_ragged}
    # every alternative computes the same values, and they are the oracle's (the
    # fields a fill stores are taken as zero by the mode, so a second pass agrees)
    want = O.C().batch(packed[0].cpu().numpy().reshape(-1), m, stride=ln, length=ln, n=n, threads=16).reshape(-1)
    for a, fn in alts.items():
        out.zero_()
        fn(0)
        assert np.array_equal(out.cpu().numpy(), want), a
    # the two packing alternatives leave the same bytes: the datagrams, in the fill
    # workload with both fields in each (packed[0] got them from `packed` above)
    assert torch.equal(dst, dst2), "pack_fused and pack_then_ragged leave different bytes"
    assert torch.equal(dst, packed[0].view(-1)), "pack_fused: dst is not the packed datagrams"
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
    alg = n * (ln + 2 * 16 + 8 + 2 * k_out + (4 if fill else 0))  # bytes, view records, first_iov, results, fields
    res = {
        "workload": name, "n": n, "launches": launches, "sets": sets,
        "pool_bytes": sets * n * (64 + pl),
        "variant": batch.iov_datagram_variant(mode, n, fill), "floor_variant": batch.variant(ln, ln, mode, 0, n),
        "knobs": {k: v for k, v in os.environ.items() if k.startswith("YU_")},
        "us": {a: round(v, 2) for a, v in med.items()},
        "us_min": {a: round(min(t), 2) for a, t in times.items()},
        "us_max": {a: round(max(t), 2) for a, t in times.items()},
        "iov_vs_pack_sum": round(med["iov"] / med["pack+sum"], 3),
        "iov_vs_floor": round(med["iov"] / med["packed"], 3),
        "iov_algorithmic_bytes": alg,
        "iov_fraction_of_hbm_peak": round(alg / (med["iov"] * 1e-6) / PEAK, 3),
        "pack_variant": batch.iov_pack_datagram_variant(mode, n, fill),
        "pack_fused_vs_pack_then_ragged": round(med["pack_fused"] / med["pack_then_ragged"], 3),
        "pack_fused_vs_pack_sum": round(med["pack_fused"] / med["pack+sum"], 3),
        # one read of the views and tables, one write of the copy
        "pack_fused_fraction_of_hbm_peak": round((alg + n * (ln + 16)) / (med["pack_fused"] * 1e-6) / PEAK, 3),
    }
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--workloads", default="tcp1500,udp72")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for w in a.workloads.split(","):
        if w in DATAGRAM_WORKLOADS:
            run_datagram(w, a.n, a.launches, a.sets, dev)
        else:
            # the small workload needs more copies to leave the Infinity Cache behind
            sets = a.sets if WORKLOADS[w][2] > 1000 else max(a.sets, 16)
            run(w, a.n, a.launches, sets, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
