"""Times yu_rx_stream alone (batch.stream_datagrams with every buffer given) on 2**20 TCP
segments of 1460 bytes: HIP events, the median of 10 launches after 3 warm-up launches, the
receivers' state put back before each launch (outside the timed span). Shapes: 65536
connections of 16 segments in order; the same with every adjacent pair swapped (every second
segment parked and drained); one connection holding the whole batch (the floor of the
wave-per-connection mapping). Run it twice for the A/B of the plain runs:

    python tools/rx_stream_bench.py
    YU_TUNING=1 YU_STREAM=walk python tools/rx_stream_bench.py

Prints one JSON line per shape."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yustack_amd import batch, packets  # noqa: E402

N, L, CAP = 1 << 20, 1460, 4


def shape(m, swapped, dev):
    per = N // m
    k = np.arange(N, dtype=np.int64) % per
    if swapped:
        k = k ^ 1
    recs = packets.tx_records(N, proto=6, flags=16, doff=20, seq=(1000 + k * L).astype(np.uint32))
    views = np.stack((0x10000 + np.arange(N, dtype=np.int64) * 2048, np.full(N, L, dtype=np.int64)), 1)
    order = torch.arange(N, dtype=torch.int32, device=dev)
    first = torch.from_numpy(np.minimum(np.arange(m + 2, dtype=np.int64) * per, N)).to(dev)
    st0 = packets.tcp_rcv(m, rcv_nxt=1000, wnd=0x7FFFFFFF)
    return (torch.from_numpy(recs.view(np.uint8).reshape(N, 32).copy()).to(dev), torch.from_numpy(views).to(dev), order,
            first, st0)


def main():
    dev = torch.device("cuda:0")
    for name, m, swapped in (("65536x16 in order", 65536, False), ("65536x16 pairs swapped", 65536, True),
                             ("1x1048576 in order", 1, False)):
        recs, views, order, first, st0 = shape(m, swapped, dev)
        st, heap = batch.tcp_receivers(m, CAP, dev, st0)
        keep = st.clone()
        NN = N + m * CAP
        bufs = dict(status=torch.empty(N, dtype=torch.uint8, device=dev),
                    s_views=torch.empty((NN, 2), dtype=torch.int64, device=dev),
                    s_offsets=torch.empty(NN + 1, dtype=torch.int64, device=dev),
                    work=torch.empty(batch.stream_workspace_bytes(N, m, CAP), dtype=torch.uint8, device=dev))
        times = []
        for it in range(13):
            st.copy_(keep)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            batch.stream_datagrams(recs, views, order, first, m, (st, heap), **bufs)
            b.record()
            torch.cuda.synchronize()
            if it >= 3:
                times.append(a.elapsed_time(b) * 1e3)
        done = int((bufs["status"] == batch.SEG_CONSUMED).sum() + (bufs["status"] == batch.SEG_CONSUMED_LATE).sum())
        print(json.dumps(dict(shape=name, variant=batch.stream_variant(N, m, CAP), median_us=round(float(np.median(times)), 1),
                              min_us=round(min(times), 1), max_us=round(max(times), 1), delivered=done)))


if __name__ == "__main__":
    main()
