"""The case grid of yu_rx_stream for the GPU tests and the golden generator: one TCP
connection's initial state, carried heap and queue of segments per case, as plain Python
values for stream_ref.walk. A plain module, like kernel_cases.py.

Addresses are offsets: queue segment k's view starts at ``k * PITCH`` of a notional
buffer, a carried heap entry h's data at ``(HEAP_AT + h) * PITCH``; the GPU tests add a
device pointer."""
import numpy as np

import stream_ref as R

PITCH = 2048
HEAP_AT = 200           # queues hold fewer segments than this
LENS = (0, 1, 2, 63, 64, 65, 130)
CAPS = (0, 1, 4)
KINDS = ("in_order", "swap", "gap", "gap_filled_last", "duplicates", "overlap", "overshoot", "zero_window",
         "zero_window_reopens", "fin_in_order", "fin_parked", "fin_only_parked", "data_after_fin", "rst_middle",
         "no_ack_flag", "pure_acks", "doff32", "wrap", "byte_budget", "full_cap", "state0", "state2", "state3",
         "carried_heap", "shuffle", "not_tcp")


def seg(seq, dlen, flags=R.ACK, doff=20, proto=6):
    return dict(proto=proto, doff=doff, flags=flags, seq=seq & R.M32, vlen=dlen + (doff - 20))


def dl(s):
    return s["vlen"] - (s["doff"] - 20)


def scenario(kind, L, cap, rng):
    """Returns (st, heap, segs): segs without pkt and base, which place() assigns."""
    nxt = 0xFFFFFF00 if kind == "wrap" else 1000 + int(rng.integers(0, 1 << 20))
    st = R.new_state(nxt, 1 << 20, snd_nxt=5000 + int(rng.integers(0, 1 << 16)), wnd_scale=int(rng.integers(0, 3)))
    heap = []
    total = L + (2 if kind == "carried_heap" else 0)
    s, seq = [], nxt
    for _ in range(total):
        d = 1 + int(rng.integers(0, 1460))
        doff = 32 if kind == "doff32" or rng.integers(0, 5) == 0 else 20
        s.append(seg(seq, d, R.ACK | (R.PSH if rng.integers(0, 2) else 0), doff))
        seq += d
    if kind == "swap" and L >= 2:
        i = L // 2 - (1 if L // 2 == L - 1 else 0)
        s[i], s[i + 1] = s[i + 1], s[i]
    elif kind == "gap":
        for x in s[L // 3 + 1:]:
            x["seq"] = (x["seq"] + 100) & R.M32
    elif kind == "gap_filled_last" and L >= 2:
        s.append(s.pop(L // 3))
    elif kind == "duplicates":
        for i in range(1, L, 3):
            s[i] = dict(s[i - 1])
    elif kind == "overlap":
        for i in range(1, L, 2):
            back = 1 + int(rng.integers(0, 3))
            s[i]["seq"] = (s[i]["seq"] - back) & R.M32
            s[i]["vlen"] += back
        if L >= 4:
            s[2], s[3] = s[3], s[2]
    elif kind == "overshoot":
        half = sum(dl(x) for x in s[:L // 2])
        st["rcv_acc"], st["buf_size"] = (nxt + half + 1) & R.M32, half + 1
    elif kind in ("zero_window", "zero_window_reopens"):
        st["rcv_acc"] = nxt
        if kind == "zero_window":
            st["buf_used"] = st["buf_size"]
        if L >= 2:
            s[1] = seg(nxt, 0)
    elif kind == "fin_in_order" and L:
        s[-1]["flags"] |= R.FIN
    elif kind == "fin_parked" and L:
        s[-1]["flags"] |= R.FIN
        if L >= 2:
            s[-1], s[-2] = s[-2], s[-1]
    elif kind == "fin_only_parked" and L >= 2:
        s[-1] = seg(s[-1]["seq"], 0, R.ACK | R.FIN)
        s[-1], s[-2] = s[-2], s[-1]
    elif kind == "data_after_fin" and L:
        s[L // 2]["flags"] |= R.FIN
        for x in s[L // 2 + 1:]:
            x["seq"] = (x["seq"] + 1) & R.M32
    elif kind == "rst_middle" and L:
        s[L // 2]["flags"] |= R.F_RST
    elif kind == "no_ack_flag" and L:
        s[L // 2]["flags"] &= ~R.ACK
    elif kind == "pure_acks":
        q = nxt
        for i, x in enumerate(s):
            if i % 3 == 0:
                s[i] = seg(q + (5 if i % 2 else 0), 0, R.ACK, x["doff"])
            else:
                x["seq"] = q & R.M32
                q += dl(x)
    elif kind == "byte_budget":
        s.reverse()
        st["pend_size"] = 2000
    elif kind == "full_cap":
        s.reverse()
    elif kind in ("state0", "state2", "state3"):
        st["state"] = int(kind[-1])
    elif kind == "carried_heap":
        rest, a, b = [], total // 2, total - 1
        for i, x in enumerate(s):
            if i in (a, b) and i > 0 and len(heap) < cap:
                R.heap_push(heap, dict(base=(HEAP_AT + len(heap)) * PITCH + x["doff"] - 20, len=dl(x), seq=x["seq"],
                                       pkt=R.DEMUX_NONE, flags=x["flags"]))
                st["pend_used"] += dl(x)
            else:
                rest.append(x)
        s = rest
        st["pend_count"] = len(heap)
    elif kind == "shuffle":
        for i in range(L, 1, -1):
            if rng.integers(0, 3) == 0:
                j = int(rng.integers(0, i))
                s[i - 1], s[j] = s[j], s[i - 1]
    elif kind == "not_tcp":
        if L:
            s[L // 2]["proto"] = 17
        if L > 2:
            s[1]["doff"] = 16
        if L > 3:
            s[2]["vlen"] = 65536
        if L > 4:
            s[3] = dict(proto=6, doff=60, flags=R.ACK, seq=s[3]["seq"], vlen=39)
    return st, heap, s[:L]


def place(segs, pkts=None, origin=0):
    """The queue with packet numbers (0 .. L-1, or ``pkts``); packet p's view starts at
    ``origin + p * PITCH``."""
    pkts = range(len(segs)) if pkts is None else [int(p) for p in pkts]
    return [dict(x, pkt=p, base=origin + p * PITCH) for x, p in zip(segs, pkts)]


def grid(seed=20261021):
    """(name, cap, st, heap, segs) for every kind, queue length and capacity."""
    rng = np.random.default_rng(seed)
    for kind in KINDS:
        for L in LENS:
            for cap in CAPS:
                st, heap, segs = scenario(kind, L, cap, rng)
                yield f"{kind}-L{L}-cap{cap}", cap, st, heap, segs
