"""The rule of yu_rx_stream (include/yucsum.h) restated in Python: receiver.handleRcvdSegment
of the reference (transport/tcp/rcv.go) over one endpoint's queue, with the gates of
handleSegments around it (RST, the ACK flag, the final ACK check) and the project's own
`cap`. One endpoint and one queue in, every output out. A plain module, like demux_ref.py.

All sequence arithmetic is uint32 and wraps; lt is seqnum.LessThan."""
import copy

NONE, CONSUMED, CONSUMED_LATE, PENDING, DUPLICATE, DROPPED, UNACCEPTABLE, NOOP, IGNORED, AFTER_CLOSE, RST, \
    UNPROCESSED = range(12)
STATUS_NAMES = ("NONE", "CONSUMED", "CONSUMED_LATE", "PENDING", "DUPLICATE", "DROPPED", "UNACCEPTABLE", "NOOP",
                "IGNORED", "AFTER_CLOSE", "RST", "UNPROCESSED")
FIN, SYN, F_RST, PSH, ACK = 1, 2, 4, 8, 16
OFF, OPEN, CLOSED, RESET = 0, 1, 2, 3
DEMUX_NONE = 0xFFFFFFFF
M32 = 0xFFFFFFFF
ST_FIELDS = ("rcv_nxt", "rcv_acc", "pend_used", "pend_size", "buf_size", "buf_used", "snd_nxt", "max_sent_ack",
             "pend_count", "wnd_scale", "state")


def lt(a, b):
    return ((a - b) & M32) >= 0x80000000


def new_state(rcv_nxt=1000, wnd=65535, **kw):
    """A connection as newReceiver leaves it: rcv_acc = rcv_nxt + wnd, pend_size = wnd."""
    st = dict(rcv_nxt=rcv_nxt & M32, rcv_acc=(rcv_nxt + wnd) & M32, pend_used=0, pend_size=wnd, buf_size=wnd,
              buf_used=0, snd_nxt=5000, max_sent_ack=rcv_nxt & M32, pend_count=0, wnd_scale=0, state=OPEN)
    st.update(kw)
    return st


def heap_push(heap, x):
    """container/heap.Push over segmentHeap."""
    heap.append(x)
    j = len(heap) - 1
    while True:
        i = (j - 1) // 2
        if i == j or j == 0 or not lt(heap[j]["seq"], heap[i]["seq"]):
            break
        heap[i], heap[j] = heap[j], heap[i]
        j = i


def heap_pop(heap):
    """container/heap.Pop: swap first and last, sift down over the first n - 1, remove the last."""
    n = len(heap) - 1
    heap[0], heap[n] = heap[n], heap[0]
    i = 0
    while True:
        j1 = 2 * i + 1
        if j1 >= n:
            break
        j = j1
        if j1 + 1 < n and lt(heap[j1 + 1]["seq"], heap[j1]["seq"]):
            j = j1 + 1
        if not lt(heap[j]["seq"], heap[i]["seq"]):
            break
        heap[i], heap[j] = heap[j], heap[i]
        i = j
    return heap.pop()


def walk(st, heap, cap, segs, n=None):
    """st: a dict of ST_FIELDS; heap: the list of entries {base, len, seq, pkt, flags} in array
    order; segs: the queue, dicts of pkt, proto, doff, flags, seq, base, vlen. Returns a dict:
    status {pkt: verdict}, delivered [(base, len)], st, heap, n_acks, and ack, the ACK
    record's (seq, ack, window) or None. The inputs are not changed."""
    st, heap = dict(st), copy.deepcopy(heap)
    status, delivered = {}, []
    acks = [0]
    out = dict(status=status, delivered=delivered, st=st, heap=heap, n_acks=0, ack=None)
    if not segs:
        return out
    if st["state"] in (OFF, RESET):
        for s in segs:
            status[s["pkt"]] = NONE if st["state"] == OFF else UNPROCESSED
        return out
    heap[:] = heap[:st["pend_count"]]

    def ack():
        acks[0] += 1
        avail = 0 if st["buf_used"] >= st["buf_size"] else st["buf_size"] - st["buf_used"]
        acc = (st["rcv_nxt"] + avail) & M32
        if lt(st["rcv_acc"], acc):
            st["rcv_acc"] = acc
        st["max_sent_ack"] = st["rcv_nxt"]

    def consume(seq, dlen, base, flags):
        """Returns the trimmed length, or None when the segment cannot be consumed yet."""
        if dlen > 0:
            diff = (st["rcv_nxt"] - seq) & M32
            if not diff < dlen:
                return None
            seq, dlen, base = (seq + diff) & M32, dlen - diff, base + diff
            delivered.append((base, dlen))
            st["buf_used"] = (st["buf_used"] + dlen) & M32
        elif seq != st["rcv_nxt"]:
            return None
        st["rcv_nxt"] = (seq + dlen) & M32
        if flags & FIN:
            st["rcv_nxt"] = (st["rcv_nxt"] + 1) & M32
            ack()
            st["state"] = CLOSED
        return dlen

    def logical(dlen, flags):
        return dlen + (1 if flags & SYN else 0) + (1 if flags & FIN else 0)

    stopped = False
    for s in segs:
        i = s["pkt"]
        if stopped:
            status[i] = UNPROCESSED
            continue
        opt = s["doff"] - 20
        if s["proto"] != 6 or s["doff"] < 20 or opt > s["vlen"] or s["vlen"] > 65535:
            status[i] = NONE
            continue
        if s["flags"] & F_RST:
            status[i] = RST
            st["state"] = RESET
            stopped = True
            continue
        if not s["flags"] & ACK:
            status[i] = IGNORED
            continue
        if st["state"] == CLOSED:
            status[i] = AFTER_CLOSE
            continue
        seq, dlen, base = s["seq"], s["vlen"] - opt, s["base"] + opt
        wnd = (st["rcv_acc"] - st["rcv_nxt"]) & M32
        if wnd == 0:
            ok = dlen == 0 and seq == st["rcv_nxt"]
        else:
            ok = ((seq - st["rcv_nxt"]) & M32) < wnd or \
                (lt(st["rcv_nxt"], (seq + dlen) & M32) and lt(seq, st["rcv_acc"]))
        if not ok:
            ack()
            status[i] = UNACCEPTABLE
            continue
        if consume(seq, dlen, base, s["flags"]) is None:
            if dlen > 0 or s["flags"] & FIN:
                if st["pend_used"] < st["pend_size"] and len(heap) < cap:
                    st["pend_used"] = (st["pend_used"] + logical(dlen, s["flags"])) & M32
                    heap_push(heap, dict(base=base, len=dlen, seq=seq, pkt=i, flags=s["flags"]))
                    status[i] = PENDING
                else:
                    status[i] = DROPPED
                ack()
            else:
                status[i] = NOOP
            continue
        status[i] = CONSUMED
        while st["state"] == OPEN and heap:
            t = heap[0]
            tl, late = t["len"], False
            if not lt((t["seq"] + tl - 1) & M32, st["rcv_nxt"]):
                tl = consume(t["seq"], tl, t["base"], t["flags"])
                if tl is None:
                    break
                late = True
            heap_pop(heap)
            st["pend_used"] = (st["pend_used"] - logical(tl, t["flags"])) & M32
            if t["pkt"] != DEMUX_NONE:
                status[t["pkt"]] = CONSUMED_LATE if late else DUPLICATE
    if st["state"] in (OPEN, CLOSED) and st["rcv_nxt"] != st["max_sent_ack"]:
        ack()
    for t in heap:
        t["pkt"] = DEMUX_NONE
    st["pend_count"] = len(heap)
    out["n_acks"] = acks[0]
    if acks[0]:
        w = ((st["rcv_acc"] - st["rcv_nxt"]) & M32) >> st["wnd_scale"] if st["wnd_scale"] < 32 else 0
        out["ack"] = (st["snd_nxt"], st["rcv_nxt"], min(w, 0xFFFF))
    return out
