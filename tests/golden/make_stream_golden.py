"""Writes tests/golden/tcp_stream.json: vectors for yu_rx_stream, one TCP connection each:
the initial state, the carried heap, the segments (seq, view length, flags, doff, proto)
and every expected output of the rule in include/yucsum.h.

A vector marked ``executed`` has its receiver outputs (st_out, heap_out, delivered, n_acks,
ack) from the reference's own receiver.handleRcvdSegment, consumeSegment, acceptable and
getSendParams (transport/tcp/rcv.go) and segment.logicalLen / flagIsSet (segment.go), run by
goexec.py, one call per segment that passes the gates. Around the executed text stand, as
Python and marked RESTATED below:
  * r.ep: readyToRead, receiveBufferAvailable and snd.sendAck (which calls the executed
    getSendParams and records maxSentAck), and the segment's data as (address, length);
  * container/heap's Push and Pop over pendingRcvdSegments, with the executed
    seqnum.LessThan as Less (segment_heap.go takes interface{} parameters, outside the
    interpreter's subset);
  * two things outside the subset, added in a subclass of the interpreter here, goexec.py
    staying as it is: the `break` of the drain loop, and a pointer-receiver method changing
    a named integer in the caller's variable (seqnum.Value.UpdateForward);
  * the gates of handleSegments (state, the usable-record test, RST, the ACK flag, closed,
    the final ACK check) and the project's own `cap` (a full heap reads as a full byte budget).
The verdict names (``status``) are this project's, not the reference's; they come from
tests/stream_ref.py in every vector, and the generator refuses to write a vector whose
executed outputs differ from that model's. Vectors whose connection is in state 0 or 3 at
entry never reach the receiver and are marked ``restated``.

The ACK datagrams are the executed sendTCP's (make_refexec.Ref.send_tcp).

Run from the repository root, with the reference's source tree present:
python tests/golden/make_stream_golden.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import goexec as G  # noqa: E402
import make_refexec  # noqa: E402
import stream_cases as C  # noqa: E402
import stream_ref as R  # noqa: E402

LOCAL, REMOTE, LPORT, RPORT = bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2]), 80, 40000


class Break(Exception):
    pass


class Interp(G.Interp):
    """goexec's interpreter plus `break` and UpdateForward's write-back (RESTATED: see above)."""

    def _eval(self, e, env, pkg):
        if e[0] == "name" and e[1] == "break":
            raise Break()
        if e[0] == "call" and e[1][0] == "sel" and e[1][2] == "UpdateForward":  # func (v *Value): *v += Value(s)
            cur, d = self._eval(e[1][1], env, pkg), self._eval(e[2][0], env, pkg)
            self._store(e[1][1], G.Int((cur.v + d.v) & R.M32, cur.t), env, pkg)
            return None
        return super()._eval(e, env, pkg)

    def _exec(self, s, env, pkg):
        if s[0] != "for":
            return super()._exec(s, env, pkg)
        try:
            return super()._exec(s, env, pkg)
        except Break:
            return None


def load(root=make_refexec.REF):
    it = Interp(root)
    it.load("seqnum", ["seqnum.go"])
    it.load("buffer", ["view.go", "prependable.go"])
    it.load("types", ["types.go", "route.go", "transport.go", "network.go"])
    it.load("header", ["ipv4.go", "tcp.go", "udp.go", "icmpv4.go"])
    it.load("transport/tcp", ["rcv.go", "segment.go"])
    return it


class Data:  # RESTATED: buffer.VectorisedView as (address, length)
    def __init__(self, base, n):
        self.base, self.n = base, n

    def Size(self):  # noqa: N802
        return G.Int(self.n, "int")

    def TrimFront(self, k):  # noqa: N802
        self.base += k.v
        self.n -= k.v


class Heap:  # RESTATED: segmentHeap's array
    def __init__(self):
        self.a = []

    def Len(self):  # noqa: N802
        return G.Int(len(self.a), "int")

    def get(self, i):
        return self.a[i.v if isinstance(i, G.Int) else i]

    @property
    def len(self):
        return len(self.a)


class Snd:  # RESTATED: sender.sendAck -> getSendParams, maxSentAck
    def __init__(self, ep):
        self.ep = ep

    def sendAck(self):  # noqa: N802
        self.ep.acks += 1
        self.ep.it.method("tcp", self.ep.r, "getSendParams")
        self.ep.max_sent_ack = self.ep.r.f["rcvNxt"].v


class Ep:  # RESTATED: endpoint.readyToRead, receiveBufferAvailable
    def __init__(self, it, st):
        self.it, self.acks, self.delivered = it, 0, []
        self.buf_size, self.buf_used, self.max_sent_ack = st["buf_size"], st["buf_used"], st["max_sent_ack"]
        self.snd = Snd(self)

    def readyToRead(self, seg):  # noqa: N802
        if seg is not None:
            d = seg.f["data"]
            self.delivered.append((d.base, d.n))
            self.buf_used = (self.buf_used + d.n) & R.M32

    def receiveBufferAvailable(self):  # noqa: N802
        return G.Int(0 if self.buf_used >= self.buf_size else self.buf_size - self.buf_used, "int")


def executed(it, st, heap0, cap, segs):
    """The receiver outputs of one queue from the executed rcv.go; None for a connection that
    never reaches the receiver (state 0 or 3 at entry)."""
    if st["state"] in (R.OFF, R.RESET) or not segs:
        return None
    tcp = it.pkgs["tcp"]
    val = lambda v: G.Int(v & R.M32, "Value")  # noqa: E731
    size = lambda v: G.Int(v & R.M32, "Size")  # noqa: E731
    ep, h = Ep(it, st), Heap()
    r = it._zero("receiver", tcp)
    ep.r = r
    r.f.update(ep=ep, rcvNxt=val(st["rcv_nxt"]), rcvAcc=val(st["rcv_acc"]), rcvWndScale=G.Int(st["wnd_scale"], "uint8"),
               closed=st["state"] == R.CLOSED, pendingRcvdSegments=h, pendingBufUsed=size(st["pend_used"]),
               pendingBufSize=size(st["pend_size"]))

    def less(i, j):
        return it.method("seqnum", h.a[i].f["sequenceNumber"], "LessThan", h.a[j].f["sequenceNumber"])

    def push(_, s):  # RESTATED: container/heap.Push
        h.a.append(s)
        j = len(h.a) - 1
        while j > 0:
            i = (j - 1) // 2
            if not less(j, i):
                break
            h.a[i], h.a[j] = h.a[j], h.a[i]
            j = i

    def pop(_):  # RESTATED: container/heap.Pop
        n = len(h.a) - 1
        h.a[0], h.a[n] = h.a[n], h.a[0]
        i = 0
        while 2 * i + 1 < n:
            j = 2 * i + 1
            if j + 1 < n and less(j + 1, j):
                j += 1
            if not less(j, i):
                break
            h.a[i], h.a[j] = h.a[j], h.a[i]
            i = j
        return h.a.pop()

    it.stubs["heap.Push"], it.stubs["heap.Pop"] = push, pop

    def segment(seq, base, n, flags):
        s = it._zero("segment", tcp)
        s.f["sequenceNumber"], s.f["flags"], s.f["data"] = val(seq), G.Int(flags, "uint8"), Data(base, n)
        return s

    for t in heap0[:st["pend_count"]]:
        h.a.append(segment(t["seq"], t["base"], t["len"], t["flags"]))
    reset = False
    for s in segs:  # RESTATED: the gates of handleSegments
        opt = s["doff"] - 20
        if s["proto"] != 6 or s["doff"] < 20 or opt > s["vlen"] or s["vlen"] > 65535:
            continue
        if s["flags"] & R.F_RST:
            reset = True
            break
        if not s["flags"] & R.ACK:
            continue
        full = len(h.a) >= cap  # RESTATED: the project's cap reads as a full byte budget
        keep = r.f["pendingBufSize"]
        if full:
            r.f["pendingBufSize"] = size(0)
        it.method("tcp", r, "handleRcvdSegment", segment(s["seq"], s["base"] + opt, s["vlen"] - opt, s["flags"]))
        r.f["pendingBufSize"] = keep
    if not reset and r.f["rcvNxt"].v != ep.max_sent_ack:  # RESTATED: handleSegments' last act
        ep.snd.sendAck()
    out = dict(st, rcv_nxt=r.f["rcvNxt"].v, rcv_acc=r.f["rcvAcc"].v, pend_used=r.f["pendingBufUsed"].v,
               buf_used=ep.buf_used, max_sent_ack=ep.max_sent_ack, pend_count=len(h.a),
               state=R.RESET if reset else (R.CLOSED if r.f["closed"] else R.OPEN))
    heap = [dict(base=x.f["data"].base, len=x.f["data"].n, seq=x.f["sequenceNumber"].v, pkt=R.DEMUX_NONE,
                 flags=x.f["flags"].v) for x in h.a]
    w = (((out["rcv_acc"] - out["rcv_nxt"]) & R.M32) >> st["wnd_scale"]) if st["wnd_scale"] < 32 else 0
    ack = [st["snd_nxt"], out["rcv_nxt"], min(w, 0xFFFF)] if ep.acks else None
    return dict(st=out, heap=heap, delivered=[list(d) for d in ep.delivered], n_acks=ep.acks, ack=ack)


def vector(it, ref, name, cap, st, heap, segs):
    q = C.place(segs)
    got = R.walk(st, heap, cap, q)
    v = dict(name=name, source="restated", cap=cap, st=st, heap=heap, segs=segs,
             status=[got["status"][k] for k in range(len(segs))], delivered=[list(d) for d in got["delivered"]],
             st_out=got["st"], heap_out=got["heap"], n_acks=got["n_acks"], ack=list(got["ack"]) if got["ack"] else None)
    ex = executed(it, st, heap, cap, q)
    if ex is not None:
        for k in ("delivered", "n_acks", "ack"):
            assert ex[k] == v[k], (name, k, ex[k], v[k])
        assert ex["st"] == v["st_out"] and ex["heap"] == v["heap_out"], (name, ex["st"], v["st_out"], ex["heap"])
        v["source"] = "executed"
    if v["ack"]:
        seq, ack, wnd = v["ack"]
        v["ack_datagram"] = ref.send_tcp(LOCAL, REMOTE, None, LPORT, RPORT, R.ACK, seq, ack, wnd).hex()
    return v


def main():
    it, ref = load(), make_refexec.Ref()
    rng = np.random.default_rng(20)
    vectors = []
    for kind in C.KINDS:
        L = 7 if kind != "carried_heap" else 5
        st, heap, segs = C.scenario(kind, L, 2, rng)
        vectors.append(vector(it, ref, f"{kind}-L{L}-cap2", 2, st, heap, segs))
    # the pins the header names: the trimmed length leaves the byte budget; cap 0 keeps nothing
    st = R.new_state(1000, 65535)
    segs = [C.seg(1100, 100), C.seg(1000, 150), C.seg(1250, 10)]
    vectors.append(vector(it, ref, "trimmed-length-leaves-budget", 4, st, [], segs))
    vectors.append(vector(it, ref, "cap0-keeps-nothing", 0, st, [], segs))
    vectors.append(vector(it, ref, "dup-popped-as-acknowledged", 4, st, [], [C.seg(1100, 50), C.seg(1000, 200)]))
    path = os.path.join(HERE, "tcp_stream.json")
    with open(path, "w") as f:
        json.dump(dict(format=1, pitch=C.PITCH, heap_at=C.HEAP_AT, local=list(LOCAL), remote=list(REMOTE),
                       local_port=LPORT, remote_port=RPORT, vectors=vectors), f, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(vectors), "vectors,",
          sum(v["source"] == "executed" for v in vectors), "executed")


if __name__ == "__main__":
    main()
