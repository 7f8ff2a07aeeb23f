"""Runs the host-ledger cases (tests/host_cases.py) of one knob set on the GPU:
    python tests/host_child.py <knob set index>
The knobs are in the environment already (tests/test_gpu_host_ledger.py sets them: the
library reads them once). Per case: the idle staging is trimmed and reads (0, 0); the call
goes through the C ABI (yustack_amd._lib.lib()) with pointers into guarded host
allocations, pageable or pinned, at the addresses the case asks for; the results equal
the C oracle's on the same bytes, every packet compared; the guard entries around h_out
are untouched (a call without h_out: the whole allocation); every byte of the packet
memory, every view and guard included, equals the input except, in place, the fields the
rule defines (test_gpu_contract._fields, the one statement of it on the test side), which
hold the oracle's values big-endian; the side arrays and tables are unchanged; and
yu_host_staging_bytes equals what the model (tests/host_slices.py) predicts from the
largest slice of the cut, which ties the model's cut and route to what the library did.
One line per case; exits non-zero at the first mismatch.

prepare, check_out and check_memory need no GPU: tests/test_host_ledger.py feeds them
wrong results."""
import ctypes
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import host_cases as H  # noqa: E402
import rxgen  # noqa: E402
from ledger_child import GUARD, OUT_FILL, OUT_GUARD, check_memory, check_out  # noqa: E402,F401
from oracle import oracle as O  # noqa: E402

FILL = 0xA5
PER_PACKET = 4096  # datagram batches up to this size take their packets from rxgen one by one


def _datagrams(rng, mode, lens):
    """Datagrams of exactly these lengths. Small batches: out of a pool of rxgen's (outgoing
    ones, 30 % damaged or malformed; received ones, half of them damaged), padded with
    trailing bytes, which both contracts allow; below 20 bytes, or where none fits, random
    bytes. Large batches: IHL-5 headers written in bulk, one in sixteen malformed."""
    n = lens.size
    offs = np.concatenate(([0], np.cumsum(lens)))
    blob = rng.integers(0, 256, size=int(offs[-1]), dtype=np.uint8)
    if n > PER_PACKET:
        s = offs[:-1][lens >= 20]
        ln = lens[lens >= 20]
        tl = ln + (rng.integers(0, 16, size=s.size) == 0)  # TotalLength past the packet: malformed
        blob[s] = 0x45
        blob[s + 2], blob[s + 3] = (tl >> 8).astype(np.uint8), (tl & 0xFF).astype(np.uint8)
        proto = np.array([1, 6, 17, 47], np.uint8)[rng.integers(0, 4, size=s.size)]
        blob[s + 9] = proto
        t = s[(proto == 6) & (ln >= 40)]
        blob[t + 32] = 0x50  # DataOffset 5: inside YU_MODE_TCP's contract
        return blob
    hi = int(min(max(lens.max(), 20), 1400))
    pb, po = (rxgen.tx_batch(rng, 96, lo=0, hi=hi, bad=0.3) if mode == "tx_datagram" else
              rxgen.rx_batch(rng, 96, lo=0, hi=hi, bad=0.5))
    pool = sorted((bytes(pb[int(po[i]):int(po[i + 1])]) for i in range(96)), key=len)
    sizes = np.array([len(p) for p in pool])
    for i in range(n):
        fit = int(np.searchsorted(sizes, lens[i], side="right"))
        if lens[i] < 20 or not fit:
            continue
        p = bytearray(pool[int(rng.integers(0, fit))])
        p += rng.integers(0, 256, size=int(lens[i]) - len(p), dtype=np.uint8).tobytes()
        if mode == "tx_datagram":
            p = rxgen.tcp_contract(p)  # (the padding may have brought TotalLength inside the packet)
        blob[offs[i]:offs[i + 1]] = np.frombuffer(bytes(p), np.uint8)
    return blob


def packet_bytes(rng, mode, lens):
    """The packets laid back to back, inside each mode's contract."""
    lens = np.asarray(lens, np.int64)
    if mode in ("verify_rx", "tx_datagram"):
        return _datagrams(rng, mode, lens)
    offs = np.concatenate(([0], np.cumsum(lens)))
    blob = rng.integers(0, 256, size=int(offs[-1]), dtype=np.uint8)
    if mode in ("tcp", "verify_tcp"):  # 20 <= DataOffset <= len, as sendTCP encodes
        s, ln = offs[:-1][lens >= 20], lens[lens >= 20]
        blob[s + 12] = ((5 + rng.integers(0, 11, size=s.size) % (np.minimum(15, ln // 4) - 4)) << 4).astype(np.uint8)
    if mode in ("ipv4", "verify_ipv4"):  # any IHL: below 3, past the packet
        s = offs[:-1][lens >= 1]
        blob[s] = (0x40 | rng.integers(0, 16, size=s.size)).astype(np.uint8)
    return blob


def _field_offsets(mode, pkt):
    if mode == "tx_datagram" and len(pkt) >= 20:
        hl = (int(pkt[0]) & 15) * 4
        fo = {17: 6, 6: 16, 1: 2}.get(int(pkt[9]), 0)
        return [10] + ([hl + fo] if fo else [])
    return [H.K.FIELD.get(mode, 6)]


def _view_lens(rng, kind, mode, pkt):
    """One packet's bytes cut into views. rand: 0..4 views, empty ones among them;
    split_field: a cut inside each field, an empty view between its two bytes; ones:
    one-byte views around and inside the field, empty views between them."""
    ln = len(pkt)
    if kind == "one":
        return [ln]
    if kind == "rand":
        k = int(rng.integers(0 if ln == 0 else 1, 5))
        edges = [0] + sorted(int(x) for x in rng.integers(0, ln + 1, size=max(k - 1, 0))) + [ln]
        return [edges[j + 1] - edges[j] for j in range(len(edges) - 1)] if k else []
    cuts = set()
    for f in _field_offsets(mode, pkt):
        cuts |= {f + 1} if kind == "split_field" else {f - 1, f, f + 1, f + 2}
    edges = [0] + sorted(c for c in cuts if 0 < c < ln) + [ln]
    out = []
    for j in range(len(edges) - 1):
        out += [edges[j + 1] - edges[j], 0]
    return out[:-1] if ln else [0, 0]


class Prepared:
    """A case as far as the CPU takes it (prepare)."""


def prepare(case, oracle):
    """The arena (packet memory with its guards), where the packets lie in it, the side
    data, the oracle's values and the expected arena after the call."""
    from test_gpu_contract import _fields
    P = Prepared()
    f = H.facts(case)
    P.n = n = f["n"]
    mode, layout = case["mode"], case["layout"]
    P.mode_i = mi = H.MODES.index(mode)
    P.k = 2 if mode == "tx_datagram" else 1
    rng = np.random.default_rng(H.seed_of(case))
    P.first = P.vpos = P.vlen = None
    if layout == "U":
        stride, ln, _ = f["geometry"]
        P.stride, P.len = stride, ln
        span = (n - 1) * stride + ln
        P.arena = rng.integers(0, 256, size=GUARD + span + GUARD, dtype=np.uint8)
        P.starts = GUARD + stride * np.arange(n, dtype=np.int64)
        P.lens = np.full(n, ln, np.int64)
        if stride >= ln or stride == 0:  # (overlapping packets, 0 < stride < len: bytes as they fall)
            m = 1 if stride == 0 else n
            pk = packet_bytes(rng, mode, np.full(m, ln, np.int64)).reshape(m, ln)
            if stride == ln:
                P.arena[GUARD:GUARD + span] = pk.reshape(-1)
            else:
                np.lib.stride_tricks.as_strided(P.arena[GUARD:], (m, ln), (max(stride, 1), 1))[:] = pk
    else:
        P.lens = lens = f["geometry"]
        blob = packet_bytes(rng, mode, lens)
        offs = np.concatenate(([0], np.cumsum(lens)))
        if layout == "R" or (case["views"] == "one" and n > PER_PACKET):
            P.arena = np.concatenate((rng.integers(0, 256, size=GUARD, dtype=np.uint8), blob,
                                      rng.integers(0, 256, size=GUARD, dtype=np.uint8)))
            P.starts = GUARD + offs[:-1]
            P.offsets = (case["off0"] + offs).astype(np.uint64)
            if layout == "V":
                P.vpos, P.vlen, P.first = P.starts.copy(), lens.copy(), np.arange(n + 1, dtype=np.uint64)
        else:  # views, with 0..3 guard bytes between them
            vpos, vlen, first, pos = [], [], [0], GUARD
            for i in range(n):
                for v in _view_lens(rng, case["views"], mode, blob[offs[i]:offs[i + 1]]):
                    vpos.append(pos)
                    vlen.append(v)
                    pos += v + int(rng.integers(0, 4))
                first.append(len(vpos))
            P.vpos, P.vlen = np.asarray(vpos, np.int64).reshape(-1), np.asarray(vlen, np.int64).reshape(-1)
            P.first = np.asarray(first, np.uint64)
            P.arena = rng.integers(0, 256, size=pos + GUARD, dtype=np.uint8)
            # byte j of the packets laid back to back lies at arena[P.where[j]]
            vid = np.repeat(np.arange(P.vlen.size), P.vlen)
            P.where = np.arange(int(offs[-1])) + (P.vpos - np.concatenate(([0], np.cumsum(P.vlen)[:-1])))[vid]
            P.arena[P.where] = blob
            P.starts = None
    P.offs0 = np.concatenate(([0], np.cumsum(P.lens)))  # packet i = bytes [offs0[i], offs0[i+1]) back to back
    # side data
    side = case["side"]
    P.init = rng.integers(0, 65536, size=n, dtype=np.uint16) if side == "init" or (
        side == "junk" and mode == "raw") else None
    P.addrs = rng.integers(0, 256, size=8 * n, dtype=np.uint8) if side == "addrs" or (
        side == "junk" and mode in H.PSEUDO) else None
    P.initial = 0x1234 if side == "absent" and (mode in H.PSEUDO or mode == "raw") else 0
    P.call_init, P.call_addrs, P.call_initial = P.init, P.addrs, P.initial
    if side == "junk":  # junk in what the mode ignores; the oracle never sees it
        if P.init is None:
            P.call_init, P.call_initial = rng.integers(0, 65536, size=n, dtype=np.uint16), 0xBEEF
        if P.addrs is None:
            P.call_addrs = rng.integers(0, 256, size=8 * n, dtype=np.uint8)
    # the oracle's values, for every packet whose value is defined
    low = H.UNDEFINED_BELOW.get(mode, 0)
    P.defined = P.lens >= low
    threads = 8 if P.arena.size > (1 << 20) else 1
    if layout == "U":
        P.want = oracle.batch(P.arena[GUARD:], mi, stride=P.stride, length=P.len, n=n, initial_arr=P.init,
                              initial=P.initial, addrs=P.addrs, threads=threads)
    else:
        flat = P.arena[GUARD:GUARD + int(P.offs0[-1])] if P.starts is not None else P.arena[P.where]
        if P.defined.all():
            P.want = oracle.batch(np.append(flat, np.uint8(0)), mi, offsets=P.offs0.astype(np.uint64), initial_arr=P.init,
                                  initial=P.initial, addrs=P.addrs, threads=threads)
        else:
            keep = np.flatnonzero(P.defined)
            sel = np.concatenate([np.arange(P.offs0[i], P.offs0[i + 1]) for i in keep] + [np.zeros(0, np.int64)])
            o = np.concatenate(([0], np.cumsum(P.lens[keep]))).astype(np.uint64)
            w = oracle.batch(np.append(flat[sel.astype(np.int64)], np.uint8(0)), mi, offsets=o,
                             initial_arr=None if P.init is None else P.init[keep], initial=P.initial,
                             addrs=None if P.addrs is None else P.addrs.reshape(-1, 8)[keep].reshape(-1))
            P.want = np.zeros(n * P.k, np.uint16)
            P.want.reshape(n, P.k)[keep] = w.reshape(-1, P.k)
    # the arena after the call
    P.expected = P.arena
    if case["call"] != "batch":
        P.expected = exp = P.arena.copy()
        w2 = P.want.reshape(n, P.k)
        for i in np.flatnonzero(P.defined):
            vals = [int(x) for x in w2[i]]
            if P.starts is not None:
                for pos, v in _fields(mi, P.arena, int(P.starts[i]), int(P.starts[i] + P.lens[i]), vals):
                    exp[pos] = v
            else:
                a, b = int(P.offs0[i]), int(P.offs0[i + 1])
                for pos, v in _fields(mi, P.arena[P.where[a:b]], 0, b - a, vals):
                    exp[P.where[a + pos]] = v
    return P


# ---------------------------------------------------------------------------
# On the GPU
# ---------------------------------------------------------------------------
class Mem:
    """A host allocation, pageable or pinned, that holds `payload` so that it starts at an
    address congruent to `mod` (mod `align`), FILL bytes around it."""

    def __init__(self, torch, payload, pinned, mod=0, align=16):
        raw = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        size = raw.size + 2 * align + 64
        if pinned:
            self.keep = torch.empty(size, dtype=torch.uint8, pin_memory=True)
            self.whole = self.keep.numpy()
            assert self.keep.is_pinned()
        else:
            self.whole = np.empty(size, np.uint8)
        base = self.whole.ctypes.data
        self.off = off = 32 + (mod - (base + 32)) % align
        self.whole[:] = FILL
        self.view = self.whole[off:off + raw.size]
        self.view[:] = raw
        self.raw = raw.copy()
        self.ptr = base + off
        assert self.ptr % align == mod

    def outside_changed(self):
        return not ((self.whole[:self.off] == FILL).all() and (self.whole[self.off + self.raw.size:] == FILL).all())

    def changed(self):
        return self.outside_changed() or not np.array_equal(self.view, self.raw)


def run_case(case, oracle, torch, L, host_staging):
    f = H.facts(case)
    P = prepare(case, oracle)
    n, layout, call = P.n, case["layout"], case["call"]
    assert L.yu_host_staging_trim(0) == 0
    if host_staging(0) != (0, 0):
        return f"staging {host_staging(0)} after a trim"
    pinned_in = case["inmem"] != "pageable"
    # the packet memory: the first packet's byte (views: the arena's payload) at the case's address mod 16
    data = Mem(torch, P.arena, pinned_in, (case["align"] - GUARD) % 16)
    assert (data.ptr + GUARD) % 16 == case["align"] and (case["inmem"] != "pinned_odd" or (data.ptr + GUARD) % 2 == 1)
    # results: guard entries on both sides; pageable, or pinned at 2 (mod 4)
    pin_out = case["outmem"] == "pinned2"
    out = Mem(torch, np.full(2 * OUT_GUARD + n * P.k, OUT_FILL, np.uint16), pin_out, 2 if pin_out else 0, 4)
    out_ptr = None if call == "fill_null" else out.ptr + 2 * OUT_GUARD
    assert not pin_out or out_ptr is None or out_ptr % 4 == 2
    side = []
    pi = pa = None
    if P.call_init is not None:
        pi = Mem(torch, P.call_init, False, 2, 4)
        side.append(pi)
    if P.call_addrs is not None:
        pa = Mem(torch, P.call_addrs, False, 4, 8)
        side.append(pa)
    tail = [None if pi is None else pi.ptr, P.call_initial, None if pa is None else pa.ptr, out_ptr]
    dv = case["devices"]
    if isinstance(dv, list):
        arr = (ctypes.c_int * len(dv))(*dv)
        tail += [ctypes.cast(arr, ctypes.c_void_p), len(dv)]
        suffix = "_multi"
    else:
        tail.append(dv)
        suffix = ""
    kind = "batch" if call == "batch" else "fill"
    if layout == "U":
        fn = getattr(L, f"yu_csum_{kind}_host_uniform{suffix}")
        rc = fn(data.ptr + GUARD, P.stride, P.len, n, P.mode_i, *tail)
    elif layout == "R":
        offs = Mem(torch, P.offsets, False, 8, 16)
        side.append(offs)
        # offsets[0] may lie above 0: packet 0 starts at data + offsets[0]
        fn = getattr(L, f"yu_csum_{kind}_host_ragged{suffix}")
        rc = fn(data.ptr + GUARD - case["off0"], offs.ptr, n, P.mode_i, *tail)
    else:  # the yu_iovec table {base, len}; empty views: NULL and wild bases
        base = (np.uint64(data.ptr) + P.vpos.astype(np.uint64))
        empty = P.vlen == 0
        base[empty] = np.where(np.arange(P.vlen.size) % 2, 0xDEAD0001, 0).astype(np.uint64)[empty]
        table = Mem(torch, np.stack((base, P.vlen.astype(np.uint64)), 1), False, 8, 16)
        first = Mem(torch, P.first, False, 8, 16)
        side += [table, first]
        fn = getattr(L, f"yu_csum_{kind}_host_iov{suffix}")
        rc = fn(table.ptr, first.ptr, n, P.mode_i, *tail)
    if rc != 0:
        return f"status {rc}"
    got = out.view.view(np.uint16)
    if call == "fill_null":
        err = "the result allocation changed in a call without h_out" if out.changed() else None
    else:
        assert P.defined.all(), "a case with undefined values takes no result array"
        err = check_out(got, OUT_GUARD, P.want)
    if err is None and out.outside_changed():
        err = "bytes around the result allocation changed"
    err = err or check_memory(data.view, P.expected)
    if err is None and data.outside_changed():
        err = "bytes around the packet memory changed"
    if err is None and any(x.changed() for x in side):
        err = "a side array, a table or its guard bytes changed"
    if err is None and host_staging(0) != f["staging"]:
        err = f"staging {host_staging(0)}, the model predicts {f['staging']} (cuts {[c[:3] for c in f['cuts']]})"
    return err


def main():
    s = int(sys.argv[1])
    import torch
    from yustack_amd import _lib
    assert torch.cuda.is_available()
    oracle = O.C()
    L = _lib.lib()
    cases = [c for c in H.CASES if c["set"] == s]
    print(f"host set {s} {H.KNOB_SETS[s]}: {len(cases)} cases", flush=True)
    t0 = time.perf_counter()
    slow = (0.0, "")
    for c in cases:
        t1 = time.perf_counter()
        err = run_case(c, oracle, torch, L, _lib.host_staging)
        slow = max(slow, (time.perf_counter() - t1, c["id"]))
        print(f"{'FAIL' if err else 'ok'} {c['id']}{': ' + err if err else ''}", flush=True)
        if err:
            return 1
    assert L.yu_host_staging_trim(0) == 0
    print(f"slowest case {slow[0]:.2f} s: {slow[1]}", flush=True)
    print(f"host ledger set {s}: {len(cases)} cases in {time.perf_counter() - t0:.2f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
