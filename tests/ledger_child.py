"""Runs the ledger cases (tests/kernel_cases.py) of one knob set on the GPU:
    python tests/ledger_child.py <knob set index>
The knobs are in the environment already (tests/test_gpu_kernel_ledger.py sets them:
the library reads them once). Per case: the library names the written kernel; the results
equal the C oracle's on the same bytes; `out` lies inside an allocation with 64 guard
entries on each side, which are untouched; the packets are a view into a buffer with 128
guard bytes on each side (scatter-gather: every pool), and afterwards every byte of it
equals the input except, in place, the fields the oracle defines, which hold its values
big-endian. One line per case; exits non-zero at the first mismatch.

A case's `call` says how the call is made. "plain": through yustack_amd.batch, `out` 128-byte
aligned. Otherwise through the C ABI (yustack_amd._lib.lib()) with pointers into guarded
allocations (Placed) that are compared afterwards: "offset" puts out and initial_arr at
2 (mod 4), addrs at 4 (mod 8) (4 or 12 mod 16 by case index), offsets, the yu_iovec table
and first_iov at 8 (mod 16), asserted before the call; "null_out" passes out = NULL to the
in-place call (the packet memory is the evidence); "ignored" passes junk arrays, at those
alignments, and initial = 0xBEEF in the arguments the mode does not use, while the oracle
gets only the ones it uses. The scatter-gather cases (layout "I") always take the C ABI,
with the table written here.

A case's `kind` beyond the byte patterns: "pole_side" and "pole_data" solve initial_arr or
one word of every packet with the oracle so that every packet sums to 0x0000 (the TX modes)
or 0xFFFF (RAW, VERIFY_*); prepare() refuses a case with a packet off its pole. An all-zero
packet written in place first gets random nonzero bytes in its field.

A ragged case with gen = ("seam", CH, T) takes its packets from tests/seg_seams.py, which
plants every seam class of the case's k_seg kind; its model of the tiling takes `data` to
lie on a 128-byte line, which is asserted of the pointer passed.

prepare, expected_memory, check_out and check_memory need no GPU: tests/test_kernel_ledger.py
feeds them wrong results."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import kernel_cases as K  # noqa: E402
import rxgen  # noqa: E402
import seg_seams  # noqa: E402
from iov_layout import general_layout, set_tcp_offset  # noqa: E402

GUARD = 128
OUT_GUARD = 64
OUT_FILL = 0xA5A5


def rand(rng, n, kind):
    if kind == "zero":
        return np.zeros(n, np.uint8)
    if kind == "ff":
        return np.full(n, 255, np.uint8)
    return rng.integers(0, 256, size=n, dtype=np.uint8)


def headers(rng, blob, starts, lens, mode, fill):
    """The header bytes the per-packet modes read: TCP's DataOffset (20..min(60, len), as
    sendTCP encodes), IPv4's IHL (within the packet; 5 and more where the field is written)."""
    lens = np.broadcast_to(lens, starts.shape)
    if mode in ("tcp", "verify_tcp"):
        hi = np.minimum(15, lens // 4)
        blob[starts + 12] = ((5 + rng.integers(0, 11, size=starts.size) % (hi - 4)) << 4).astype(np.uint8)
    if mode in ("ipv4", "verify_ipv4"):
        lo = 5 if fill else 0
        hi = np.minimum(15, lens // 4)
        blob[starts] = (0x40 | (lo + rng.integers(0, 16, size=starts.size) % (hi - lo + 1))).astype(np.uint8)


def datagram_pool(rng, mode, count, lo, hi, length=None):
    """Up to 256 datagrams from rxgen (received ones, 40 % damaged, or outgoing ones);
    `length`: cut or padded to a uniform slot's length."""
    pool = []
    for _ in range(min(count, 256)):
        if length is not None:
            p = (rxgen.make_packet if mode == "verify_rx" else rxgen.tx_packet)(rng, max(length - 20, 0), ihl=5)
        else:
            p = (rxgen.make_packet if mode == "verify_rx" else rxgen.tx_packet)(rng, int(rng.integers(lo, hi + 1)))
        if rng.random() < (0.4 if mode == "verify_rx" else 0.1):
            p = rxgen.damage(rng, p)
            if mode == "tx_datagram":
                p = rxgen.tcp_contract(p)
        p = bytes(p)
        if length is not None:
            p = p[:length].ljust(length, b"\0")
        pool.append(np.frombuffer(p, np.uint8))
    if length is None and lo == 0 and count > 8:  # empty and headerless datagrams among them
        pool[1] = np.zeros(0, np.uint8)
        pool[5] = rand(rng, 7, "rand")
    return pool


def datagram_fields(blob, starts, ends, want):
    """TX_DATAGRAM in place: the positions and big-endian values of the fields the mode
    defines (include/yucsum.h YU_MODE_TX_DATAGRAM; the logic of test_gpu_parity._tx_expected)."""
    size = ends - starts
    a = starts[size >= 20]
    i = np.nonzero(size >= 20)[0]
    hl = (blob[a].astype(np.int64) & 15) * 4
    tl = (blob[a + 2].astype(np.int64) << 8) | blob[a + 3]
    ok = (hl >= 20) & (hl <= tl) & (tl <= size[i])
    a, i, hl, tl = a[ok], i[ok], hl[ok], tl[ok]
    proto = blob[a + 9]
    fo = np.select([proto == 17, proto == 6, proto == 1], [6, 16, 2], 0)
    mn = np.select([proto == 17, proto == 6, proto == 1], [8, 20, 4], 0)
    l4 = (fo > 0) & (tl - hl >= mn)
    pos = np.concatenate([a + 10, (a + hl + fo)[l4]])
    val = np.concatenate([want[2 * i], want[2 * i[l4] + 1]])
    return pos, val


def build(case, n, rng):
    """(buffer with guards, view offset, geometry, packet starts, packet ends)."""
    mode, base = case["mode"], case["base"]
    dgram = mode in ("verify_rx", "tx_datagram")
    if case["layout"] == "U":
        ln, st = case["len"], case["stride"]
        span = base + (n - 1) * st + ln
        starts = GUARD + base + st * np.arange(n, dtype=np.int64)
        if st > 4 * ln + 64:  # far apart: only the packets are drawn
            buf = np.zeros(GUARD + span + GUARD, np.uint8)
            for s in starts:
                buf[s:s + ln] = rand(rng, ln, case["kind"])
            buf[:GUARD], buf[-GUARD:] = rand(rng, GUARD, "rand"), rand(rng, GUARD, "rand")
        else:
            buf = rand(rng, GUARD + span + GUARD, case["kind"])
        if dgram:
            pool = np.stack(datagram_pool(rng, mode, n, 0, 0, length=ln))
            slots = np.lib.stride_tricks.as_strided(buf[GUARD + base:], (n, ln), (st, 1))
            slots[:] = pool[rng.integers(0, len(pool), size=n)]
        elif ln:
            headers(rng, buf, starts, ln, mode, case["fill"] or case["kind"] == "pole_data")
        return buf, starts, starts + ln
    name, lo, hi = case["gen"]
    if name == "seam":  # (CH, T): every seam class of the case's kind, planted (tests/seg_seams.py)
        kind = K.seg_shape(K.kernel_of(case)[0])[2]
        line128 = kind == "txw" and case["fill"]
        b = seg_seams.batch(lo, hi, mode, line128, base, seg_seams.classes_for(kind, mode, line128), n, rng)
        lens, parts = b.lens, b.parts
    elif dgram:
        pool = datagram_pool(rng, mode, n, lo, hi)
        pick = rng.integers(0, len(pool), size=n) if n > len(pool) else np.arange(n)
        parts = [pool[i] for i in pick]
        lens = np.array([p.size for p in parts], np.int64)
    else:
        lens = rng.integers(lo, hi + 1, size=n).astype(np.int64)
        if name == "jumbo":  # long packets among them; RAW: past the LE sum's 131072 bytes
            lens[::61] = 131073 + np.arange(len(lens[::61])) if mode == "raw" else 9000
        if lo == 0 and n > 20:
            lens[3::17] = 0
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    offs += GUARD + base
    buf = rand(rng, int(offs[-1]) + GUARD, case["kind"])
    if dgram:
        buf[GUARD + base:int(offs[-1])] = np.concatenate(parts) if parts else 0
    else:
        headers(rng, buf, offs[:-1], lens, mode, case["fill"] or case["kind"] == "pole_data")
    return buf, offs[:-1], offs[1:]


class Prepared:
    """A case as far as the CPU takes it (prepare)."""


def prepare(case, s, cus, oracle):
    """The bytes, the side data and the oracle's values of a case under knob set `s`;
    a string when the case itself is wrong (a pole case off its pole)."""
    P = Prepared()
    P.n = n = K.resolve_n(case, cus, K.KNOB_SETS[s])
    mode, fill, kind, layout = case["mode"], case["fill"], case["kind"], case["layout"]
    P.index = int(case["id"].split()[0])
    rng = np.random.default_rng(P.index * 16 + s)
    P.k = 2 if mode == "tx_datagram" else 1
    P.lay = P.buf = None
    if layout == "I":
        P.lay = lay = general_layout(K.iov_packets(case, n), rng, fillbyte={"zero": 0, "ff": 255}.get(kind))
        if mode in ("tcp", "verify_tcp") and kind in ("zero", "ff"):
            set_tcp_offset(lay)
        P.starts, P.ends = lay.offsets[:-1].astype(np.int64), lay.offsets[1:].astype(np.int64)
        put = lay.put
    else:
        P.buf, P.starts, P.ends = build(case, n, rng)

        def put(pos, values):
            P.buf[pos] = values
    starts, lens = P.starts, P.ends - P.starts
    side = case["side"]
    P.init = rng.integers(0, 65536, size=n, dtype=np.uint16) if side == "init" else None
    P.addrs = rng.integers(0, 256, size=8 * n, dtype=np.uint8) if side == "addrs" else None
    P.initial = initial = 0x1234 if side == "scalar" and mode in K.SIDES else 0
    threads = 8 if (P.buf.size if P.buf is not None else lay.bpos.size) > (1 << 20) else 1

    def ask(init):
        if layout == "U":
            return oracle.batch(P.buf[GUARD + case["base"]:], K.MODES.index(mode), stride=case["stride"],
                                length=case["len"], n=n, initial_arr=init, initial=initial, addrs=P.addrs, threads=threads)
        if layout == "R":
            return oracle.batch(P.buf[GUARD:], K.MODES.index(mode), offsets=P.offs, initial_arr=init, initial=initial,
                                addrs=P.addrs, threads=threads)
        return oracle.batch(lay.blob(), K.MODES.index(mode), offsets=lay.offsets, initial_arr=init, initial=initial,
                            addrs=P.addrs, threads=threads)

    if layout == "R":
        P.offs = np.append(starts, P.ends[-1:]).astype(np.uint64) - GUARD
    if kind == "zero" and fill and mode in K.FIELD:
        # a nonzero stored field: "the field is taken as 0" is what keeps the packet all-zero
        at = starts[lens >= K.FIELD[mode] + 2] + K.FIELD[mode]
        put(at, rng.integers(1, 256, size=at.size, dtype=np.uint8))
        put(at + 1, rng.integers(1, 256, size=at.size, dtype=np.uint8))
    if kind == "pole_data":
        # the word at POLE_W: zeroed, then the oracle's value (VERIFY: its complement) stored there
        w = K.POLE_W[mode]
        if (lens < w + 2).any():
            return f"test bug: a packet shorter than {w + 2} bytes in a pole_data case"
        put(starts + w, 0)
        put(starts + w + 1, 0)
        r = ask(P.init)
        r = r if mode in K.TX_POLE else ~r & 0xFFFF
        put(starts + w, (r >> 8).astype(np.uint8))
        put(starts + w + 1, (r & 0xFF).astype(np.uint8))
    if kind == "pole_side":
        # initial_arr: the oracle's value with initial_arr all 0 (RAW / VERIFY: its complement)
        if mode == "raw" and (lens > 65535).any():
            return "test bug: a RAW packet above 65535 bytes in a pole_side case"
        r0 = ask(np.zeros(n, np.uint16))
        P.init = r0 if mode in K.TX_POLE else (~r0 & 0xFFFF).astype(np.uint16)
    P.want = want = ask(P.init)
    if kind in K.POLE_KINDS and not (want == K.pole(mode)).all():
        off = np.nonzero(want != K.pole(mode))[0]
        return f"test bug: {off.size} packets off the pole {K.pole(mode):#06x}, first {off[:6].tolist()}"
    if fill and mode == "icmp" and kind in ("zero", "ff"):  # all-zero: 0xFFFF; all-0xFF, even length: 0x0000
        on = want == 0xFFFF if kind == "zero" else want[lens % 2 == 0] == 0
        if not on.all():
            return f"test bug: an all-{kind} ICMP packet off its pole"
    # `ignored`: junk in the arguments the mode does not use; the oracle never sees it
    P.junk_init = P.junk_addrs = None
    P.call_initial = initial
    what = K.ignores(mode, side) if "ignored" in K.calls(case) else None
    if what in ("both", "init"):
        P.junk_init = rng.integers(0, 65536, size=n, dtype=np.uint16)
        P.call_initial = 0xBEEF
    if what in ("both", "addrs"):
        P.junk_addrs = rng.integers(0, 256, size=8 * n, dtype=np.uint8)
    return P


def expected_memory(case, P):
    """The packet memory after the call: the buffer (uniform, ragged) or the list of
    pools (scatter-gather), the input but for the fields the oracle defines."""
    mode = case["mode"]
    if P.lay is not None:
        return P.lay.filled(K.MODES.index(mode), P.want) if case["fill"] else P.lay.pools
    if not case["fill"]:
        return P.buf
    exp = P.buf.copy()
    if mode == "tx_datagram":
        pos, val = datagram_fields(P.buf, P.starts, P.ends, P.want)
    else:
        pos, val = P.starts + K.FIELD[mode], P.want
    exp[pos] = (val >> 8).astype(np.uint8)
    exp[pos + 1] = (val & 0xFF).astype(np.uint8)
    return exp


def check_out(got, lo, want):
    """`got`: the whole result allocation, guards included; the results start at entry lo."""
    res = got[lo:lo + want.size]
    if not np.array_equal(res, want):
        bad = np.nonzero(res != want)[0]
        return f"{bad.size} results differ, first at {bad[:6].tolist()}: got {res[bad[:3]].tolist()} want {want[bad[:3]].tolist()}"
    if not (got[:lo] == OUT_FILL).all():
        return f"guard entries before the results changed: {np.nonzero(got[:lo] != OUT_FILL)[0][:6].tolist()}"
    if not (got[lo + want.size:] == OUT_FILL).all():
        return f"guard entries after the results changed: {np.nonzero(got[lo + want.size:] != OUT_FILL)[0][:6].tolist()}"
    return None


def check_memory(after, exp, what="the expected buffer"):
    if not np.array_equal(after, exp):
        bad = np.nonzero(after != exp)[0]
        return f"{bad.size} bytes differ from {what}, first at {(bad[:6] - GUARD).tolist()} (view offsets)"
    return None


class Placed:
    """A host array in device memory at an address congruent to `mod` (mod `align`),
    with guard bytes on both sides."""

    def __init__(self, torch, dev, payload, mod, align):
        raw = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        self.t = torch.empty(GUARD + align + raw.size + GUARD, dtype=torch.uint8, device=dev)
        off = GUARD + (mod - (self.t.data_ptr() + GUARD)) % align
        self.host = np.full(self.t.numel(), 0xA5, np.uint8)
        self.host[off:off + raw.size] = raw
        self.t.copy_(torch.from_numpy(self.host))
        self.ptr = self.t.data_ptr() + off
        assert self.ptr % align == mod and off + raw.size + GUARD <= self.t.numel()

    def changed(self):
        return not np.array_equal(self.t.cpu().numpy(), self.host)


def run_case(case, s, cus, dev, oracle, torch, batch):
    env = K.KNOB_SETS[s]
    n = K.resolve_n(case, cus, env)
    mode, fill, layout = case["mode"], case["fill"], case["layout"]
    kernel = case["plans"][s].split()[0]
    name = (batch.variant(case["stride"], case["len"], mode, case["base"], n=n) if layout == "U" else
            batch.ragged_variant(mode, n, fill=fill) if layout == "R" else batch.iov_variant(mode, n, fill=fill))
    if name != kernel:
        return f"the library names {name}"
    P = prepare(case, s, cus, oracle)
    if isinstance(P, str):
        return P
    shapes = K.calls(case)
    offset = "offset" in shapes
    want = P.want
    # out: inside an allocation with OUT_GUARD entries on both sides; 128-byte aligned, or at 2 (mod 4)
    lo = OUT_GUARD + (1 if offset else 0)
    big = torch.from_numpy(np.full(lo + n * P.k + OUT_GUARD, OUT_FILL, np.uint16)).to(dev)
    out_ptr = big.data_ptr() + 2 * lo
    assert out_ptr % 4 == 2 if offset else out_ptr % 128 == 0
    if P.lay is None:
        whole = torch.from_numpy(P.buf).to(dev)
        memory = [whole]
        # the seam model (tests/seg_seams.py) takes `data` to lie on a 128-byte line
        assert not K.is_seam(case) or (whole.data_ptr() + GUARD) % 128 == 0
    else:
        memory = [torch.from_numpy(p).to(dev) for p in P.lay.pools]
    if shapes == {"plain"} and P.lay is None:  # through the Python front end
        side_t = dict(initial=P.initial, initial_arr=None if P.init is None else torch.from_numpy(P.init).to(dev),
                      addrs=None if P.addrs is None else torch.from_numpy(P.addrs).to(dev), out=big[lo:lo + n * P.k],
                      fill=fill)
        if layout == "U":
            batch.checksum_uniform(whole[GUARD + case["base"]:], case["stride"], case["len"], n, mode, **side_t)
        else:
            batch.checksum_ragged(whole[GUARD:], torch.from_numpy(P.offs.view(np.int64)).to(dev), mode, **side_t)
        placed = []
    else:  # the C ABI itself: pointers at the least alignment it allows, NULL out, junk in unused arguments
        from yustack_amd import _lib
        init = P.init if P.init is not None else P.junk_init
        addrs = P.addrs if P.addrs is not None else P.junk_addrs
        # the arrays the mode reads: at the least alignment when `offset`; junk ones always
        low_i, low_a = offset or P.init is None, offset or P.addrs is None
        pi = None if init is None else Placed(torch, dev, init, 2 if low_i else 0, 4 if low_i else 256)
        pa = None if addrs is None else Placed(torch, dev, addrs, (4, 12)[P.index % 2] if low_a else 0, 16 if low_a else 256)
        placed = [x for x in (pi, pa) if x is not None]
        assert pi is None or not low_i or pi.ptr % 4 == 2
        assert pa is None or not low_a or (pa.ptr % 8 == 4 and pa.ptr % 16 == (4, 12)[P.index % 2])
        tail = (None if pi is None else pi.ptr, P.call_initial, None if pa is None else pa.ptr,
                None if "null_out" in shapes else out_ptr, torch.cuda.current_stream(dev).cuda_stream)
        L = _lib.lib()
        if layout == "U":
            data = whole.data_ptr() + GUARD + case["base"]
            assert not fill or (data % 4 == 0 and case["stride"] % 4 == 0)
            rc = (L.yu_csum_fill_uniform if fill else L.yu_csum_batch_uniform)(
                data, case["stride"], case["len"], n, K.MODES.index(mode), *tail)
        else:
            if layout == "R":
                tables = [P.offs]
                first_arg = whole.data_ptr() + GUARD
            else:  # the yu_iovec table {base, len} and first_iov; empty views: NULL and wild bases
                lay = P.lay
                base = np.array([t.data_ptr() for t in memory], np.uint64)[lay.vp] + np.uint64(GUARD) + lay.vo.astype(np.uint64)
                base[lay.vl == 0] = np.where(np.arange(lay.vl.size) % 2, 0xDEAD0001, 0).astype(np.uint64)[lay.vl == 0]
                tables = [np.stack((base, lay.vl.astype(np.uint64)), 1), lay.first.astype(np.uint64)]
                first_arg = None
            pt = [Placed(torch, dev, t, 8 if offset else 0, 16 if offset else 256) for t in tables]
            placed += pt
            assert not offset or all(x.ptr % 16 == 8 for x in pt)
            f = getattr(L, "yu_csum_%s_%s" % ("fill" if fill else "batch", "ragged" if layout == "R" else "iov"))
            rc = f(first_arg if layout == "R" else pt[0].ptr, pt[-1].ptr, n, K.MODES.index(mode), *tail)
        if rc != 0:
            return f"status {rc}"
    err = None if "null_out" in shapes else check_out(big.cpu().numpy(), lo, want)
    if err is None and "null_out" in shapes and not (big.cpu().numpy() == OUT_FILL).all():
        err = "the result allocation changed in a call without out"
    exp = expected_memory(case, P)
    for k, t in enumerate(memory):
        err = err or check_memory(t.cpu().numpy(), exp[k] if P.lay is not None else exp,
                                  f"the expected pool {k}" if P.lay is not None else "the expected buffer")
    if err is None and any(x.changed() for x in placed):
        err = "a side array, a table or its guard bytes changed"
    return err


def main():
    s = int(sys.argv[1])
    import torch
    from oracle import oracle as O
    from yustack_amd import batch
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    oracle = O.C()
    cases = [c for c in K.CASES if s in c["plans"]]
    print(f"set {s} {K.KNOB_SETS[s]}: {len(cases)} cases, {cus} CUs", flush=True)
    t0 = time.perf_counter()
    for c in cases:
        err = run_case(c, s, cus, dev, oracle, torch, batch)
        print(f"{'FAIL' if err else 'ok'} {c['id']}{': ' + err if err else ''}", flush=True)
        if err:
            return 1
    torch.cuda.synchronize()
    print(f"ledger set {s}: {len(cases)} cases in {time.perf_counter() - t0:.2f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
