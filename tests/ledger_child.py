"""Runs the ledger cases (tests/kernel_cases.py) of one knob set on the GPU:
    python tests/ledger_child.py <knob set index>
The knobs are in the environment already (tests/test_gpu_kernel_ledger.py sets them:
the library reads them once). Per case: the library names the written kernel; the results
equal the C oracle's on the same bytes; the 64 guard entries after the results are
untouched; in place, the packets are a view into a buffer with 128 guard bytes on each
side, and afterwards every byte of that buffer equals the input except the fields the
oracle defines, which hold its values big-endian. One line per case; exits non-zero at
the first mismatch."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import kernel_cases as K  # noqa: E402
import rxgen  # noqa: E402

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
            headers(rng, buf, starts, ln, mode, case["fill"])
        return buf, starts, starts + ln
    name, lo, hi = case["gen"]
    if dgram:
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
        headers(rng, buf, offs[:-1], lens, mode, case["fill"])
    return buf, offs[:-1], offs[1:]


def run_case(case, s, cus, dev, oracle, torch, batch):
    env = K.KNOB_SETS[s]
    n = K.resolve_n(case, cus, env)
    mode, fill = case["mode"], case["fill"]
    rng = np.random.default_rng(int(case["id"].split()[0]) * 16 + s)
    kernel = case["plans"][s].split()[0]
    uniform = case["layout"] == "U"
    name = (batch.variant(case["stride"], case["len"], mode, case["base"], n=n) if uniform
            else batch.ragged_variant(mode, n, fill=fill))
    if name != kernel:
        return f"the library names {name}"
    buf, starts, ends = build(case, n, rng)
    side = case["side"]
    init = rng.integers(0, 65536, size=n, dtype=np.uint16) if side == "init" else None
    addrs = rng.integers(0, 256, size=8 * n, dtype=np.uint8) if side == "addrs" else None
    initial = 0x1234 if side == "scalar" and mode in K.SIDES else 0
    k = 2 if mode == "tx_datagram" else 1
    threads = 8 if buf.size > (1 << 20) else 1
    view = buf[GUARD:]
    if uniform:
        want = oracle.batch(view[case["base"]:], K.MODES.index(mode), stride=case["stride"], length=case["len"], n=n,
                            initial_arr=init, initial=initial, addrs=addrs, threads=threads)
    else:
        offs = np.append(starts, ends[-1:]).astype(np.uint64) - GUARD
        want = oracle.batch(view, K.MODES.index(mode), offsets=offs, initial_arr=init, initial=initial, addrs=addrs,
                            threads=threads)
    whole = torch.from_numpy(buf).to(dev)
    out = torch.from_numpy(np.full(n * k + OUT_GUARD, OUT_FILL, np.uint16)).to(dev)
    side_t = dict(initial=initial, initial_arr=None if init is None else torch.from_numpy(init).to(dev),
                  addrs=None if addrs is None else torch.from_numpy(addrs).to(dev), out=out, fill=fill)
    if uniform:
        batch.checksum_uniform(whole[GUARD + case["base"]:], case["stride"], case["len"], n, mode, **side_t)
    else:
        batch.checksum_ragged(whole[GUARD:], torch.from_numpy(offs.view(np.int64)).to(dev), mode, **side_t)
    got = out.cpu().numpy()
    if not np.array_equal(got[:n * k], want):
        bad = np.nonzero(got[:n * k] != want)[0]
        return f"{bad.size} results differ, first at {bad[:6].tolist()}: got {got[bad[:3]].tolist()} want {want[bad[:3]].tolist()}"
    if not (got[n * k:] == OUT_FILL).all():
        return f"guard entries after the results changed: {np.nonzero(got[n * k:] != OUT_FILL)[0][:6].tolist()}"
    after = whole.cpu().numpy()
    exp = buf
    if fill:
        exp = buf.copy()
        if mode == "tx_datagram":
            pos, val = datagram_fields(buf, starts, ends, want)
        else:
            pos, val = starts + K.FIELD[mode], want
        exp[pos] = (val >> 8).astype(np.uint8)
        exp[pos + 1] = (val & 0xFF).astype(np.uint8)
    if not np.array_equal(after, exp):
        bad = np.nonzero(after != exp)[0]
        return f"{bad.size} bytes differ from the expected buffer, first at {(bad[:6] - GUARD).tolist()} (view offsets)"
    return None


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
