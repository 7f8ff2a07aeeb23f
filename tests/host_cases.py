"""The host ledger: the batches that go through the host-memory entry points
(yu_csum_batch_host_* / yu_csum_fill_host_*, yustack_amd/csrc/yucsum_host.cpp) on the
GPU, placed where that code cuts: slice seams, slot reuse, the two routes, the shard
split, the staging copies and the host field writer.

tests/test_host_ledger.py (CPU) checks that the enumeration plants what it claims, told
by the model tests/host_slices.py and not by a recipe's name; tests/host_child.py runs
the cases of one knob set on the GPU; tests/test_gpu_host_ledger.py starts one child per
knob set.

A case is a dict:
  id       its position in CASES and what it is (cases are only appended: a case's bytes
           are seeded from its position)
  set      the index into KNOB_SETS of the process environment it runs under
  layout   "U" (uniform), "R" (ragged) or "V" (views: scatter-gather)
  mode     one of kernel_cases.MODES
  call     "batch", "fill", or "fill_null" (h_out == NULL at the C ABI)
  inmem    "pageable" | "pinned" | "pinned_odd" (pinned, the data at an odd address inside
           the allocation); `align`: the data address modulo 16 (pinned_odd: odd)
  off0     ragged: offsets[0] (odd and above 0 where it is not 0)
  outmem   "pageable" | "pinned2" (pinned, at 2 modulo 4); guard entries on both sides
  side     "addrs" | "init" (the array the mode reads), "absent" (none; the scalar initial
           where the mode takes one) or "junk" (junk values in full-size arrays, and
           initial = 0xBEEF, in the arguments the mode ignores, next to the ones it reads)
  devices  0, or a list such as [0, 0, 0]: the _multi call
  plan     (recipe, arguments...): the packet lengths (lengths(case)); `views`: how a "V"
           case cuts its packets into views
"""
import hashlib

import numpy as np

import host_slices as S
import kernel_cases as K

MODES = K.MODES
TX_MODES = ["udp", "tcp", "ipv4", "icmp", "tx_datagram"]
PSEUDO = ["udp", "tcp", "verify_tcp", "verify_udp"]  # addrs or initial_arr; RAW: initial_arr
MIN_LEN = dict(K.MIN_LEN)  # the least length the ledgers give a mode (0: RAW and the datagram modes)
# below these the value is not defined (include/yucsum.h [len-min]; the oracle is not asked)
UNDEFINED_BELOW = {"udp": 8, "tcp": 20, "icmp": 4, "verify_tcp": 20}

KNOB_SETS = [
    {},
    {"YU_HOST_SLICE_BYTES": "4096", "YU_HOST_SLICE_PACKETS": "16"},
    {"YU_HOST_SLICE_BYTES": "4096", "YU_HOST_SLICE_PACKETS": "16", "YU_HOST_DIRECT_MAX": "0"},
    {"YU_HOST_SLICE_BYTES": "65536", "YU_HOST_SLICE_PACKETS": "16", "YU_HOST_DIRECT_MAX": "1024",
     "YU_HOST_COPY_THREADS": "0"},
]
H0, H1, H2, H3 = range(4)
COPY_THREADS = 7  # the library's default staging helpers (yucsum_host.cpp CopyPool)


def limits(s):
    """(slice bytes, slice packets, direct cut-over) of a knob set."""
    env = KNOB_SETS[s]
    return (S.limit(env.get("YU_HOST_SLICE_BYTES"), S.SLICE_BYTES),
            S.limit(env.get("YU_HOST_SLICE_PACKETS"), S.SLICE_PACKETS),
            int(env.get("YU_HOST_DIRECT_MAX", S.DIRECT_MAX)))


CASES = []


def seed_of(case):
    return 0x4057 * 65536 + int(case["id"].split()[0])


# ---------------------------------------------------------------------------
# Recipes: packet lengths of a ragged or view batch, slice by slice. Every recipe is
# built against the limits of the case's knob set; what it plants is read back from the
# model's cut (facts), never from its name.
# ---------------------------------------------------------------------------
def _parts(rng, total, cnt, m, first_min=0):
    """cnt lengths >= m (the first >= first_min) that sum to total."""
    first_min = max(first_min, m)
    extra = total - (cnt - 1) * m - first_min
    assert extra >= 0 and cnt >= 1, (total, cnt, m, first_min)
    for _ in range(100):
        cuts = np.sort(rng.integers(0, extra + 1, size=cnt - 1))
        p = np.diff(np.concatenate(([0], cuts, [extra]))) + m
        p[0] += first_min - m
        if p.max() <= 60000:
            return [int(x) for x in p]
    raise AssertionError("no composition")


class _Builder:
    def __init__(self, rng, lim_b, lim_p, m):
        self.rng, self.b, self.p, self.m = rng, lim_b, lim_p, m
        self.lens, self.need = [], 0  # need: the least first packet that opens a new slice here

    def by_bytes(self, r=None, cnt=None):
        """A slice of lim_b - r bytes, closed by the byte limit (the next packet is longer than r)."""
        r = int(self.rng.integers(0, max(self.m, 9))) if r is None else r
        first = max(self.need, self.m)
        most = min(self.p - 1, (self.b - r - first) // max(self.m, 1) + 1)
        cnt = cnt or int(self.rng.integers(2, max(most, 2) + 1))
        self.lens += _parts(self.rng, self.b - r, cnt, self.m, first)
        self.need = r + 1
        return self

    def by_packets(self, total=None):
        """A slice of lim_p packets, closed by the packet limit."""
        first = max(self.need, self.m)
        low = first + (self.p - 1) * self.m
        total = int(self.rng.integers(low, max(low, min(self.b // 8, low + 400)) + 1)) if total is None else total
        self.lens += _parts(self.rng, total, self.p, self.m, first)
        self.need = 0
        return self

    def tail(self, cnt=None, most=60):
        """A last slice: fewer packets than the limit, few bytes."""
        cnt = cnt or int(self.rng.integers(1, self.p))
        first = max(self.need, self.m, 1)
        self.lens += [first + int(self.rng.integers(0, most))] + [self.m + int(x) for x in
                                                                   self.rng.integers(0, most, size=cnt - 1)]
        self.need = 0
        return self

    def raw(self, lens):
        self.lens += [int(x) for x in lens]
        self.need = 0
        return self


def lengths(case):
    """The packet lengths of a ragged or view case (uniform: (stride, len, n))."""
    name, *a = case["plan"]
    lim_b, lim_p, _ = limits(case["set"])
    m = MIN_LEN.get(case["mode"], 0)
    rng = np.random.default_rng(a[-1] if name in ("exact", "one_over") else seed_of(case) ^ 0x5A5A)
    B = _Builder(rng, lim_b, lim_p, m)
    if name == "uniform":
        return tuple(a)
    if name == "lens":  # written out
        return np.asarray(a[0], np.int64)
    if name == "draw":  # n lengths in [lo, hi] (the shipped limits)
        n, lo, hi = a
        return rng.integers(lo, hi + 1, size=n).astype(np.int64)
    if name == "fill_first":  # a first slice of exactly lim_b bytes in `size`-byte packets, then three more
        size, = a
        return np.asarray([size] * (lim_b // size) + [lim_b % size or size] * (1 if lim_b % size else 0) + [size] * 3, np.int64)
    if name == "one":  # one slice of at most `most` bytes
        most, = a
        cnt = int(rng.integers(2, lim_p))
        total = int(rng.integers(cnt * max(m, 1), min(most, lim_b, cnt * (m + 80)) + 1))
        B.raw(_parts(rng, total, cnt, m))
    elif name == "one_exact":  # one slice of exactly `total` bytes
        B.raw(_parts(rng, a[0], 5, m))
    elif name == "slices":  # k slices, closed by the byte and the packet limit in turn
        k, variant = a
        for j in range(k - 1):
            B.by_bytes() if (j + variant) % 2 == 0 and lim_b <= 8192 else B.by_packets()
        B.tail()
    elif name == "last_one":
        k, = a
        for j in range(k - 1):
            B.by_bytes() if j % 2 and lim_b <= 8192 else B.by_packets()
        B.tail(cnt=1)
    elif name in ("exact", "one_over"):  # the same batch; one_over: one byte more in slice 0's last packet
        B.by_bytes(r=0, cnt=int(rng.integers(3, 9)))
        last = len(B.lens) - 1
        B.tail(cnt=3)
        if name == "one_over":
            B.lens[last] += 1
    elif name == "packet_limit":
        B.by_packets().by_packets().tail()
    elif name == "zeros":  # 16 or more empty packets that make slices of zero bytes
        variant, = a
        if variant % 2:
            B.by_packets()
        B.raw([0] * (lim_p * (1 + variant // 2))).tail()
    elif name == "empty_edges":
        B.raw([0] + _parts(rng, int(rng.integers(200, 900)), lim_p - 2, 1) + [0]).raw([0, 33, 0]).tail()
    elif name.startswith("long_"):
        long_ = lambda: lim_b + int(rng.integers(1, 2000))  # noqa: E731
        if name == "long_first":
            B.raw([long_()]).tail()
        elif name == "long_last":
            B.tail().raw([long_()])
        elif name == "long_middle":
            B.tail(cnt=3).raw([long_()]).tail(cnt=2)
        else:  # long_twice
            B.tail(cnt=2).raw([long_(), long_()]).tail(cnt=2)
    elif name == "equal":  # n packets of one length: slices by the packet limit, shards on or off them
        n, ln = a
        B.raw([ln] * n)
    elif name == "short":  # packets around the mode's header sizes, 0 and 1 bytes among them
        n, = a
        B.raw(rng.integers(0, 30, size=n))
        B.lens[0], B.lens[-1] = 0, 1
    else:
        raise AssertionError(name)
    return np.asarray(B.lens, np.int64)


def shards(case, lens_or_uniform):
    """([(first, count)] of the packets each call of the case's pipeline gets, the bounds)."""
    if case["layout"] == "U":
        n = lens_or_uniform[2]
    else:
        n = len(lens_or_uniform)
    dv = case["devices"]
    if not isinstance(dv, list):
        return [(0, n)], [0, n]
    if case["layout"] == "R":
        off = np.concatenate(([case["off0"]], case["off0"] + np.cumsum(lens_or_uniform)))
        b = S.byte_bounds_np(off, len(dv))
    else:
        b = S.even_bounds(n, len(dv))
    return [(b[i], b[i + 1] - b[i]) for i in range(len(dv)) if b[i + 1] > b[i]], b


def facts(case):
    """What the model says of a case: its cuts (one per shard), seam classes, route,
    predicted staging. Memoised on the case."""
    if "_facts" in case:
        return case["_facts"]
    lim_b, lim_p, dmax = limits(case["set"])
    g = lengths(case)
    uniform = case["layout"] == "U"
    if uniform:
        stride, ln, n = g
        whole = S.cut_uniform(stride, ln, n, lim_b, lim_p)
        classes = S.classes_uniform(stride, ln, n, lim_b, lim_p)
    else:
        n = len(g)
        whole = S.cut_lens(g, lim_b, lim_p)
        classes = S.classes_lens(g, lim_b, lim_p)
    sh, bounds = shards(case, g)
    classes |= S.classes_multi(whole, bounds)
    cuts = []
    for first, cnt in sh:
        cuts.append(S.cut_uniform(g[0], g[1], cnt, lim_b, lim_p) if uniform else
                    S.cut_lens(g[first:first + cnt], lim_b, lim_p))
    # staging: per pool, the component-wise largest slice over the shards that take it
    pinned = device = 0
    routes = set()
    for burst in (True, False):
        mine = [c for c in cuts if S.is_burst(c, dmax) == burst]
        if mine:
            routes.add("direct" if burst else "copied")
            max_b, max_pk = max(S.largest(c)[0] for c in mine), max(S.largest(c)[1] for c in mine)
            # (a context that grew past the shipped bounds, for a packet longer than a slice,
            # gives everything back when the call returns: include/yucsum.h)
            if max_b <= (S.DIRECT_MAX if burst else S.SLICE_BYTES) and max_pk <= S.SLICE_PACKETS:
                p, d = S.staging(max_b, max_pk, burst)
                pinned, device = pinned + p, device + d
    f = dict(n=n, geometry=g, shards=sh, cuts=cuts, classes=classes, routes=routes, staging=(pinned, device),
             slices=max(len(c) for c in cuts), multi=isinstance(case["devices"], list),
             data_bytes=(g[2] - 1) * g[0] + g[1] if uniform else int(np.sum(g)))
    case["_facts"] = f
    return f


# ---------------------------------------------------------------------------
# The enumeration.
# ---------------------------------------------------------------------------
INMEM = ["pageable", "pinned", "pinned_odd"]
OUTMEM = ["pageable", "pinned2"]


def sides_of(mode):
    if mode in PSEUDO:
        return ["addrs", "init", "absent", "junk"]
    if mode == "raw":
        return ["init", "absent", "junk"]
    return ["absent", "junk"]


def add(s, layout, mode, plan, *, call="batch", side=None, devices=0, inmem=None, outmem=None, views="rand",
        off0=None, align=None):
    k = len(CASES)
    assert call == "batch" or mode in TX_MODES
    side = side or sides_of(mode)[k % len(sides_of(mode))]
    inmem = inmem or INMEM[k % 3]
    if align is None:
        align = (2 * k + 1) % 16 if inmem == "pinned_odd" else (0, 4, 8, 3, 6)[k % 5]
    off0 = off0 if off0 is not None else ((0, 7, 101)[k % 3] if layout == "R" else 0)
    c = dict(set=s, layout=layout, mode=mode, call=call, inmem=inmem, align=align, off0=off0,
             outmem=outmem or OUTMEM[(k // 3) % 2], side=side, devices=devices, plan=tuple(plan), views=views)
    what = " ".join(str(x) for x in plan if not isinstance(x, (list, np.ndarray)))
    c["id"] = (f"{k:04d} H{s} {layout} {mode} {call} {what} in={inmem}@{align}"
               f"{'+' + str(off0) if off0 else ''} out={c['outmem']} {side}"
               f"{' dev=' + str(devices) if devices else ''}{' views=' + views if layout == 'V' else ''}")
    CASES.append(c)
    return c


def _uniform(mode, lim_b, lim_p, k, what):
    """(stride, len, n) of a uniform recipe."""
    ln = max(MIN_LEN.get(mode, 0), 20) + 4 * (k % 9)
    stride = ln + 4 * (k % 3)
    per = min(lim_p, max(1, lim_b // stride))
    if what == "one":
        return stride, ln, max(per - 1 - k % 3, 1)
    if isinstance(what, int):  # that many slices
        return stride, ln, per * (what - 1) + 1 + k % per
    if what == "last_one" or what == "n_multiple_plus1":
        return stride, ln, per * (3 + k % 2) + 1
    if what == "n_multiple":
        return stride, ln, per * (2 + k % 3)
    if what == "stride0":
        return 0, ln, lim_p * 2 + 1 + k % 5
    if what == "stride_lt_len":
        return ln - 1 - k % 7, ln, lim_p * 3 + k % 4
    if what == "stride_gt_slice":
        return lim_b + 4 * (1 + k % 4), ln, (4, 7, 3, 5)[k % 4]
    raise AssertionError(what)


def _enumerate():
    # --- every (layout, mode): direct, one slice copied, four or more slices; H3's two routes
    for layout in "URV":
        for mode in MODES:
            k = len(CASES)
            for s in (H1, H2):
                lim_b, lim_p, _ = limits(s)
                add(s, layout, mode, ("uniform", *_uniform(mode, lim_b, lim_p, k, "one")) if layout == "U" else ("one", 3000))
            for s, slices in ((H1, 4), (H2, 7), (H3, 4)):
                lim_b, lim_p, _ = limits(s)
                side = None
                if mode in PSEUDO:
                    side = ("addrs", "init", "addrs")[s - 1] if layout != "R" else ("init", "addrs", "init")[s - 1]
                elif mode == "raw":
                    side = "init"
                add(s, layout, mode, ("uniform", *_uniform(mode, lim_b, lim_p, k + s, slices)) if layout == "U" else
                    ("slices", slices, k % 2), side=side)
            lim_b, lim_p, _ = limits(H3)
            if layout == "U":
                ln = max(MIN_LEN.get(mode, 0), 20) + 12  # 1024 bytes: direct; 1025: a bulk context
                add(H3, layout, mode, ("uniform", 124, ln, (1024 - ln) // 124 + 1), inmem="pinned")
                assert 124 * ((1024 - ln) // 124) + ln <= 1024
                add(H3, layout, mode, ("uniform", 124, ln + 1, (1024 - ln) // 124 + 1))
            else:
                add(H3, layout, mode, ("one_exact", 1024))
                add(H3, layout, mode, ("one_exact", 1025))
    # --- seam classes, four of each per layout, modes and memory in rotation
    any_len = [m for m in MODES if MIN_LEN.get(m, 0) == 0]  # empty packets: RAW and the datagram modes
    for layout in "RV":
        for ci, (plan, modes, sets) in enumerate([
                (lambda j: ("slices", 2, j), MODES, (H1, H2)), (lambda j: ("slices", 3, j), MODES, (H1, H2, H3)),
                (lambda j: ("slices", 7, j), MODES, (H1, H2)), (lambda j: ("last_one", 2 + j), MODES, (H1, H2, H3)),
                (lambda j: ("exact", 900 + 10 * ci + j), MODES, (H1, H2)),
                (lambda j: ("one_over", 900 + 10 * (ci - 1) + j), MODES, (H1, H2)),
                (lambda j: ("packet_limit",), MODES, (H1, H2, H3)), (lambda j: ("zeros", j), any_len, (H1, H2, H3)),
                (lambda j: ("empty_edges",), any_len, (H1, H2, H3)), (lambda j: ("long_first",), MODES, (H1, H2)),
                (lambda j: ("long_middle",), MODES, (H1, H2)), (lambda j: ("long_last",), MODES, (H1, H2)),
                (lambda j: ("long_twice",), MODES, (H1, H2))]):
            for j in range(4):
                mi = ci - 1 if plan(j)[0] == "one_over" else ci  # (the same batch as its `exact` twin)
                mode = modes[(3 * mi + j + (layout == "V")) % len(modes)]
                call = ("fill", "fill_null")[j % 2] if mode in TX_MODES and j >= 2 else "batch"
                add(sets[j % len(sets)], layout, mode, plan(j), call=call)
    for ci, what in enumerate(["last_one", "stride0", "stride_lt_len", "stride_gt_slice", "n_multiple",
                               "n_multiple_plus1", 2, 3, 7]):
        for j in range(4):
            s = (H1, H2, H3, H1)[j]
            lim_b, lim_p, _ = limits(s)
            # (overlapping packets: not the modes whose packets carry a contract of their own)
            modes = [m for m in MODES if m not in ("tcp", "verify_tcp", "tx_datagram")] if what == "stride_lt_len" else MODES
            mode = modes[(3 * ci + j) % len(modes)]
            overlap = what in ("stride0", "stride_lt_len")
            call = "fill" if mode in TX_MODES and j >= 2 and not overlap else "batch"
            add(s, "U", mode, ("uniform", *_uniform(mode, lim_b, lim_p, 5 * ci + j, what)), call=call)
    # --- _multi: a shard edge on a slice edge, and one off it
    for layout in "URV":
        for j in range(8):
            s = (H1, H2)[j % 2]
            on = j < 4
            ndev = 2 + j % 2
            mode = MODES[(j + 3 * "URV".index(layout)) % 10]
            n = 16 * ndev if on else 16 * ndev + (2, 5)[j % 2]
            ln = max(MIN_LEN.get(mode, 0), 20) + 4 * j
            add(s, layout, mode, ("uniform", ln + 4, ln, n) if layout == "U" else ("equal", n, ln), devices=[0] * ndev,
                side="init" if mode == "raw" else "addrs" if mode in PSEUDO else None)
    # --- the TX modes in place: fill and fill_null on both routes, every layout
    for layout in "URV":
        for mode in TX_MODES:
            for call in ("fill", "fill_null"):
                for s, slices in ((H1, 1), (H2, 1), (H1, 3), (H3, 1)):
                    lim_b, lim_p, _ = limits(s)
                    k = len(CASES)
                    views = "split_field" if layout == "V" and k % 2 else "rand"
                    if layout == "U":
                        plan = ("uniform", *_uniform(mode, lim_b, lim_p, k, "one" if slices == 1 else slices))
                    else:
                        plan = ("one", 3000) if slices == 1 else ("slices", slices, k % 2)
                    add(s, layout, mode, plan, call=call, views=views)
    # --- TX_DATAGRAM: two results per packet across seams, pinned and pageable h_out
    for layout in "URV":
        for outmem in OUTMEM:
            for call in ("batch", "fill"):
                lim_b, lim_p, _ = limits(H1)
                add(H1, layout, "tx_datagram", ("uniform", *_uniform("tx_datagram", lim_b, lim_p, len(CASES), 4))
                    if layout == "U" else ("slices", 4, len(CASES) % 2), call=call, outmem=outmem)
    # --- the host field writer where packets are short or malformed (no result array: below a
    #     mode's header size a value is not defined; the packet memory is the evidence)
    for layout in "RV":
        for mode in ("udp", "icmp", "ipv4", "tx_datagram"):
            for s in (H1, H2):
                add(s, layout, mode, ("short", 40), call="fill_null", views=("split_field", "ones")[s - 1])
    # --- a batch of a few bytes (its staging: 16 bytes at the least)
    add(H1, "R", "raw", ("lens", [3, 0, 2]), side="init")
    add(H2, "V", "raw", ("lens", [1]), side="absent")
    add(H2, "U", "icmp", ("uniform", 4, 4, 2))
    # --- H0: the shipped constants at their real sizes
    P, Bb = S.SLICE_PACKETS, S.SLICE_BYTES
    for n in (P, P + 1):
        add(H0, "R", "raw", ("draw", n, 0, 40), side="init", inmem="pageable")
        add(H0, "V", "tx_datagram", ("draw", n, 0, 40), views="one", call="batch" if n == P else "fill",
            outmem="pinned2" if n == P else "pageable")
        add(H0, "U", "verify_udp", ("uniform", 8, 8, n), side="addrs", inmem="pinned")
    add(H0, "R", "verify_tcp", ("fill_first", 1500), side="addrs", inmem="pageable")  # slice 0 ends at 32 MiB exactly
    add(H0, "R", "raw", ("lens", [33 << 20]), side="absent", inmem="pageable")  # one RAW packet past a slice
    for nbytes in ((2 << 20) - 1, 2 << 20, (2 << 20) + 1, (8 << 20) + 63):  # stage_copy's split
        n = (nbytes + 32767) // 32768
        add(H0, "U", "raw", ("uniform", 32768, nbytes - (n - 1) * 32768, n), inmem="pageable", align=0,
            side=("init", "absent")[n % 2])
    add(H0, "V", "raw", ("lens", [3 << 20, 3 << 20, 2 << 20]), views="one", side="init")  # gather: fewer packets than threads
    add(H0, "V", "udp", ("draw", 3000, 900, 1500), views="rand", side="addrs")  # and more
    for n in (1 << 17, (1 << 17) + 1):  # the parallel set_fields
        add(H0, "R", "udp", ("draw", n, 8, 40), call="fill", side="addrs", inmem="pageable")
        add(H0, "U", "tx_datagram", ("uniform", 44, 40, n), call="fill_null", inmem="pinned")
    for a in range(16):  # the direct path from pinned memory at every data alignment
        add(H0, "UR"[a % 2], MODES[a % 10], ("uniform", 1500 + a, 1500, 64) if a % 2 == 0 else ("draw", 64, 64, 1500),
            inmem="pinned_odd" if a % 2 else "pinned", align=a, off0=0)


_enumerate()


def digest():
    return hashlib.sha256("\n".join(c["id"] for c in CASES).encode()).hexdigest()[:16]
