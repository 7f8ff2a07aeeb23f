"""The kernel ledger: for every function the planner (yustack_amd/csrc/yucsum_plan.h)
can name, the batches that are compared with the C oracle on the GPU, and the plan
each one is expected to get, as written text "kernel form policy".

tests/test_kernel_ledger.py (CPU) checks the written plans against the planner and
that the cases cover every reachable key (kernel, form, policy, in place, layout);
tests/ledger_child.py runs the cases of one knob set on the GPU;
tests/test_gpu_kernel_ledger.py starts one child per knob set.

A case is a dict:
  id        its position in CASES and a short description (cases are only appended: the
            child seeds a case's bytes from its position)
  layout    "U" (uniform: stride, len, base = the first packet's offset in a 128-byte
            aligned buffer), "R" (ragged: gen = (name, lo, hi), base; ("seam", CH, T): a batch
            of tests/seg_seams.py for a kind with CH-packet chunks and T-byte tiles) or "I" (scatter-gather,
            k_iov: iov = the view shape, iov_packets)
  mode, fill, side ("scalar" | "init" | "addrs")
  kind      "rand" | "zero" | "ff" (constant bytes), or a zero pole: "pole_side"
            (initial_arr solved so that every packet sums to its pole) or "pole_data" (the
            16-bit word at POLE_W solved instead); the pole is 0x0000 for UDP, TCP, ICMP and
            IPV4, 0xFFFF for RAW and the VERIFY modes (pole)
  call      how the call is made: "plain" (through batch.py, fresh aligned arrays), or the
            C ABI itself with any of "offset" (out, initial_arr, addrs, offsets and the
            scatter-gather tables at the least alignment include/yucsum.h allows),
            "null_out" (in place, out = NULL) and "ignored" (junk in the arguments the mode
            does not use: ignores), joined by "+"
  n         the packet count, or "n_wrap": the smallest n above one pass of the grid
            (resolve_n), kept within [n_lo, n_hi], the planner's count cut-overs
  ppw       packets per wave the plan is expected to have (n_wrap needs it)
  plans     {knob set index: "kernel form policy"}: the sets the case runs under
"""

MODES = ["raw", "udp", "tcp", "ipv4", "icmp", "verify_ipv4", "verify_tcp", "verify_udp", "verify_rx",
         "tx_datagram"]
MIN_LEN = {"udp": 8, "tcp": 20, "icmp": 4, "ipv4": 20, "verify_ipv4": 20, "verify_tcp": 20, "verify_udp": 8}
FIELD = {"udp": 6, "tcp": 16, "icmp": 2, "ipv4": 10}
SIDES = {"raw": ("scalar", "init"), "udp": ("addrs", "init", "scalar"), "tcp": ("addrs", "init", "scalar"),
         "verify_tcp": ("addrs", "init", "scalar"), "verify_udp": ("addrs", "init", "scalar")}
SMALL_BURST, MID_BATCH = 4096, 65536  # the planner's count cut-overs (yucsum_plan.cpp)
MAX_CASE_BYTES = 64 << 20
CU_COUNTS = (64, 256, 304)

# ---------------------------------------------------------------------------
# Knob sets. The first is the production choice (no knob, no YU_TUNING). The keys need
# YU_RAGGED in {unset, seg4} x YU_FILL_WB in {unset, 0} x YU_NT in {0, 1, 2}: k_seg<4,tx>
# and k_seg<4,txw> write ragged batches in place only under seg4 with the write-back off
# and on, k_seg<8,tx,c16> / k_seg<8,tx> and k_seg<8,txw,c16> / k_seg<8,txw,c48> only
# without seg4, and each has three policy slots: 12 environments, none of which can stand
# for another, plus the default one.
# ---------------------------------------------------------------------------
KNOB_SETS = [{}]


def _add_set(rag, wb, nt):
    env = {"YU_BLOCKS_PER_CU": "1", "YU_NT": str(nt)}
    if rag:
        env["YU_RAGGED"] = rag
    if not wb:
        env["YU_FILL_WB"] = "0"
    if not rag:  # k_small: runs at every count / never (the uniform picks ignore YU_RAGGED)
        env["YU_RUNS"] = "2" if wb else "0"
    if (rag, wb, nt) in ((None, 0, 2), ("seg4", 1, 1)):
        env["YU_XCD"] = "1"
    if (rag, wb, nt) in ((None, 1, 1), ("seg4", 0, 0)):
        env["YU_SEG_SMALL_BLOCKS"] = "0"
    KNOB_SETS.append(env)


for _rag in (None, "seg4"):
    for _wb in (1, 0):
        for _nt in (0, 1, 2):
            _add_set(_rag, _wb, _nt)
MAX_KNOB_SETS = 13


def trio(rag, wb):
    """The three sets (YU_NT = 0, 1, 2) with this YU_RAGGED and YU_FILL_WB."""
    first = 1 + (6 if rag else 0) + (0 if wb else 3)
    return [first, first + 1, first + 2]


DEFAULT = [0]
RUNS2, RUNS0 = trio(None, 1), trio(None, 0)  # YU_RUNS=2 / YU_RUNS=0
SEG4_WB, SEG4_NOWB = trio("seg4", 1), trio("seg4", 0)  # YU_RUNS unset

CASES = []


def _policy(s, fill, fill_plain):
    nt = KNOB_SETS[s].get("YU_NT")
    return int(nt) if nt is not None else (0 if fill and fill_plain else 2)


def kernel_of(c):
    """(kernel, form) of a case: the same under every set it runs in."""
    return tuple(next(iter(c["plans"].values())).split()[:2])


def _append(c):
    """Gives the case its id (its position in CASES and what it is) and appends it."""
    kernel, form = kernel_of(c)
    g = (f"{c['len']}/{c['stride']}@{c['base']}" if c["layout"] == "U" else c["iov"] if c["layout"] == "I" else
         "%s[%d..%d]@%d" % (*c["gen"], c["base"]))
    c["id"] = (f"{len(CASES):04d} {kernel} {form} {c['layout']} {c['mode']}{' fill' if c['fill'] else ''} {g} "
               f"n={c['n']} {c['side']} {c['kind']}{'' if c['call'] == 'plain' else ' ' + c['call']}")
    CASES.append(c)


def _add(layout, kernel, form, mode, sets, n, ppw, *, fill=False, fill_plain=False, side=None, kind="rand",
         n_lo=1, n_hi=None, call="plain", **geom):
    if side is None:  # rotate through what the mode takes
        allowed = SIDES.get(mode, ("scalar",))
        side = allowed[len(CASES) % len(allowed)]
    assert side in SIDES.get(mode, ("scalar",)), (mode, side)
    _append(dict(layout=layout, mode=mode, fill=fill, side=side, kind=kind, n=n, n_lo=n_lo, n_hi=n_hi, ppw=ppw,
                 call=call, plans={s: f"{kernel} {form} {_policy(s, fill, fill_plain)}" for s in sets}, **geom))


def U(kernel, form, mode, length, stride, sets, n, ppw, base=0, **kw):
    _add("U", kernel, form, mode, sets, n, ppw, len=length, stride=stride, base=base, **kw)


def R(kernel, mode, gen, sets, n, ppw, base=0, **kw):
    _add("R", kernel, "plain", mode, sets, n, ppw, gen=gen, base=base, **kw)


def _counts(ppw):
    return sorted({1, max(ppw - 1, 1), ppw, ppw + 1})


PLAIN6 = ["raw", "udp", "tcp", "icmp", "verify_tcp", "verify_udp"]
FILL3 = ["udp", "tcp", "icmp"]
KINDS = ["rand", "zero", "ff"]


def _per_packet(kernel, form, fill_form, shapes, ppw, tuned, *, fill_plain=False, modes=PLAIN6, fills=FILL3,
                bases=(0,), fill_ppw=None, default=True):
    """One per-packet kernel on uniform batches. `shapes`: (len, stride) pairs the kernel
    takes at the given bases. Under the default set every mode with every side it takes
    (and in place); under the `tuned` trio every shape at n in {1, ppw-1, ppw, ppw+1},
    rotating modes, side data and data kinds, and n_wrap once read-only and once in place."""
    fill_ppw = fill_ppw or ppw
    k = len(CASES)

    def fillable(mode):
        return [s for s in shapes if s[0] >= MIN_LEN.get(mode, 0) and s[1] % 4 == 0 and s[1] >= s[0]]

    if default:
        for mode in modes:
            ok = [s for s in shapes if s[0] >= MIN_LEN.get(mode, 0)]
            for side in SIDES.get(mode, ("scalar",)):
                ln, st = ok[k % len(ok)]
                U(kernel, form, mode, ln, st, DEFAULT, 37, None, base=bases[k % len(bases)], side=side)
                k += 1
        for mode in fills:
            ln, st = fillable(mode)[k % len(fillable(mode))]
            U(kernel, fill_form, mode, ln, st, DEFAULT, 37, None, fill=True, fill_plain=fill_plain,
              base=bases[k % len(bases)] & ~3)
            k += 1
    for ln, st in shapes:
        ok = [m for m in modes if ln >= MIN_LEN.get(m, 0)]
        for n in _counts(ppw):
            U(kernel, form, ok[k % len(ok)], ln, st, tuned, n, ppw, base=bases[k % len(bases)], kind=KINDS[k % 3])
            k += 1
    for j, mode in enumerate(fills):
        ln, st = fillable(mode)[(k + j) % len(fillable(mode))]
        for n in (_counts(fill_ppw)[j % len(_counts(fill_ppw))], "n_wrap" if j == 0 else 37):
            U(kernel, fill_form, mode, ln, st, tuned, n, fill_ppw, fill=True, fill_plain=fill_plain,
              base=bases[(k + j) % len(bases)] & ~3)
    ln, st = shapes[0]
    U(kernel, form, [m for m in modes if ln >= MIN_LEN.get(m, 0)][0], ln, st, tuned, "n_wrap", ppw, base=bases[0])


# ---------------------------------------------------------------------------
# k_lane<U>: dense 4-aligned packets up to 112 bytes, stride in (16(U-1), 16U]
# ---------------------------------------------------------------------------
for _u in range(2, 9):
    _w = 16 * _u
    _shapes = ([(3, 4), (20, 20), (29, 32), (32, 32)] if _u == 2 else
               [(86, 128), (112, 116), (109, 128), (112, 128)] if _u == 8 else
               [(_w - 12, _w - 12), (_w - 3, _w), (_w - 1, _w), (_w, _w)])
    _per_packet(f"k_lane<{_u}>", "plain", "plain", _shapes, 64, SEG4_WB, bases=(0, 4, 60, 124))

# k_tiny<4>: sparse packets up to 64 bytes; k_tiny<8>: 65..128 bytes that k_lane leaves
# (its own in-place instantiation: form fill, k_tiny<4> only)
_per_packet("k_tiny<4>", "plain", "fill", [(1, 4), (20, 32), (40, 64), (61, 132), (63, 128), (64, 132)], 64,
            SEG4_NOWB, bases=(0, 4, 60, 124))
_per_packet("k_tiny<8>", "plain", "plain", [(65, 100), (113, 116), (125, 128), (127, 128), (128, 128), (128, 256)],
            64, SEG4_NOWB, bases=(0, 4, 60, 124))

# ---------------------------------------------------------------------------
# k_small<G,U>: window 16*G*U. Aligned packets of 129 bytes and more (the two smallest
# windows only at unaligned starts, or at strides of 32 MiB where k_tiny's 64 packets per
# step pass 2 GiB). Lengths: the first and the last of the window, each side of a
# multiple of 16*G, and window - 3 at an unaligned base (3 head bytes: the window is full).
# ---------------------------------------------------------------------------
_SMALL = [(4, 1), (8, 1), (8, 2), (16, 2), (16, 3), (16, 4), (16, 6), (32, 4), (32, 6), (64, 4)]
_FAR = 1 << 25  # stride at which 64 packets span 2 GiB
_prev = 0
for _g, _uu in _SMALL:
    _w, _name, _p = 16 * _g * _uu, f"k_small<{_g},{_uu}>", 64 // _g
    if _w <= 128:
        # unaligned starts only (RAW and the transport modes; no in-place form there)
        _lo = 1 if _w == 64 else 62
        _sh = [(_lo, _lo), (_w - 3, _w - 3), (_w - 4, _w - 3), (max(_w - 40, 21), _w)]
        for _form, _tr, _pp in (("inter", RUNS0, _p), ("runs", RUNS2, 16)):
            _per_packet(_name, _form, "inter", _sh, _pp, _tr, fills=(), bases=(1, 2, 3, 127), default=_form == "inter")
        # in place: two packets 32 MiB apart
        for _m, _ln in (("udp", _w - 8), ("tcp", _w)):
            for _sets in (DEFAULT, RUNS0):
                U(_name, "inter", _m, _ln, _FAR, _sets, 2, _p, fill=True, fill_plain=True, side="addrs")
    else:
        _m16 = (_w - 1) // (16 * _g) * (16 * _g)  # a multiple of 16*G inside the window's range
        _sh = [(_prev + 1, _prev + 4), (_w, _w), (_w - 1, _w)]
        _sh += [(_m16 - 1, _m16), (_m16 + 1, _m16 + 4)] if _m16 > _prev + 1 else [(_w - 17, _w - 16)]
        _sh = [s for s in _sh if _prev < s[0] <= _w]
        _per_packet(_name, "inter", "inter", _sh, _p, RUNS0, fill_plain=True, bases=(0, 4, 60, 124))
        _per_packet(_name, "runs", "inter", _sh, 16, RUNS2, fill_plain=True, bases=(0, 4, 60, 124), fills=FILL3[:1],
                    fill_ppw=_p, default=False)
        # window - 3 at an unaligned base stays; window - 1 there is the next kernel's
        for _b in (1, 3):
            U(_name, "inter", "raw", _w - 3, _w - 3, RUNS0, 37, _p, base=_b)
            U(_name, "runs", "udp", _w - 3, _w + 1, RUNS2, 37, 16, base=_b)
    if _prev >= 64:  # the window before this one, less 1, at an unaligned base: 2 bytes too many for it
        U(_name, "inter", "raw", _prev - 1, _prev - 1, RUNS0, 37, _p, base=1, side="init")
        U(_name, "runs", "verify_udp", _prev - 1, _prev, RUNS2, 37, 16, base=2, side="addrs")
    _prev = _w

# ---------------------------------------------------------------------------
# k_loop<4,LE> / <4,BE>: a wave per packet. Uniform: past k_small's largest window
# (4096 bytes with the head bytes), BE past 131072 bytes (RAW). Ragged: bursts of up to
# 4096 packets.
# ---------------------------------------------------------------------------
_k = 0
for _m in PLAIN6:
    for _side in SIDES[_m] if _m in SIDES else ("scalar",):
        U("k_loop<4,LE>", "plain", _m, (4097, 4100, 9000, 65535)[_k % 4], (4100, 4100, 9001, 65536)[_k % 4], DEFAULT,
          (5, 9, 3, 2)[_k % 4], None, base=_k % 4, side=_side)
        _k += 1
for _m in FILL3:
    U("k_loop<4,LE>", "plain", _m, 4100, 4100, DEFAULT, 9, None, fill=True)
    for _n in (1, 2, "n_wrap"):
        U("k_loop<4,LE>", "plain", _m, 4100, 4104, SEG4_WB, _n, 1, fill=True, base=4)
for _ln, _st, _b in ((4094, 4094, 1), (4097, 4097, 0), (4095, 4096, 3), (9001, 9001, 2), (65535, 65535, 0)):
    for _n in (1, 2):
        U("k_loop<4,LE>", "plain", PLAIN6[_k % 6], _ln, _st, SEG4_WB, _n, 1, base=_b, kind=KINDS[_k % 3])
        _k += 1
U("k_loop<4,LE>", "plain", "tcp", 4097, 4097, SEG4_WB, "n_wrap", 1)
U("k_loop<4,LE>", "plain", "raw", 131072, 131072, SEG4_WB, 3, 1, base=1, side="init")
for _sets in (DEFAULT, SEG4_WB):
    for _ln, _b, _n, _kind in ((131073, 0, 2, "rand"), (131075, 3, 3, "ff"), (200001, 1, 1, "rand")):
        U("k_loop<4,BE>", "plain", "raw", _ln, _ln, _sets, _n, 1, base=_b, kind=_kind, side=("init", "scalar")[_n % 2])
U("k_loop<4,BE>", "plain", "raw", 131073, 131073 - 131000, SEG4_WB, "n_wrap", 1, side="init")  # overlapping: 75 KB

_RLO = {"raw": 0, "verify_udp": 8, "udp": 8, "tcp": 20, "icmp": 4, "verify_tcp": 20, "ipv4": 20, "verify_ipv4": 20}
for _sets in (DEFAULT, RUNS0):
    for _m in PLAIN6[1:]:
        for _side in SIDES.get(_m, ("scalar",)):
            R("k_loop<4,LE>", _m, ("range", _RLO[_m], 1500), _sets, 600, 1, base=_k % 4, n_hi=SMALL_BURST, side=_side)
            _k += 1
    for _m in FILL3:
        R("k_loop<4,LE>", _m, ("range", _RLO[_m], 300), _sets, 4096, 1, base=_k % 4, fill=True, n_hi=SMALL_BURST)
        _k += 1
    R("k_loop<4,BE>", "raw", ("jumbo", 0, 9000), _sets, 300, 1, base=3, n_hi=SMALL_BURST, side="init")
    R("k_loop<4,BE>", "raw", ("range", 0, 64), _sets, 4096, 1, base=1, n_hi=SMALL_BURST, side="scalar")
for _n in (1, 2, "n_wrap"):
    R("k_loop<4,LE>", "verify_udp", ("range", 8, 200), RUNS0, _n, 1, base=1, n_hi=SMALL_BURST)
    R("k_loop<4,LE>", "tcp", ("range", 20, 200), RUNS0, _n, 1, base=2, fill=True, n_hi=SMALL_BURST)
    R("k_loop<4,BE>", "raw", ("range", 0, 200), RUNS0, _n, 1, base=3, n_hi=SMALL_BURST)

# ---------------------------------------------------------------------------
# k_hdr: the IPv4 header-only modes, a lane per packet, uniform and ragged, any count
# ---------------------------------------------------------------------------
for _sets in (DEFAULT, SEG4_NOWB):
    for _m, _f in (("ipv4", False), ("verify_ipv4", False), ("ipv4", True)):
        for _ln, _st, _b, _n in ((20, 20, 0, 65), (40, 44, 4, 63), (60, 60, 0, 64), (61, 64, 0, 1), (1500, 1500, 4, 37)):
            if _sets is DEFAULT and _n not in (65, 37):
                continue
            U("k_hdr", "plain", _m, _ln, _st, _sets, _n, 64, base=_b if _f else _b + (_n & 3), fill=_f)
        R("k_hdr", _m, ("range", 20, 1500), _sets, 600, 64, base=0 if _f else 3, fill=_f)
        R("k_hdr", _m, ("range", 20, 100), _sets, 5000, 64, base=1, fill=_f)
for _m, _f in (("ipv4", False), ("verify_ipv4", False), ("ipv4", True)):
    U("k_hdr", "plain", _m, 24, 24, SEG4_NOWB, "n_wrap", 64, fill=_f)
    R("k_hdr", _m, ("range", 20, 64), SEG4_NOWB, "n_wrap", 64, base=2, fill=_f)

# ---------------------------------------------------------------------------
# k_seg on uniform batches: dense packets, 65536 and more, of 129..704 bytes or not
# 4-aligned (4 KiB tiles below 448 bytes) or above 3072 bytes. In place the TX kind
# stores each field on its own.
# ---------------------------------------------------------------------------
_BIG = (MID_BATCH, MID_BATCH + 1, MID_BATCH + 63)
_SEG_U = {"k_seg<4>": [(129, 129, 0), (136, 200, 0), (62, 62, 1), (447, 447, 3), (444, 444, 4)],
          "k_seg<8>": [(448, 448, 0), (449, 672, 1), (704, 704, 4), (500, 501, 2), (452, 452, 4), (451, 451, 3)]}
_k = 0
for _kern, _shapes in _SEG_U.items():
    _tx = _kern.replace(">", ",tx>")
    for _sets in (DEFAULT, SEG4_WB):
        for _m in ("raw", "verify_tcp", "verify_udp"):
            for _side in SIDES[_m][:1] if _sets is DEFAULT else SIDES[_m]:
                _ln, _st, _b = _shapes[_k % len(_shapes)]
                U(_kern, "plain", _m, _ln, _st, _sets, _BIG[_k % 3], 64, base=_b, side=_side, n_lo=MID_BATCH,
                  kind=KINDS[_k % 3])
                _k += 1
        for _m in FILL3:
            _ln, _st, _b = _shapes[_k % len(_shapes)]
            U(_tx, "plain", _m, _ln, _st, _sets, _BIG[_k % 3], 64, base=_b, n_lo=MID_BATCH)
            _ln, _st, _b = [s for s in _shapes if s[1] % 4 == 0 and s[2] % 4 == 0][_k % 2]
            U(_tx, "plain", _m, _ln, _st, _sets, _BIG[(_k + 1) % 3], 64, base=_b, fill=True, n_lo=MID_BATCH)
            _k += 1
    _ln, _st, _b = _shapes[0]
    U(_kern, "plain", "raw", _ln, _st, SEG4_WB, "n_wrap", 64, n_lo=MID_BATCH, side="init")
    U(_tx, "plain", "udp", _ln, _st, SEG4_WB, "n_wrap", 64, n_lo=MID_BATCH, side="addrs")
    _ln, _st, _b = [s for s in _shapes if s[1] % 4 == 0 and s[2] % 4 == 0][0]
    U(_tx, "plain", "tcp", _ln, _st, SEG4_WB, "n_wrap", 64, n_lo=MID_BATCH, fill=True, side="addrs")
# above 3072 bytes: a few cases (a batch is 200 MB at 65536 packets: overlapping packets
# keep it small, results only; in place at 3076 bytes it is the directed test's)
U("k_seg<8>", "plain", "raw", 3073, 40, DEFAULT, MID_BATCH + 63, 64, base=1, n_lo=MID_BATCH, side="init")
U("k_seg<8,tx>", "plain", "tcp", 9000, 64, DEFAULT, MID_BATCH + 1, 64, n_lo=MID_BATCH, side="addrs")

# ---------------------------------------------------------------------------
# Whole datagrams (VERIFY_RX, TX_DATAGRAM), uniform slots and ragged: the ragged picks.
# Up to 4096 a wave per datagram, up to 65535 16-datagram chunks, then 64-datagram ones
# (in place: 40); YU_RAGGED=seg4: 4 KiB tiles for VERIFY_RX at every count, 8 KiB ones for
# TX_DATAGRAM. The datagrams come from tests/rxgen.py.
# ---------------------------------------------------------------------------
_DG = [  # kernel, mode, fill, fill_plain, ppw, counts, n_lo, n_hi, trio, uniform too
    ("k_loop<4,rx>", "verify_rx", False, False, 1, (1, 2, 4096), 1, SMALL_BURST, RUNS0, True),
    ("k_loop<4,dg>", "tx_datagram", False, False, 1, (1, 2, 4096), 1, SMALL_BURST, RUNS0, True),
    ("k_loop<4,dg>", "tx_datagram", True, False, 1, (1, 2, 4096), 1, SMALL_BURST, RUNS0, True),
    ("k_seg<8,rx,c16>", "verify_rx", False, False, 16, (4097, 4111, 4112), 4097, MID_BATCH - 1, RUNS2, True),
    ("k_seg<8,dg,c16>", "tx_datagram", False, False, 16, (4097, 4111, 4112), 4097, MID_BATCH - 1, RUNS2, True),
    ("k_seg<8,dg,c16>", "tx_datagram", True, True, 16, (4097, 4111, 4112), 4097, MID_BATCH - 1, RUNS2, True),
    ("k_seg<8,rx>", "verify_rx", False, False, 64, _BIG, MID_BATCH, None, RUNS0, True),
    ("k_seg<8,dg>", "tx_datagram", False, False, 64, _BIG, MID_BATCH, None, RUNS0, True),
    ("k_seg<8,dg>", "tx_datagram", True, True, 64, _BIG, MID_BATCH, None, RUNS0, "only"),
    ("k_seg<8,dg,c40>", "tx_datagram", True, True, 40, _BIG, MID_BATCH, None, RUNS0, False),
    ("k_seg<4,rx>", "verify_rx", False, False, 64, (1, 63, 64, 65, 5000), 1, None, SEG4_WB, True),
    ("k_seg<8,dg>", "tx_datagram", False, False, 64, (1, 63, 64, 65, 5000), 1, None, SEG4_NOWB, True),
    ("k_seg<8,dg>", "tx_datagram", True, True, 64, (1, 63, 64, 65), 1, None, SEG4_NOWB, "only"),
    ("k_seg<8,dg,c40>", "tx_datagram", True, True, 40, (1, 39, 40, 41, 5000), 1, None, SEG4_NOWB, False),
]
for _kern, _m, _f, _fp, _p, _ns, _lo, _hi, _tr, _uni in _DG:
    _auto = _tr[0] < 7  # the default set makes the same pick
    for _j, _n in enumerate(_ns):
        for _sets in ((DEFAULT, _tr) if _auto and _j == len(_ns) - 1 else (_tr,)):
            if _uni != "only":
                # small datagrams (mean under 400 bytes: seg_waves' narrow grid) and large ones
                R(_kern, _m, ("dgram", 0, 180) if _j % 2 == 0 else ("dgram", 300, 1100) if _n < 60000 else
                  ("dgram", 380, 600), _sets, _n, _p, base=_j % 4, fill=_f, fill_plain=_fp, n_lo=_lo, n_hi=_hi)
            if _uni:
                _ln = (20, 28, 64, 576, 1500)[_j] if _n < 60000 else (64, 28, 136)[_j]
                U(_kern, "plain", _m, _ln, (_ln + 7) // 4 * 4, _sets, _n, _p, base=0 if _f else _j % 4, fill=_f,
                  fill_plain=_fp, n_lo=_lo, n_hi=_hi)
    if _uni != "only":
        R(_kern, _m, ("dgram", 0, 100), _tr, "n_wrap", _p, base=0 if _f else 1, fill=_f, fill_plain=_fp, n_lo=_lo,
          n_hi=_hi)
    if _uni:
        U(_kern, "plain", _m, 40, 44, _tr, "n_wrap", _p, fill=_f, fill_plain=_fp, n_lo=_lo, n_hi=_hi)

# ---------------------------------------------------------------------------
# k_seg on ragged batches of the per-packet modes. Read-only: <8,c16> / <8,tx,c16> from
# 4097 packets, <8> / <8,tx> from 65536, <4> / <4,tx> under YU_RAGGED=seg4. In place the
# TX kinds take the whole-line write-back (txw; 48-packet chunks from 65536) unless
# YU_FILL_WB=0, which keeps the TX kind's single field stores.
# ---------------------------------------------------------------------------
_MID = (4097, 4111, 4112, 4113)
_RSEG = [  # kernel, modes, fill, ppw, counts, n_lo, n_hi, trios
    ("k_seg<8,c16>", ("raw", "verify_tcp", "verify_udp"), False, 16, _MID, 4097, MID_BATCH - 1, (RUNS2,)),
    ("k_seg<8,tx,c16>", FILL3, False, 16, _MID, 4097, MID_BATCH - 1, (RUNS0,)),
    ("k_seg<8,txw,c16>", FILL3, True, 16, _MID, 4097, MID_BATCH - 1, (RUNS2,)),
    ("k_seg<8,tx,c16>", FILL3, True, 16, _MID, 4097, MID_BATCH - 1, (RUNS0,)),
    ("k_seg<8>", ("raw", "verify_tcp", "verify_udp"), False, 64, _BIG, MID_BATCH, None, (RUNS0,)),
    ("k_seg<8,tx>", FILL3, False, 64, _BIG, MID_BATCH, None, (RUNS2,)),
    ("k_seg<8,txw,c48>", FILL3, True, 48, _BIG, MID_BATCH, None, (RUNS2,)),
    ("k_seg<8,tx>", FILL3, True, 64, _BIG, MID_BATCH, None, (RUNS0,)),
    ("k_seg<4>", ("raw", "verify_tcp", "verify_udp"), False, 64, (1, 63, 64, 65, 5000), 1, None, (SEG4_NOWB,)),
    ("k_seg<4,tx>", FILL3, False, 64, (1, 63, 64, 65, 5000), 1, None, (SEG4_WB,)),
    ("k_seg<4,txw>", FILL3, True, 64, (1, 63, 64, 65, 5000), 1, None, (SEG4_WB,)),
    ("k_seg<4,tx>", FILL3, True, 64, (1, 63, 64, 65, 5000), 1, None, (SEG4_NOWB,)),
]
_k = 0
for _kern, _ms, _f, _p, _ns, _lo, _hi, _trs in _RSEG:
    _tr = _trs[0]
    # does the default set make this pick too? (no YU_RAGGED; the TX kind in place needs YU_FILL_WB=0)
    _dflt = _tr[0] < 7 and not (_f and "txw" not in _kern)
    for _m in _ms:
        for _j, _n in enumerate(_ns):
            for _sets in ((DEFAULT, _tr) if _dflt and _j == 0 else (_tr,)):
                for _side in (SIDES.get(_m, ("scalar",)) if _j == 0 else (None,)):
                    _big = _n >= 60000
                    _gen = (("range", _RLO[_m], 200), ("jumbo", _RLO[_m], 1500) if not _big else
                            ("range", 380, 640), ("range", max(_RLO[_m], 40), 200))[(_j + _k) % 3]
                    R(_kern, _m, _gen, _sets, _n, _p, base=(_j + _k) % 4, fill=_f, n_lo=_lo, n_hi=_hi, side=_side,
                      kind=KINDS[(_k + _j) % 3] if not _f else "rand")
        _k += 1
    R(_kern, _ms[0], ("range", _RLO[_ms[0]], 120), _tr, "n_wrap", _p, base=1, fill=_f, n_lo=_lo, n_hi=_hi)
    R(_kern, _ms[1], ("range", _RLO[_ms[1]], 120), _tr, "n_wrap", _p, base=2, fill=_f, n_lo=_lo, n_hi=_hi,
      side="addrs" if _ms[1] in SIDES else None)


# ---------------------------------------------------------------------------
# Everything above is the ledger as it was before the call shapes, the zero poles and
# k_iov: N_BASE cases, each with call="plain". An id is a position, and the child seeds
# a case's bytes from it, so cases are only ever appended: first the call shapes and
# poles of the planner's kernels, derived from the base cases (_call_shapes_and_poles,
# called at the end of the module), then the k_iov cases (_iov_cases).
# ---------------------------------------------------------------------------
N_BASE = 1592
assert len(CASES) == N_BASE

# The word a pole_data case solves for: an even packet offset the mode sums that is not
# the checksum field, TCP's byte 12 or IPv4's byte 0.
POLE_W = {"udp": 0, "tcp": 0, "verify_tcp": 0, "verify_udp": 0, "icmp": 4, "ipv4": 4, "verify_ipv4": 4}
TX_POLE = ("udp", "tcp", "icmp", "ipv4")  # these sit at 0x0000, RAW and the VERIFY modes at 0xFFFF
NO_SIDE = ("ipv4", "verify_ipv4", "icmp", "verify_rx", "tx_datagram")  # initial and addrs are ignored
DGRAM = ("verify_rx", "tx_datagram")
POLE_KINDS = ("pole_side", "pole_data")


def calls(case):
    """The call shapes of a case: {"plain"}, or a subset of {"offset", "null_out", "ignored"}."""
    return set(case["call"].split("+"))


def pole(mode):
    return 0x0000 if mode in TX_POLE else 0xFFFF


def ignores(mode, side):
    """What an `ignored` case adds as junk: "both" arrays (and initial = 0xBEEF), "addrs"
    (RAW), "init" (a pseudo mode given addrs, with initial = 0xBEEF); None: nothing to ignore."""
    if mode in NO_SIDE:
        return "both"
    if mode == "raw":
        return "addrs"
    return "init" if side == "addrs" else None


def _template(kernel, form, fill, layout, mode, wrap, need, most):
    """The smallest base case of this key and mode (uniform: with need <= len <= most)."""
    found = [c for c in CASES[:N_BASE] if kernel_of(c) == (kernel, form) and c["fill"] == fill and
             c["layout"] == layout and c["mode"] == mode and (c["n"] == "n_wrap") == wrap and
             (layout == "R" or need <= c["len"] <= most)]
    return min(found, key=lambda c: case_bytes(c, _small_n(c)), default=None)


def _small_n(t):
    """The smallest count at which the template's kernel is still the planner's pick:
    37 for the per-packet kernels, 4097 for the c16 kinds, MID_BATCH + 1 for the 64-, 48-
    and 40-packet chunk kinds; the far-stride k_small cases keep their two packets."""
    if t["layout"] == "U" and t["stride"] == _FAR:
        return t["n"]
    return MID_BATCH + 1 if t["n_lo"] == MID_BATCH else max(t["n_lo"], 37)


def _derive(kernel, form, fill, layout, modes, *, call, kind="rand", sides=("init", "addrs", "scalar"), wrap=False):
    """Appends one case of the key (kernel, form, fill, layout): the first of `modes` x
    `sides` the key's base cases hold, with that base case's geometry (ragged: short
    packets), at the smallest count, under one of the base case's knob sets."""
    for mode in modes:
        side = next((s for s in sides if s in SIDES.get(mode, ("scalar",))), None)
        if side is None:
            continue
        need = max(MIN_LEN.get(mode, 0), POLE_W[mode] + 2 if kind == "pole_data" else 0)
        t = _template(kernel, form, fill, layout, mode, wrap, need, 65535 if kind == "pole_side" else 1 << 32)
        if t is None:
            continue
        sets = sorted(s for s in t["plans"] if s or not wrap)
        s = sets[len(CASES) % len(sets)]
        c = dict(t, call=call, kind=kind, side=side, n="n_wrap" if wrap else _small_n(t), plans={s: t["plans"][s]})
        if layout == "R":
            c["gen"] = (("dgram", 0, 180) if mode in DGRAM else ("range", 0, 200) if mode == "raw" else
                        ("range", max(_RLO[mode], need), 120 if wrap else 200))
        _append(c)
        return True
    return False


def _rot(modes):
    modes = sorted(modes)
    k = len(CASES) % max(len(modes), 1)
    return modes[k:] + modes[:k]


def _call_shapes_and_poles():
    keys = {}  # kernel -> {(form, fill, layout): modes}
    for c in CASES[:N_BASE]:
        keys.setdefault(kernel_of(c)[0], {}).setdefault((kernel_of(c)[1], c["fill"], c["layout"]), set()).add(c["mode"])
    for kernel in sorted(keys):
        ks = keys[kernel]
        # read-only keys first: a kernel that only writes in place (the TXW kinds) is held by those
        order = sorted(ks, key=lambda k: (k[1], k[0], k[2]))
        per_layout = {lay: next(k for k in order if k[2] == lay) for lay in sorted({k[2] for k in order})}
        some = order[0]
        # 1. offset: out and every side array the kernel's modes take, in each layout it takes
        #    (ragged: offsets too), at the least alignment include/yucsum.h allows
        for lay, k in per_layout.items():
            took = [_derive(kernel, *k, _rot(ks[k]), call="offset", sides=(side,)) for side in ("init", "addrs")]
            if not any(took):
                assert _derive(kernel, *k, _rot(ks[k]), call="offset"), (kernel, k)
        # 2. ignored: junk in every argument the mode does not use
        took = [_derive(kernel, *some, _rot(ks[some] & set(NO_SIDE)), call="ignored"),
                _derive(kernel, *some, ["raw"], call="ignored", sides=("init", "scalar")),
                _derive(kernel, *some, _rot(ks[some] - {"raw"}), call="ignored", sides=("addrs",))]
        assert any(took), kernel
        # 3. null_out: every in-place key without a result array, side arrays at the offset
        #    alignments; once per (kernel, form) across a second pass of the grid
        wrapped = set()
        for k in order:
            if not k[1]:
                continue
            assert _derive(kernel, *k, _rot(ks[k]), call="offset+null_out"), (kernel, k)
            if k[0] not in wrapped and _derive(kernel, *k, _rot(ks[k]), call="null_out", wrap=True):
                wrapped.add(k[0])
        # 4. pole_side: initial_arr puts every packet on its pole (TX: 0x0000, RAW / VERIFY: 0xFFFF)
        for modes in ({"udp", "tcp"}, {"raw", "verify_tcp", "verify_udp"}):
            took = [k for k in order if ks[k] & modes]
            assert not took or any(_derive(kernel, *k, _rot(ks[k] & modes), call="plain", kind="pole_side",
                                           sides=("init",)) for k in took), (kernel, modes)
        # 5. pole_data: one word of the packet puts it on its pole (the pseudo modes: with
        #    addrs); the TX and IPv4 modes read-only and in place, then a VERIFY mode
        for fill in (False, True):
            took = [k for k in order if k[1] == fill and ks[k] & set(TX_POLE)]
            assert not took or any(_derive(kernel, *k, _rot(ks[k] & set(TX_POLE)), call="plain", kind="pole_data",
                                           sides=("addrs", "scalar")) for k in took), (kernel, fill)
        for k in order:
            if ks[k] & {"verify_ipv4", "verify_tcp", "verify_udp"} and _derive(
                    kernel, *k, _rot(ks[k] & {"verify_ipv4", "verify_tcp", "verify_udp"}), call="plain",
                    kind="pole_data", sides=("addrs", "scalar")):
                break
        # 6. all-zero and all-0xFF packets in place (ICMP lands on the poles: 0xFFFF and 0x0000)
        for form in sorted({k[0] for k in order if k[1]}):
            k = next(k for k in order if k[1] and k[0] == form)
            if ks[k] <= set(DGRAM):
                continue
            for kind in ("zero", "ff"):
                assert _derive(kernel, *k, ["icmp"] + _rot(ks[k]), call="plain", kind=kind), (kernel, k)


def resolve_n(case, cus, env):
    """The case's packet count on a card with `cus` CUs under the knob set `env`. n_wrap:
    the smallest n above 4 * ppw * CUs * blocks_per_cu + ppw, so that under
    YU_BLOCKS_PER_CU=1 the grid-stride loop makes a second, partial pass, raised to n_lo:
    the case stays on its side of the planner's count cut-overs."""
    if case["n"] != "n_wrap":
        return case["n"]
    bpc = int(env["YU_BLOCKS_PER_CU"])  # n_wrap cases run under the one-block-per-CU sets only
    n = max(4 * case["ppw"] * cus * bpc + case["ppw"] + 1, case["n_lo"])
    assert case["n_hi"] is None or n <= case["n_hi"], (case["id"], n)
    return n


def case_bytes(case, n):
    """An upper bound of the bytes the case moves (the packet buffer)."""
    if case["layout"] == "I":
        return n * (1500 + 64 if case["iov"] == "hdr+pay" else 40 * 32)
    if case["layout"] == "U":
        return case["base"] + (n - 1) * case["stride"] + case["len"]
    name, lo, hi = case["gen"]
    if name == "seam":
        # (CH, T): over the six chunk slots of seg_seams.batch at most 5 * per + 4 tiles, so per + 1/2 a
        # chunk, and the short packets behind the last seam; RAW: four exact chunks of 128 KiB and more
        return case["base"] + (n // lo + 1) * ((2 * seam_per(n, lo) + 1) * hi // 2 + 256) + \
            (8 * 140000 if case["mode"] == "raw" else 0)
    extra = (n // 61 + 1) * (140000 if case["mode"] == "raw" else 9000) if name == "jumbo" else 0
    return int(case["base"] + n * ((lo + hi) / 2 + (60 if name == "dgram" else 0)) + extra)


def query_line(case, n, cus):
    """The case in the left-hand format of plan_table's rows (tests/cpp/plan_query.cpp)."""
    u = case["layout"] == "U"
    return "%s %s %d %d %d %d %d %d" % (case["layout"], case["mode"], case["base"] if u else 0,
                                        case["stride"] if u else 0, case["len"] if u else 0, n, case["fill"], cus)


_call_shapes_and_poles()


# ---------------------------------------------------------------------------
# Layout "I": k_iov<4> / k_iov<4,fill>, the scatter-gather device calls (yu::plan_wave: a
# wave per packet at every count, the policy slot YU_NT's, else 2). A packet is a list of
# (pool, alignment mod 16, length) views, the form of iov_layout.general_layout; the child
# builds the yu_iovec table and first_iov by hand. Under the default set and the RUNS0 trio.
# ---------------------------------------------------------------------------
IOV_KERNELS = ("k_iov<4>", "k_iov<4,fill>")
IOV_SHAPES = ("hdr+pay", "split", "bytes40", "empty")
IOV_MODES = PLAIN6


def iov_packets(case, n):
    """The views of the n packets of an "I" case. hdr+pay: a 20-byte and a 1480-byte view
    in two pools; split: a small datagram cut inside its checksum field (RAW and the
    VERIFY modes: where UDP's lies); bytes40: forty 1-byte views; empty: two views with
    empty ones before, between and after (and, where the mode defines them, packets of
    empty views only)."""
    mode, shape = case["mode"], case["iov"]
    f = FIELD.get(mode, 6)
    need = MIN_LEN.get(mode, 0)
    packets = []
    for i in range(n):
        a, b = (5 * i) % 16, (3 * i + 1) % 16
        if shape == "hdr+pay":
            packets.append([(0, a, 20), (1, b, 1480)])
        elif shape == "split":
            packets.append([(0, a, f + 1), (1, b, max(need, f + 2) + (7 * i) % 64 - f - 1)])
        elif shape == "bytes40":
            packets.append([(j % 2, (a + j) % 16, 1) for j in range(40)])
        elif need == 0 and i % 7 == 3:
            packets.append([(0, 0, 0), (1, 0, 0)])
        else:
            packets.append([(0, 0, 0), (0, a, 21), (1, 0, 0), (1, 0, 0), (1, b, 33 + i % 5), (0, 0, 0)])
    return packets


def I(mode, shape, n, sets, *, fill=False, **kw):
    assert shape in IOV_SHAPES and mode in (FILL3 if fill else IOV_MODES)
    _add("I", IOV_KERNELS[fill], "plain", mode, sets, n, 1, fill=fill, iov=shape, **kw)


def _iov_cases():
    both = DEFAULT + RUNS0
    k = 0
    for shape in IOV_SHAPES:  # counts 1, 2 and 37, every mode in turn
        for n in (1, 2, 37):
            I(IOV_MODES[k % 6], shape, n, both)
            k += 1
        I(FILL3[k // 3 % 3], shape, 37, both, fill=True)
    I("udp", "split", 1, both, fill=True)
    I("tcp", "split", 2, both, fill=True)
    # a second, partial pass of the grid under one block per CU (a wave per packet)
    I("tcp", "hdr+pay", "n_wrap", RUNS0, side="addrs")
    I("raw", "empty", "n_wrap", RUNS0, side="init")
    I("udp", "split", "n_wrap", RUNS0, fill=True, side="addrs")
    I("icmp", "bytes40", "n_wrap", RUNS0, fill=True, call="null_out")
    # the call shapes: the table and first_iov at 8 (mod 16) too
    I("raw", "hdr+pay", 37, both, side="init", call="offset")
    I("verify_tcp", "split", 37, both, side="addrs", call="offset")
    I("udp", "split", 37, both, fill=True, side="addrs", call="offset")
    I("tcp", "hdr+pay", 37, both, fill=True, side="init", call="offset+null_out")
    I("icmp", "empty", 37, both, fill=True, call="offset+null_out")
    I("icmp", "split", 37, both, call="ignored")
    I("raw", "empty", 37, both, side="init", call="ignored")
    I("verify_udp", "hdr+pay", 37, both, side="addrs", call="ignored")
    I("icmp", "bytes40", 37, both, fill=True, call="ignored")
    # the zero poles
    I("udp", "split", 37, both, side="init", kind="pole_side")
    I("tcp", "hdr+pay", 37, both, fill=True, side="init", kind="pole_side")
    I("raw", "empty", 37, both, side="init", kind="pole_side")
    I("verify_tcp", "bytes40", 37, both, side="init", kind="pole_side")
    I("udp", "split", 37, both, side="addrs", kind="pole_data")
    I("icmp", "hdr+pay", 37, both, kind="pole_data")
    I("tcp", "split", 37, both, fill=True, side="addrs", kind="pole_data")
    I("verify_udp", "bytes40", 37, both, side="addrs", kind="pole_data")
    I("icmp", "bytes40", 37, both, fill=True, kind="pole_data")
    I("icmp", "split", 37, both, fill=True, kind="zero")
    I("icmp", "split", 37, both, fill=True, kind="ff")
    I("raw", "empty", 37, both, side="scalar", kind="zero")
    I("udp", "hdr+pay", 37, both, fill=True, side="scalar", kind="ff")


_iov_cases()


# ---------------------------------------------------------------------------
# k_seg's seams (tests/seg_seams.py): every value k_seg produces is a difference of prefix
# sums taken inside tiles of T = 1024 * U bytes that start at the chunk's b0, and the rules
# at a tile's edge (a point at q == T, a field or a header window across two tiles, the
# TXW kinds' whole-line write-back) are reached by the cases above almost only by chance.
# Ragged: gen = ("seam", CH, T), batches that plant every seam class of the kind, at the
# smallest count at which the kind is the pick, at base 0 and at 1 or 3. Uniform: the dense
# sizes at which every chunk ends on a seam, and shapes that put a TX field across one in
# every chunk. Under the default set where it makes the pick, else the first set of the
# key's trio.
# ---------------------------------------------------------------------------
N_BEFORE_SEAMS = len(CASES)
SEAM_MAX_BYTES = 24 << 20


def seg_shape(kernel):
    """(CH, T, kind) of a k_seg instantiation's name: k_seg<U[,tx|txw|rx|dg][,cCH]>."""
    args = kernel[len("k_seg<"):-1].split(",")
    kind = next((a for a in args[1:] if not a.startswith("c")), "plain")
    ch = next((int(a[1:]) for a in args[1:] if a.startswith("c")), 64)
    return ch, 1024 * int(args[0]), kind


def seam_per(n, ch):
    """Seam classes planted per chunk (seg_seams.batch): with some 70 (class, variant)
    plants of 4 each to place, one a chunk where there are a thousand chunks, 3 from 200
    chunks (16 packets hold no more), 6 in the 24 chunks of a 1537-packet case."""
    chunks = n // ch
    return 1 if chunks >= 1000 else 3 if chunks >= 200 else 6


def is_seam(case):
    return case["layout"] == "R" and case["gen"][0] == "seam"


def _seam_cases():
    seen = set()
    k = 0
    rows = [(kern, ms, f, False, p, lo, hi, tr[0]) for kern, ms, f, p, _ns, lo, hi, tr in _RSEG]
    rows += [(kern, (m,), f, fp, p, lo, hi, tr) for kern, m, f, fp, p, _ns, lo, hi, tr, uni in _DG
             if kern.startswith("k_seg") and uni != "only"]
    for kern, ms, f, fp, p, lo, hi, tr in rows:
        if (kern, f) in seen:  # (the 40-packet datagram kind is the pick with and without seg4)
            continue
        seen.add((kern, f))
        ch, t, kind = seg_shape(kern)
        assert ch == p
        seg4 = tr[0] >= 7
        dflt = not seg4 and not (f and kind == "tx")
        n = 1537 if seg4 else MID_BATCH + 1 if lo == MID_BATCH else 4097
        for m in ms:
            # the 24-chunk cases take 3: with base 1 less than half of their chunks would start on a line
            for base in (0, 3 if seg4 else (1, 3)[k % 2]):
                R(kern, m, ("seam", ch, t), DEFAULT if dflt else tr[:1], n, p, base=base, fill=f,
                  fill_plain=fp, n_lo=lo, n_hi=hi)
            k += 1
    # uniform, dense: every chunk ends on a seam and packets inside it start on one
    big = MID_BATCH + 1
    for j, ln in enumerate((192, 256, 384, 512, 640)):
        U("k_seg<4>" if ln < 448 else "k_seg<8>", "plain", ("raw", "verify_tcp", "verify_udp")[j % 3], ln, ln,
          DEFAULT, big, 64, n_lo=MID_BATCH)
    for j, ln in enumerate((256, 512)):
        for f in (False, True):
            U("k_seg<4,tx>" if ln < 448 else "k_seg<8,tx>", "plain", FILL3[(j + f) % 3], ln, ln, DEFAULT, big, 64,
              fill=f, n_lo=MID_BATCH)
    for f in (False, True):
        U("k_seg<8,dg>", "plain", "tx_datagram", 256, 256, DEFAULT, big, 64, fill=f, fill_plain=f, n_lo=MID_BATCH)
    U("k_seg<8,rx>", "plain", "verify_rx", 512, 512, DEFAULT, big, 64, n_lo=MID_BATCH)
    U("k_seg<4,rx>", "plain", "verify_rx", 512, 512, SEG4_WB[:1], 1537, 64)
    # 16-packet chunks: 512-byte slots make a chunk one tile, 1024-byte ones two
    for ln in (512, 1024):
        U("k_seg<8,rx,c16>", "plain", "verify_rx", ln, ln, DEFAULT, 4097, 16, n_lo=4097, n_hi=MID_BATCH - 1)
        for f in (False, True):
            U("k_seg<8,dg,c16>", "plain", "tx_datagram", ln, ln, DEFAULT, 4097, 16, fill=f, fill_plain=f, n_lo=4097,
              n_hi=MID_BATCH - 1)
    # a TX field across a seam in every chunk (read-only; tests/test_kernel_ledger.py confirms the lanes
    # with the model): UDP 141, lane 29: 29 * 141 + 6 = 4095; TCP 327, lane 25: 8175 + 16 = 8191; ICMP 431,
    # lane 19: 8189 + 2 = 8191. In place a uniform field lies at an even position: TCP 272 puts lane 15's
    # at q == 0 of tile 1.
    for m, ln in (("udp", 141), ("tcp", 327), ("icmp", 431)):
        U("k_seg<4,tx>", "plain", m, ln, ln, DEFAULT, big, 64, n_lo=MID_BATCH)
    U("k_seg<4,tx>", "plain", "tcp", 272, 272, DEFAULT, big, 64, fill=True, n_lo=MID_BATCH)
    # 8 KiB tiles: TCP 545, lane 15: 8175 + 16 = 8191 (no UDP or ICMP length of 449..704 bytes does it)
    U("k_seg<8,tx>", "plain", "tcp", 545, 545, DEFAULT, big, 64, n_lo=MID_BATCH)


_seam_cases()
