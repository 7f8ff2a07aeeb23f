"""The kernel ledger: for every function the planner (yustack_amd/csrc/yucsum_plan.h)
can name, the batches that are compared with the C oracle on the GPU, and the plan
each one is expected to get, as written text "kernel form policy".

tests/test_kernel_ledger.py (CPU) checks the written plans against the planner and
that the cases cover every reachable key (kernel, form, policy, in place, layout);
tests/ledger_child.py runs the cases of one knob set on the GPU;
tests/test_gpu_kernel_ledger.py starts one child per knob set.

A case is a dict:
  id        its position in CASES and a short description
  layout    "U" (uniform: stride, len, base = the first packet's offset in a 128-byte
            aligned buffer) or "R" (ragged: gen = (name, lo, hi), base)
  mode, fill, side ("scalar" | "init" | "addrs"), kind ("rand" | "zero" | "ff")
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


def _add(layout, kernel, form, mode, sets, n, ppw, *, fill=False, fill_plain=False, side=None, kind="rand",
         n_lo=1, n_hi=None, **geom):
    if side is None:  # rotate through what the mode takes
        allowed = SIDES.get(mode, ("scalar",))
        side = allowed[len(CASES) % len(allowed)]
    assert side in SIDES.get(mode, ("scalar",)), (mode, side)
    c = dict(layout=layout, mode=mode, fill=fill, side=side, kind=kind, n=n, n_lo=n_lo, n_hi=n_hi, ppw=ppw,
             plans={s: f"{kernel} {form} {_policy(s, fill, fill_plain)}" for s in sets}, **geom)
    g = f"{geom['len']}/{geom['stride']}@{geom['base']}" if layout == "U" else "%s[%d..%d]@%d" % (*geom["gen"], geom["base"])
    c["id"] = f"{len(CASES):04d} {kernel} {form} {layout} {mode}{' fill' if fill else ''} {g} n={n} {side} {kind}"
    CASES.append(c)


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
    if case["layout"] == "U":
        return case["base"] + (n - 1) * case["stride"] + case["len"]
    name, lo, hi = case["gen"]
    extra = (n // 61 + 1) * (140000 if case["mode"] == "raw" else 9000) if name == "jumbo" else 0
    return int(case["base"] + n * ((lo + hi) / 2 + (60 if name == "dgram" else 0)) + extra)


def query_line(case, n, cus):
    """The case in the left-hand format of plan_table's rows (tests/cpp/plan_query.cpp)."""
    u = case["layout"] == "U"
    return "%s %s %d %d %d %d %d %d" % (case["layout"], case["mode"], case["base"] if u else 0,
                                        case["stride"] if u else 0, case["len"] if u else 0, n, case["fill"], cus)
