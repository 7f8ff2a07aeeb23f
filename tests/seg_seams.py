"""k_seg's seams: a model of how the kernel tiles a chunk, a count of the packets and
chunks of a batch that sit on a seam rule, and a generator of ragged batches that puts
every rule's case there on purpose (test data, numpy only, no GPU). The ledger's
("seam", CH, T) cases are made here (tests/kernel_cases.py, tests/ledger_child.py build).

The model restates seg_geom / seg_fetch of yustack_amd/csrc/yucsum_kernels.hip: it is the
kernel's test-side twin, and a change of the tile origin in the kernel must change
geometry() too (the ledger's CPU tests then show which classes the cases still hold).

  A chunk is the packets [c*CH, c*CH + CH). With a the address of its first packet,
  b0 = floor4(a); the in-place TXW kinds (line128) take b0 = floor128(a) unless that lies
  before floor4(data). Tile t covers [b0 + t*T, b0 + (t+1)*T), T = 1024 * U. Every position
  is relative to b0: a packet's x (start) and y (end), the chunk's x0 (its first byte) and
  xe (its end). A seam is k*T with k >= 1. Addresses are relative to a 128-byte line, which
  the ledger's child asserts of the `data` pointer it passes.

Classes (features). d is the offset from a seam. Counts are split by the parity of the
packet's start address, which decides the byte weights in le_to_be and fsum; b0, T, the
field offsets (6, 16, 2) and every header length are even, so a class that fixes a point of
the packet at seam + d has one parity only, d's (wanted() below).
  start@d          an interior packet (not its chunk's first) starts at seam + d
  chunk_end@d      xe = seam + d (parity: of the chunk's last packet); chunk_end:one_tile
                   xe == T, chunk_end:multi xe == k*T >= 2T, chunk_end:nopark the same with
                   the last packet starting 64 bytes or more before the last tile: no start,
                   field or header window lies in it and the chunk's end is a carry
  empty@0          a zero-length interior packet on a seam; empty@end: one on the chunk's end
  field@d          TX kinds: the checksum field's first byte at seam + d (-1: the straddle)
  exact            plain kind, RAW: a chunk with a packet of 131073 bytes or more and, after
                   it, start@0, start@-1 and chunk_end@0 (counted per chunk)
  l4field@d        DG kinds: an in-contract datagram's transport field (byte hl + fo) at
                   seam + d; l4field:ihl5 / l4field:ihl>5 by header length;
                   l4field:same_seam: header and field around one seam (a 20-byte header
                   ending on it, so its 24-byte window is parsed in the second tile and the
                   field is read there at q = 2, 6 or 16). A header across one seam with the
                   field at the next cannot exist: hl + fo <= 76 < T.
  hdr_end@0:ihl5 / hdr_end@0:ihl>5    RX, DG kinds: the header ends on a seam
  tl_end@d         RX, DG kinds: TotalLength() ends at seam + d; tl_end:tl<len with trailing
                   bytes after it, tl_end:tl==len without
  short_hdr        RX kinds: a datagram with IHL 0..4 (rxgen.short_header_packet) whose
                   24-byte header window lies across a seam
  wb_*             TXW kinds in place, positions wq relative to the chunk's last tile:
                   wb_last_line_cut (the field's 128-byte line reaches past xe),
                   wb_first_line_cut (it begins before x0), wb_line_straddle (wq = 127 mod 128),
                   wb_prev@-1 / wb_prev@-2 (the field begins on the last byte / the last two
                   bytes of the tile before), wb_one_tile (a chunk of one tile, per chunk),
                   wb_shared_line (a chunk boundary in mid-line with a field of each chunk
                   in that line, per boundary)
"""
import collections
import types

import numpy as np

import kernel_cases as K
import rxgen

EXACT_LEN = 131073  # the first RAW length on the exact uint32 path (kLEMax + 1)
RESIDUES = (1, 2, 3, 4, 60, 127)  # chunk starts (mod 128) beside the 128-byte line
L4 = {17: (6, 8), 6: (16, 20), 1: (2, 4)}  # protocol: (field offset, least segment)


def lo_of(mode):
    return K._RLO.get(mode, 0)


def geometry(starts, ends, CH, T, line128, data=0):
    """Per packet x, y and per chunk xe, x0 (and b0, the chunk's last packet `last`, its
    tile count) of a batch at the addresses `starts` / `ends`, all relative to a 128-byte
    line; `data` is the batch pointer's address (the line128 origin never lies before
    floor4(data)). Uniform batches: a chunk ends where its last packet ends."""
    starts, ends = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    n = starts.size
    first = starts[::CH]
    b0 = first & ~3
    if line128:
        b128 = first & ~127
        b0 = np.where(b128 >= (data & ~3), b128, b0)
    last = np.minimum(np.arange(first.size) * CH + CH, n) - 1
    xe = ends[last] - b0
    b0p = np.repeat(b0, CH)[:n]
    return types.SimpleNamespace(x=starts - b0p, y=ends - b0p, xe=xe, x0=first - b0, b0=b0, last=last,
                                 tiles=-(-xe // T), chunk=np.arange(n) // CH, lane=np.arange(n) % CH)


def _parse(buf, starts, length):
    """(in contract, hl, tl, protocol, has a transport field, fo) per packet, from the bytes."""
    n = starts.size
    hl, tl, proto = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    i = np.nonzero(length >= 20)[0]
    a = starts[i]
    hl[i] = (buf[a].astype(np.int64) & 15) * 4
    tl[i] = (buf[a + 2].astype(np.int64) << 8) | buf[a + 3]
    proto[i] = buf[a + 9]
    ok = (length >= 20) & (hl >= 20) & (hl <= tl) & (tl <= length)
    fo = np.select([proto == 17, proto == 6, proto == 1], [6, 16, 2], 0)
    mn = np.select([proto == 17, proto == 6, proto == 1], [8, 20, 4], 0)
    return ok, hl, tl, proto, ok & (fo > 0) & (tl - hl >= mn), fo


def features(starts, ends, CH, T, line128, mode, buf=None, data=0):
    """Counter {(class, start parity): packets or chunks of the batch that sit there}.
    `buf`: the bytes `starts` index (the datagram modes' classes are decided from them;
    without it they are left out)."""
    g = geometry(starts, ends, CH, T, line128, data)
    starts, ends = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    length, par = ends - starts, starts & 1
    C = collections.Counter()

    def add(name, mask, p=par):
        for q in (0, 1):
            k = int(np.count_nonzero(mask & (p == q)))
            if k:
                C[(name, q)] += k

    def at(pos, d):
        return (pos - d >= T) & ((pos - d) % T == 0)

    interior = g.lane > 0
    xe_p = g.xe[g.chunk]
    for d in (-2, -1, 0, 1, 2):
        add(f"start@{d}", interior & at(g.x, d))
    lp, lx = par[g.last], g.x[g.last]
    for d in (-1, 0, 1):
        add(f"chunk_end@{d}", at(g.xe, d), lp)
    add("chunk_end:one_tile", g.xe == T, lp)
    add("chunk_end:multi", at(g.xe, 0) & (g.xe >= 2 * T), lp)
    add("chunk_end:nopark", at(g.xe, 0) & (g.xe >= 2 * T) & (lx + 64 <= g.xe - T), lp)
    add("empty@0", interior & (length == 0) & at(g.x, 0))
    add("empty@end", (length == 0) & (g.x == xe_p) & (xe_p > 0))
    fld = K.FIELD.get(mode) if mode in K.FILL3 else None
    if fld is not None:
        has = length >= fld + 2
        for d in (-2, -1, 0):
            add(f"field@{d}", has & at(g.x + fld, d))
    if mode == "raw":
        for c in np.unique(g.chunk[length >= EXACT_LEN]):
            i = np.nonzero(g.chunk == c)[0]
            after = i[i > i[length[i] >= EXACT_LEN][0]]
            if at(g.x[after], 0).any() and at(g.x[after], -1).any() and at(g.xe[c:c + 1], 0)[0]:
                C[("exact", int(par[i[0]]))] += 1
    if mode in K.DGRAM and buf is not None:
        ok, hl, tl, proto, l4, fo = _parse(buf, starts, length)
        any_d = np.zeros(starts.size, bool)
        for d in (-2, -1, 0):
            m = l4 & at(g.x + hl + fo, d)
            add(f"l4field@{d}", m)
            any_d |= m
        add("l4field:ihl5", any_d & (hl == 20))
        add("l4field:ihl>5", any_d & (hl > 20))
        add("l4field:same_seam", l4 & (hl == 20) & at(g.x + 20, 0))
        add("hdr_end@0:ihl5", ok & (hl == 20) & at(g.x + hl, 0))
        add("hdr_end@0:ihl>5", ok & (hl > 20) & at(g.x + hl, 0))
        any_d = np.zeros(starts.size, bool)
        for d in (-1, 0, 1):
            m = ok & at(g.x + tl, d)
            add(f"tl_end@{d}", m)
            any_d |= m
        add("tl_end:tl<len", any_d & (tl < length))
        add("tl_end:tl==len", any_d & (tl == length))
        w = g.x & ~3
        ihl = np.zeros(starts.size, np.int64)
        ihl[length >= 20] = buf[starts[length >= 20]] & 15
        add("short_hdr", (length >= 20) & (ihl < 5) & (w // T != (w + 23) // T))
    if line128 and fld is not None:
        tb = (np.maximum(g.tiles, 1) - 1) * T
        wq = g.x + fld - tb[g.chunk]
        ins = has & (wq >= 0) & (wq <= T - 2)
        ls = tb[g.chunk] + (wq & ~127)
        add("wb_last_line_cut", ins & (ls + 128 > xe_p))
        add("wb_first_line_cut", ins & (ls < g.x0[g.chunk]))
        add("wb_line_straddle", ins & (wq % 128 == 127))
        add("wb_prev@-1", has & (wq == -1))
        add("wb_prev@-2", has & (wq == -2))
        first = np.arange(g.xe.size) * CH
        held = np.zeros(g.xe.size, bool)
        held[np.unique(g.chunk[has])] = True
        add("wb_one_tile", (g.xe > 0) & (g.xe <= T) & held, par[first])
        # a boundary in mid-line: the last packet of a chunk and the first of the next,
        # both with their field inside that one line
        a, b = g.last[:-1], first[1:]
        edge = ends[a]
        line = edge & ~127
        add("wb_shared_line", (edge % 128 != 0) & has[a] & (starts[a] + fld >= line) & has[b] &
            (starts[b] == edge) & (starts[b] + fld + 2 <= line + 128), par[b])
    return C


# ---------------------------------------------------------------------------
# What a kind's cases must hold
# ---------------------------------------------------------------------------
def classes_for(kind, mode, line128=False):
    """The classes of a k_seg kind ("plain", "tx", "txw", "rx", "dg") in `mode`."""
    cl = [f"start@{d}" for d in (-2, -1, 0, 1, 2)] + [f"chunk_end@{d}" for d in (-1, 0, 1)]
    cl += ["chunk_end:one_tile", "chunk_end:multi", "chunk_end:nopark"]
    if lo_of(mode) == 0:
        cl += ["empty@0", "empty@end"]
    if kind in ("tx", "txw"):
        cl += [f"field@{d}" for d in (-2, -1, 0)]
    if kind == "plain" and mode == "raw":
        cl += ["exact"]
    if kind == "dg":
        cl += [f"l4field@{d}" for d in (-2, -1, 0)] + ["l4field:ihl5", "l4field:ihl>5", "l4field:same_seam"]
    if kind in ("rx", "dg"):
        cl += ["hdr_end@0:ihl5", "hdr_end@0:ihl>5"] + [f"tl_end@{d}" for d in (-1, 0, 1)]
        cl += ["tl_end:tl<len", "tl_end:tl==len"]
    if kind == "rx":
        cl += ["short_hdr"]
    if line128:
        cl += ["wb_last_line_cut", "wb_first_line_cut", "wb_line_straddle", "wb_prev@-1", "wb_prev@-2",
               "wb_one_tile", "wb_shared_line"]
    return cl


ONCE = ("chunk_end:one_tile", "chunk_end:multi", "chunk_end:nopark", "wb_shared_line", "exact")


def wanted(cl):
    """[(parity or None: both together, least count)] of a class. A class that pins a point
    of the packet at seam + d has d's parity; tl_end@d leaves the start free: both
    parities; a chunk's end is one per chunk (a 1537-packet case has 24 full chunks, of
    which half start on a line): 4 in all and each parity of the last packet once; the
    variants the issue asks for "once", and exact (at most 8 chunks a case), once."""
    if cl in ONCE:
        return [(None, 1)]
    head, _, d = cl.partition("@")
    if head in ("start", "field", "l4field"):
        return [(int(d) & 1, 4)]
    if head == "tl_end":
        return [(0, 4), (1, 4)]
    if head == "chunk_end":
        return [(None, 4), (0, 1), (1, 1)]
    if cl in ("empty@0", "l4field:same_seam") or head == "hdr_end":
        return [(0, 4)]
    if cl == "wb_line_straddle":
        return [(1, 4)]
    return [(None, 4)]


def missing(counts, classes):
    """The classes (with the parity) a batch holds too few of: ["start@-2 parity 0: 0 < 4", ...]."""
    out = []
    for cl in classes:
        for p, least in wanted(cl):
            got = counts[(cl, p)] if p is not None else counts[(cl, 0)] + counts[(cl, 1)]
            if got < least:
                out.append(f"{cl}{'' if p is None else ' parity %d' % p}: {got} < {least}")
    return out


# ---------------------------------------------------------------------------
# The generator
# ---------------------------------------------------------------------------
class _Chunk:
    """One chunk under construction: `cur` is the next packet's start relative to b0."""

    def __init__(self, a, T, line128, gap):
        self.b0 = a & ~127 if line128 else a & ~3
        self.cur = self.x0 = a - self.b0
        self.T, self.gap = T, gap
        self.pk = []  # (length, bytes | None: a filler, class planted there | None)

    def add(self, length, body=None, cl=None):
        assert 0 <= length <= 65535 or cl == "exact"
        self.pk.append((length, body, cl))
        self.cur += length

    def seam(self, before=0):
        """The first seam k*T, k >= 1, with room for one filler in front of k*T - before."""
        return max(1, -(-(self.cur + self.gap + before) // self.T)) * self.T

    def goto(self, x):
        """One filler: the next packet starts at x."""
        assert x - self.cur >= self.gap, (x, self.cur)
        self.add(x - self.cur)


def batch(CH, T, mode, line128, base, classes, n, rng, per=None):
    """A ragged batch of n packets of `mode` whose first starts at `base` (mod 128), for a
    kind that tiles chunks of CH packets in tiles of T bytes from floor128 (line128) or
    floor4 of the chunk's start. Returns lens (int64), parts (the datagram modes: a list
    of uint8 arrays, else None), planted ([(packet index, class)] of the packets built for
    a class, datagram modes) and the chunk starts' residues (mod 128).

    Every full chunk c has a slot c % 6 that sets its end, and with it where the next
    chunk starts (the previous chunk's last filler sets the alignment):
      0  xe = seam + 1            -> the next chunk starts at 1 (mod 128)
      1  xe == T, a one-tile chunk (x0 = 1)                       -> on a line
      2  xe = seam - 1            -> 127 (mod 128)
      3  a free end at r (mod 128), r through {2, 3, 4, 60} less `base`, then four times 0
      4  a free end on a line (the modes that take them: one to three empty packets there)
      5  xe = seam: >= 2T with a boundary in the last tile, >= 2T with one packet filling
         the last tile (nopark), the next seam, in turn           -> on a line
    so slots 0, 2 and 5 start on a line, slot 4 too after an r of 0: at least half (a seam
    lies on a line only where the chunk starts within 3 bytes of one, so a slot whose end
    is a seam follows a start on a line or at 1 or 127). Slots 3 and 4 plant `per` seam
    classes of `classes`, in rotation, at successive seams, slots 0, 2 and 5 per - 1, slot
    1 none. line128: slots 3 and 4 then plant wb_prev@-1 / -2 in turn at the next seam,
    wb_line_straddle behind it, and end with a field in the last line; slot 2's last
    packet has its field in the cut last line; slot 1's first has it in the cut first
    line. RAW: three of the first four slot-5 chunks are the exact ones. The packets a
    chunk has left over come first, as short fillers of the mode's least length."""
    lo = lo_of(mode)
    dgram = mode in K.DGRAM
    fld = K.FIELD.get(mode) if mode in K.FILL3 else None
    small = 20 if dgram else max(lo, 2 if fld is None else fld + 2)  # a short packet (with its field)
    per = K.seam_per(n, CH) if per is None else per
    gap = max(lo, 1)
    res = [r for r in (2, 3, 4, 60) if r != base] + [0, 0, 0, 0]
    insts = []
    for cl in classes:
        head, _, d = cl.partition("@")
        if head in ("start", "field", "l4field"):
            insts.append((head, int(d)))
        elif head == "tl_end":  # both start parities
            insts += [(head, int(d), 0), (head, int(d), 1)]
        elif cl == "empty@0":
            insts.append(("empty",))
        elif cl in ("hdr_end@0:ihl5", "hdr_end@0:ihl>5", "short_hdr"):
            insts.append((cl,))
    state = dict(q=0, wb=0)
    pads = ([np.frombuffer(bytes(_contract(mode, rxgen.filler_packet(rng, ln))), np.uint8)
             for ln in (20, 21, 22, 23, 24, 26, 28, 33, 7, 0)] if dgram else None)
    seed = int(rng.integers(0, 2 ** 62))

    def dg(crng, ihl, proto, plen, trail=0):
        plen = max(plen, L4.get(proto, (0, 0))[1])
        p = (rxgen.make_packet if mode == "verify_rx" else rxgen.tx_packet)(crng, plen, proto=proto, ihl=ihl)
        p += crng.integers(0, 256, size=trail, dtype=np.uint8).tobytes()
        return bytes(p)

    def body(ch, crng):
        """A short packet of the mode's own: what starts at a planted boundary."""
        if dgram:
            b = dg(crng, 5, int(crng.choice([6, 17, 1, 47])), int(crng.integers(0, 40)))
            ch.add(len(b), b)
        else:
            ch.add(small + int(crng.integers(0, 9)))

    def plant(ch, crng):
        inst = insts[state["q"] % len(insts)]
        k = state["q"] // len(insts)  # how often the rotation has come round: the variants' turn
        state["q"] += 1
        head = inst[0]
        if head == "start":
            ch.goto(ch.seam(-inst[1]) + inst[1])
            body(ch, crng)
        elif head == "empty":
            ch.goto(ch.seam())
            for _ in range(1 + k % 3):
                ch.add(0, b"")
            body(ch, crng)
        elif head == "field":
            ch.goto(ch.seam(fld - inst[1]) + inst[1] - fld)
            ch.add(small + int(crng.integers(0, 9)))
        elif head == "l4field":
            proto = (17, 6, 1)[k % 3]
            ihl = 5 if (k + inst[1]) % 2 == 0 else int(crng.integers(6, 16))
            off = 4 * ihl + L4[proto][0] - inst[1]
            ch.goto(ch.seam(off) - off)
            b = dg(crng, ihl, proto, int(crng.integers(0, 64)))
            ch.add(len(b), b, f"l4field@{inst[1]}")
        elif head.startswith("hdr_end"):
            ihl = 5 if head.endswith("ihl5") else int(crng.integers(6, 16))
            ch.goto(ch.seam(4 * ihl) - 4 * ihl)
            b = dg(crng, ihl, (17, 6, 1)[k % 3], int(crng.integers(0, 64)))
            ch.add(len(b), b, "l4field:same_seam" if ihl == 5 and mode == "tx_datagram" else head)
        elif head == "tl_end":
            d, want = inst[1], inst[2]  # the start's parity
            ihl = int(crng.integers(5, 9))
            plen = 24 + 2 * int(crng.integers(0, 30)) + ((d - want) & 1)
            tl = 4 * ihl + plen
            ch.goto(ch.seam(tl - d) + d - tl)
            b = dg(crng, ihl, (17, 6, 1, 47)[k % 4], plen, trail=int(crng.integers(1, 41)) if k & 1 else 0)
            ch.add(len(b), b, f"tl_end@{d}")
        elif head == "short_hdr":
            dd, s = 4 * int(crng.integers(1, 6)), int(crng.integers(0, 4))
            ch.goto(ch.seam(dd) - dd + s)
            total = int(crng.integers(20, 81))
            ch.add(total, bytes(rxgen.short_header_packet(crng, total)), "short_hdr")

    def last_packet(ch, e, want):
        """Fillers up to the chunk end e: the last one starts at the parity `want`."""
        ch.add(small + ((ch.cur + small - want) & 1))
        ch.goto(e)

    def finish(ch, slot, period):
        T_, want = T, period & 1  # the parity the chunk's last packet starts at
        if slot in (0, 2):
            d = 1 if slot == 0 else -1
            if line128 and slot == 2:  # the last packet's field in the last line, which xe cuts
                e = ch.seam(small + 1 - d) + d
                m = small + ((e - small - want) & 1)
                ch.goto(e - m)
                ch.add(m)
            else:
                e = max(1, -(-(ch.cur + small + 1 + gap - d) // T_)) * T_ + d
                last_packet(ch, e, want)
        elif slot == 1:
            last_packet(ch, T_, want)
        elif slot == 5:
            how = period % 3
            ch.add(small + ((ch.cur + small - want) & 1))
            if how == 0:  # >= 2T, a boundary in the last tile
                e = max(2, -(-(ch.cur + gap + small + 2) // T_)) * T_
                m = small + ((e - small - want) & 1)
                ch.goto(e - m)
                ch.add(m)
            elif how == 1:  # one packet fills the last tile
                ch.goto(-(-(ch.cur + T_ + 64) // T_) * T_)
            else:
                ch.goto(ch.seam())
        else:  # a free end at r (mod 128)
            r = res[period % len(res)] if slot == 3 else 0
            if line128:
                e = ch.cur + gap + small
                e += (r - (ch.b0 + e)) % 128
                ch.goto(e - small)
                ch.add(small)
            else:
                e = ch.cur + small + 1 + gap
                e += (r - (ch.b0 + e)) % 128
                last_packet(ch, e, want)
            if slot == 4 and lo == 0:
                for _ in range(1 + period % 3):
                    ch.add(0, b"")

    def make(c, a, npad):
        crng = np.random.default_rng([seed, c])
        ch = _Chunk(a, T, line128, gap)
        slot, period = c % 6, c // 6
        for i in range(npad):
            if dgram:
                p = pads[(i + c) % len(pads)]
                ch.add(p.size, p)
            else:
                ch.add(lo + (i * 5 + c) % 3)
        if mode == "raw" and "exact" in classes and slot == 5 and period < 4 and period % 3 != 1:
            ch.add(EXACT_LEN + c % 7, None, "exact")
            ch.goto(ch.seam())
            body(ch, crng)
            ch.goto(ch.seam(1) - 1)
            body(ch, crng)
            ch.goto(ch.seam())
            return ch
        for _ in range(0 if slot == 1 or not insts else per if slot in (3, 4) else per - 1):
            plant(ch, crng)
        if line128 and slot in (3, 4):
            d = -1 - state["wb"] % 2
            state["wb"] += 1
            if f"wb_prev@{d}" in classes:
                ch.goto(ch.seam(fld - d) + d - fld)
                ch.add(small)
            if "wb_line_straddle" in classes:
                x = ch.cur + gap
                x += (127 - (x + fld)) % 128
                ch.goto(x)
                ch.add(small)
        finish(ch, slot, period)
        return ch

    lens, parts, planted, starts = [], [], [], []
    a = base
    for c in range(n // CH):
        keep = dict(state)
        used = len(make(c, a, 0).pk)
        assert used <= CH, (c, used, CH)
        state.update(keep)
        ch = make(c, a, CH - used)
        assert len(ch.pk) == CH, (c, len(ch.pk))
        starts.append(a % 128)
        for ln, b, cl in ch.pk:
            if cl is not None and cl != "exact":
                planted.append((len(lens), cl))
            lens.append(ln)
            if dgram:
                parts.append(np.frombuffer(b, np.uint8) if isinstance(b, (bytes, bytearray)) else b if b is not None
                             else np.frombuffer(bytes(_contract(mode, rxgen.filler_packet(rng, ln))), np.uint8))
        a += ch.cur - ch.x0
    if n % CH:
        starts.append(a % 128)
    for i in range(n % CH):  # the last, partial chunk: short fillers
        lens.append(pads[i % len(pads)].size if dgram else lo + i % 3)
        if dgram:
            parts.append(pads[i % len(pads)])
    lens = np.array(lens, np.int64)
    assert lens.size == n and (not dgram or all(p.size == ln for p, ln in zip(parts, lens)))
    return types.SimpleNamespace(lens=lens, parts=parts if dgram else None, planted=planted,
                                 residues=np.array(starts, np.int64))


def _contract(mode, pkt):
    """A filler of TX_DATAGRAM stays inside YU_MODE_TCP's contract (rxgen.tcp_contract)."""
    return rxgen.tcp_contract(pkt) if mode == "tx_datagram" else pkt
