"""Scatter-gather packets as lists of views over host pools, for the tests of
yu_csum_batch_iov / yu_csum_fill_iov (tests/test_gpu_iov.py, and layout "I" of the
kernel ledger: tests/kernel_cases.py, tests/ledger_child.py). numpy only; torch is
imported where a layout goes to the device."""
import numpy as np

GUARD = 128
FIELD = {1: 6, 2: 16, 4: 2}  # UDP, TCP, ICMP: the checksum field's offset


class Layout:
    """Packets as lists of views over host pools. ``vp``/``vo``/``vl``: pool, offset
    and length of each view; ``first``: n+1 view indices. Offsets count from the
    start of a pool's payload: every pool carries GUARD bytes in front and behind."""

    def __init__(self, pools, vp, vo, vl, first):
        self.pools = [np.ascontiguousarray(p, dtype=np.uint8) for p in pools]
        self.vp, self.vo, self.vl, self.first = (np.asarray(x, dtype=np.int64) for x in (vp, vo, vl, first))
        self.n = len(self.first) - 1
        self._sel = {}
        # where every packet byte lies: (pool, position), in packet order
        vid = np.repeat(np.arange(len(self.vl), dtype=np.int32), self.vl)
        vstart = np.concatenate(([0], np.cumsum(self.vl)))
        self.bpool = self.vp.astype(np.int8)[vid]
        self.bpos = np.arange(vstart[-1]) + (self.vo + GUARD - vstart[:-1])[vid]
        del vid
        self.offsets = vstart[self.first].astype(np.uint64)
        self.lens = np.diff(self.offsets.astype(np.int64))

    def blob(self):
        out = np.zeros(len(self.bpos) + 1, np.uint8)
        for k, p in enumerate(self.pools):
            sel = np.flatnonzero(self.bpool == k)
            out[sel] = p[self.bpos[sel]]
        return out

    def put(self, g, values, pools=None):
        """Stores values[i] at byte g[i] of the packets laid back to back (blob's
        numbering), where that byte lies in the pools (`pools`: copies of them)."""
        g = np.asarray(g, dtype=np.int64)
        values = np.broadcast_to(np.asarray(values, dtype=np.uint8), g.shape)
        for q, p in enumerate(self.pools if pools is None else pools):
            sel = self.bpool[g] == q
            p[self.bpos[g][sel]] = values[sel]

    def at_least(self, min_len):
        """The packets of at least min_len bytes (all of them: the layout itself)."""
        if min_len not in self._sel:
            keep = np.flatnonzero(self.lens >= min_len)
            self._sel[min_len] = self if len(keep) == self.n else self.select(keep)
        return self._sel[min_len]

    def select(self, keep):
        """The same pools and views with only the packets ``keep`` (indices)."""
        keep = np.asarray(keep, dtype=np.int64)
        cnt = (self.first[1:] - self.first[:-1])[keep]
        idx = np.repeat(self.first[:-1][keep] - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt) + np.arange(cnt.sum())
        first = np.concatenate(([0], np.cumsum(cnt)))
        return Layout(self.pools, self.vp[idx], self.vo[idx], self.vl[idx], first)

    def device(self, dev):
        import torch
        pools = [torch.from_numpy(p).to(dev) for p in self.pools]
        views = [t[GUARD:t.numel() - GUARD] for t in pools]
        ix = [torch.from_numpy(x).to(dev) for x in (self.vp, self.vo, self.vl, self.first)]
        return pools, views, ix

    def filled(self, mode, values):
        """The pools after an in-place call that computed ``values``."""
        want = [p.copy() for p in self.pools]
        f = FIELD[mode]
        pk = np.flatnonzero(self.lens >= f + 2)
        for k, byte in ((0, values[pk] >> 8), (1, values[pk] & 0xFF)):
            self.put(self.offsets[pk].astype(np.int64) + f + k, byte.astype(np.uint8), want)
        return want


def two_view_layout(lens, cuts, a1, a2, rng):
    """Packet i: lens[i] bytes split after cuts[i]; the first view at an address
    congruent to a1[i] mod 16 in pool 0, the second at a2[i] mod 4 in pool 1."""
    lens, cuts, a1, a2 = (np.asarray(x, dtype=np.int64) for x in (lens, cuts, a1, a2))
    l1, l2 = cuts, lens - cuts
    pitch1 = (l1 + a1 + 31) // 16 * 16
    pitch2 = (l2 + a2 + 19) // 16 * 16
    o1 = np.concatenate(([0], np.cumsum(pitch1)[:-1])) + a1
    o2 = np.concatenate(([0], np.cumsum(pitch2)[:-1])) + a2
    pools = [rng.integers(0, 256, int(pitch1.sum()) + 2 * GUARD, dtype=np.uint8),
             rng.integers(0, 256, int(pitch2.sum()) + 2 * GUARD, dtype=np.uint8)]
    n = len(lens)
    vp = np.tile([0, 1], n)
    vo = np.stack((o1, o2), 1).reshape(-1)
    vl = np.stack((l1, l2), 1).reshape(-1)
    lay = Layout(pools, vp, vo, vl, 2 * np.arange(n + 1))
    set_tcp_offset(lay)
    return lay


def set_tcp_offset(lay):
    pk = np.flatnonzero(lay.lens >= 13)
    lay.put(lay.offsets[pk].astype(np.int64) + 12, 0x50)


def general_layout(packets, rng, npools=2, fillbyte=None, null_empty=False):
    """packets: a list of lists of (pool, alignment mod 16, length). Views are laid
    out in the order given; an empty view gets a wild offset (never read)."""
    cursor = [0] * npools
    vp, vo, vl, first = [], [], [], [0]
    for pk in packets:
        for pool, al, ln in pk:
            pos = (cursor[pool] + 15) // 16 * 16 + al
            cursor[pool] = pos + ln + 5
            vp.append(pool)
            vo.append(pos if ln else 0)
            vl.append(ln)
        first.append(len(vp))
    pools = []
    for c in cursor:
        p = rng.integers(0, 256, c + 16 + 2 * GUARD, dtype=np.uint8)
        if fillbyte is not None:
            p[GUARD:len(p) - GUARD] = fillbyte
        pools.append(p)
    lay = Layout(pools, vp, vo, vl, first)
    if fillbyte is None:
        set_tcp_offset(lay)
    return lay
