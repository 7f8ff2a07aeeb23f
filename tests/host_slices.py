"""A model of the host path's geometry, written from the comments of
yustack_amd/csrc/yucsum_hostgeom.h and include/yucsum.h (not from its code): where a
host batch is cut into slices, whether it goes direct, how a _multi call is cut into
shards, how much staging the call leaves behind, and which seam classes a batch plants.

A cut is a list of (first, count, bytes). tests/test_host_geom.py compares it with the
header's own cut (tests/cpp/host_geom.cpp); tests/host_cases.py builds its plans with it,
and tests/host_child.py predicts yu_host_staging_bytes from it."""
import numpy as np

SLICE_BYTES, SLICE_PACKETS, DIRECT_MAX = 32 << 20, 1 << 18, 4 << 20


def limit(value, compiled):
    """A slice-limit knob: a number in [1, compiled], or the compiled constant."""
    try:
        v = int(value)
    except (TypeError, ValueError):
        return compiled
    return v if 1 <= v <= compiled else compiled


def cut_lens(lens, lim_b, lim_p):
    """Ragged and view batches: whole packets in order, at most lim_p of them and, beyond
    the first, only while the slice stays within lim_b bytes."""
    lens = np.asarray(lens, np.int64)
    n = lens.size
    c = np.zeros(n + 1, np.int64)
    c[1:] = np.cumsum(lens)
    out, first = [], 0
    while first < n:
        # the last boundary whose bytes from `first` fit (empty packets that follow fit too)
        e = int(np.searchsorted(c, c[first] + lim_b, side="right")) - 1
        e = max(min(e, first + lim_p, n), first + 1)
        out.append((first, e - first, int(c[e] - c[first])))
        first = e
    return out


def cut_uniform(stride, length, n, lim_b, lim_p):
    """Uniform batches: the same count in every slice but the last, a span that leaves
    out the gap after the slice's last packet."""
    per = min(n, lim_p, max(1, lim_b // max(stride, 1)))
    return [(f, min(per, n - f), (min(per, n - f) - 1) * stride + length) for f in range(0, n, per)]


def largest(cut):
    return max(s[2] for s in cut), max(s[1] for s in cut)


def is_burst(cut, direct_max):
    """One slice of at most direct_max bytes: the kernel reads it in place."""
    return len(cut) == 1 and cut[0][2] <= direct_max


def staging(max_b, max_pk, burst):
    """(pinned, device) bytes a context holds after serving a call whose largest slice is
    (max_b, max_pk): include/yucsum.h's YU_HOST_*CONTEXT_*_MAX with the slice's own size."""
    slots = 1 if burst else 3
    return slots * (max(max_b, 16) + 26 * max_pk + 72), slots * (max(max_b, 16) + 22 * max_pk + 8)


def even_bounds(n, ndev):
    return [n * i // ndev for i in range(ndev + 1)]


def byte_bounds(offsets, ndev):
    """Ragged shards: the first packet boundary at or above an even split of the bytes,
    never below the previous bound."""
    off = [int(x) for x in offsets]
    n = len(off) - 1
    b = [0]
    for i in range(1, ndev):
        target = off[0] + (off[n] - off[0]) * i // ndev
        k = next((j for j in range(n + 1) if off[j] >= target), n)
        b.append(max(k, b[-1]))
    return b + [n]


def byte_bounds_np(offsets, ndev):
    """byte_bounds for large batches (the same rule through a binary search)."""
    off = np.asarray(offsets, np.uint64).astype(np.int64)
    n = off.size - 1
    b = [0]
    for i in range(1, ndev):
        target = int(off[0]) + (int(off[n]) - int(off[0])) * i // ndev
        b.append(max(min(int(np.searchsorted(off, target, side="left")), n), b[-1]))
    return b + [n]


# ---------------------------------------------------------------------------
# Seam classes: what a batch plants, told from its cut alone.
# ---------------------------------------------------------------------------
RAGGED_CLASSES = ["slices1", "slices2", "slices3", "slices4", "slices7", "last_one", "exact_bytes", "one_over",
                  "packet_limit", "zero_slice", "empty_edges", "long_first", "long_middle", "long_last",
                  "long_twice"]
UNIFORM_CLASSES = ["slices1", "slices2", "slices3", "slices4", "slices7", "last_one", "stride0", "stride_lt_len",
                   "stride_gt_slice", "n_multiple", "n_multiple_plus1"]
MULTI_CLASSES = ["shard_on_seam", "shard_off_seam"]


def classes_lens(lens, lim_b, lim_p):
    lens = np.asarray(lens, np.int64)
    n = lens.size
    cut = cut_lens(lens, lim_b, lim_p)
    got = set()
    if len(cut) in (1, 2, 3, 4, 7):
        got.add(f"slices{len(cut)}")
    if len(cut) > 1 and cut[-1][1] == 1:
        got.add("last_one")
    for f, c, b in cut:
        more = f + c < n
        if more and b == lim_b:
            got.add("exact_bytes")  # the slice ends exactly on the byte limit
        if more and c < lim_p and b < lim_b and b + lens[f + c] == lim_b + 1:
            got.add("one_over")  # one byte more than fits closed it
        if more and c == lim_p and 8 * b <= lim_b:
            got.add("packet_limit")  # closed by the packet limit, bytes far below the byte limit
        if b == 0 and c == lim_p and len(cut) > 1:
            got.add("zero_slice")
        if b and c > 2 and lens[f] == 0 and lens[f + c - 1] == 0:
            got.add("empty_edges")
    long_ = lens > lim_b
    if n > 1 and long_[0]:
        got.add("long_first")
    if n > 1 and long_[-1]:
        got.add("long_last")
    if n > 2 and long_[1:-1].any():
        got.add("long_middle")
    if (long_[1:] & long_[:-1]).any():
        got.add("long_twice")
    return got


def classes_uniform(stride, length, n, lim_b, lim_p):
    cut = cut_uniform(stride, length, n, lim_b, lim_p)
    got = set()
    if len(cut) in (1, 2, 3, 4, 7):
        got.add(f"slices{len(cut)}")
    if len(cut) > 1 and cut[-1][1] == 1:
        got.add("last_one")
    if stride == 0 and n > 1:
        got.add("stride0")
    if 0 < stride < length and n > 1:
        got.add("stride_lt_len")
    if stride > lim_b and n > 1:
        got.add("stride_gt_slice")
    per = cut[0][1]
    if n >= 2 * per and n % per == 0:
        got.add("n_multiple")
    if n > 2 * per and n % per == 1:
        got.add("n_multiple_plus1")
    return got


def classes_multi(cut, bounds):
    """A shard edge on an edge of the undivided batch's slices, or inside a slice."""
    edges = {f for f, _, _ in cut}
    got = set()
    for a in bounds[1:-1]:
        if 0 < a < bounds[-1]:
            got.add("shard_on_seam" if a in edges else "shard_off_seam")
    return got
