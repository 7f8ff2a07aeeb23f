"""The host path's geometry and field writer on a CPU (yustack_amd/csrc/yucsum_hostgeom.h,
the parts of yucsum_host.cpp that make no HIP call): tests/cpp/host_geom.cpp, a plain g++
program with its own main, prints the header's slice cut, burst predicate and shard
bounds for batches written here and dumps what its field writer did to guarded buffers.

Slices: uniform, ragged and view batches over a grid of (slice bytes, slice packets),
(4096, 16) and the shipped (32 MiB, 256K) among them, against the model tests/host_slices.py
(written from the header's comments), plus on every batch: every packet in exactly one
slice, slices in order, no slice over a limit unless it holds one packet, the burst
predicate. Shards: even_bounds and byte_bounds for 1..8 devices (offsets starting above 0,
runs of empty packets at a target, more devices than packets): the model's bounds,
monotone, covering [0, n]. Fields: every TX mode through the three accessors with
arbitrary result words, packets of 0..96 bytes, IHL 0..15, TotalLength from HL - 1 to
len + 1, protocols 1, 6, 17, 47, views of 0 and 1 bytes around the fields; the whole
buffer, guard bytes included, against the rule as tests/test_gpu_contract.py states it
(_fields). The same program runs once more under AddressSanitizer + UBSan, as its own
executable."""
import os
import subprocess

import numpy as np
import pytest

import host_slices as S
from oracle import oracle as O
from test_gpu_contract import _fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "host_geom.cpp")
INC = [f"-I{ROOT}/include", f"-I{ROOT}/yustack_amd/csrc"]
PLAIN = ["-O2"]
SANITIZED = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
GRID = [(4096, 16), (4096, 1), (1, 16), (65536, 16), (1000, 7), (S.SLICE_BYTES, S.SLICE_PACKETS),
        (S.SLICE_BYTES, 5), (100, S.SLICE_PACKETS)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_geom")
    built = {}

    def get(name, flags):
        if name not in built:
            path = str(d / name)
            r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, *INC, SOURCE, "-o", path],
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-3000:]
            built[name] = path
        return built[name]

    get.dir = d
    return get


def _run(exe_path, *args):
    r = subprocess.run([exe_path, *args], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


# ---------------------------------------------------------------------------
# slices
# ---------------------------------------------------------------------------
def _length_lists(rng, lim_b, lim_p):
    """Packet lengths placed where the cut decides: around both limits, empty runs, long
    packets, and random ones."""
    out = []
    small = lim_b <= (1 << 20)
    if small:
        q = lim_b // 4
        out += [[q] * 4 + [1], [q] * 3 + [lim_b - 3 * q, 1, 0, 0], [q] * 3 + [lim_b - 3 * q + 1, 5],
                [0] * (3 * min(lim_p, 64) + 1), [0] * min(lim_p, 64) + [7] + [0] * min(lim_p, 64),
                [lim_b + 1, 3, lim_b + 9, lim_b + 1, 0, 2, lim_b + 5], [lim_b], [lim_b + 1], [0], [1],
                [0, lim_b, 0, 0, lim_b, 1, 0]]
        for _ in range(6):
            n = int(rng.integers(1, 200))
            lens = rng.integers(0, max(lim_b // 3, 2), size=n)
            lens[rng.random(n) < 0.3] = 0
            lens[rng.random(n) < 0.05] = lim_b + int(rng.integers(0, 3))
            out.append(lens.tolist())
    else:  # the shipped limits: the packet seam, the byte seam, a packet past the slice
        out += [rng.integers(0, 41, size=lim_p + 1).tolist() if lim_p < (1 << 20) else [3],
                [65535] * (lim_b // 65535) + [lim_b % 65535, 0, 1], [65535] * (lim_b // 65535) + [lim_b % 65535 + 1, 2],
                [lim_b + 1, 1, lim_b + 1], [0] * min(lim_p + 3, 300_000)]
    return out


def _views_of(rng, lens):
    """Each packet's bytes in 0..4 views (an empty packet: no view, or empty views)."""
    out = []
    for ln in lens:
        k = int(rng.integers(0 if ln == 0 else 1, 5))
        cuts = sorted(int(x) for x in rng.integers(0, ln + 1, size=max(k - 1, 0)))
        edges = [0] + cuts + [ln]
        out.append([edges[j + 1] - edges[j] for j in range(len(edges) - 1)] if k else [])
    return out


def _slice_batches():
    rng = np.random.default_rng(1204)
    batches = []  # (line, model cut, limits, n, direct_max)
    for lim_b, lim_p in GRID:
        for dmax in (0, 1024, S.DIRECT_MAX):
            for lens in _length_lists(rng, lim_b, lim_p):
                if len(lens) > 1000 and dmax != S.DIRECT_MAX:
                    continue
                cut = S.cut_lens(lens, lim_b, lim_p)
                o0 = int(rng.integers(0, 1000))
                batches.append((f"R {{id}} {lim_b} {lim_p} {dmax} {len(lens)} {o0} " + " ".join(map(str, lens)),
                                cut, (lim_b, lim_p), len(lens), dmax))
                if len(lens) <= 1000:
                    views = _views_of(rng, lens)
                    batches.append((f"V {{id}} {lim_b} {lim_p} {dmax} {len(lens)} " +
                                    " ".join(" ".join(map(str, [len(v)] + v)) for v in views),
                                    cut, (lim_b, lim_p), len(lens), dmax))
            per = max(1, lim_b // 64)
            shapes = [(0, 40, 100), (0, 0, 5), (64, 64, min(lim_p, per) * 3), (64, 64, min(lim_p, per) * 3 + 1),
                      (16, 40, 3 * lim_p + 2), (lim_b + 8, 20, 5), (lim_b, 20, 5), (1, 1, 1), (1500, 1500, 1),
                      (8, 8, lim_p), (8, 8, lim_p + 1), (8, 6, 2 * lim_p - 1)]
            for stride, ln, n in shapes:
                if n > 2_000_000:
                    continue
                batches.append((f"U {{id}} {lim_b} {lim_p} {dmax} {stride} {ln} {n}",
                                S.cut_uniform(stride, ln, n, lim_b, lim_p), (lim_b, lim_p), n, dmax))
    return batches


def _check_cut(cut, n, lim_b, lim_p, bytes_bound=True):
    """Every packet in exactly one slice, in order; no slice over a limit unless one packet."""
    nxt = 0
    for first, cnt, b in cut:
        assert first == nxt and cnt >= 1, cut[:5]
        assert cnt <= lim_p, (first, cnt, lim_p)
        assert b <= lim_b or cnt == 1 or not bytes_bound, (first, cnt, b, lim_b)
        nxt = first + cnt
    assert nxt == n


def _slices(exe_path, d):
    batches = _slice_batches()
    knobs = [("-", 4096, 4096), ("''", 4096, 4096), ("0", 4096, 4096), ("1", 4096, 1), ("4096", 4096, 4096),
             ("4097", 4096, 4096), ("16", 1 << 18, 16), ("abc", 4096, 4096), ("12x", 4096, 4096),
             (str(1 << 25), 1 << 25, 1 << 25), (str((1 << 25) + 1), 1 << 25, 1 << 25)]
    path = str(d / "slices.in")
    with open(path, "w") as f:
        for i, b in enumerate(batches):
            f.write(b[0].format(id=i) + "\n")
        for i, (v, compiled, _) in enumerate(knobs):
            f.write(f"K {len(batches) + i} {v} {compiled}\n")
    lines = _run(exe_path, "slices", path).splitlines()
    assert len(lines) == len(batches) + len(knobs)
    kinds = set()
    for i, (line, model, (lim_b, lim_p), n, dmax) in enumerate(batches):
        w = lines[i].split()
        assert int(w[0]) == i
        cut = [tuple(int(x) for x in s.split(":")) for s in w[2:]]
        # (a uniform slice's span may pass the byte limit by under len when stride < len)
        overlapping = line[0] == "U" and int(line.split()[5]) < int(line.split()[6])
        _check_cut(cut, n, lim_b, lim_p, bytes_bound=not overlapping)
        assert cut == model, (line[:80], cut[:4], model[:4])
        assert w[1] == f"burst={int(S.is_burst(model, dmax))}", (line[:80], w[1])
        kinds.add((line[0], len(cut) > 1, w[1]))
    assert len(kinds) == 9, kinds  # three layouts x (one slice direct, one slice copied, several slices)
    for i, (v, compiled, want) in enumerate(knobs):
        assert lines[len(batches) + i].split() == [str(len(batches) + i), str(want)], (v, lines[len(batches) + i])
        assert S.limit(None if v == "-" else "" if v == "''" else v, compiled) == want
    return len(batches)


# ---------------------------------------------------------------------------
# shards
# ---------------------------------------------------------------------------
def _shards(exe_path, d):
    rng = np.random.default_rng(877)
    jobs = []
    for ndev in range(1, 9):
        for n in (0, 1, 2, 3, 7, 8, 9, 1000, (1 << 18) + 1):
            jobs.append((f"E {{id}} {n} {ndev}", S.even_bounds(n, ndev), n))
        lists = [[5], [0], [0] * 9, [10] * 8, [0, 0, 0, 40, 0, 0, 0, 40, 0, 0], [40] + [0] * 20 + [40],
                 [0] * 10 + [8] * 8 + [0] * 10, [1, 2, 3], rng.integers(0, 100, size=50).tolist(),
                 (rng.integers(0, 3, size=200) * rng.integers(0, 50, size=200)).tolist()]
        for lens in lists:
            for o0 in (0, 7, 1 << 33):
                off = np.concatenate(([o0], o0 + np.cumsum(lens))).astype(np.uint64)
                model = S.byte_bounds(off, ndev)
                assert model == S.byte_bounds_np(off, ndev)
                jobs.append((f"B {{id}} {ndev} {len(lens)} {o0} " + " ".join(map(str, lens)), model, len(lens)))
    path = str(d / "shards.in")
    with open(path, "w") as f:
        for i, j in enumerate(jobs):
            f.write(j[0].format(id=i) + "\n")
    lines = _run(exe_path, "shards", path).splitlines()
    assert len(lines) == len(jobs)
    for i, (line, model, n) in enumerate(jobs):
        got = [int(x) for x in lines[i].split()]
        assert got[0] == i
        b = got[1:]
        assert b[0] == 0 and b[-1] == n and all(x <= y for x, y in zip(b, b[1:])), (line[:60], b)
        assert b == model, (line[:60], b, model)
    return len(jobs)


# ---------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------
HEAD, ARENA, VIEWS = 4 + 8 + 2 * 14, 128, 14


def _fields_check(exe_path, d):
    path = str(d / "fields.bin")
    out = _run(exe_path, "fields", path)
    count = int(out.split()[0])
    rec = np.fromfile(path, np.uint8).reshape(-1, HEAD + 2 * ARENA)
    assert rec.shape[0] == count and count > 100_000
    seen = set()
    stored = 0
    for r in rec:
        mode, acc, ln, nv = (int(x) for x in r[:4])
        vals = [int(x) for x in r[4:8].view(np.uint16)]
        before, after = r[HEAD:HEAD + ARENA], r[HEAD + ARENA:]
        # packet byte -> arena index, through the views
        where = np.concatenate([np.arange(int(r[12 + 2 * v]), int(r[12 + 2 * v]) + int(r[13 + 2 * v])) for v in range(nv)]
                               + [np.zeros(0, np.int64)]).astype(np.int64)
        assert where.size == ln
        pkt = before[where]
        exp = before.copy()
        writes = _fields(mode, pkt, 0, ln, vals)
        for pos, v in writes:
            exp[where[pos]] = v
        assert np.array_equal(after, exp), (mode, acc, ln, r[12:12 + 2 * nv].tolist(), pkt.tolist(), vals,
                                            np.nonzero(after != exp)[0].tolist())
        stored += len(writes) // 2
        seen.add((mode, acc, len(writes) // 2))
    # every TX mode x accessor both stores and declines; datagrams store none, one and two fields
    for acc in range(3):
        for mode in (O.MODE_UDP, O.MODE_TCP, O.MODE_ICMP, O.MODE_IPV4):
            assert {(mode, acc, 0), (mode, acc, 1)} <= seen
        assert {(O.MODE_TX_DATAGRAM, acc, k) for k in (0, 1, 2)} <= seen
    return count, stored


def test_slices_match_the_model(exe):
    print(_slices(exe("host_geom", PLAIN), exe.dir), "batches")


def test_shard_bounds_match_the_model(exe):
    print(_shards(exe("host_geom", PLAIN), exe.dir), "splits")


def test_field_writer_matches_the_rule(exe):
    print("%d records, %d fields stored" % _fields_check(exe("host_geom", PLAIN), exe.dir))


def test_host_geom_under_sanitizers(exe):
    """The same program as its own executable under AddressSanitizer + UBSan: all three
    parts, with the same comparisons (nothing is preloaded anywhere)."""
    path = exe("host_geom_san", SANITIZED)
    d = exe.dir / "san"
    d.mkdir()
    _slices(path, d)
    _shards(path, d)
    _fields_check(path, d)
