"""The host ledger's enumeration (tests/host_cases.py), on a CPU: it plants what the issue
lists, told by the model of the slice cut (tests/host_slices.py) and not by a recipe's
name, and the child's comparisons (tests/host_child.py) refuse wrong results."""
import collections

import numpy as np
import pytest

import host_cases as H
import host_child as C
import host_slices as S
from ledger_child import OUT_FILL, OUT_GUARD
from oracle import oracle as O

DIGEST = "e837ce36a59b8ee9"  # host_cases.digest() of the 559 ids


@pytest.fixture(scope="module")
def facts():
    return [H.facts(c) for c in H.CASES]


def test_knob_sets():
    assert H.KNOB_SETS[0] == {}
    assert H.limits(0) == (32 << 20, 1 << 18, 4 << 20)
    assert H.limits(1) == (4096, 16, 4 << 20) and H.limits(2) == (4096, 16, 0) and H.limits(3) == (65536, 16, 1024)
    assert H.KNOB_SETS[3]["YU_HOST_COPY_THREADS"] == "0"
    assert all(k.startswith("YU_HOST_") for env in H.KNOB_SETS for k in env)


def test_the_cases_keep_their_ids():
    """Cases are only appended: a case's bytes are seeded from its position."""
    assert [int(c["id"].split()[0]) for c in H.CASES] == list(range(len(H.CASES)))
    assert H.digest() == DIGEST, (H.digest(), len(H.CASES))


def test_cases_are_well_formed(facts):
    for c, f in zip(H.CASES, facts):
        mode = c["mode"]
        assert c["call"] == "batch" or mode in H.TX_MODES, c["id"]
        assert c["side"] in H.sides_of(mode), c["id"]
        assert (c["inmem"] == "pinned_odd") <= (c["align"] % 2 == 1), c["id"]
        assert c["off0"] == 0 or (c["layout"] == "R" and c["off0"] % 2 == 1 and c["off0"] <= 128), c["id"]
        lens = np.asarray([f["geometry"][1]] if c["layout"] == "U" else f["geometry"])
        cap = (0xFFFF0000 if mode == "raw" else 65535)
        assert lens.max() <= cap, c["id"]
        # below a mode's header size no value is defined: such packets go without a result array
        low = H.UNDEFINED_BELOW.get(mode, 0)
        assert (lens >= low).all() or c["call"] == "fill_null", c["id"]
        if c["layout"] == "U" and f["n"] > 1 and f["geometry"][0] < f["geometry"][1]:
            assert c["call"] == "batch" and mode not in ("tcp", "verify_tcp", "tx_datagram") or f["geometry"][0] == 0, c["id"]
        # sizes: the tuned sets stay small, the shipped one within about 72 MiB of host data
        if c["set"]:
            assert f["n"] <= 400 and f["data_bytes"] <= 512 << 10, (c["id"], f["n"], f["data_bytes"])
        else:
            assert f["data_bytes"] <= 72 << 20, c["id"]
        # every cut is whole: in order, no slice over a limit unless it is one packet
        lim_b, lim_p, _ = H.limits(c["set"])
        for (first, cnt), cut in zip(f["shards"], f["cuts"]):
            assert sum(s[1] for s in cut) == cnt and all(s[1] <= lim_p for s in cut), c["id"]


def _count(facts, layout, cls):
    return sum(1 for c, f in zip(H.CASES, facts) if c["layout"] == layout and cls in f["classes"])


def test_every_seam_class_is_planted_four_times(facts):
    short = {}
    for layout in "URV":
        for cls in (S.UNIFORM_CLASSES if layout == "U" else S.RAGGED_CLASSES) + S.MULTI_CLASSES:
            k = _count(facts, layout, cls)
            if k < 4:
                short[layout, cls] = k
    assert not short, short


def test_seam_pairs_differ_by_one_byte(facts):
    """exact / one_over: the same batch, one byte more in the packet that closed slice 0."""
    pairs = collections.defaultdict(dict)
    for c, f in zip(H.CASES, facts):
        if c["plan"][0] in ("exact", "one_over"):
            pairs[c["layout"], c["plan"][1]][c["plan"][0]] = (c, f)
    assert len(pairs) >= 8
    for p in pairs.values():
        (ca, fa), (cb, fb) = p["exact"], p["one_over"]
        assert ca["mode"] == cb["mode"] and ca["set"] == cb["set"]
        d = fb["geometry"] - fa["geometry"]
        assert d.sum() == 1 and np.count_nonzero(d) == 1
        assert "exact_bytes" in fa["classes"] and "one_over" in fb["classes"]
        assert fa["cuts"][0][0][1] == fb["cuts"][0][0][1] + 1


def test_every_layout_and_mode_on_both_routes_and_over_four_slices(facts):
    have = collections.defaultdict(set)
    for c, f in zip(H.CASES, facts):
        if f["multi"]:
            continue
        key = c["layout"], c["mode"]
        if f["slices"] == 1:
            have[key] |= {"direct" if f["routes"] == {"direct"} else "one slice copied"}
        if f["slices"] >= 4:
            have[key].add("four or more")
        if f["slices"] >= 7:
            have[key].add("slot 0 a third time")
    for layout in "URV":
        for mode in H.MODES:
            assert {"direct", "one slice copied", "four or more"} <= have[layout, mode], (layout, mode, have[layout, mode])
    assert sum("slot 0 a third time" in v for v in have.values()) >= 20


def test_side_arrays_cross_seams(facts):
    have = collections.defaultdict(set)
    for c, f in zip(H.CASES, facts):
        if f["slices"] >= 4 and c["side"] in ("addrs", "init"):
            have[c["mode"]].add(c["side"])
    for mode in H.PSEUDO:
        assert have[mode] == {"addrs", "init"}, (mode, have[mode])
    assert have["raw"] == {"init"}
    # junk in the ignored arguments of every mode
    assert {c["mode"] for c in H.CASES if c["side"] == "junk"} == set(H.MODES)


def test_tx_modes_in_place_on_both_routes(facts):
    have = collections.defaultdict(set)
    for c, f in zip(H.CASES, facts):
        if c["call"] != "batch" and not f["multi"]:
            have[c["layout"], c["mode"], c["call"]] |= f["routes"]
    for layout in "URV":
        for mode in H.TX_MODES:
            for call in ("fill", "fill_null"):
                assert have[layout, mode, call] == {"direct", "copied"}, (layout, mode, call)


def test_tx_datagram_results_cross_seams_into_pinned_and_pageable_memory(facts):
    have = {(c["layout"], c["outmem"]) for c, f in zip(H.CASES, facts)
            if c["mode"] == "tx_datagram" and f["slices"] >= 2 and c["call"] != "fill_null"}
    assert have == {(lay, o) for lay in "URV" for o in H.OUTMEM}


def test_memory_kinds_and_views(facts):
    for layout in "URV":
        mine = [c for c in H.CASES if c["layout"] == layout]
        assert {c["inmem"] for c in mine} == set(H.INMEM) and {c["outmem"] for c in mine} == set(H.OUTMEM)
    assert {c["off0"] for c in H.CASES if c["layout"] == "R"} >= {0, 7, 101}
    assert {c["views"] for c in H.CASES if c["layout"] == "V"} >= {"rand", "split_field", "ones", "one"}
    assert {type(c["devices"]) for c in H.CASES} == {int, list}


def test_short_and_malformed_packets_reach_the_field_writer(facts):
    oracle = O.C()
    seen = collections.Counter()
    for c, f in zip(H.CASES, facts):
        if c["plan"][0] != "short":
            continue
        P = C.prepare(c, oracle)
        seen[c["mode"], "undefined"] += int((~P.defined).sum())
        seen[c["mode"], "stored"] += int(np.count_nonzero(P.expected != P.arena) > 0)
        if c["layout"] == "V" and c["views"] == "split_field":
            # a field's two bytes in different views, an empty view between them
            k = 0
            for i in range(P.n):
                v = P.vlen[int(P.first[i]):int(P.first[i + 1])]
                k += any(v[j] > 0 and v[j + 1] == 0 and v[j + 2] > 0 for j in range(len(v) - 2))
            assert k >= 5, c["id"]
    assert seen["udp", "undefined"] and seen["icmp", "undefined"]
    assert all(seen[m, "stored"] for m in ("udp", "icmp", "ipv4", "tx_datagram"))


def test_shipped_constants_at_their_real_sizes(facts):
    h0 = [(c, f) for c, f in zip(H.CASES, facts) if c["set"] == 0]
    P, B = S.SLICE_PACKETS, S.SLICE_BYTES
    for layout in "URV":
        assert {f["n"] for c, f in h0 if c["layout"] == layout} >= {P, P + 1}
        assert any(f["slices"] == 2 and f["cuts"][0][0][1] == P for c, f in h0 if c["layout"] == layout)
    assert any(c["layout"] == "R" and f["cuts"][0][0][2] == B and f["slices"] == 2 for c, f in h0)
    assert any(f["n"] == 1 and f["data_bytes"] == 33 << 20 and f["staging"] == (0, 0) for c, f in h0)
    sizes = {f["data_bytes"] for c, f in h0 if c["layout"] == "U" and c["inmem"] == "pageable"}
    assert sizes >= {(2 << 20) - 1, 2 << 20, (2 << 20) + 1, (8 << 20) + 63}
    big_v = [f for c, f in h0 if c["layout"] == "V" and f["data_bytes"] >= 2 << 20]
    parts = [min(H.COPY_THREADS + 1, f["data_bytes"] >> 20) for f in big_v]
    # the gather: split over the copy threads when there are as many packets as parts, else serial
    assert any(f["n"] < p and p >= 2 for f, p in zip(big_v, parts)), "fewer packets than copy threads"
    assert any(f["n"] >= p >= 2 for f, p in zip(big_v, parts)), "more packets than copy threads"
    assert {f["n"] for c, f in h0 if c["call"] != "batch"} >= {1 << 17, (1 << 17) + 1}
    direct = {c["align"] for c, f in h0 if c["inmem"] != "pageable" and f["routes"] == {"direct"}}
    assert direct == set(range(16))


def _slice_seam(f):
    """(first packet of the second slice, count of the first slice) of a case of several slices."""
    cut = f["cuts"][0]
    return cut[1][0], cut[0][1]


def test_the_childs_comparisons_fail_on_wrong_results(facts):
    """As tests/test_kernel_ledger.py does for the kernel ledger: four faulty outcomes, each
    refused by the comparison the child makes."""
    oracle = O.C()
    pick = lambda pred: next((c, f) for c, f in zip(H.CASES, facts) if pred(c, f))  # noqa: E731
    # a result flipped at a slice's first packet
    c, f = pick(lambda c, f: f["slices"] >= 4 and c["call"] == "batch" and not f["multi"] and c["mode"] == "udp")
    P = C.prepare(c, oracle)
    alloc = np.full(2 * OUT_GUARD + P.n * P.k, OUT_FILL, np.uint16)
    alloc[OUT_GUARD:OUT_GUARD + P.n * P.k] = P.want
    assert C.check_out(alloc, OUT_GUARD, P.want) is None
    bad = alloc.copy()
    bad[OUT_GUARD + _slice_seam(f)[0] * P.k] ^= 1
    assert "results differ" in C.check_out(bad, OUT_GUARD, P.want)
    # the results shifted by one slice
    bad = alloc.copy()
    first = _slice_seam(f)[1] * P.k
    bad[OUT_GUARD + first:OUT_GUARD + P.n * P.k] = P.want[:P.n * P.k - first]
    assert "results differ" in C.check_out(bad, OUT_GUARD, P.want)
    # a changed guard entry
    bad = alloc.copy()
    bad[OUT_GUARD - 1] = 0
    assert "guard entries before" in C.check_out(bad, OUT_GUARD, P.want)
    bad = alloc.copy()
    bad[OUT_GUARD + P.n * P.k] = 0
    assert "guard entries after" in C.check_out(bad, OUT_GUARD, P.want)
    # a stored field in a packet that must not be written, and a changed guard byte of the arena
    c, f = pick(lambda c, f: c["plan"][0] == "short" and c["mode"] == "udp" and c["layout"] == "R")
    P = C.prepare(c, oracle)
    assert C.check_memory(P.expected, P.expected) is None
    i = int(np.flatnonzero((P.lens < 8) & (P.lens > 0))[0])
    bad = P.expected.copy()
    bad[P.starts[i] + P.lens[i] - 1] ^= 0x80  # its last byte: where a field store that ignored the length could land
    assert "bytes differ" in C.check_memory(bad, P.expected)
    bad = P.expected.copy()
    bad[-1] ^= 1
    assert "bytes differ" in C.check_memory(bad, P.expected)
    # and a read-only call's memory is the input itself
    c, f = pick(lambda c, f: c["call"] == "batch" and c["layout"] == "V")
    P = C.prepare(c, oracle)
    assert P.expected is P.arena


def test_the_rules_name_a_dropped_class(facts):
    """The counting rule itself: without the cases of one recipe its class comes up short."""
    keep = [(c, f) for c, f in zip(H.CASES, facts) if c["plan"][0] != "zeros"]
    assert sum(1 for c, f in keep if c["layout"] == "R" and "zero_slice" in f["classes"]) < 4
