"""The kernel ledger (tests/kernel_cases.py) against the planner, on the CPU: every
case's written plan is the planner's at 64, 256 and 304 CUs, the built library names the
same kernel, and the cases cover every key (kernel, form, policy, in place, layout) the
planner can return (tests/cpp/plan_query.cpp --reachable; layout "I", the scatter-gather
calls: tests/cpp/wave_plan.cpp under each knob set). Every kernel is also held in every
call shape (offset, null_out, ignored) and on the zero poles (pole_side, pole_data, all-zero
and all-0xFF packets in place) its modes allow, and the child's comparisons are shown to
fail on a wrong result and on a changed guard entry. tests/test_gpu_kernel_ledger.py runs
the same cases on the GPU. The seam cases (tests/seg_seams.py) are rebuilt here with the
child's own seed and shown to sit on every seam class of their kind."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_cases as K
import wave_plan
from test_plan import CSRC, HIP_HEADERS, ROOT

SOURCES = [os.path.join(ROOT, "tests", "cpp", "plan_query.cpp"), os.path.join(CSRC, "yucsum_plan.cpp")]
HEADERS = [os.path.join(ROOT, "tests", "cpp", "plan_rows.h"), os.path.join(CSRC, "yucsum_plan.h"),
           os.path.join(CSRC, "yucsum_internal.h")]
BIN = os.path.join(ROOT, "tests", "cpp", "build", "plan_query")
KERNELS = 39  # the planner's; beside them the len(K.IOV_KERNELS) = 2 of the scatter-gather calls
ALL_KERNELS = KERNELS + len(K.IOV_KERNELS)
BASE_IDS = "6501eef667e93d86c2948da7fa59f9b79ce87323018151057e04abaa6b27f201"
IDS_BEFORE_SEAMS = "dcca9c025b53cd4f79f8ace791a9e4de074a8492d0e1cc0f3ad49dc862994801"  # the first 2055


@pytest.fixture(scope="module")
def query():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in SOURCES + HEADERS):
        r = subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT}/include", *HIP_HEADERS, *SOURCES, "-o", BIN],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    return BIN


@pytest.fixture(scope="module")
def iov_plan():
    """run(s, rows) asks yu::plan_wave (tests/wave_plan.py) about the scatter-gather calls'
    (n, mode, fill, cus) rows under knob set s and returns (name, policy)."""
    def run(s, rows):
        env = dict(K.KNOB_SETS[s], YU_TUNING="1") if s else None
        return [(name, str(policy)) for _, policy, _, name in wave_plan.plans("iov", rows, env)]
    return run


@pytest.fixture(scope="module")
def reachable(query, iov_plan):
    r = subprocess.run([query, "--reachable"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [tuple(line.split()) for line in r.stdout.splitlines()]
    keys = {ln[1:] for ln in lines if ln[0] == "K"}
    defaults = {ln[1:] for ln in lines if ln[0] == "D"}
    assert len(keys) > 200 and len(defaults) > 100 and len({k[0] for k in keys}) == KERNELS
    # layout "I": what yu::plan_wave returns under each knob set
    rows = [(n, K.MODES.index(m), f, cus) for m in K.IOV_MODES for f in ((0, 1) if m in K.FILL3 else (0,))
            for n in (1, 37, 4097, 1 << 20) for cus in (64, 256)]
    iov = set()
    for s in range(len(K.KNOB_SETS)):
        for (name, policy), (_, m, f, _) in zip(iov_plan(s, rows), rows):
            iov.add((name, "plain", policy, str(f), "I"))
            if s == 0:
                defaults.add((name, K.MODES[m], str(f), "I"))
    assert {k[0] for k in iov} == set(K.IOV_KERNELS) and len(iov) == 6  # two kernels x three policy slots
    return keys | iov, defaults


def case_keys(cases=None):
    """The keys the cases hold: (kernel, form, policy, in place, layout)."""
    keys = set()
    for c in K.CASES if cases is None else cases:
        for plan in c["plans"].values():
            keys.add((*plan.split(), str(int(c["fill"])), c["layout"]))
    return keys


def default_tuples(cases=None):
    return {(c["plans"][0].split()[0], c["mode"], str(int(c["fill"])), c["layout"])
            for c in (K.CASES if cases is None else cases) if 0 in c["plans"]}


def test_knob_sets():
    sets = K.KNOB_SETS
    assert sets[0] == {}
    # the issue asked for at most 10; the keys need 12 tuned environments (kernel_cases.py, "Knob sets")
    assert len(sets) <= K.MAX_KNOB_SETS == 13
    assert all(s.get("YU_BLOCKS_PER_CU") == "1" for s in sets[1:])
    assert any(s.get("YU_XCD") == "1" for s in sets) and any(s.get("YU_SEG_SMALL_BLOCKS") == "0" for s in sets)
    assert all("YU_VARIANT" not in s and "YU_TUNING" not in s for s in sets)
    assert len({tuple(sorted(s.items())) for s in sets}) == len(sets)


def test_the_base_cases_keep_their_ids():
    """A case's id is its position and the child seeds its bytes from it: cases are only
    appended (the digest: the ids of the N_BASE cases the ledger had before the call
    shapes, the poles and k_iov)."""
    assert K.N_BASE == 1592 and all(c["call"] == "plain" for c in K.CASES[:K.N_BASE])
    assert [int(c["id"].split()[0]) for c in K.CASES] == list(range(len(K.CASES)))
    assert hashlib.sha256("\n".join(c["id"] for c in K.CASES[:K.N_BASE]).encode()).hexdigest() == BASE_IDS
    # ... and of the 2055 it had before the seam cases (call shapes, poles and k_iov included)
    assert K.N_BEFORE_SEAMS == 2055
    assert hashlib.sha256("\n".join(c["id"] for c in K.CASES[:2055]).encode()).hexdigest() == IDS_BEFORE_SEAMS


def test_cases_are_well_formed():
    assert len({c["id"] for c in K.CASES}) == len(K.CASES)
    for c in K.CASES:
        assert c["plans"] and all(0 <= s < len(K.KNOB_SETS) for s in c["plans"]), c["id"]
        assert c["mode"] in K.MODES and c["side"] in K.SIDES.get(c["mode"], ("scalar",)), c["id"]
        assert c["kind"] in ("rand", "zero", "ff", "pole_side", "pole_data"), c["id"]
        shapes = K.calls(c)
        assert shapes == {"plain"} or shapes <= {"offset", "null_out", "ignored"}, c["id"]
        assert "null_out" not in shapes or c["fill"], c["id"]  # the read-only calls refuse a NULL out
        assert "ignored" not in shapes or K.ignores(c["mode"], c["side"]), c["id"]
        assert c["id"].endswith(c["kind"] if c["call"] == "plain" else c["kind"] + " " + c["call"]), c["id"]
        if c["kind"] == "pole_side":
            assert c["side"] == "init" and c["mode"] not in K.DGRAM, c["id"]
            assert c["layout"] != "U" or c["mode"] != "raw" or c["len"] <= 65535, c["id"]
            assert c["layout"] != "R" or c["gen"][0] == "range" and c["gen"][2] <= 65535, c["id"]
        if c["kind"] == "pole_data":
            assert c["mode"] in K.POLE_W and c["side"] in ("addrs", "scalar"), c["id"]
            assert c["side"] == "addrs" or c["mode"] not in K.SIDES, c["id"]  # the pole comes out of the byte sum
            shortest = c["len"] if c["layout"] == "U" else c["gen"][1] if c["layout"] == "R" else 40
            assert shortest >= K.POLE_W[c["mode"]] + 2, c["id"]
        if c["layout"] == "I":
            assert c["mode"] in K.IOV_MODES and c["iov"] in K.IOV_SHAPES and K.kernel_of(c)[0] == K.IOV_KERNELS[c["fill"]]
            assert not (c["kind"] in ("zero", "ff") and c["mode"] in ("tcp", "verify_tcp")), c["id"]
            for n in (1, 37):
                assert all(sum(v[2] for v in pk) >= K.MIN_LEN.get(c["mode"], 0) for pk in K.iov_packets(c, n)), c["id"]
        if c["n"] == "n_wrap":
            assert 0 not in c["plans"] and c["ppw"], c["id"]  # one block per CU: not the default set
        if c["layout"] == "U":
            assert c["len"] >= K.MIN_LEN.get(c["mode"], 0), c["id"]
            if c["fill"]:  # include/yucsum.h [fill-align], [fill-overlap]
                assert c["base"] % 4 == 0 and c["stride"] % 4 == 0 and c["stride"] >= c["len"], c["id"]
        for s in c["plans"]:
            for cus in K.CU_COUNTS:
                if s == 0 and c["n"] == "n_wrap":
                    continue
                n = K.resolve_n(c, cus, K.KNOB_SETS[s])
                assert c["n_lo"] <= n and (c["n_hi"] is None or n <= c["n_hi"]), c["id"]
                assert K.case_bytes(c, n) <= K.MAX_CASE_BYTES, (c["id"], n, K.case_bytes(c, n))


def test_written_plans_are_the_planners(query, iov_plan):
    """Kernel, form and policy of every case under every set it runs in, at three CU
    counts (only `blocks` may differ between cards); ppw where the case states it. Layout
    "I": yu::plan_wave's kernel and policy (a wave per packet: ppw 1)."""
    text, want = [], []
    for s, env in enumerate(K.KNOB_SETS):
        text.append("# knobs: " + " ".join(f"{k}={v}" for k, v in env.items()))
        mine = [(c, cus) for c in K.CASES if s in c["plans"] and c["layout"] == "I" for cus in K.CU_COUNTS]
        rows = [(K.resolve_n(c, cus, env), K.MODES.index(c["mode"]), int(c["fill"]), cus) for c, cus in mine]
        for (c, cus), (name, policy) in zip(mine, iov_plan(s, rows) if rows else []):
            assert f"{name} plain {policy}" == c["plans"][s] and c["ppw"] == 1, (c["id"], s, cus, name, policy)
        for c in K.CASES:
            if s in c["plans"] and c["layout"] != "I":
                for cus in K.CU_COUNTS:
                    text.append(K.query_line(c, K.resolve_n(c, cus, env), cus))
                    want.append((c, s))
    r = subprocess.run([query], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [line for line in r.stdout.splitlines() if not line.startswith("#")]
    assert len(rows) == len(want)
    wrong = []
    for row, (c, s) in zip(rows, want):
        name, form, policy, _blocks, ppw = row.split(" | ")[1].split()[:5]
        if f"{name} {form} {policy}" != c["plans"][s] or (c["ppw"] and int(ppw) != c["ppw"]):
            wrong.append(f"{c['id']} under set {s}: wrote {c['plans'][s]} ppw {c['ppw']}, planner: {row}")
    assert not wrong, "\n".join(wrong[:20])


_ASK = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import kernel_cases as K
from yustack_amd import batch
s = int(sys.argv[1])
for c in K.CASES:
    if s in c["plans"]:
        n = K.resolve_n(c, 256, K.KNOB_SETS[s])
        if c["layout"] == "U":
            print(batch.variant(c["stride"], c["len"], c["mode"], c["base"], n=n))
        elif c["layout"] == "I":
            print(batch.iov_variant(c["mode"], n, fill=c["fill"]))
        else:
            print(batch.ragged_variant(c["mode"], n, fill=c["fill"]))
"""


@pytest.fixture(scope="module")
def library_answers():
    """One child per knob set, all started at once (they only ask for names: no GPU work)."""
    procs = []
    for s, knobs in enumerate(K.KNOB_SETS):
        env = {k: v for k, v in os.environ.items() if not k.startswith("YU_")}
        if s:
            env.update(knobs, YU_TUNING="1")
        procs.append(subprocess.Popen([sys.executable, "-c", _ASK % (ROOT, os.path.join(ROOT, "tests")), str(s)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    answers = []
    for p in procs:
        try:
            out, err = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            out, err = p.communicate()
        answers.append((p.returncode, out, err))
    return answers


@pytest.mark.parametrize("s", range(len(K.KNOB_SETS)))
def test_library_names_the_written_kernel(library_answers, s):
    """The built library, asked in a child process started with the set's knobs
    (batch.variant / batch.ragged_variant; a uniform in-place call has no query of its
    own: the uniform pick does not depend on it)."""
    rc, out, err = library_answers[s]
    assert rc == 0, err[-3000:]
    cases = [c for c in K.CASES if s in c["plans"]]
    got = out.split()
    assert len(got) == len(cases)
    wrong = [f"{c['id']}: library {g}" for c, g in zip(cases, got) if g != c["plans"][s].split()[0]]
    assert not wrong, "\n".join(wrong[:20])


def test_cases_cover_every_reachable_key(reachable):
    keys, _ = reachable
    missing = sorted(keys - case_keys())
    assert not missing, f"no case holds these keys (kernel, form, policy, in place, layout): {missing}"


def test_default_cases_cover_every_default_tuple(reachable):
    _, defaults = reachable
    missing = sorted(defaults - default_tuples())
    assert not missing, f"no default-knob case for (kernel, mode, in place, layout): {missing}"


def test_every_kernel_in_every_policy_and_form():
    triples = {k[:3] for k in case_keys()}
    kernels = sorted({t[0] for t in triples})
    assert len(kernels) == ALL_KERNELS and set(K.IOV_KERNELS) <= set(kernels), kernels
    missing = []
    for kern in kernels:
        forms = ["runs", "inter"] if kern.startswith("k_small") else ["plain", "fill"] if kern == "k_tiny<4>" \
            else ["plain"]
        assert {t[1] for t in triples if t[0] == kern} == set(forms), kern
        missing += [(kern, f, p) for f in forms for p in "012" if (kern, f, p) not in triples]
    assert not missing, missing


def test_every_kernel_sees_addrs_and_initial_arr():
    by_kernel = {}
    for c in K.CASES:
        for plan in c["plans"].values():
            by_kernel.setdefault(plan.split()[0], []).append(c)
    assert len(by_kernel) == ALL_KERNELS
    for kern, cases in by_kernel.items():
        allowed = {side for c in cases for side in K.SIDES.get(c["mode"], ())}
        seen = {c["side"] for c in cases}
        assert allowed - {"scalar"} <= seen, (kern, allowed, seen)


def test_every_key_has_a_second_pass():
    """One n_wrap case per key: the grid-stride loop's second pass (and k_seg's chunk
    pipeline across it) under one block per CU."""
    wrap = case_keys([c for c in K.CASES if c["n"] == "n_wrap"])
    # the far-stride k_small cases hold two packets: no second pass at 32 MiB a packet
    missing = sorted(k for k in case_keys() - wrap if not (k[0] in ("k_small<4,1>", "k_small<8,1>") and k[3] == "1"))
    assert not missing, missing


# ---------------------------------------------------------------------------
# Call shapes and zero poles: what every kernel must be held in. Each rule returns the
# kernels (and what they lack), so that a missing case is named.
# ---------------------------------------------------------------------------
def by_kernel(cases=None):
    found = {}
    for c in K.CASES if cases is None else cases:
        found.setdefault(K.kernel_of(c)[0], []).append(c)
    return found


def missing_call_shapes(cases=None):
    missing = []
    for kern, mine in sorted(by_kernel(cases).items()):
        # offset: out at 2 (mod 4) and every side array the kernel's modes take at its least alignment
        off = [c for c in mine if "offset" in K.calls(c) and "null_out" not in K.calls(c)]
        if not off:
            missing.append(f"{kern}: no offset case with a result array")
        for side in sorted({sd for c in mine for sd in K.SIDES.get(c["mode"], ())} - {"scalar"}):
            if not any(c["side"] == side for c in mine if "offset" in K.calls(c)):
                missing.append(f"{kern}: no offset case with {side}")
        for lay in ("R", "I"):  # offsets / the view table and first_iov at 8 (mod 16)
            if any(c["layout"] == lay for c in mine) and not any(c["layout"] == lay for c in mine if "offset" in K.calls(c)):
                missing.append(f"{kern}: no offset case of layout {lay}")
        if any(c["mode"] == "tx_datagram" for c in mine) and not any(c["mode"] == "tx_datagram" for c in off):
            missing.append(f"{kern}: no TX_DATAGRAM offset case (the two 16-bit result stores)")
        # null_out: every (kernel, form) that writes in place, and once across a second pass of the grid
        for form in sorted({K.kernel_of(c)[1] for c in mine if c["fill"]}):
            if not any("null_out" in K.calls(c) for c in mine if K.kernel_of(c)[1] == form):
                missing.append(f"{kern} {form}: no null_out case")
        # (the in-place cases of the two smallest k_small windows hold two packets 32 MiB apart: no second pass)
        if any(c["fill"] for c in mine) and kern not in ("k_small<4,1>", "k_small<8,1>") and \
                not any("null_out" in K.calls(c) and c["n"] == "n_wrap" for c in mine):
            missing.append(f"{kern}: no null_out case across a second pass (n_wrap)")
        # ignored: every kernel runs a mode with something to ignore
        if not any("ignored" in K.calls(c) for c in mine):
            missing.append(f"{kern}: no ignored case")
    return missing


def missing_poles(cases=None):
    missing = []
    for kern, mine in sorted(by_kernel(cases).items()):
        if any("init" in K.SIDES.get(c["mode"], ()) for c in mine) and not any(c["kind"] == "pole_side" for c in mine):
            missing.append(f"{kern}: no pole_side case")
        for fill in (False, True):  # the TX and IPv4 field modes, read-only and in place where the kernel runs them
            if any(c["mode"] in K.TX_POLE and c["fill"] == fill for c in mine) and \
                    not any(c["kind"] == "pole_data" and c["mode"] in K.TX_POLE and c["fill"] == fill for c in mine):
                missing.append(f"{kern}: no {'in-place' if fill else 'read-only'} pole_data case")
        # all-zero and all-0xFF packets in place (the datagram modes are outside the pole kinds); ICMP where taken
        for form in sorted({K.kernel_of(c)[1] for c in mine if c["fill"] and c["mode"] not in K.DGRAM}):
            key = [c for c in mine if c["fill"] and K.kernel_of(c)[1] == form]
            icmp = any(c["mode"] == "icmp" for c in key)
            for kind in ("zero", "ff"):
                if not any(c["kind"] == kind and (c["mode"] == "icmp" or not icmp) for c in key):
                    missing.append(f"{kern} {form}: no in-place {kind} case{' in ICMP' if icmp else ''}")
    return missing


def test_every_kernel_in_every_call_shape():
    assert not missing_call_shapes(), "\n".join(missing_call_shapes())


def test_every_kernel_on_its_zero_poles():
    assert not missing_poles(), "\n".join(missing_poles())


def test_k_iov_cases():
    """Layout "I": every view shape at the counts 1, 2, 37 and n_wrap, under the default
    set and one YU_NT trio."""
    mine = [c for c in K.CASES if c["layout"] == "I"]
    assert 40 <= len(mine) <= 50
    assert {c["iov"] for c in mine} == set(K.IOV_SHAPES)
    for shape in K.IOV_SHAPES:
        assert {1, 2, 37, "n_wrap"} <= {c["n"] for c in mine if c["iov"] == shape}, shape
    assert all(set(c["plans"]) in ({0, *K.RUNS0}, set(K.RUNS0)) for c in mine)
    assert {c["mode"] for c in mine} == set(K.IOV_MODES) and {c["mode"] for c in mine if c["fill"]} == set(K.FILL3)


def test_the_rules_name_a_missing_case():
    """The rules above fail, naming the kernel, when one appended case is taken away."""
    def without(pred):
        return [c for c in K.CASES if not pred(c)]

    def of(kern, c):
        return K.kernel_of(c)[0] == kern
    got = missing_call_shapes(without(lambda c: of("k_lane<5>", c) and "null_out" in K.calls(c)))
    assert got == ["k_lane<5> plain: no null_out case", "k_lane<5>: no null_out case across a second pass (n_wrap)"], got
    got = missing_call_shapes(without(lambda c: of("k_seg<8,dg,c40>", c) and c["call"] == "offset"))
    assert got and all(m.startswith("k_seg<8,dg,c40>:") for m in got), got
    got = missing_call_shapes(without(lambda c: of("k_loop<4,BE>", c) and c["call"] == "ignored"))
    assert got == ["k_loop<4,BE>: no ignored case"], got
    got = missing_poles(without(lambda c: of("k_iov<4>", c) and c["kind"] == "pole_side"))
    assert got == ["k_iov<4>: no pole_side case"], got
    got = missing_poles(without(lambda c: of("k_seg<8,txw,c48>", c) and c["kind"] == "pole_data"))
    assert got == ["k_seg<8,txw,c48>: no in-place pole_data case"], got
    got = missing_poles(without(lambda c: of("k_tiny<4>", c) and c["kind"] == "ff"))
    assert got == ["k_tiny<4> fill: no in-place ff case in ICMP"], got


# ---------------------------------------------------------------------------
# The child's comparisons can fail (no GPU: the "got" arrays are made here)
# ---------------------------------------------------------------------------
def test_the_childs_comparisons_fail_on_wrong_results():
    import ledger_child as C
    from oracle import oracle as O
    case = next(c for c in K.CASES if c["kind"] == "pole_side" and c["layout"] == "U" and c["mode"] in K.TX_POLE)
    s = next(iter(case["plans"]))
    P = C.prepare(case, s, 256, O.C())
    assert not isinstance(P, str), P
    assert (P.want == 0x0000).all() and P.want.size == P.n  # every packet on the TX pole
    lo = C.OUT_GUARD + 1
    good = np.concatenate((np.full(lo, C.OUT_FILL, np.uint16), P.want, np.full(C.OUT_GUARD, C.OUT_FILL, np.uint16)))
    assert C.check_out(good, lo, P.want) is None
    flipped = good.copy()
    flipped[lo + 5] ^= 0xFFFF  # the other representation of zero
    assert "1 results differ, first at [5]: got [65535] want [0]" in C.check_out(flipped, lo, P.want)
    front = good.copy()
    front[lo - 1] = 0
    assert "guard entries before the results changed: [%d]" % (lo - 1) in C.check_out(front, lo, P.want)
    back = good.copy()
    back[-1] ^= 1
    assert "guard entries after the results changed" in C.check_out(back, lo, P.want)
    # RAW and the VERIFY modes sit at the other pole
    case = next(c for c in K.CASES if c["kind"] == "pole_side" and c["mode"] not in K.TX_POLE and c["n"] == 37)
    P = C.prepare(case, next(iter(case["plans"])), 256, O.C())
    assert (P.want == 0xFFFF).all()
    wrong = np.concatenate((np.full(lo, C.OUT_FILL, np.uint16), P.want, np.full(C.OUT_GUARD, C.OUT_FILL, np.uint16)))
    wrong[lo] = 0x0000
    assert "got [0] want [65535]" in C.check_out(wrong, lo, P.want)
    # the packet memory: one byte off, inside the packets or in a guard
    exp = C.expected_memory(case, P)
    after = (exp if P.lay is None else exp[0]).copy()
    after[3] ^= 0x80
    assert "1 bytes differ" in C.check_memory(after, exp if P.lay is None else exp[0])


# ---------------------------------------------------------------------------
# k_seg's seams (tests/seg_seams.py): the seam cases hold what they are there for. The
# generator's parameters, for which the conditions below hold: K.seam_per (classes planted
# per chunk: 1 from 1000 chunks, 3 from 200, 6 below), the six chunk slots of
# seg_seams.batch, and base 3 (not 1) for the 24-chunk cases of the YU_RAGGED=seg4 kinds.
# ---------------------------------------------------------------------------
def seam_setup(case):
    ch, t, kind = K.seg_shape(K.kernel_of(case)[0])
    return ch, t, kind, kind == "txw" and case["fill"] and case["layout"] == "R"


@pytest.fixture(scope="module")
def seams():
    """Every ragged seam case rebuilt as the child builds it (prepare, its seed): the
    class counts, the chunk starts' residues, the planted datagrams, the buffer's size."""
    import ledger_child as C
    import seg_seams as S
    from oracle import oracle as O
    oracle = O.C()
    found = {}
    for c in K.CASES:
        if not K.is_seam(c):
            continue
        ch, t, kind, line128 = seam_setup(c)
        s = next(iter(c["plans"]))
        P = C.prepare(c, s, 256, oracle)
        assert not isinstance(P, str), (c["id"], P)
        b = S.batch(ch, t, c["mode"], line128, c["base"], S.classes_for(kind, c["mode"], line128), P.n,
                    np.random.default_rng(P.index * 16 + s))
        assert np.array_equal(b.lens, P.ends - P.starts), c["id"]  # the same batch
        found[c["id"]] = dict(case=c, P=P, planted=b.planted, residues=b.residues, size=P.buf.size,
                              classes=S.classes_for(kind, c["mode"], line128),
                              counts=S.features(P.starts, P.ends, ch, t, line128, c["mode"], P.buf, data=C.GUARD))
    return found


def test_seam_cases_are_what_the_issue_lists():
    """One case or more per k_seg key of the ragged tables (kernel x in place, every mode of
    the per-packet kinds) at base 0 and at 1 or 3, one knob set each, none on a pole; at most
    24 MiB each; no case before them changed."""
    mine = [c for c in K.CASES[K.N_BEFORE_SEAMS:]]
    assert all(K.kernel_of(c)[0].startswith("k_seg") and len(c["plans"]) == 1 and c["kind"] == "rand" and
               c["call"] == "plain" for c in mine)
    ragged = [c for c in mine if K.is_seam(c)]
    assert not any(K.is_seam(c) for c in K.CASES[:K.N_BEFORE_SEAMS]) and all(c["layout"] == "U" for c in mine if c not in ragged)
    want = {(K.kernel_of(c)[0], c["fill"], c["mode"]) for c in K.CASES[:K.N_BASE]
            if c["layout"] == "R" and K.kernel_of(c)[0].startswith("k_seg")}
    got = {}
    for c in ragged:
        got.setdefault((K.kernel_of(c)[0], c["fill"], c["mode"]), []).append(c["base"])
        assert c["gen"][1:] == K.seg_shape(K.kernel_of(c)[0])[:2], c["id"]
        s = next(iter(c["plans"]))
        seg4 = K.KNOB_SETS[s].get("YU_RAGGED") == "seg4"
        assert c["n"] == (1537 if seg4 else K.MID_BATCH + 1 if c["n_lo"] == K.MID_BATCH else 4097), c["id"]
        assert K.case_bytes(c, c["n"]) <= K.SEAM_MAX_BYTES, c["id"]
    assert set(got) == want
    assert all(sorted(b)[0] == 0 and sorted(b)[1] in (1, 3) and len(b) == 2 for b in got.values()), got
    for c in mine:
        if c["layout"] == "U":
            assert K.case_bytes(c, c["n"]) <= 44 << 20 and c["stride"] == c["len"] and c["base"] == 0, c["id"]


def test_seam_cases_hold_every_class_of_their_kind(seams):
    """Every class seg_seams lists for the kind, 4 times or more, per start parity where
    the class leaves the parity free (seg_seams.wanted says which, and why a chunk's end
    counts 4 in all); exact: 1 to 8 chunks."""
    import seg_seams as S
    wrong = []
    for cid, f in seams.items():
        wrong += [f"{cid}: {m}" for m in S.missing(f["counts"], f["classes"])]
        if "exact" in f["classes"] and f["counts"][("exact", 0)] + f["counts"][("exact", 1)] > 8:
            wrong.append(f"{cid}: more than 8 exact chunks")
        assert f["size"] <= K.case_bytes(f["case"], f["P"].n) + 2 * 128 <= K.SEAM_MAX_BYTES + 256, cid
    assert not wrong, "\n".join(wrong[:40])
    kinds = {K.seg_shape(K.kernel_of(f["case"])[0])[2] for f in seams.values()}
    assert kinds == {"plain", "tx", "txw", "rx", "dg"}


def test_seam_cases_start_half_of_their_chunks_on_a_line(seams):
    import seg_seams as S
    for cid, f in seams.items():
        r = f["residues"]
        assert np.count_nonzero(r == 0) * 2 >= r.size, (cid, np.count_nonzero(r == 0), r.size)
        assert set(S.RESIDUES) <= set(r.tolist()), (cid, sorted(set(r.tolist())))


def test_planted_datagrams_are_in_contract(seams):
    """From the bytes: 20 <= hl <= tl <= len for every datagram a class was planted with
    (short_hdr is the class of IHL 0..4: outside it by design), and where the class needs a
    transport field, protocol 1, 6 or 17 with the segment holding its header."""
    seen = 0
    for cid, f in seams.items():
        P = f["P"]
        for i, cl in f["planted"]:
            if cl == "short_hdr":
                continue
            a, ln = int(P.starts[i]), int(P.ends[i] - P.starts[i])
            hl, tl, proto = (int(P.buf[a]) & 15) * 4, (int(P.buf[a + 2]) << 8) | int(P.buf[a + 3]), int(P.buf[a + 9])
            assert 20 <= hl <= tl <= ln, (cid, i, cl, hl, tl, ln)
            if cl.startswith("l4field"):
                assert proto in (1, 6, 17) and tl - hl >= {1: 4, 6: 20, 17: 8}[proto], (cid, i, cl, proto, tl - hl)
            seen += 1
    assert seen > 1000


def test_the_class_counts_name_a_dropped_class():
    """A generator that leaves one class out is named by the count check (not RAW's start@d: its 2-byte packets behind
    one planted start make the next)."""
    import seg_seams as S
    for mode, kind, line128, drop in (("udp", "tx", False, "field@-1"), ("tx_datagram", "dg", False, "l4field@-2"),
                                      ("verify_udp", "plain", False, "start@2"), ("tcp", "txw", True, "field@0")):
        full = S.classes_for(kind, mode, line128)
        b = S.batch(64, 4096, mode, line128, 0, [c for c in full if c != drop], 1537, np.random.default_rng(5))
        offs = np.concatenate(([128], 128 + np.cumsum(b.lens)))
        buf = np.zeros(int(offs[-1]), np.uint8)
        if b.parts is not None:
            buf[128:] = np.concatenate(b.parts)
        got = S.missing(S.features(offs[:-1], offs[1:], 64, 4096, line128, mode, buf, data=128), full)
        assert got and all(m.startswith(drop) for m in got), (drop, got)


def seam_table(seams):
    """Per k_seg key (kernel, in place, layout) over the seam cases: chunks, chunk ends on a
    seam, interior packet starts on a seam, fields across a seam (TX: field@-1, DG: l4field@-1)."""
    import seg_seams as S
    rows = {}
    for c in K.CASES[K.N_BEFORE_SEAMS:]:
        ch, t, kind, line128 = seam_setup(c)
        if K.is_seam(c):
            counts, n = seams[c["id"]]["counts"], seams[c["id"]]["P"].n
        else:
            n = c["n"]
            starts = c["base"] + c["stride"] * np.arange(n, dtype=np.int64)
            counts = S.features(starts, starts + c["len"], ch, t, False, c["mode"], data=c["base"])
        row = rows.setdefault((K.kernel_of(c)[0], c["fill"], c["layout"]), [0, 0, 0, 0, False])
        both = lambda cl: counts[(cl, 0)] + counts[(cl, 1)]  # noqa: E731
        row[0] += -(-n // ch)
        row[1] += both("chunk_end@0")
        row[2] += both("start@0")
        row[3] += both("field@-1") + both("l4field@-1")
        row[4] |= both("chunk_end@0") > 0 and both("start@0") > 0
    return rows


def test_every_k_seg_key_has_a_case_on_the_seams(seams, reachable):
    """Every k_seg key the planner can reach, uniform ones included, has a case with a chunk
    that ends on a seam and an interior packet that starts on one; the uniform TX shapes
    put a field across a seam (in place: on one) in every chunk."""
    import seg_seams as S
    rows = seam_table(seams)
    keys = {(k[0], k[3] == "1", k[4]) for k in reachable[0] if k[0].startswith("k_seg")}
    assert keys == {k for k in case_keys_of_layouts() if k[0].startswith("k_seg")}
    lacking = sorted(k for k in keys if not rows.get(k, [0, 0, 0, 0, False])[4])
    assert not lacking, lacking
    for k, row in sorted(rows.items()):
        print("%-18s %-8s %s: %6d chunks, %6d chunk ends, %6d starts, %5d fields across a seam" % (
            k[0], "in place" if k[1] else "", k[2], *row[:4]))
    for c in K.CASES[K.N_BEFORE_SEAMS:]:
        if c["layout"] == "U" and c["len"] in (141, 327, 431, 545, 272):
            ch, t, _, _ = seam_setup(c)
            starts = c["stride"] * np.arange(c["n"], dtype=np.int64)
            f = S.features(starts, starts + c["len"], ch, t, False, c["mode"])
            cl = "field@0" if c["fill"] else "field@-1"
            assert f[(cl, 0)] + f[(cl, 1)] >= c["n"] // ch, (c["id"], f)


def case_keys_of_layouts():
    return {(K.kernel_of(c)[0], c["fill"], c["layout"]) for c in K.CASES}
