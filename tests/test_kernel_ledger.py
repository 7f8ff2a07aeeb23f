"""The kernel ledger (tests/kernel_cases.py) against the planner, on the CPU: every
case's written plan is the planner's at 64, 256 and 304 CUs, the built library names the
same kernel, and the cases cover every key (kernel, form, policy, in place, layout) the
planner can return (tests/cpp/plan_query.cpp --reachable). tests/test_gpu_kernel_ledger.py
runs the same cases on the GPU."""
import os
import subprocess
import sys

import pytest

import kernel_cases as K
from test_plan import CSRC, HIP_HEADERS, ROOT

SOURCES = [os.path.join(ROOT, "tests", "cpp", "plan_query.cpp"), os.path.join(CSRC, "yucsum_plan.cpp")]
HEADERS = [os.path.join(ROOT, "tests", "cpp", "plan_rows.h"), os.path.join(CSRC, "yucsum_plan.h"),
           os.path.join(CSRC, "yucsum_internal.h")]
BIN = os.path.join(ROOT, "tests", "cpp", "build", "plan_query")
KERNELS = 39


@pytest.fixture(scope="module")
def query():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in SOURCES + HEADERS):
        r = subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT}/include", *HIP_HEADERS, *SOURCES, "-o", BIN],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    return BIN


@pytest.fixture(scope="module")
def reachable(query):
    r = subprocess.run([query, "--reachable"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [tuple(line.split()) for line in r.stdout.splitlines()]
    keys = {ln[1:] for ln in lines if ln[0] == "K"}
    defaults = {ln[1:] for ln in lines if ln[0] == "D"}
    assert len(keys) > 200 and len(defaults) > 100 and len({k[0] for k in keys}) == KERNELS
    return keys, defaults


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


def test_cases_are_well_formed():
    assert len({c["id"] for c in K.CASES}) == len(K.CASES)
    for c in K.CASES:
        assert c["plans"] and all(0 <= s < len(K.KNOB_SETS) for s in c["plans"]), c["id"]
        assert c["mode"] in K.MODES and c["side"] in K.SIDES.get(c["mode"], ("scalar",)), c["id"]
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


def test_written_plans_are_the_planners(query):
    """Kernel, form and policy of every case under every set it runs in, at three CU
    counts (only `blocks` may differ between cards); ppw where the case states it."""
    text, want = [], []
    for s, env in enumerate(K.KNOB_SETS):
        text.append("# knobs: " + " ".join(f"{k}={v}" for k, v in env.items()))
        for c in K.CASES:
            if s in c["plans"]:
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
    assert len(kernels) == KERNELS, kernels
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
    assert len(by_kernel) == KERNELS
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
