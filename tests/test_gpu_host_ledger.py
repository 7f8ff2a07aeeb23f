"""The host ledger on the GPU: one child process (tests/host_child.py) per knob set of
tests/host_cases.py, one after another. The library reads its knobs once, so each set
needs a process of its own; the first set runs with no knob and no YU_TUNING, the shipped
constants. A child that ends by a signal, at its time limit or with a HIP error stops the
rest: the later sets fail at once without starting a process. For the tuned sets the
library's gate must have named every knob on stderr ("yucsum: tuning knob ..."): a knob
that was not read would leave the shipped cut in place."""
import os
import re
import subprocess
import sys

import pytest

import host_cases as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "host_child.py")
_stopped = []  # why no further child may start


@pytest.mark.parametrize("s", range(len(H.KNOB_SETS)))
def test_host_cases_match_the_oracle_and_the_model(dev, s):
    assert not _stopped, f"not started: {_stopped[0]}"
    env = {k: v for k, v in os.environ.items() if not k.startswith("YU_")}
    if s:
        env.update(H.KNOB_SETS[s], YU_TUNING="1")
    try:
        r = subprocess.run([sys.executable, CHILD, str(s)], env=env, capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        _stopped.append(f"the child of set {s} ran into its time limit")
        raise
    tail = "\n".join(r.stdout.splitlines()[-4:]) + "\n" + r.stderr[-3000:]
    # (a status below YU_EHIP_BASE = -1000 is a HIP error code)
    if r.returncode < 0 or r.returncode in (134, 139) or re.search(r"HIP error|hipError|status -1\d\d\d", tail):
        _stopped.append(f"the child of set {s} ended with {r.returncode}: {tail[-500:]}")
    assert r.returncode == 0, tail
    cases = sum(1 for c in H.CASES if c["set"] == s)
    lines = r.stdout.splitlines()
    assert sum(1 for line in lines if line.startswith("ok ")) == cases, tail
    for knob, value in H.KNOB_SETS[s].items():
        assert f"yucsum: tuning knob {knob}={value} " in r.stderr, (knob, r.stderr[-2000:])
    assert s or "tuning knob" not in r.stderr
    print("\n".join(lines[-2:]))  # the slowest case; "host ledger set <s>: <cases> cases in <seconds> s"
