"""The kernel ledger on the GPU: one child process (tests/ledger_child.py) per knob set
of tests/kernel_cases.py, one after another. The library reads its knobs once, so each
set needs a process of its own; the default set runs with no knob and no YU_TUNING. A
child that ends by a signal, at its time limit or with a HIP error stops the rest: the
later sets fail at once without starting a process."""
import os
import re
import subprocess
import sys

import pytest

import kernel_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "ledger_child.py")
_stopped = []  # why no further child may start


@pytest.mark.parametrize("s", range(len(K.KNOB_SETS)))
def test_ledger_cases_match_the_oracle(dev, s):
    assert not _stopped, f"not started: {_stopped[0]}"
    env = {k: v for k, v in os.environ.items() if not k.startswith("YU_")}
    if s:
        env.update(K.KNOB_SETS[s], YU_TUNING="1")
    try:
        r = subprocess.run([sys.executable, CHILD, str(s)], env=env, capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        _stopped.append(f"the child of set {s} ran into its time limit")
        raise
    tail = "\n".join(r.stdout.splitlines()[-4:]) + "\n" + r.stderr[-3000:]
    # (a YuError status below YU_EHIP_BASE = -1000 is a HIP error code)
    if r.returncode < 0 or r.returncode in (134, 139) or re.search(r"HIP error|hipError|status -1\d\d\d", tail):
        _stopped.append(f"the child of set {s} ended with {r.returncode}: {tail[-500:]}")
    assert r.returncode == 0, tail
    cases = sum(1 for c in K.CASES if s in c["plans"])
    lines = r.stdout.splitlines()
    assert sum(1 for line in lines if line.startswith("ok ")) == cases, tail
    print(lines[-1])  # "ledger set <s>: <cases> cases in <seconds> s"
