"""yu::plan_group (yustack_amd/csrc/yucsum_plan.h) for the tests of yu_rx_group:
tests/cpp/group_plan.cpp, built once into tests/cpp/build/ (again when a source is
newer) and run under a given environment. A plain module, like demux_plan.py."""
import os
import subprocess
from collections import namedtuple

from test_plan import CSRC, HIP_HEADERS, ROOT

SOURCES = [os.path.join(ROOT, "tests", "cpp", "group_plan.cpp"), os.path.join(CSRC, "yucsum_plan.cpp")]
HEADERS = [os.path.join(CSRC, h) for h in ("yucsum_plan.h", "yucsum_internal.h", "yucsum_iov.h", "yucsum_group.h")]
BIN = os.path.join(ROOT, "tests", "cpp", "build", "group_plan")

Plan = namedtuple("Plan", "digit_bits passes tile blocks lane_blocks hist sums count pair0 pair1 bytes name")


def binary():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in SOURCES + HEADERS):
        r = subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT}/include", *HIP_HEADERS, *SOURCES, "-o", BIN],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    return BIN


def plans(cases, env=None):
    """One Plan per (n, m, cus) case; a region is (offset, bytes). `env`: the YU_
    variables the printer sees (none else)."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("YU_")}
    e.update(env or {})
    r = subprocess.run([binary(), *[str(x) for c in cases for x in c]], capture_output=True, text=True, timeout=60,
                       env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [line.split(maxsplit=16) for line in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    out = []
    for row in rows:
        v = [int(x) for x in row[:16]]
        out.append(Plan(*v[:5], *[(v[5 + 2 * k], v[6 + 2 * k]) for k in range(5)], v[15], row[16]))
    return out
