"""yu::plan_wave (yustack_amd/csrc/yucsum_plan.h) for the tests of the wave-per-packet
calls: tests/cpp/wave_plan.cpp, built once into tests/cpp/build/ (again when a source
is newer) and run under a given environment. A plain module, like iov_layout.py."""
import os
import subprocess

from test_plan import CSRC, HIP_HEADERS, ROOT

SOURCES = [os.path.join(ROOT, "tests", "cpp", "wave_plan.cpp"), os.path.join(CSRC, "yucsum_plan.cpp")]
HEADERS = [os.path.join(CSRC, h) for h in ("yucsum_plan.h", "yucsum_internal.h", "yucsum_iov.h")]
BIN = os.path.join(ROOT, "tests", "cpp", "build", "wave_plan")


def binary():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in SOURCES + HEADERS):
        r = subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT}/include", *HIP_HEADERS, *SOURCES, "-o", BIN],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    return BIN


def run(args, env=None):
    """The printer's output lines for `args`; `env`: the YU_ variables it sees (none else)."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("YU_")}
    e.update(env or {})
    out = []
    for i in range(0, len(args), 2500):  # whole quintuples
        r = subprocess.run([binary(), *[str(x) for x in args[i:i + 2500]]], capture_output=True, text=True,
                           timeout=60, env=e)
        assert r.returncode == 0, r.stderr[-2000:]
        out += r.stdout.splitlines()
    return out


def plans(family, cases, env=None):
    """[(kernel, policy, blocks, name)] for the (n, mode, fill, cus) cases of a family."""
    rows = [line.split(maxsplit=3) for line in run([x for c in cases for x in (family, *c)], env)]
    assert len(rows) == len(cases)
    return [(int(k), int(pol), int(blocks), name) for k, pol, blocks, name in rows]


def pack_and_iov(cases, env=None):
    """[(the packing plan, the in-place calls' plan)] for the same (n, mode, fill, cus) cases."""
    return list(zip(plans("pack", cases, env), plans("iov", cases, env)))


def enum():
    """The yu::WaveKernel enumerators in order, then their count."""
    (line,) = run(["enum"])
    return [int(x) for x in line.split()[1:]]
