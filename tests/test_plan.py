"""The launch plan (yustack_amd/csrc/yucsum_plan.h): which kernel, form, load policy,
grid, packets per wave, uf, small_waves and block order every batch shape gets.
tests/cpp/plan_table.cpp prints the plan of a fixed case list; tests/golden/launch_plans.txt
holds the decisions the library made before the planner existed (recorded from its old
launch code), so a changed line is a changed decision and needs a measurement. CPU only."""
import os
import subprocess

import pytest

from test_cpp import SAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yustack_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cpp", "plan_table.cpp"), os.path.join(CSRC, "yucsum_plan.cpp")]
HEADERS = [os.path.join(CSRC, "yucsum_plan.h"), os.path.join(CSRC, "yucsum_internal.h")]
BIN = os.path.join(ROOT, "tests", "cpp", "build", "plan_table")
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.txt")
# yucsum_internal.h includes hip/hip_runtime.h for its __host__ __device__ tables
HIP_HEADERS = ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{CSRC}"]


def _compare(binary, env=None):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    got, want = r.stdout.splitlines(), open(GOLDEN).read().splitlines()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch_plans.txt:{k + 1}: the plan changed"
    assert len(got) == len(want)
    return got


@pytest.fixture(scope="module")
def binary():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in SOURCES + HEADERS):
        r = subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT}/include", *HIP_HEADERS, *SOURCES, "-o", BIN],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    return BIN


def test_launch_plans_match_the_record(binary):
    got = _compare(binary)
    cases = [line for line in got if not line.startswith("#")]
    assert len(cases) > 2000 and os.path.getsize(GOLDEN) < 1 << 20
    # every kernel of the list (YU_KERNELS: 39) is planned somewhere in the table
    names = {line.split(" | ")[1].split()[0] for line in cases}
    assert len(names) == 39, sorted(names)


def test_launch_plans_under_sanitizers(tmp_path):
    """The planner under AddressSanitizer + UBSan (a stand-alone host program)."""
    san = str(tmp_path / "plan_table_san")
    r = subprocess.run(["g++", *SAN, *HIP_HEADERS, *SOURCES, "-o", san], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    _compare(san, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
