"""k_small's dense fetch geometry (yustack_amd/csrc/yucsum_dense.h) on a CPU:
tests/cpp/dense_geom.cpp walks every step and lane of a set of dense batches and
checks what is loaded (inside the batch, each packet byte exactly once, whole
lines), where each group's window sits in the LDS slice, and which batches the
predicate admits. The header makes no HIP call, so a plain g++ compiles it; the
same program also runs under AddressSanitizer + UBSan (host code with its own
main)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dense_geom.cpp")
INC = f"-I{ROOT}/yustack_amd/csrc"


def _build_and_run(tmp_path, name, flags, env=None):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, INC, SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-3000:], r.stderr[-3000:])


def test_dense_geometry(tmp_path):
    _build_and_run(tmp_path, "dense_geom", ["-O2"])


def test_dense_geometry_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "dense_geom_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer"],
                   env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
