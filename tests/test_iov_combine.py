"""k_iov's arithmetic (yustack_amd/csrc/yucsum_iov.h) on a CPU: tests/cpp/iov_combine.cpp
drives the view walk, the load slots, the masked sums, the two parity classes, the
field bytes and the epilogue as the kernel does, for packets of 0..64 bytes in every
split into 1..4 views at every address mod 4 (random, all 0x00, all 0xFF; initial 0
and 0xFFFF), against the scalar library's composition over the concatenated bytes.
The header makes no HIP call, so a plain g++ compiles it; the same program also runs
under AddressSanitizer + UBSan (host code with its own main)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "iov_combine.cpp"),
           os.path.join(ROOT, "yustack_amd", "csrc", "yucsum_scalar.cpp")]
INC = [f"-I{ROOT}/include", f"-I{ROOT}/yustack_amd/csrc"]


def _build_and_run(tmp_path, name, flags, env=None):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, *INC, *SOURCES, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("packets ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert int(r.stdout.split()[0]) > 1_000_000


def test_iov_combine(tmp_path):
    _build_and_run(tmp_path, "iov_combine", ["-O2"])


def test_iov_combine_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "iov_combine_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer"],
                   env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
