"""k_pack on a CPU (yustack_amd/csrc/yucsum_iov.h + yucsum_iov_pack.h):
tests/cpp/iov_pack.cpp drives the walk, the slots, the sums and the destination
geometry as the kernel does (steps of 4 slots, 64 lanes of 16 bytes, neighbour
dwords as the kernel takes them) into exact-size blocks between canaries, and counts
the stores per byte: the copy equals the concatenation (the field patched in fill),
no byte is stored twice, no slack byte or canary is touched, the value is the scalar
library's composition. Packets of 0..64 and 1020..1030 bytes in 1..3 views, every
source address mod 4 x destination start mod 16, the six modes, fill on and off,
slack 0 and 5, 70 one-byte views, and the out-of-contract rooms.

The headers make no HIP call, so a plain g++ compiles the program; the same program
(with its own main, run as that program only) also runs under AddressSanitizer +
UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "iov_pack.cpp"),
           os.path.join(ROOT, "yustack_amd", "csrc", "yucsum_scalar.cpp")]
INC = [f"-I{ROOT}/include", f"-I{ROOT}/yustack_amd/csrc"]


def _build_and_run(tmp_path, name, flags, env=None):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, *INC, *SOURCES, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("packets ok"), (r.stdout[-3000:], r.stderr[-3000:])
    return int(r.stdout.split()[0])


def test_iov_pack(tmp_path):
    assert _build_and_run(tmp_path, "iov_pack", ["-O2"]) > 500000


def test_iov_pack_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "iov_pack_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer"],
                   env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
