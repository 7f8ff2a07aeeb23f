"""The whole-datagram kind of k_iov (yustack_amd/csrc/yucsum_iov.h: IPV4, VERIFY_IPV4,
VERIFY_RX and TX_DATAGRAM on scatter-gather packets) on a CPU: tests/cpp/iov_datagram.cpp
drives the header gather, the parse, the lanes' header sums, the windowed view walk,
the load slots, the two parity classes, the field bytes and the epilogue as the kernel
does, for datagrams of 0..96 bytes (IHL 0..15, TotalLength from HL - 1 to len + 1,
protocols 1, 6, 17, 47; random, all 0x00, all 0xFF) in every split into 1..4 views up to
40 bytes and cycling splits above, against a byte-wise composition with the scalar
library over the concatenated bytes. The header makes no HIP call, so a plain g++
compiles it; the same program also runs under AddressSanitizer + UBSan (host code with
its own main)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "iov_datagram.cpp"),
           os.path.join(ROOT, "yustack_amd", "csrc", "yucsum_scalar.cpp")]
INC = [f"-I{ROOT}/include", f"-I{ROOT}/yustack_amd/csrc"]


def _build_and_run(tmp_path, name, flags, env=None):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, *INC, *SOURCES, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("packets ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert int(r.stdout.split()[0]) > 2_000_000


def test_iov_datagram(tmp_path):
    _build_and_run(tmp_path, "iov_datagram", ["-O2"])


def test_iov_datagram_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "iov_datagram_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer"],
                   env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
