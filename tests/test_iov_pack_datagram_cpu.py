"""k_pack_dg on a CPU (yustack_amd/csrc/yucsum_iov.h + yucsum_iov_pack.h):
tests/cpp/iov_pack_datagram.cpp drives the header gather, the parse, the plain walk,
the window-masked sums, the destination geometry and the four held-back bytes as the
kernel does (steps of 4 slots, 64 lanes of 16 bytes, neighbour dwords as the kernel
takes them) into exact-size blocks between canaries, and counts the stores per byte:
the copy is every byte of the packet whatever its header says (the fields patched in
fill), no byte is stored twice, no slack byte or canary is touched, no store is
misaligned, and the results are the byte-wise scalar composition's. Datagrams of
0..96 bytes x IHL 0..15 x TL from HL-1 to len+1 x protocols 1, 6, 17, 47 x three
payloads, 1..4 views at every source address mod 4 and destination start mod 16,
slack 0 and 5, fill on and off, the 1024-byte slot seam, and the out-of-contract
rooms.

The headers make no HIP call, so a plain g++ compiles the program; the same program
(with its own main, run as that program only) also runs under AddressSanitizer +
UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "iov_pack_datagram.cpp"),
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


def test_iov_pack_datagram(tmp_path):
    assert _build_and_run(tmp_path, "iov_pack_datagram", ["-O2"]) > 3000000


def test_iov_pack_datagram_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "iov_pack_datagram_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer"],
                   env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))


def test_the_sibling_programs_still_compile_against_the_headers(tmp_path):
    """yucsum_iov.h and yucsum_iov_pack.h grew by addition only: the programs of the
    earlier kernels compile against them unchanged."""
    for src in ("iov_combine.cpp", "iov_datagram.cpp", "iov_pack.cpp"):
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-fsyntax-only", *INC,
                            os.path.join(ROOT, "tests", "cpp", src)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (src, r.stderr[-3000:])
