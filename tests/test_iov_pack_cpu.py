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
from cpp_program import build_and_run


def test_iov_pack(tmp_path):
    assert build_and_run(tmp_path, "iov_pack") > 500000


def test_iov_pack_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "iov_pack", sanitize=True)
