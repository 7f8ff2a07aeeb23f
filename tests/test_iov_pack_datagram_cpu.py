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
from cpp_program import build_and_run, models_compile


def test_iov_pack_datagram(tmp_path):
    assert build_and_run(tmp_path, "iov_pack_datagram") > 3000000


def test_iov_pack_datagram_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "iov_pack_datagram", sanitize=True)


def test_the_sibling_programs_still_compile_against_the_headers(tmp_path):
    """yucsum_iov.h and yucsum_iov_pack.h grew by addition only: the programs of the
    earlier kernels compile against them unchanged."""
    models_compile()
