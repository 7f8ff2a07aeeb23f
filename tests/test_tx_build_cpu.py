"""k_build on a CPU (yustack_amd/csrc/yucsum_build.h + yucsum_iov.h + yucsum_iov_pack.h):
tests/cpp/tx_build.cpp drives the header encode, the three header sums, the value
composition, the contract test, the single-view walk and the destination geometry as
the kernel does (steps of 4 slots, 64 lanes of 16 bytes, neighbour dwords as the kernel
takes them, the header stored last by lanes 0..10) into exact-size blocks between
canaries, and counts the stores per byte: the image is the one assembled byte by byte
with the scalar library's yu_checksum, every in-room byte is stored exactly once, and
no byte outside the packet's span is stored. Every L in 0..96 and 1016..1032 x payload
address mod 4 x destination mod 4 x UDP, ICMP, protocol 47, TCP with doff 20, 24 and 60
x room exact, slack 1..5 and short by 1..45; then the device test's contract batch.

The headers make no HIP call, so a plain g++ compiles the program; the same program
(with its own main, run as that program only) also runs under AddressSanitizer +
UBSan."""
from cpp_program import build_and_run, models_compile


def test_tx_build(tmp_path):
    # 114 lengths x 6 kinds x 16 phase pairs x 51 rooms, and the all-0x00 / all-0xFF runs
    assert build_and_run(tmp_path, "tx_build") > 550000


def test_tx_build_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "tx_build", sanitize=True)


def test_the_sibling_programs_still_compile_against_the_headers(tmp_path):
    """yucsum_iov.h and yucsum_iov_pack.h are used as they are (yucsum_build.h only adds
    beside them): the programs of the earlier kernels compile against them unchanged."""
    models_compile()
