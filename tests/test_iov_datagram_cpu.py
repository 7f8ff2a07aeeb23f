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
from cpp_program import build_and_run


def test_iov_datagram(tmp_path):
    assert build_and_run(tmp_path, "iov_datagram") > 2_000_000


def test_iov_datagram_under_sanitizers(tmp_path):
    assert build_and_run(tmp_path, "iov_datagram", sanitize=True) > 2_000_000
