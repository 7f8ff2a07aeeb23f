"""k_iov's arithmetic (yustack_amd/csrc/yucsum_iov.h) on a CPU: tests/cpp/iov_combine.cpp
drives the view walk, the load slots, the masked sums, the two parity classes, the
field bytes and the epilogue as the kernel does, for packets of 0..64 bytes in every
split into 1..4 views at every address mod 4 (random, all 0x00, all 0xFF; initial 0
and 0xFFFF), against the scalar library's composition over the concatenated bytes.
The header makes no HIP call, so a plain g++ compiles it; the same program also runs
under AddressSanitizer + UBSan (host code with its own main)."""
from cpp_program import build_and_run


def test_iov_combine(tmp_path):
    assert build_and_run(tmp_path, "iov_combine") > 1_000_000


def test_iov_combine_under_sanitizers(tmp_path):
    assert build_and_run(tmp_path, "iov_combine", sanitize=True) > 1_000_000
