"""k_build_iov ("k_build<4,iov>", yu_tx_build_iov) on a CPU: tests/cpp/tx_build_iov.cpp is
tests/cpp/tx_build.cpp's model of k_build fed from views, compared byte for byte (and store
for store) with that contiguous model: payload byte phases 0..3 x destination byte phases
0..3 x L in {0..5, 1019..1025, 4091..4097, 65507 (UDP: T = 65535), 65508 (over the limit)}
x UDP, ICMP, TCP and protocol 47. Every batch has skipped packets (an empty destination
span) between the built ones, one with a view that must not be dereferenced and one with
{NULL, 0}, and two packets naming one view.

The headers make no HIP call, so a plain g++ compiles the program; the same program (with
its own main, run as that program only) also runs under AddressSanitizer + UBSan."""
from cpp_program import build_and_run

LENGTHS = 6 + 7 + 7 + 2
PROTOCOLS = 4
PHASES = 4 * 4
ENTRIES = 4  # per batch: built, skipped, built from the same view, skipped
TOTAL = LENGTHS * PROTOCOLS * PHASES * ENTRIES


def test_tx_build_iov(tmp_path):
    assert build_and_run(tmp_path, "tx_build_iov") == TOTAL


def test_tx_build_iov_under_sanitizers(tmp_path):
    assert build_and_run(tmp_path, "tx_build_iov", sanitize=True) == TOTAL
