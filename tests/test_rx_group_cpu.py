"""The kernels of yu_rx_group on a CPU (yustack_amd/csrc/yucsum_group.h):
tests/cpp/rx_group.cpp runs each pass as the kernels do (a block per tile, four waves on
their quarters in 64-lane steps, the match-by-digit ballots as 64-bit words, the per-wave
digit counts combined as in LDS, the digit-major histogram) and the scan in its three
phases, on heap blocks of the exact sizes, every store index checked and counted, against
std::stable_sort, a count and a direct loop for the grouped views and their offsets.

The header makes no HIP call, so a plain g++ compiles the program; the same program (with
its own main, run as that program only) also runs under AddressSanitizer + UBSan."""
from cpp_program import build_and_run

NS = 10          # 0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 2 tile + 3, 9 tile - 27 (two scan tiles per histogram)
MS = 6           # 0, 1, 255, 256, 65535, 65536
PATTERNS = 6     # all equal, all none, distinct descending, top digit only, m / m + 1 / 0x7FFFFFFF mixed in, random
GROWN_TILE = 6   # a tile twice as large, the patterns again
FOUR_PASSES = 6  # m = 2^24 at n = 300
SCAN_ALONE = 1   # 600000 elements: the middle launch's threads take two tile sums each
TOTAL = NS * MS * PATTERNS + GROWN_TILE + FOUR_PASSES + SCAN_ALONE


def test_rx_group(tmp_path):
    assert build_and_run(tmp_path, "rx_group", sources=(), ends="cases ok") == TOTAL


def test_rx_group_under_sanitizers(tmp_path):
    assert build_and_run(tmp_path, "rx_group", sources=(), sanitize=True, ends="cases ok") == TOTAL
