"""yu_rx_stream on a CPU (yustack_amd/csrc/yucsum_stream.h): tests/cpp/rx_stream.cpp runs
k_stream's walk, yu::stream_endpoint, in wave steps of 64 lanes as the kernel runs it, once
with the run test and once with it forced off, then the kernel's own stores, the second
launch and the two sums, on heap blocks of the exact sizes with every index checked, against
a direct one-segment-at-a-time loop with its heap in a std::vector.

One endpoint: 26 cases (in order, an adjacent swap, a gap never filled, a gap filled by the
last segment, duplicates, overlaps that need a trim, an overshoot of rcv_acc, a zero window
that stays shut and one that reopens, FIN in order, FIN parked and reached, a parked FIN
without data, data after FIN, RST in the middle, a missing ACK flag, pure ACKs on and off
rcv_nxt, doff 32, sequence numbers that wrap, a full byte budget, a full cap, state 0, 2 and
3 at entry, a carried heap, a shuffle, records that are not TCP) x queue lengths 0, 1, 2, 63,
64, 65, 130 x cap 0, 1, 4; then m = 0, 1, 3, 70 endpoints x cap x three rounds with the cases
dealt round and packets of no endpoint mixed in. The program itself checks that the grid
reached every verdict, took runs and left segments parked.

The header makes no HIP call, so a plain g++ compiles the program; the same program (with
its own main, run as that program only) also runs under AddressSanitizer + UBSan."""
from cpp_program import build_and_run

TOTAL = 26 * 7 * 3 + 4 * 3 * 3


def test_rx_stream(tmp_path):
    assert build_and_run(tmp_path, "rx_stream", sources=(), ends="cases ok") == TOTAL


def test_rx_stream_under_sanitizers(tmp_path):
    assert build_and_run(tmp_path, "rx_stream", sources=(), sanitize=True, ends="cases ok") == TOTAL
