"""k_demux on a CPU (yustack_amd/csrc/yucsum_demux.h): tests/cpp/rx_demux.cpp drives one
lane's work as the kernel does (eligibility, the three keys out of the record's dwords,
the hash, the probe chain with its bound, the clamp of an index to m) on tables
yu::demux_fill wrote, against a std::map restatement of deliverPacketLocked and the gate
of DeliverTransportPacket. Every probe is recorded: each is 16-byte aligned and inside
the table, and no lookup makes more than `slots` of them, also on a table without an
empty slot.

The header makes no HIP call, so a plain g++ compiles the program; the same program
(with its own main, run as that program only) also runs under AddressSanitizer + UBSan,
where the table's exact-size block turns a stray probe into a report."""
from cpp_program import build_and_run

SUBSETS = 8 * 4            # subsets of the three kinds x {the peer, another peer, another address, another port}
ZERO_REMOTE = 3 * 2        # {both, the connection alone, the listener alone} x {from 0.0.0.0:0, from a peer}
PROTOCOLS = 2 * 2          # {both protocols registered, TCP alone} x {a TCP, a UDP packet}
GATE = 3                   # ICMP, protocol 47, a zero record
NEED_FLAGS = 8 * (32 + 1)  # need 0..7 x (flags 0..31, and no flags array)
EMPTY = 3                  # m = 0: TCP, UDP, a zero record
WRAPPED = 8 + 1            # the eight ids of home slot 15, and a ninth key that misses
FULL = 2 * 2               # no empty slot: two protocols x two ports
CLAMP = 3                  # index m, index 2^24 - 1, and an index left alone
FUZZ = 5000
TOTAL = SUBSETS + ZERO_REMOTE + PROTOCOLS + GATE + NEED_FLAGS + EMPTY + WRAPPED + FULL + CLAMP + FUZZ


def test_rx_demux(tmp_path):
    assert build_and_run(tmp_path, "rx_demux") == TOTAL


def test_rx_demux_under_sanitizers(tmp_path):
    assert build_and_run(tmp_path, "rx_demux", sanitize=True) == TOTAL
