"""k_parse on a CPU (yustack_amd/csrc/yucsum_parse.h + yucsum_split.h):
tests/cpp/rx_parse.cpp drives one lane's work as the kernel does (the window dwords it
loads, d0 .. d4 and t0 .. t3 out of them, the second load for an IHL other than 5, the
parse, the record, the header bits and the view) against a byte-by-byte restatement of
ipv4.HandlePacket, Nic.DeliverTransportPacket, segment.parse and
udp.endpoint.HandlePacket. Every load is recorded: none lies outside the window of the
packet's first min(len, 80) bytes or outside the batch, and a lane makes fifteen at
the most.

The headers make no HIP call, so a plain g++ compiles the program; the same program
(with its own main, run as that program only) also runs under AddressSanitizer +
UBSan, where the batch's exact-size block turns a stray read into a report."""
from cpp_program import build_and_run

PHASES = 4
KINDS = 7                                   # UDP, ICMP, protocol 47, TCP doff 20 / 24 / 60 / 16
WELL_FORMED = PHASES * 11 * KINDS * 5 * 2   # IHL 5..15 x payloads x {batch end, bytes behind}
SHORT_HEADER = PHASES * 5 * KINDS * 3       # IHL 0..4
SHORT_PACKET = PHASES * 20                  # len 0..19
TOTAL_LENGTH = PHASES * KINDS * 3 * 2       # TL below HL, TL past len
SLEN = PHASES * 3 * 3                       # slen = H - 1: three protocols x three IHLs
DOFF = PHASES * 3 * 4                       # TCP doff past slen
UDP_LENGTH = PHASES * 3 * 3 * 2             # Length() = slen + 1, slen - 1
BATCH_END = PHASES * 81 * 3                 # len 20..100 ending at the batch end
LIMITS = PHASES * 4                         # 65535 and 65536 bytes, decreasing offsets, an end past offsets[n]
TOTAL = WELL_FORMED + SHORT_HEADER + SHORT_PACKET + TOTAL_LENGTH + SLEN + DOFF + UDP_LENGTH + BATCH_END + LIMITS


def test_rx_parse(tmp_path):
    assert build_and_run(tmp_path, "rx_parse") == TOTAL


def test_rx_parse_under_sanitizers(tmp_path):
    assert build_and_run(tmp_path, "rx_parse", sanitize=True) == TOTAL
