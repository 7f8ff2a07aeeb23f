"""k_split on a CPU (yustack_amd/csrc/yucsum_split.h + yucsum_iov.h + yucsum_iov_pack.h):
tests/cpp/rx_split.cpp drives the parse, the delivery tests, the record, the header sums,
the value composition, the single-view walk and the destination geometry as the kernel
does (the header as one window dword per lane, steps of 4 slots, 64 lanes of 16 bytes,
neighbour dwords as the kernel takes them) into exact-size blocks between canaries, and
counts the stores per byte. out, the record, pay_len and the payload are those of a
byte-by-byte restatement of ipv4.HandlePacket, Nic.DeliverTransportPacket, segment.parse
and udp.endpoint.HandlePacket with the scalar library's yu_checksum; every in-room byte
is stored exactly once and no byte outside the packet's span is stored.

The headers make no HIP call, so a plain g++ compiles the program; the same program
(with its own main, run as that program only) also runs under AddressSanitizer +
UBSan."""
from cpp_program import build_and_run, models_compile

LENGTHS = 97 + 17            # L in 0..96 and 1016..1032
PHASES = 4 * 4               # source address mod 4 x destination mod 4
KINDS = 6                    # UDP, ICMP, protocol 47, TCP doff 20 / 24 / 60
# per (L, phases, kind): IHL 5, 6, 15 x (0..3 trailing bytes, all-0x00, all-0xFF) at exact
# room, and at IHL 5 slack 1..5 and short by 1..45
WELL_FORMED = LENGTHS * PHASES * KINDS * (3 * (4 + 2) + 5 + 45)
# per phase pair: len 0..19; 6 kinds x 4 lengths x (IHL 0..4, HL > TL, TL > len, a damaged
# IPv4 sum, a damaged transport sum); slen = H - 1 for 3 protocols x 3 IHLs; TCP doff 16 and
# doff past slen at 4 lengths; UDP Length() = slen + 1 and slen - 1 at 4 lengths
MALFORMED = PHASES * (20 + KINDS * 4 * (5 + 4) + 3 * 3 + 4 * 2 + 4 * 2)
# per phase pair: 65535 bytes, 5 long payloads, and the contract batch's 65536 bytes,
# decreasing offsets, an end past offsets[n], room short by 3, decreasing pay_offsets
LIMITS = PHASES * (1 + 5 + 5)


def test_rx_split(tmp_path):
    assert build_and_run(tmp_path, "rx_split") == WELL_FORMED + MALFORMED + LIMITS


def test_rx_split_under_sanitizers(tmp_path):
    assert build_and_run(tmp_path, "rx_split", sanitize=True) == WELL_FORMED + MALFORMED + LIMITS


def test_the_sibling_programs_still_compile_against_the_headers(tmp_path):
    """yucsum_iov.h, yucsum_iov_pack.h and yucsum_build.h are used as they are
    (yucsum_split.h only adds beside them): the programs of the earlier kernels compile
    against them unchanged."""
    models_compile()
