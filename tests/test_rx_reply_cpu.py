"""yu_rx_reply on a CPU (yustack_amd/csrc/yucsum_reply.h): tests/cpp/rx_reply.cpp runs
k_reply's per-lane function in wave steps of 64 lanes, a lane loading ep and ep_echo only
where the header's predicates allow it, and the scan of yucsum_group.h in its three phases
in place over r_offsets, on heap blocks of the exact sizes (the workspace exactly
yu_rx_reply_workspace_bytes(n)), every store index checked and counted, against a direct
loop over the records' fields.

n covers the wave-step and scan-tile seams (0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 +
5); at each n every `what`, flags NULL and given with need 0 and IP_OK | L4_OK, ep_echo
NULL, all zero and mixed; the packets cycle through ICMP types 8 (with and without a code),
0 and 3, UDP, TCP, protocol 47, all-zero records and view lengths at the limit and one past
it, and ep through 0, m - 1, m and YU_DEMUX_NONE.

The header makes no HIP call, so a plain g++ compiles the program; the same program (with
its own main, run as that program only) also runs under AddressSanitizer + UBSan."""
from cpp_program import build_and_run

NS = 9          # 0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 5
COMBOS = 4 * 3 * 3  # what x (flags NULL, need 0, need IP_OK | L4_OK) x (ep_echo NULL, zero, mixed)
ONE_ENDPOINT = COMBOS  # m = 1 at n = 65
NO_ENDPOINT = 3        # m = 0
TOTAL = NS * COMBOS + ONE_ENDPOINT + NO_ENDPOINT


def test_rx_reply(tmp_path):
    assert build_and_run(tmp_path, "rx_reply", sources=(), ends="cases ok") == TOTAL


def test_rx_reply_under_sanitizers(tmp_path):
    assert build_and_run(tmp_path, "rx_reply", sources=(), sanitize=True, ends="cases ok") == TOTAL
