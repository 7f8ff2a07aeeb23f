#!/usr/bin/env python3
"""Generate tests/golden/echo_icmp.json: the ICMP Echo replies the reference's own
sender produces when executed.

ipv4.handleICMP answers an Echo with sendICMPv4(r, ICMPv4EchoReply, 0, v)
(network/ipv4/icmp.go:28-63). As for tests/golden/refexec.json, tests/golden/goexec.py
(imported unchanged, through make_refexec.Ref) loads the reference's Go files at
generation time only and executes that call, through types.Route into the ipv4
endpoint's WritePacket and a stub link endpoint: each vector is the datagram the
reference would put on the wire for one payload, with both checksum fields as the
sender stored them. Nothing of the reference is copied into this repo: the fixture
holds vectors only (addresses, the payload, the datagram), each marked as executed.

Payload lengths 0..5, 63..65, 1023..1025 and 1472 (a 1500-byte datagram).
tests/test_gpu_rx_echo.py builds the matching type-8 requests and expects the device
echo to reproduce each datagram byte for byte.

Run from the repo root: python tests/golden/make_echo_golden.py [out.json]
"""
from __future__ import annotations

import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_refexec import Ref  # noqa: E402  (goexec, and the route / link stubs around it)

ICMPV4_ECHO_REPLY = 0  # header.ICMPv4EchoReply
LENGTHS = list(range(0, 6)) + [63, 64, 65, 1023, 1024, 1025, 1472]


def build(ref: Ref) -> dict:
    rng = random.Random(20261021)
    vecs = []
    for n in LENGTHS:
        a = bytes(rng.getrandbits(8) for _ in range(8))
        data = bytes(rng.getrandbits(8) for _ in range(n))
        # the reply leaves from the request's destination: src is the replier's address
        dg = ref.send_icmp(a[:4], a[4:], ICMPV4_ECHO_REPLY, 0, data)
        assert len(dg) == 24 + n and dg[9] == 1 and dg[20] == 0 and dg[21] == 0 and dg[24:] == data
        assert dg[12:16] == a[:4] and dg[16:20] == a[4:]
        vecs.append({"src": a[:4].hex(), "dst": a[4:].hex(), "data": data.hex(), "reply": dg.hex(), "executed": True})
    return {"generator": "tests/golden/make_echo_golden.py: sendICMPv4(route, ICMPv4EchoReply, 0, data) of the "
                         "reference's Go source executed by tests/golden/goexec.py",
            "icmp_echo_reply": vecs}


def main() -> None:
    out = build(Ref())
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "echo_icmp.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    size = os.path.getsize(path)
    assert size < 64 << 10, size
    print(f"wrote {path}: {len(out['icmp_echo_reply'])} executed vectors, {size} bytes")


if __name__ == "__main__":
    main()
