"""tests/stream_ref.py, the Python restatement of yu_rx_stream's rule, against the vectors of
tests/golden/tcp_stream.json, whose receiver outputs tests/golden/make_stream_golden.py took
from the reference's rcv.go executed in goexec.py: it reproduces every one, and the fixture
holds vectors only, stays small and reaches every YU_SEG_* verdict. CPU."""
import json
import os

import stream_cases as C
import stream_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "tcp_stream.json")


def load():
    with open(PATH) as f:
        return json.load(f)


def test_fixture_is_small_and_holds_vectors_only():
    assert os.path.getsize(PATH) < 64 * 1024
    g = load()
    assert set(g) == {"format", "pitch", "heap_at", "local", "remote", "local_port", "remote_port", "vectors"}
    assert g["pitch"] == C.PITCH and g["heap_at"] == C.HEAP_AT and len(g["vectors"]) >= 20
    # every vector whose connection reaches the receiver is executed from rcv.go; the two whose
    # connection is off or reset at entry never call it
    assert sum(v["source"] == "executed" for v in g["vectors"]) >= len(g["vectors"]) - 2
    assert all(len(bytes.fromhex(v["ack_datagram"])) == 40 for v in g["vectors"] if v["ack"])
    for v in g["vectors"]:
        assert v["source"] in ("executed", "restated"), v["name"]
        assert v["source"] == "executed" or v["st"]["state"] in (R.OFF, R.RESET), v["name"]
        assert set(v) - {"ack_datagram"} == {"name", "source", "cap", "st", "heap", "segs", "status", "delivered",
                                             "st_out", "heap_out", "n_acks", "ack"}


def test_fixture_reaches_every_verdict():
    seen = set()
    for v in load()["vectors"]:
        seen |= set(v["status"])
    assert seen == set(range(12)), sorted(set(range(12)) - seen)


def test_model_reproduces_every_vector():
    for v in load()["vectors"]:
        got = R.walk(v["st"], v["heap"], v["cap"], C.place(v["segs"]))
        name = v["name"]
        assert [got["status"][k] for k in range(len(v["segs"]))] == v["status"], name
        assert [list(d) for d in got["delivered"]] == v["delivered"], name
        assert got["st"] == v["st_out"] and got["heap"] == v["heap_out"], name
        assert got["n_acks"] == v["n_acks"], name
        assert (list(got["ack"]) if got["ack"] else None) == v["ack"], name


def test_the_pins_of_the_rule():
    """What the reference does that a reader might not expect, by hand."""
    by = {v["name"]: v for v in load()["vectors"]}
    v = by["trimmed-length-leaves-budget"]
    # 1100+100 parked (budget 100); 1000+150 consumed, the parked one trimmed by 50 and delivered: the
    # budget goes down by the trimmed 50, not by 100 (rcv.go:162 after consumeSegment's TrimFront)
    assert v["status"] == [R.CONSUMED_LATE, R.CONSUMED, R.PENDING]
    assert v["delivered"] == [[C.PITCH, 150], [0 * C.PITCH + 50, 50]]
    assert v["st_out"]["pend_used"] == 100 - 50 + 10 and v["st_out"]["rcv_nxt"] == 1200
    v = by["cap0-keeps-nothing"]
    assert v["status"] == [R.DROPPED, R.CONSUMED, R.DROPPED] and v["st_out"]["pend_count"] == 0
    v = by["dup-popped-as-acknowledged"]
    assert v["status"] == [R.DUPLICATE, R.CONSUMED] and v["st_out"]["pend_used"] == 0


def test_heap_is_container_heap():
    """Push and Pop against a sorted list: the first entry is always the least."""
    import numpy as np
    rng = np.random.default_rng(3)
    heap, ref = [], []
    for step in range(400):
        if ref and rng.integers(0, 3) == 0:
            assert R.heap_pop(heap)["seq"] == ref.pop(0)
        else:
            s = int(rng.integers(0, 1 << 20))
            R.heap_push(heap, dict(seq=s))
            ref.append(s)
            ref.sort()
        assert not heap or heap[0]["seq"] == ref[0]
        for j in range(1, len(heap)):
            assert not R.lt(heap[j]["seq"], heap[(j - 1) // 2]["seq"])
