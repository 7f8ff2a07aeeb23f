"""k_small<16,6>'s dense fetch (dense uniform batches of 4-aligned MTU-size packets on
16-aligned data: the step's byte range loaded as whole lines and repacked through
LDS) against the C oracle, bit for bit, in the interleaved and the runs form, with
the lead-in chunks of a batch that does not start on a line, partial last steps,
and the shapes that must keep the window path.

Every call is read-only: the data tensor is compared with its host copy afterwards,
and the result array sits between guard elements that must stay unchanged.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from yustack_amd import batch

pytestmark = pytest.mark.gpu

GUARD = 8
GUARD_VALUE = 0xA5A5
N_SMALL = (1, 3, 4, 5, 16, 17, 63, 65, 4099)  # the interleaved form at default knobs
N_RUNS = 32768 + 17                           # the runs form (>= 8 runs per CU on 256 CUs)
OFFSETS = (0, 16, 48, 112)                    # of the data pointer in its (line-aligned) tensor
MODES = (O.MODE_TCP, O.MODE_UDP, O.MODE_RAW, O.MODE_VERIFY_TCP)
PAD = 128 + 64


@pytest.fixture(scope="module")
def pool():
    """One host byte pool the cases cut their batches from (left unchanged)."""
    rng = np.random.default_rng(7)
    n = N_RUNS * 1504 + PAD
    return {"rand": rng.integers(0, 256, size=n, dtype=np.uint8),
            "ff": np.full(4099 * 1504 + PAD, 255, np.uint8),
            "zero": np.zeros(4099 * 1504 + PAD, np.uint8),
            "addrs": rng.integers(0, 256, size=8 * N_RUNS, dtype=np.uint8),
            "init": rng.integers(0, 65536, size=N_RUNS, dtype=np.uint16)}


def _case(dev, oracle_c, pool, mode, length, stride, n, off, kind="rand"):
    total = off + (n - 1) * stride + length
    host = pool[kind][:total + 64].copy()
    if mode in (O.MODE_TCP, O.MODE_VERIFY_TCP):
        # DataOffset 5, as bench.py sets it for config 3
        host[off + 12:off + 12 + n * stride:stride] = 0x50
    addrs = pool["addrs"][:8 * n] if mode in (O.MODE_TCP, O.MODE_UDP) else None
    init = pool["init"][:n] if mode == O.MODE_RAW else None
    d = torch.from_numpy(host).to(dev)
    assert d.data_ptr() % 128 == 0  # so `off` is the batch's offset in its first line
    view = d[off:]
    big = torch.full((n + 2 * GUARD,), GUARD_VALUE, dtype=torch.uint16, device=dev)
    out = big[GUARD:GUARD + n]
    batch.checksum_uniform(view, stride, length, n, mode,
                           initial_arr=None if init is None else torch.from_numpy(init.copy()).to(dev),
                           addrs=None if addrs is None else torch.from_numpy(addrs.copy()).to(dev),
                           out=out)
    res = big.cpu().numpy()
    want = oracle_c.batch(host[off:], mode, stride=stride, length=length, n=n,
                          initial_arr=init, addrs=addrs)
    ctx = (mode, length, stride, n, off, kind)
    assert np.array_equal(res[GUARD:GUARD + n], want), ctx
    assert (res[:GUARD] == GUARD_VALUE).all() and (res[GUARD + n:] == GUARD_VALUE).all(), ctx
    assert np.array_equal(d.cpu().numpy(), host), ctx  # a read-only call writes nothing


@pytest.mark.parametrize("length", [1500, 1496, 1400])
@pytest.mark.parametrize("mode", MODES)
def test_dense_interleaved(dev, oracle_c, pool, mode, length):
    assert batch.variant(length, length, mode, 0) == "k_small<16,6>"
    for i, n in enumerate(N_SMALL):
        # every pointer offset at each n up to 65; the large batch takes them in turn
        for off in (OFFSETS if n <= 65 else (OFFSETS[(i + length // 4) % 4],)):
            _case(dev, oracle_c, pool, mode, length, length, n, off)


@pytest.mark.parametrize("length", [1500, 1496, 1400])
@pytest.mark.parametrize("kind", ["ff", "zero"])
def test_dense_constant_bytes(dev, oracle_c, pool, kind, length):
    for mode in MODES:
        for n, off in ((5, 48), (65, 112), (4099, 16)):
            _case(dev, oracle_c, pool, mode, length, length, n, off, kind=kind)


@pytest.mark.parametrize("length", [1500, 1496, 1400])
@pytest.mark.parametrize("mode", MODES)
def test_dense_runs(dev, oracle_c, pool, mode, length):
    """32768 + 17 packets: the runs form, a last run of one step and a last step of one packet."""
    _case(dev, oracle_c, pool, mode, length, length, N_RUNS, OFFSETS[(mode + length // 4) % 4])


# data 4 bytes off a 16-byte boundary, a length that is not whole dwords, a gap between packets
@pytest.mark.parametrize("length,stride,off", [(1500, 1500, 4), (1498, 1498, 16), (1500, 1504, 48)])
@pytest.mark.parametrize("mode", MODES)
def test_window_path_kept(dev, oracle_c, pool, mode, length, stride, off):
    """Shapes the dense predicate refuses keep matching the oracle, in both forms."""
    for n in (5, 17, 65, 4099, N_RUNS):
        _case(dev, oracle_c, pool, mode, length, stride, n, off)
