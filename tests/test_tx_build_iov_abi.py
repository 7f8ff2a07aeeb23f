"""yu_tx_build_iov at the C-ABI boundary (include/yucsum.h: yu_tx_build_iov,
yu_tx_build_iov_variant_n): exported and declared, every documented YU_EINVAL returned
before any device work, the empty batch, YU_ENODEV without a device for what the header
says is not an error, the variant name, that the call added no row to the wave-kernel
table, and what the Python front end refuses. CPU only: no call here reaches a device
(the arguments are refused first, or there is no device)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from yustack_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "yucsum.h")
NAMES = ("yu_tx_build_iov", "yu_tx_build_iov_variant_n")


def test_symbols_exported_and_declared():
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert re.search(rf" T {name}$", nm, flags=re.M), name
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None
    assert len(L.yu_tx_build_iov.argtypes) == 7
    assert L.yu_abi_version() == 1


@pytest.fixture
def tables():
    pay = (ctypes.c_uint8 * 256)()
    dst = (ctypes.c_uint8 * 512)()
    out = (ctypes.c_uint16 * 16)()
    recs = (_lib.YuTxRecord * 5)()
    for r in recs:
        r.proto, r.doff, r.ttl = 17, 20, 64
    p = ctypes.addressof(pay)
    views = (_lib.YuIovec * 5)(*[_lib.YuIovec(p + 64 * (i % 4), 64) for i in range(5)])
    do = (ctypes.c_uint64 * 6)(0, 92, 184, 276, 368, 0)
    yield (ctypes.addressof(views), ctypes.addressof(recs), ctypes.addressof(dst), ctypes.addressof(do),
           ctypes.addressof(out))
    del pay, dst, out, recs, views, do


def test_every_einval_precedes_device_work(tables):
    """Each refused argument returns YU_EINVAL, whether or not a device is present
    (nothing is launched: the pointers here are host memory)."""
    f = _lib.lib().yu_tx_build_iov
    v, r, d, do, o = tables
    E = _lib.YU_EINVAL
    assert f(None, r, 4, d, do, o, None) == E       # [data] views
    assert f(v, None, 4, d, do, o, None) == E       # [data] recs
    assert f(v, r, 4, None, do, o, None) == E       # [data] dst
    assert f(v, r, 4, d, None, o, None) == E        # [offsets] dst_offsets
    assert f(v, r, 4, d, do + 4, o, None) == E      # [offsets] dst_offsets alignment
    assert f(v + 4, r, 4, d, do, o, None) == E      # [offsets] views alignment
    assert f(v, r + 4, 4, d, do, o, None) == E      # [offsets] recs alignment
    for n in (4, 0):
        assert f(v, r, n, d, do, o + 1, None) == E  # [side-align] out, checked without n
    assert bytes(ctypes.string_at(d, 512)) == bytes(512)


def test_empty_batch_is_a_no_op(tables):
    f = _lib.lib().yu_tx_build_iov
    v, r, d, do, o = tables
    assert f(v, r, 0, d, do, o, None) == _lib.YU_OK
    assert f(None, None, 0, None, None, None, None) == _lib.YU_OK
    assert bytes(ctypes.string_at(d, 512)) == bytes(512)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_valid_calls_fail_without_gpu(tables):
    f = _lib.lib().yu_tx_build_iov
    v, r, d, do, o = tables
    assert f(v, r, 4, d, do, o, None) == _lib.YU_ENODEV
    assert f(v + 8, r + 8, 4, d + 3, do, None, None) == _lib.YU_ENODEV  # 8-byte tables, any dst alignment, NULL out
    assert bytes(ctypes.string_at(d, 512)) == bytes(512)


def test_variant_name_and_no_new_table_row():
    L = _lib.lib()
    for n in (0, 1, 64, 4097, 1 << 20):
        assert L.yu_tx_build_iov_variant_n(n) == b"k_build<4,iov>"
        assert batch.build_iov_variant(n) == "k_build<4,iov>"
        assert L.yu_tx_build_variant_n(n) == b"k_build<4>"          # the contiguous call keeps its kernel
    plan_h = open(os.path.join(ROOT, "yustack_amd", "csrc", "yucsum_plan.h")).read()
    table = plan_h[plan_h.index("#define YU_WAVE_KERNELS(X)"):plan_h.index("enum class WaveFamily")]
    assert len(re.findall(r"^\s*X\(", table, flags=re.M)) == 10 and "k_build<4,iov>" not in table


def test_python_front_end_refuses_before_the_library():
    views = torch.zeros((1, 2), dtype=torch.int64)
    do = torch.tensor([0, 92], dtype=torch.int64)
    recs = torch.zeros((1, 32), dtype=torch.uint8)
    with pytest.raises(TypeError):
        batch.build_datagrams_iov(views, recs, do, torch.zeros(128, dtype=torch.uint8))  # CPU tensors
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda:0")
    views, do, recs = views.to(dev), do.to(dev), recs.to(dev)
    dst = torch.zeros(128, dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError):
        batch.build_datagrams_iov(views.to(torch.int32), recs, do, dst)          # dtype
    with pytest.raises(TypeError):
        batch.build_datagrams_iov(views, recs.to(torch.int32), do, dst)          # dtype
    with pytest.raises(TypeError):
        batch.build_datagrams_iov(views, recs, do.to(torch.float32), dst)        # dtype
    with pytest.raises(ValueError):
        batch.build_datagrams_iov(views, recs.reshape(32), do, dst)              # shape
    with pytest.raises(ValueError):
        batch.build_datagrams_iov(torch.zeros((2, 2), dtype=torch.int64, device=dev), recs, do, dst)  # n views
    with pytest.raises(ValueError):
        batch.build_datagrams_iov(views, recs, torch.zeros(3, dtype=torch.int64, device=dev), dst)  # n + 1 offsets
    with pytest.raises(ValueError):
        batch.build_datagrams_iov(views, recs, do, recs.reshape(32))             # dst overlaps records
    with pytest.raises(TypeError):
        batch.build_datagrams_iov(views, recs, do, torch.zeros(128, dtype=torch.uint8))  # CPU dst
