"""Loader for the in-tree C-ABI library ``yustack_amd/libyucsum.so`` (include/yucsum.h).

There is no fallback: if the library is missing or cannot be loaded, importing
anything that needs it raises, and the batched (GPU) entry points return a negative
status that :func:`check` turns into an exception when no HIP device is usable.
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libyucsum.so")

_vp, _u16, _u32, _u64, _sz, _i32, _str = (ctypes.c_void_p, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64,
                                          ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p)
# what the batch calls share: (data, stride, len, n | tables, n), mode, initial_arr, initial, addrs, out
_UNIFORM = [_vp, _u64, _u32, _u64, _i32, _vp, _u16, _vp, _vp]
_RAGGED = [_vp, _vp, _u64, _i32, _vp, _u16, _vp, _vp]


def _same(names: str, restype, argtypes) -> dict:
    return {name: (restype, argtypes) for name in names.split()}


# Every exported symbol declared in include/yucsum.h: (restype, argtypes).
PROTOTYPES = {
    "yu_checksum": (_u16, [_vp, _sz, _u16]),
    "yu_checksum_combine": (_u16, [_u16, _u16]),
    "yu_pseudo_header_checksum": (_u16, [_u32, _vp, _sz, _vp, _sz]),
    **_same("yu_csum_batch_uniform yu_csum_fill_uniform", _i32, _UNIFORM + [_vp]),  # + stream
    **_same("yu_csum_batch_ragged yu_csum_fill_ragged yu_csum_batch_iov yu_csum_fill_iov", _i32, _RAGGED + [_vp]),
    **_same("yu_csum_batch_iov_datagram yu_csum_fill_iov_datagram", _i32, [_vp, _vp, _u64, _i32, _vp, _vp]),
    **_same("yu_csum_pack_iov yu_csum_pack_fill_iov", _i32, _RAGGED[:-1] + [_vp, _vp, _vp, _vp]),  # + dst, dst_offsets
    **_same("yu_csum_pack_iov_datagram yu_csum_pack_fill_iov_datagram", _i32,
            [_vp, _vp, _u64, _i32, _vp, _vp, _vp, _vp]),
    "yu_tx_build_ragged": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    # data, offsets, n, pay, pay_offsets, recs, pay_len, out, stream
    "yu_rx_split_ragged": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    # data, offsets, n, verify, recs, pay_views, out, stream
    "yu_rx_parse_ragged": (_i32, [_vp, _vp, _u64, _i32, _vp, _vp, _vp, _vp]),
    "yu_demux_table_bytes": (_u64, [_u64]),
    "yu_demux_hash": (_u32, [_vp]),
    # ids, m, h_table, table_bytes, bad
    "yu_demux_table_fill": (_i32, [_vp, _u64, _vp, _u64, _vp]),
    # recs, flags, need, n, table, table_bytes, m, ep, ep_count, stream
    "yu_rx_demux": (_i32, [_vp, _vp, _u16, _u64, _vp, _u64, _u64, _vp, _vp, _vp]),
    "yu_rx_group_workspace_bytes": (_u64, [_u64, _u64]),
    # ep, n, m, views, order, first, q_views, q_offsets, work, work_bytes, stream
    "yu_rx_group": (_i32, [_vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "yu_rx_group_variant_n": (_str, [_u64, _u64]),
    "yu_rx_reply_workspace_bytes": (_u64, [_u64]),
    # recs, flags, need, views, ep, m, ep_echo, what, n, r_recs, r_offsets, work, work_bytes, stream
    "yu_rx_reply": (_i32, [_vp, _vp, _u16, _vp, _vp, _u64, _vp, _u32, _u64, _vp, _vp, _vp, _u64, _vp]),
    # views, recs, n, dst, dst_offsets, out, stream
    "yu_tx_build_iov": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    **_same("yu_rx_reply_variant_n yu_tx_build_iov_variant_n", _str, [_u64]),
    "yu_rx_stream_workspace_bytes": (_u64, [_u64, _u64, _u32]),
    # recs, views, n, order, first, m, ids, st, heap, cap, status, s_views, s_offsets, a_recs, a_offsets, n_acks,
    # work, work_bytes, stream
    "yu_rx_stream": (_i32, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                            _u64, _vp]),
    "yu_rx_stream_variant_n": (_str, [_u64, _u64, _u32]),
    **_same("yu_csum_batch_host_uniform yu_csum_fill_host_uniform", _i32, _UNIFORM + [_i32]),  # + device
    **_same("yu_csum_batch_host_ragged yu_csum_fill_host_ragged yu_csum_batch_host_iov yu_csum_fill_host_iov", _i32,
            _RAGGED + [_i32]),
    "yu_csum_batch_host_uniform_multi": (_i32, _UNIFORM + [_vp, _i32]),  # + devices, count
    **_same("yu_csum_batch_host_ragged_multi yu_csum_batch_host_iov_multi", _i32, _RAGGED + [_vp, _i32]),
    "yu_abi_version": (_i32, []),
    "yu_strerror": (_str, [_i32]),
    "yu_device_count": (_i32, []),
    "yu_uniform_variant": (_str, [_u64, _u32, _i32, _u64]),
    "yu_uniform_variant_n": (_str, [_u64, _u32, _u64, _i32, _u64]),
    "yu_ragged_variant": (_str, [_i32]),
    **_same("yu_ragged_variant_n yu_ragged_fill_variant_n", _str, [_i32, _u64]),
    **_same("yu_iov_variant_n yu_iov_datagram_variant_n yu_iov_pack_variant_n yu_iov_pack_datagram_variant_n", _str,
            [_i32, _u64, _i32]),
    **_same("yu_tx_build_variant_n yu_rx_split_variant_n yu_rx_parse_variant_n yu_rx_demux_variant_n", _str,
            [_u64]),
    "yu_host_contexts": (_i32, []),
    "yu_host_staging_bytes": (_u64, [_i32, _vp]),
    "yu_host_staging_trim": (_i32, [_i32]),
    "yu_hip_runtime_path": (_str, []),
}
EXPORTS = tuple(PROTOTYPES)  # checked by tests/test_abi.py

# Host-path staging bounds (include/yucsum.h): per context, between calls.
HOST_SLICE_BYTES, HOST_SLICE_PACKETS = 32 << 20, 1 << 18
HOST_CONTEXT_PINNED_MAX = 3 * (HOST_SLICE_BYTES + 26 * HOST_SLICE_PACKETS + 72)
HOST_CONTEXT_DEVICE_MAX = 3 * (HOST_SLICE_BYTES + 22 * HOST_SLICE_PACKETS + 8)
HOST_BURST_CONTEXT_PINNED_MAX = (4 << 20) + 26 * HOST_SLICE_PACKETS + 72
HOST_BURST_CONTEXT_DEVICE_MAX = (4 << 20) + 22 * HOST_SLICE_PACKETS + 8

YU_OK, YU_EINVAL, YU_ENODEV, YU_ENOMEM, YU_EHIP_BASE = 0, -22, -19, -12, -1000


class YuIovec(ctypes.Structure):
    """struct yu_iovec (include/yucsum.h): one view of a scatter-gather packet."""
    _fields_ = [("base", ctypes.c_void_p), ("len", ctypes.c_uint64)]


class YuTxRecord(ctypes.Structure):
    """struct yu_tx_record (include/yucsum.h): one outgoing datagram's header fields."""
    _fields_ = [("src", ctypes.c_uint8 * 4), ("dst", ctypes.c_uint8 * 4), ("sport", ctypes.c_uint16),
                ("dport", ctypes.c_uint16), ("seq", ctypes.c_uint32), ("ack", ctypes.c_uint32),
                ("window", ctypes.c_uint16), ("flags", ctypes.c_uint8), ("doff", ctypes.c_uint8),
                ("proto", ctypes.c_uint8), ("ttl", ctypes.c_uint8), ("ip_id", ctypes.c_uint16),
                ("tos", ctypes.c_uint8), ("reserved", ctypes.c_uint8), ("frag", ctypes.c_uint16)]


class YuEndpointId(ctypes.Structure):
    """struct yu_endpoint_id (include/yucsum.h): one registered endpoint id of the demultiplexer's table."""
    _fields_ = [("local_addr", ctypes.c_uint8 * 4), ("remote_addr", ctypes.c_uint8 * 4),
                ("local_port", ctypes.c_uint16), ("remote_port", ctypes.c_uint16), ("proto", ctypes.c_uint8),
                ("kind", ctypes.c_uint8), ("reserved", ctypes.c_uint16)]


class YuError(RuntimeError):
    def __init__(self, status: int, what: str):
        self.status = status
        super().__init__(f"{what} failed: status {status} ({strerror(status)})")


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not built — run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C yustack_amd/csrc`")
    # One process, two HIP runtimes: PyTorch-ROCm bundles its own libamdhip64 (no
    # SONAME), the library binds /opt/rocm's. Measured on the GPU box
    # (tools/load_order_probe.py): with torch's loaded first both see the device in
    # either order of first use; with this library loaded first, whichever runtime
    # initialises second sees no device. So torch, when installed, is loaded first
    # (a torch that fails to import for any reason is skipped: the library itself
    # does not need it), and the binding is then checked (check_runtime).
    try:
        import torch  # noqa: F401
    except Exception:  # noqa: BLE001 — any broken torch install: load without it
        pass
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    check_runtime(L)
    _lib = L
    return L


def torch_hip_runtime() -> str | None:
    """Path of the HIP runtime PyTorch-ROCm bundles (torch/lib/libamdhip64*), when
    torch is imported and that file is mapped into this process; else None (no
    torch, or a torch that uses the system runtime like this library)."""
    import sys
    torch = sys.modules.get("torch")
    if torch is None or not getattr(torch, "__file__", None):
        return None
    tlib = os.path.join(os.path.dirname(os.path.realpath(torch.__file__)), "lib") + os.sep
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.split(maxsplit=5)[-1].strip()
                if path.startswith(tlib) and os.path.basename(path).startswith("libamdhip64"):
                    return path
    except OSError:  # pragma: no cover - /proc is always there on Linux
        return None
    return None


def check_runtime(L) -> None:
    """One HIP runtime per process: when torch's bundled runtime is
    loaded, the library's HIP calls must be bound to it. They are not when the
    library was loaded (e.g. by ctypes) before torch was imported; every HIP call of
    the library would then run on a second runtime, and whichever of the two
    initialises second sees no device (profiles/r05/load_order_r05.log). Raises
    ImportError naming the fix instead of failing later as "no device"."""
    theirs = torch_hip_runtime()
    if theirs is None:
        return
    raw = L.yu_hip_runtime_path()
    ours = raw.decode() if raw else None
    if ours is None or os.path.realpath(ours) != os.path.realpath(theirs):
        raise ImportError(
            f"{LIB_PATH} is bound to the HIP runtime {ours}, but torch uses {theirs}: two HIP "
            "runtimes in one process (the one initialised second sees no device). The library "
            "was loaded before torch; import torch (or yustack_amd) before loading "
            "libyucsum.so by any other means.")


def strerror(status: int) -> str:
    try:
        return lib().yu_strerror(status).decode()
    except Exception:  # pragma: no cover - only when the library itself is unusable
        return "unknown"


def check(status: int, what: str) -> None:
    if status != YU_OK:
        raise YuError(status, what)


def host_staging(device: int = 0) -> tuple[int, int]:
    """(pinned host bytes, device bytes) the host-path staging of `device` holds now
    (yu_host_staging_bytes); both 0 before its first host call."""
    d = ctypes.c_uint64(0)
    pinned = lib().yu_host_staging_bytes(device, ctypes.byref(d))
    return int(pinned), int(d.value)
