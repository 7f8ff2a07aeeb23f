"""k_small's dense fetch geometry (yustack_amd/csrc/yucsum_dense.h) on a CPU:
tests/cpp/dense_geom.cpp walks every step and lane of a set of dense batches and
checks what is loaded (inside the batch, each packet byte exactly once, whole
lines), where each group's window sits in the LDS slice, and which batches the
predicate admits. The header makes no HIP call, so a plain g++ compiles it; the
same program also runs under AddressSanitizer + UBSan (host code with its own
main)."""
from cpp_program import build_and_run


def test_dense_geometry(tmp_path):
    build_and_run(tmp_path, "dense_geom", sources=(), ends="ok")


def test_dense_geometry_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "dense_geom", sources=(), sanitize=True, ends="ok")
