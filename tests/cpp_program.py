"""Builds and runs one of the stand-alone CPU programs of tests/cpp/ (each has its own
main) for the test_*_cpu.py files, test_iov_combine.py and test_dense_geom.py: plain,
or under AddressSanitizer + UBSan (host code only, run directly, nothing preloaded).
A plain module, like iov_layout.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
INC = [f"-I{ROOT}/include", f"-I{ROOT}/yustack_amd/csrc"]
SCALAR = os.path.join(ROOT, "yustack_amd", "csrc", "yucsum_scalar.cpp")
SAN_FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
MODELS = ("iov_combine.cpp", "iov_datagram.cpp", "iov_pack.cpp", "iov_pack_datagram.cpp", "tx_build.cpp",
          "rx_split.cpp")


def build_and_run(tmp_path, program, sources=(SCALAR,), sanitize=False, ends="packets ok"):
    """Compiles tests/cpp/<program>.cpp with `sources` (-Wall -Werror) and runs it: it
    exits 0 and its output ends with `ends`. Returns the number its last line starts
    with (the packets it checked), None when that line has none."""
    exe = str(tmp_path / (program + ("_san" if sanitize else "")))
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *(SAN_FLAGS if sanitize else ["-O2"]), *INC,
                        os.path.join(CPP, program + ".cpp"), *sources, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0") if sanitize else None
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith(ends), (r.stdout[-3000:], r.stderr[-3000:])
    first = r.stdout.strip().splitlines()[-1].split()[0]
    return int(first) if first.isdigit() else None


def models_compile():
    """The six CPU models of the wave-per-packet kernels compile against the library's
    headers as they are."""
    for src in MODELS:
        r =subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-fsyntax-only", *INC,
                            os.path.join(CPP, src)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (src, r.stderr[-3000:])
