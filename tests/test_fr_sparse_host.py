"""CPU suite: csrc/fr_sparse.h, the per-row routine of the sparse Fr matrix kernels (csrc/fr_sparse.hip), compiled for the
host against big-integer arithmetic: tests/cpp/test_fr_sparse.cc, plain and under ASan + UBSan as a stand-alone program (the
flags and the link probe of test_fr_dot_host.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_fr_sparse.cc")
INCLUDE = ["-I", os.path.join(ROOT, "legosnark_amd", "csrc")]
SANITIZE = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-3000:]
    return r.stdout


def test_fr_sparse(tmp_path):
    exe = str(tmp_path / "test_fr_sparse")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *INCLUDE, SRC, "-o", exe])
    assert "unit max 20, dot max partials 60, group 4" in _run(exe)


@pytest.fixture(scope="module")
def sanitizer_toolchain(tmp_path_factory):
    """Skips only where a one-line program does not LINK with the sanitizer flags (no runtime libraries installed)."""
    d = tmp_path_factory.mktemp("sanitizer_probe")
    src = d / "probe.cc"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *SANITIZE, str(src), "-o", str(d / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here: " + r.stdout[-300:])


def test_fr_sparse_sanitized(tmp_path, sanitizer_toolchain):
    exe = str(tmp_path / "test_fr_sparse_san")
    subprocess.check_call(["g++", *SANITIZE, *INCLUDE, SRC, "-o", exe])
    _run(exe)
