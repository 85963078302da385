"""CPU suite: csrc/fr_batch_inv.h, the per-lane code of the Lagrange row and of the Lipmaa quotient's table of 1 / Z
(csrc/fr_poly.hip), compiled for the host: tests/cpp/test_fr_batch_inv.cc, plain and under ASan + UBSan as a stand-alone
program (the flags and the link probe of test_host_cpp.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_fr_batch_inv.cc")
INCLUDE = ["-I", os.path.join(ROOT, "legosnark_amd", "csrc")]
SANITIZE = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-3000:]
    return r.stdout


def test_fr_batch_inv(tmp_path):
    exe = str(tmp_path / "test_fr_batch_inv")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *INCLUDE, SRC, "-o", exe])
    _run(exe)


def test_fr_batch_inv_with_the_device_limbs_and_another_run_length(tmp_path):
    """-DLSA_FP_HOST32: the 32-bit-limb product and the Fermat inverse the kernels compile; a run of 5 puts the run
    boundaries elsewhere."""
    exe = str(tmp_path / "test_fr_batch_inv_32")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-DLSA_FP_HOST32", "-DFR_BATCH_INV_RUN=5", *INCLUDE, SRC, "-o", exe])
    assert "run length 5" in _run(exe)


@pytest.fixture(scope="module")
def sanitizer_toolchain(tmp_path_factory):
    """Skips only where a one-line program does not LINK with the sanitizer flags (no runtime libraries installed)."""
    d = tmp_path_factory.mktemp("sanitizer_probe")
    src = d / "probe.cc"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *SANITIZE, str(src), "-o", str(d / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here: " + r.stdout[-300:])


def test_fr_batch_inv_sanitized(tmp_path, sanitizer_toolchain):
    exe = str(tmp_path / "test_fr_batch_inv_san")
    subprocess.check_call(["g++", *SANITIZE, *INCLUDE, SRC, "-o", exe])
    _run(exe)
