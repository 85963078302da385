"""CPU suite: csrc/fq_sqrt.h compiled for the host (tests/cpp/test_fq_sqrt.cc, a stand-alone program) -- fq_sqrt / fq2_sqrt
against Euler's criterion and root^2 == a on 0, 1, p - 1, squares, non-squares, (t, 0) with t a residue and a non-residue,
elements that take the second candidate of x0 and a few thousand pseudo-random ones; g2_in_subgroup against [r]P == O by plain
double-and-add on generator multiples, twist points found by trying x, [c]T, points of order 10069 and 5864401, sums of a G2
point and a small-order point, infinity, each with Z = 1 and with a Z outside Fq.  Built at -O2 and again under ASan + UBSan
(any report fatal), as tests/test_host_cpp.py builds its programs.  And: without a GPU the Python entry point fails loudly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_fq_sqrt.cc")
INC = ["-I", os.path.join(ROOT, "legosnark_amd", "csrc")]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "PASS" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:]
    return r.stdout


@pytest.mark.parametrize("tag,flags", [("o2", ["-O2"]), ("o2_limbs32", ["-O2", "-DLSA_FP_HOST32"])])
def test_roots_and_subgroup_predicate_on_the_host(tag, flags, tmp_path):
    """(-DLSA_FP_HOST32: the 32-bit-limb product the device compiles, on the host.)"""
    exe = str(tmp_path / ("test_fq_sqrt_" + tag))
    subprocess.check_call(["g++", "-std=c++17", *flags, *INC, SRC, "-o", exe])
    out = run(exe)
    assert "points 20 in G2, 22 outside" in out


def test_roots_and_subgroup_predicate_under_sanitizers(tmp_path):
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", *SANITIZE, str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here: " + r.stdout[-300:])
    exe = str(tmp_path / "test_fq_sqrt_san")
    subprocess.check_call(["g++", "-std=c++17", *SANITIZE, *INC, SRC, "-o", exe])
    assert "runtime error" not in run(exe)


def test_decompress_fails_loudly_without_a_device():
    import numpy as np
    import legosnark_amd
    if not os.path.exists(legosnark_amd.LIB_PATH):
        legosnark_amd.build()
    if legosnark_amd.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(legosnark_amd.LsaError):
        legosnark_amd.decompress("g1", np.zeros((1, 4), dtype=np.uint64), np.zeros(1, dtype=np.uint8))
    with pytest.raises(legosnark_amd.LsaError):
        legosnark_amd.validate_points("g2", np.zeros((1, 24), dtype=np.uint64))
    with pytest.raises(legosnark_amd.LsaError):
        legosnark_amd.compress("g2", np.zeros((1, 24), dtype=np.uint64))
