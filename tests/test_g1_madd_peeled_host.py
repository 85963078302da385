"""CPU suite: tests/cpp/test_g1_madd_peeled.cc -- the arithmetic of the G1 bucket accumulation (fp29.h: the signed mixed
addition, the affine + affine head of a bucket list, the carry-free subtractions and the column bounds of dot2 they rest
on) against the unchanged xyzz29_madd and the canonical 32-bit-limb code, as a plain program and as a stand-alone
AddressSanitizer + UndefinedBehaviorSanitizer build run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_g1_madd_peeled.cc")
INC = os.path.join(ROOT, "legosnark_amd", "csrc")
SANITIZE = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "PASS" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:]
    return r.stdout


@pytest.mark.parametrize("defines", [[], ["-DLSA_FP29_COLS"], ["-DLSA_FP_HOST32"]], ids=["serial", "cols", "host32"])
def test_g1_bucket_addition_host(defines, tmp_path):
    exe = str(tmp_path / "test_g1_madd_peeled")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *defines, "-I", INC, SRC, "-o", exe])
    out = run(exe)
    assert "dot2 column maxima" in out


def test_g1_bucket_addition_host_sanitized(tmp_path):
    """The same program with ASan + UBSan as a stand-alone binary run directly, any report fatal.  No probe and no skip:
    where the sanitizer runtime is missing the link fails, and so does this test."""
    exe = str(tmp_path / "test_g1_madd_peeled_san")
    subprocess.check_call(["g++", *SANITIZE, "-I", INC, SRC, "-o", exe])
    run(exe)
