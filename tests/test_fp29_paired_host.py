"""CPU suite: tests/cpp/test_fp29_paired.cc -- the paired products of fp29.h (mul2, sqr2) on the host build, where they
fall back to the single forms, and the column stepper of the device forms with a plain C++ step, both limb for limb
against mul / sqr; as a plain program, with the column-wise single forms, and as a stand-alone AddressSanitizer +
UndefinedBehaviorSanitizer build run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_fp29_paired.cc")
INC = os.path.join(ROOT, "legosnark_amd", "csrc")


def run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "PASS" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:]


@pytest.mark.parametrize("defines", [[], ["-DLSA_FP29_COLS"]], ids=["serial", "cols"])
def test_paired_products_host(defines, tmp_path):
    exe = str(tmp_path / "test_fp29_paired")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *defines, "-I", INC, SRC, "-o", exe])
    run(exe)


def test_paired_products_host_sanitized(tmp_path):
    exe = str(tmp_path / "test_fp29_paired_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])
    run(exe)
