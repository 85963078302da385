"""GPU: tools/paired_check.hip -- the paired products of fp29.h (mul2, sqr2) and the G1 point formulas that use them
(xyzz29_madd_signed of the bucket accumulation, xyzz29_add_affine of a bucket list's head, xyzz29_add_paired of the
tail) run on the device and compared on the host with mul / sqr limb for limb and with the plain xyzz29_madd /
xyzz29_add as canonical affine points: 4096 random
operand pairs and the stated extremes of each form, 64 x 8 lanes of random accumulators and bases and the degenerate
lanes (accumulator at infinity, doubling, cancellation, both signs).  A stand-alone program: no symbol is added to the
library.  The library's Makefile has a target for it outside `all`; this test makes that target (nothing to do where the
program is already up to date) and runs the program under a time limit of its own."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "legosnark_amd", "csrc")
EXE = os.path.join(ROOT, "legosnark_amd", "paired_check")


def test_paired_products_and_point_formulas_on_the_device():
    subprocess.check_call(["make", "-C", CSRC, "-s", "../paired_check"], timeout=600)
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:]
    assert "mul2 differs in 0, sqr2 in 0" in r.stdout
    assert r.stdout.count("limbs differ in 0, points in 0") == 3      # mixed addition, head, general addition
