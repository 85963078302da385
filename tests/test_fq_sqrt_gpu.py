"""GPU: tools/fq_sqrt_check.hip -- the device compilation of csrc/fq_sqrt.h (fq_sqrt, fq2_sqrt, g2_in_subgroup) against the
host compilation, on the operand list tests/cpp/test_fq_sqrt.cc checks on the host against Euler's criterion and [r]P == O
(tests/cpp/fq_sqrt_cases.h): verdicts and canonical root words one for one.  The a1 == 0 branches of fq2_sqrt are not
reachable through curve points, so this is where they run on the device.  A stand-alone program: no symbol is added to the
library.  The library's Makefile has a target for it outside `all`; this test makes that target (nothing to do where the
program is up to date) and runs the program under a time limit of its own."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "legosnark_amd", "csrc")
EXE = os.path.join(ROOT, "legosnark_amd", "fq_sqrt_check")


def test_device_roots_and_subgroup_verdicts_equal_the_hosts():
    subprocess.check_call(["make", "-C", CSRC, "-s", "../fq_sqrt_check"], timeout=600)
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:]
    lines = r.stdout.splitlines()
    fq = [l for l in lines if l.startswith("fq_sqrt:")]
    fq2 = [l for l in lines if l.startswith("fq2_sqrt:")]
    sub = [l for l in lines if l.startswith("g2_in_subgroup:")]
    assert len(fq) == 1 and fq[0].endswith("verdicts or words differ in 0")
    assert len(fq2) == 1 and fq2[0].endswith("verdicts or words differ in 0") and "(19 with a1 == 0," in fq2[0]
    assert sub == ["g2_in_subgroup: 42 points, 20 in G2: verdicts differ in 0"]
