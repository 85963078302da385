"""GPU: tools/w12_rows_check.hip -- the device-only forms of the pairing engines at the limits of their operand contract
("operands < 2p, tight limbs; result < 2p, tight"): the one-phase Fq12 row product w12_rows of csrc/w12.h (product, the
three Frobenius maps, the line product; destination apart from, or aliasing, either operand), the 256-lane final
exponentiation with its helper wavefront, the multiply-add branch of fp29.h's lin2 and tmiller.h's wt_swap / wt_xi_comp.
All of it sits behind __HIP_DEVICE_COMPILE__ -- the host tests run other implementations of the same operations -- and the
C-ABI converts every input with a Montgomery product, so the suite's inputs reach it as pseudo-random canonical limbs.
The program copies RAW limbs (tests/cpp/w12_edge_cases.h: 0, 1, p - 1, p, p + 1, 2p - 1, every low limb 2^29 - 1 below p
and below 2p, v and v + p, one-hot elements) into LDS, runs one call per workgroup and compares canonical values with the
host's tower code, raw results with the contract, lin2 / wt_* limb for limb with the host branch.  A stand-alone program:
no symbol is added to the library.  The library's Makefile has a target for it outside `all`; this test makes that target
(nothing to do where the program is up to date) and runs the program under a time limit of its own."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "legosnark_amd", "csrc")
EXE = os.path.join(ROOT, "legosnark_amd", "w12_rows_check")


def test_row_engine_at_its_operand_limits_on_the_device():
    subprocess.check_call(["make", "-C", CSRC, "-s", "../w12_rows_check"], timeout=600)
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:]
    clean = "values differ in 0, results outside the contract in 0"
    for section in ("rows product: 860 workgroups", "rows frobenius: 324 workgroups", "rows line: 564 workgroups", "final exponentiation: 19 elements (2 of them zero)"):
        line = [l for l in r.stdout.splitlines() if l.startswith(section)]
        assert len(line) == 1 and line[0].endswith(clean), (section, line)
    assert r.stdout.count(clean) == 4
    assert "lin2: 968 lanes" in r.stdout and "limbs differ in 0, results outside the contract in 0" in [l for l in r.stdout.splitlines() if l.startswith("lin2:")][0]
    assert "wt_swap / wt_xi_comp: 256 lanes: swapped limbs differ in 0, xi limbs differ in 0, results outside the contract in 0" in r.stdout
