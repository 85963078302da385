"""CPU suite: csrc/smul_g2.h, the per-item body of the G2 scalar-multiplication kernel, compiled for the host with the
one-lane Fq2 type and run against plain double-and-add (tests/cpp/test_smul_g2.cc), once with -O2 and once as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, as tests/test_host_cpp.py does for its programs.

The program's two special bases come from the big-integer model, so that the C++ file holds no magic constants: the first
point (i + u, y) of the twist, which lies outside the order-r subgroup, and T = [r (2p - r) / 10069] S, a twist point of
order 10069 whose small multiples collide with the ladder's table entries."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "pymodel"))
import bn254_model as m  # noqa: E402

SMALL_ORDER = 10069
SANITIZE = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def fq_sqrt(a):
    r = pow(a, (m.P + 1) // 4, m.P)
    return r if r * r % m.P == a % m.P else None


def f2_sqrt(a):
    a0, a1 = a
    sn = fq_sqrt((a0 * a0 + a1 * a1) % m.P)
    if sn is None:
        return None
    for s in (sn, -sn):
        x0 = fq_sqrt((a0 + s) * m.inv(2) % m.P)
        if x0:
            y = (x0, a1 * m.inv(2 * x0) % m.P)
            if m.f2_sqr(y) == (a0 % m.P, a1 % m.P):
                return y
    return None


def twist_ladder(p, k):
    """[k]p on the whole twist, k not reduced (bn254_model.g2_mul reduces mod r)."""
    acc = None
    for bit in bin(k)[2:]:
        acc = m.g2_add(acc, acc)
        if bit == "1":
            acc = m.g2_add(acc, p)
    return acc


def special_points():
    order = m.R * (2 * m.P - m.R)
    assert order % SMALL_ORDER == 0
    outside = small = None
    i = 1
    while outside is None or small is None:
        x = (i, 1)
        y = f2_sqrt(m.f2_add(m.f2_mul(m.f2_sqr(x), x), m.TWIST_B))
        i += 1
        if y is None:
            continue
        s = (x, y)
        assert m.g2_is_on_curve(s)
        if outside is None and twist_ladder(s, m.R) is not None:
            outside = s
        if small is None:
            t = twist_ladder(s, order // SMALL_ORDER)
            if t is not None:
                assert twist_ladder(t, SMALL_ORDER) is None
                small = t
    return outside, small


@pytest.fixture(scope="module")
def point_args():
    outside, small = special_points()
    return ["%x" % c for pt in (outside, small) for coord in pt for c in coord]


def run(exe, args):
    r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-3000:]
    assert "2000 random scalars" in r.stdout


def test_smul_g2_host(tmp_path, point_args):
    src = os.path.join(ROOT, "tests", "cpp", "test_smul_g2.cc")
    exe = str(tmp_path / "test_smul_g2")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "legosnark_amd", "csrc"), src, "-o", exe])
    run(exe, point_args)


def test_smul_g2_host_sanitized(tmp_path, point_args):
    """The same program with ASan + UBSan, any report fatal.  Skips only where a one-line program does not LINK with the
    sanitizer flags (no runtime libraries installed)."""
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *SANITIZE, str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here: " + r.stdout[-300:])
    src = os.path.join(ROOT, "tests", "cpp", "test_smul_g2.cc")
    exe = str(tmp_path / "test_smul_g2_san")
    subprocess.check_call(["g++", *SANITIZE, "-I", os.path.join(ROOT, "legosnark_amd", "csrc"), src, "-o", exe])
    run(exe, point_args)
