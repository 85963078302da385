"""CPU suite: csrc/ecntt.h, the stage geometry and the per-butterfly body of the group-element transform's kernels
(csrc/ecntt.hip), compiled for the host: tests/cpp/test_ecntt.cc, plain and under ASan + UBSan as a stand-alone program (the
flags and the link probe of test_fr_elem_host.py).  Also, without a GPU: the three entry points are declared and exported,
the Python wrappers exist, ecntt_params() answers, and the argument refusals come back as LSA_ERR_INVALID -- the library
checks them before it asks for a device, so they can be told apart from LSA_ERR_NO_DEVICE here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ecntt.cc")
INCLUDE = ["-I", os.path.join(ROOT, "legosnark_amd", "csrc")]
SANITIZE = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SYMBOLS = ("lsa_g1_ecntt", "lsa_g2_ecntt", "lsa_ecntt_param")
WRAPPERS = ("ecntt", "ecntt_params")
ERR_INVALID = -2
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-3000:]
    return r.stdout


def test_ecntt_header(tmp_path):
    exe = str(tmp_path / "test_ecntt")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *INCLUDE, SRC, "-o", exe])
    out = _run(exe)
    assert "geometry: log_n = 1 .. 10" in out
    assert "G1: 18 inputs, forward and inverse, n = 1, 2, 4, 16" in out and "G2: 18 inputs, forward and inverse, n = 1, 2, 4, 16" in out


@pytest.fixture(scope="module")
def sanitizer_toolchain(tmp_path_factory):
    """Skips only where a one-line program does not LINK with the sanitizer flags (no runtime libraries installed)."""
    d = tmp_path_factory.mktemp("sanitizer_probe")
    src = d / "probe.cc"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *SANITIZE, str(src), "-o", str(d / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here: " + r.stdout[-300:])


def test_ecntt_header_sanitized(tmp_path, sanitizer_toolchain):
    exe = str(tmp_path / "test_ecntt_san")
    subprocess.check_call(["g++", *SANITIZE, *INCLUDE, SRC, "-o", exe])
    _run(exe)


def _library():
    import legosnark_amd
    if not os.path.exists(legosnark_amd.LIB_PATH):
        legosnark_amd.build()
    return legosnark_amd


def test_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "legosnark_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s + " is not declared"
    lsa = _library()
    out = subprocess.run(["nm", "-D", "--defined-only", lsa.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in SYMBOLS if s not in names]
    for w in WRAPPERS:
        assert callable(getattr(lsa, w)), w


def test_ecntt_params_answers_without_a_device():
    lsa = _library()
    p = lsa.ecntt_params()
    assert set(p) == set(lsa.ECNTT_PARAMS)
    assert p["g1_resident_butterflies"] >= 64 and p["g2_resident_butterflies"] >= 64 // p["g2_lanes_per_butterfly"]
    assert p["g1_resident_butterflies"] == p["g2_resident_butterflies"] * p["g2_lanes_per_butterfly"]    # one grid for both
    assert p["max_log_n"] == 24
    assert lsa.lib().lsa_ecntt_param(99) == 0 and lsa.lib().lsa_ecntt_param(-1) == 0


def _mont(x):
    return np.frombuffer((x % R * (1 << 256) % R).to_bytes(32, "little"), dtype=np.uint64).copy()


def _root(log_n):
    w = pow(5, (R - 1) >> 28, R)
    for _ in range(28 - log_n):
        w = w * w % R
    return w


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_refusals_come_before_the_device(group):
    """Null pointers, log_n = 25, a partial overlap and an omega of the wrong order are LSA_ERR_INVALID whether or not a device
    was ever initialised (a valid call without one is LSA_ERR_NO_DEVICE, or runs where a test before this one called lsa_init)."""
    lsa = _library()
    fn = lsa.lib().lsa_g1_ecntt if group == "g1" else lsa.lib().lsa_g2_ecntt
    width = 12 if group == "g1" else 24
    buf = np.zeros((16, width), dtype=np.uint64)
    out = np.zeros((8, width), dtype=np.uint64)
    w8 = _mont(_root(3))
    hp = lambda a, off=0: C.c_void_p(a.ctypes.data + off)  # noqa: E731
    row = width * 8
    calls = {
        "null in": fn(None, hp(out), 3, hp(w8), 0, 0),
        "null out": fn(hp(buf), None, 3, hp(w8), 0, 0),
        "null omega": fn(hp(buf), hp(out), 3, None, 0, 0),
        "null in, device mode": fn(None, hp(out), 3, hp(w8), 0, 1),
        "log_n = 25": fn(hp(buf), hp(out), 25, hp(w8), 0, 0),
        "overlap by one point": fn(hp(buf), hp(buf, row), 3, hp(w8), 0, 0),
        "overlap, out below in": fn(hp(buf, 7 * row), hp(buf), 3, hp(w8), 1, 0),
        "omega of order 4": fn(hp(buf), hp(out), 3, hp(_mont(_root(2))), 0, 0),
        "omega of order 16": fn(hp(buf), hp(out), 3, hp(_mont(_root(4))), 1, 0),
        "omega = 1": fn(hp(buf), hp(out), 3, hp(_mont(1)), 0, 0),
        "omega = 0": fn(hp(buf), hp(out), 3, hp(_mont(0)), 0, 0),
        "one point, omega = -1": fn(hp(buf), hp(out), 0, hp(_mont(R - 1)), 0, 0),
    }
    assert calls == {k: ERR_INVALID for k in calls}
    assert not buf.any() and not out.any()
    assert b"" != lsa.lib().lsa_last_error()
    # the wrapper refuses a length that is no power of two before it calls the library
    with pytest.raises(ValueError):
        lsa.ecntt(group, buf[:6], w8)
