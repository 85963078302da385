"""CPU suite: csrc/fr_elem.h, the per-element and per-run arithmetic of the element-wise Fr vector kernels (csrc/fr_elem.hip),
compiled for the host against fp.h's plain Fr operators: tests/cpp/test_fr_elem.cc, plain and under ASan + UBSan as a stand-alone
program (the flags and the link probe of test_fr_dot_host.py).  Also, without a GPU: the six entry points are declared and
exported, the Python wrappers exist, and fr_vec_params() answers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_fr_elem.cc")
INCLUDE = ["-I", os.path.join(ROOT, "legosnark_amd", "csrc")]
SANITIZE = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SYMBOLS = ("lsa_fr_vec_mul", "lsa_fr_vec_lincomb", "lsa_fr_powers", "lsa_fr_batch_inverse", "lsa_fr_poly_eval", "lsa_fr_vec_param")
WRAPPERS = ("fr_vec_mul", "fr_vec_lincomb", "fr_powers", "fr_batch_inverse", "fr_poly_eval", "fr_vec_params")


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-3000:]
    return r.stdout


def test_fr_elem(tmp_path):
    exe = str(tmp_path / "test_fr_elem")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *INCLUDE, SRC, "-o", exe])
    assert "lincomb max 8, inv run 16, powers run 16, eval items 16, dot max partials 60, group 4" in _run(exe)


@pytest.fixture(scope="module")
def sanitizer_toolchain(tmp_path_factory):
    """Skips only where a one-line program does not LINK with the sanitizer flags (no runtime libraries installed)."""
    d = tmp_path_factory.mktemp("sanitizer_probe")
    src = d / "probe.cc"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *SANITIZE, str(src), "-o", str(d / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here: " + r.stdout[-300:])


def test_fr_elem_sanitized(tmp_path, sanitizer_toolchain):
    exe = str(tmp_path / "test_fr_elem_san")
    subprocess.check_call(["g++", *SANITIZE, *INCLUDE, SRC, "-o", exe])
    _run(exe)


def test_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "legosnark_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s + " is not declared"
    import legosnark_amd
    if not os.path.exists(legosnark_amd.LIB_PATH):
        legosnark_amd.build()
    out = subprocess.run(["nm", "-D", "--defined-only", legosnark_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in SYMBOLS if s not in names]
    for w in WRAPPERS:
        assert callable(getattr(legosnark_amd, w)), w


def test_fr_vec_params_answers_without_a_device():
    import legosnark_amd
    if not os.path.exists(legosnark_amd.LIB_PATH):
        legosnark_amd.build()
    p = legosnark_amd.fr_vec_params()
    assert p["lincomb_max"] == 8 and p["inv_run"] == 16 and p["powers_run"] == 16 and p["eval_items"] == 16
    assert p["eval_block"] == 256 * p["eval_items"]
    assert p["pass_elems"] >= 0                          # (0 until lsa_init has picked a device)
    assert legosnark_amd.lib().lsa_fr_vec_param(99) == 0
