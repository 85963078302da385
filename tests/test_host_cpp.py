"""CPU suite: host-compiled unit tests of the device arithmetic headers (the same code the
kernels compile): 29-bit-limb field + bound-aware XYZZ formulas against the canonical
32-bit-limb code, and the GLV decomposition (k1 + k2*lambda == k mod r, |k_i| < 2^127)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["test_fp29", "test_glv", "test_fp29x2", "test_tower29", "test_smul", "test_w12", "test_tmiller", "test_inv29", "test_ntt_core", "test_msm_plan", "test_w12_edges", "test_crs_index", "test_g2_table_index", "test_pairing_plan"])
def test_host_cpp(name, tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", name + ".cc")
    if not os.path.exists(src):
        pytest.skip(name + " not present")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "legosnark_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("name", ["test_fp29", "test_fp29x2", "test_tmiller", "test_w12", "test_ntt_core", "test_w12_edges"])
def test_host_cpp_with_the_column_wise_products(name, tmp_path):
    """-DLSA_FP29_COLS / -DLSA_F29_COLS / -DLSA_FR29_COLS select the column-wise forms of the 29-bit-limb products (17
    independent column accumulators instead of one serial multiply-add chain: fs29.h f29_dot_cols, fp29.h redc_cols,
    fr29.h mul).  Round 6 measured them equal to the serial forms on the GPU and left them behind these switches; they must
    stay the same functions: every host test of the field, tower, Miller and NTT code passes with them too."""
    src = os.path.join(ROOT, "tests", "cpp", name + ".cc")
    exe = str(tmp_path / (name + "_cols"))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-DLSA_FP29_COLS", "-DLSA_F29_COLS", "-DLSA_FR29_COLS", "-I", os.path.join(ROOT, "legosnark_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("name", ["test_fp29", "test_glv", "test_tower29"])
def test_host_cpp_with_the_32_bit_limb_product(name, tmp_path):
    """On the host Fp's Montgomery product runs on four 64-bit limbs; the device compiles the
    32-bit-limb CIOS.  LSA_FP_HOST32 forces the device variant on the host: the same tests must
    pass with either, i.e. both agree with the independent 29-bit-limb code and the integer
    identities."""
    src = os.path.join(ROOT, "tests", "cpp", name + ".cc")
    exe = str(tmp_path / (name + "_32"))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-DLSA_FP_HOST32", "-I", os.path.join(ROOT, "legosnark_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-2000:]


def test_host_64_bit_limbs_agree_with_the_device_limbs(tmp_path):
    """fp.h on the host: four 64-bit limbs, carry intrinsics, binary-Euclid inverse (what the reference's own host
    loops run on through the shim).  The device variant (-DLSA_FP_HOST32: eight 32-bit limbs, Fermat inverse) must
    print the same digests over the same operand sequence, edge values included."""
    src = os.path.join(ROOT, "tests", "cpp", "test_fp_host.cc")
    outs = []
    for tag, flags in (("64", []), ("32", ["-DLSA_FP_HOST32"])):
        exe = str(tmp_path / ("test_fp_host_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-O2", *flags, "-I", os.path.join(ROOT, "legosnark_amd", "csrc"), src, "-o", exe])
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1] and outs[0].count("inv ") == 2


# ---- the same programs under AddressSanitizer + UndefinedBehaviorSanitizer ------------------------------------------
# The headers under csrc/ are device code as well: what is undefined behaviour on the host (a shift of a negative value,
# an out-of-range index into a limb array) is undefined in the kernels too, where nothing reports it.  Pure host code
# only: the two programs that link the HIP library (test_shim_io.cc, test_shim_domains.cc) stay out of this tier.
SANITIZE = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
_HEADER_TESTS = ["test_fp29", "test_glv", "test_fp29x2", "test_tower29", "test_smul", "test_w12", "test_tmiller", "test_inv29", "test_ntt_core", "test_msm_plan", "test_w12_edges", "test_crs_index", "test_g2_table_index", "test_pairing_plan"]
_COLS = ["-DLSA_FP29_COLS", "-DLSA_F29_COLS", "-DLSA_FR29_COLS"]
SANITIZED_PROGRAMS = ([(n, n, []) for n in _HEADER_TESTS]
                      + [(n + "_cols", n, _COLS) for n in ["test_fp29", "test_fp29x2", "test_tmiller", "test_w12", "test_ntt_core", "test_w12_edges"]]
                      + [(n + "_32", n, ["-DLSA_FP_HOST32"]) for n in ["test_fp29", "test_glv", "test_tower29"]]
                      + [("test_fp_host_64", "test_fp_host", []), ("test_fp_host_32", "test_fp_host", ["-DLSA_FP_HOST32"])])


@pytest.fixture(scope="module")
def sanitizer_toolchain(tmp_path_factory):
    """Skips only where a one-line program does not LINK with the sanitizer flags (no runtime libraries installed)."""
    d = tmp_path_factory.mktemp("sanitizer_probe")
    src = d / "probe.cc"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *SANITIZE, str(src), "-o", str(d / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here: " + r.stdout[-300:])


@pytest.mark.parametrize("tag,name,defines", SANITIZED_PROGRAMS, ids=[p[0] for p in SANITIZED_PROGRAMS])
def test_host_cpp_sanitized(tag, name, defines, tmp_path, sanitizer_toolchain):
    """Every program of this file again with ASan + UBSan, any report fatal: exit status 0 and PASS."""
    src = os.path.join(ROOT, "tests", "cpp", name + ".cc")
    exe = str(tmp_path / (tag + "_san"))
    subprocess.check_call(["g++", *SANITIZE, "-pthread", *defines, "-I", os.path.join(ROOT, "legosnark_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-3000:]


def test_hash_pool_under_thread_sanitizer(tmp_path):
    """csrc/hash_pool.h is the library's one piece of hand-written thread code (mutex, condition variables, a generation
    counter, restarted by lsa_shutdown -> lsa_init): tests/cpp/test_crs_index.cc as a stand-alone program built with
    ThreadSanitizer reports nothing.  Skips only where a one-line program does not link with -fsanitize=thread."""
    tsan = ["-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread"]
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *tsan, str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link with -fsanitize=thread here: " + r.stdout[-300:])
    exe = str(tmp_path / "test_crs_index_tsan")
    subprocess.check_call(["g++", *tsan, "-I", os.path.join(ROOT, "legosnark_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_crs_index.cc"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "PASS" in r.stdout and "ThreadSanitizer" not in r.stdout, r.stdout[-3000:]


def test_oracle_under_ubsan_passes_the_cpu_vector_tests(tmp_path, sanitizer_toolchain):
    """oracle/bn254.c is the checker of every parity test: built with UBSan (any report fatal) it must still pass its own
    golden vectors and the public EVM vectors.  A child pytest loads that build through LSA_ORACLE_LIB (oracle_lib.build).
    UBSan only: ASan inside a library loaded by an uninstrumented interpreter would need its runtime preloaded."""
    import sys
    so = str(tmp_path / "liboracle_bn254_ubsan.so")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-fPIC", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-shared",
                           "-o", so, os.path.join(ROOT, "oracle", "bn254.c"), "-lpthread"])
    env = dict(os.environ, LSA_ORACLE_LIB=so)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "not gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_oracle_golden.py"), os.path.join(ROOT, "tests", "test_public_vectors.py")],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stdout


def test_frobenius_row_constants_are_the_generators_output():
    """csrc/frob_rows.h is generated (tools/gen_frob_rows.py: the Frobenius factors of bn254_constants.h multiplied out,
    conjugation and signs folded in, 29-bit-limb Montgomery form); the committed table must be what the script prints,
    and must satisfy gamma_(P,k) = FROB6_C{k>>1}[P] * (k odd ? FROB12_C1[P] : 1) against the oracle's Fq2 arithmetic."""
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "gen_frob_rows.py")], cwd=root, capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(root, "legosnark_amd", "csrc", "frob_rows.h")).read()
    want = re.findall(r"0x[0-9a-f]{8}u", out)
    got = re.findall(r"0x[0-9a-f]{8}u", header)
    assert len(want) == 3 * 6 * 2 * 2 * 9 and got == want
    # spot value: power 2, k = 0 is the identity map: rows (1, -0) / (0, 1) in Montgomery form R = 2^261
    p = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    one = (1 << 261) % p
    limbs = [int(x[2:-1], 16) for x in want]
    base = ((1 * 6 + 0) * 2 + 0) * 2 * 9                      # [power - 1 = 1][k = 0][part 0][h 0]
    assert sum(l << (29 * i) for i, l in enumerate(limbs[base:base + 9])) == one
    assert all(l == 0 for l in limbs[base + 9:base + 18])       # -g1 = 0


def test_final_exponentiation_scalar_exponent_is_the_generators_output():
    """csrc/w12.h: W12_FE_SCALAR_EXP is generated (tools/gen_fe_scalar_exponent.py walks libff's final-exponentiation chain
    symbolically, with conjugations NOT changing the sign of a stray Fq factor, and checks on the big-int model that the
    chain without its inversion, times n1^e, is f^(libff's exponent)); the committed words must be what the script prints."""
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "gen_fe_scalar_exponent.py")], cwd=root, capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(root, "legosnark_amd", "csrc", "w12.h")).read()
    want = re.search(r"W12_FE_SCALAR_EXP\[8\] = \{([^}]*)\}", out).group(1)
    got = re.search(r"W12_FE_SCALAR_EXP\[8\] = \{([^}]*)\}", header).group(1)
    assert got == want
    bits = re.search(r"W12_FE_SCALAR_EXP_BITS = (\d+)", out).group(1)
    assert re.search(r"W12_FE_SCALAR_EXP_BITS = (\d+)", header).group(1) == bits == "254"
    # e < q - 1, and the chain has the links to run it: 264 row products follow the norm (w12.h: w12_final_exponentiation_h)
    words = [int(x.strip()[:-1], 16) for x in want.split(",")]
    e = sum(w << (32 * i) for i, w in enumerate(words))
    q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    assert 0 < e < q - 1 and e.bit_length() == 254
