"""Crafted limbs through the C-ABI.  Every pairing kernel converts its inputs with F29::from_mont256 -- a Montgomery product by
2^266 mod p -- so the suite's "edge" inputs (0, 1, subfield elements) reach the 29-bit-limb engines as pseudo-random limbs.
The conversion can be steered: for the 256-bit input x = t * 32^-1 mod p it returns t itself (x * 2^266 / 2^261 = 32 x), exactly
the limbs of t for t = 0x30644d * 2^232 + (2^232 - 1) (every low limb 2^29 - 1, still below p) and for t = p - 1, and the
non-canonical t + p for small t (1, 2^232 - 1).  The CPU test below pins that with csrc/fp29.h compiled for the host; the GPU
tests feed such inputs, all valid canonical field elements, to lsa.fq12_product (k_fq12_prod8_wave and its second level),
lsa.final_exponentiation (both kernels) and lsa.miller_loop (every kernel) and compare byte for byte with the oracle.
tools/w12_rows_check.hip drives the same limb patterns into the row engine directly."""
import os
import subprocess
import sys

import numpy as np
import pytest

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV32 = pow(32, -1, P)
MASK29 = (1 << 29) - 1
TMAX = (0x30644D << 232) + (1 << 232) - 1          # every low limb 2^29 - 1, top limb one under p's
SMALL = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233]


def preimage(t):
    """The four 64-bit words of x = t * 32^-1 mod p: the canonical input that from_mont256 turns into t (or t + p)."""
    x = t % P * INV32 % P
    return np.array([(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def limbs29(v):
    return [(v >> (29 * i)) & MASK29 for i in range(8)] + [v >> 232]


def element(ts):
    """An Fq12 element (48 words) whose twelve components are the preimages of ts."""
    assert len(ts) == 12
    return np.concatenate([preimage(t) for t in ts])


def crafted_elements():
    """tight maximum / p - 1 / 2^232 - 1 in every component, twelve small t (they enter as t + p), mixes with random components."""
    import random
    rng = random.Random(20261019)
    rand = lambda: rng.randrange(P)
    els = {
        "tmax": element([TMAX] * 12),
        "pm1": element([P - 1] * 12),
        "low232": element([(1 << 232) - 1] * 12),
        "small": element(SMALL),
        "mix_tmax": element([TMAX if i % 2 else rand() for i in range(12)]),
        "mix_small": element([SMALL[i] if i % 3 == 0 else (P - 1 if i % 3 == 1 else rand()) for i in range(12)]),
        "one_hot_tmax": element([TMAX if i == 7 else 0 for i in range(12)]),
        "random": element([rand() for _ in range(12)]),
    }
    return els


def test_preimage_limbs_on_the_host(tmp_path):
    """fp29.h compiled for the host: from_mont256(preimage(t)) is exactly t for the tight maximum below p and for p - 1, exactly
    t + p for t = 1 and t = 2^232 - 1 (and for the small values the GPU cases use), and t or t + p, tight, for random t."""
    import random
    exe = str(tmp_path / "from_mont256_limbs")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "legosnark_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "from_mont256_limbs.cc"), "-o", exe])
    rng = random.Random(7)
    exact = [TMAX, P - 1]
    plus_p = [1, (1 << 232) - 1] + SMALL
    rand = [rng.randrange(P) for _ in range(64)]
    ts = exact + plus_p + rand
    args = ["%064x" % (t * INV32 % P) for t in ts]
    out = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60, check=True).stdout.split("\n")
    got = [[int(w, 16) for w in line.split()] for line in out if line]
    assert len(got) == len(ts)
    assert limbs29(TMAX) == [MASK29] * 8 + [0x30644D] and TMAX < P
    for t, g in zip(ts, got):
        assert all(l <= MASK29 for l in g[:8])
        if t in exact:
            assert g == limbs29(t), hex(t)
        elif t in plus_p:
            assert g == limbs29(t + P), hex(t)
        else:
            assert g in (limbs29(t), limbs29(t + P)), hex(t)


_CHILD = (
    "import sys, numpy as np\n"
    "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import legosnark_amd as lsa, oracle_lib as o\n"
    "import test_pairing_edges_gpu as t\n"
    "lsa.init(0)\n"
)


def _run_child(body, env):
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests")) + body + "print('OK')\n"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
def test_fq12_product_of_crafted_elements(lsa):
    """Groups of 2, 8 and 9 factors (one workgroup's chain of row products; 9: a second level) built from the crafted elements."""
    import oracle_lib as o
    e = crafted_elements()
    groups = [
        ["tmax", "tmax"], ["tmax", "pm1"], ["small", "small"], ["small", "tmax"], ["low232", "pm1"], ["mix_tmax", "mix_small"], ["one_hot_tmax", "random"],
        ["tmax", "pm1", "small", "low232", "mix_tmax", "mix_small", "random", "tmax"],
        ["tmax"] * 8,
        ["small", "pm1", "tmax", "low232", "mix_small", "one_hot_tmax", "mix_tmax", "random", "small"],
        ["pm1"] * 9,
    ]
    for names in groups:
        fs = np.stack([e[n] for n in names])
        assert np.array_equal(lsa.fq12_product(fs).reshape(-1), o.fq12_product(fs).reshape(-1)), names


@pytest.mark.gpu
@pytest.mark.parametrize("helper", ["1", "0"])
def test_final_exponentiation_of_crafted_elements(helper):
    """LSA_FE_HELPER=1: the 256-lane kernel with the helper wavefront, 0: the 192-lane kernel; each in its own process."""
    body = (
        "e = t.crafted_elements()\n"
        "fs = np.stack([e[n] for n in sorted(e)])\n"
        "got = lsa.final_exponentiation(fs)\n"
        "for i, n in enumerate(sorted(e)):\n"
        "    assert np.array_equal(got[i].reshape(-1), o.final_exponentiation(fs[i]).reshape(-1)), n\n"
    )
    _run_child(body, {"LSA_FE_HELPER": helper})


def crafted_points():
    """P = (x, y, 1), Q = ((x0, x1), (y0, y1), (1, 0)) with coordinates from the preimages: off the curves, but the step formulas
    are plain field arithmetic and libff's loop defines a value for any coordinates."""
    import oracle_lib as o
    one = o.fq_mont(1)
    zero = np.zeros(4, dtype=np.uint64)
    coords = [
        ([TMAX, TMAX], [TMAX, TMAX, TMAX, TMAX]),
        ([P - 1, P - 1], [P - 1, P - 1, P - 1, P - 1]),
        ([1, 2], [3, 5, 8, 13]),
        ([TMAX, 1], [P - 1, TMAX, 2, (1 << 232) - 1]),
        ([(1 << 232) - 1, P - 1], [TMAX, 1, P - 1, TMAX]),
    ]
    ps = np.stack([np.concatenate([preimage(a), preimage(b), one]) for (a, b), _ in coords])
    qs = np.stack([np.concatenate([preimage(q[0]), preimage(q[1]), preimage(q[2]), preimage(q[3]), one, zero]) for _, q in coords])
    return ps, qs


def test_oracle_accepts_the_crafted_points():
    """The oracle's loop takes the off-curve coordinates and gives a value that depends on them (no rejection, no constant)."""
    import oracle_lib as o
    ps, qs = crafted_points()
    f = o.miller_loop_batch(ps, qs)
    assert f.shape == (len(ps), 48) and len({f[i].tobytes() for i in range(len(ps))}) == len(ps)
    assert all(f[i].any() for i in range(len(ps)))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["default", "3", "5", "6"])
def test_miller_loop_on_crafted_coordinates(kernel):
    """Every Miller-loop path (LSA_MILLER_KERNEL: 3 one pairing per lane, 5 line tables, 6 fused; unset: the default choice) on the
    crafted coordinates, alone and between ordinary pairs, byte for byte against the oracle."""
    body = (
        "ps, qs = t.crafted_points()\n"
        "assert np.array_equal(lsa.miller_loop(ps, qs), o.miller_loop_batch(ps, qs))\n"
        "gp = o.arith_bases('g1', 77, 5, 7); gq = o.arith_bases('g2', 99, 7, 7)\n"
        "ps2 = np.concatenate([gp[:3], ps, gp[3:]]); qs2 = np.concatenate([gq[:3], qs, gq[3:]])\n"
        "assert np.array_equal(lsa.miller_loop(ps2, qs2), o.miller_loop_batch(ps2, qs2))\n"
    )
    _run_child(body, {} if kernel == "default" else {"LSA_MILLER_KERNEL": kernel})
