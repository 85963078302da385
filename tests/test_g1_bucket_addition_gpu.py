"""GPU: the G1 bucket accumulation (k_accumulate<CurveG1, 1>, k_accumulate_heavy, the plain path's two-lane kernel and the
compact pipeline's kernel, which all share CurveG1::madd) after the change of its arithmetic: the head of every bucket
list added as affine + affine, the sign folded into the addition, two carry passes skipped.

n = 2^16 is the smallest call on the wide-digit path that runs the one-lane kernel, and a G1 handle of 2^16 points
carries the pre-shifted copies by default.  By default such a call takes the compact four-launch pipeline; LSA_NO_COMPACT
sends it to the general one, and the library reads that switch once per process, so the five wide cases run together in
ONE interpreter of their own (as tests/test_sort_paths_gpu.py does for its switch).  Every result is compared, after
affine normalisation, with the oracle's multiple of the generator by the known discrete logarithm sum_i s_i * k_i (the
bases are k_i * G); the plain path also with the oracle's own multi-exponentiation.

Each case runs under a limit of its own: a watchdog (faulthandler.dump_traceback_later(..., exit=True)) that ends the
process a case runs in even when a call into the library does not return.  In the child interpreter that is the child;
the test that waits for it arms none itself and relies on subprocess's timeout, which kills the child."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R
N = 1 << 16
A0, B0 = 0x1F2E3D4C5B6A7988 << 60 | 0x11, 0x9E3779B97F4A7C15 << 20 | 0x3
LIMIT_S = 120
CASES = ["uniform", "one_value", "small_signed", "short_lists", "infinity_positions"]


@pytest.fixture
def watchdog():
    """for the tests that call the library in THIS process"""
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def canon(pt):
    return o.g1_canonical_affine(pt)


def expected(scalars, dlogs):
    k = sum(s * d for s, d in zip(scalars, dlogs)) % R
    return canon(o.g1_mul(o.generator("g1"), o.fr_mont(k)))


def run_wide(lsa, bases, scalars):
    """One blocking MSM of 2^16 pairs over a handle that carries the copies."""
    import torch
    assert len(bases) == N and len(scalars) == N
    lsa.set_table_threshold(0)
    B = lsa.Bases("g1", bases)
    try:
        assert B.has_table()
        d_s = torch.from_numpy(o.fr_mont_array(scalars).view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        return canon(B.msm(d_s))
    finally:
        B.close()


def progression():
    """k_i = A0 + i * B0 and the points k_i * G."""
    return o.arith_bases("g1", A0, B0, N), [(A0 + i * B0) % R for i in range(N)]


def triples(m):
    """P_i, -P_i and the discrete logarithms k_i of m points: -(a + i b) = (r - a) + i (r - b) is a progression too."""
    pts = o.arith_bases("g1", A0 + 5, B0, m)
    neg = o.arith_bases("g1", R - (A0 + 5), R - B0, m)
    return pts, neg, [(A0 + 5 + i * B0) % R for i in range(m)]


def shared_scalars(seed):
    """one uniform scalar for every group of three consecutive bases: its three entries share their buckets, mostly alone
    (2^16 / 3 groups x 13 digits over 2^19 buckets), so the lists have one to three entries and a few more"""
    _, group_sc = o.random_scalars(N // 3 + 1, seed=seed)
    return [s for s in group_sc for _ in range(3)][:N]


def build_case(name, prog):
    """-> (bases, scalars, discrete logarithms of the bases), 2^16 of each"""
    bases, dlogs = prog
    if name == "uniform":
        return bases, o.random_scalars(N, seed=20261018)[1], dlogs
    if name == "one_value":
        # every entry of a window in ONE bucket: all lists long, all through k_heavy_plan / k_accumulate_heavy
        return bases, [0x0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F % R] * N, dlogs
    m = N // 3 + 2
    pts, neg, k = triples(m)
    if name == "small_signed":
        # scalars from {1, r-1, 2, r-2} over bases in which every point appears twice and once negated: equal and opposite
        # points meet in the same buckets
        b = np.stack([pts, pts, neg], axis=1).reshape(-1, 12)[:N]
        dl = [d for ki in k for d in (ki, ki, R - ki)][:N]
        rng = np.random.default_rng(7)
        return b, [(1, R - 1, 2, R - 2)[int(c)] for c in rng.integers(0, 4, size=N)], dl
    if name == "short_lists":
        # (P, P, -P): the head doubles, the third entry takes one P back.  (P, -P, P): the head cancels and the third entry
        # lands on an infinity accumulator.  (P, Q, -Q) / (P, Q, -P): the third entry undoes the second / the first.
        rows, dl = [], []
        for i in range(m - 1):
            P_, Pn, Q_, Qn, kp, kq = pts[i], neg[i], pts[i + 1], neg[i + 1], k[i], k[i + 1]
            group = ((P_, kp), (P_, kp), (Pn, R - kp)), ((P_, kp), (Pn, R - kp), (P_, kp)), ((P_, kp), (Q_, kq), (Qn, R - kq)), ((P_, kp), (Q_, kq), (Pn, R - kp))
            for row, d in group[i % 4]:
                rows.append(row)
                dl.append(d)
        return np.array(rows[:N], dtype=np.uint64), shared_scalars(99), dl[:N]
    if name == "infinity_positions":
        # the infinity point is the first, the second or the third of its group in turn (and some groups are all
        # infinity): whichever order the sort leaves a bucket's entries in, infinity bases stand at list positions 0, 1, 2
        b, dl = bases.copy(), list(dlogs)
        for g in range(N // 3):
            where = g % 4
            for j in ([where] if where < 3 else ([0, 1, 2] if g % 16 == 3 else [])):
                b[3 * g + j] = 0
                dl[3 * g + j] = 0
        return b, shared_scalars(123), dl
    raise KeyError(name)


SNIPPET = r"""
import faulthandler, json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import legosnark_amd as lsa
import test_g1_bucket_addition_gpu as T
faulthandler.dump_traceback_later(T.LIMIT_S, exit=True)      # set-up under a limit too
lsa.init(0)
prog = T.progression()
out = {}
for name in T.CASES:
    faulthandler.dump_traceback_later(T.LIMIT_S, exit=True)  # re-arms: each case has its own limit
    bases, sc, dlogs = T.build_case(name, prog)
    out[name] = T.run_wide(lsa, bases, sc) == T.expected(sc, dlogs)
    faulthandler.cancel_dump_traceback_later()
    print("CASE", name, out[name], flush=True)
print("RESULT " + json.dumps(out))
"""


def test_wide_path_one_lane_kernel_and_heavy_kernels():
    """The five cases at n = 2^16 on the general wide-digit pipeline: k_accumulate<CurveG1, 1>; 'one_value' and
    'small_signed' put (nearly) everything into heavy buckets."""
    env = dict(os.environ, LSA_NO_COMPACT="1")
    r = subprocess.run([sys.executable, "-c", SNIPPET % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=(len(CASES) + 1) * LIMIT_S + 60)
    assert r.returncode == 0, r.stdout[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert set(out) == set(CASES)
    for name in CASES:
        assert out[name], name


@pytest.mark.parametrize("name", ["short_lists", "infinity_positions"])
def test_compact_pipeline_shares_the_addition(lsa, watchdog, name):
    """The same call in this process takes the compact four-launch pipeline, whose kernel calls CurveG1::madd too."""
    bases, sc, dlogs = build_case(name, progression())
    assert run_wide(lsa, bases, sc) == expected(sc, dlogs)


def test_plain_glv_path_keeps_the_endomorphism(lsa, watchdog):
    """n = 4096 without the copies: GLV halves, two lanes per bucket, entries with the endo bit."""
    import torch
    n = 4096
    bases = o.arith_bases("g1", A0, B0, n)
    lsa.set_table_threshold(1 << 30)
    try:
        B = lsa.Bases("g1", bases)
        assert not B.has_table()
        mont, sc = o.random_scalars(n, seed=4096)
        d_s = torch.from_numpy(mont.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        got = canon(B.msm(d_s))
        B.close()
    finally:
        lsa.set_table_threshold(0)
    assert got == expected(sc, [(A0 + i * B0) % R for i in range(n)])
    assert got == canon(o.multi_exp("g1", bases, mont, mode="mixed"))
