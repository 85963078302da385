"""GPU: lsa_shutdown frees every staging buffer the calls grew, and the library works again after a second lsa_init.

Every grow-only staging buffer (csrc/staging.h: StageBuf) links itself into one list that lsa_shutdown walks.  A fresh
child process (the session's library, tests/conftest.py, must stay up for the other tests) runs init -> one host-buffer
call of every family -> shutdown twice, with LSA_TRACE=2 (one `stage_grow A -> B bytes` line on stderr per growth) and
LSA_WARM=0 (no staging allocated by lsa_init).  Each call runs at the smallest shape that reaches every staging buffer its
family owns.

  * Every result of cycle 1 equals the reference of the fixed-shape tests of that call (the oracle, Python integers, the
    big-integer model: the helpers are imported from those test modules), and every result of cycle 2 equals cycle 1's
    (byte for byte; group elements as points -- an MSM's Jacobian representative is not the same in every run).
  * Call by call, the growth lines of cycle 2 are those of cycle 1.  Cycle 1 starts from a fresh process, so each buffer's
    first growth there starts at 0: a buffer that shutdown did not free (or freed without resetting its capacity) has no
    such line in cycle 2.
  * At least REACHED_BUFFERS growths from 0 per cycle, so the comparison above is not one of two empty lists.
"""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The staging buffers the calls of CHILD reach in host mode, from the code (csrc/*.hip); fr_fold, fr_scale_upper, the
# scalar multiplications and the sparse-matrix MSM stage in per-call allocations (DevBuf) and grow nothing.
REACHED = {
    "fr_ntt": ["g_stage_ntt_tmp", "g_stage_ntt_a"],                                   # (the second buffer: above 2^10 points only)
    "cppoly_witness": ["g_stage_fr_tmp", "g_stage_fr_v", "g_stage_fr_r", "g_stage_fr_w"],
    "sumcheck_round": ["g_stage_sc_partial", "g_stage_sc_out"],
    "matvec_sliced": ["g_mat_limbs", "g_mat_part", "g_mat_a", "g_mat_b", "g_mat_c"],  # (g_mat_part: a plan with slices only)
    "quotient_basic": ["g_poly_b", "g_poly_c", "g_poly_h"],
    "quotient_step": ["g_poly_tmp", "g_poly_ztab"],                                  # (up to 2^10 points the basic domain needs neither)
    "sparse_matvec_1": ["g_sp_part", "g_sp_x", "g_sp_out"],                           # (g_sp_part: a row longer than short_max)
    "qap_witness": ["g_sp_h", "g_sp_abc[0]", "g_sp_abc[1]", "g_sp_abc[2]"],
    "decompress_g1": ["g_pl_in", "g_pl_flags", "g_pl_out", "g_pl_status", "g_pl_count"],
    "compress_g1": ["g_pl_aff"],
    # (a first-seen Q: the fused kernel; one product of one pair is exponentiated into pinned memory, g_pair_o stays empty)
    "pairing": ["g_pair_meta", "g_pair_scratch_tabs", "g_pair_f", "g_pair_s", "g_pair_p", "g_pair_q"],
    # (through the CRS cache: bases_create stages the points, and a G1 entry gets its prefix table at the first request)
    "msm_g1": ["g_stage_scalars", "g_stage_jac", "g_stage_prefix_scratch"],
}
REACHED_BUFFERS = sum(len(v) for v in REACHED.values())
assert REACHED_BUFFERS == 40

# Measured on an MI355X machine, before and after the staging list became one registry: the child alone takes 3.0 - 3.3 s
# (two library start-ups, 2 s of reference side, a few hundred milliseconds of GPU work), the test 4.9 - 5.5 s; the
# child's time limit is three times the latter.
TEST_SECONDS = 5
CHILD_TIMEOUT = 3 * TEST_SECONDS

CHILD = r"""
import json, os, random, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import legosnark_amd as lsa
import oracle_lib as o
import fuzz_parity as fz
h = fz.helpers()
lip, sp, pl = h.lip, h.sp, h.pl
R = o.R
rng = random.Random(20261021)
words, fr_raw = fz.words, fz.fr_raw

def fr(n):
    return o.random_scalars(n, seed=rng.randrange(1 << 30))[0]

calls = []          # (name, the call, the reference, how to compare: exact bytes, or as affine points for Jacobian results)
same = lambda got, want: fz.same(got, want)
def add(name, call, want, eq=same):
    calls.append((name, call, want, eq))

# ---- Fr vectors and transforms
a11, w11 = fr(1 << 11), o.fr_mont(o.fr_root_of_unity(11))
add("fr_ntt", lambda: lsa.fr_ntt(a11, w11), o.fr_domain_transform(a11, w11))
a42, w5 = fr(16 + 4), o.fr_mont(o.fr_root_of_unity(5))
add("fr_ntt_step", lambda: lsa.fr_ntt_step(a42, 4, 2, w5), o.fr_step_domain_transform(a42, 4, 2, w5))
v4, r4 = fr(16), fr(4)
add("cppoly_witness", lambda: lsa.cppoly_witness(v4, r4), o.fr_cppoly_witness(v4, r4))
add("eval_mle", lambda: lsa.eval_mle(v4, r4), o.fr_eval_mle(v4, r4))
r3 = fr(3)
add("eq_table", lambda: lsa.fr_eq_table(r3, 0), o.fr_eq_table(r3))
v16, k1 = fr(16), fr(1)[0]
add("fr_fold", lambda: lsa.fr_fold(v16, k1), o.fr_push_randomness(v16, k1))
add("fr_scale_upper", lambda: lsa.fr_scale_upper(v16, k1), o.fr_scale_upper(v16, k1))
tabs, suff, pre, rho = [fr(16), fr(16)], fr(8), fr(1)[0], fr(1)[0]
add("sumcheck_round", lambda: lsa.sumcheck_round(tabs, suff=suff, pre=pre, rho_j=rho), o.fr_sumcheck_round(tabs, suff=suff, pre=pre, rho_j=rho))

# ---- Fr matrices
M1, W1 = fr_raw(rng, 16 * 512), fr_raw(rng, 512)
m1, x1 = words(M1), words(W1)
add("matvec_sliced", lambda: lsa.fr_matvec(m1, x1, 16, 512, 1), fz.matvec_words(M1, W1, 16, 512, 1))
M2, W2 = fr_raw(rng, 64), fr_raw(rng, 8)
m2, x2 = words(M2), words(W2)
for side in (0, 1):
    add("matvec_8x8_side%%d" %% side, lambda side=side: lsa.fr_matvec(m2, x2, 8, 8, side), fz.matvec_words(M2, W2, 8, 8, side))
A3, B3 = fr_raw(rng, 64), fr_raw(rng, 64)
a3, b3 = words(A3), words(B3)
add("matmul", lambda: lsa.fr_matmul(a3, b3, 8, 8, 8), fz.matmul_words(A3, B3, 8, 8, 8))

# ---- the Lipmaa quotient and the Lagrange row, basic and step domain
for name, key in (("basic", (4, None)), ("step", (4, 2))):
    D = lip.dom(key)
    qa, qb, qc = (words(fr_raw(rng, D.m)) for _ in range(3))
    d = [rng.randrange(R) for _ in range(3)]
    t = rng.randrange(R)
    add("quotient_" + name, lambda D=D, qa=qa, qb=qb, qc=qc, d=d: lsa.fr_hadamard_quotient(qa, qb, qc, lip.enc(d), D.big_log, D.small_log, omega=D.w, coset=o.fr_mont(lip.G)),
        lip.expected_h(D, qa, qb, qc, d))
    add("lagrange_" + name, lambda D=D, t=t: lsa.fr_lagrange(D.big_log, D.small_log, D.w, o.fr_mont(t)), lip.enc(lip.lagrange_closed(D, t)))

# ---- sparse Fr: a system of 8 constraints over 12 variables; one row longer than short_max (cut into chunks)
long_row = lsa.fr_sparse_params()["short_max"] + 8
def csr():
    rows = [[(rng.randrange(12), rng.randrange(R)) for _ in range(long_row if i == 3 else rng.randrange(4))] for i in range(8)]
    return sp.Csr(rows, 12)
mats = [csr() for _ in range(3)]
X0, X1 = fr_raw(rng, 8), fr_raw(rng, 12)
handles = []
def sparse_create():
    handles[:] = [m.handle(lsa, keep_transpose=(i == 0)) for i, m in enumerate(mats)]
    return np.array([handles[0].rows, handles[0].cols, handles[0].nnz], dtype=np.uint64)
add("sparse_create", sparse_create, np.array([8, 12, len(mats[0].cols)], dtype=np.uint64))
add("sparse_matvec_1", lambda: handles[0].matvec(words(X1), 1), mats[0].times(X1, 1))
add("sparse_matvec_0", lambda: handles[0].matvec(words(X0), 0), mats[0].times(X0, 0))
Dq = lip.dom((4, None))
dq = [rng.randrange(R) for _ in range(3)]
add("qap_witness", lambda: lsa.fr_qap_witness(handles[0], handles[1], handles[2], words(X1), Dq.big_log, Dq.small_log, omega=Dq.w, coset=o.fr_mont(lip.G), d123=lip.enc(dq)),
    lip.expected_h(Dq, *(m.times(X1, 1) for m in mats), dq))
def sparse_close():
    lsa.synchronize()
    for hd in handles:
        hd.close()
    return np.zeros(1, dtype=np.uint64)
add("sparse_close", sparse_close, np.zeros(1, dtype=np.uint64))

# ---- key loading: 5 points a group
model = pl.Model()
for group in ("g1", "g2"):
    w = pl.width(group)
    es = pl.batch(pl.decompress_entries(group, model, True), 5, offset=len(pl.decompress_entries(group, model, True)) - 8)
    x = pl.words([v for e in es for v in e.x_raw]).reshape(5, 4 * w)
    flags = np.array([e.flag for e in es], dtype=np.uint8)
    want_st = np.array([e.status for e in es], dtype=np.uint8)
    want_pts = pl.words([v for e in es for v in e.out_words]).reshape(5, 12 * w)
    assert 0 < int((want_st >= pl.MALFORMED).sum()) < 5
    def decompress(group=group, x=x, flags=flags):
        pts, st, rejected = lsa.decompress(group, x, flags, check_subgroup=True, count_rejected=True)
        return np.concatenate([pts.reshape(-1), st.astype(np.uint64), np.array([rejected], dtype=np.uint64)])
    add("decompress_" + group, decompress, np.concatenate([want_pts.reshape(-1), want_st.astype(np.uint64), np.array([(want_st >= pl.MALFORMED).sum()], dtype=np.uint64)]))
    ventries = pl.validate_entries(group, model, True)
    vs = pl.batch(ventries, 5, offset=len(ventries) - 9)
    vpts = pl.words([v for e in vs for v in e.raw]).reshape(5, 12 * w)
    add("validate_" + group, lambda group=group, vpts=vpts: lsa.validate_points(group, vpts, check_subgroup=True), np.array([e.status for e in vs], dtype=np.uint8))
    centries = [e for e in pl.validate_entries(group, model, False) if e.affine is not None]
    cs = pl.batch(centries, 5, offset=len(centries) - 3)
    cpts = pl.words([v for e in cs for v in e.raw]).reshape(5, 12 * w)
    want_x = pl.words([v for e in cs for v in (pl.zero_of(group) if e.affine == "inf" else [pl.mont(c) for c in pl.coords(group, e.affine[0])])]).reshape(5, 4 * w)
    want_f = np.array([3 if e.affine == "inf" else pl.parity(group, e.affine[1]) for e in cs], dtype=np.uint8)
    def compress(group=group, cpts=cpts):
        cx, cf = lsa.compress(group, cpts)
        return np.concatenate([cx.reshape(-1), cf.astype(np.uint64)])
    add("compress_" + group, compress, np.concatenate([want_x.reshape(-1), want_f.astype(np.uint64)]))

# ---- group operations: results are compared as affine points
def points_eq(group):
    return lambda got, want: len(got) == len(want) and all(fz.canon(group, g) == fz.canon(group, x) for g, x in zip(got, want))
for group in ("g1", "g2"):
    pts, sc = fz.bases(rng, group, 3), fz.scalars(rng, 3)
    mul = o.g1_mul if group == "g1" else o.g2_mul
    add("scalar_mul_batch_" + group, lambda group=group, pts=pts, sc=sc: lsa.scalar_mul_batch(pts, sc, group=group).reshape(3, -1),
        [mul(pts[i], sc[i]) for i in range(3)], points_eq(group))
    vals, rows, col_ptr, exps = fz.bases(rng, group, 5), [0, 2, 1, 1, 3], [0, 2, 2, 5], fz.scalars(rng, 4)      # 3 columns, the second one empty
    add("sparse_matrix_msm_" + group, lambda group=group, vals=vals, exps=exps: lsa.sparse_matrix_msm(vals, rows, col_ptr, exps, group=group),
        fz.mtxmultiexp_by_columns(group, vals, rows, col_ptr, exps), points_eq(group))
p1, q1 = fz.bases(rng, "g1", 1), fz.bases(rng, "g2", 1)
add("pairing", lambda: lsa.pairing_product(p1, q1), o.pairing_product(p1, q1))
for group, n in (("g1", 2048), ("g2", 1024)):                    # (the CRS cache ignores vectors under 1024 points)
    bases, sc = o.arith_bases(group, rng.randrange(1, R), rng.randrange(R), n), o.random_scalars(n, seed=rng.randrange(1 << 30))[0]
    add("msm_" + group, lambda group=group, bases=bases, sc=sc: np.asarray(lsa.msm(group, bases, sc)).reshape(1, -1),
        np.asarray(o.multi_exp(group, bases, sc, mode="mixed")).reshape(1, -1), points_eq(group))

res = {}
first = {}
for cycle in (1, 2):
    lsa.init(0)
    for name, call, want, eq in calls:
        sys.stderr.write("CALL %%d %%s\n" %% (cycle, name))
        sys.stderr.flush()
        got = call()
        if cycle == 1:
            first[name] = got
            res["reference/" + name] = bool(eq(got, want))
        else:
            res["repeat/" + name] = bool(eq(got, first[name]))
    sys.stderr.write("CALL %%d shutdown\n" %% cycle)
    sys.stderr.flush()
    lsa.shutdown()
print("RESULT " + json.dumps(res))
"""

CALLS = ["fr_ntt", "fr_ntt_step", "cppoly_witness", "eval_mle", "eq_table", "fr_fold", "fr_scale_upper", "sumcheck_round",
         "matvec_sliced", "matvec_8x8_side0", "matvec_8x8_side1", "matmul", "quotient_basic", "lagrange_basic", "quotient_step", "lagrange_step",
         "sparse_create", "sparse_matvec_1", "sparse_matvec_0", "qap_witness", "sparse_close",
         "decompress_g1", "validate_g1", "compress_g1", "decompress_g2", "validate_g2", "compress_g2",
         "scalar_mul_batch_g1", "sparse_matrix_msm_g1", "scalar_mul_batch_g2", "sparse_matrix_msm_g2", "pairing", "msm_g1", "msm_g2"]

GROW = re.compile(r"stage_grow\s+(\d+) -> (\d+) bytes")
MARK = re.compile(r"^CALL (\d) (\S+)$")


def growth_by_call(stderr):
    """{cycle: {call: sorted [(from, to)] of the stage_grow lines between its marker and the next}}"""
    out, at = {1: {}, 2: {}}, None
    for line in stderr.splitlines():
        mk = MARK.match(line.strip())
        if mk:
            at = out[int(mk.group(1))].setdefault(mk.group(2), [])
            continue
        g = GROW.search(line)
        if g and at is not None:
            at.append((int(g.group(1)), int(g.group(2))))
    return {c: {k: sorted(v) for k, v in d.items()} for c, d in out.items()}


def test_two_init_shutdown_cycles_grow_and_free_the_same_staging():
    import legosnark_amd as lsa
    assert lsa.fr_matvec_slices(16, 512, 1) > 1                  # the shape meant to grow the partial-sum buffer takes the sliced path
    env = {k: v for k, v in os.environ.items() if k not in ("LSA_WARM_MB", "LSA_H2D", "LSA_CRS_CACHE")}
    env.update({"LSA_TRACE": "2", "LSA_WARM": "0"})
    # one child, one attempt: a child that fails or is killed is the finding
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    # 1. cycle 1 against the references, cycle 2 against cycle 1
    assert set(res) == {"%s/%s" % (k, c) for k in ("reference", "repeat") for c in CALLS}
    assert all(res.values()), sorted(k for k, v in res.items() if not v)
    # 2. the same growths, call by call (hence the same multiset per cycle); a first growth starts at 0 in both cycles
    grow = growth_by_call(r.stderr)
    assert set(grow[1]) == set(grow[2]) == set(CALLS) | {"shutdown"}
    assert grow[2] == grow[1], {c: (grow[1][c], grow[2][c]) for c in grow[1] if grow[1][c] != grow[2][c]}
    assert grow[1]["shutdown"] == []
    from_zero = {c: sum(1 for a, _ in v if a == 0) for c, v in grow[2].items()}
    for call, buffers in REACHED.items():
        assert from_zero[call] >= len(buffers), (call, buffers, grow[2][call])
    # 3. not vacuous: every buffer of the list above grew from nothing in each cycle
    for cycle in (1, 2):
        assert sum(1 for v in grow[cycle].values() for a, _ in v if a == 0) >= REACHED_BUFFERS, grow[cycle]
