#!/usr/bin/env python3
"""tests/fuzz_parity.py [seconds] [seed] [--big] -- randomised differential run of the C-ABI against the oracle (GPU box).

The parametrised tests under tests/ pin chosen shapes; the case generators here draw shapes and contents at random and
compare every result with the oracle's restatement of the reference algorithm: MSMs (G1 / G2; bases with random Z,
points at infinity, repeated bases; scalars of 254 / 128 / 64 / 31 / 16 bits with 0, 1, r - 1 and the digit recoder's
edge values planted), batch_exp, batched scalar multiplication, pairing products with conjugated terms and several
segments, final exponentiations of arbitrary Fq12 elements, the radix-2 and the step NTT in all four modes, the witness
recursion, evalMLE, pushRandomness, the sumcheck round polynomial -- and the entry points a prover holds its CRS through:
resident `Bases` handles with and without pre-shifted copies (sub-ranges, segment lists, the commitment pair with its
shared sort), the sparse-matrix MSM, normalisation, point sums, Fq12 products, Miller loops and pairing terms over
precomputed G2 tables, the suffix update of the sumcheck; and the calls of the later provers and of key loading: the Lipmaa
quotient and Lagrange row over basic and step domains, dense and sparse Fr matrix products, the QAP witness map, batch
decompression / validation / compression of points, the G2 batch scalar multiplication and sparse-matrix MSM.  Fr operands
of these are uniform in [0, r) -- not masked below 2^252 -- with 0, 1, r - 1, r - 2, (r - 1) / 2 and 2^252 +- 1 planted, each
case runs in host or in device mode by its own draw, and inputs the header calls unmodified are compared after the call.

Every generator is `fn(rng, lsa, big=False) -> (ok, what)`: everything it draws comes from `rng` (a random.Random), so
`fn(random.Random(seed), lsa)` replays a case.  tests/test_fuzz_gpu.py runs a fixed number of cases per kind and seed
inside `pytest -m gpu`; tests/test_fuzz_harness.py runs the same generators on the CPU against a stand-in library that
answers with the oracle (and must pass) or with the oracle's answer one bit off (and must fail every kind).

As a script this stays a time-budget loop for exploration: one JSON line per operation kind at the end (cases,
failures, the seeds of failures); exit status 1 on any mismatch.  The oracle is the only checker."""
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import oracle_lib as o  # noqa: E402

R, P = o.R, o.P
HALF = (R - 1) // 2                  # the largest scalar the digit recoder does not replace by its negative


def canon(group, pt):
    return o.g1_canonical_affine(pt) if group == "g1" else o.g2_canonical_affine(pt)


def width(group):
    return 12 if group == "g1" else 24


# ------------------------------------------------------------ device buffers (the stand-in of the CPU harness says "cpu")
def _device(lsa):
    return getattr(lsa, "FUZZ_DEVICE", "cuda:0")


def to_dev(lsa, arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).to(_device(lsa))


def zeros_dev(lsa, shape):
    import torch
    return torch.zeros(shape, dtype=torch.int64, device=_device(lsa))


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------ the digit plan (mirror of csrc/msm_plan.h) and its edge scalars
def table_positions(n_table):
    """Bit positions of the pre-shifted copies, table_grid() of csrc/msm_plan.h (tests/test_msm_gpu.py:_table_positions)."""
    nbig = 12 if n_table >= 6 << 20 else 13
    base, rem = divmod(255, nbig)
    pos, bit = [], 0
    for k in range(nbig):
        w = base + (1 if k < rem else 0)
        pos += [bit, bit + (w + 1) // 2]
        bit += w
    return pos


def wide_plan(n_table, big):
    """(start, width) of every window: wide_plan_for() -- 13 (12) wide digits, or all 26 (24) positions as narrow ones."""
    pos = table_positions(n_table)[::2 if big else 1] + [255]
    return [(pos[k], pos[k + 1] - pos[k]) for k in range(len(pos) - 1)]


def edge_scalars(rng, n_table):
    """Scalars at the edges of wide_digits(): the balanced-representative boundary, and for every recoded window of both
    plans a digit of exactly 2^(width-1) (the first value recoded to a negative digit: bucket index B for the widest
    window), 2^(width-1) - 1, and an all-ones run from that window up to the un-recoded top one (a carry through every
    window on the way); every recoded window at 2^(width-1) at once."""
    k = rng.randrange(1, 253)
    vals = [HALF, HALF + 1, HALF - 1, HALF + 2, HALF - (1 << k), HALF + (1 << k), HALF + 1 - (1 << k), HALF + 1 + (1 << k), 1 << k, R - (1 << k)]
    for big in (False, True):
        plan = wide_plan(max(n_table, 1), big)
        top = plan[-1][0]
        for start, w in plan[:-1]:
            vals += [1 << (start + w - 1), ((1 << (w - 1)) - 1) << start, (1 << top) - (1 << start)]
        vals.append(sum(1 << (start + w - 1) for start, w in plan[:-1]))
        vals.append(sum(((1 << (w - 1)) - 1) << start for start, w in plan[:-1]))
    return [v % R for v in vals]


def mont_array(ints):
    """Python ints -> (n, 4) Montgomery limbs (oracle_lib.fr_mont_array without one numpy call per element)."""
    buf = b"".join((x % R * o.MONT % R).to_bytes(32, "little") for x in ints)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def scalar_ints(rng, n, n_table=None, first=0):
    """n scalars as Python ints and the name of the shape drawn: random of some bit length with 0 / 1 / 2 / r - 1 and edge
    values planted; the whole vector one edge value; or that value at even base positions and its negative at odd ones
    (with the bases repeated pairwise every bucket cancels to infinity: bases(pairs=True))."""
    if n == 0:
        return [], "random"
    edges = edge_scalars(rng, n_table if n_table else n)
    mode = rng.choice(["random"] * 5 + ["one_value", "cancel"])
    if mode == "one_value":
        v = rng.choice(edges)
        if rng.random() < 0.5:
            v = R - v
        return [v % R] * n, mode
    if mode == "cancel":
        v = rng.choice(edges)
        return [(v if (first + i) % 2 == 0 else R - v) % R for i in range(n)], mode
    bits = rng.choice([254, 254, 254, 128, 64, 31, 16])
    ints = [rng.getrandbits(bits) % R for _ in range(n)]
    for _ in range(min(n, rng.choice([0, 0, 1, 3, n // 3 + 1]))):
        ints[rng.randrange(n)] = rng.choice([0, 1, R - 1, 2] + edges)
    return ints, mode


def scalars(rng, n, n_table=None):
    return mont_array(scalar_ints(rng, n, n_table)[0])


# ------------------------------------------------------------ bases
def bases_with_logs(rng, group, n):
    """n points (a + i b) G with infinities and repeats planted, and the discrete logarithm of every one."""
    a, b = rng.randrange(1, R), rng.randrange(R)
    pts = o.arith_bases(group, a, b, n)                     # un-normalised Jacobian
    logs = [(a + i * b) % R for i in range(n)]
    w = pts.shape[1]
    for _ in range(min(n, rng.choice([0, 0, 1, 2, n // 4 + 1]))):
        i = rng.randrange(n)
        if rng.random() < 0.5:
            pts[i, 2 * w // 3:] = 0                         # Z = 0: the point at infinity
            logs[i] = 0
        else:
            j = rng.randrange(n)
            pts[i], logs[i] = pts[j], logs[j]               # a repeated base
    return pts, logs


def bases(rng, group, n):
    return bases_with_logs(rng, group, n)[0]


# Large resident vectors come from two fixed progressions (a + i b) G per group, computed once per process and sliced:
# the oracle needs ~2 us per point, a case must not pay that for 2^16 points each time.  A case still depends on its
# rng alone (which progression, how many points, what is planted).
_POOL_AB = [(0x1234567 << 100 | 5, 0x7654321 << 64 | 9), (0xA5A5A5A5A5A5A5A5A5A5 << 40 | 0x31, 0x1234567 << 20 | 0x5)]
_pool = {}


def pool_bases(rng, group, n, pairs=False):
    """n points (a + i b) G with some infinities and repeats planted, and the discrete logarithm of every one.
    pairs: base 2i + 1 = base 2i (for the cancelling scalar shape)."""
    which = rng.randrange(len(_POOL_AB))
    a, b = _POOL_AB[which]
    have = _pool.get((group, which))
    if have is None or len(have) < n:
        size = 1 << 12
        while size < n:
            size *= 2
        have = _pool[(group, which)] = o.arith_bases(group, a, b, size)
    pts = have[:n].copy()
    logs = [(a + i * b) % R for i in range(n)]
    w = pts.shape[1]
    if pairs:
        m = n // 2
        pts[1:2 * m:2] = pts[0:2 * m:2]
        logs[1:2 * m:2] = logs[0:2 * m:2]
    for _ in range(min(n, rng.choice([0, 0, 1, 2, 5]))):
        i = rng.randrange(n)
        if rng.random() < 0.5:
            if rng.random() < 0.5:
                pts[i] = 0                                  # all-zero words
            else:
                pts[i, 2 * w // 3:] = 0                     # Z = 0, X and Y left
            logs[i] = 0
        else:
            j = rng.randrange(n)
            pts[i], logs[i] = pts[j], logs[j]
    return pts, logs


def msm_matches(group, got, pts, logs, sc, ints):
    """got == sum ints[i] * pts[i]: by the known-discrete-log identity (one oracle scalar multiplication of the generator),
    and for short vectors by the oracle's multi-exponentiation over the points themselves as well."""
    n = len(ints)
    k = sum(s * l for s, l in zip(ints, logs)) % R
    mul = o.g1_mul if group == "g1" else o.g2_mul
    ok = canon(group, got) == canon(group, mul(o.generator(group), o.fr_mont(k)))
    if 0 < n <= 300:
        ok = ok and canon(group, got) == canon(group, o.multi_exp(group, pts, sc, chunks=1, mode="mixed"))
    return ok


# ------------------------------------------------------------ the kinds of tests/fuzz_parity.py since round 5
def case_msm(rng, lsa, big=False):
    group = rng.choice(["g1", "g1", "g2"])
    top = (19 if group == "g1" else 16) if big else (16 if group == "g1" else 13)
    n = rng.choice([rng.randrange(0, 40), rng.randrange(40, 3000), 1 << rng.randrange(5, top), (1 << rng.randrange(5, top)) + rng.randrange(-3, 4)])
    n = max(n, 0)
    pts, sc = bases(rng, group, n) if n else np.zeros((0, 12 if group == "g1" else 24), dtype=np.uint64), scalars(rng, n) if n else np.zeros((0, 4), dtype=np.uint64)
    want = canon(group, o.multi_exp(group, pts, sc, chunks=1, mode="mixed")) if n else None
    got = canon(group, lsa.msm(group, pts, sc))
    return got == want, "%s n=%d" % (group, n)


def case_batch_exp(rng, lsa, big=False):
    group = rng.choice(["g1", "g2"])
    n = rng.choice([1, rng.randrange(1, 200), rng.randrange(200, 3000)])
    base = o.arith_bases(group, rng.randrange(1, R), 0, 1)[0]       # an un-normalised Jacobian point
    sc = scalars(rng, n)
    want = o.batch_exp(group, base, sc)
    got = lsa.batch_exp(group, base, sc)
    ok = len(got) == n and all(canon(group, got[i]) == canon(group, want[i]) for i in range(n))
    return ok, "%s n=%d" % (group, n)


def case_smul(rng, lsa, big=False):
    n = rng.choice([1, rng.randrange(1, 100), rng.randrange(100, 1500)])
    pts, sc = bases(rng, "g1", n), scalars(rng, n)
    want = o.g1_mul_batch(pts, sc)
    got = lsa.scalar_mul_batch(pts, sc)
    return len(got) == n and all(canon("g1", got[i]) == canon("g1", want[i]) for i in range(n)), "n=%d" % n


def _oracle_terms(fs, off, flags, final):
    want = []
    for j in range(len(off) - 1):
        acc = o.fq12_one()
        for i in range(int(off[j]), int(off[j + 1])):
            acc = o.fq12_mul(acc, o.fq12_unitary_inverse(fs[i]) if flags[i] else fs[i])
        want.append(o.final_exponentiation(acc) if final else acc)
    return want


def case_pairing(rng, lsa, big=False):
    nseg = rng.choice([1, 1, 2, 3])
    sizes = [rng.randrange(1, 6) for _ in range(nseg)]
    n = sum(sizes)
    g1, g2 = bases(rng, "g1", n), bases(rng, "g2", n)
    flags = np.array([rng.randrange(2) for _ in range(n)], dtype=np.uint8)
    final = rng.random() < 0.7
    off = np.cumsum([0] + sizes).astype(np.uint64)
    want = _oracle_terms(o.miller_loop_batch(g1, g2), off, flags, final)
    got = lsa.pairing_terms(g1, off, g2=g2, flags=flags, final_exp=final)
    return len(got) == nseg and all(np.array_equal(got[j], want[j]) for j in range(nseg)), "segments=%s final=%d" % (sizes, final)


def case_ntt(rng, lsa, big=False):
    log_n = rng.randrange(0, 15)
    a, _ = o.random_scalars(1 << log_n, seed=rng.randrange(1 << 30))
    w = o.fr_mont(o.fr_root_of_unity(log_n))
    inverse, coset = rng.random() < 0.5, (o.fr_mont(rng.randrange(2, R)) if rng.random() < 0.5 else None)
    got = lsa.fr_ntt(a, w, inverse=inverse, coset=coset)
    want = o.fr_domain_transform(a, w, inverse=inverse, coset=coset) if log_n else a
    return np.array_equal(got, want), "log_n=%d inverse=%d coset=%d" % (log_n, inverse, coset is not None)


def case_ntt_step(rng, lsa, big=False):
    big_log = rng.randrange(1, 14)
    small = rng.randrange(0, big_log)
    m = (1 << big_log) + (1 << small)
    a, _ = o.random_scalars(m, seed=rng.randrange(1 << 30))
    w = o.fr_mont(o.fr_root_of_unity(big_log + 1))
    inverse, coset = rng.random() < 0.5, (o.fr_mont(rng.randrange(2, R)) if rng.random() < 0.5 else None)
    got = lsa.fr_ntt_step(a, big_log, small, w, inverse=inverse, coset=coset)
    want = o.fr_step_domain_transform(a, big_log, small, w, inverse=inverse, coset=coset)
    return np.array_equal(got, want), "2^%d+2^%d inverse=%d coset=%d" % (big_log, small, inverse, coset is not None)


def case_fold(rng, lsa, big=False):
    kind = rng.choice(["witness", "eval_mle", "push"])
    lo = 1 if kind == "push" else 0                            # pushRandomness halves a vector: at least two values
    d = rng.choice([rng.randrange(lo, 15), rng.randrange(lo, 15), rng.randrange(15, 18)])      # (evalMLE takes another route from d = 16 on)
    v, _ = o.random_scalars(1 << d, seed=rng.randrange(1 << 30))
    r, _ = o.random_scalars(max(d, 1), seed=rng.randrange(1 << 30))
    r = r[:d]
    for i in range(d):
        if rng.random() < 0.1:
            r[i] = o.fr_mont(rng.choice([0, 1, R - 1]))
    if kind == "witness":
        return np.array_equal(lsa.cppoly_witness(v, r), o.fr_cppoly_witness(v, r)), "witness d=%d" % d
    if kind == "eval_mle":
        return np.array_equal(lsa.eval_mle(v, r), o.fr_eval_mle(v, r)), "eval_mle d=%d" % d
    return np.array_equal(lsa.fr_fold(v, r[0]), o.fr_push_randomness(v, r[0])), "push d=%d" % d


def case_sumcheck(rng, lsa, big=False):
    m = rng.randrange(1, 5)
    half = rng.choice([1, rng.randrange(1, 50), rng.randrange(50, 6000)])
    tabs = [o.random_scalars(2 * half, seed=rng.randrange(1 << 30))[0] for _ in range(m)]
    for t in tabs:                                             # the values at the edges of the kernels' lazy bounds
        for _ in range(rng.choice([0, 0, 2, half])):
            t[rng.randrange(2 * half)] = o.fr_mont(rng.choice([0, 1, R - 1, R - 2, (R - 1) // 2]))
    beta = rng.random() < 0.6
    suff = o.random_scalars(half, seed=rng.randrange(1 << 30))[0] if (beta and rng.random() < 0.8) else None
    pre = o.random_scalars(1, seed=rng.randrange(1 << 30))[0][0] if beta else None
    rho = o.random_scalars(1, seed=rng.randrange(1 << 30))[0][0] if beta else None
    got = lsa.sumcheck_round(tabs, suff=suff, pre=pre, rho_j=rho)
    want = o.fr_sumcheck_round(tabs, suff=suff, pre=pre, rho_j=rho)
    return np.array_equal(got, want), "m=%d half=%d beta=%d suff=%d" % (m, half, beta, suff is not None)


def case_eq_table(rng, lsa, big=False):
    d = rng.randrange(1, 15)
    r, _ = o.random_scalars(d, seed=rng.randrange(1 << 30))
    for i in range(d):
        if rng.random() < 0.15:
            r[i] = o.fr_mont(rng.choice([0, 1, R - 1]))
    ok = np.array_equal(lsa.fr_eq_table(r, 0), o.fr_eq_table(r))          # DPBeta::compute_eq_tbl as the reference's loop computes it
    v, _ = o.random_scalars(1 << d, seed=rng.randrange(1 << 30))
    rinv = pow(o.MONT, -1, R)
    ok = ok and o.fr_dot(v, lsa.fr_eq_table(r, 1)) == o.limbs_to_int(o.fr_eval_mle(v, r)) * rinv % R   # the eq monomials: <v, eq> = evalMLE(v, r)
    return ok, "eq_table d=%d" % d


def random_fq12(rng, n):
    """arbitrary Fq12 elements (not Miller values): random components, random subsets of them zero"""
    fs = np.zeros((n, 48), dtype=np.uint64)
    for i in range(n):
        mask = rng.choice([0xfff, 0xfff, 0xfff, rng.randrange(1, 0x1000)])
        for c in range(12):
            if (mask >> c) & 1:
                fs[i, 4 * c:4 * c + 4] = o.fq_mont(rng.randrange(P))
    return fs


def case_final_exp(rng, lsa, big=False):
    """lsa_final_exponentiation on arbitrary Fq12 elements"""
    n = rng.choice([1, 1, 2, 5, 17])
    fs = random_fq12(rng, n)
    got = lsa.final_exponentiation(fs)
    ok = len(got) == n and all(np.array_equal(got[i].reshape(-1), o.final_exponentiation(fs[i]).reshape(-1)) for i in range(n))
    return ok, "final_exp n=%d" % n


# ------------------------------------------------------------ resident handles and the other entry points a prover calls
def _table_size(rng, group, big):
    """Sizes of a resident vector on both sides of 2^16, where calls switch from narrow to wide digits (msm.hip:
    wide_big_min; the wide plan's 2^19 buckets take the partitioned sort); --big: up to 2^19 + and beyond."""
    if big:
        top = 1 << (19 if group == "g1" else 17)
        return rng.choice([rng.randrange(1, 3000), (1 << 16) + rng.randrange(-300, 300), top + rng.randrange(-3, 5000), rng.randrange(1 << 16, top + 5000)])
    if group == "g2":
        return rng.choice([rng.randrange(1, 40), rng.randrange(40, 1500), rng.randrange(40, 1500), rng.randrange(1500, 8000), (1 << 16) + rng.randrange(-200, 200)])
    return rng.choice([rng.randrange(1, 40), rng.randrange(40, 3000), rng.randrange(3000, 30000), (1 << 16) + rng.randrange(-300, 300), rng.randrange((1 << 16) + 1, 80000)])


def _sub_range(rng, n_table):
    """(first, n) of a call on a handle of n_table points: the whole vector, a prefix, or any sub-range (n >= 1)."""
    shape = rng.choice(["all", "prefix", "range", "range"])
    if shape == "all":
        return 0, n_table
    first = 0 if shape == "prefix" else rng.randrange(n_table)
    return first, rng.randrange(1, n_table - first + 1)


def case_resident_msm(rng, lsa, big=False):
    """lsa_msm_run on a `Bases` handle built with the pre-shifted copies (threshold 1) or without (1 << 30), a handle with
    copies also called on the plain path; random sub-ranges."""
    group = rng.choice(["g1", "g1", "g2"])
    n_table = _table_size(rng, group, big)
    build_thr = rng.choice([1, 1, 1 << 30])
    call_thr = 1 << 30 if (build_thr == 1 and rng.random() < 0.2) else build_thr
    calls = [_sub_range(rng, n_table) for _ in range(rng.choice([1, 2, 3]))]
    drawn = [scalar_ints(rng, n, n_table, first) for first, n in calls]
    pts, logs = pool_bases(rng, group, n_table, pairs=any(mode == "cancel" for _, mode in drawn))
    what = "%s table=%d build_thr=%d call_thr=%d calls=%s" % (group, n_table, build_thr, call_thr, [(f, n, m) for (f, n), (_, m) in zip(calls, drawn)])
    ok = True
    lsa.set_table_threshold(build_thr)
    try:
        B = lsa.Bases(group, pts)
        try:
            lsa.set_table_threshold(call_thr)
            for (first, n), (ints, _) in zip(calls, drawn):
                sc = mont_array(ints)
                got = B.msm(to_dev(lsa, sc), n=n, first=first)
                ok = msm_matches(group, got, pts[first:first + n], logs[first:first + n], sc, ints) and ok
        finally:
            B.close()
    finally:
        lsa.set_table_threshold(0)
    return ok, what


def case_segments(rng, lsa, big=False):
    """lsa_msm_run_segments_async: randomly cut offset lists (empty and one-element segments among them) over prefixes of
    bases[first:] of a table-carrying handle."""
    group = rng.choice(["g1", "g1", "g2"])
    n_table = _table_size(rng, group, big)
    first = rng.choice([0, 0, rng.randrange(n_table)])
    room = n_table - first
    nseg = rng.choice([1, 2, rng.randrange(3, 12), rng.randrange(12, 40)])
    lens = [min(room, rng.choice([0, 1, 2, 63, 64, 65, rng.randrange(1, 400), rng.randrange(1, 400), rng.randrange(1, 3000), room])) for _ in range(nseg)]
    if sum(lens) > 40000:                                      # a few whole-vector segments of a large handle are enough
        lens = [m if m < 3000 or j == 0 else rng.randrange(0, 3000) for j, m in enumerate(lens)]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ints, mode = scalar_ints(rng, int(offs[-1]), n_table, first)
    if mode == "cancel":                                       # the sign goes by the base's position, in every segment
        v = ints[0] if first % 2 == 0 else (R - ints[0]) % R
        ints = [(v if (first + i) % 2 == 0 else R - v) % R for m in lens for i in range(m)]
    pts, logs = pool_bases(rng, group, n_table, pairs=mode == "cancel")
    what = "%s table=%d first=%d lens=%s scalars=%s" % (group, n_table, first, lens, mode)
    sc = mont_array(ints) if ints else np.zeros((0, 4), dtype=np.uint64)
    ok = True
    lsa.set_table_threshold(1)
    try:
        B = lsa.Bases(group, pts)
        try:
            if not B.has_table():
                raise RuntimeError("segmented MSMs need the pre-shifted copies (LSA_PRECOMPUTE=0?)")
            outs = zeros_dev(lsa, (nseg, width(group)))
            B.msm_segments_async(to_dev(lsa, sc) if len(sc) else zeros_dev(lsa, (1, 4)), offs, outs, first=first)
            lsa.synchronize()
            got = to_host(outs)
            for j, m in enumerate(lens):
                lo = int(offs[j])
                ok = msm_matches(group, got[j], pts[first:first + m], logs[first:first + m], sc[lo:lo + m], ints[lo:lo + m]) and ok
        finally:
            B.close()
    finally:
        lsa.set_table_threshold(0)
    return ok, what


def case_commit(rng, lsa, big=False):
    """lsa_commit_run_async: the G1 and the G2 MSM of a commitment over one scalar vector (one shared sort when both handles
    carry copies), full length and a prefix."""
    n = _table_size(rng, "g2", big)
    thr = rng.choice([1, 1, 1 << 30])
    ints, mode = scalar_ints(rng, n, n, 0)
    p1, l1 = pool_bases(rng, "g1", n, pairs=mode == "cancel")
    p2, l2 = pool_bases(rng, "g2", n, pairs=mode == "cancel")
    sc = mont_array(ints)
    m = rng.randrange(1, n + 1)
    what = "n=%d prefix=%d thr=%d scalars=%s" % (n, m, thr, mode)
    ok = True
    lsa.set_table_threshold(thr)
    try:
        B1 = lsa.Bases("g1", p1)
        try:
            B2 = lsa.Bases("g2", p2)
            try:
                d_s = to_dev(lsa, sc)
                o1, o2 = zeros_dev(lsa, (12,)), zeros_dev(lsa, (24,))
                for k in (n, m):
                    lsa.commit_async(B1, B2, d_s, o1, o2, n=k)
                    lsa.synchronize()
                    ok = msm_matches("g1", to_host(o1), p1[:k], l1[:k], sc[:k], ints[:k]) and ok
                    ok = msm_matches("g2", to_host(o2), p2[:k], l2[:k], sc[:k], ints[:k]) and ok
            finally:
                B2.close()
        finally:
            B1.close()
    finally:
        lsa.set_table_threshold(0)
    return ok, what


def _g1_negated(pt):
    neg = pt.copy()
    neg[4:8] = o.int_to_limbs((P - o.limbs_to_int(pt[4:8])) % P)
    return neg


def _g2_negated(pt):
    neg = pt.copy()
    for k in (8, 12):
        neg[k:k + 4] = o.int_to_limbs((P - o.limbs_to_int(pt[k:k + 4])) % P)
    return neg


def _sparse_matrix_msm(rng, lsa, group):
    """mtxmultiexp on a random CSC matrix of group elements: ragged columns (empty ones too), zero and generator entries,
    repeated rows, a column of P and -P under one exponent.  G1 against the oracle's mtxmultiexp; G2, which the oracle has
    no such call for, against its multi-exponentiation of every column."""
    w = width(group)
    negated = _g1_negated if group == "g1" else _g2_negated
    nrows = rng.randrange(1, 13)
    ncols = rng.choice([0, 1, rng.randrange(1, 30), rng.randrange(1, 30)])
    pool = bases(rng, group, 16)
    gen = o.generator(group)
    vals, rows, col_ptr = [], [], [0]
    for j in range(ncols):
        shape = rng.randrange(8)
        if shape == 0:
            i, row = rng.randrange(16), rng.randrange(nrows)
            vals += [pool[i], negated(pool[i])]
            rows += [row, row]
        else:
            for _ in range(rng.choice([0, 1, 2, rng.randrange(0, 10)])):
                t = rng.randrange(10)
                vals.append(np.zeros(w, dtype=np.uint64) if t == 0 else gen if t == 1 else pool[rng.randrange(16)])
                rows.append(rng.randrange(nrows))
        col_ptr.append(len(vals))
    vals = np.array(vals, dtype=np.uint64).reshape(-1, w)
    exps = scalars(rng, nrows)
    if group == "g1":
        got = lsa.sparse_matrix_msm(vals, rows, col_ptr, exps)
        want = o.mtxmultiexp(vals, rows, col_ptr, exps)
    else:
        got = lsa.sparse_matrix_msm(vals, rows, col_ptr, exps, group="g2")
        want = mtxmultiexp_by_columns(group, vals, rows, col_ptr, exps)
    ok = len(got) == ncols and all(canon(group, got[j]) == canon(group, want[j]) for j in range(ncols))
    return ok, "rows=%d cols=%d entries=%d" % (nrows, ncols, len(vals))


def mtxmultiexp_by_columns(group, vals, rows, col_ptr, exps):
    """out[j] = sum_e exps[rows[e]] * vals[e] over column j: one oracle multi-exponentiation (its plain inner loop) a column."""
    w = width(group)
    vals = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, w)
    exps = np.ascontiguousarray(exps, dtype=np.uint64).reshape(-1, 4)
    rows = np.asarray(rows, dtype=np.int64)
    out = np.zeros((len(col_ptr) - 1, w), dtype=np.uint64)
    for j in range(len(col_ptr) - 1):
        lo, hi = int(col_ptr[j]), int(col_ptr[j + 1])
        out[j] = o.multi_exp(group, vals[lo:hi], exps[rows[lo:hi]], mode="inner") if hi > lo else o.g2_from_affine(None) if group == "g2" else o.g1_from_affine(None)
    return out


def case_sparse_matrix_msm(rng, lsa, big=False):
    return _sparse_matrix_msm(rng, lsa, "g1")


def case_sparse_matrix_msm_g2(rng, lsa, big=False):
    return _sparse_matrix_msm(rng, lsa, "g2")


def case_normalize(rng, lsa, big=False):
    """lsa_g{1,2}_normalize: the same point with Z = 1, every point of a batch (infinities and repeats among them)."""
    group = rng.choice(["g1", "g2"])
    n = rng.choice([1, 2, rng.randrange(1, 70), rng.randrange(70, 600 if group == "g1" else 300)])
    pts = bases(rng, group, n)
    got = lsa.normalize(group, pts)
    w = width(group)
    one = np.zeros(w // 3, dtype=np.uint64)
    one[:4] = o.fq_mont(1)
    ok = len(got) == n
    for i in range(n):
        c = canon(group, pts[i])
        ok = ok and canon(group, got[i]) == c and (c is None or np.array_equal(got[i, 2 * w // 3:], one))
    return ok, "%s n=%d" % (group, n)


def case_sum(rng, lsa, big=False):
    """lsa_g{1,2}_sum_async: the sum of n device-resident Jacobian points against the oracle's additions one by one."""
    group = rng.choice(["g1", "g2"])
    n = rng.choice([1, 2, rng.randrange(1, 70), rng.randrange(70, 300), rng.randrange(300, 1500 if group == "g1" else 600)])
    pts = bases(rng, group, n)
    d_out = zeros_dev(lsa, (width(group),))
    lsa.sum_async(group, to_dev(lsa, pts), n, d_out)
    lsa.synchronize()
    add = o.g1_add if group == "g1" else o.g2_add
    acc = pts[0]
    for i in range(1, n):
        acc = add(acc, pts[i])
    return canon(group, to_host(d_out)) == canon(group, acc), "%s n=%d" % (group, n)


def case_fq12_product(rng, lsa, big=False):
    """lsa_fq12_product over arbitrary Fq12 elements, ones and an empty batch among them."""
    n = rng.choice([0, 1, 2, rng.randrange(1, 40), rng.randrange(40, 200)])
    fs = random_fq12(rng, n)
    for _ in range(rng.choice([0, 0, 1, 3])):
        if n:
            fs[rng.randrange(n)] = o.fq12_one()
    got = lsa.fq12_product(fs)
    return np.array_equal(np.asarray(got).reshape(-1), o.fq12_product(fs).reshape(-1)), "fq12_product n=%d" % n


def case_pairing_precomp(rng, lsa, big=False):
    """lsa_g2_precompute tables (byte for byte libff's G2 precomputation), lsa_miller_loop_precomp and lsa_pairing_terms
    over them through an index with repeated Qs; some terms by point instead (index -1); empty segments."""
    nq = rng.randrange(1, 6)
    qs = bases(rng, "g2", nq)
    if rng.random() < 0.3:
        qs[rng.randrange(nq)] = o.generator("g2")             # Z = 1
    n = rng.randrange(1, 11)
    ps = bases(rng, "g1", n)
    idx = [rng.randrange(nq) for _ in range(n)]
    flags = np.array([rng.randrange(2) for _ in range(n)], dtype=np.uint8)
    cuts = sorted(rng.randrange(0, n + 1) for _ in range(rng.choice([0, 0, 1, 3])))
    off = np.array([0] + cuts + [n], dtype=np.uint64)
    final = rng.random() < 0.6
    mixed = rng.random() < 0.4
    what = "qs=%d terms=%d segments=%s final=%d mixed=%d" % (nq, n, [int(x) for x in off], final, mixed)
    tabs = lsa.g2_precompute(qs)
    ok = len(tabs) == nq and all(np.array_equal(np.asarray(tabs[i]).reshape(-1), o.precompute_g2(qs[i])) for i in range(nq))
    fs = o.miller_loop_batch(ps, qs[idx])
    ml = lsa.miller_loop_precomp(ps, tabs, idx)
    ok = ok and len(ml) == n and all(np.array_equal(ml[i], fs[i]) for i in range(n))
    want = _oracle_terms(fs, off, flags, final)
    if mixed:
        index = [i if rng.random() < 0.5 else -1 for i in idx]
        got = lsa.pairing_terms(ps, off, g2=qs[idx], tables=tabs, index=index, flags=flags, final_exp=final)
    else:
        got = lsa.pairing_terms(ps, off, tables=tabs, index=idx, flags=flags, final_exp=final)
    ok = ok and len(got) == len(off) - 1 and all(np.array_equal(got[j], want[j]) for j in range(len(off) - 1))
    return ok, what


def case_scale_upper(rng, lsa, big=False):
    """lsa_fr_scale_upper: cur[p] = old[half + p] * k (DPBeta's suffix update)."""
    half = rng.choice([1, rng.randrange(1, 50), rng.randrange(50, 6000), 1 << rng.randrange(0, 14)])
    old = mont_array([rng.getrandbits(254) % R for _ in range(2 * half)])
    for _ in range(rng.choice([0, 0, 2, half])):
        old[rng.randrange(2 * half)] = o.fr_mont(rng.choice([0, 1, R - 1, R - 2, HALF]))
    k = o.fr_mont(rng.choice([rng.randrange(R), rng.randrange(R), 0, 1, R - 1, HALF]))
    got = lsa.fr_scale_upper(old, k)
    return np.array_equal(got, o.fr_scale_upper(old, k)), "scale_upper half=%d" % half


# ------------------------------------------------------------ the Lipmaa, Fr-matrix, sparse, QAP, key-loading and G2 calls
# These entry points share state that no run of one of them alone moves: the quotient (and through it the witness map) runs
# seven transforms over ntt.hip's domain and coset table caches, which lsa_fr_ntt / lsa_fr_ntt_step fill and evict too; the
# step domain's table of 1 / Z is kept under one key; the staging of every one of these files grows and moves when a larger
# call arrives.  The interleaved plan of tests/test_fuzz_gpu.py puts them between each other and the older kinds.
#
# Their references are Python integers mod r / mod p, the oracle's transforms and group operations, and the big-integer
# model (oracle/pymodel/bn254_model.py) -- through the plain helpers that live beside the fixed-shape tests of each call.
_helpers = None


def helpers():
    """The test modules that own the reference helpers, imported on first use (at run time, after pytest has collected
    and rewritten them): lip.Dom / expected_h / lagrange_closed, sp.Csr, pl.f2_sqrt / g2_rhs / twist_ladder, g2.EDGE."""
    global _helpers
    if _helpers is None:
        import types
        import test_fr_sparse_gpu as sp
        import test_lipmaa_gpu as lip
        import test_point_load_gpu as pl
        import test_scalar_mul_g2_gpu as g2
        _helpers = types.SimpleNamespace(lip=lip, sp=sp, pl=pl, g2=g2, m=pl.m)
    return _helpers


RINV = pow(o.MONT, -1, R)
FR_EDGES = [0, 1, R - 1, R - 2, HALF, (1 << 252) - 1, (1 << 252) + 1]
ONES = (1 << 256) - 1


def words(xs):
    """256-bit integers -> (n, 4) uint64."""
    if not len(xs):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


def unwords(arr):
    b = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def fr_raw(rng, n, plant=True):
    """The words of n Fr values, as integers: uniform in [0, r) -- multiplication by 2^256 permutes the residues, so uniform
    words are uniform values -- with 0, 1, r - 1, r - 2, (r - 1) / 2 and 2^252 +- 1 planted (as values) at random places."""
    xs = [rng.randrange(R) for _ in range(n)]
    if plant and n:
        for _ in range(rng.choice([0, 0, 1, 3, n // 4 + 1])):
            xs[rng.randrange(n)] = rng.choice(FR_EDGES) * o.MONT % R
    return xs


def send(lsa, arr, device):
    """An operand in the case's mode: a private numpy copy, or a tensor on the library's device (an empty one has no
    address: the calls get a null pointer with an empty extent)."""
    arr = np.ascontiguousarray(arr)
    if not device:
        return arr.copy()
    if arr.dtype == np.uint8:
        import torch
        return torch.from_numpy(arr.copy()).to(_device(lsa))
    return to_dev(lsa, arr)


def fetch(lsa, t, device):
    """A result, or an operand after the call, as numpy (uint64 words or bytes)."""
    if not device:
        return np.asarray(t)
    lsa.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def same(got, want):
    """Exact bytes, shape and all (a result of another dtype or length is a mismatch, not an accident)."""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.size == want.size and np.array_equal(got.reshape(-1), want.reshape(-1))


def mode_name(device):
    return "device" if device else "host"


def draw_domain(rng, top=13):
    """(big_log, small_log): the basic radix-2 domain of 2^1 .. 2^top points (small_log None) or the step domain with
    small_log < big_log <= top - 1; both sides of the transforms' tile (2^10), small = 1 and small = big / 2."""
    basic = rng.random() < 0.5
    hi = top if basic else top - 1
    around = lambda: rng.randrange(9, min(11, hi) + 1)         # noqa: E731
    big_log = rng.choice([rng.randrange(1, 10), rng.randrange(1, 10), around(), around(), rng.randrange(min(11, hi), hi + 1)])
    return big_log, None if basic else rng.choice([0, big_log - 1, rng.randrange(big_log), rng.randrange(big_log)])


def domain_name(D):
    return "basic 2^%d" % D.big_log if D.small_log is None else "step 2^%d+2^%d" % (D.big_log, D.small_log)


def draw_coset(rng, D, refused=0.0):
    """(g, name): Fr's multiplicative generator, a random element the call accepts, or -- with probability `refused` -- one
    it must refuse: g^m = 1 on the basic domain, g^(2 * 2^big_log) = 1 on the step domain (a power of omega either way)."""
    order = D.m if D.small_log is None else 2 * D.big
    u = rng.random()
    if u < refused:
        return pow(D.w_int, rng.randrange(order), R), "refused"
    if u < 0.5 + refused / 2:
        return o.FR_GENERATOR, "generator"
    while True:
        g = rng.randrange(2, R)
        if pow(g, order, R) != 1:
            return g, "random"


def draw_d123(rng):
    shape = rng.choice(["random", "random", "zeros", "planted"])
    if shape == "random":
        return [rng.randrange(R) for _ in range(3)], shape
    if shape == "zeros":
        return [0, 0, 0], shape
    return [rng.choice([0, 0, 1, R - 1, rng.randrange(R)]) for _ in range(3)], shape


def case_hadamard_quotient(rng, lsa, big=False):
    """lsa_fr_hadamard_quotient against tests/test_lipmaa_gpu.py:expected_h (the oracle's seven transforms, integers between
    them): n = m, fewer, none; b the very buffer of a; refused cosets; inputs untouched."""
    lip = helpers().lip
    D = lip.dom(draw_domain(rng))
    n = rng.choice([D.m, D.m, rng.randrange(1, D.m + 1), rng.randrange(1, D.m + 1), 0])
    device = rng.random() < 0.5
    alias = rng.random() < 0.25
    a, c = words(fr_raw(rng, n)), words(fr_raw(rng, n))
    b = a if alias else words(fr_raw(rng, n))
    d, dname = draw_d123(rng)
    g, gname = draw_coset(rng, D, refused=0.12)
    what = "%s n=%d mode=%s coset=%s d=%s b_is_a=%d" % (domain_name(D), n, mode_name(device), gname, dname, alias)
    ta, tc = send(lsa, a, device), send(lsa, c, device)
    tb = ta if alias else send(lsa, b, device)
    call = lambda: lsa.fr_hadamard_quotient(ta, tb, tc, lip.enc(d), D.big_log, D.small_log, omega=D.w, coset=o.fr_mont(g))      # noqa: E731
    if gname == "refused":                                     # (any other refusal, and a refusal of any other case, raises out of here: a failure)
        try:
            call()
        except lsa.LsaError as e:
            lsa.synchronize()
            return "coset" in str(e), what
        return False, what
    got = fetch(lsa, call(), device)
    ok = same(got, lip.expected_h(D, a, b, c, d, g=g))
    ok = ok and same(fetch(lsa, ta, device), a) and same(fetch(lsa, tb, device), b) and same(fetch(lsa, tc, device), c)
    return ok, what


def case_lagrange(rng, lsa, big=False):
    """lsa_fr_lagrange against the closed formulae (tests/test_lipmaa_gpu.py:lagrange_closed), small domains against the
    product formula as well; t random, 0, 1, a point of the domain (the unit vector), omega times a point."""
    lip = helpers().lip
    D = lip.dom(draw_domain(rng))
    device = rng.random() < 0.5
    tname = rng.choice(["random", "random", "0", "1", "point", "point", "omega_point"])
    i = rng.randrange(D.m)
    t = {"random": rng.randrange(R), "0": 0, "1": 1, "point": D.point(i), "omega_point": D.w_int * D.point(i) % R}[tname]
    products = D.m <= 64 and rng.randrange(3) == 0
    what = "%s t=%s mode=%s products=%d" % (domain_name(D), tname, mode_name(device), products)
    out = zeros_dev(lsa, (D.m, 4)) if device else None
    got = fetch(lsa, lsa.fr_lagrange(D.big_log, D.small_log, D.w, o.fr_mont(t), out=out), device)
    want = lip.lagrange_closed(D, t)
    ok = same(got, lip.enc(want))
    if tname in ("1", "point"):
        ok = ok and want == [1 if x == t else 0 for x in D.points()]
    if products:
        ok = ok and want == lip.lagrange_products(D.points(), t)
    return ok, what


def matvec_words(M, W, rows, cols, side):
    """The words of the weighted sums of a row-major matrix: on words a product is X Y 2^-256, sums stay sums."""
    if side == 0:
        return words([sum(W[r] * M[r * cols + c] for r in range(rows)) * RINV % R for c in range(cols)])
    return words([sum(x * y for x, y in zip(M[r * cols:(r + 1) * cols], W)) * RINV % R for r in range(rows)])


def matmul_words(A, B, rows, inner, cols):
    Bt = [B[c::cols] for c in range(cols)]
    return words([sum(x * y for x, y in zip(A[r * inner:(r + 1) * inner], col)) * RINV % R for r in range(rows) for col in Bt])


def case_fr_matvec(rng, lsa, big=False):
    """lsa_fr_matvec, both sides, against Python integers: empty and one-element dimensions, the matmul tile's edge, the
    one-workgroup threshold from both sides, summed dimensions long enough to be cut into slices; side 0 also with the
    weights of DPMatrixMle (the oracle's eq table of a random rho)."""
    p = lsa.fr_matrix_params()
    T, small = p["matmul_tile"], p["matvec_small"]
    side = rng.randrange(2)
    shape = rng.choice(["edge", "edge", "threshold", "long_sum", "long_sum", "eq"] if side == 0 else ["edge", "edge", "threshold", "long_sum", "long_sum"])
    edge = lambda: rng.choice([0, 1, 1, rng.randrange(2, 9), T + rng.randrange(-1, 2), rng.randrange(2, 300)])     # noqa: E731
    if shape == "edge":
        rows, cols = edge(), edge()
    elif shape == "threshold":                                 # rows * cols just below, at and above the one-workgroup limit
        rows = rng.randrange(1, 200)
        cols = max(small // rows + rng.choice([-1, 0, 0, 1]), 1)
    elif shape == "long_sum":                                  # few outputs, a long summed dimension: the split-and-finish path
        nsum, nout = rng.randrange(200, 900), rng.randrange(1, 48)
        rows, cols = (nout, nsum) if side else (nsum, nout)
    else:
        rows, cols = 1 << rng.randrange(1, 10), rng.randrange(1, 100)
    while rows * cols > 1 << 16:
        rows, cols = (rows // 2, cols) if rows > cols else (rows, cols // 2)
    device = rng.random() < 0.5
    slices = lsa.fr_matvec_slices(rows, cols, side)
    what = "rows=%d cols=%d side=%d slices=%d small=%d mode=%s w=%s" % (rows, cols, side, slices, rows * cols <= small, mode_name(device), "eq_table" if shape == "eq" else "random")
    M = fr_raw(rng, rows * cols)
    if shape == "eq":
        W = unwords(o.fr_eq_table(words(fr_raw(rng, rows.bit_length() - 1))))
    else:
        W = fr_raw(rng, cols if side else rows)
    m, w = words(M), words(W)
    tm, tw = send(lsa, m, device), send(lsa, w, device)
    got = fetch(lsa, lsa.fr_matvec(tm, tw, rows, cols, side), device)
    ok = same(got, matvec_words(M, W, rows, cols, side))
    return ok and same(fetch(lsa, tm, device), m) and same(fetch(lsa, tw, device), w), what


def case_fr_matmul(rng, lsa, big=False):
    """lsa_fr_matmul against Python integers: every dimension at 0, 1 and the tile's edge, the summed one at 0 .. 5, the
    K-step's edge and one past the number of products csrc/fr_dot.h sums before it folds its running sum."""
    p = lsa.fr_matrix_params()
    T, K = p["matmul_tile"], p["matmul_kstep"]
    dim = lambda: rng.choice([0, 1, T - 1, T, T + 1, rng.randrange(2 * T + 4), rng.randrange(2 * T + 4)])      # noqa: E731
    rows, cols = dim(), dim()
    inner = rng.choice([rng.randrange(6), K - 1, K, K + 1, rng.randrange(2 * K + 4), rng.randrange(2 * K + 4), p["dot_max_partials"] * p["dot_group"] + 1])
    if inner > 2 * K + 3 and inner > 1 << 12:                  # one past the partial-sum count only while that is small
        inner = rng.randrange(2 * K + 4)
    while rows * inner * cols > 1 << 18:
        rows, cols = (rows // 2, cols) if rows > cols else (rows, cols // 2)
    device = rng.random() < 0.5
    what = "rows=%d inner=%d cols=%d past_partials=%d mode=%s" % (rows, inner, cols, inner > p["dot_max_partials"] * p["dot_group"], mode_name(device))
    A, B = fr_raw(rng, rows * inner), fr_raw(rng, inner * cols)
    a, b = words(A), words(B)
    ta, tb = send(lsa, a, device), send(lsa, b, device)
    got = fetch(lsa, lsa.fr_matmul(ta, tb, rows, inner, cols), device)
    ok = same(got, matmul_words(A, B, rows, inner, cols))
    return ok and same(fetch(lsa, ta, device), a) and same(fetch(lsa, tb, device), b), what


def draw_coefficient(rng, seen):
    """The raw words of a stored coefficient: the canonical words of +1 or -1 (the units the kernels add instead of
    multiplying), a general residue, or any 256-bit pattern (it counts mod r); `seen` collects the classes drawn."""
    k = rng.randrange(8)
    if k < 3:
        seen.add("unit")
        return o.MONT % R if k < 2 else R - o.MONT % R
    if k < 6:
        seen.add("general")
        return rng.randrange(R)
    seen.add("pattern")
    return rng.choice([rng.getrandbits(256) | 1 << 255, ONES, o.MONT % R + R, R, R + rng.randrange(R)])


def draw_csr(rng, sp, nrows, ncols, lengths, seen, budget):
    """A Csr of rows of the given lengths (cut when the entry budget runs out): random columns, some of them repeated
    inside the row."""
    rows = []
    for n in lengths:
        n = min(n, budget)
        budget -= n
        row = [(rng.randrange(ncols), draw_coefficient(rng, seen)) for _ in range(n)]
        for j in range(1, n):
            if rng.random() < 0.1:
                row[j] = (row[rng.randrange(j)][0], row[j][1])          # a duplicate column in the row
        rows.append(row)
    return sp.Csr(rows, ncols)


def case_fr_sparse_matvec(rng, lsa, big=False):
    """FrSparse.matvec against tests/test_fr_sparse_gpu.py:Csr.times: empty rows, duplicate columns, unit / general /
    non-canonical coefficients, row lengths around the kernels' thresholds, a matrix without entries, one row, one column;
    two or three products on one handle, side 0 refused when the transpose was not kept."""
    sp = helpers().sp
    p = lsa.fr_sparse_params()
    S, L, K = p["short_max"], p["lane_max"], p["chunk"]
    shape = rng.choice(["general", "general", "general", "general", "empty", "one_row", "one_col"])
    size = lambda: rng.choice([rng.randrange(1, 8), rng.randrange(1, 60), rng.randrange(1, 200)])          # noqa: E731
    nrows = 1 if shape == "one_row" else size()
    ncols = 1 if shape == "one_col" else size()
    length = lambda: rng.choice([0, 0, 1, 1, 2, 3, rng.randrange(6), rng.randrange(6), S + rng.randrange(-1, 2), L + rng.randrange(-1, 2),    # noqa: E731
                                 K + rng.randrange(-1, 2), 2 * K + 3, rng.randrange(2 * K)])
    seen = set()
    M = draw_csr(rng, sp, nrows, ncols, [0 if shape == "empty" else length() for _ in range(nrows)], seen, 6000)
    keep = rng.random() < 0.7
    device = rng.random() < 0.5
    sides = [rng.randrange(2) for _ in range(rng.choice([2, 3]))]
    what = "rows=%d cols=%d nnz=%d transpose=%d mode=%s sides=%s refusals=%d coefficients=%s" % (
        nrows, ncols, len(M.cols), keep, mode_name(device), sides, 0 if keep else sides.count(0), ",".join(sorted(seen)) or "none")
    ok = True
    handle = M.handle(lsa, keep_transpose=keep)
    try:
        ok = (handle.rows, handle.cols, handle.nnz) == (nrows, ncols, len(M.cols))
        for side in sides:
            X = fr_raw(rng, ncols if side else nrows)
            x = words(X)
            tx = send(lsa, x, device)
            if side == 0 and not keep:                                 # (a refusal of any other product raises out of here: a failure)
                try:
                    handle.matvec(tx, side)
                    ok = False
                except lsa.LsaError as e:
                    ok = ok and "keep_transpose" in str(e)
                continue
            got = fetch(lsa, handle.matvec(tx, side), device)
            ok = ok and same(got, M.times(X, side)) and same(fetch(lsa, tx, device), x)
    finally:
        lsa.synchronize()
        handle.close()
    return ok, what


def case_qap_witness(rng, lsa, big=False):
    """lsa_fr_qap_witness on three random CSR matrices of one shape (mostly units, empty rows, as libsnark's gadgets lay
    them out) at an assignment with z[0] = 1: the Csr.times products fed to expected_h."""
    h = helpers()
    lip, sp = h.lip, h.sp
    D = lip.dom(draw_domain(rng, top=12))
    nrows = rng.choice([D.m, rng.randrange(1, D.m + 1), rng.randrange(1, D.m + 1)])
    nvars = rng.choice([1, rng.randrange(1, 10), rng.randrange(1, 2 * nrows + 2)])
    length = lambda: rng.choice([0, 1, 1, 1, 2, 2, 3, rng.randrange(40)])              # noqa: E731
    unit = lambda: o.MONT % R if rng.random() < 0.7 else R - o.MONT % R                # noqa: E731
    mats = []
    for _ in range(3):
        rows = []
        for _ in range(nrows):
            rows.append([(rng.randrange(nvars), unit() if rng.random() < 0.85 else rng.randrange(R)) for _ in range(length())])
        mats.append(sp.Csr(rows, nvars))
    Z = fr_raw(rng, nvars)
    Z[0] = o.MONT % R
    d, dname = draw_d123(rng)
    if rng.random() < 0.3:
        d, dname = None, "none"
    g, gname = draw_coset(rng, D)
    device = rng.random() < 0.5
    what = "%s rows=%d vars=%d nnz=%s d=%s coset=%s mode=%s" % (domain_name(D), nrows, nvars, [len(m.cols) for m in mats], dname, gname, mode_name(device))
    z = words(Z)
    tz = send(lsa, z, device)
    hs = []
    try:
        for m in mats:
            hs.append(m.handle(lsa, keep_transpose=False))
        got = lsa.fr_qap_witness(hs[0], hs[1], hs[2], tz, D.big_log, D.small_log, omega=D.w, coset=o.fr_mont(g), d123=None if d is None else lip.enc(d))
        got = fetch(lsa, got, device)
    finally:
        lsa.synchronize()
        for hd in hs:
            hd.close()
    a, b, c = (m.times(Z, 1) for m in mats)
    ok = same(got, lip.expected_h(D, a, b, c, d or [0, 0, 0], g=g))
    return ok and same(fetch(lsa, tz, device), z), what


# ---- key loading: compressed points, validation, compression
_small_order = {}


def small_order_point():
    """A point T of order 10069 (a prime factor of the twist's cofactor 2p - r) on the twist: Q + k T, Q in G2 and 10069 not
    dividing k, lies outside G2 by construction.  Computed once per process; no case's draws depend on it."""
    if "T" not in _small_order:
        pl = helpers().pl
        order, i = R * (2 * P - R), 1
        assert order % 10069 == 0
        while "T" not in _small_order:
            y = pl.f2_sqrt(pl.g2_rhs((i, 1)))
            T = pl.twist_ladder(((i, 1), y), order // 10069) if y is not None else None
            if T is not None:
                assert pl.twist_ladder(T, 10069) is None
                _small_order["T"] = T
            i += 1
    return _small_order["T"]


def valid_affine(rng, group, k):
    """k multiples of the generator (in the subgroup) as affine Python integers."""
    pts = [canon(group, pt) for pt in o.arith_bases(group, rng.randrange(1, R), rng.randrange(R), k)]
    return [pt for pt in pts if pt is not None] or [canon(group, o.generator(group))]


def outside_affine(rng, q):
    """q + k T for the point T of order 10069: on the twist, outside G2 (sometimes k T itself, of small order)."""
    h = helpers()
    kt = h.pl.twist_ladder(small_order_point(), rng.randrange(1, 10069))
    return kt if rng.random() < 0.25 else h.m.g2_add(q, kt)


def random_z(rng, group):
    return rng.randrange(1, P) if group == "g1" else (rng.randrange(1, P), rng.randrange(P))


def point_array(group, rows):
    """Rows of 256-bit integers -> (n, words per row) uint64."""
    cols = len(rows[0]) if rows else 4
    return words([v for r in rows for v in r]).reshape(len(rows), 4 * cols)


PT_OK, PT_INFINITY, PT_MALFORMED, PT_NOT_ON_CURVE, PT_NOT_IN_SUBGROUP = range(5)


def case_decompress(rng, lsa, big=False):
    """lsa_g{1,2}_decompress on lanes mixed from: multiples of the generator, random abscissae (a residue or not by the
    reference's own root; G2: membership of at most 16 of them settled by the ladder over the whole twist), points outside
    G2 by construction, the is_zero flag over junk, words >= p, flag bytes with other bits set; both parities.  Exact
    points, status bytes and n_rejected; x and flags untouched."""
    h = helpers()
    pl = h.pl
    group = rng.choice(["g1", "g2"])
    w = pl.width(group)
    check = rng.random() < 0.5
    device = rng.random() < 0.5
    n = rng.choice([1, rng.randrange(1, 40), rng.randrange(1, 40), rng.randrange(40, 300), rng.randrange(300, 601)])
    inf = pl.inf_words(group)
    valid = valid_affine(rng, group, rng.randrange(1, 9))
    outside = [outside_affine(rng, rng.choice(valid)) for _ in range(rng.choice([0, 1, 3]))] if group == "g2" else []
    # random abscissae: (words of x, a root or None, its status)
    drawn, ladders = [], 0
    for _ in range(rng.choice([0, 2, 6, 16]) if group == "g2" else rng.choice([0, 4, 40])):
        if group == "g1":
            x = rng.randrange(P)
            y = pl.fq_sqrt((x * x * x + 3) % P)
            st = PT_OK                                            # the curve's order is r: a point of it is in G1
        else:
            x = (rng.randrange(P), rng.randrange(P))
            y = pl.f2_sqrt(pl.g2_rhs(x))
            st = PT_OK
            if y is not None and check:
                ladders += 1
                st = PT_NOT_IN_SUBGROUP if pl.twist_ladder((x, y), R) is not None else PT_OK
        drawn.append((x, y, st if y is not None else PT_NOT_ON_CURVE))
    lanes = []
    for _ in range(n):
        t = rng.choice(["valid", "valid", "valid", "abscissa", "abscissa", "outside", "zero", "range", "flag"])
        bit = rng.randrange(2)
        if t == "abscissa" and drawn:
            x, y, st = rng.choice(drawn)
            xw = [pl.mont(v) for v in pl.coords(group, x)]
            if st == PT_OK:
                want_y = y if pl.parity(group, y) == bit else pl.neg(group, y)     # (G2 roots with c0 == 0: (0, r2) for bit 0, its negative for bit 1)
                lanes.append(pl.Entry(xw, bit, st, pl.point_words(group, x, want_y, 1 if group == "g1" else (1, 0))))
            else:
                lanes.append(pl.Entry(xw, bit, st, inf))
        elif t == "outside" and outside:
            e = pl.accepted(group, rng.choice(outside), flip=bool(bit))
            if check:
                e.status, e.out_words = PT_NOT_IN_SUBGROUP, inf
            lanes.append(e)
        elif t == "zero":                                          # is_zero: X is ignored, whatever it spells
            lanes.append(pl.Entry([rng.choice([rng.getrandbits(256), ONES, 0, P]) for _ in range(w)], 2 | bit, PT_INFINITY, inf))
        elif t == "range":                                         # a word >= p in one component
            xw = [pl.mont(v) for v in pl.coords(group, rng.choice(valid)[0])]
            xw[rng.randrange(w)] = rng.choice([P, P + 1, ONES, rng.randrange(P, 1 << 256)])
            lanes.append(pl.Entry(xw, bit, PT_MALFORMED, inf))
        elif t == "flag":                                          # a bit other than 0 and 1, with and without is_zero
            xw = [pl.mont(v) for v in pl.coords(group, rng.choice(valid)[0])]
            lanes.append(pl.Entry(xw, rng.randrange(4, 256), PT_MALFORMED, inf))
        else:
            lanes.append(pl.accepted(group, rng.choice(valid), flip=bool(bit)))
    x = point_array(group, [e.x_raw for e in lanes])
    flags = np.array([e.flag for e in lanes], dtype=np.uint8)
    want_st = np.array([e.status for e in lanes], dtype=np.uint8)
    want = point_array(group, [e.out_words for e in lanes])
    what = "%s n=%d check=%d mode=%s statuses=%s ladders=%d" % (group, n, check, mode_name(device), sorted(set(int(s) for s in want_st)), ladders)
    tx, tf = send(lsa, x, device), send(lsa, flags, device)
    pts, st, rejected = lsa.decompress(group, tx, tf, check_subgroup=check, count_rejected=True)
    ok = same(fetch(lsa, st, device), want_st) and same(fetch(lsa, pts, device), want) and rejected == int((want_st >= PT_MALFORMED).sum())
    return ok and same(fetch(lsa, tx, device), x) and same(fetch(lsa, tf, device), flags), what


def perturbed(rng, raw, lo, hi):
    """One word of raw[lo:hi] with one bit flipped, still below p and not zero."""
    raw = list(raw)
    pos = rng.randrange(lo, hi)
    while True:
        v = raw[pos] ^ (1 << rng.randrange(254))
        if 0 < v < P:
            raw[pos] = v
            return raw


def jacobian_lanes(rng, group, n, check, rejected=True):
    """n Jacobian points as (raw words, status, affine point / "inf" / None): valid points under a random Z (and Z = one),
    G2 twist points outside the subgroup, Z = 0, and -- with `rejected` -- words >= p and one coordinate perturbed, in the
    combinations that show the precedence MALFORMED > INFINITY, NOT_ON_CURVE > NOT_IN_SUBGROUP."""
    pl = helpers().pl
    w = pl.width(group)
    valid = valid_affine(rng, group, rng.randrange(1, 9))
    outside = [outside_affine(rng, rng.choice(valid)) for _ in range(rng.choice([0, 1, 3]))] if group == "g2" else []
    one = 1 if group == "g1" else (1, 0)
    kinds = ["valid", "valid", "valid", "valid", "outside", "zero"] + (["range", "perturbed", "perturbed"] if rejected else [])
    lanes = []
    for _ in range(n):
        t = rng.choice(kinds)
        q, status = rng.choice(valid), PT_OK
        if t == "outside" and outside:
            q, status = rng.choice(outside), PT_NOT_IN_SUBGROUP if check else PT_OK
        raw = pl.point_words(group, *pl.rescaled(group, q, one if rng.random() < 0.15 else random_z(rng, group)))
        affine = q
        if t == "zero":
            raw = rng.choice([pl.inf_words(group), raw[:2 * w] + [0] * w, [rng.randrange(P) for _ in range(2 * w)] + [0] * w])
            status, affine = PT_INFINITY, "inf"
        elif t == "perturbed":                                     # off the curve, whatever the subgroup test would say
            raw, status, affine = perturbed(rng, raw, 0, 3 * w), PT_NOT_ON_CURVE, None
        elif t == "range":                                         # a word >= p: in a good point, with Z = 0, off the curve
            also = rng.randrange(3)
            if also == 1:
                raw = raw[:2 * w] + [0] * w
            elif also == 2:
                raw = perturbed(rng, raw, 0, 3 * w)
            raw[rng.randrange(3 * w)] = rng.choice([P, P + 1, ONES, rng.randrange(P, 1 << 256)])
            status, affine = PT_MALFORMED, None
        lanes.append((raw, status, affine))
    return lanes


def case_validate_points(rng, lsa, big=False):
    """lsa_g{1,2}_validate on Jacobian points with random Z: exact status bytes, the points untouched."""
    group = rng.choice(["g1", "g2"])
    check = rng.random() < 0.5
    device = rng.random() < 0.5
    n = rng.choice([1, rng.randrange(1, 40), rng.randrange(40, 300), rng.randrange(300, 601)])
    lanes = jacobian_lanes(rng, group, n, check)
    pts = point_array(group, [raw for raw, _, _ in lanes])
    want = np.array([st for _, st, _ in lanes], dtype=np.uint8)
    what = "%s n=%d check=%d mode=%s statuses=%s" % (group, n, check, mode_name(device), sorted(set(int(s) for s in want)))
    tp = send(lsa, pts, device)
    got = fetch(lsa, lsa.validate_points(group, tp, check_subgroup=check), device)
    return same(got, want) and same(fetch(lsa, tp, device), pts), what


def case_compress(rng, lsa, big=False):
    """lsa_g{1,2}_compress on valid points with random Z and infinities (G2: twist points outside G2 too, compression does
    not care): exact X words and flags, X = 0 and flags = 3 for infinity; then decompress(compress(P)) is P normalised."""
    pl = helpers().pl
    group = rng.choice(["g1", "g2"])
    device = rng.random() < 0.5
    n = rng.choice([1, rng.randrange(1, 40), rng.randrange(40, 300), rng.randrange(300, 601)])
    lanes = jacobian_lanes(rng, group, n, False, rejected=False)
    one = 1 if group == "g1" else (1, 0)
    pts = point_array(group, [raw for raw, _, _ in lanes])
    want_x = point_array(group, [pl.zero_of(group) if q == "inf" else [pl.mont(v) for v in pl.coords(group, q[0])] for _, _, q in lanes])
    want_f = np.array([3 if q == "inf" else pl.parity(group, q[1]) for _, _, q in lanes], dtype=np.uint8)
    want_back = point_array(group, [pl.inf_words(group) if q == "inf" else pl.point_words(group, q[0], q[1], one) for _, _, q in lanes])
    want_st = np.array([st for _, st, _ in lanes], dtype=np.uint8)
    what = "%s n=%d mode=%s infinities=%d" % (group, n, mode_name(device), int((want_st == PT_INFINITY).sum()))
    tp = send(lsa, pts, device)
    tx, tf = lsa.compress(group, tp)
    ok = same(fetch(lsa, tx, device), want_x) and same(fetch(lsa, tf, device), want_f) and same(fetch(lsa, tp, device), pts)
    back, st = lsa.decompress(group, tx, tf, check_subgroup=False)
    return ok and same(fetch(lsa, back, device), want_back) and same(fetch(lsa, st, device), want_st), what


def case_scalar_mul_batch_g2(rng, lsa, big=False):
    """lsa_g2_scalar_mul_batch: multiples of the generator (infinities and repeats among them) under the MSM's edge scalars
    and the edges of the ladder's signed 4-bit recoding, against the oracle -- its fixed-base multiples of the generator by
    the known discrete logarithms, and for short vectors its scalar * point on every item -- and up to four planted points
    outside G2 or of small order against the model's ladder over the whole twist."""
    h = helpers()
    n = rng.choice([1, rng.randrange(1, 101), rng.randrange(1, 1501)])
    pts, logs = bases_with_logs(rng, "g2", n)
    ints = scalar_ints(rng, n)[0]
    for _ in range(rng.choice([0, 1, 3, n // 3 + 1])):
        v = rng.choice(h.g2.EDGE)
        ints[rng.randrange(n)] = (R - v) % R if rng.random() < 0.3 else v
    planted = {}
    for _ in range(rng.choice([0, 0, 1, 2, 4])):
        i = rng.randrange(n)
        planted[i] = outside_affine(rng, canon("g2", o.generator("g2")))
        pts[i] = o.g2_from_affine(planted[i], random_z(rng, "g2") if rng.random() < 0.7 else (1, 0))
    device = rng.random() < 0.5
    what = "n=%d mode=%s outside=%d" % (n, mode_name(device), len(planted))
    sc = mont_array(ints)
    tp, ts = send(lsa, pts, device), send(lsa, sc, device)
    got = fetch(lsa, lsa.scalar_mul_batch(tp, ts, group="g2"), device).reshape(-1, 24)
    want = o.batch_exp("g2", o.generator("g2"), mont_array([s * l for s, l in zip(ints, logs)]))
    ok = len(got) == n
    for i in range(n if ok else 0):
        c = canon("g2", got[i])
        if i in planted:
            ok = ok and c == h.pl.twist_ladder(planted[i], ints[i])        # (the scalar is canonical: nothing is reduced)
        else:
            ok = ok and c == canon("g2", want[i]) and (n > 100 or c == canon("g2", o.g2_mul(pts[i], sc[i])))
    return ok and same(fetch(lsa, tp, device), pts) and same(fetch(lsa, ts, device), sc), what


# (name, generator, weight in the script's time-budget loop)
CASES = [("final_exp", case_final_exp, 1), ("eq_table", case_eq_table, 1), ("msm", case_msm, 5), ("batch_exp", case_batch_exp, 2), ("scalar_mul_batch", case_smul, 2), ("pairing_terms", case_pairing, 3),
         ("ntt", case_ntt, 2), ("ntt_step", case_ntt_step, 2), ("fr_fold", case_fold, 3), ("sumcheck_round", case_sumcheck, 2),
         ("resident_msm", case_resident_msm, 5), ("segments", case_segments, 3), ("commit", case_commit, 2), ("sparse_matrix_msm", case_sparse_matrix_msm, 1), ("normalize", case_normalize, 1),
         ("sum_async", case_sum, 1), ("fq12_product", case_fq12_product, 1), ("pairing_precomp", case_pairing_precomp, 2), ("fr_scale_upper", case_scale_upper, 1),
         ("hadamard_quotient", case_hadamard_quotient, 3), ("lagrange", case_lagrange, 2), ("fr_matvec", case_fr_matvec, 2), ("fr_matmul", case_fr_matmul, 2),
         ("fr_sparse_matvec", case_fr_sparse_matvec, 2), ("qap_witness", case_qap_witness, 3), ("decompress", case_decompress, 2), ("validate_points", case_validate_points, 1),
         ("compress", case_compress, 1), ("scalar_mul_batch_g2", case_scalar_mul_batch_g2, 2), ("sparse_matrix_msm_g2", case_sparse_matrix_msm_g2, 1)]
KINDS = {name: fn for name, fn, _ in CASES}


def case_seeds(kind, seed, count):
    """The case seeds of (kind, seed): a function of the two alone, the same on every machine and commit."""
    master = random.Random("%s/%d" % (kind, seed))
    return [master.randrange(1 << 40) for _ in range(count)]


def run_case(lsa, fn, seed, big=False):
    """One case from its seed; an exception is a failure too."""
    try:
        ok, what = fn(random.Random(seed), lsa, big)
    except Exception as e:
        ok, what = False, "raised %r" % (e,)
    return bool(ok), what


def run_kind(lsa, kind, seed, count, big=False):
    """`count` cases of one kind -> (cases executed, [(case seed, what) of every failure])."""
    executed, failed = 0, []
    for s in case_seeds(kind, seed, count):
        ok, what = run_case(lsa, KINDS[kind], s, big)
        executed += 1
        if not ok:
            failed.append((s, what))
    return executed, failed


def interleaved_plan(seed, per_kind):
    """per_kind cases of every kind in one shuffled order, a function of the seed alone: what the script's loop does, and
    what a run of one kind after the other cannot show -- state one entry point leaves behind for the next (staging
    buffers that grow and move, cached graphs and tables, the table threshold, the host heap)."""
    master = random.Random("interleaved/%d" % seed)
    plan = [(name, master.randrange(1 << 40)) for name, _, _ in CASES for _ in range(per_kind)]
    master.shuffle(plan)
    return plan


def main():
    import legosnark_amd as lsa
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    big = "--big" in sys.argv        # larger MSMs (the general pipeline beyond the compact one's range, the CRS cache's prefix tables, resident vectors of 2^19 + points)
    budget = float(args[0]) if len(args) > 0 else 300.0
    seed0 = int(args[1]) if len(args) > 1 else 20261003
    lsa.init(0)
    stats = {name: {"cases": 0, "failures": 0, "failed": []} for name, _, _ in CASES}
    pick = [c for c in CASES for _ in range(c[2])]
    master = random.Random(seed0)
    t0 = time.time()
    k = 0
    while time.time() - t0 < budget:
        name, fn, _ = master.choice(pick)
        seed = master.randrange(1 << 40)
        ok, what = run_case(lsa, fn, seed, big)
        st = stats[name]
        st["cases"] += 1
        if not ok:
            st["failures"] += 1
            st["failed"].append({"seed": seed, "what": what})
            print("MISMATCH", name, seed, what, flush=True)
        k += 1
    total_fail = sum(s["failures"] for s in stats.values())
    for name, st in stats.items():
        print(json.dumps({"op": name, **st}))
    print(json.dumps({"fuzz_parity": {"seconds": round(time.time() - t0, 1), "seed": seed0, "cases": k, "failures": total_fail}}))
    return 1 if total_fail else 0


if __name__ == "__main__":
    sys.exit(main())
