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
precomputed G2 tables, the suffix update of the sumcheck.

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
def bases(rng, group, n):
    a, b = rng.randrange(1, R), rng.randrange(R)
    pts = o.arith_bases(group, a, b, n)                     # un-normalised Jacobian
    w = pts.shape[1]
    for _ in range(min(n, rng.choice([0, 0, 1, 2, n // 4 + 1]))):
        i = rng.randrange(n)
        if rng.random() < 0.5:
            pts[i, 2 * w // 3:] = 0                         # Z = 0: the point at infinity
        else:
            pts[i] = pts[rng.randrange(n)]                  # a repeated base
    return pts


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


def case_sparse_matrix_msm(rng, lsa, big=False):
    """mtxmultiexp on a random CSC matrix of G1 elements: ragged columns (empty ones too), zero and generator entries,
    repeated rows, a column of P and -P under one exponent."""
    nrows = rng.randrange(1, 13)
    ncols = rng.choice([0, 1, rng.randrange(1, 30), rng.randrange(1, 30)])
    pool = bases(rng, "g1", 16)
    gen = o.generator("g1")
    vals, rows, col_ptr = [], [], [0]
    for j in range(ncols):
        shape = rng.randrange(8)
        if shape == 0:
            i, row = rng.randrange(16), rng.randrange(nrows)
            vals += [pool[i], _g1_negated(pool[i])]
            rows += [row, row]
        else:
            for _ in range(rng.choice([0, 1, 2, rng.randrange(0, 10)])):
                t = rng.randrange(10)
                vals.append(np.zeros(12, dtype=np.uint64) if t == 0 else gen if t == 1 else pool[rng.randrange(16)])
                rows.append(rng.randrange(nrows))
        col_ptr.append(len(vals))
    vals = np.array(vals, dtype=np.uint64).reshape(-1, 12)
    exps = scalars(rng, nrows)
    got = lsa.sparse_matrix_msm(vals, rows, col_ptr, exps)
    want = o.mtxmultiexp(vals, rows, col_ptr, exps)
    ok = len(got) == ncols and all(canon("g1", got[j]) == canon("g1", want[j]) for j in range(ncols))
    return ok, "rows=%d cols=%d entries=%d" % (nrows, ncols, len(vals))


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


# (name, generator, weight in the script's time-budget loop)
CASES = [("final_exp", case_final_exp, 1), ("eq_table", case_eq_table, 1), ("msm", case_msm, 5), ("batch_exp", case_batch_exp, 2), ("scalar_mul_batch", case_smul, 2), ("pairing_terms", case_pairing, 3),
         ("ntt", case_ntt, 2), ("ntt_step", case_ntt_step, 2), ("fr_fold", case_fold, 3), ("sumcheck_round", case_sumcheck, 2),
         ("resident_msm", case_resident_msm, 5), ("segments", case_segments, 3), ("commit", case_commit, 2), ("sparse_matrix_msm", case_sparse_matrix_msm, 1), ("normalize", case_normalize, 1),
         ("sum_async", case_sum, 1), ("fq12_product", case_fq12_product, 1), ("pairing_precomp", case_pairing_precomp, 2), ("fr_scale_upper", case_scale_upper, 1)]
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
