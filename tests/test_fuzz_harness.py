"""CPU suite: the randomised parity harness (tests/fuzz_parity.py, run on the GPU by tests/test_fuzz_gpu.py) is not vacuous.

A stand-in for the library answers every call with the oracle's own result: every kind must pass.  The same stand-in
with ONE bit flipped in every array it returns must fail every kind -- which a comparison of None with None, a loop over
nothing or a result nobody looks at would not.  That is the evidence that a subtly wrong kernel turns the GPU test red.
Few cases per kind: the oracle runs twice for each."""
import numpy as np
import pytest

import fuzz_parity as fz
import oracle_lib as o

R = o.R
SEED = 20261016
CASES_PER_KIND = 10


def _canon_to_jacobian(group, c):
    return (o.g1_from_affine if group == "g1" else o.g2_from_affine)(c)


class StandInBases:
    """A `Bases` handle that keeps the host array and slices it."""

    def __init__(self, lib, group, pts):
        self.lib, self.group, self.w = lib, group, fz.width(group)
        self.pts = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, self.w).copy()
        self.n = len(self.pts)
        self.table = self.n >= (lib.threshold or 1 << 19)          # lsa_msm_set_table_threshold: 0 = the default

    def _msm(self, sc, first, n):
        return self.lib.out(o.multi_exp(self.group, self.pts[first:first + n], sc[:n], mode="mixed") if n else np.zeros(self.w, dtype=np.uint64))

    def msm(self, d_scalars, n=None, first=0):
        n = self.n - first if n is None else n
        assert 0 <= first and first + n <= self.n
        return self._msm(fz.to_host(d_scalars).reshape(-1, 4), first, n)

    def msm_segments_async(self, d_scalars, offsets, d_outs, first=0):
        import torch
        assert self.table
        sc = fz.to_host(d_scalars).reshape(-1, 4)
        for j in range(len(offsets) - 1):
            lo, hi = int(offsets[j]), int(offsets[j + 1])
            assert first + hi - lo <= self.n
            d_outs[j].copy_(torch.from_numpy(self._msm(sc[lo:hi], first, hi - lo).view(np.int64)))

    def has_table(self):
        return self.table

    def close(self):
        self.pts = None


class StandIn:
    """The entry points the generators call, answered by the oracle; flip: bit 0 of the first word of every returned array."""
    FUZZ_DEVICE = "cpu"

    def __init__(self, flip):
        self.flip = flip
        self.threshold = 0
        self.calls = set()

    def out(self, a):
        a = np.array(a, dtype=np.uint64)
        if self.flip and a.size:
            a.reshape(-1)[0] ^= np.uint64(1)
        return a

    def set_table_threshold(self, n):
        self.threshold = n

    def synchronize(self):
        pass

    def Bases(self, group, pts):
        self.calls.add("Bases")
        return StandInBases(self, group, pts)

    def msm(self, group, bases, scalars):
        n = min(len(bases), len(scalars))
        return self.out(o.multi_exp(group, bases, scalars, mode="mixed") if n else np.zeros(fz.width(group), dtype=np.uint64))

    def commit_async(self, B1, B2, d_scalars, o1, o2, n=None):
        import torch
        o1.copy_(torch.from_numpy(B1.msm(d_scalars, n=n).view(np.int64)))
        o2.copy_(torch.from_numpy(B2.msm(d_scalars, n=n).view(np.int64)))

    def batch_exp(self, group, base, scalars):
        return self.out(o.batch_exp(group, base, scalars))

    def scalar_mul_batch(self, pts, scalars):
        return self.out(o.g1_mul_batch(pts, scalars))

    def sparse_matrix_msm(self, vals, rows, col_ptr, exps):
        return self.out(o.mtxmultiexp(vals, rows, col_ptr, exps))

    def normalize(self, group, pts):
        return self.out(np.array([_canon_to_jacobian(group, fz.canon(group, p)) for p in pts], dtype=np.uint64))

    def sum_async(self, group, d_pts, n, d_out):
        import torch
        pts = fz.to_host(d_pts).reshape(-1, fz.width(group))
        add = o.g1_add if group == "g1" else o.g2_add
        acc = pts[0]
        for i in range(1, n):
            acc = add(acc, pts[i])
        d_out.copy_(torch.from_numpy(self.out(acc).view(np.int64)))

    def _terms(self, fs, off, flags, final_exp):
        return self.out(np.array(fz._oracle_terms(fs, off, flags, final_exp), dtype=np.uint64).reshape(-1, 48))

    def pairing_terms(self, g1, offsets, g2=None, tables=None, index=None, flags=None, final_exp=True):
        if tables is None:
            fs = o.miller_loop_batch(g1, g2)
        else:
            fs = np.array([o.miller_loop_batch(g1[i:i + 1], g2[i:i + 1])[0] if index[i] < 0 else o.miller_loop_precomp(g1[i], tables[index[i]])
                           for i in range(len(g1))], dtype=np.uint64)
        return self._terms(fs, offsets, flags, final_exp)

    def g2_precompute(self, qs):
        return self.out(np.array([o.precompute_g2(q) for q in qs], dtype=np.uint64))

    def miller_loop_precomp(self, g1, tables, index=None):
        idx = range(len(g1)) if index is None else index
        return self.out(np.array([o.miller_loop_precomp(g1[i], tables[j]) for i, j in zip(range(len(g1)), idx)], dtype=np.uint64))

    def fq12_product(self, fs):
        return self.out(o.fq12_product(fs))

    def final_exponentiation(self, fs):
        return self.out(np.array([o.final_exponentiation(f) for f in fs], dtype=np.uint64))

    def fr_ntt(self, a, omega, inverse=False, coset=None):
        return self.out(o.fr_domain_transform(a, omega, inverse=inverse, coset=coset) if len(a) > 1 else a)

    def fr_ntt_step(self, a, big_log, small_log, omega, inverse=False, coset=None):
        return self.out(o.fr_step_domain_transform(a, big_log, small_log, omega, inverse=inverse, coset=coset))

    def cppoly_witness(self, v, r):
        return self.out(o.fr_cppoly_witness(v, r))

    def eval_mle(self, v, r):
        return self.out(o.fr_eval_mle(v, r))

    def fr_fold(self, old, r):
        return self.out(o.fr_push_randomness(old, r))

    def fr_scale_upper(self, old, k):
        return self.out(o.fr_scale_upper(old, k))

    def sumcheck_round(self, tables, suff=None, pre=None, rho_j=None):
        return self.out(o.fr_sumcheck_round(tables, suff=suff, pre=pre, rho_j=rho_j))

    def fr_eq_table(self, r, variant=0):
        if variant == 0:
            return self.out(o.fr_eq_table(r))
        rinv = pow(o.MONT, -1, R)
        t = [1]
        for x in r:                                          # the eq monomials: bit j of the index selects r[j] or 1 - r[j]
            x = o.limbs_to_int(x) * rinv % R
            t = [v * (1 - x) % R for v in t] + [v * x % R for v in t]
        return self.out(fz.mont_array(t))


KIND_NAMES = [name for name, _, _ in fz.CASES]


def test_every_kind_the_issue_names_is_there():
    want = {"final_exp", "eq_table", "msm", "batch_exp", "scalar_mul_batch", "pairing_terms", "ntt", "ntt_step", "fr_fold", "sumcheck_round",
            "resident_msm", "segments", "commit", "sparse_matrix_msm", "normalize", "sum_async", "fq12_product", "pairing_precomp", "fr_scale_upper"}
    assert set(KIND_NAMES) == want and len(KIND_NAMES) == len(want)


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_the_oracle_as_the_library_passes(kind):
    lib = StandIn(flip=False)
    executed, failed = fz.run_kind(lib, kind, SEED, CASES_PER_KIND)
    assert executed == CASES_PER_KIND
    assert not failed, "%s: %s" % (kind, failed)
    assert lib.threshold == 0                                 # every generator restores the table threshold


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_one_bit_off_fails(kind):
    lib = StandIn(flip=True)
    executed, failed = fz.run_kind(lib, kind, SEED, CASES_PER_KIND)
    assert executed == CASES_PER_KIND
    assert failed, "%s: a library one bit off passed all %d cases" % (kind, executed)
    assert not any(what.startswith("raised") for _, what in failed), failed     # mismatches, not accidents of the stand-in
    assert lib.threshold == 0


def test_a_raising_case_is_a_failure_and_is_counted():
    class Broken(StandIn):
        def fq12_product(self, fs):
            raise RuntimeError("boom")
    executed, failed = fz.run_kind(Broken(flip=False), "fq12_product", SEED, 5)
    assert executed == 5 and len(failed) == 5 and all("boom" in what for _, what in failed)


def test_case_seeds_depend_on_kind_and_seed_only():
    a = fz.case_seeds("msm", 1, 50)
    assert a == fz.case_seeds("msm", 1, 50) and len(set(a)) == 50
    assert a != fz.case_seeds("msm", 2, 50) and a != fz.case_seeds("segments", 1, 50)


def test_interleaved_plan_holds_every_kind_and_depends_on_the_seed_only():
    plan = fz.interleaved_plan(7, 10)
    assert plan == fz.interleaved_plan(7, 10) and plan != fz.interleaved_plan(8, 10)
    assert sorted(k for k, _ in plan) == sorted(KIND_NAMES * 10) and [k for k, _ in plan] != sorted(k for k, _ in plan)
    lib = StandIn(flip=False)
    assert all(fz.run_case(lib, fz.KINDS[k], s)[0] for k, s in fz.interleaved_plan(7, 1))


def test_digit_plan_mirror_and_edge_scalars():
    """fuzz_parity's mirror of csrc/msm_plan.h agrees with the one beside the MSM tests, the windows tile the 255 bits,
    and the edge scalars recode as intended under wide_digits()'s rule (a model of it in integers)."""
    import random
    import test_msm_gpu
    for n_table in (1, 70000, 1 << 20, 6 << 20):
        assert fz.table_positions(n_table) == test_msm_gpu._table_positions(n_table)
        for big in (False, True):
            plan = fz.wide_plan(n_table, big)
            assert len(plan) == (13 if n_table < 6 << 20 else 12) * (1 if big else 2)
            assert plan[0][0] == 0 and all(plan[k][0] + plan[k][1] == plan[k + 1][0] for k in range(len(plan) - 1)) and sum(plan[-1]) == 255

    def digits(s, plan):
        s %= R
        if s > fz.HALF:
            s = R - s
        out, carry = [], 0
        for k, (start, w) in enumerate(plan):
            d = ((s >> start) & ((1 << w) - 1)) + carry
            if k + 1 < len(plan) and d >= 1 << (w - 1):
                d, carry = d - (1 << w), 1
            else:
                carry = 0
            out.append(d)
        assert sum(d << start for d, (start, _) in zip(out, plan)) == s
        return out

    for big in (False, True):
        plan = fz.wide_plan(70000, big)
        edges = fz.edge_scalars(random.Random(1), 70000)
        ds = [digits(v, plan) for v in edges]
        for k, (start, w) in enumerate(plan[:-1]):
            assert any(d[k] == -(1 << (w - 1)) for d in ds)          # the first value recoded to negative: bucket B
            assert any(d[k] == (1 << (w - 1)) - 1 for d in ds)       # the last one that is not
        assert any(all(x in (0, -1) for x in d[k:-1]) and d[-1] == 1 and d[k] == -1 for d in ds for k in range(len(plan) - 1))   # a carry into the top window
        assert all(abs(d[-1]) <= 1 << (plan[-1][1] - 1) for d in ds)
    assert fz.HALF in edges and fz.HALF + 1 in edges
