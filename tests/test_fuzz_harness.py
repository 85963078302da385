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


PINV = pow(1 << 256, -1, o.P)
PT_OK, PT_INFINITY, PT_MALFORMED, PT_NOT_ON_CURVE, PT_NOT_IN_SUBGROUP = range(5)


def _np(x):
    """An operand as numpy: what a generator sends in device mode is a CPU tensor here."""
    if isinstance(x, np.ndarray):
        return x
    a = x.numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def _like(a, ref):
    """A result on the side its operand came from: numpy for numpy, a tensor for a tensor."""
    if isinstance(ref, np.ndarray):
        return a
    import torch
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a)


def _compiled():
    """The library itself, for its compiled shape alone (pure functions of the build: no device is touched)."""
    import os
    import legosnark_amd
    if not os.path.exists(legosnark_amd.LIB_PATH):
        legosnark_amd.build()
    return legosnark_amd


class StandInSparse:
    """An `FrSparse` handle that keeps the matrix as a Csr of Python integers."""

    def __init__(self, lib, vals, cols, row_ptr, ncols, keep_transpose=True):
        raw = fz.unwords(vals)
        ptr = [int(v) for v in row_ptr]
        self.lib, self.keep = lib, keep_transpose
        self.csr = fz.helpers().sp.Csr([[(int(cols[e]), raw[e]) for e in range(ptr[r], ptr[r + 1])] for r in range(len(ptr) - 1)], ncols)
        self.rows, self.cols, self.nnz = self.csr.nrows, ncols, len(raw)

    def matvec(self, x, side=1, out=None):
        if side == 0 and not self.keep:
            raise self.lib.LsaError("fr_sparse_matvec: side 0 needs keep_transpose")
        return _like(self.lib.out(self.csr.times(fz.unwords(_np(x)), side)), x)

    def close(self):
        self.csr = None


class StandIn:
    """The entry points the generators call, answered by the oracle; flip: bit 0 of the first word (or byte) of every
    returned array -- True: of all of them; a name: of the one returned array a call gives that name, alone."""
    FUZZ_DEVICE = "cpu"

    class LsaError(RuntimeError):
        pass

    def __init__(self, flip):
        self.flip = flip
        self.threshold = 0
        self.calls = set()
        self.members = {}

    def flips(self, name):
        return self.flip is True or (name is not None and self.flip == name)

    def out(self, a, name=None):
        a = np.array(a)
        if a.dtype != np.uint8:                                    # status and flag bytes stay bytes
            a = a.astype(np.uint64)
        if self.flips(name) and a.size:
            a.reshape(-1)[0] ^= a.dtype.type(1)
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

    def scalar_mul_batch(self, pts, scalars, out=None, group="g1"):
        if group == "g1":
            return self.out(o.g1_mul_batch(pts, scalars))
        p, s = _np(pts).reshape(-1, 24), _np(scalars).reshape(-1, 4)       # libff's scalar * point: the integer multiple on the whole twist
        return _like(self.out(np.array([o.g2_mul(p[i], s[i]) for i in range(len(p))], dtype=np.uint64).reshape(-1, 24)), pts)

    def sparse_matrix_msm(self, vals, rows, col_ptr, exps, group="g1"):
        if group == "g1":
            return self.out(o.mtxmultiexp(vals, rows, col_ptr, exps))
        return self.out(fz.mtxmultiexp_by_columns(group, vals, rows, col_ptr, exps))

    # ---- the Lipmaa prover, Fr matrices, the witness map
    def _domain(self, big_log, small_log, coset):
        lip = fz.helpers().lip
        D = lip.dom((big_log, small_log))
        g = lip.dec(np.asarray(coset).reshape(1, 4))[0]
        if pow(g, D.m if small_log is None else 2 * D.big, R) == 1:
            raise self.LsaError("fr_hadamard_quotient: coset_g: the vanishing polynomial may have a root on this coset")
        return D, g

    def fr_hadamard_quotient(self, a, b, c, d123, big_log, small_log=None, omega=None, coset=None, out=None):
        lip = fz.helpers().lip
        D, g = self._domain(big_log, small_log, coset)
        return _like(self.out(lip.expected_h(D, _np(a), _np(b), _np(c), lip.dec(d123), g=g)), a)

    def fr_lagrange(self, big_log, small_log, omega, t, out=None):
        lip = fz.helpers().lip
        row = self.out(lip.enc(lip.lagrange_closed(lip.dom((big_log, small_log)), lip.dec(np.asarray(t).reshape(1, 4))[0])))
        if out is None:
            return row
        out.copy_(_like(row, out))
        return out

    def fr_matrix_params(self):
        return _compiled().fr_matrix_params()

    def fr_matvec_slices(self, rows, cols, side=0):
        return _compiled().fr_matvec_slices(rows, cols, side)

    def fr_sparse_params(self):
        return _compiled().fr_sparse_params()

    def fr_matvec(self, m, w, rows, cols, side=0, out=None):
        return _like(self.out(fz.matvec_words(fz.unwords(_np(m)), fz.unwords(_np(w)), rows, cols, side)), m)

    def fr_matmul(self, a, b, rows_a, inner, cols_b, out=None):
        return _like(self.out(fz.matmul_words(fz.unwords(_np(a)), fz.unwords(_np(b)), rows_a, inner, cols_b)), a)

    def FrSparse(self, vals, cols, row_ptr, ncols, keep_transpose=True):
        return StandInSparse(self, vals, cols, row_ptr, ncols, keep_transpose)

    def fr_qap_witness(self, A, B, C, z, big_log, small_log=None, omega=None, coset=None, d123=None, out=None):
        lip = fz.helpers().lip
        D, g = self._domain(big_log, small_log, coset)
        Z = fz.unwords(_np(z))
        a, b, c = (M.csr.times(Z, 1) for M in (A, B, C))
        return _like(self.out(lip.expected_h(D, a, b, c, [0, 0, 0] if d123 is None else lip.dec(d123), g=g)), z)

    # ---- key loading, from the words themselves
    def _in_g2(self, q):
        """[r - 1] q == -q by libff's scalar * point (the oracle's), once per point."""
        if q not in self.members:
            m = fz.helpers().m
            self.members[q] = o.g2_canonical_affine(o.g2_mul(o.g2_from_affine(q), o.fr_mont(R - 1))) == m.g2_neg(q)
        return self.members[q]

    def decompress(self, group, x, flags, check_subgroup=True, out=None, count_rejected=False):
        pl = fz.helpers().pl
        w = pl.width(group)
        X, F = fz.unwords(_np(x)), _np(flags)
        one = 1 if group == "g1" else (1, 0)
        rows, status = [], []
        for i in range(len(F)):
            xw, f, st, q = X[w * i:w * i + w], int(F[i]), PT_OK, None
            if f & ~3:
                st = PT_MALFORMED
            elif f & 2:
                st = PT_INFINITY
            elif max(xw) >= o.P:
                st = PT_MALFORMED
            else:
                xv = [v * PINV % o.P for v in xw]
                xq = xv[0] if group == "g1" else tuple(xv)
                y = pl.fq_sqrt((xq ** 3 + 3) % o.P) if group == "g1" else pl.f2_sqrt(pl.g2_rhs(xq))
                if y is None:
                    st = PT_NOT_ON_CURVE
                else:
                    q = (xq, y if pl.parity(group, y) == f & 1 else pl.neg(group, y))
                    if group == "g2" and check_subgroup and not self._in_g2(q):
                        st, q = PT_NOT_IN_SUBGROUP, None
            rows.append(pl.inf_words(group) if q is None else pl.point_words(group, q[0], q[1], one))
            status.append(st)
        pts = _like(self.out(fz.point_array(group, rows), "points"), x)
        st = _like(self.out(np.array(status, dtype=np.uint8), "status"), x)
        if not count_rejected:
            return pts, st
        return pts, st, sum(1 for s in status if s >= PT_MALFORMED) ^ (1 if self.flips("n_rejected") else 0)

    def _jacobian(self, group, pts):
        """Every point as (raw words, coordinates as values or None when a word is >= p)."""
        pl = fz.helpers().pl
        w = pl.width(group)
        raw = fz.unwords(_np(pts))
        for i in range(len(raw) // (3 * w)):
            words = raw[3 * w * i:3 * w * (i + 1)]
            vals = None
            if max(words) < o.P:
                v = [x * PINV % o.P for x in words]
                vals = v if group == "g1" else [tuple(v[0:2]), tuple(v[2:4]), tuple(v[4:6])]
            yield words, vals

    @staticmethod
    def _affine(group, vals):
        m = fz.helpers().m
        X, Y, Z = vals
        if group == "g1":
            zi = m.inv(Z)
            return X * zi * zi % o.P, Y * zi * zi * zi % o.P
        zi = m.f2_inv(Z)
        z2 = m.f2_sqr(zi)
        return m.f2_mul(X, z2), m.f2_mul(Y, m.f2_mul(z2, zi))

    def validate_points(self, group, pts, check_subgroup=True):
        m = fz.helpers().m
        status = []
        for _, vals in self._jacobian(group, pts):
            if vals is None:
                status.append(PT_MALFORMED)
            elif vals[2] in (0, (0, 0)):
                status.append(PT_INFINITY)
            else:
                q = self._affine(group, vals)
                on = m.g1_is_on_curve(q) if group == "g1" else m.g2_is_on_curve(q)
                status.append(PT_NOT_ON_CURVE if not on else PT_NOT_IN_SUBGROUP if group == "g2" and check_subgroup and not self._in_g2(q) else PT_OK)
        return _like(self.out(np.array(status, dtype=np.uint8)), pts)

    def compress(self, group, pts):
        pl = fz.helpers().pl
        xs, flags = [], []
        for _, vals in self._jacobian(group, pts):
            if vals[2] in (0, (0, 0)):
                xs.append(pl.zero_of(group))
                flags.append(3)
            else:
                q = self._affine(group, vals)
                xs.append([pl.mont(v) for v in pl.coords(group, q[0])])
                flags.append(pl.parity(group, q[1]))
        return _like(self.out(fz.point_array(group, xs), "x"), pts), _like(self.out(np.array(flags, dtype=np.uint8), "flags"), pts)

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
    want |= set(NEW_KINDS)
    assert set(KIND_NAMES) == want and len(KIND_NAMES) == len(want) == 30


NEW_KINDS = ["hadamard_quotient", "lagrange", "fr_matvec", "fr_matmul", "fr_sparse_matvec", "qap_witness", "decompress", "validate_points", "compress",
             "scalar_mul_batch_g2", "sparse_matrix_msm_g2"]


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


@pytest.mark.parametrize("kind,which", [("decompress", "points"), ("decompress", "status"), ("decompress", "n_rejected"), ("compress", "x"), ("compress", "flags")])
def test_a_flip_in_one_returned_array_alone_fails(kind, which):
    """The calls that return several arrays: every one of them is looked at."""
    lib = StandIn(flip=which)
    executed, failed = fz.run_kind(lib, kind, SEED, CASES_PER_KIND)
    assert executed == CASES_PER_KIND
    assert failed, "%s: a library whose %s alone is one bit off passed all %d cases" % (kind, which, executed)
    assert not any(what.startswith("raised") for _, what in failed), failed


# What the 50 cases per seed of tests/test_fuzz_gpu.py must contain, per kind, as patterns over the `what` strings of its
# first seed: a condition on the generators' draw weights, met by the reference alone.
_BOTH_MODES = [r"mode=host\b", r"mode=device\b"]
_DOMAINS = [r"^basic 2\^([1-9]|10) ", r"^basic 2\^1[1-9] ", r"^step 2\^([1-9]|10)\+", r"^step 2\^1[1-9]\+", r"^step 2\^\d+\+2\^0 "]
_STATUSES = [r"^g1 ", r"^g2 "] + [r"check=%d .*statuses=\[[^\]]*\b%d\b" % (check, st) for check in (0, 1) for st in range(4 + check)]
COVERAGE = {
    "hadamard_quotient": _BOTH_MODES + _DOMAINS + [r"coset=refused\b", r"coset=generator\b", r"coset=random\b", r" n=0 ", r"b_is_a=1", r"d=zeros\b", r"d=planted\b"],
    "lagrange": _BOTH_MODES + _DOMAINS + [r"t=random\b", r"t=0\b", r"t=1\b", r"t=point\b", r"t=omega_point\b", r"products=1"],
    "fr_matvec": _BOTH_MODES + [r"side=0\b", r"side=1\b", r"side=0 slices=1\b", r"side=1 slices=1\b", r"side=0 slices=([2-9]|\d\d)", r"side=1 slices=([2-9]|\d\d)",
                                r"small=1\b", r"small=0\b", r"w=eq_table", r"rows=0 |cols=0 ", r"rows=1 |cols=1 "],
    "fr_matmul": _BOTH_MODES + [r"rows=0 |cols=0 ", r"inner=0 ", r"past_partials=1"],         # (and the tile's edges: added from the compiled shape)
    "fr_sparse_matvec": _BOTH_MODES + [r"sides=\[[^\]]*0", r"sides=\[[^\]]*1", r"\bunit\b", r"\bgeneral\b", r"\bpattern\b", r"nnz=0 ", r"rows=1 ", r"cols=1 ",
                                       r"transpose=0 .*refusals=[1-9]", r"transpose=1"],
    "qap_witness": _BOTH_MODES + _DOMAINS[:4] + [r"d=none\b", r"d=zeros\b", r"d=random\b"],
    "decompress": _BOTH_MODES + _STATUSES + [r"ladders=[1-9]"],
    "validate_points": _BOTH_MODES + _STATUSES,
    "compress": _BOTH_MODES + [r"^g1 ", r"^g2 ", r"infinities=[1-9]"],
    "scalar_mul_batch_g2": _BOTH_MODES + [r"^n=1 ", r"^n=\d{4} ", r"outside=[1-9]"],
    "sparse_matrix_msm_g2": [r"cols=0 ", r"cols=[1-9]"],
}


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_the_drawn_cases_cover_what_they_are_meant_to(kind):
    """Over the 50 case seeds of the GPU test's first seed: both domain families on both sides of 2^10, host and device mode,
    both sides, sliced and unsliced sums, unit / general / non-canonical coefficients, every status with and without the
    subgroup check, a refused coset, an empty matrix, a point outside the subgroup -- each at least once."""
    import re
    import test_fuzz_gpu
    lib = StandIn(flip=False)
    whats = []
    for s in fz.case_seeds(kind, test_fuzz_gpu.SEEDS[0], test_fuzz_gpu.CASES):
        ok, what = fz.run_case(lib, fz.KINDS[kind], s)
        assert ok, (s, what)
        whats.append(what)
    want = list(COVERAGE[kind])
    if kind == "fr_matmul":
        p = lib.fr_matrix_params()
        T, K = p["matmul_tile"], p["matmul_kstep"]
        want += [r"rows=(%d|%d|%d) " % (T - 1, T, T + 1), r"cols=(%d|%d|%d) " % (T - 1, T, T + 1), r"inner=(%d|%d|%d) " % (K - 1, K, K + 1)]
    missing = [pat for pat in want if not any(re.search(pat, w) for w in whats)]
    assert not missing, "%s: no case of the 50 matches %s" % (kind, missing)


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
