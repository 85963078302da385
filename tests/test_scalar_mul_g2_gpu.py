"""GPU parity tests for the G2 twins of the key-generation operators: variable-base batch scalar multiplication and
mtxmultiexp on a column-sparse G2 matrix (lsa_g2_scalar_mul_batch, lsa_g2_sparse_matrix_msm), through the C-ABI, against
the oracle and, where the points lie outside the order-r subgroup or have small order, against the big-integer model
(which has no endomorphism anywhere).  Group elements are compared after affine normalisation.

The shapes follow the kernel's own figures (lsa_smul_param): the window width drives the simulation of the ladder's
accumulator in test 3, the number of resident items the grid-stride test."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "pymodel"))
import bn254_model as m  # noqa: E402
import test_point_load_gpu as pl  # noqa: E402  (f2_sqrt, g2_rhs, twist_ladder: plain helpers)
import test_points_io_gpu as pio  # noqa: E402  (outside_point)

pytestmark = pytest.mark.gpu
R, P = o.R, o.P
SMALL = 10069                                                  # a prime factor of the twist's cofactor 2p - r
INF = np.zeros(24, dtype=np.uint64)                            # Z = 0

# the edges of the signed 4-bit recoding over the whole scalar (digit boundaries 7 / 8 / 9, carries through whole words,
# the top digit) and of the field
EDGE = ([0, 1, 2, 7, 8, 9, 15, 16, 17, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2]
        + [int(c * 64, 16) % R for c in "78f"]
        + [v for k in [4] + list(range(124, 133)) + [252, 253] for v in (1 << k, (1 << k) - 1)])


def mont_array(ints):
    buf = b"".join((x % R * o.MONT % R).to_bytes(32, "little") for x in ints)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def canon_all(pts):
    return [o.g2_canonical_affine(p) for p in np.asarray(pts, dtype=np.uint64).reshape(-1, 24)]


def g2_negated(pt):
    neg = pt.copy()
    for k in (8, 12):
        neg[k:k + 4] = o.int_to_limbs((P - o.limbs_to_int(pt[k:k + 4])) % P)
    return neg


def rand_z(rng):
    return (rng.randrange(1, P), rng.randrange(P))


# ---------------------------------------------------------------- 1. batch against the oracle
def test_scalar_mul_batch_vs_oracle(lsa):
    n, a, b = 300, 424242, 1717
    pts = o.arith_bases("g2", a, b, n)                        # un-normalised Jacobian
    _, vals = o.random_scalars(n, seed=4242)
    vals[:len(EDGE)] = EDGE
    pts[40] = 0                                                # infinity (Z = 0)
    pts[41] = o.generator("g2")
    sc = mont_array(vals)
    got = canon_all(lsa.scalar_mul_batch(pts, sc, group="g2"))
    logs = [(a + i * b) % R for i in range(n)]
    logs[41] = 1
    want = canon_all(o.batch_exp("g2", o.generator("g2"), mont_array([vals[i] * logs[i] for i in range(n)])))
    want[40] = None
    assert got == want
    for i in list(range(16)) + list(range(36, 52)):           # 32 items: libff's own scalar * point route as well
        assert got[i] == o.g2_canonical_affine(o.multi_exp("g2", pts[i:i + 1], sc[i:i + 1]))


# ---------------------------------------------------------------- 2. outside the subgroup
def test_scalar_mul_batch_outside_the_subgroup(lsa):
    """Points of the twist that are NOT in G2: the product must still be the integer multiple.  Any endomorphism shortcut
    (GLV, psi, the four-dimensional split) fails here, because those maps are scalars on the subgroup only."""
    rng = random.Random(2)
    t = pio.outside_point()
    bases = [t, m.g2_add(t, t), pl.twist_ladder(t, 3), pl.twist_ladder(t, 5)]
    vals = [EDGE[i] if i < 40 else rng.randrange(R) for i in range(64)]
    vals[40:44] = [R - 3, R - 8, R - 9, (1 << 253) + 8]
    pts = np.stack([o.g2_from_affine(bases[i % 4], rand_z(rng) if i % 3 else (1, 0)) for i in range(64)])
    got = canon_all(lsa.scalar_mul_batch(pts, mont_array(vals), group="g2"))
    want = [m.g2_mul(bases[i % 4], vals[i]) for i in range(64)]
    assert got == want
    assert want[9] != m.g2_neg(bases[1])                        # (r - 1) P = -P holds inside the subgroup only


# ---------------------------------------------------------------- 3. the rare branches of the complete addition
def recode(s, w):
    """The ladder's digits, least significant first: csrc/smul_g2.h recode_nibbles_256 for a window of w bits."""
    ndig = -(-256 // w)
    half = 1 << (w - 1)
    sp = s + sum(half << (w * j) for j in range(ndig - 1))
    return [((sp >> (w * j)) & ((1 << w) - 1)) - (half if j < ndig - 1 else 0) for j in range(ndig)]


def rare_branches(s, w, order):
    """(doublings, cancellations) the general addition meets for [s]T, T of odd order `order`: the accumulator is simulated
    as an integer mod `order` (w doublings, then + digit).  A finite accumulator equal to the table entry is the doubling
    branch, equal to its negative the cancellation."""
    acc, dbl, cancel = 0, 0, 0
    for d in reversed(recode(s, w)):
        acc = (acc << w) % order
        if d == 0:
            continue
        if acc != 0 and (acc - d) % order == 0:
            dbl += 1
        if acc != 0 and (acc + d) % order == 0:
            cancel += 1
        acc = (acc + d) % order
    return dbl, cancel, acc


@pytest.fixture(scope="module")
def small_order():
    """T = [r (2p - r) / 10069] S for the first twist point S = (i + u, y) for which T is finite, and all its multiples."""
    order = R * (2 * P - R)
    assert order % SMALL == 0 and order % 5864401 == 0 and order % 1875725156269 == 0
    i = 1
    while True:
        y = pl.f2_sqrt(pl.g2_rhs((i, 1)))
        i += 1
        if y is None:
            continue
        T = pl.twist_ladder(((i - 1, 1), y), order // SMALL)
        if T is not None:
            break
    mult = [None, T]
    for _ in range(SMALL - 2):
        mult.append(m.g2_add(mult[-1], T))
    assert m.g2_add(mult[-1], T) is None                      # order 10069 exactly (a prime)
    for k in (2, 77, 5000, SMALL - 1):
        assert mult[k] == m.g2_mul(T, k)
    return mult


def test_rare_branches_constructed(lsa, small_order):
    """For every table entry d and both signs a scalar whose LAST addition is a doubling (+) or cancels to infinity (-)."""
    w = lsa.smul_param("g2_window_bits")
    rng = random.Random(3)
    inv = pow(1 << w, -1, SMALL)
    vals, kinds = [], []
    for d in range(1, (1 << (w - 1))):
        for sign in (1, -1):
            q = rng.getrandbits(250 - w) | (1 << (249 - w))
            q += (sign * d * inv - q) % SMALL                   # 2^w q = +-d (mod 10069)
            s = (q << w) + d
            assert s < R and ((q << w) - sign * d) % SMALL == 0
            dbl, cancel, _ = rare_branches(s, w, SMALL)
            assert (dbl if sign == 1 else cancel) >= 1
            vals.append(s)
            kinds.append(sign)
    T = small_order[1]
    pts = np.stack([o.g2_from_affine(T, rand_z(rng) if i % 2 else (1, 0)) for i in range(len(vals))])
    got = canon_all(lsa.scalar_mul_batch(pts, mont_array(vals), group="g2"))
    want = [small_order[s % SMALL] for s in vals]
    assert got == want
    assert all((want[i] is None) == (kinds[i] == -1) for i in range(len(vals)))


def test_rare_branches_sweep(lsa, small_order):
    """8192 random scalars on the point of order 10069: prefix multiples collide with table entries often enough that the
    doubling and the cancellation inside the ladder's addition are each taken by at least 20 items (52 and 51 with the
    4-bit recoding)."""
    w = lsa.smul_param("g2_window_bits")
    n = 8192
    rng = np.random.default_rng(SMALL)
    vals = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]
    hits = [rare_branches(s, w, SMALL) for s in vals]
    n_dbl, n_cancel = sum(1 for h in hits if h[0]), sum(1 for h in hits if h[1])
    print("items that take the doubling branch: %d, the cancellation branch: %d" % (n_dbl, n_cancel))
    assert n_dbl >= 20 and n_cancel >= 20
    assert all(h[2] == s % SMALL for h, s in zip(hits, vals))  # the simulation is the ladder of this recoding
    T = o.g2_from_affine(small_order[1])
    got = canon_all(lsa.scalar_mul_batch(np.tile(T, (n, 1)), mont_array(vals), group="g2"))
    assert got == [small_order[s % SMALL] for s in vals]


# ---------------------------------------------------------------- 4. device buffers and the grid-stride wrap
@pytest.mark.parametrize("parity", ["even", "odd"])
def test_scalar_mul_batch_device_buffers_and_grid_stride(lsa, parity):
    """More items than the persistent grid holds, so that the loop wraps, with an even and an odd count (a kernel that
    gives an item to a lane pair meets a last pair with and without a neighbour).  Checked by the known-discrete-log
    identity: pts[i] = c_i G, so scalars[i] * pts[i] = batch_exp(G, s_i c_i)."""
    import torch
    n = lsa.smul_param("g2_resident_items") + 1000
    n += (n % 2) != (parity == "odd")
    assert n % 2 == (parity == "odd") and n > lsa.smul_param("g2_resident_items")
    a, b = 987654321, 1234577
    g = o.generator("g2")
    coef = [(a + i * b) % R for i in range(n)]
    d_pts = lsa.batch_exp("g2", g, torch.from_numpy(mont_array(coef).view(np.int64)).to("cuda:0"))
    rng = np.random.default_rng(7 + n)
    raw = rng.bytes(32 * n)
    vals = [int.from_bytes(raw[32 * i:32 * i + 32], "little") % R for i in range(n)]
    vals[-1], vals[-2] = R - 1, 8
    d_sc = torch.from_numpy(mont_array(vals).view(np.int64)).to("cuda:0")
    d_out = lsa.scalar_mul_batch(d_pts, d_sc, group="g2")
    assert tuple(d_out.shape) == (n, 24)
    d_want = lsa.batch_exp("g2", g, torch.from_numpy(mont_array([vals[i] * coef[i] for i in range(n)]).view(np.int64)).to("cuda:0"))
    lsa.synchronize()
    got = lsa.normalize("g2", d_out.cpu().numpy().view(np.uint64))
    want = lsa.normalize("g2", d_want.cpu().numpy().view(np.uint64))
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- 5. sparse matrix
def column_sums(vals, rows, col_ptr, exps):
    exps = np.asarray(exps, dtype=np.uint64).reshape(-1, 4)
    rows = np.asarray(rows, dtype=np.int64)
    out = []
    for j in range(len(col_ptr) - 1):
        lo, hi = int(col_ptr[j]), int(col_ptr[j + 1])
        out.append(None if lo == hi else o.g2_canonical_affine(o.multi_exp("g2", vals[lo:hi], exps[rows[lo:hi]], mode="inner")))
    return out


def test_sparse_matrix_msm_cplink_shape(lsa):
    """The CPlink relation matrix in CSC form with G2 entries: 2 rows, column 0 = (h), column 1 = (F[0]) in row 1, columns
    2..N+1 = (bases1[i]; F[i+1]), the remaining N columns empty."""
    N, seed = 64, 99
    h = o.arith_bases("g2", seed, 3, 1)[0]
    bases1 = o.arith_bases("g2", seed + 1, 5, N)
    F = o.arith_bases("g2", seed + 2, 7, N + 1)
    vals, rows, col_ptr = [h, F[0]], [0, 1], [0, 1, 2]
    for i in range(N):
        vals += [bases1[i], F[i + 1]]
        rows += [0, 1]
        col_ptr.append(len(vals))
    col_ptr += [len(vals)] * N
    vals = np.array(vals, dtype=np.uint64)
    k, _ = o.random_scalars(2, seed=11)
    got = canon_all(lsa.sparse_matrix_msm(vals, rows, col_ptr, k, group="g2"))
    assert len(got) == 2 * N + 2
    assert got == column_sums(vals, rows, col_ptr, k)
    assert all(c is None for c in got[N + 2:])                  # empty columns -> infinity


def test_sparse_matrix_msm_general_columns(lsa):
    """Ragged columns (0..9 non-zeros), generator-valued and infinity-valued entries, repeated rows, cancelling entries,
    exponents 0 and 1."""
    rng = np.random.default_rng(5)
    nrows, ncols = 7, 40
    pool = o.arith_bases("g2", 31337, 11, 64)
    gen = o.generator("g2")
    vals, rows, col_ptr = [], [], [0]
    for j in range(ncols):
        for _ in range(j % 10):
            t = rng.integers(0, 10)
            vals.append(INF if t == 0 else gen if t == 1 else pool[rng.integers(0, 64)])
            rows.append(int(rng.integers(0, nrows)))
        col_ptr.append(len(vals))
    vals += [pool[3], g2_negated(pool[3])]                      # P and -P under the same exponent -> infinity
    rows += [2, 2]
    col_ptr.append(len(vals))
    k, _ = o.random_scalars(nrows, seed=12)
    k[5] = o.fr_mont(0)
    k[6] = o.fr_mont(1)
    vals = np.array(vals, dtype=np.uint64)
    got = canon_all(lsa.sparse_matrix_msm(vals, rows, col_ptr, k, group="g2"))
    assert got == column_sums(vals, rows, col_ptr, k)
    assert got[-1] is None and got[0] is None


def test_sparse_matrix_msm_verifier_shape(lsa):
    """evalAsPolyOn over the commitments of 20 sumcheck rounds as one call: column i = the three non-constant coefficients of
    round i, exps = (r_i, r_i^2, r_i^3), rows[e] = e."""
    rounds = 20
    vals = o.arith_bases("g2", 777, 13, 3 * rounds)
    _, rs = o.random_scalars(rounds, seed=21)
    exps = mont_array([pow(r, e, R) for r in rs for e in (1, 2, 3)])
    rows = np.arange(3 * rounds, dtype=np.uint32)
    col_ptr = np.arange(0, 3 * rounds + 1, 3, dtype=np.uint64)
    got = canon_all(lsa.sparse_matrix_msm(vals, rows, col_ptr, exps, group="g2"))
    assert len(got) == rounds and got == column_sums(vals, rows, col_ptr, exps)


def test_sparse_matrix_msm_rejects_bad_input(lsa):
    import legosnark_amd
    vals = o.arith_bases("g2", 1, 1, 2)
    k, _ = o.random_scalars(2, seed=1)
    with pytest.raises(legosnark_amd.LsaError):
        lsa.sparse_matrix_msm(vals, [0, 2], [0, 2], k, group="g2")        # row index out of range
    with pytest.raises(legosnark_amd.LsaError):
        lsa.sparse_matrix_msm(vals, [0, 1], [1, 2], k, group="g2")        # col_ptr[0] != 0
    with pytest.raises(legosnark_amd.LsaError):
        lsa.sparse_matrix_msm(vals, [0, 1], [0, 2, 1, 2], k, group="g2")  # col_ptr not monotone
    assert lsa.sparse_matrix_msm(vals[:0], [], [0], k, group="g2").shape == (0, 24)   # the empty matrix


# ---------------------------------------------------------------- 6. randomised
SEEDS = [20261016, 7, 314159]
CASES = 50


def fuzz_scalars(rng, n):
    """Uniform scalars, each replaced by an edge of the signed-digit recoder (or its negative) with probability 1/4."""
    out = []
    for _ in range(n):
        if rng.random() < 0.25:
            v = rng.choice(EDGE)
            out.append((R - v) % R if rng.random() < 0.3 else v)
        else:
            out.append(rng.getrandbits(rng.choice([254, 254, 254, 128, 64, 16])) % R)
    return out


def fuzz_bases(rng, n):
    """n multiples of the generator with known discrete logs (0 = infinity among them) and a random Z each."""
    a, b = rng.randrange(1, R), rng.randrange(R)
    pts = o.arith_bases("g2", a, b, n)
    logs = [(a + i * b) % R for i in range(n)]
    for i in range(n):
        t = rng.randrange(12)
        if t == 0:
            pts[i], logs[i] = INF, 0
        elif t == 1:
            pts[i], logs[i] = o.generator("g2"), 1
        elif t < 6:
            pts[i] = o.g2_from_affine(o.g2_canonical_affine(pts[i]), rand_z(rng))
    return pts, logs


def case_scalar_mul(rng, lsa):
    n = rng.randrange(0, 201)
    pts, logs = fuzz_bases(rng, n) if n else (np.zeros((0, 24), dtype=np.uint64), [])
    vals = fuzz_scalars(rng, n)
    got = lsa.scalar_mul_batch(pts, mont_array(vals).reshape(-1, 4), group="g2")
    want = o.batch_exp("g2", o.generator("g2"), mont_array([vals[i] * logs[i] for i in range(n)])) if n else []
    return len(got) == n and canon_all(got) == canon_all(want), "n=%d" % n


def case_sparse(rng, lsa):
    nnz = rng.randrange(0, 201)
    nrows = rng.randrange(1, 13)
    ncols = rng.choice([0, 1, rng.randrange(1, 30), rng.randrange(1, 60)])
    pts, logs = fuzz_bases(rng, nnz) if nnz else (np.zeros((0, 24), dtype=np.uint64), [])
    cuts = sorted(rng.randrange(0, nnz + 1) for _ in range(max(ncols - 1, 0)))
    col_ptr = ([0] + cuts + [nnz]) if ncols else [0]
    if ncols == 0:
        pts, logs, nnz = pts[:0], [], 0
    rows = [rng.randrange(nrows) for _ in range(nnz)]
    exps = fuzz_scalars(rng, nrows)
    got = lsa.sparse_matrix_msm(pts, rows, col_ptr, mont_array(exps).reshape(-1, 4), group="g2")
    sums = [sum(exps[rows[e]] * logs[e] for e in range(col_ptr[j], col_ptr[j + 1])) % R for j in range(ncols)]
    want = o.batch_exp("g2", o.generator("g2"), mont_array(sums)) if ncols else []
    return len(got) == ncols and canon_all(got) == canon_all(want), "rows=%d cols=%d entries=%d" % (nrows, ncols, nnz)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kind", ["scalar_mul_batch", "sparse_matrix_msm"])
def test_fuzz_parity(lsa, kind, seed):
    """3 fixed seeds x 50 drawn cases per call, each against the oracle through the known discrete logs; a failure names the
    case seed and shape."""
    case = case_scalar_mul if kind == "scalar_mul_batch" else case_sparse
    master = random.Random("%s/%d" % (kind, seed))
    failed, executed = [], 0
    for _ in range(CASES):
        case_seed = master.randrange(1 << 32)
        ok, what = case(random.Random(case_seed), lsa)
        executed += 1
        if not ok:
            failed.append((case_seed, what))
    assert executed == CASES
    assert not failed, "%s seed %d: %d of %d cases failed: %s" % (
        kind, seed, len(failed), CASES, "; ".join("case seed %d (%s)" % f for f in failed[:8]))


# ---------------------------------------------------------------- 7. shim
def test_shim_overloads(lsa, tmp_path):
    """libff::lsa_scalar_mul_batch on 200 G2 points and libff::lsa_mtxmultiexp on a G2 matrix against the shim's own host
    operator* and + (tests/cpp/test_shim_smul_g2.cc), built against legosnark_amd/shim only."""
    import legosnark_amd
    if not os.path.exists(legosnark_amd.LIB_PATH):
        legosnark_amd.build()
    exe = str(tmp_path / "shim_smul_g2")
    libdir = os.path.join(ROOT, "legosnark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "legosnark_amd", "shim"),
                           os.path.join(ROOT, "tests", "cpp", "test_shim_smul_g2.cc"), "-o", exe,
                           "-L" + libdir, "-llegosnark_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:]


def test_smul_param_reports_the_compiled_shape(lsa):
    assert lsa.smul_param("g1_window_bits") == 4 and lsa.smul_param("g1_resident_items") == 512 * 256
    w, lanes, resident = (lsa.smul_param(k) for k in ("g2_window_bits", "g2_lanes_per_item", "g2_resident_items"))
    assert 2 <= w <= 8 and lanes in (1, 2) and resident > 0 and resident % (256 // lanes) == 0
    assert lsa.smul_param(99) == 0
