"""GPU suite: sparse Fr matrices resident on the device -- FrSparse.matvec (lsa_fr_sparse_matvec, both sides) and
fr_qap_witness (lsa_fr_qap_witness), the R1CS products and the witness map of a Groth16-style prover; csrc/fr_sparse.hip,
csrc/fr_sparse.h.

Every expected value is Python integers mod r.  The words of a value x are X = x 2^256 mod r, so on words a product is
X Y 2^-256 and sums stay sums: expected words of sum_e v_e x_e = (sum_e V_e X_e) 2^-256 mod r, with every coefficient -- the
units +1 and -1 included -- taken as a product.

The shapes follow the kernels' own figures, read from the library (fr_sparse_params): rows of 1 .. 5 entries, S - 1, S, S + 1
around the length S up to which a row is one lane's, K - 1, K, K + 1, 2 K + 3 around the chunk length K of the longer rows,
and matrices with one row fewer than, and exactly, the number of rows of S + 1 .. lane_max entries from which such rows
become lanes' too."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R
RINV = pow(MONT, -1, R)
ONES = (1 << 256) - 1
PLUS, MINUS = MONT, R - MONT                       # the canonical words of +1 and -1
GENERATOR, TWO_ADICITY = 5, 28                     # libff alt_bn128 Fr::multiplicative_generator, Fr::s


def raw(arr):
    """(n, 4) uint64 words -> the integers they spell."""
    b = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def unraw(xs):
    if not len(xs):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


def dec(arr):
    return [x * RINV % R for x in raw(arr)]


def enc(xs):
    return unraw([x % R * MONT % R for x in xs])


def rand_words(n, rng):
    """n canonical residues (below 2^252) as integers: any canonical residue is some value's Montgomery form."""
    return [int(rng.integers(0, 1 << 63)) | int(rng.integers(0, 1 << 63)) << 63 | int(rng.integers(0, 1 << 63)) << 126 |
            int(rng.integers(0, 1 << 63)) << 189 for _ in range(n)]


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


class Csr:
    """A CSR matrix as Python integers (the raw words of its coefficients) next to the arrays the library takes."""

    def __init__(self, rows, ncols):
        """rows: a list of rows, each a list of (column, raw words of the coefficient)."""
        self.nrows, self.ncols = len(rows), ncols
        self.rows = rows
        self.row_ptr = np.zeros(len(rows) + 1, dtype=np.uint64)
        self.row_ptr[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
        self.cols = np.array([c for r in rows for c, _ in r], dtype=np.uint32)
        self.vals = unraw([v for r in rows for _, v in r])

    def handle(self, lsa, keep_transpose=True):
        return lsa.FrSparse(self.vals, self.cols, self.row_ptr, self.ncols, keep_transpose)

    def transposed(self):
        t = [[] for _ in range(self.ncols)]
        for r, row in enumerate(self.rows):
            for c, v in row:
                t[c].append((r, v))
        return Csr(t, self.nrows)

    def times(self, x, side):
        """The expected words of the product with the raw words x."""
        if side == 1:
            return unraw([sum(v * x[c] for c, v in row) * RINV % R for row in self.rows])
        acc = [0] * self.ncols
        for r, row in enumerate(self.rows):
            for c, v in row:
                acc[c] += v * x[r]
        return unraw([a * RINV % R for a in acc])


def run(lsa, h, x, side, device):
    """The product in one mode; also: x is untouched."""
    if not device:
        keep = x.copy()
        got = h.matvec(x, side)
        assert np.array_equal(x, keep), "x was modified"
        return got
    import torch
    dx = to_dev(x)
    keep = dx.clone()
    out = h.matvec(dx, side)
    lsa.synchronize()
    assert torch.equal(dx, keep), "x was modified"
    return to_host(out)


@pytest.fixture(scope="module")
def shape(lsa):
    p = lsa.fr_sparse_params()
    assert 1 <= p["short_max"] <= p["lane_max"] < p["chunk"] and p["unit_max"] >= 1 and p["lane_fill"] >= 1
    return p


def coefficient(mix, e, rng):
    if mix == "general":
        return rand_words(1, rng)[0]
    if mix == "plus":
        return PLUS
    if mix == "minus":
        return MINUS
    if mix == "alternate":
        return MINUS if e & 1 else PLUS
    k = int(rng.integers(0, 6))
    return (PLUS, MINUS, 0, PLUS + R)[k] if k < 4 else rand_words(1, rng)[0]       # (an explicit zero; a non-canonical 1: general)


def special_x(n, rng):
    """n operands: random residues with 0, r - 1 and the pattern 2^256 - 1 among them."""
    x = rand_words(n, rng)
    for i, v in enumerate((0, R - 1, ONES, 1)):
        if i < n:
            x[(5 * i + 1) % n] = v
    return x


# ---------------------------------------------------------------------------------------------- single rows
@pytest.mark.parametrize("mix", ["general", "plus", "minus", "alternate", "mixed"])
def test_single_row_lengths(lsa, shape, mix):
    S, K = shape["short_max"], shape["chunk"]
    rng = np.random.default_rng(len(mix))
    ncols = 37
    x = special_x(ncols, rng)
    for n in sorted({1, 2, 3, 4, 5, S - 1, S, S + 1, shape["lane_max"], shape["lane_max"] + 1, K - 1, K, K + 1, 2 * K + 3}):
        if n < 1:
            continue
        m = Csr([[(int(rng.integers(0, ncols)), coefficient(mix, e, rng)) for e in range(n)]], ncols)
        h = m.handle(lsa)
        assert (h.rows, h.cols, h.nnz) == (1, ncols, n)
        want1, want0 = m.times(x, 1), m.times([x[3]], 0)
        for device in (False, True):
            assert np.array_equal(run(lsa, h, unraw(x), 1, device), want1), (mix, n, device, "side 1")
            assert np.array_equal(run(lsa, h, unraw([x[3]]), 0, device), want0), (mix, n, device, "side 0")
        h.close()


def test_minus_row_summing_to_zero(lsa, shape):
    rng = np.random.default_rng(5)
    for pairs in (1, shape["unit_max"] // 2 + 1, shape["short_max"], shape["chunk"] // 2 + 1):
        a = rand_words(pairs, rng)
        a = [v % R for v in a]
        x = a + [(R - v) % R for v in a]
        m = Csr([[(c, MINUS) for c in range(2 * pairs)]], 2 * pairs)
        h = m.handle(lsa, keep_transpose=False)
        assert raw(h.matvec(unraw(x))) == [0], pairs
        h.close()


def test_many_middling_rows_become_lanes(lsa, shape):
    """Rows of short_max + 1 .. lane_max entries are wavefronts' until a matrix has lane_fill of them, then lanes': one row
    fewer than that and exactly that many, lengths at both ends of the range, and a long row that stays chunked."""
    S, Lmax, fill, K = shape["short_max"], shape["lane_max"], shape["lane_fill"], shape["chunk"]
    assert S <= Lmax < K
    if S == Lmax:
        return
    rng = np.random.default_rng(17)
    ncols = 97
    x = special_x(ncols, rng)
    pool = rand_words(64, rng) + [PLUS, MINUS] * 16

    def row(n):
        return [(int(c), pool[int(k)]) for c, k in zip(rng.integers(0, ncols, n), rng.integers(0, len(pool), n))]

    rows = [row(K + 5), row(Lmax)] + [row(S + 1) for _ in range(fill - 3)] + [row(Lmax)]
    for extra in ([], [row(S + 1)]):                                        # fill - 1 middling rows, then fill
        m = Csr(rows + extra + [row(Lmax + 1), row(2)], ncols)
        h = m.handle(lsa, keep_transpose=False)
        want = m.times(x, 1)
        assert np.array_equal(h.matvec(unraw(x), 1), want), len(extra)
        h.close()


# ---------------------------------------------------------------------------------------------- one mixed matrix
@pytest.fixture(scope="module")
def mixed(shape):
    S, K = shape["short_max"], shape["chunk"]
    rng = np.random.default_rng(11)
    ncols = 2 * K + 9
    lengths = [2 * K + 3, 0, 3, 0, 0, S, S + 1, 1, 2, K, 0, S - 1, 5, K + 1, 4, 0, 70, K - 1]      # a long row first and last
    rows = []
    for i, n in enumerate(lengths):
        mix = ("mixed", "plus", "general", "alternate", "minus")[i % 5]
        row = [(int(rng.integers(0, ncols)), coefficient(mix, e, rng)) for e in range(n)]
        if n >= 2:
            row[1] = (row[0][0], row[1][1])                                 # a duplicate column in the row
        if n >= 5:
            row[4] = (row[0][0], MINUS)                                     # ... and once more, as a unit
        rows.append(row)
    rows[2] = [(7, PLUS), (7, PLUS), (7, rand_words(1, rng)[0])]            # one column three times
    m = Csr(rows, ncols)
    return m, special_x(ncols, rng), special_x(len(rows), rng)


@pytest.mark.parametrize("device", [False, True])
def test_mixed_matrix_both_sides(lsa, mixed, device):
    m, x1, x0 = mixed
    h = m.handle(lsa)
    assert np.array_equal(run(lsa, h, unraw(x1), 1, device), m.times(x1, 1))
    got0 = run(lsa, h, unraw(x0), 0, device)
    assert np.array_equal(got0, m.times(x0, 0))
    ht = m.transposed().handle(lsa)                                         # side 0 = side 1 of the explicit transpose
    assert (ht.rows, ht.cols, ht.nnz) == (m.ncols, m.nrows, h.nnz)
    assert np.array_equal(run(lsa, ht, unraw(x0), 1, device), got0)
    assert np.array_equal(run(lsa, ht, unraw(x1), 0, device), m.times(x1, 1))
    h.close()
    ht.close()


def test_dense_cross_check(lsa):
    rows, cols = 33, 70
    rng = np.random.default_rng(3)
    M = rand_words(rows * cols, rng)
    M[5], M[cols + 1], M[100] = PLUS, MINUS, 0
    m = Csr([[(c, M[r * cols + c]) for c in range(cols)] for r in range(rows)], cols)
    h = m.handle(lsa)
    for side, n in ((1, cols), (0, rows)):
        w = unraw(special_x(n, rng))
        dense = lsa.fr_matvec(unraw(M), w, rows, cols, side)
        assert np.array_equal(h.matvec(w, side), dense), side
        got = h.matvec(to_dev(w), side)
        lsa.synchronize()                                                    # (the library's stream, which torch's copy does not wait for)
        assert np.array_equal(to_host(got), dense), side
    h.close()


# ---------------------------------------------------------------------------------------------- modes, refusals, degenerate shapes
def test_out_argument_and_overlap(lsa):
    import torch
    rng = np.random.default_rng(8)
    m = Csr([[(c, rand_words(1, rng)[0]) for c in range(4)] for _ in range(4)], 4)
    h = m.handle(lsa)
    x = special_x(4, rng)
    dx = to_dev(unraw(x))
    out = torch.zeros((4, 4), dtype=torch.int64, device="cuda:0")
    assert h.matvec(dx, 1, out=out) is out
    lsa.synchronize()
    assert np.array_equal(to_host(out), m.times(x, 1))
    with pytest.raises(lsa.LsaError, match="overlaps"):
        h.matvec(dx, 1, out=dx)
    buf = torch.zeros((9, 4), dtype=torch.int64, device="cuda:0")
    with pytest.raises(lsa.LsaError, match="overlaps"):
        h.matvec(buf[:4], 1, out=buf.view(-1)[8:24])                         # half of out inside x
    with pytest.raises(lsa.LsaError, match="aligned"):
        h.matvec(buf[:4], 1, out=buf.view(-1)[17:33])
    hx = unraw(x)
    rc = lsa.lib().lsa_fr_sparse_matvec(h.handle, hx.ctypes.data_as(C.c_void_p), 1, hx.ctypes.data_as(C.c_void_p), 0)
    assert rc == -2 and b"overlaps" in lsa.lib().lsa_last_error()
    assert np.array_equal(hx, unraw(x))
    with pytest.raises(ValueError):
        h.matvec(unraw(x), 2)
    with pytest.raises(ValueError):
        h.matvec(unraw(x[:3]), 1)
    h1 = m.handle(lsa, keep_transpose=False)
    assert np.array_equal(h1.matvec(unraw(x), 1), m.times(x, 1))
    with pytest.raises(lsa.LsaError, match="keep_transpose"):
        h1.matvec(unraw(x), 0)
    h1.close()
    h.close()
    h.close()                                                                # closing twice is harmless
    with pytest.raises(ValueError):
        h.matvec(unraw(x), 1)


def test_degenerate_shapes(lsa):
    rng = np.random.default_rng(9)
    # no rows: nothing to compute on side 1, zeros on side 0
    h = Csr([], 5).handle(lsa)
    assert (h.rows, h.cols, h.nnz) == (0, 5, 0)
    assert h.matvec(unraw(special_x(5, rng)), 1).shape == (0, 4)
    assert raw(h.matvec(np.zeros((0, 4), dtype=np.uint64), 0)) == [0] * 5
    h.close()
    # rows without entries: zeros, in both modes, over whatever out held
    import torch
    h = Csr([[], [], []], 4).handle(lsa)
    assert raw(h.matvec(unraw(special_x(4, rng)), 1)) == [0] * 3
    out = torch.full((3, 4), -1, dtype=torch.int64, device="cuda:0")
    h.matvec(to_dev(unraw(special_x(4, rng))), 1, out=out)
    lsa.synchronize()
    assert raw(to_host(out)) == [0] * 3
    assert raw(h.matvec(unraw(special_x(3, rng)), 0)) == [0] * 4
    h.close()
    # one column
    m = Csr([[(0, PLUS)], [], [(0, MINUS), (0, rand_words(1, rng)[0])], [(0, 0)]], 1)
    h = m.handle(lsa)
    for v in (0, R - 1, ONES, rand_words(1, rng)[0]):
        assert np.array_equal(h.matvec(unraw([v]), 1), m.times([v], 1))
    x0 = special_x(4, rng)
    assert np.array_equal(h.matvec(unraw(x0), 0), m.times(x0, 0))
    h.close()


def test_creation_refusals(lsa):
    L = lsa.lib()
    vals = unraw([PLUS, MINUS, 5])
    cols = np.array([0, 1, 2], dtype=np.uint32)
    ptr = np.array([0, 2, 3], dtype=np.uint64)

    def create(v, c, p, nrows, ncols, nnz):
        as_ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        h = C.c_void_p(0xdead)
        # (a failing call that set no message would leave this marker, a successful one in between too)
        assert L.lsa_fr_sparse_create(None, None, None, 0, 0, 0, 0, None) == -2 and b"null out" in L.lsa_last_error()
        rc = L.lsa_fr_sparse_create(as_ptr(v), as_ptr(c), as_ptr(p), nrows, ncols, nnz, 1, C.byref(h))
        return rc, h, L.lsa_last_error()

    def refused(what, *args):
        rc, h, msg = create(*args)
        assert rc == -2, what
        assert not h.value, what
        assert b"fr_sparse_create" in msg and b"null out" not in msg, (what, msg)

    rc, h, _ = create(vals, cols, ptr, 2, 3, 3)                               # the arrays are fine as they are
    assert rc == 0 and h.value
    L.lsa_fr_sparse_destroy(h)
    refused("row_ptr[0] != 0", vals, cols, np.array([1, 2, 3], dtype=np.uint64), 2, 3, 3)
    refused("decreasing row_ptr", vals, cols, np.array([0, 3, 2, 3], dtype=np.uint64), 3, 3, 3)
    refused("row_ptr[nrows] < nnz", vals, cols, np.array([0, 1, 2], dtype=np.uint64), 2, 3, 3)
    refused("row_ptr[nrows] > nnz", vals, cols, np.array([0, 2, 4], dtype=np.uint64), 2, 3, 3)
    refused("column == ncols", vals, cols, ptr, 2, 2, 3)
    refused("column far out", vals, np.array([0, 0xffffffff, 2], dtype=np.uint32), ptr, 2, 3, 3)
    refused("null vals", None, cols, ptr, 2, 3, 3)
    refused("null cols", vals, None, ptr, 2, 3, 3)
    refused("null row_ptr", vals, cols, None, 2, 3, 3)
    refused("entries without rows", vals, cols, ptr, 0, 3, 3)
    refused("nrows = 2^32", vals, cols, ptr, 1 << 32, 3, 3)
    refused("ncols = 2^32", vals, cols, ptr, 2, 1 << 32, 3)
    with pytest.raises(lsa.LsaError):
        lsa.FrSparse(vals, cols, ptr, 2)
    # null arrays with empty extents are fine
    rc, h, _ = create(None, None, np.array([0, 0], dtype=np.uint64), 1, 3, 0)
    assert rc == 0 and h.value
    L.lsa_fr_sparse_destroy(h)
    rc, h, _ = create(None, None, None, 0, 0, 0)
    assert rc == 0 and h.value
    L.lsa_fr_sparse_destroy(h)


# ---------------------------------------------------------------------------------------------- the witness map
def root_of_unity(log_n):
    w = pow(GENERATOR, (R - 1) >> TWO_ADICITY, R)
    for _ in range(TWO_ADICITY - log_n):
        w = w * w % R
    return w


class Dom:
    """The basic radix-2 domain of 2^big_log points, or libfqfft's step domain of 2^big_log + 2^small_log."""

    def __init__(self, big_log, small_log):
        self.big_log, self.small_log = big_log, small_log
        self.big, self.small = 1 << big_log, 0 if small_log is None else 1 << small_log
        self.m = self.big + self.small
        self.w = root_of_unity(big_log if small_log is None else big_log + 1)
        if small_log is None:
            self.pts = [pow(self.w, i, R) for i in range(self.m)]
        else:
            sigma = pow(self.w, 2 * self.big // self.small, R)
            self.pts = [pow(self.w, 2 * i, R) for i in range(self.big)] + [self.w * pow(sigma, j, R) % R for j in range(self.small)]
        assert len(set(self.pts)) == self.m

    def Z(self, t):
        z = 1
        for p in self.pts:
            z = z * (t - p) % R
        return z

    def lagrange(self, t):
        out = []
        for i, xi in enumerate(self.pts):
            num = den = 1
            for j, xj in enumerate(self.pts):
                if j != i:
                    num, den = num * (t - xj) % R, den * (xi - xj) % R
            out.append(num * pow(den, -1, R) % R)
        return out


def matrix_product_r1cs(n, rng):
    """The constraint system of src/examples/legogrothmatrix.cc for n x n matrices, as libsnark's gadgets lay it out: variable
    0 is the constant 1; rows of M and columns of N; per output U[r][c] an inner-product gadget with n - 1 running sums
    S_0 .. S_(n-2) and the constraints M[r][0] N[0][c] = S_0, M[r][i] N[i][c] = S_i - S_(i-1) (the last S is U[r][c]) -- every
    coefficient +1 or -1.  Then the one input-consistency row the QAP reduction appends for z[0]: A = z[0], B = C = 0.
    Returns the three Csr matrices and a satisfying assignment (values, not words)."""
    nvars = 1
    Mv, Nv = [], []
    for _ in range(n):
        Mv.append(list(range(nvars, nvars + n))); nvars += n
        Nv.append(list(range(nvars, nvars + n))); nvars += n
    z = [1] + [int(rng.integers(0, 1 << 32)) for _ in range(nvars - 1)]
    A, B, Cm = [], [], []
    for r in range(n):
        for c in range(n):
            u = nvars
            sums = list(range(nvars + 1, nvars + n)) + [u]                    # S_0 .. S_(n-2), then the result
            nvars += n
            z += [0] * n
            acc = 0
            for i in range(n):
                a, b = Mv[r][i], Nv[c][i]
                acc = (acc + z[a] * z[b]) % R
                z[sums[i]] = acc
                A.append([(a, PLUS)])
                B.append([(b, PLUS)])
                Cm.append([(sums[i], PLUS)] + ([(sums[i - 1], MINUS)] if i else []))
    A.append([(0, PLUS)]); B.append([]); Cm.append([])
    return Csr(A, nvars), Csr(B, nvars), Csr(Cm, nvars), z


def horner(coeffs, t):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * t + c) % R
    return acc


@pytest.fixture(scope="module")
def r1cs():
    return matrix_product_r1cs(2, np.random.default_rng(21))


def test_r1cs_generator_is_satisfied(r1cs):
    """(CPU arithmetic only: the generator's own sanity, so that a failure below is the library's.)"""
    A, B, Cm, z = r1cs
    assert (A.nrows, A.ncols) == (9, 17)
    zw = [v * MONT % R for v in z]
    a, b, c = (dec(m.times(zw, 1)) for m in (A, B, Cm))
    assert all((x * y - w) % R == 0 for x, y, w in zip(a, b, c)) and a[-1] == 1


@pytest.mark.parametrize("key", [(4, None), (3, 2)], ids=["basic16", "step8+4"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_witness_map(lsa, r1cs, key, device):
    A, B, Cm, z = r1cs
    D = Dom(*key)
    assert A.nrows <= D.m
    hs = [m.handle(lsa, keep_transpose=False) for m in (A, B, Cm)]
    omega, coset = enc([D.w])[0], enc([GENERATOR])[0]
    rng = np.random.default_rng(31)
    d = [v % R for v in rand_words(3, rng)]
    t = rand_words(1, rng)[0] % R

    def witness(zvals, d123):
        zz = enc(zvals)
        if not device:
            keep = zz.copy()
            h = lsa.fr_qap_witness(*hs, zz, D.big_log, D.small_log, omega=omega, coset=coset, d123=d123)
            abc = [m.matvec(zz) for m in hs]
            assert np.array_equal(zz, keep), "z was modified"
            ref = lsa.fr_hadamard_quotient(*abc, np.zeros((3, 4), dtype=np.uint64) if d123 is None else d123, D.big_log, D.small_log, omega=omega, coset=coset)
            return h, ref, abc
        import torch
        dz = to_dev(zz)
        keep = dz.clone()
        h = lsa.fr_qap_witness(*hs, dz, D.big_log, D.small_log, omega=omega, coset=coset, d123=d123)
        abc = [m.matvec(dz) for m in hs]
        ref = lsa.fr_hadamard_quotient(*abc, np.zeros((3, 4), dtype=np.uint64) if d123 is None else d123, D.big_log, D.small_log, omega=omega, coset=coset)
        lsa.synchronize()
        assert torch.equal(dz, keep), "z was modified"
        return to_host(h), to_host(ref), [to_host(v) for v in abc]

    def identity_gap(h, abc, dd):
        """(A(t) + d1 Z(t)) (B(t) + d2 Z(t)) - (C(t) + d3 Z(t)) - H(t) Z(t) on Python integers."""
        lag, zt = D.lagrange(t), D.Z(t)
        at, bt, ct = (sum(v * l for v, l in zip(dec(vec), lag)) % R for vec in abc)
        return ((at + dd[0] * zt) * (bt + dd[1] * zt) - (ct + dd[2] * zt) - horner(dec(h), t) * zt) % R

    # no blinding: Groth16's H; equal to the standalone quotient of the three products, byte for byte
    h, ref, abc = witness(z, None)
    assert h.shape == (D.m + 1, 4) and np.array_equal(h, ref)
    assert [np.array_equal(v, m.times(raw(enc(z)), 1)) for v, m in zip(abc, (A, B, Cm))] == [True] * 3
    assert identity_gap(h, abc, [0, 0, 0]) == 0
    # blinded
    h, ref, abc = witness(z, enc(d))
    assert np.array_equal(h, ref)
    assert identity_gap(h, abc, d) == 0
    # one entry of z changed: the constraints no longer hold, A B - C is no multiple of Z, and the same identity fails
    bad = list(z)
    bad[3] = (bad[3] + 1) % R
    h, ref, abc = witness(bad, enc(d))
    assert np.array_equal(h, ref)
    assert identity_gap(h, abc, d) != 0
    for m in hs:
        m.close()


def test_witness_map_refusals(lsa, r1cs):
    A, B, Cm, z = r1cs
    a, b, c = (m.handle(lsa, keep_transpose=False) for m in (A, B, Cm))
    zz = enc(z)
    omega, coset = enc([root_of_unity(4)])[0], enc([GENERATOR])[0]
    assert lsa.fr_qap_witness(a, b, c, zz, 4, None, omega=omega, coset=coset).shape == (17, 4)
    fewer_rows = Csr(A.rows[:-1], A.ncols).handle(lsa, keep_transpose=False)
    fewer_cols = Csr([[(0, PLUS)]] * A.nrows, A.ncols - 1).handle(lsa, keep_transpose=False)
    for trio, what in (((fewer_rows, b, c), "one shape"), ((a, fewer_rows, c), "one shape"), ((a, b, fewer_cols), "one shape")):
        with pytest.raises(lsa.LsaError, match=what):
            lsa.fr_qap_witness(*trio, zz, 4, None, omega=omega, coset=coset)
    with pytest.raises(lsa.LsaError, match="9 constraints on a domain of m = 8"):
        lsa.fr_qap_witness(a, b, c, zz, 3, None, omega=enc([root_of_unity(3)])[0], coset=coset)
    with pytest.raises(lsa.LsaError, match="fr_hadamard_quotient"):              # the domain and coset refusals are the quotient's
        lsa.fr_qap_witness(a, b, c, zz, 29, None, omega=omega, coset=coset)
    with pytest.raises(lsa.LsaError, match="fr_hadamard_quotient"):
        lsa.fr_qap_witness(a, b, c, zz, 4, 4, omega=omega, coset=coset)
    with pytest.raises(lsa.LsaError, match="coset_g"):
        lsa.fr_qap_witness(a, b, c, zz, 4, None, omega=omega, coset=enc([1])[0])
    for m in (a, b, c, fewer_rows, fewer_cols):
        m.close()
