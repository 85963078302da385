"""GPU suite: Fr vectors as row-major matrices -- lsa_fr_matmul (the witness C = A B of the matrix-product gadget,
matrixsc.cc:83-91) and lsa_fr_matvec (the contraction in DPMatrixMle's constructor, mle.h:241-258, and its column-wise twin);
csrc/fr_matrix.hip, csrc/fr_dot.h.

Every expected value is Python integers mod r.  The words of a value x are X = x 2^256 mod r, so on words a product is
X Y 2^-256 and sums stay sums: expected words of sum_k a_k b_k = (sum_k A_k B_k) 2^-256 mod r.

The shapes follow the kernels' own figures, read from the library (fr_matrix_params): dimensions 1, T - 1, T, T + 1, 2 T + 3
around the tile edge T of C, summed lengths 1 .. 5, K - 1, K, K + 1, 2 K + 3 around the K-step, one length past the number
of products csrc/fr_dot.h sums before it brings the running sum back below 2r, and for fr_matvec the shapes on either side
of its single-workgroup and split-and-finish thresholds (fr_matvec_slices)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R
RINV = pow(MONT, -1, R)


def raw(arr):
    """(n, 4) uint64 words -> the integers they spell."""
    b = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def unraw(xs):
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


def dec(arr):
    return [x * RINV % R for x in raw(arr)]


def enc(xs):
    return unraw([x % R * MONT % R for x in xs])


def rand_fr(n, seed):
    """n canonical residues (below 2^252) as words: any canonical residue is some value's Montgomery form."""
    a = np.random.default_rng(seed).integers(0, 1 << 64, (n, 4), dtype=np.uint64, endpoint=False)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


def filled(n, word):
    return unraw([word] * n)


def identity(n):
    return unraw([MONT if i == j else 0 for i in range(n) for j in range(n)])


def matmul_words(a, b, rows, inner, cols):
    A, B = raw(a), raw(b)
    Bt = [B[c::cols] for c in range(cols)]
    out = []
    for r in range(rows):
        row = A[r * inner:(r + 1) * inner]
        out += [sum(x * y for x, y in zip(row, col)) * RINV % R for col in Bt]
    return unraw(out)


def matvec_words(m, w, rows, cols, side):
    M, W = raw(m), raw(w)
    if side == 0:
        return unraw([sum(W[r] * M[r * cols + c] for r in range(rows)) * RINV % R for c in range(cols)])
    return unraw([sum(x * y for x, y in zip(M[r * cols:(r + 1) * cols], W)) * RINV % R for r in range(rows)])


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def run_matmul(lsa, a, b, rows, inner, cols, device):
    """The product in one mode; in device mode also: the inputs are untouched."""
    if not device:
        ka, kb = a.copy(), b.copy()
        got = lsa.fr_matmul(a, b, rows, inner, cols)
        assert np.array_equal(a, ka) and np.array_equal(b, kb), "an input was modified"
        return got
    import torch
    da, db = to_dev(a), to_dev(b)
    ka, kb = da.clone(), db.clone()
    out = lsa.fr_matmul(da, db, rows, inner, cols)
    lsa.synchronize()
    assert torch.equal(da, ka) and torch.equal(db, kb), "an input was modified"
    return to_host(out)


def run_matvec(lsa, m, w, rows, cols, side, device):
    if not device:
        km, kw = m.copy(), w.copy()
        got = lsa.fr_matvec(m, w, rows, cols, side)
        assert np.array_equal(m, km) and np.array_equal(w, kw), "an input was modified"
        return got
    import torch
    dm, dw = to_dev(m), to_dev(w)
    km, kw = dm.clone(), dw.clone()
    out = lsa.fr_matvec(dm, dw, rows, cols, side)
    lsa.synchronize()
    assert torch.equal(dm, km) and torch.equal(dw, kw), "an input was modified"
    return to_host(out)


@pytest.fixture(scope="module")
def shape(lsa):
    return lsa.fr_matrix_params()


# ---------------------------------------------------------------------------------------------- matmul, exact
def matmul_shapes(p):
    """(rows_a, inner, cols_b): every dimension class beside every other at inner = K + 1, every class of inner beside a
    rotating pair of dimensions, the non-square case, and the length past fr_dot.h's partial-sum count."""
    T, K = p["matmul_tile"], p["matmul_kstep"]
    dims = [1, T - 1, T, T + 1, 2 * T + 3]
    inners = [1, 2, 3, 4, 5, K - 1, K, K + 1, 2 * K + 3]
    out = [(r, K + 1, c) for r in dims for c in dims]
    out += [(dims[i % 5], k, dims[(2 * i + 1) % 5]) for i, k in enumerate(inners)]
    out += [(130, 67, 129), (T + 1, p["dot_max_partials"] * p["dot_group"] + 1, K + 1)]
    return out


_products = {}


def product_case(key):
    """Random operands of a shape and their product in Python integers: computed once, shared, never modified."""
    if key not in _products:
        rows, inner, cols = key
        v = rand_fr(rows * inner + inner * cols, 7919 * rows + 104729 * inner + cols)
        a, b = v[:rows * inner].copy(), v[rows * inner:].copy()
        want = matmul_words(a, b, rows, inner, cols)
        for x in (a, b, want):
            x.setflags(write=False)
        _products[key] = (a, b, want)
    return _products[key]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_matmul_random_operands_at_every_tile_edge(lsa, shape, device):
    for key in matmul_shapes(shape):
        a, b, want = product_case(key)
        assert np.array_equal(run_matmul(lsa, a, b, *key, device), want), key


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_matmul_zero_identity_and_largest_entries(lsa, shape, device):
    T, K = shape["matmul_tile"], shape["matmul_kstep"]
    n, longest = T + 1, 2 * K + 3
    past = shape["dot_max_partials"] * shape["dot_group"] + 1
    b = rand_fr(n * n, 31)
    zero = np.zeros((n * n, 4), dtype=np.uint64)
    assert np.array_equal(run_matmul(lsa, zero, b, n, n, n, device), zero)
    assert np.array_equal(run_matmul(lsa, b, zero, n, n, n, device), zero)
    assert np.array_equal(run_matmul(lsa, identity(n), b, n, n, n, device), b)
    assert np.array_equal(run_matmul(lsa, b, identity(n), n, n, n, device), b)
    # every entry r - 1 in both operands: every limb product of every column at the top of what canonical inputs reach, at
    # the largest summed length of the shape classes and at the length that makes fr_dot.h fold its running sum
    for inner in (longest, past):
        rows, cols = 2 * T + 3, T - 1
        want = filled(rows * cols, inner * (R - 1) * (R - 1) * RINV % R)
        got = run_matmul(lsa, filled(rows * inner, R - 1), filled(inner * cols, R - 1), rows, inner, cols, device)
        assert np.array_equal(got, want), inner


def test_matmul_summed_length_zero_and_empty_outputs(lsa):
    a = rand_fr(12, 5)
    assert np.array_equal(lsa.fr_matmul(a[:0], a[:0], 3, 0, 4), np.zeros((12, 4), dtype=np.uint64))
    out = to_dev(rand_fr(12, 6))
    got = lsa.fr_matmul(to_dev(a[:0]), to_dev(a[:0]), 3, 0, 4, out=out)
    lsa.synchronize()
    assert got is out and not to_host(out).any()
    assert lsa.fr_matmul(a[:0], a, 0, 3, 4).shape == (0, 4)
    assert lsa.fr_matmul(a, a[:0], 4, 3, 0).shape == (0, 4)


# ---------------------------------------------------------------------------------------------- matmul, medium
@pytest.mark.parametrize("key", [(256, 256, 256), (300, 257, 260)], ids=str)
def test_matmul_medium_by_two_random_vectors(lsa, key):
    """A (B x) = C x for two random x, in Python integers (O(n^2)); outputs canonical.  Host and device mode agree byte for byte."""
    rows, inner, cols = key
    v = rand_fr(rows * inner + inner * cols, 4242 + rows)
    a, b = v[:rows * inner], v[rows * inner:]
    c = run_matmul(lsa, a, b, rows, inner, cols, device=True)
    assert np.array_equal(run_matmul(lsa, a, b, rows, inner, cols, device=False), c)
    Cw = raw(c)
    assert max(Cw) < R, "an output is not canonical"
    A, B = dec(a), dec(b)
    Cv = [x * RINV % R for x in Cw]
    for seed in (1, 2):
        x = dec(rand_fr(cols, 900 + seed))
        bx = [sum(p * q for p, q in zip(B[k * cols:(k + 1) * cols], x)) % R for k in range(inner)]
        abx = [sum(p * q for p, q in zip(A[r * inner:(r + 1) * inner], bx)) % R for r in range(rows)]
        cx = [sum(p * q for p, q in zip(Cv[r * cols:(r + 1) * cols], x)) % R for r in range(rows)]
        assert abx == cx, seed


# ---------------------------------------------------------------------------------------------- matvec, exact
MATVEC_SHAPES = [(1, 1), (1, 65), (65, 1), (3, 4096), (4096, 3), (63, 65), (257, 129), (512, 512)]
_sums = {}


def sums_case(key):
    """Random M and both weight vectors of a shape, with both sides' expected sums: computed once, shared, never modified."""
    if key not in _sums:
        rows, cols = key
        v = rand_fr(rows * cols + rows + cols, 1009 * rows + cols)
        m, w0, w1 = v[:rows * cols].copy(), v[rows * cols:rows * cols + rows].copy(), v[rows * cols + rows:].copy()
        want = (matvec_words(m, w0, rows, cols, 0), matvec_words(m, w1, rows, cols, 1))
        for x in (m, w0, w1) + want:
            x.setflags(write=False)
        _sums[key] = (m, (w0, w1), want)
    return _sums[key]


def test_matvec_shapes_cover_every_path(lsa, shape):
    """A later retune of the thresholds must not silently stop covering a path: the shapes below are on the side of each
    threshold the tests rely on."""
    assert lsa.fr_matvec_slices(4096, 3, 0) > 1 and lsa.fr_matvec_slices(3, 4096, 1) > 1          # split and finish
    assert lsa.fr_matvec_slices(512, 512, 0) > 1 and lsa.fr_matvec_slices(512, 512, 1) > 1
    assert lsa.fr_matvec_slices(3, 4096, 0) == 1 and lsa.fr_matvec_slices(4096, 3, 1) == 1          # many workgroups, no slices
    assert 3 * 4096 > shape["matvec_small"] >= 63 * 65                                             # one workgroup: 63 x 65 and below
    assert lsa.fr_matvec_slices(63, 65, 0) == 1 and lsa.fr_matvec_slices(63, 65, 1) == 1
    assert lsa.fr_matvec_slices(5, 5, 2) == 0


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("key", MATVEC_SHAPES, ids=str)
def test_matvec_random_operands(lsa, key, device):
    m, w, want = sums_case(key)
    for side in (0, 1):
        assert np.array_equal(run_matvec(lsa, m, w[side], *key, side, device), want[side]), side


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_matvec_zero_identity_and_largest_entries(lsa, device):
    for rows, cols in [(1, 1), (63, 65), (257, 129)]:
        m, w, _ = sums_case((rows, cols))
        for side in (0, 1):
            nout = rows if side else cols
            zero = np.zeros((nout, 4), dtype=np.uint64)
            assert np.array_equal(run_matvec(lsa, np.zeros_like(m), w[side], rows, cols, side, device), zero)
            assert np.array_equal(run_matvec(lsa, m, np.zeros_like(w[side]), rows, cols, side, device), zero)
    for n in (1, 65, 512):
        w = rand_fr(n, 77 + n)
        for side in (0, 1):
            assert np.array_equal(run_matvec(lsa, identity(n), w, n, n, side, device), w), (n, side)
    # every entry r - 1: through the split path (4096 summed on either side) and the single-workgroup path
    for rows, cols in [(3, 4096), (4096, 3), (63, 65), (512, 512)]:
        for side in (0, 1):
            nout, nsum = (rows, cols) if side else (cols, rows)
            want = filled(nout, nsum * (R - 1) * (R - 1) * RINV % R)
            got = run_matvec(lsa, filled(rows * cols, R - 1), filled(nsum, R - 1), rows, cols, side, device)
            assert np.array_equal(got, want), (rows, cols, side)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_matvec_one_lane_sums_past_the_partial_count(lsa, shape, device):
    """Side 0 without slices and with more summed rows than fr_dot.h adds up before it brings its running sum back below 2r:
    ONE lane pushes a 61st partial inside k_fr_matvec_cols' loop.  One past the count and 4096 rows, both on the
    single-workgroup path; random values and every entry r - 1.  (Side 1 of the same shapes rides along.)"""
    past = shape["dot_max_partials"] * shape["dot_group"]
    for rows, cols in [(past + 1, 3), (4096, 1)]:
        assert rows > past and rows * cols <= shape["matvec_small"] and lsa.fr_matvec_slices(rows, cols, 0) == 1, (rows, cols)
        m, w, want = sums_case((rows, cols))
        for side in (0, 1):
            assert np.array_equal(run_matvec(lsa, m, w[side], rows, cols, side, device), want[side]), (rows, cols, side)
        expect = filled(cols, rows * (R - 1) * (R - 1) * RINV % R)
        assert np.array_equal(run_matvec(lsa, filled(rows * cols, R - 1), filled(rows, R - 1), rows, cols, 0, device), expect), (rows, cols)


def test_matvec_side1_lane_sums_past_the_partial_count(lsa, shape):
    """The same for k_fr_matvec_rows, whose lanes are 64 apart along a row: a lane pushes a 61st partial only when an unsliced
    row has more than 64 * 240 columns, and rows stay unsliced from 2048 rows on -- a 1 GB matrix, so it is built on the device,
    every entry r - 1, against the closed form cols (r - 1)^2."""
    import torch
    rows, cols = 2048, 64 * shape["dot_max_partials"] * shape["dot_group"] + 1
    assert lsa.fr_matvec_slices(rows, cols, 1) == 1, "retuned: choose rows from which side 1 is unsliced"
    word = torch.from_numpy(filled(1, R - 1).view(np.int64)).to("cuda:0")
    m, w = word.repeat(rows * cols, 1), word.repeat(cols, 1)
    out = lsa.fr_matvec(m, w, rows, cols, side=1)
    lsa.synchronize()
    assert np.array_equal(to_host(out), filled(rows, cols * (R - 1) * (R - 1) * RINV % R))
    assert bool((m == word).all()) and bool((w == word).all()), "an input was modified"


def test_matvec_summed_length_zero_and_empty_outputs(lsa):
    w = rand_fr(5, 3)
    assert np.array_equal(lsa.fr_matvec(w[:0], w[:0], 0, 5, 0), np.zeros((5, 4), dtype=np.uint64))
    assert np.array_equal(lsa.fr_matvec(w[:0], w[:0], 5, 0, 1), np.zeros((5, 4), dtype=np.uint64))
    out = to_dev(w)
    got = lsa.fr_matvec(to_dev(w[:0]), to_dev(w[:0]), 0, 5, 0, out=out)
    lsa.synchronize()
    assert got is out and not to_host(out).any()
    assert lsa.fr_matvec(w[:0], w, 5, 0, 0).shape == (0, 4)
    assert lsa.fr_matvec(w[:0], w, 0, 5, 1).shape == (0, 4)


# ---------------------------------------------------------------------------------------------- guard words
GUARD = 8


def guarded(nout, seed):
    """A device buffer of GUARD + nout + GUARD entries of a fixed pattern, and the view the call may write."""
    whole = to_dev(rand_fr(nout + 2 * GUARD, seed))
    return whole, whole[GUARD:GUARD + nout], whole.clone()


def assert_guards(whole, before, nout):
    import torch
    assert torch.equal(whole[:GUARD], before[:GUARD]) and torch.equal(whole[GUARD + nout:], before[GUARD + nout:]), "a guard entry was written"


def test_matmul_writes_exactly_its_outputs(lsa, shape):
    T, K = shape["matmul_tile"], shape["matmul_kstep"]
    for key in [(1, 1, 1), (T + 1, K + 1, T - 1), (T - 1, 3, 2 * T + 3)]:
        a, b, want = product_case(key)
        whole, view, before = guarded(key[0] * key[2], 11)
        lsa.fr_matmul(to_dev(a), to_dev(b), *key, out=view)
        lsa.synchronize()
        assert np.array_equal(to_host(view), want), key
        assert_guards(whole, before, key[0] * key[2])
        # host mode, straight through the C interface: the library writes the caller's buffer itself
        buf = rand_fr(key[0] * key[2] + 2 * GUARD, 12)
        keep = buf.copy()
        dst = C.c_void_p(buf.ctypes.data + 32 * GUARD)
        assert lsa.lib().lsa_fr_matmul(a.ctypes.data, b.ctypes.data, key[0], key[1], key[2], dst, 0) == 0
        assert np.array_equal(buf[GUARD:-GUARD], want) and np.array_equal(buf[:GUARD], keep[:GUARD]) and np.array_equal(buf[-GUARD:], keep[-GUARD:]), key


def test_matvec_writes_exactly_its_outputs(lsa):
    for key in [(1, 65), (65, 1), (3, 4096), (4096, 3), (63, 65), (257, 129)]:
        m, w, want = sums_case(key)
        for side in (0, 1):
            nout = key[0] if side else key[1]
            whole, view, before = guarded(nout, 13)
            lsa.fr_matvec(to_dev(m), to_dev(w[side]), *key, side, out=view)
            lsa.synchronize()
            assert np.array_equal(to_host(view), want[side]), (key, side)
            assert_guards(whole, before, nout)
            buf = rand_fr(nout + 2 * GUARD, 14)
            keep = buf.copy()
            dst = C.c_void_p(buf.ctypes.data + 32 * GUARD)
            assert lsa.lib().lsa_fr_matvec(m.ctypes.data, key[0], key[1], w[side].ctypes.data, side, dst, 0) == 0
            assert np.array_equal(buf[GUARD:-GUARD], want[side]) and np.array_equal(buf[:GUARD], keep[:GUARD]) and np.array_equal(buf[-GUARD:], keep[-GUARD:]), (key, side)


# ---------------------------------------------------------------------------------------------- error paths
def still_works(lsa):
    a, b, want = product_case((1, 2, 1))
    assert np.array_equal(lsa.fr_matmul(a, b, 1, 2, 1), want)
    assert np.array_equal(run_matmul(lsa, a, b, 1, 2, 1, device=True), want)
    m, w, sums = sums_case((1, 65))
    assert np.array_equal(lsa.fr_matvec(m, w[0], 1, 65, 0), sums[0])
    assert np.array_equal(run_matvec(lsa, m, w[1], 1, 65, 1, device=True), sums[1])


def refused(lsa, rc, *words):
    assert rc != 0
    text = lsa.lib().lsa_last_error().decode()
    assert all(w in text for w in words), text


def test_overlapping_ranges_are_refused(lsa):
    L = lsa.lib()
    n = 8
    for device in (0, 1):
        if device:
            buf = to_dev(rand_fr(4 * n * n, 21))
            keep = buf.clone()
            base = buf.data_ptr()
        else:
            buf = rand_fr(4 * n * n, 21)
            keep = buf.copy()
            base = buf.ctypes.data
        a, b, c_on_a, c_on_b, c_tail_of_b = base, base + 32 * n * n, base + 32 * (n * n - 1), base + 32 * n * n, base + 32 * (2 * n * n - 1)
        for c in (c_on_a, c_on_b, c_tail_of_b):
            refused(lsa, L.lsa_fr_matmul(a, b, n, n, n, c, device), "fr_matmul", "overlaps")
        w = base + 32 * n * n
        for side in (0, 1):
            refused(lsa, L.lsa_fr_matvec(a, n, n, w, side, base + 32 * (n * n - 1), device), "fr_matvec", "overlaps")
            refused(lsa, L.lsa_fr_matvec(a, n, n, w, side, base + 32 * (n * n + n - 1), device), "fr_matvec", "overlaps")
        lsa.synchronize()
        assert (buf == keep).all(), "a refused call wrote something"
        # adjacent ranges are fine
        assert L.lsa_fr_matmul(a, b, n, n, n, base + 32 * 2 * n * n, device) == 0
        assert L.lsa_fr_matvec(a, n, n, w, 0, base + 32 * (n * n + n), device) == 0
        lsa.synchronize()
    still_works(lsa)


def test_null_pointers_overflowing_sizes_and_bad_side_are_refused(lsa):
    L = lsa.lib()
    x = rand_fr(16, 22)
    p = x.ctypes.data
    for device in (0, 1):
        dx = to_dev(x)
        q = dx.data_ptr() if device else p
        for args in [(None, q, 2, 2, 2, q), (q, None, 2, 2, 2, q), (q, q, 2, 2, 2, None)]:
            refused(lsa, L.lsa_fr_matmul(*args, device), "fr_matmul", "null")
        for args in [(None, 2, 2, q, 0, q), (q, 2, 2, None, 1, q), (q, 2, 2, q, 0, None)]:
            refused(lsa, L.lsa_fr_matvec(*args, device), "fr_matvec", "null")
        big = 1 << 62
        for dims in [(big, 4, 1), (1, big, 4), (4, 1, big), (1 << 32, 1, 1 << 32), ((1 << 59) + 1, 1, 1)]:
            refused(lsa, L.lsa_fr_matmul(q, q, *dims, q, device), "fr_matmul", "overflow")
        for dims in [(big, 4), (4, big), (1 << 32, 1 << 32), (1 << 59, 1)]:
            refused(lsa, L.lsa_fr_matvec(q, *dims, q, 0, q, device), "fr_matvec", "overflow")
        for side in (-1, 2):
            refused(lsa, L.lsa_fr_matvec(q, 2, 2, q, side, q, device), "fr_matvec", "side")
    still_works(lsa)


def test_wrappers_check_lengths_and_arguments(lsa):
    a = rand_fr(12, 23)
    for bad in [lambda: lsa.fr_matmul(a, a, 3, 4, 4), lambda: lsa.fr_matmul(a[:11], a, 3, 4, 3), lambda: lsa.fr_matmul(a, a, 3, 4, -3),
                lambda: lsa.fr_matvec(a, a[:4], 3, 4, 0), lambda: lsa.fr_matvec(a, a[:3], 3, 4, 1), lambda: lsa.fr_matvec(a[:11], a[:3], 3, 4, 0),
                lambda: lsa.fr_matvec(a, a[:3], 3, 4, 2), lambda: lsa.fr_matmul(a, to_dev(a), 3, 4, 3),
                lambda: lsa.fr_matmul(to_dev(a), to_dev(a), 3, 4, 3, out=to_dev(a[:8])), lambda: lsa.fr_matvec(to_dev(a), to_dev(a[:3]), 3, 4, 0, out=to_dev(a[:3])),
                lambda: lsa.fr_matvec(a, a[:3], 3, 4, 0, out=a[:4])]:
        with pytest.raises(ValueError):
            bad()
    still_works(lsa)


# ---------------------------------------------------------------------------------------------- the gadget's own shape
@pytest.mark.parametrize("d", [3, 5])
def test_matrix_sumcheck_preprocessing_end_to_end(lsa, d):
    """CPSumcheckMatrix::prove's first steps on device tensors: the table of eq(., rho), DPMatrixMle's contraction of a and of
    b against mle.h:252-258 restated literally, then the first round polynomial without the beta factor; and, separately,
    x^T (A B) y through both sides of fr_matvec."""
    n = 1 << d
    v = rand_fr(2 * n * n + d + 2 * n, 600 + d)
    a, b, rho = v[:n * n], v[n * n:2 * n * n], v[2 * n * n:2 * n * n + d]
    x, y = v[2 * n * n + d:2 * n * n + d + n], v[2 * n * n + d + n:]
    table = lsa.fr_eq_table(rho, variant=0)
    eq_tbl = dec(table)
    d_table = to_dev(table)
    contracted = []
    for mat in (a, b):
        A = dec(mat)
        vtab = [0] * n
        for r in range(n):                       # mle.h:252-258
            for l in range(n):
                p = (l << d) + r
                inc = A[p] * eq_tbl[l] % R
                vtab[r] = (vtab[r] + inc) % R
        d_mat = to_dev(mat)
        got = lsa.fr_matvec(d_mat, d_table, n, n, side=0)
        lsa.synchronize()
        assert np.array_equal(to_host(got), enc(vtab))
        assert np.array_equal(lsa.fr_matvec(mat, table, n, n, side=0), enc(vtab))
        contracted.append((got, vtab))
    h = dec(lsa.sumcheck_round([contracted[0][0], contracted[1][0]]))
    assert len(h) == 3
    assert (2 * h[0] + h[1] + h[2]) % R == sum(p * q for p, q in zip(contracted[0][1], contracted[1][1])) % R      # h(0) + h(1)

    da, db, dx, dy = to_dev(a), to_dev(b), to_dev(x), to_dev(y)      # kept alive until the library's stream is done with them
    c = lsa.fr_matmul(da, db, n, n, n)
    xa = lsa.fr_matvec(da, dx, n, n, side=0)
    by = lsa.fr_matvec(db, dy, n, n, side=1)
    xc = lsa.fr_matvec(c, dx, n, n, side=0)
    lsa.synchronize()
    lhs = sum(p * q for p, q in zip(dec(to_host(xa)), dec(to_host(by)))) % R
    rhs = sum(p * q for p, q in zip(dec(to_host(xc)), dec(y))) % R
    assert lhs == rhs
    A, B, X, Y = dec(a), dec(b), dec(x), dec(y)
    assert lhs == sum(X[r] * A[r * n + k] * B[k * n + c2] * Y[c2] for r in range(n) for k in range(n) for c2 in range(n)) % R
