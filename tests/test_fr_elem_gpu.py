"""GPU suite: element-wise algebra on Fr vectors -- lsa_fr_vec_mul, lsa_fr_vec_lincomb, lsa_fr_powers, lsa_fr_batch_inverse,
lsa_fr_poly_eval (csrc/fr_elem.hip, csrc/fr_elem.h).

Every expected value is Python integers mod r, never the library's.  The words of a value x are X = x 2^256 mod r, so on words a
product is X Y 2^-256, sums stay sums, and ANY 256-bit pattern stands for its value mod r.

Every case runs with host pointers and with device pointers, and where the call has an input vector also in place (out is the
first input).  The shapes follow the kernels' own figures, read from the library (fr_vec_params): lengths around a wavefront,
a workgroup and one trip of the streaming kernels' loop, around the runs of the per-lane kernels and around a workgroup of
fr_poly_eval, and one length whose block partials outnumber what csrc/fr_dot.h adds up before it folds a running sum."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R
RINV = pow(MONT, -1, R)
ALL_ONES = (1 << 256) - 1
EDGE = [0, MONT, R - 1, R, R + 1, ALL_ONES]          # the values 0, 1, (r - 1) / 2^256, and three non-canonical patterns
EDGE_IDS = ["0", "one", "r-1", "r", "r+1", "2^256-1"]
MODES = ("host", "dev", "inplace")
STREAM_LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257]


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


def word(x):
    return unraw([x]).reshape(4)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def run(lsa, mode, f, vecs):
    """f(vectors, out) in one mode; the inputs that are not the output are untouched."""
    if mode == "host":
        keep = [v.copy() for v in vecs]
        got = f(vecs, None)
        assert all(np.array_equal(v, k) for v, k in zip(vecs, keep)), "an input was modified"
        return got
    import torch
    dv = [to_dev(v) for v in vecs]
    keep = [d.clone() for d in dv]
    out = f(dv, dv[0] if mode == "inplace" else None)
    lsa.synchronize()
    if mode == "inplace":
        assert out.data_ptr() == dv[0].data_ptr()
    for i, (d, k) in enumerate(zip(dv, keep)):
        if not (mode == "inplace" and i == 0):
            assert torch.equal(d, k), "an input was modified"
    return to_host(out)


# ---- the expected words, on integers
def exp_mul(A, B, S=MONT):
    return [a * b * S * RINV * RINV % R for a, b in zip(A, B)]


def exp_lin(Xs, Cs):
    return [sum(c * x[i] for c, x in zip(Cs, Xs)) * RINV % R for i in range(len(Xs[0]))]


def exp_pow(B, n, F=MONT):
    b, cur, out = B * RINV % R, F % R, []
    for _ in range(n):
        out.append(cur)
        cur = cur * b % R
    return out


def exp_inv(X):
    return [0 if x % R == 0 else MONT * MONT * pow(x, -1, R) % R for x in X]


def exp_eval(Cs, X):
    xv, acc = X * RINV % R, 0
    for c in reversed(Cs):
        acc = (acc * xv + c) % R
    return acc


def same(got, want_ints):
    return np.array_equal(np.asarray(got).reshape(-1, 4), unraw(want_ints).reshape(-1, 4))


def sample_idx(n):
    return sorted(set(range(0, n, 4099)) | set(range(max(0, n - 600), n)))


@pytest.fixture(scope="module")
def P(lsa):
    p = lsa.fr_vec_params()
    p.update(lsa.fr_matrix_params())
    assert p["pass_elems"] > 0 and p["lincomb_max"] == 8
    return p


@pytest.fixture(scope="module")
def big(lsa, P):
    """Two vectors of pass_elems + 257 elements (a second, ragged trip of the grid-stride loop) and the sampled integers."""
    n = P["pass_elems"] + 257
    x, y = rand_fr(n, 901), rand_fr(n, 902)
    idx = sample_idx(n) if n > (1 << 20) else list(range(n))
    for k, w in enumerate(EDGE):                         # edge words where the comparison looks
        x[idx[3 + k]] = word(w)
        y[idx[-5 - k]] = word(w)
    ii = np.array(idx)
    return {"n": n, "x": x, "y": y, "idx": ii, "X": raw(x[ii]), "Y": raw(y[ii])}


# ---------------------------------------------------------------------------------------------- vec_mul
@pytest.mark.parametrize("mode", MODES)
def test_vec_mul_lengths(lsa, mode):
    s = rand_fr(1, 5)[0]
    for n in STREAM_LENGTHS:
        a, b = rand_fr(n, 10 + n), rand_fr(n, 20 + n)
        got = run(lsa, mode, lambda v, o: lsa.fr_vec_mul(v[0], v[1], scale=s, out=o), [a, b])
        assert same(got, exp_mul(raw(a), raw(b), raw(s)[0])), n
        got = run(lsa, mode, lambda v, o: lsa.fr_vec_mul(v[0], v[1], out=o), [a, b])
        assert same(got, exp_mul(raw(a), raw(b))), n


@pytest.mark.parametrize("mode", MODES)
def test_vec_mul_second_trip_of_the_loop(lsa, mode, big):
    got = run(lsa, mode, lambda v, o: lsa.fr_vec_mul(v[0], v[1], out=o), [big["x"], big["y"]])
    assert len(got) == big["n"]
    assert same(got[big["idx"]], exp_mul(big["X"], big["Y"]))


@pytest.mark.parametrize("mode", MODES)
def test_vec_mul_edge_operands(lsa, mode):
    n = 65
    fills = [rand_fr(n, 33)] + [filled(n, w) for w in EDGE]
    scales = [None] + EDGE
    for i, a in enumerate(fills):
        for j, b in enumerate(fills):
            sw = scales[(i + j) % len(scales)]
            got = run(lsa, mode, lambda v, o: lsa.fr_vec_mul(v[0], v[1], scale=None if sw is None else word(sw), out=o), [a, b])
            assert same(got, exp_mul(raw(a), raw(b), MONT if sw is None else sw)), (i, j)
    a = fills[0]
    for sw in EDGE:                                      # every edge word as the scale of random data
        got = run(lsa, mode, lambda v, o: lsa.fr_vec_mul(v[0], v[1], scale=word(sw), out=o), [a, fills[0][::-1].copy()])
        assert same(got, exp_mul(raw(a), raw(a)[::-1], sw)), sw
    # squares: the same vector twice
    got = run(lsa, mode, lambda v, o: lsa.fr_vec_mul(v[0], v[0], out=o), [a])
    assert same(got, exp_mul(raw(a), raw(a)))
    # scale NULL against the scale one; the scale zero (also spelled r)
    one = run(lsa, mode, lambda v, o: lsa.fr_vec_mul(v[0], v[1], scale=word(MONT), out=o), [a, fills[3]])
    none = run(lsa, mode, lambda v, o: lsa.fr_vec_mul(v[0], v[1], out=o), [a, fills[3]])
    assert np.array_equal(one, none)
    for z in (0, R):
        got = run(lsa, mode, lambda v, o: lsa.fr_vec_mul(v[0], v[1], scale=word(z), out=o), [a, fills[3]])
        assert not got.any()


# ---------------------------------------------------------------------------------------------- lincomb
@pytest.mark.parametrize("mode", MODES)
def test_lincomb_lengths(lsa, mode):
    c = rand_fr(2, 6)
    for n in STREAM_LENGTHS:
        x, y = rand_fr(n, 30 + n), rand_fr(n, 40 + n)
        got = run(lsa, mode, lambda v, o: lsa.fr_vec_lincomb(v, c, out=o), [x, y])
        assert same(got, exp_lin([raw(x), raw(y)], raw(c))), n


@pytest.mark.parametrize("k", [1, 3, 5])                 # one k per unroll of the kernel (4, 2, 1 elements per lane and trip)
@pytest.mark.parametrize("mode", MODES)
def test_lincomb_second_trip_of_the_loop(lsa, mode, k, big):
    c = rand_fr(k, 60 + k)
    got = run(lsa, mode, lambda v, o: lsa.fr_vec_lincomb([v[t % 2] for t in range(k)], c, out=o), [big["x"], big["y"]])
    assert len(got) == big["n"]
    assert same(got[big["idx"]], exp_lin([(big["X"], big["Y"])[t % 2] for t in range(k)], raw(c)))


@pytest.mark.parametrize("mode", MODES)
def test_lincomb_vector_counts_and_widest_accumulator(lsa, mode, P):
    n = 257
    ks = sorted({1, 2, P["dot_group"], P["dot_group"] + 1, P["lincomb_max"]})
    for k in ks:
        xs = [rand_fr(n, 70 + 10 * k + t) for t in range(k)]
        for t in range(k):                               # edge words among the data and the coefficients
            xs[t][(7 * t) % n] = word(EDGE[t % len(EDGE)])
        c = rand_fr(k, 80 + k)
        c[k - 1] = word(EDGE[(k + 2) % len(EDGE)])
        got = run(lsa, mode, lambda v, o: lsa.fr_vec_lincomb(v, c, out=o), xs)
        assert same(got, exp_lin([raw(x) for x in xs], raw(c))), k
        for w in (R - 1, ALL_ONES, R + 1):               # everything at the top: the widest accumulator
            xs = [filled(n, w) for _ in range(k)]
            got = run(lsa, mode, lambda v, o: lsa.fr_vec_lincomb(v, filled(k, w), out=o), xs)
            assert same(got, exp_lin([[w] * n] * k, [w] * k)), (k, w)
        # the same vector k times
        x = rand_fr(n, 90 + k)
        got = run(lsa, mode, lambda v, o: lsa.fr_vec_lincomb([v[0]] * k, c, out=o), [x])
        assert same(got, exp_lin([raw(x)] * k, raw(c))), k
    # coefficients (1, r - 1): the difference
    x, y = rand_fr(n, 95), rand_fr(n, 96)
    y[5] = x[5]
    got = run(lsa, mode, lambda v, o: lsa.fr_vec_lincomb(v, unraw([MONT, R - MONT]), out=o), [x, y])
    assert same(got, [(a - b) % R for a, b in zip(raw(x), raw(y))])


def test_lincomb_refuses_no_vectors_and_too_many(lsa, P):
    x = rand_fr(4, 1)
    with pytest.raises(lsa.LsaError):
        lsa.fr_vec_lincomb([], np.zeros((0, 4), dtype=np.uint64))
    k = P["lincomb_max"] + 1
    with pytest.raises(lsa.LsaError):
        lsa.fr_vec_lincomb([x] * k, rand_fr(k, 2))
    with pytest.raises(lsa.LsaError):
        lsa.fr_vec_lincomb([to_dev(x)] * k, rand_fr(k, 2))
    assert same(lsa.fr_vec_lincomb([x], unraw([MONT])), raw(x))          # still usable


# ---------------------------------------------------------------------------------------------- powers
def powers_both_modes(lsa, base, n, first=None):
    import torch
    host = lsa.fr_powers(base, n, first=first)
    out = torch.full((n + 1, 4), -1, dtype=torch.int64, device="cuda:0")
    res = lsa.fr_powers(base, n, first=first, out=out[:n])
    lsa.synchronize()
    got = to_host(res)
    assert np.array_equal(got, host), "host and device mode differ"
    assert (to_host(out[n:]) == np.uint64(ALL_ONES & ((1 << 64) - 1))).all(), "written past n"
    return host


def test_powers(lsa, P):
    run_len = P["powers_run"]
    root = pow(5, (R - 1) >> 4, R)                        # a primitive 16th root of unity
    assert pow(root, 16, R) == 1 and pow(root, 8, R) != 1
    bases = [raw(rand_fr(1, 7))[0], 0, R, MONT, R - 1, R - MONT, root * MONT % R, ALL_ONES]
    ns = sorted({0, 1, 2, run_len - 1, run_len, run_len + 1, 256 * run_len - 1, 256 * run_len, 256 * run_len + 1})
    f = raw(rand_fr(1, 8))[0]
    for B in bases:
        for n in ns:
            assert same(powers_both_modes(lsa, word(B), n), exp_pow(B, n)), (B, n)
        n = 3 * run_len + 5
        for F in (f, 0, R + 1, ALL_ONES):
            assert same(powers_both_modes(lsa, word(B), n, first=word(F)), exp_pow(B, n, F)), (B, F)
        assert np.array_equal(lsa.fr_powers(word(B), n), lsa.fr_powers(word(B), n, first=word(MONT)))
    # base 0: first, 0, 0, ...; 0^0 = 1
    assert same(lsa.fr_powers(word(0), 4), [MONT, 0, 0, 0])
    assert same(lsa.fr_powers(word(0), 4, first=word(f)), [f, 0, 0, 0])
    # the root's powers come round
    w = raw(lsa.fr_powers(word(root * MONT % R), 33))
    assert w[16] == MONT and w[32] == MONT and w[8] == R - MONT


def test_powers_long_vector_in_full(lsa):
    n = (1 << 16) + 3
    B, F = raw(rand_fr(2, 9))
    assert same(powers_both_modes(lsa, word(B), n, first=word(F)), exp_pow(B, n, F))
    # against Python's pow, entry by entry
    b = B * RINV % R
    got = raw(lsa.fr_powers(word(B), n))
    assert all(got[i] == pow(b, i, R) * MONT % R for i in range(0, n, 97)) and got[n - 1] == pow(b, n - 1, R) * MONT % R


# ---------------------------------------------------------------------------------------------- batch inverse
def check_inverse(lsa, x, mode):
    cnt = []

    def f(v, o):
        res, nz = lsa.fr_batch_inverse(v[0], out=o, count_zeros=True)
        cnt.append(nz)
        return res
    got = run(lsa, mode, f, [x])
    X = raw(x)
    assert cnt == [sum(1 for v in X if v % R == 0)]
    assert same(got, exp_inv(X))
    G = raw(got)
    assert all((g * RINV) * (v * RINV) % R == 1 for g, v in zip(G, X) if v % R) and all(g < R for g in G)
    # without the count the call gives the same bytes
    assert np.array_equal(run(lsa, mode, lambda v, o: lsa.fr_batch_inverse(v[0], out=o), [x]), got)


@pytest.mark.parametrize("mode", MODES)
def test_batch_inverse(lsa, mode, P):
    run_len = P["inv_run"]
    ns = sorted({0, 1, run_len - 1, run_len, run_len + 1, 64 * run_len + 1, 256 * run_len - 1, 256 * run_len, 256 * run_len + 1})
    for n in ns:
        check_inverse(lsa, rand_fr(n, 100 + n), mode)                      # no zero
    n = 3 * run_len + 5
    for zero in (0, R, 2 * R):
        x = rand_fr(n, 200)
        x[run_len] = word(zero)                                            # the first and the last slot of a run
        x[2 * run_len - 1] = word(zero)
        check_inverse(lsa, x, mode)
        x = rand_fr(n, 201)
        x[run_len:2 * run_len] = word(zero)                                # a whole run
        x[n - 1] = word(zero)                                              # and the last element of the short run
        check_inverse(lsa, x, mode)
        check_inverse(lsa, filled(n, zero), mode)                          # nothing but zeros
    x = rand_fr(n, 202)
    for i, w in enumerate(EDGE):                                           # every edge word, zeros and non-zeros
        x[2 * i] = word(w)
    check_inverse(lsa, x, mode)


# ---------------------------------------------------------------------------------------------- poly_eval
def eval_both_modes(lsa, c, xw):
    host = lsa.fr_poly_eval(c, word(xw))
    dc = to_dev(c)
    keep = dc.clone()
    out = lsa.fr_poly_eval(dc, word(xw))
    lsa.synchronize()
    import torch
    assert torch.equal(dc, keep)
    assert np.array_equal(to_host(out), host), "host and device mode differ"
    return host


def test_poly_eval(lsa, P):
    items, block = P["eval_items"], P["eval_block"]
    xr = raw(rand_fr(1, 11))[0]
    ns = sorted({0, 1, 2, items - 1, items, items + 1, block - 1, block, block + 1, 3 * block + 7})
    for n in ns:
        c = rand_fr(n, 300 + n)
        for xw in (xr, 0, MONT, R - MONT, R - 1, R + 1, ALL_ONES):
            assert same(eval_both_modes(lsa, c, xw), [exp_eval(raw(c), xw)]), (n, xw)
    n = block + items + 1
    for w in (R - 1, ALL_ONES, 0):
        assert same(eval_both_modes(lsa, filled(n, w), xr), [exp_eval([w] * n, xr)]), w
        assert same(eval_both_modes(lsa, filled(n, w), R - MONT), [exp_eval([w] * n, R - MONT)]), w


def test_poly_eval_more_block_partials_than_a_running_sum_holds(lsa, P):
    n = (P["dot_max_partials"] + 1) * P["eval_block"] + 3
    c = rand_fr(n, 12)
    c[n - 1] = word(ALL_ONES)
    for xw in (raw(rand_fr(1, 13))[0], R - MONT):
        assert same(eval_both_modes(lsa, c, xw), [exp_eval(raw(c), xw)])
    assert same(eval_both_modes(lsa, filled(n, R - 1), MONT), [(R - 1) * n % R])


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_are_argument_checks(lsa):
    """Every refusal happens before any device work (LsaError from the argument checks); the library works afterwards."""
    import torch
    L = lsa.lib()
    n = 8
    a, b = rand_fr(n, 1), rand_fr(n, 2)
    out = np.zeros((n, 4), dtype=np.uint64)
    one = word(MONT)
    hp = lambda v: v.ctypes.data_as(C.c_void_p)
    da, db = to_dev(a), to_dev(b)
    dout = torch.zeros((n + 1, 4), dtype=torch.int64, device="cuda:0")
    dp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    xs_h = (C.c_void_p * 2)(a.ctypes.data, b.ctypes.data)
    xs_d = (C.c_void_p * 2)(da.data_ptr(), db.data_ptr())
    xs_null = (C.c_void_p * 2)(a.ctypes.data, None)
    coef = rand_fr(2, 3)
    nz = C.c_uint64(0)
    huge = 1 << 59                                      # * 32 bytes wraps size_t
    refused = [
        # null with n > 0
        lambda: L.lsa_fr_vec_mul(None, hp(b), None, n, hp(out), 0),
        lambda: L.lsa_fr_vec_mul(hp(a), hp(b), None, n, None, 0),
        lambda: L.lsa_fr_vec_lincomb(xs_null, hp(coef), 2, n, hp(out), 0),
        lambda: L.lsa_fr_vec_lincomb(xs_h, None, 2, n, hp(out), 0),
        lambda: L.lsa_fr_vec_lincomb(None, hp(coef), 2, n, hp(out), 0),
        lambda: L.lsa_fr_powers(None, None, n, hp(out), 0),
        lambda: L.lsa_fr_powers(hp(one), None, n, None, 0),
        lambda: L.lsa_fr_batch_inverse(None, n, hp(out), None, 0),
        lambda: L.lsa_fr_batch_inverse(dp(da), n, None, None, 1),
        lambda: L.lsa_fr_poly_eval(None, n, hp(one), hp(out), 0),
        lambda: L.lsa_fr_poly_eval(hp(a), n, None, hp(out), 0),
        lambda: L.lsa_fr_poly_eval(hp(a), n, hp(one), None, 0),
        # partial overlap: out = a + 1 element
        lambda: L.lsa_fr_vec_mul(hp(a), hp(b), None, n - 1, C.c_void_p(a.ctypes.data + 32), 0),
        lambda: L.lsa_fr_vec_mul(dp(da), dp(db), None, n - 1, dp(da, 32), 1),
        lambda: L.lsa_fr_vec_mul(dp(db), dp(da), None, n - 1, dp(da, 32), 1),
        lambda: L.lsa_fr_vec_lincomb(xs_d, hp(coef), 2, n - 1, dp(db, 32), 1),
        lambda: L.lsa_fr_batch_inverse(dp(da), n - 1, dp(da, 32), None, 1),
        lambda: L.lsa_fr_poly_eval(dp(da), n, hp(one), dp(da, 64), 1),
        lambda: L.lsa_fr_poly_eval(dp(da), n, hp(one), dp(da), 1),           # (no in-place here)
        # a device pointer offset by 8 bytes
        lambda: L.lsa_fr_vec_mul(dp(da, 8), dp(db), None, n - 1, dp(dout), 1),
        lambda: L.lsa_fr_vec_mul(dp(da), dp(db), None, n, dp(dout, 8), 1),
        lambda: L.lsa_fr_vec_lincomb((C.c_void_p * 2)(da.data_ptr(), db.data_ptr() + 8), hp(coef), 2, n - 1, dp(dout), 1),
        lambda: L.lsa_fr_powers(hp(one), None, n, dp(dout, 8), 1),
        lambda: L.lsa_fr_batch_inverse(dp(da, 8), n - 1, dp(dout), None, 1),
        lambda: L.lsa_fr_poly_eval(dp(da, 8), n - 1, hp(one), dp(dout), 1),
        lambda: L.lsa_fr_poly_eval(dp(da), n, hp(one), dp(dout, 8), 1),
        # n * 32 does not fit size_t
        lambda: L.lsa_fr_vec_mul(dp(da), dp(db), None, huge, dp(dout), 1),
        lambda: L.lsa_fr_vec_mul(hp(a), hp(b), None, huge, hp(out), 0),
        lambda: L.lsa_fr_vec_lincomb(xs_d, hp(coef), 2, huge, dp(dout), 1),
        lambda: L.lsa_fr_powers(hp(one), None, huge, dp(dout), 1),
        lambda: L.lsa_fr_batch_inverse(dp(da), huge, dp(dout), C.byref(nz), 1),
        lambda: L.lsa_fr_poly_eval(dp(da), huge, hp(one), dp(dout), 1),
        lambda: L.lsa_fr_poly_eval(dp(da), (1 << 64) - 1, hp(one), dp(dout), 1),
    ]
    for i, call in enumerate(refused):
        rc = call()
        assert rc != 0, i
        with pytest.raises(lsa.LsaError):
            lsa._check(rc)
    lsa.synchronize()
    assert torch.equal(da, to_dev(a)) and torch.equal(db, to_dev(b)) and not dout.any() and not out.any()
    # n == 0: fine with null vectors, and nothing is written
    assert L.lsa_fr_vec_mul(None, None, None, 0, None, 1) == 0
    assert L.lsa_fr_vec_lincomb(None, None, 1, 0, None, 1) == 0
    assert L.lsa_fr_powers(None, None, 0, None, 0) == 0
    assert L.lsa_fr_batch_inverse(None, 0, None, C.byref(nz), 1) == 0 and nz.value == 0
    # exact aliasing is legal; the library is still usable
    prod = lsa.fr_vec_mul(da, db)
    lsa.synchronize()
    assert same(to_host(prod), exp_mul(raw(a), raw(b)))


# ---------------------------------------------------------------------------------------------- chains, no synchronise in between
@pytest.mark.parametrize("key", [(1, None), (1, 0)], ids=str)
def test_chain_lipmaa_keygen_scalars_stay_on_the_device(lsa, key):
    """fr_lagrange -> fr_vec_lincomb([row], [gamma]) -> batch_exp(g2), and fr_powers(chi, m + 1) -> batch_exp(g1), queued without a
    synchronise: the points are those from scalars built with Python integers on the host."""
    import torch
    import oracle_lib as o
    big_log, small_log = key
    m = (1 << big_log) + (0 if small_log is None else 1 << small_log)
    w = o.fr_mont(o.fr_root_of_unity(big_log if small_log is None else big_log + 1))
    chi, gamma = dec(rand_fr(2, 2024 + m))
    g1, g2 = o.generator("g1"), o.generator("g2")
    row = torch.empty((m, 4), dtype=torch.int64, device="cuda:0")
    lsa.fr_lagrange(big_log, small_log, w, o.fr_mont(chi), out=row)
    d_g2 = lsa.batch_exp("g2", g2, lsa.fr_vec_lincomb([row], enc([gamma])))
    d_pows = torch.empty((m + 1, 4), dtype=torch.int64, device="cuda:0")
    d_g1 = lsa.batch_exp("g1", g1, lsa.fr_powers(o.fr_mont(chi), m + 1, out=d_pows))
    lsa.synchronize()
    Li = dec(lsa.fr_lagrange(big_log, small_log, w, o.fr_mont(chi)))
    want_g2 = lsa.batch_exp("g2", g2, enc([gamma * x % R for x in Li]))
    want_g1 = lsa.batch_exp("g1", g1, enc([pow(chi, i, R) for i in range(m + 1)]))
    assert np.array_equal(lsa.normalize("g2", to_host(d_g2)), lsa.normalize("g2", want_g2))
    assert np.array_equal(lsa.normalize("g1", to_host(d_g1)), lsa.normalize("g1", want_g1))


def test_chain_groth16_key_scalars(lsa):
    """Three FrSparse.matvec(side=0) -> fr_vec_lincomb([At, Bt, Ct], [beta / delta, alpha / delta, 1 / delta]) on a 5 x 7 R1CS with
    +-1 and random coefficients, against Python integers."""
    rows, cols = 5, 7
    rng = np.random.default_rng(77)
    alpha, beta, delta = dec(rand_fr(3, 78))
    u = rand_fr(rows, 79)                                 # the Lagrange row at the toxic point
    U = dec(u)
    mats, dense = [], []
    for s in range(3):
        vals, cidx, ptr, D = [], [], [0], [[0] * cols for _ in range(rows)]
        for r in range(rows):
            for c in sorted(rng.choice(cols, size=int(rng.integers(1, 5)), replace=False)):
                kind = int(rng.integers(0, 3))
                v = 1 if kind == 0 else (R - 1 if kind == 1 else dec(rand_fr(1, 1000 * s + 10 * r + int(c)))[0])
                vals.append(v)
                cidx.append(int(c))
                D[r][int(c)] = v
            ptr.append(len(vals))
        mats.append(lsa.FrSparse(enc(vals), np.array(cidx, dtype=np.uint32), np.array(ptr, dtype=np.uint64), cols))
        dense.append(D)
    du = to_dev(u)
    t = [M.matvec(du, side=0) for M in mats]
    dinv = pow(delta, -1, R)
    got = lsa.fr_vec_lincomb(t, enc([beta * dinv, alpha * dinv, dinv]))
    lsa.synchronize()
    T = [[sum(U[r] * D[r][c] for r in range(rows)) % R for c in range(cols)] for D in dense]
    want = [(beta * T[0][c] + alpha * T[1][c] + T[2][c]) * dinv % R for c in range(cols)]
    assert dec(to_host(got)) == want
    for M in mats:
        M.close()


@pytest.mark.parametrize("key", [(5, None), (5, 2)], ids=str)
def test_chain_quotient_checked_on_the_device(lsa, key):
    """c = fr_vec_mul(a, b); H = fr_hadamard_quotient(a, b, c, 0); then H(x) Z(x) = A(x) B(x) - C(x) with H(x) = fr_poly_eval(H, x) and
    A(x) = fr_matvec(a, 1, m, fr_lagrange(x), side 1) -- every vector stays on the device and nothing waits in between.  With one
    entry of c changed the identity fails."""
    import torch
    import oracle_lib as o
    big_log, small_log = key
    big, small = 1 << big_log, (0 if small_log is None else 1 << small_log)
    m = big + small
    w_int = o.fr_root_of_unity(big_log if small_log is None else big_log + 1)
    w = o.fr_mont(w_int)
    x = dec(rand_fr(1, 555 + m))[0]
    Zx = (pow(x, m, R) - 1) % R if small_log is None else (pow(x, big, R) - 1) * (pow(x, small, R) - pow(w_int, small, R)) % R
    da, db = to_dev(rand_fr(m, 556)), to_dev(rand_fr(m, 557))
    zero3 = np.zeros((3, 4), dtype=np.uint64)

    def sides(tamper):
        dc = lsa.fr_vec_mul(da, db)
        if tamper:
            lsa.synchronize()                             # (torch's stream is not ordered behind the library's: wait, then edit)
            dc[m // 2, 0] += 1                            # (the wrappers order the library's stream behind torch's)
        dh = lsa.fr_hadamard_quotient(da, db, dc, zero3, big_log, small_log, omega=w, coset=o.fr_mont(o.FR_GENERATOR))
        hx = lsa.fr_poly_eval(dh, o.fr_mont(x))
        row = torch.empty((m, 4), dtype=torch.int64, device="cuda:0")
        lsa.fr_lagrange(big_log, small_log, w, o.fr_mont(x), out=row)
        vals = [lsa.fr_matvec(v, row, 1, m, side=1) for v in (da, db, dc)]
        lsa.synchronize()
        Hx, Ax, Bx, Cx = (dec(to_host(v))[0] for v in [hx] + vals)
        return Hx * Zx % R, (Ax * Bx - Cx) % R

    lhs, rhs = sides(False)
    assert lhs == rhs
    lhs, rhs = sides(True)
    assert lhs != rhs


# ---------------------------------------------------------------------------------------------- randomised
def rand_words(rng, n):
    v = rand_fr(n, int(rng.integers(0, 1 << 62)))
    for i in np.nonzero(rng.random(n) < 0.05)[0]:
        v[i] = word(EDGE[int(rng.integers(0, len(EDGE)))])
    return v


def rand_scalar(rng):
    return rand_words(rng, 1)[0] if rng.random() < 0.8 else word(EDGE[int(rng.integers(0, len(EDGE)))])


@pytest.mark.parametrize("seed", [20260101, 20260102, 20260103])
def test_randomised(lsa, seed, P):
    rng = np.random.default_rng(seed)
    length = lambda: int(math.exp(rng.uniform(0, math.log(5001)))) - 1
    for case in range(40):
        mode = MODES[int(rng.integers(0, 3))]
        n = length()
        a, b = rand_words(rng, n), rand_words(rng, n)
        s = rand_scalar(rng) if rng.random() < 0.7 else None
        got = run(lsa, mode, lambda v, o: lsa.fr_vec_mul(v[0], v[1], scale=s, out=o), [a, b])
        assert same(got, exp_mul(raw(a), raw(b), MONT if s is None else raw(s)[0])), ("vec_mul", case, n, mode)
    for case in range(40):
        mode = MODES[int(rng.integers(0, 3))]
        n, k = length(), int(rng.integers(1, P["lincomb_max"] + 1))
        xs = [rand_words(rng, n) for _ in range(k)]
        c = np.stack([rand_scalar(rng) for _ in range(k)])
        got = run(lsa, mode, lambda v, o: lsa.fr_vec_lincomb(v, c, out=o), xs)
        assert same(got, exp_lin([raw(x) for x in xs], raw(c))), ("lincomb", case, n, k, mode)
    for case in range(40):
        n = length()
        B = raw(rand_scalar(rng))[0]
        F = raw(rand_scalar(rng))[0] if rng.random() < 0.5 else None
        got = powers_both_modes(lsa, word(B), n, first=None if F is None else word(F))
        assert same(got, exp_pow(B, n, MONT if F is None else F)), ("powers", case, n)
    for case in range(40):
        mode = MODES[int(rng.integers(0, 3))]
        check_inverse(lsa, rand_words(rng, length()), mode)
    for case in range(40):
        c = rand_words(rng, length())
        xw = raw(rand_scalar(rng))[0]
        assert same(eval_both_modes(lsa, c, xw), [exp_eval(raw(c), xw)]), ("poly_eval", case, len(c))
