"""GPU suite: the Lipmaa Hadamard prover on resident vectors -- lsa_fr_hadamard_quotient (CPHadL::prove's
coefficients_for_H) and lsa_fr_lagrange (evaluate_all_lagrange_polynomials), over the basic radix-2 domain and libfqfft's
step radix-2 domain (csrc/fr_poly.hip, csrc/fr_batch_inv.h).

The expected quotient follows the reference's schedule (src/gadgets/lipmaa.cc:103-176): the seven transforms are the
oracle's, everything between them (the pointwise steps, the values of 1 / Z on the coset, add_poly_Z) is Python integers
mod r.  Sizes: one-, two- and three-pass transforms, small = 1 and small = big / 2, and vectors that end inside, at and one
past a run of the batch inversion (16 elements: m = 2, 3, 6, 9, 32, 36, ...; the step domain's table of 1 / Z has 2 .. 256
entries).
"""
import numpy as np
import pytest

import oracle_lib as o

pytestmark = pytest.mark.gpu

R = o.R
RINV = pow(o.MONT, -1, R)
G = o.FR_GENERATOR
BASIC = [1, 2, 5, 10, 11, 16, 17]
STEP = [(1, 0), (2, 1), (3, 0), (5, 2), (10, 9), (11, 3), (17, 16)]
DOMAINS = [(b, None) for b in BASIC] + STEP
SMALL_DOMAINS = [d for d in DOMAINS if d[0] <= 11]            # the Python side of a check is O(m) big-integer work
MID = [(5, None), (11, None), (5, 2), (11, 3)]


def dec(arr):
    """(n, 4) uint64 Montgomery limbs -> Python ints."""
    arr = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)
    b = arr.tobytes()
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") * RINV % R for i in range(len(arr))]


def enc(xs):
    return np.frombuffer(b"".join((x % R * o.MONT % R).to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


def rand_fr(n, seed):
    """n canonical residues (below 2^252) as limbs: any canonical residue is some value's Montgomery form."""
    a = np.random.default_rng(seed).integers(0, 1 << 64, (n, 4), dtype=np.uint64, endpoint=False)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


class Dom:
    def __init__(self, big_log, small_log=None):
        self.big_log, self.small_log = big_log, small_log
        self.big = 1 << big_log
        self.small = 0 if small_log is None else 1 << small_log
        self.m = self.big + self.small
        self.w_int = o.fr_root_of_unity(big_log if small_log is None else big_log + 1)
        self.w = o.fr_mont(self.w_int)
        self.c = pow(self.w_int, self.small, R)               # omega^small (step domain)
        self._pts = None

    def point(self, i):
        if self.small_log is None:
            return pow(self.w_int, i, R)
        if i < self.big:
            return pow(self.w_int, 2 * i, R)
        return self.w_int * pow(self.w_int, (2 * self.big // self.small) * (i - self.big), R) % R

    def points(self):
        if self._pts is None:
            if self.small_log is None:
                self._pts = [pow(self.w_int, i, R) for i in range(self.m)]
            else:
                sigma = pow(self.w_int, 2 * self.big // self.small, R)
                self._pts = [pow(self.w_int, 2 * i, R) for i in range(self.big)] + [self.w_int * pow(sigma, j, R) % R for j in range(self.small)]
        return self._pts

    def transform(self, a, inverse=False, coset=None):
        cg = o.fr_mont(coset) if coset is not None else None
        if self.small_log is None:
            return o.fr_domain_transform(a, self.w, inverse=inverse, coset=cg)
        return o.fr_step_domain_transform(a, self.big_log, self.small_log, self.w, inverse=inverse, coset=cg)

    def Z(self, x):
        if self.small_log is None:
            return (pow(x, self.m, R) - 1) % R
        return (pow(x, self.big, R) - 1) * (pow(x, self.small, R) - self.c) % R

    def zinv_on_coset(self, g):
        """1 / Z(g x_i) for every point: one value on the basic domain; on the step domain big / small distinct values on
        the big part (x^small has that period there) and one on the small part -- each by direct evaluation of Z."""
        if self.small_log is None:
            return [pow(self.Z(g), -1, R)] * self.m
        period = self.big // self.small
        tab = [pow(self.Z(g * self.point(k) % R), -1, R) for k in range(period)]
        z1 = pow(self.Z(g * self.point(self.big) % R), -1, R)
        return [tab[i % period] for i in range(self.big)] + [z1] * self.small

    def add_poly_Z(self, k, H):
        if self.small_log is None:
            H[self.m] = (H[self.m] + k) % R
            H[0] = (H[0] - k) % R
        else:
            H[self.m] = (H[self.m] + k) % R
            H[self.big] = (H[self.big] - k * self.c) % R
            H[self.small] = (H[self.small] - k) % R
            H[0] = (H[0] + k * self.c) % R

    def pad(self, a):
        out = np.zeros((self.m, 4), dtype=np.uint64)
        out[:len(a)] = a
        return out


_doms = {}


def dom(key):
    if key not in _doms:
        _doms[key] = Dom(*key)
    return _doms[key]


def raw(arr):
    """(n, 4) uint64 limbs -> the integers they spell (x 2^256 mod r for the value x): sums, differences and products with
    a plain integer stay in that form; a product of two such integers needs one factor 2^-256."""
    b = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def unraw(xs):
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


def expected_h(D, a, b, c, d, g=G):
    """coefficients_for_H as lipmaa.cc:103-176 computes it (with b where the reference reads a second copy of a)."""
    d1, d2, d3 = d
    A, B, C = (D.transform(D.pad(x), inverse=True) for x in (a, b, c))
    H = [(d2 * x + d1 * y) % R for x, y in zip(raw(A), raw(B))] + [0]
    corr = [0] * (D.m + 1)
    corr[0] = -d3 % R
    D.add_poly_Z(d1 * d2 % R, corr)
    Ac, Bc, Cc = (raw(D.transform(x, coset=g)) for x in (A, B, C))
    zi = D.zinv_on_coset(g)
    q = [(x * y * RINV - z) * w % R for x, y, z, w in zip(Ac, Bc, Cc, zi)]
    Hq = raw(D.transform(unraw(q), inverse=True, coset=g))
    for i in range(D.m):
        H[i] = (H[i] + Hq[i]) % R
    for i in {0, D.small, D.big, D.m}:
        H[i] = (H[i] + corr[i] * o.MONT) % R
    return unraw(H)


_cases = {}


def case(key, n=None):
    """Random a, b, c (n values), d1..d3 and the expected H of a domain: computed once, shared, never modified."""
    D = dom(key)
    n = D.m if n is None else n
    if (key, n) not in _cases:
        seed = 1000 * key[0] + (0 if key[1] is None else 31 * key[1] + 7) + 100000 * (n != D.m) + n % 97
        v = rand_fr(3 * n, seed)
        a, b, c = v[:n].copy(), v[n:2 * n].copy(), v[2 * n:].copy()
        d = dec(rand_fr(3, seed + 1))
        want = expected_h(D, a, b, c, d)
        for x in (a, b, c, want):
            x.setflags(write=False)
        _cases[(key, n)] = (a, b, c, d, want)
    return _cases[(key, n)]


def quotient(lsa, key, a, b, c, d, device=False, coset=G):
    D = dom(key)
    if not device:
        return lsa.fr_hadamard_quotient(a, b, c, enc(d), D.big_log, D.small_log, omega=D.w, coset=o.fr_mont(coset))
    import torch
    t = [torch.from_numpy(np.array(x).view(np.int64)).to("cuda:0") for x in (a, b, c)]
    keep = [x.clone() for x in t]
    h = lsa.fr_hadamard_quotient(t[0], t[1], t[2], enc(d), D.big_log, D.small_log, omega=D.w, coset=o.fr_mont(coset))
    lsa.synchronize()
    for x, k in zip(t, keep):
        assert torch.equal(x, k), "an input was modified"
    return h.cpu().numpy().view(np.uint64)


def horner(coeffs, x):
    acc = 0
    for cf in reversed(coeffs):
        acc = (acc * x + cf) % R
    return acc


def lagrange_products(pts, t):
    """L_i(t) = prod_(j != i) (t - x_j) / (x_i - x_j): the definition, O(m^2)."""
    out = []
    for i, xi in enumerate(pts):
        num = den = 1
        for j, xj in enumerate(pts):
            if j != i:
                num = num * (t - xj) % R
                den = den * (xi - xj) % R
        out.append(num * pow(den, -1, R) % R)
    return out


def lagrange_basic(n, w, t):
    """libfqfft _basic_radix2_evaluate_all_lagrange_polynomials."""
    if n == 1:
        return [1]
    pts = [pow(w, i, R) for i in range(n)]
    if pow(t, n, R) == 1:
        return [1 if x == t else 0 for x in pts]
    l = (pow(t, n, R) - 1) * pow(n, -1, R) % R
    return [l * x % R * pow(t - x, -1, R) % R for x in pts]


def lagrange_closed(D, t):
    """evaluate_all_lagrange_polynomials: the basic row, and the step row as two basic rows times the other part's
    vanishing factor (libfqfft step_radix2_domain)."""
    if D.small_log is None:
        return lagrange_basic(D.m, D.w_int, t)
    w = D.w_int
    inner_big = lagrange_basic(D.big, w * w % R, t)
    inner_small = lagrange_basic(D.small, pow(w, 2 * D.big // D.small, R), t * pow(w, -1, R) % R)
    L0 = (pow(t, D.small, R) - D.c) % R
    big_part = [u * L0 % R * pow(pow(x, D.small, R) - D.c, -1, R) % R for u, x in zip(inner_big, D.points()[:D.big])]
    L1 = (pow(t, D.big, R) - 1) * pow(pow(w, D.big, R) - 1, -1, R) % R
    return big_part + [L1 * u % R for u in inner_small]


# ---------------------------------------------------------------------------------------------- quotient
@pytest.mark.parametrize("key", DOMAINS, ids=str)
def test_quotient_vs_oracle_transforms_and_integers(lsa, key):
    """Byte for byte, host mode and device mode, n = m."""
    a, b, c, d, want = case(key)
    assert np.array_equal(quotient(lsa, key, a, b, c, d), want)
    assert np.array_equal(quotient(lsa, key, a, b, c, d, device=True), want)


@pytest.mark.parametrize("key", SMALL_DOMAINS, ids=str)
def test_quotient_of_shorter_vectors(lsa, key):
    """n = m - 3 and n = 1: entries n .. m-1 count as zero."""
    D = dom(key)
    for n in sorted({max(D.m - 3, 1), 1}):
        a, b, c, d, want = case(key, n)
        assert np.array_equal(quotient(lsa, key, a, b, c, d), want), n
        assert np.array_equal(quotient(lsa, key, a, b, c, d, device=True), want), n


@pytest.mark.parametrize("key", [(3, None), (12, None), (7, 0)], ids=str)
def test_quotient_of_no_values_takes_empty_device_tensors(lsa, key):
    """n = 0 in device mode: an empty tensor's address is null, and null a, b, c were refused whatever n was (found by the
    randomised parity run: hadamard_quotient, case seed 333683051795).  All three vectors count as zero: H = d1 d2 Z - d3."""
    import torch
    D = dom(key)
    d = dec(rand_fr(3, 4040 + D.m))
    H = [0] * (D.m + 1)
    H[0] = -d[2] % R
    D.add_poly_Z(d[0] * d[1] % R, H)
    none = np.zeros((0, 4), dtype=np.uint64)
    assert np.array_equal(quotient(lsa, key, none, none, none, d), enc(H))
    t = [torch.zeros((0, 4), dtype=torch.int64, device="cuda:0") for _ in range(3)]
    assert all(x.data_ptr() == 0 for x in t)
    h = lsa.fr_hadamard_quotient(t[0], t[1], t[2], enc(d), D.big_log, D.small_log, omega=D.w, coset=o.fr_mont(G))
    lsa.synchronize()
    assert np.array_equal(h.cpu().numpy().view(np.uint64), enc(H))


@pytest.mark.parametrize("key", [k for k in DOMAINS if dom(k).m <= 96], ids=str)
def test_quotient_identity_at_a_random_point(lsa, key):
    """Independent of the oracle's transforms, for c = a o b: H(x) Z(x) = (A(x) + d1 Z(x))(B(x) + d2 Z(x)) - (C(x) + d3 Z(x)) at a random x,
    A, B, C evaluated by the Lagrange product formula over the domain's points."""
    D = dom(key)
    a, b, _, d, _ = case(key)
    c = enc([x * y % R for x, y in zip(dec(a), dec(b))])       # a satisfied relation: only then is (A B - C) / Z a polynomial
    H = dec(quotient(lsa, key, a, b, c, d, device=True))
    assert np.array_equal(enc(H), quotient(lsa, key, a, b, c, d))
    chi = dec(rand_fr(1, 4242 + D.m))[0]
    L = lagrange_products(D.points(), chi)
    Ax, Bx, Cx = (sum(v * l for v, l in zip(dec(x), L)) % R for x in (a, b, c))
    Zx = D.Z(chi)
    assert Zx != 0
    assert horner(H, chi) * Zx % R == ((Ax + d[0] * Zx) * (Bx + d[1] * Zx) - (Cx + d[2] * Zx)) % R


@pytest.mark.parametrize("key", MID, ids=str)
def test_quotient_special_inputs(lsa, key):
    D = dom(key)
    m = D.m
    a, b, _, d, _ = case(key)
    # c = a o b and no randomness: H is the exact quotient (A B - C) / Z.  It is identically zero where A B has degree < m
    # (constant vectors: A = alpha, B = beta, C = alpha beta); in general it has degree <= m - 2 and H Z = A B - C holds as
    # polynomials -- checked at a random point on the oracle's interpolants
    zero3 = [0, 0, 0]
    alpha, beta = dec(a[:2])
    const = [np.tile(o.fr_mont(v), (m, 1)) for v in (alpha, beta, alpha * beta)]
    c = enc([x * y % R for x, y in zip(dec(a), dec(b))])
    A, B, C = (dec(D.transform(x, inverse=True)) for x in (a, b, c))
    chi = dec(rand_fr(1, 777 + m))[0]
    for device in (False, True):
        assert not quotient(lsa, key, const[0], const[1], const[2], zero3, device=device).any()
        H = dec(quotient(lsa, key, a, b, c, zero3, device=device))
        assert H[m] == 0 and H[m - 1] == 0 and any(H)
        assert horner(H, chi) * D.Z(chi) % R == (horner(A, chi) * horner(B, chi) - horner(C, chi)) % R
    # all-zero vectors: exactly d1 d2 Z - d3
    z = np.zeros((m, 4), dtype=np.uint64)
    H = [0] * (m + 1)
    H[0] = -d[2] % R
    D.add_poly_Z(d[0] * d[1] % R, H)
    for device in (False, True):
        assert np.array_equal(quotient(lsa, key, z, z, z, d, device=device), enc(H))
    # entries r - 1 (all of them; alternating with random ones), randomness r - 1
    top = np.tile(o.fr_mont(R - 1), (m, 1))
    mix = np.array(a)
    mix[::2] = o.fr_mont(R - 1)
    dtop = [R - 1, R - 1, R - 1]
    for x, y, w, dd in ((top, top, top, dtop), (mix, top, np.array(b), d), (top, mix, mix, dtop)):
        want = expected_h(D, x, y, w, dd)
        assert np.array_equal(quotient(lsa, key, x, y, w, dd), want)
        assert np.array_equal(quotient(lsa, key, x, y, w, dd, device=True), want)


@pytest.mark.parametrize("key", [(2, None), (11, None), (3, 0), (11, 3)], ids=str)
def test_quotient_writes_m_plus_one_entries_and_leaves_inputs_alone(lsa, key):
    import torch
    D = dom(key)
    m = D.m
    a, b, c, d, want = case(key)
    guard = np.uint64(0xA5A5A5A5A5A5A5A5)
    # host mode: the C entry point on a buffer with a guard entry behind the m + 1
    h = np.full((m + 2, 4), guard, dtype=np.uint64)
    ha, hb, hc = np.array(a), np.array(b), np.array(c)
    d123, cg = enc(d), o.fr_mont(G)
    sl = -1 if D.small_log is None else D.small_log
    lsa._check(lsa.lib().lsa_fr_hadamard_quotient(lsa._host_ptr(ha), lsa._host_ptr(hb), lsa._host_ptr(hc), m, D.big_log, sl, lsa._host_ptr(D.w),
                                                  lsa._host_ptr(cg), lsa._host_ptr(d123), lsa._host_ptr(h), 0))
    assert np.array_equal(h[:m + 1], want) and (h[m + 1] == guard).all()
    assert np.array_equal(ha, a) and np.array_equal(hb, b) and np.array_equal(hc, c)
    # device mode: the same through the wrapper's `out`
    t = [torch.from_numpy(np.array(x).view(np.int64)).to("cuda:0") for x in (a, b, c)]
    out = torch.from_numpy(np.full((m + 2, 4), guard, dtype=np.uint64).view(np.int64)).to("cuda:0")
    res = lsa.fr_hadamard_quotient(t[0], t[1], t[2], d123, D.big_log, D.small_log, omega=D.w, coset=cg, out=out)
    lsa.synchronize()
    assert res is out
    got = out.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:m + 1], want) and (got[m + 1] == guard).all()
    for x, k in zip(t, (a, b, c)):
        assert np.array_equal(x.cpu().numpy().view(np.uint64), k)


def test_quotient_over_alternating_domains(lsa):
    """Staging and the transforms' tables are reused across calls and the step domain's table of 1 / Z is replaced when
    the domain changes: the bytes stay the same."""
    order = [(11, 3), (5, 2), (11, 3), (11, None), (10, 9), (11, None), (5, 2), (17, 16), (11, 3)]
    for device in (False, True):
        for key in order:
            a, b, c, d, want = case(key)
            assert np.array_equal(quotient(lsa, key, a, b, c, d, device=device), want), (key, device)
    # another coset generator on the same step domain, then the first one again
    key = (5, 2)
    a, b, c, d, want = case(key)
    assert np.array_equal(quotient(lsa, key, a, b, c, d, coset=7), expected_h(dom(key), a, b, c, d, g=7))
    assert np.array_equal(quotient(lsa, key, a, b, c, d), want)


def test_quotient_error_paths(lsa):
    a, b, c, d, want = case((5, 2))
    a16, b16, c16, d16, want16 = case((5, None))
    step, basic = dom((5, 2)), dom((5, None))

    def call(D, x, y, z, n, big_log, sl, g, h=None, omega=True, dd=d):
        h = np.zeros((D.m + 1, 4), dtype=np.uint64) if h is None else h
        p = lambda v: None if v is None else lsa._host_ptr(np.ascontiguousarray(v))           # noqa: E731
        lsa._check(lsa.lib().lsa_fr_hadamard_quotient(p(x), p(y), p(z), n, big_log, sl, p(D.w) if omega else None,
                                                      p(o.fr_mont(g)) if g is not None else None, p(enc(dd)) if dd is not None else None, p(h), 0))
        return h

    def refused(match, *args, **kw):
        with pytest.raises(lsa.LsaError, match=match):
            call(*args, **kw)
        assert lsa.lib().lsa_last_error()                      # a message is left
        # a correct call right afterwards gives the right bytes
        assert np.array_equal(call(step, a, b, c, step.m, 5, 2, G), want)

    refused("coset", basic, a16, b16, c16, 32, 5, -1, 1)                             # g = 1
    refused("coset", basic, a16, b16, c16, 32, 5, -1, basic.w_int)                   # an m-th root of unity
    refused("coset", step, a, b, c, step.m, 5, 2, 1)
    refused("coset", step, a, b, c, step.m, 5, 2, step.w_int)                        # a 2 big-th root of unity
    refused("coset", step, a, b, c, step.m, 5, 2, R - 1)
    refused("n = 37", step, a, b, c, step.m + 1, 5, 2, G)
    refused("n = 33", basic, a16, b16, c16, 33, 5, -1, G)
    refused("null", step, None, b, c, step.m, 5, 2, G)
    refused("null", step, a, None, c, step.m, 5, 2, G)
    refused("null", step, a, b, None, step.m, 5, 2, G)
    refused("null", step, a, b, c, step.m, 5, 2, None)
    refused("null", step, a, b, c, step.m, 5, 2, G, omega=False)
    refused("null", step, a, b, c, step.m, 5, 2, G, dd=None)
    with pytest.raises(lsa.LsaError, match="null"):            # h_out
        lsa._check(lsa.lib().lsa_fr_hadamard_quotient(lsa._host_ptr(np.array(a)), lsa._host_ptr(np.array(b)), lsa._host_ptr(np.array(c)), step.m, 5, 2,
                                                      lsa._host_ptr(step.w), lsa._host_ptr(o.fr_mont(G)), lsa._host_ptr(enc(d)), None, 0))
    assert np.array_equal(call(step, a, b, c, step.m, 5, 2, G), want)
    refused("big_log", basic, a16, b16, c16, 1, 0, -1, G)                            # m = 1
    refused("big_log", basic, a16, b16, c16, 1, 29, -1, G)
    refused("big_log", step, a, b, c, 1, 28, 0, G)
    refused("big_log", step, a, b, c, 1, 5, 5, G)
    refused("big_log", step, a, b, c, 1, 5, 6, G)
    assert np.array_equal(call(basic, a16, b16, c16, 32, 5, -1, G, dd=d16), want16)
    # the Lagrange row's arguments
    out = np.zeros((40, 4), dtype=np.uint64)
    t = o.fr_mont(12345)
    for args, match in (((0, -1, lsa._host_ptr(basic.w), lsa._host_ptr(t), lsa._host_ptr(out), 0), "big_log"),
                        ((29, -1, lsa._host_ptr(basic.w), lsa._host_ptr(t), lsa._host_ptr(out), 0), "big_log"),
                        ((28, 0, lsa._host_ptr(basic.w), lsa._host_ptr(t), lsa._host_ptr(out), 0), "big_log"),
                        ((5, 5, lsa._host_ptr(basic.w), lsa._host_ptr(t), lsa._host_ptr(out), 0), "big_log"),
                        ((5, -1, None, lsa._host_ptr(t), lsa._host_ptr(out), 0), "null"),
                        ((5, -1, lsa._host_ptr(basic.w), None, lsa._host_ptr(out), 0), "null"),
                        ((5, -1, lsa._host_ptr(basic.w), lsa._host_ptr(t), None, 0), "null")):
        with pytest.raises(lsa.LsaError, match=match):
            lsa._check(lsa.lib().lsa_fr_lagrange(*args))
        assert np.array_equal(lsa.fr_lagrange(5, 2, step.w, t), enc(lagrange_closed(step, 12345)))


# ---------------------------------------------------------------------------------------------- Lagrange row
def lagrange_both_modes(lsa, D, t):
    import torch
    host = lsa.fr_lagrange(D.big_log, D.small_log, D.w, o.fr_mont(t))
    guard = np.uint64(0x5A5A5A5A5A5A5A5A)
    out = torch.from_numpy(np.full((D.m + 1, 4), guard, dtype=np.uint64).view(np.int64)).to("cuda:0")
    assert lsa.fr_lagrange(D.big_log, D.small_log, D.w, o.fr_mont(t), out=out) is out
    lsa.synchronize()
    dev = out.cpu().numpy().view(np.uint64)
    assert np.array_equal(dev[:D.m], host) and (dev[D.m] == guard).all()
    return host


@pytest.mark.parametrize("key", [k for k in DOMAINS if dom(k).m <= 96], ids=str)
def test_lagrange_vs_the_product_formula(lsa, key):
    D = dom(key)
    for t in (dec(rand_fr(1, 99 + D.m))[0], 0, 2):                 # (2^(2^28) != 1: 2 is in no domain)
        assert t not in D.points()
        assert np.array_equal(lagrange_both_modes(lsa, D, t), enc(lagrange_products(D.points(), t))), t


@pytest.mark.parametrize("key", SMALL_DOMAINS, ids=str)
def test_lagrange_vs_the_closed_formulae(lsa, key):
    """Random t, t = 0, and t a point of the domain: the first, the last, the first of the small part (the unit vector)."""
    D = dom(key)
    pts = D.points()
    ts = [dec(rand_fr(1, 555 + D.m))[0], 0, pts[0], pts[-1], pts[D.m // 2], pts[D.big - 1]]
    if D.small_log is not None:
        ts.append(pts[D.big])
    for t in ts:
        want = lagrange_closed(D, t)
        if t in pts:
            assert want == [1 if x == t else 0 for x in pts]
        assert np.array_equal(lagrange_both_modes(lsa, D, t), enc(want)), t


@pytest.mark.parametrize("key", [(16, None), (17, None), (17, 16)], ids=str)
def test_lagrange_identities_at_large_sizes(lsa, key):
    """sum_i L_i(t) = 1 and sum_i a_i L_i(t) = A(t), A the oracle's interpolant of a (Horner at t)."""
    D = dom(key)
    t = dec(rand_fr(1, 31337 + D.m))[0]
    row = lagrange_both_modes(lsa, D, t)
    ones = np.tile(o.fr_mont(1), (D.m, 1))
    assert o.fr_dot(ones, row) == 1
    a = rand_fr(D.m, 8000 + D.m)
    assert o.fr_dot(a, row) == horner(dec(D.transform(a, inverse=True)), t)
    # t a point of the domain: the unit vector
    for idx in (0, D.big - 1, D.big if D.small_log is not None else D.m // 3, D.m - 1):
        unit = np.zeros((D.m, 4), dtype=np.uint64)
        unit[idx] = o.fr_mont(1)
        assert np.array_equal(lagrange_both_modes(lsa, D, D.point(idx)), unit), idx


# ---------------------------------------------------------------------------------------------- end to end
def g1_neg(pt):
    x, y = o.g1_canonical_affine(pt)
    return o.g1_from_affine((x, o.P - y))


@pytest.mark.parametrize("key", [(3, 2), (4, None)], ids=str)
def test_lipmaa_keygen_commit_prove_verify(lsa, key):
    """CPHadL end to end on m = 12 (step 2^3 + 2^2) and m = 16: key from fr_lagrange + batch_exp, commitments by msm, the
    proof by Bases.msm_async on the device-resident quotient (nothing downloaded in between), and the verifier's pairing
    product e(c_a, kc_b) e(-G1, kc_c) e(-pi, gamma Z(chi) G2) = 1 (lipmaa.cc:187-207); with one entry of c changed it is not."""
    import torch
    D = dom(key)
    m = D.m
    chi, gamma = dec(rand_fr(2, 2024 + m))
    g1, g2 = o.generator("g1"), o.generator("g2")
    # keygen
    row = lsa.fr_lagrange(D.big_log, D.small_log, D.w, o.fr_mont(chi))
    Li = dec(row)
    Zchi = D.Z(chi)
    lag_g1 = lsa.batch_exp("g1", g1, np.concatenate([row, o.fr_mont(Zchi).reshape(1, 4)]))
    lag_g2 = lsa.batch_exp("g2", g2, enc([gamma * x % R for x in Li] + [gamma * Zchi % R]))
    chipows = lsa.Bases("g1", lsa.batch_exp("g1", g1, enc([pow(chi, i, R) for i in range(m + 1)])))
    # witness and commitments (the randomness rides on the Z(chi) base)
    a, b, _, d, _ = case(key)
    ai, bi = dec(a), dec(b)
    ci = [x * y % R for x, y in zip(ai, bi)]

    def verify(ci):
        c = enc(ci)
        c_a = lsa.msm("g1", lag_g1, np.concatenate([a, enc(d[0:1])]))
        kc_b = lsa.msm("g2", lag_g2, np.concatenate([b, enc(d[1:2])]))
        kc_c = lsa.msm("g2", lag_g2, np.concatenate([c, enc(d[2:3])]))
        # prove: the quotient stays on the device and is the MSM's scalar vector
        t = [torch.from_numpy(np.array(x).view(np.int64)).to("cuda:0") for x in (a, b, c)]
        d_h = lsa.fr_hadamard_quotient(t[0], t[1], t[2], enc(d), D.big_log, D.small_log, omega=D.w, coset=o.fr_mont(G))
        d_pi = torch.zeros(12, dtype=torch.int64, device="cuda:0")
        chipows.msm_async(d_h, d_pi)
        lsa.stream_join()
        lsa.synchronize()
        pi = d_pi.cpu().numpy().view(np.uint64)
        return lsa.pairing_product(np.stack([c_a, g1_neg(g1), g1_neg(pi)]), np.stack([kc_b, kc_c, lag_g2[m]]))

    assert np.array_equal(verify(ci), o.fq12_one())
    ci[m // 2] = (ci[m // 2] + 1) % R
    assert not np.array_equal(verify(ci), o.fq12_one())
