"""GPU suite: batch point decompression, validation and compression (csrc/point_load.hip, csrc/fq_sqrt.h) through the Python
wrapper -- legosnark_amd.decompress / validate_points / compress -- in host mode (numpy) and in device mode (torch CUDA tensors).

Every expected value is Python integers (oracle/pymodel/bn254_model.py for the curve arithmetic; the ladder over the whole twist
is this file's own, because the model's g2_mul reduces the scalar mod r).  The words of a value v are v 2^256 mod p.  Expected
outputs are exact bytes: the Y of a decompressed point is the root of x^3 + b whose parity equals flag bit 0, which is unique.

The case lists mix accepted and rejected entries; a batch of n entries is the list repeated, so that good and bad lanes sit
next to each other in every wavefront.  Sizes 0, 1, 255, 256, 257 (around the 256-lane workgroup) and 600 (three workgroups of
mixed lanes).  The kernels have no grid-stride loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "pymodel"))
import bn254_model as m  # noqa: E402

P, R = m.P, m.R
MONT = (1 << 256) % P
COFACTOR = 2 * P - R
OK, INFINITY, MALFORMED, NOT_ON_CURVE, NOT_IN_SUBGROUP = range(5)
SIZES = [0, 1, 255, 256, 257, 600]
KS = [1, 2, 3, 12345, 1000003]
JUNK = (1 << 256) - 1


def mont(v):
    return v % P * MONT % P


def words(ints):
    """256-bit integers -> their little-endian uint64 words, four per integer, flat."""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype=np.uint64).copy()


def fq_sqrt(a):
    r = pow(a, (P + 1) // 4, P)
    return r if r * r % P == a % P else None


def f2_sqrt(a):
    a0, a1 = a
    if a1 == 0:
        r = fq_sqrt(a0)
        if r is not None:
            return (r, 0)
        r = fq_sqrt(-a0 % P)
        return None if r is None else (0, r)
    sn = fq_sqrt((a0 * a0 + a1 * a1) % P)
    if sn is None:
        return None
    for s in (sn, -sn):
        x0 = fq_sqrt((a0 + s) * m.inv(2) % P)
        if x0:
            y = (x0, a1 * m.inv(2 * x0) % P)
            assert m.f2_sqr(y) == (a0 % P, a1 % P)
            return y
    return None


def twist_ladder(p, k):
    """[k]p on the whole twist, k not reduced."""
    acc = None
    for bit in bin(k)[2:]:
        acc = m.g2_add(acc, acc)
        if bit == "1":
            acc = m.g2_add(acc, p)
    return acc


def g2_rhs(x):
    return m.f2_add(m.f2_mul(m.f2_sqr(x), x), m.TWIST_B)


class Model:
    """The points of the tests, as Python integers, computed once."""

    def __init__(self):
        assert fq_sqrt(3) is None                                   # x = 0 is not the abscissa of a G1 point
        self.g1 = [m.g1_mul(m.G1_GEN, k) for k in KS]
        self.g2 = [m.g2_mul(m.G2_GEN, k) for k in KS]
        twist = []
        i = 1
        while len(twist) < 2:
            y = f2_sqrt(g2_rhs((i, 1)))
            if y is not None:
                twist.append(((i, 1), y))
            i += 1
        self.twist = twist
        for t in twist:
            assert m.g2_is_on_curve(t) and twist_ladder(t, R) is not None       # outside G2
        self.cofactor_multiples = [twist_ladder(t, COFACTOR) for t in twist]
        for q in self.cofactor_multiples:
            assert q is not None and twist_ladder(q, R) is None                    # in G2
        assert COFACTOR % 10069 == 0 and COFACTOR % 5864401 == 0
        rt = twist_ladder(twist[0], R)
        self.s1 = twist_ladder(rt, COFACTOR // 10069)
        self.s2 = twist_ladder(rt, COFACTOR // 5864401)
        assert self.s1 is not None and twist_ladder(self.s1, 10069) is None
        assert self.s2 is not None and twist_ladder(self.s2, 5864401) is None
        self.outside = [twist[0], twist[1], self.s1, self.s2, m.g2_add(self.g2[3], self.s1), m.g2_add(self.g2[4], self.s2)]
        for q in self.outside:
            assert m.g2_is_on_curve(q) and twist_ladder(q, R) is not None
        # an x of the twist's field with a non-square right-hand side
        i = 1
        while f2_sqrt(g2_rhs((i, 1))) is not None:
            i += 1
        self.g2_no_root = (i, 1)


@pytest.fixture(scope="module")
def model():
    return Model()


# ---------------------------------------------------------------- encodings
def width(group):
    return 1 if group == "g1" else 2


def coords(group, v):
    """A field element of the group's coordinate field as a list of integers (1 or 2)."""
    return [v] if group == "g1" else list(v)


def zero_of(group):
    return [0] * width(group)


def parity(group, y):
    return (y if group == "g1" else y[0]) & 1


def neg(group, y):
    return (-y) % P if group == "g1" else m.f2_neg(y)


def point_words(group, x, y, z):
    """Jacobian words of (x, y, z), each a coordinate as integers (values, not words)."""
    return [mont(v) for v in coords(group, x) + coords(group, y) + coords(group, z)]


def inf_words(group):
    return [0] * width(group) + [MONT] + [0] * (width(group) - 1) + [0] * width(group)


class Entry:
    """One compressed input and what decompression must make of it: x_raw are WORDS (integers below 2^256)."""

    def __init__(self, x_raw, flag, status, out_words):
        self.x_raw, self.flag, self.status, self.out_words = x_raw, flag, status, out_words


def accepted(group, pt, flip=False):
    x, y = pt
    want_y = neg(group, y) if flip else y
    one = 1 if group == "g1" else (1, 0)
    return Entry([mont(v) for v in coords(group, x)], parity(group, want_y), OK, point_words(group, x, want_y, one))


def decompress_entries(group, model, check_subgroup):
    w = width(group)
    inf = inf_words(group)
    pts = model.g1 if group == "g1" else model.g2
    es = []
    for pt in pts:
        es.append(accepted(group, pt))
        es.append(accepted(group, pt, flip=True))
    good_x = [mont(v) for v in coords(group, pts[1][0])]
    if group == "g1":
        es.append(Entry([0], 0, NOT_ON_CURVE, inf))                               # rhs = 3
        es.append(Entry([0], 1, NOT_ON_CURVE, inf))
    else:
        es.append(Entry([mont(v) for v in model.g2_no_root], 0, NOT_ON_CURVE, inf))
        for q in model.outside:
            e = accepted(group, q)
            if check_subgroup:
                e.status, e.out_words = NOT_IN_SUBGROUP, inf
            es.append(e)
        for q in model.cofactor_multiples:
            es.append(accepted(group, q))
            es.append(accepted(group, q, flip=True))
    for bad in (P, JUNK, P + 1):
        for pos in range(w):                                                       # the bad word in each component
            xr = list(good_x)
            xr[pos] = bad
            es.append(Entry(xr, 0, MALFORMED, inf))
    es.append(Entry([JUNK] * w, 2, INFINITY, inf))                                 # the zero flag, junk in X
    es.append(Entry([JUNK] * w, 3, INFINITY, inf))
    es.append(Entry([0] * w, 2, INFINITY, inf))
    es.append(Entry(good_x, 4, MALFORMED, inf))
    es.append(Entry(good_x, 0x81, MALFORMED, inf))
    es.append(Entry([P] * w, 4, MALFORMED, inf))
    return es


def batch(entries, n, offset=0):
    return [entries[(i + offset) % len(entries)] for i in range(n)]


def run_decompress(lsa, group, mode, x, flags, check_subgroup):
    if mode == "host":
        return lsa.decompress(group, x, flags, check_subgroup=check_subgroup)
    import torch
    d_x = torch.from_numpy(x.view(np.int64)).to("cuda:0")
    d_f = torch.from_numpy(flags).to("cuda:0")
    pts, st = lsa.decompress(group, d_x, d_f, check_subgroup=check_subgroup)
    lsa.synchronize()
    return pts.cpu().numpy().view(np.uint64), st.cpu().numpy()


def run_validate(lsa, group, mode, pts, check_subgroup):
    if mode == "host":
        return lsa.validate_points(group, pts, check_subgroup=check_subgroup)
    import torch
    st = lsa.validate_points(group, torch.from_numpy(pts.view(np.int64)).to("cuda:0"), check_subgroup=check_subgroup)
    lsa.synchronize()
    return st.cpu().numpy()


def run_compress(lsa, group, mode, pts):
    if mode == "host":
        return lsa.compress(group, pts)
    import torch
    x, f = lsa.compress(group, torch.from_numpy(pts.view(np.int64)).to("cuda:0"))
    lsa.synchronize()
    return x.cpu().numpy().view(np.uint64), f.cpu().numpy()


# ---------------------------------------------------------------- decompress
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("group,check_subgroup", [("g1", True), ("g2", True), ("g2", False)])
def test_decompress(lsa, model, group, check_subgroup, mode):
    entries = decompress_entries(group, model, check_subgroup)
    w = width(group)
    assert {e.status for e in entries} == ({OK, INFINITY, MALFORMED, NOT_ON_CURVE} | ({NOT_IN_SUBGROUP} if group == "g2" and check_subgroup else set()))
    for n in SIZES:
        es = batch(entries, n, offset=n)
        x = words([v for e in es for v in e.x_raw]).reshape(n, 4 * w)
        flags = np.array([e.flag for e in es], dtype=np.uint8)
        pts, st = run_decompress(lsa, group, mode, x, flags, check_subgroup)
        assert pts.shape == (n, 12 * w) and st.shape == (n,)
        want_st = np.array([e.status for e in es], dtype=np.uint8)
        want = words([v for e in es for v in e.out_words]).reshape(n, 12 * w)
        assert np.array_equal(st, want_st), (n, np.nonzero(st != want_st)[0][:8], st[st != want_st][:8], want_st[st != want_st][:8])
        assert np.array_equal(pts, want), (n, np.nonzero((pts != want).any(axis=1))[0][:8])


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("group", ["g1", "g2"])
def test_decompress_counts_the_rejected(lsa, model, group, mode):
    """n_rejected through the C-ABI itself (the wrapper passes NULL): the number of statuses >= 2; with it the device mode blocks."""
    entries = decompress_entries(group, model, True)
    w = width(group)
    L = lsa.lib()
    for n in (257, 600):
        es = batch(entries, n)
        x = words([v for e in es for v in e.x_raw]).reshape(n, 4 * w)
        flags = np.array([e.flag for e in es], dtype=np.uint8)
        want = sum(1 for e in es if e.status >= MALFORMED)
        assert 0 < want < n
        count = C.c_uint64(12345)
        if mode == "host":
            out = np.zeros((n, 12 * w), dtype=np.uint64)
            st = np.zeros(n, dtype=np.uint8)
            ptrs = [a.ctypes.data for a in (x, flags, out, st)]
        else:
            import torch
            d = [torch.from_numpy(x.view(np.int64)).to("cuda:0"), torch.from_numpy(flags).to("cuda:0"),
                 torch.empty((n, 12 * w), dtype=torch.int64, device="cuda:0"), torch.empty(n, dtype=torch.uint8, device="cuda:0")]
            torch.cuda.synchronize()
            ptrs = [t.data_ptr() for t in d]
        dev = 0 if mode == "host" else 1
        if group == "g1":
            rc = L.lsa_g1_decompress(ptrs[0], ptrs[1], n, ptrs[2], ptrs[3], C.byref(count), dev)
        else:
            rc = L.lsa_g2_decompress(ptrs[0], ptrs[1], n, 1, ptrs[2], ptrs[3], C.byref(count), dev)
        assert rc == 0 and count.value == want
        if mode == "device":
            st = d[3].cpu().numpy()                                               # no synchronize: the call blocked
        assert int((st >= MALFORMED).sum()) == want


# ---------------------------------------------------------------- validate
def rand_z(group, rng):
    vals = [int.from_bytes(rng.bytes(31), "little") + 1 for _ in range(width(group))]
    return vals[0] if group == "g1" else tuple(vals)


def fmul(group, a, b):
    return a * b % P if group == "g1" else m.f2_mul(a, b)


def rescaled(group, pt, z):
    x, y = pt
    z2 = fmul(group, z, z)
    return fmul(group, x, z2), fmul(group, y, fmul(group, z2, z)), z


class VEntry:
    def __init__(self, raw, status, affine=None):
        self.raw, self.status, self.affine = raw, status, affine                   # raw: the 3 w WORDS; affine: (x, y) or "inf" for valid points


def validate_entries(group, model, check_subgroup):
    rng = np.random.default_rng(7)
    w = width(group)
    es = []
    valid = (model.g1 + [m.g1_neg(q) for q in model.g1]) if group == "g1" else (model.g2 + [m.g2_neg(q) for q in model.g2] + model.cofactor_multiples)
    for q in valid:
        es.append(VEntry(point_words(group, *rescaled(group, q, rand_z(group, rng))), OK, q))
    es.append(VEntry(point_words(group, valid[0][0], valid[0][1], 1 if group == "g1" else (1, 0)), OK, valid[0]))       # Z = one
    if group == "g2":
        for q in model.outside:
            es.append(VEntry(point_words(group, *rescaled(group, q, rand_z(group, rng))), NOT_IN_SUBGROUP if check_subgroup else OK, q if not check_subgroup else None))
    good = point_words(group, *rescaled(group, valid[2], rand_z(group, rng)))
    for bit in (0, 1, 200):                                                        # one bit of Y flipped
        for comp in range(w):
            raw = list(good)
            raw[w + comp] ^= 1 << bit
            assert raw[w + comp] < P
            es.append(VEntry(raw, NOT_ON_CURVE))
    raw = list(good)
    raw[0] ^= 1 << 7                                                               # ... and one of X
    assert raw[0] < P
    es.append(VEntry(raw, NOT_ON_CURVE))
    # Z == 0: infinity, whatever X and Y spell below p
    es.append(VEntry(inf_words(group), INFINITY, "inf"))
    es.append(VEntry(good[:2 * w] + [0] * w, INFINITY, "inf"))
    es.append(VEntry([P - 1] * (2 * w) + [0] * w, INFINITY, "inf"))
    # a malformed word in each coordinate (each component of it)
    for pos in range(3 * w):
        for bad in (P, JUNK):
            raw = list(good)
            raw[pos] = bad
            es.append(VEntry(raw, MALFORMED))
    # precedence: MALFORMED before INFINITY and before NOT_ON_CURVE
    es.append(VEntry([P] + good[1:2 * w] + [0] * w, MALFORMED))                    # Z == 0 and X out of range
    raw = list(good)
    raw[w] ^= 1                                                                     # off the curve ...
    raw[0] = P                                                                      # ... and out of range
    es.append(VEntry(raw, MALFORMED))
    if group == "g2":                                                              # NOT_ON_CURVE before NOT_IN_SUBGROUP
        raw = point_words(group, *rescaled(group, model.outside[0], rand_z(group, rng)))
        raw[w] ^= 2
        assert raw[w] < P
        es.append(VEntry(raw, NOT_ON_CURVE))
    return es


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("group,check_subgroup", [("g1", True), ("g2", True), ("g2", False)])
def test_validate(lsa, model, group, check_subgroup, mode):
    entries = validate_entries(group, model, check_subgroup)
    w = width(group)
    assert {e.status for e in entries} == ({OK, INFINITY, MALFORMED, NOT_ON_CURVE} | ({NOT_IN_SUBGROUP} if group == "g2" and check_subgroup else set()))
    for n in SIZES:
        es = batch(entries, n, offset=n)
        pts = words([v for e in es for v in e.raw]).reshape(n, 12 * w)
        before = pts.copy()
        st = run_validate(lsa, group, mode, pts, check_subgroup)
        want_st = np.array([e.status for e in es], dtype=np.uint8)
        assert st.shape == (n,) and np.array_equal(st, want_st), (n, np.nonzero(st != want_st)[0][:8], st[st != want_st][:8], want_st[st != want_st][:8])
        assert np.array_equal(pts, before)
    # n_rejected through the C-ABI
    n = 600
    es = batch(entries, n)
    pts = words([v for e in es for v in e.raw]).reshape(n, 12 * w)
    st = np.zeros(n, dtype=np.uint8)
    count = C.c_uint64(0)
    if group == "g1":
        rc = lsa.lib().lsa_g1_validate(pts.ctypes.data, n, st.ctypes.data, C.byref(count), 0)
    else:
        rc = lsa.lib().lsa_g2_validate(pts.ctypes.data, n, 1 if check_subgroup else 0, st.ctypes.data, C.byref(count), 0)
    assert rc == 0 and count.value == sum(1 for e in es if e.status >= MALFORMED) > 0


# ---------------------------------------------------------------- compress
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("group", ["g1", "g2"])
def test_compress_and_round_trip(lsa, model, group, mode):
    """compress: X of the affine form, the model's parity; decompress(compress(P)) is the normalised P, for every valid point
    of the validation list (for G2 the twist points outside G2 too: compression does not care), infinity included."""
    entries = [e for e in validate_entries(group, model, False) if e.affine is not None]
    w = width(group)
    assert any(e.affine == "inf" for e in entries) and len(entries) > 12
    one = 1 if group == "g1" else (1, 0)
    for n in SIZES:
        es = batch(entries, n, offset=n)
        pts = words([v for e in es for v in e.raw]).reshape(n, 12 * w)
        x, flags = run_compress(lsa, group, mode, pts)
        assert x.shape == (n, 4 * w) and flags.shape == (n,)
        want_x = words([v for e in es for v in (zero_of(group) if e.affine == "inf" else [mont(c) for c in coords(group, e.affine[0])])]).reshape(n, 4 * w)
        want_f = np.array([3 if e.affine == "inf" else parity(group, e.affine[1]) for e in es], dtype=np.uint8)
        assert np.array_equal(x, want_x), (n, np.nonzero((x != want_x).any(axis=1))[0][:8])
        assert np.array_equal(flags, want_f), (n, np.nonzero(flags != want_f)[0][:8])
        back, st = run_decompress(lsa, group, mode, x, flags, False)
        want_back = words([v for e in es for v in (inf_words(group) if e.affine == "inf" else point_words(group, e.affine[0], e.affine[1], one))]).reshape(n, 12 * w)
        assert np.array_equal(st, np.array([INFINITY if e.affine == "inf" else OK for e in es], dtype=np.uint8))
        assert np.array_equal(back, want_back)
        if mode == "host" and n:
            assert np.array_equal(lsa.normalize(group, pts), want_back)           # the library's own normalisation agrees


# ---------------------------------------------------------------- argument checks
INVALID = -2


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_argument_checks(lsa, model, group):
    L = lsa.lib()
    w = width(group)
    n = 4
    es = batch(decompress_entries(group, model, True), n)
    x = words([v for e in es for v in e.x_raw]).reshape(n, 4 * w)
    flags = np.array([e.flag for e in es], dtype=np.uint8)
    out = np.zeros((n, 12 * w), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    count = C.c_uint64(77)
    sub = [] if group == "g1" else [1]
    dec = L.lsa_g1_decompress if group == "g1" else L.lsa_g2_decompress
    val = L.lsa_g1_validate if group == "g1" else L.lsa_g2_validate
    com = L.lsa_g1_compress if group == "g1" else L.lsa_g2_compress
    px, pf, po, ps = x.ctypes.data, flags.ctypes.data, out.ctypes.data, st.ctypes.data
    # n == 0 is fine, nulls and all
    assert dec(None, None, 0, *sub, None, None, C.byref(count), 0) == 0 and count.value == 0
    assert val(None, 0, *sub, None, None, 0) == 0
    assert com(None, 0, None, None, 0) == 0
    # a null pointer with n > 0
    for args in ((None, pf, n, *sub, po, ps), (px, None, n, *sub, po, ps), (px, pf, n, *sub, None, ps), (px, pf, n, *sub, po, None)):
        assert dec(*args, None, 0) == INVALID
        assert dec(*args, None, 1) == INVALID
    assert val(None, n, *sub, ps, None, 0) == INVALID and val(po, n, *sub, None, None, 0) == INVALID
    assert com(None, n, px, pf, 0) == INVALID and com(po, n, None, pf, 0) == INVALID and com(po, n, px, None, 0) == INVALID
    # an output that overlaps an input
    assert dec(px, pf, n, *sub, px, ps, None, 0) == INVALID                       # out on x
    assert dec(po + 8, pf, n, *sub, po, ps, None, 0) == INVALID                   # x inside out
    assert dec(px, pf, n, *sub, po, pf, None, 0) == INVALID                       # status on flags
    assert dec(px, pf, n, *sub, po, po + 16, None, 0) == INVALID                  # status inside out
    assert val(po, n, *sub, po + 5, None, 0) == INVALID
    assert com(po, n, po, pf, 0) == INVALID and com(po, n, px, po + 1, 0) == INVALID
    # a byte count that overflows
    assert dec(px, pf, (1 << 63), *sub, po, ps, None, 0) == INVALID
    assert val(po, (1 << 62), *sub, ps, None, 0) == INVALID
    assert com(po, (1 << 62) + 1, px, pf, 0) == INVALID
    assert b"overflow" in L.lsa_last_error()
    # nothing was written by the refused calls, and the same buffers still work
    assert not out.any() and not st.any()
    assert dec(px, pf, n, *sub, po, ps, C.byref(count), 0) == 0
    assert np.array_equal(st, np.array([e.status for e in es], dtype=np.uint8)) and count.value == sum(1 for e in es if e.status >= MALFORMED)
    # the wrapper refuses mixed or mis-sized operands before the library sees them
    with pytest.raises(ValueError):
        lsa.decompress(group, x, flags[:-1])
    with pytest.raises(ValueError):
        lsa.decompress(group, x, flags, out=out)
    pts, status = lsa.decompress(group, np.zeros((0, 4 * w), dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    assert pts.shape == (0, 12 * w) and status.shape == (0,)
