"""GPU parity tests for the discrete Fourier transform on group elements (lsa_g1_ecntt / lsa_g2_ecntt, csrc/ecntt.hip)
through the Python wrappers, against the oracle: every output as its own small MSM over the inputs (libff's scalar * point
sums), the known-discrete-log identity out = batch_exp(G, fr_domain_transform(a)), and the key flow of INTEGRATION.md "Lipmaa
keys from a powers string (no trapdoor)" checked with InterpCommScheme::verify's pairing equation.  Group elements are compared
after affine normalisation.  The grid-stride test takes its size from the kernel's own figures (ecntt_params)."""
import ctypes as C
import random
import sys
import os

import numpy as np
import pytest

import oracle_lib as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "pymodel"))
import test_points_io_gpu as pio  # noqa: E402  (outside_point)

pytestmark = pytest.mark.gpu
R, P = o.R, o.P
WIDTH = {"g1": 12, "g2": 24}
GROUPS = ("g1", "g2")
ERR_INVALID = -2                                               # LSA_ERR_INVALID


def mont_array(ints):
    buf = b"".join((x % R * o.MONT % R).to_bytes(32, "little") for x in ints)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def canon_all(group, pts):
    f = o.g1_canonical_affine if group == "g1" else o.g2_canonical_affine
    return [f(p) for p in np.asarray(pts, dtype=np.uint64).reshape(-1, WIDTH[group])]


def omega(n):
    return o.fr_root_of_unity(n.bit_length() - 1)


def rescaled(group, pts, rng):
    """The same points with random Z coordinates (an infinity stays Z = 0)."""
    out = []
    for c in canon_all(group, pts):
        if c is None:
            out.append(np.zeros(WIDTH[group], dtype=np.uint64))
        elif group == "g1":
            out.append(o.g1_from_affine(c, rng.randrange(1, P)))
        else:
            out.append(o.g2_from_affine(c, (rng.randrange(1, P), rng.randrange(P))))
    return np.stack(out)


def oracle_sums(group, pts, inverse):
    """want[k] = sum_i omega^(+-ik) (1/n) pts[i]: n sums of libff's scalar * point through the C oracle."""
    n = len(pts)
    w = pow(omega(n), -1, R) if inverse else omega(n)
    c = pow(n, -1, R) if inverse else 1
    return [canon_all(group, o.multi_exp(group, pts, mont_array([pow(w, i * k, R) * c for i in range(n)]), mode="inner"))[0]
            for k in range(n)]


def run(lsa, group, pts, inverse, device, in_place=False):
    """ecntt in host or device mode; the result as a host array."""
    w = o.fr_mont(omega(len(pts)))
    if not device:
        buf = pts.copy()
        out = lsa.ecntt(group, buf, w, inverse=inverse, out=buf if in_place else None)
        if not in_place:
            assert np.array_equal(buf, pts)                    # the input is left alone
        return out
    import torch
    d = torch.from_numpy(pts.view(np.int64).copy()).to("cuda:0")
    d_out = lsa.ecntt(group, d, w, inverse=inverse, out=d if in_place else None)
    lsa.synchronize()
    assert tuple(d_out.shape) == (len(pts), WIDTH[group])
    if not in_place:
        assert np.array_equal(d.cpu().numpy().view(np.uint64), pts)
    return d_out.cpu().numpy().view(np.uint64)


def sample_input(group, n, seed):
    """arith_bases (un-normalised Jacobian) with a few infinities and the generator among them."""
    pts = o.arith_bases(group, 1000003 + seed, 7919 + seed, n)
    if n >= 4:
        pts[1] = 0
        pts[n - 1] = 0
        pts[2] = o.generator(group)
    return pts


# ---------------------------------------------------------------- 1. against the oracle's own sums
@pytest.mark.parametrize("n", [1, 2, 4, 8, 64])
@pytest.mark.parametrize("group", GROUPS)
def test_ecntt_vs_oracle_sums(lsa, group, n):
    pts = sample_input(group, n, n)
    for inverse in (False, True):
        want = oracle_sums(group, pts, inverse)
        for device in (False, True):
            got = run(lsa, group, pts, inverse, device)
            assert canon_all(group, got) == want, (inverse, device)
            assert canon_all(group, run(lsa, group, pts, inverse, device, in_place=True)) == want, ("in place", inverse, device)
            back = run(lsa, group, got, not inverse, device)   # inverse(forward(x)) == x and forward(inverse(x)) == x
            assert canon_all(group, back) == canon_all(group, pts), ("round trip", inverse, device)


# ---------------------------------------------------------------- 2. degenerate inputs (a commitment key is n copies of one generator)
@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("group", GROUPS)
def test_ecntt_degenerate_inputs(lsa, group, n):
    rng = random.Random(100 + n)
    p_log = 0x1234567 + n
    pt = o.batch_exp(group, o.generator(group), mont_array([p_log]))[0]
    p_c = canon_all(group, pt)[0]
    np_c = canon_all(group, o.batch_exp(group, o.generator(group), mont_array([n * p_log])))[0]
    w = omega(n)
    # all inputs equal: stage 1 meets A == T (the doubling branch) and A - T == infinity in every butterfly
    same = rescaled(group, np.tile(pt, (n, 1)), rng)
    want = oracle_sums(group, same, False)
    assert want == [np_c] + [None] * (n - 1)
    for device in (False, True):
        assert canon_all(group, run(lsa, group, same, False, device)) == want
    # (P, infinity, ..., infinity): every output is P
    one = np.zeros((n, WIDTH[group]), dtype=np.uint64)
    one[0] = same[0]
    want = oracle_sums(group, one, False)
    assert want == [p_c] * n
    assert canon_all(group, run(lsa, group, one, False, False)) == want
    # pure frequencies: a cancellation in every stage that has a non-trivial twiddle
    for k0 in (1, n // 2, n - 1):
        logs = [p_log * pow(w, -i * k0, R) for i in range(n)]
        freq = rescaled(group, o.batch_exp(group, o.generator(group), mont_array(logs)), rng)
        want = oracle_sums(group, freq, False)
        assert want == [np_c if k == k0 else None for k in range(n)]
        assert canon_all(group, run(lsa, group, freq, False, k0 == 1)) == want, k0
        # and the inverse of the spike is the frequency again
        assert canon_all(group, run(lsa, group, np.stack([same[0] if k == k0 else one[1] for k in range(n)]), True, False)) == \
            canon_all(group, o.batch_exp(group, o.generator(group), mont_array([x * pow(n, -1, R) for x in logs])))


# ---------------------------------------------------------------- 3. known discrete logs at n = 2^10
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("group", GROUPS)
def test_ecntt_known_discrete_logs(lsa, group, inverse):
    n = 1 << 10
    _, a = o.random_scalars(n, seed=31)
    a[:5] = [0, 1, R - 1, (R - 1) // 2, (R + 1) // 2]
    a[n - 1] = 0
    g = o.generator(group)
    pts = o.batch_exp(group, g, mont_array(a))
    want = o.batch_exp(group, g, o.fr_domain_transform(mont_array(a), o.fr_mont(omega(n)), inverse=inverse))
    got = run(lsa, group, pts, inverse, device=True)
    assert canon_all(group, got) == canon_all(group, want)


# ---------------------------------------------------------------- 4. the documented key flow at m = 2^8
def test_lipmaa_keys_from_a_powers_string(lsa):
    """INTEGRATION.md, "Lipmaa keys from a powers string (no trapdoor)": from chi^i G1 (i <= m) and gamma chi^i G2 alone to
    the key of InterpCommScheme, a commitment under it, and the pairing equation of InterpCommScheme::verify."""
    m = 1 << 8
    chi, gamma = 0x1F2E3D4C5B6A79880123456789ABCDEF % R, 0x0FEDCBA9876543210F1E2D3C4B5A6978 % R
    g1, g2 = o.generator("g1"), o.generator("g2")
    w = o.fr_mont(omega(m))
    # the ceremony's output, as a caller holds it: compressed points
    string1 = lsa.compress("g1", o.batch_exp("g1", g1, mont_array([pow(chi, i, R) for i in range(m + 1)])))
    string2 = lsa.compress("g2", o.batch_exp("g2", g2, mont_array([gamma * pow(chi, i, R) for i in range(m + 1)])))
    # 1. decompress and validate
    pw1, st1 = lsa.decompress("g1", *string1)
    pw2, st2 = lsa.decompress("g2", *string2, check_subgroup=True)
    assert not st1.any() and not st2.any()                     # PT_OK
    assert not lsa.validate_points("g1", pw1).any() and not lsa.validate_points("g2", pw2).any()
    # 2, 3. the Lagrange-basis keys
    lg1 = lsa.ecntt("g1", pw1[:m], w, inverse=True)
    gammalg2 = lsa.ecntt("g2", pw2[:m], w, inverse=True)
    lag = [o.limbs_to_int(x) * pow(o.MONT, -1, R) % R for x in lsa.fr_lagrange(8, None, w, o.fr_mont(chi))]
    assert canon_all("g1", lg1) == canon_all("g1", o.batch_exp("g1", g1, mont_array(lag)))
    assert canon_all("g2", gammalg2) == canon_all("g2", o.batch_exp("g2", g2, mont_array([gamma * x for x in lag])))
    # 4, 5. Z(chi) = chi^m - 1 in the exponent
    minus_one = o.fr_mont(R - 1)
    zg1 = o.g1_add(pw1[m], o.g1_mul(pw1[0], minus_one))
    gammazg2 = o.g2_add(pw2[m], o.g2_mul(pw2[0], minus_one))
    assert canon_all("g1", zg1) == canon_all("g1", o.batch_exp("g1", g1, mont_array([pow(chi, m, R) - 1])))
    # 6. resident bases; 7. commit: c = r zg1 + sum v_i lg1[i], kc = r gammazg2 + sum v_i gammalg2[i]
    import torch
    sc, _ = o.random_scalars(m + 1, seed=77)                   # v_0 .. v_(m-1), r
    d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
    b1 = lsa.Bases("g1", np.concatenate([lg1, zg1[None, :]]))
    b2 = lsa.Bases("g2", np.concatenate([gammalg2, gammazg2[None, :]]))
    c, kc = b1.msm(d_sc), b2.msm(d_sc)
    b1.close()
    b2.close()
    # InterpCommScheme::verify: e(c, gammazg2) == e(zg1, kc)
    neg_zg1 = o.g1_mul(zg1, minus_one)
    assert np.array_equal(lsa.pairing_product(np.stack([c, neg_zg1]), np.stack([gammazg2, kc])), o.fq12_one())
    # (and not for a commitment whose two halves disagree)
    assert not np.array_equal(lsa.pairing_product(np.stack([o.g1_add(c, g1), neg_zg1]), np.stack([gammazg2, kc])), o.fq12_one())


# ---------------------------------------------------------------- 5. the grid-stride wrap
@pytest.mark.parametrize("group", GROUPS)
def test_ecntt_grid_stride_wrap(lsa, group):
    """The smallest n whose stages have more butterflies (n/2) than the stage kernel's grid holds in one pass: 2^19 for G1
    (about 5 * 10^6 ladders) and 2^18 for G2 (2 * 10^6) at the figures of this build -- well under a second of device work
    each.  in[i] = a_i G, so out = batch_exp(G, transform of a); both sides are normalised on the device and compared as bytes."""
    import torch
    resident = lsa.ecntt_params()["%s_resident_butterflies" % group]
    n = 2
    while n // 2 <= resident:
        n *= 2
    assert n // 2 > resident and n // 4 <= resident
    rng = np.random.default_rng(19)
    a = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
    a[:, 3] &= np.uint64((1 << 60) - 1)                        # words below 2^252 < r: valid Montgomery words of some a_i
    g = o.generator(group)
    w = o.fr_mont(omega(n))
    d_a = torch.from_numpy(a.view(np.int64)).to("cuda:0")
    d_pts = lsa.batch_exp(group, g, d_a)
    d_out = lsa.ecntt(group, d_pts, w)
    d_want = lsa.batch_exp(group, g, lsa.fr_ntt(d_a.clone(), w))
    lsa.synchronize()
    got = lsa.normalize(group, d_out.cpu().numpy().view(np.uint64))
    want = lsa.normalize(group, d_want.cpu().numpy().view(np.uint64))
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- 6. random cases
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_ecntt_random_cases(lsa, seed):
    rng = random.Random(seed)
    for case in range(20):
        group = rng.choice(GROUPS)
        n = 1 << rng.randrange(6)
        inverse, device, in_place = rng.random() < 0.5, rng.random() < 0.5, rng.random() < 0.3
        pts = o.arith_bases(group, rng.randrange(1, R), rng.randrange(R), n)
        for i in range(n):
            if rng.random() < 0.15:
                pts[i] = 0
        pts = rescaled(group, pts, rng)
        got = run(lsa, group, pts, inverse, device, in_place)
        assert canon_all(group, got) == oracle_sums(group, pts, inverse), (seed, case, group, n, inverse, device, in_place)


# ---------------------------------------------------------------- 7. refusals, and points outside the subgroup
def test_ecntt_refusals(lsa):
    import torch
    L = lsa.lib()
    n = 8
    for group, fn in (("g1", L.lsa_g1_ecntt), ("g2", L.lsa_g2_ecntt)):
        pts = sample_input(group, n, 3)
        buf = np.concatenate([pts, pts])
        row = WIDTH[group] * 8
        w = o.fr_mont(omega(n))
        hp = lambda a, off=0: C.c_void_p(a.ctypes.data + off)  # noqa: E731
        before = buf.copy()
        out = np.zeros_like(pts)
        d = torch.from_numpy(buf.view(np.int64).copy()).to("cuda:0")
        bad = [
            fn(None, hp(out), 3, hp(w), 0, 0), fn(hp(pts), None, 3, hp(w), 0, 0), fn(hp(pts), hp(out), 3, None, 0, 0),
            fn(hp(pts), hp(out), 25, hp(w), 0, 0),
            fn(hp(buf), hp(buf, row), 3, hp(w), 0, 0), fn(hp(buf, 4 * row), hp(buf), 3, hp(w), 1, 0),     # partial overlaps
            fn(C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr() + row), 3, hp(w), 0, 1),
            fn(hp(pts), hp(out), 3, hp(o.fr_mont(omega(4))), 0, 0),                                        # order 4, not 8
            fn(hp(pts), hp(out), 3, hp(o.fr_mont(omega(16))), 0, 0),                                       # order 16
            fn(hp(pts), hp(out), 3, hp(o.fr_mont(1)), 0, 0), fn(hp(pts), hp(out), 3, hp(o.fr_mont(0)), 0, 0),
            fn(hp(pts), hp(out), 0, hp(o.fr_mont(R - 1)), 0, 0),                                           # one point: omega must be 1
        ]
        assert bad == [ERR_INVALID] * len(bad)
        assert np.array_equal(buf, before) and not out.any()
        lsa.synchronize()
        assert np.array_equal(d.cpu().numpy().view(np.uint64), before)
        # a wrapper-level refusal: a length that is no power of two
        with pytest.raises(ValueError):
            lsa.ecntt(group, pts[:6], w)
        # one point is copied
        assert np.array_equal(lsa.ecntt(group, pts[2:3], o.fr_mont(1)), pts[2:3])


def test_ecntt_outside_the_subgroup_returns(lsa):
    """Twist points outside G2: the twiddles compose mod r only on the subgroup, so the result is not a transform -- but every
    ladder returns the integer multiple, the call succeeds and every output is a point of the twist."""
    rng = random.Random(5)
    t = pio.outside_point()
    n = 8
    pts = np.stack([o.g2_from_affine(t, (rng.randrange(1, P), rng.randrange(P))) for _ in range(n)])
    pts[3] = o.generator("g2")
    pts[5] = 0
    for inverse in (False, True):
        out = lsa.ecntt("g2", pts, o.fr_mont(omega(n)), inverse=inverse)
        status = lsa.validate_points("g2", out, check_subgroup=False)
        assert all(s in (lsa.PT_OK, lsa.PT_INFINITY) for s in status), status
