// legosnark_amd/csrc/fq_sqrt.h -- square roots in Fq and Fq2 = Fq[u]/(u^2+1) and the G2 subgroup predicate of alt_bn128,
// shared by the point-loading kernels (point_load.hip) and the host (tests/cpp/test_fq_sqrt.cc, the shim).
//
// Every loop below has a compile-time trip count and a schedule fixed by constants (the exponent (p-3)/4, the NAF of
// 6u^2): lanes of a wavefront never disagree about it.  No barriers, no LDS, no cross-lane traffic.
//
// Square roots.  p = 3 mod 4, so a^((p+1)/4) is a root of a whenever a is a square.  The power actually computed is
//   w = a^((p-3)/4),   root = a w   (= a^((p+1)/4)),   a w^2 = a^((p-1)/2) = chi(a) in {0, 1, -1}:
// for a square, w = 1/root; for a non-square, t = a w has t^2 = -a and w = -1/t.  So the power yields the inverse of the
// candidate root for free, and fq2_sqrt below needs two powers and no inversion.
//
// Fq2 by the norm method (the branch structure of the shim's alt_bn128_Fq2::sqrt), a = a0 + a1 u:
//   a1 == 0:  (sqrt(a0), 0) if a0 is a square, else (0, sqrt(-a0)) -- and sqrt(-a0) is the same t = a0 w as above
//             ((p+1)/4 is even, p = 7 mod 8: (-a0)^((p+1)/4) = a0^((p+1)/4)).
//   a1 != 0:  sn = sqrt(a0^2 + a1^2) (no root: a is a non-square), d = (a0 + sn)/2, wd = d^((p-3)/4), t = d wd.
//             d != 0 because sn = -a0 would force a1 = 0.
//             t^2 ==  d:  root = (t, a1/(2t))  = (t, a1 wd / 2)
//             t^2 == -d:  d' = (a0 - sn)/2 satisfies d d' = -a1^2/4, so a1/(2t) squares to d': root = (a1/(2t), t) with
//                         1/t = -wd, i.e. (-a1 wd / 2, t).  No third power.
//   Either way the result is accepted iff root^2 == a.
//
// Subgroup.  psi(X, Y, Z) = (gamma_x conj X, gamma_y conj Y, conj Z) is the untwist-Frobenius-twist endomorphism of the twist
// E'(Fq2), valid on Jacobian coordinates (conjugation commutes with X/Z^2, Y/Z^3).  It satisfies psi^2 - t psi + p = 0 on all of
// E'(Fq2) (t the trace of E/Fq), and #E'(Fq2) = r c with c = 2p - r.  The test is  psi(P) == [6u^2]P,  6u^2 = t - 1:
//   sound:    psi(P) = [t-1]P gives [(t-1)^2 - t(t-1) + p]P = [p + 1 - t]P = [r]P = O, so P lies in the r-torsion of E'(Fq2),
//             which is exactly G2 because gcd(r, c) = 1 (the group has order r c, its r-part is cyclic of order r);
//   complete: on G2 psi acts as multiplication by an eigenvalue of X^2 - tX + p mod r, i.e. p = t - 1 or 1 (mod r), and it is
//             t - 1 (the generator is checked in smul_host.h's gls4_ok and in tests/cpp/test_fq_sqrt.cc).
// [6u^2]P is one chain of 127 doublings and 39 additions / subtractions of P (the NAF of the 127-bit constant has 40 non-zero
// digits), with the COMPLETE jac_add / jac_dbl of ec.h: the verdict is right for every point of the twist, small-order points
// whose chain runs through O or meets P + P / P - P included.
#pragma once
#include "ec.h"
#include "tower.h"

namespace lsa {

LSA_HD Fq fq_words(const uint32_t (&c)[8]) {
    Fq r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = c[i];
    return r;
}

// limb i of (p - 3) / 4   (p = ...47 hex: the subtraction does not borrow)
constexpr uint32_t fq_sqrt_exp_limb(int i) {
    return ((i == 0 ? LSA_P[0] - 3u : LSA_P[i]) >> 2) | (i < 7 ? LSA_P[i + 1] << 30 : 0u);
}
constexpr uint32_t fq_sqrt_exp_nibble(int i) { return (fq_sqrt_exp_limb(i >> 3) >> ((i & 7) * 4)) & 15u; }
static_assert(fq_sqrt_exp_nibble(63) == 0 && fq_sqrt_exp_nibble(62) == 0xc, "(p-3)/4 has 252 bits");

// a^((p-3)/4): fixed 4-bit windows over the constant exponent -- 14 products for a^2..a^15, then 62 x (4 squarings + at most
// one product); 248 squarings and 72 products, the same in every lane (0 -> 0).
LSA_HD_NOINLINE Fq fq_pow_p3d4(const Fq &a) {
    Fq tab[16];
    tab[0] = Fq::one();
    tab[1] = a;
#pragma unroll
    for (int i = 2; i < 16; i++) tab[i] = (i & 1) ? tab[i - 1] * a : tab[i >> 1].sqr();
    Fq acc = tab[fq_sqrt_exp_nibble(62)];
#pragma unroll
    for (int i = 61; i >= 0; --i) {
        acc = acc.sqr().sqr().sqr().sqr();
        if (fq_sqrt_exp_nibble(i) != 0) acc = acc * tab[fq_sqrt_exp_nibble(i)];
    }
    return acc;
}

// root = a^((p+1)/4); true iff root^2 == a.  *inv_root (optional) = a^((p-3)/4): 1/root for a square, -1/root otherwise.
LSA_HD bool fq_sqrt(const Fq &a, Fq *root, Fq *inv_root = nullptr) {
    const Fq w = fq_pow_p3d4(a);
    *root = a * w;
    if (inv_root) *inv_root = w;
    return root->sqr() == a;
}

LSA_HD bool fq2_sqrt(const Fq2 &a, Fq2 *root) {
    if (a.c1.is_zero()) {
        Fq t;
        const bool sq = fq_sqrt(a.c0, &t);                       // not a square: t^2 = -a0, (t u)^2 = a0
        *root = sq ? Fq2{t, Fq::zero()} : Fq2{Fq::zero(), t};
        return root->sqr() == a;
    }
    const Fq n = a.c0.sqr() + a.c1.sqr();
    Fq sn, t, wd;
    const bool norm_sq = fq_sqrt(n, &sn);
    const Fq half = fq_words(LSA_FQ_TWO_INV);
    const Fq d = (a.c0 + sn) * half;
    const bool first = fq_sqrt(d, &t, &wd);
    const Fq q = a.c1 * wd * half;                               // a1 / (2t) or its negative
    *root = first ? Fq2{t, q} : Fq2{q.neg(), t};
    return norm_sq && root->sqr() == a;
}

// NAF of 6u^2 = 0x6f4d8248eeb859fbf83e9682e87cfd46 (u = 4965661367192848881): 128 digits, 40 non-zero, the top one +1
static constexpr uint64_t LSA_PSI_NAF_POS[2] = {0x0040a08408810148ull, 0x8050024900008200ull};
static constexpr uint64_t LSA_PSI_NAF_NEG[2] = {0x08020a0120040402ull, 0x1102800011482804ull};

LSA_HD Jac<Fq2> g2_psi(const Jac<Fq2> &p) {
    return {fq2_const(LSA_TWIST_MUL_BY_Q_X) * p.X.conj(), fq2_const(LSA_TWIST_MUL_BY_Q_Y) * p.Y.conj(), p.Z.conj()};
}

// P on the twist (not checked here).  true iff P lies in G2 (O does).
LSA_HD bool g2_in_subgroup(const Jac<Fq2> &p) {
    if (p.is_inf()) return true;
    const Jac<Fq2> m = jac_neg(p);
    Jac<Fq2> acc = p;                                            // digit 127
    for (int i = 126; i >= 0; --i) {
        const uint64_t pos = i < 64 ? LSA_PSI_NAF_POS[0] : LSA_PSI_NAF_POS[1], neg = i < 64 ? LSA_PSI_NAF_NEG[0] : LSA_PSI_NAF_NEG[1];
        acc = jac_dbl(acc);
        if ((pos >> (i & 63)) & 1) acc = jac_add(acc, p);
        else if ((neg >> (i & 63)) & 1) acc = jac_add(acc, m);
    }
    return jac_eq(g2_psi(p), acc);
}

}  // namespace lsa
