// legosnark_amd/csrc/smul_g2.h -- one variable-base scalar multiplication k*P on the twist of alt_bn128 (G2 and every
// other point of E'(Fq2)) with a signed 4-bit window over the WHOLE scalar: the per-item body of k_smul_g2
// (scalar_mul_g2.hip), kept in a header, templated on the Fq2 representation E like the point formulas of fp29x2.h, so
// that the host tests (tests/cpp/test_smul_g2.cc) run the very same code with E = F29x2.
//
// No endomorphism split.  The GLV map (beta x, y), the untwist-Frobenius-twist map psi and the four-dimensional
// Galbraith-Scott decomposition of smul_host.h all act as multiplication by a scalar on the order-r subgroup ONLY; the
// twist has order r (2p - r), the library takes twist points in without a subgroup check (lsa_g2_validate is a separate
// call), and this ladder returns the integer multiple [s]P for every point of the twist.  What that costs, in Fq2
// products (9 per doubling, 14 per general addition, 2 per psi applied to a table entry):
//   this ladder          63*4*9 + 64*14 + table (9 + 6*12 = 81)           ~ 3.2 * 10^3
//   four 66-bit parts    17*4*9 + 4*17*(14 + 2)*15/16 + table             ~ 1.7 .. 1.8 * 10^3   (a factor of about 1.7 .. 1.9)
// The split can come later behind a caller-asserted "these points are in G2" flag.
#pragma once
#include "fp29x2.h"

namespace lsa {

static constexpr int SMUL_G2_WINDOW = 4;                   // bits per signed digit
static constexpr int SMUL_G2_TBL = 8;                      // table entries 1P .. 8P
static constexpr int SMUL_G2_DIGITS = 64;                  // ceil(256 / 4); the scalar is < r < 2^254

// Signed 4-bit digits of s < r without a carry chain between digits: with s' = s + 0x0888..8 (an 8 in every nibble but
// the top one; r < 2^254, so s' < 2^255 and nothing leaves the eighth word), digit_j = nibble_j(s') - 8 in [-8, 7] for
// j < 63, digit_63 = nibble_63(s') in [0, 4] (nibble_63(s) <= 3 plus at most one carry), and sum digit_j 16^j = s.
LSA_HD void recode_nibbles_256(const uint32_t s[8], uint32_t out[8]) {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)s[i] + (i == 7 ? 0x08888888u : 0x88888888u);
        out[i] = (uint32_t)c;
        c >>= 32;
    }
}
// digit j (0 = least significant) of a recoding made by recode_nibbles_256
LSA_HD int smul_g2_digit(const uint32_t dg[8], int j) {
    return (int)((dg[j >> 3] >> ((j & 7) * 4)) & 15u) - (j == SMUL_G2_DIGITS - 1 ? 0 : 8);
}

// [s]P for the canonical scalar s (< r) and an affine point P of the twist (canonical coordinates; x = y = 0: infinity).
// T: SMUL_G2_TBL entries of scratch owned by the caller, in memory (a table indexed by a run-time digit must not be a
// per-lane array: it would go to scratch).
//
// Operand bounds, per Fq component in multiples of p.  Every value that reaches g2_add / g2_dbl below is
//   - a table entry: T[0] = (x, y, 1, 1) with x, y canonical [< 1] and one() [< 1]; T[1] from g2_dbl_affine,
//     T[2..7] from g2_madd: X < 4, Y < 4, ZZ < 2, ZZZ < 2, tight (the accumulator invariants of fp29x2.h);
//   - the accumulator: infinity, a (possibly negated) table entry, or the result of g2_dbl / g2_add: the same invariants,
//     with Y <= 4 instead of < 4 after a negation (below);
// g2_add needs X, Y as the left factor of mul<2> (2 * A * 2 < 169: A <= 4 gives 16) and ZZ, ZZZ < 2 as the right one; g2_dbl
// needs 2Y <= 8 into condsub4 (8p maps to 4p), U <= 4 into sqr<4> ((2*4)^2 = 64 < 169) and Y <= 4 as the right factor of
// mul<4> (4p - Y.c1 >= 0).  All met with room.
template <class E>
LSA_HD XyzzE<E> smul_g2(const AffE<E> &P, const uint32_t s[8], XyzzE<E> *T) {
    uint32_t any = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) any |= s[w];
    if (P.is_inf() || any == 0) return XyzzE<E>::inf();
    uint32_t dg[8];
    recode_nibbles_256(s, dg);
    // table d*P, d = 1..8
    XyzzE<E> t = {P.x, P.y, E::one(), E::one()};                       // [<1, <1, <1, <1; tight]
    T[0] = t;
    t = g2_dbl_affine(P);                                              // [<4, <4, <2, <2; tight]
    T[1] = t;
#pragma unroll 1
    for (int d = 2; d < SMUL_G2_TBL; d++) {
        t = g2_madd(t, P);                                             // complete: P of order 2..8 is handled   [<4, <4, <2, <2]
        T[d] = t;
    }
    XyzzE<E> acc = XyzzE<E>::inf();
#pragma unroll 1
    for (int j = SMUL_G2_DIGITS - 1; j >= 0; --j) {
        if (j != SMUL_G2_DIGITS - 1) {
#pragma unroll 1
            for (int r = 0; r < SMUL_G2_WINDOW; r++) acc = g2_dbl(acc);    // Y <= 4 in, [<4, <4, <2, <2] out
        }
        const int d = smul_g2_digit(dg, j);
        if (d == 0) continue;
        XyzzE<E> q = T[(d < 0 ? -d : d) - 1];
        // -Y as 4p - Y: Y < 4 gives (0, 4p], tight (4p itself only for a component whose limbs are all zero)   [<= 4; tight]
        if (d < 0) q.Y = sub_k<4>(E::zero(), q.Y);
        acc = g2_add(acc, q);                                          // complete: doubling, cancellation, either side infinite
    }
    return acc;
}

}  // namespace lsa
