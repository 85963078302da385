// tests/cpp/test_fq_sqrt.cc -- host compilation of csrc/fq_sqrt.h: fq_sqrt / fq2_sqrt against Euler's criterion and
// root^2 == a, g2_in_subgroup against [r]P == O by plain double-and-add, on the operand list of fq_sqrt_cases.h.
#include "fq_sqrt_cases.h"

using namespace lsa;
using namespace fqcases;

int main() {
    const Cases c = build(3000);
    size_t fq_sq = 0, fq_non = 0, fq2_sq = 0, fq2_non = 0, fq2_a1zero_res = 0, fq2_a1zero_non = 0;
    for (const Fq &a : c.fq) {
        Fq root, w;
        const bool got = fq_sqrt(a, &root, &w);
        FQC_REQUIRE(got == fq_is_square(a));
        if (got) {
            FQC_REQUIRE(root.sqr() == a);
            if (!a.is_zero()) FQC_REQUIRE(root * w == Fq::one());
            fq_sq++;
        } else {
            FQC_REQUIRE(root.sqr() == a.neg());                   // the candidate is a root of -a, and w its negated inverse
            FQC_REQUIRE(root * w == Fq::one().neg());
            fq_non++;
        }
    }
    // the three values the issue names
    { Fq r; FQC_REQUIRE(fq_sqrt(Fq::zero(), &r) && r.is_zero()); }
    { Fq r; FQC_REQUIRE(fq_sqrt(Fq::one(), &r) && r.sqr() == Fq::one()); }
    { Fq r; FQC_REQUIRE(!fq_sqrt(Fq::zero() - Fq::one(), &r)); }
    { Fq r; FQC_REQUIRE(!fq_sqrt(Fq::from_u32(3), &r)); }         // x = 0 is not the abscissa of a G1 point
    for (const Fq2 &a : c.fq2) {
        Fq2 root;
        const bool got = fq2_sqrt(a, &root);
        const bool want = a.is_zero() || fq2_is_square(a);
        FQC_REQUIRE(got == want);
        if (got) {
            FQC_REQUIRE(root.sqr() == a);
            fq2_sq++;
            if (a.c1.is_zero() && !a.is_zero()) {
                if (fq_is_square(a.c0)) { FQC_REQUIRE(root.c1.is_zero()); fq2_a1zero_res++; }
                else {                                            // (0, (-a0)^((p+1)/4)): what the shim's operator>> returns
                    uint32_t e[8];                                // (p + 1) / 4
                    for (int i = 0; i < 8; i++) e[i] = ((i == 0 ? LSA_P[0] + 1u : LSA_P[i]) >> 2) | (i < 7 ? LSA_P[i + 1] << 30 : 0u);
                    FQC_REQUIRE(root.c0.is_zero() && root.c1 == fq_pow(a.c0.neg(), e));
                    fq2_a1zero_non++;
                }
            }
        } else fq2_non++;
    }
    FQC_REQUIRE(fq_sq > 1000 && fq_non > 1000 && fq2_sq > 1500 && fq2_non > 500);
    FQC_REQUIRE(fq2_a1zero_res >= 8 && fq2_a1zero_non >= 8);
    FQC_REQUIRE(c.fq2_second > 300);                              // elements that take the second candidate of x0
    size_t in = 0, out = 0;
    for (size_t i = 0; i < c.pts.size(); i++) {
        const bool want = g2_ladder(c.pts[i], ORDER_R).is_inf();
        const bool got = g2_in_subgroup(c.pts[i]);
        if (got != want) { printf("FAIL: point %zu: g2_in_subgroup %d, [r]P == O %d\n", i, (int)got, (int)want); return 1; }
        (want ? in : out)++;
    }
    // expected split of the list: O, 5 multiples of G, 4 x [c]T, and their rescaled copies lie in G2; 4 T, 4 small-order, 3 sums do not
    FQC_REQUIRE(in == 2 * (1 + 5 + 4) && out == 2 * (4 + 4 + 3));
    printf("fq %zu squares %zu non-squares; fq2 %zu / %zu (%zu second candidate, a1 = 0: %zu / %zu); points %zu in G2, %zu outside\n", fq_sq, fq_non, fq2_sq,
           fq2_non, c.fq2_second, fq2_a1zero_res, fq2_a1zero_non, in, out);
    printf("PASS\n");
    return 0;
}
