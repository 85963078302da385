// legosnark_amd/csrc/fr_sparse.h -- one output of a sparse Fr matrix-vector product, y = sum_e val[e] * x[idx[e]] over the
// entries e of a row (or of a slice of one): what every lane of fr_sparse.hip runs, written so that the host compiles the
// same code (tests/cpp/test_fr_sparse.cc).
//
// Two accumulators.  Constraint systems from gadget libraries hold almost only the coefficients +1 and -1, and a limb
// addition costs about a tenth of a product, so every stored coefficient carries a class (fr_sparse_class, decided once
// when the matrix is created):
//   general   the product goes through fr_dot.h: up to four schoolbook products share one Montgomery reduction
//             (Fr29Wide), the reduced partials are summed in an FrDot.  A partial stands for (sum of products) 2^251;
//   +1 / -1   the coefficient is not read at all: the operand's words X = x 2^256 mod r are added to, or subtracted from,
//             a second running sum `unit` that stands for (sum of +-x) 2^256.
// The two are joined ONCE per FR_SPARSE_UNIT_MAX unit terms and at the end: mul(unit, 2^256 mod r) divides by 2^261, that
// is (sum) 2^256 2^-5 = (sum) 2^251, a value < 2r that enters the FrDot as one more partial.  fr_dot_finish closes as for
// the dense kernels: canonical words (< r), so the bytes do not depend on the order of summation.
//
// A coefficient is a unit only when its words are EXACTLY the canonical ones of +1 (2^256 mod r) or of -1 (r minus that);
// any other pattern, a non-canonical spelling of 1 included, is general and counts as its value mod r, as every operand does.
//
// Bounds, every intermediate:
//   operand       x[idx] is any 256-bit word pattern: X <= 2^256 - 1 < 5.3 r < 6r, limbs tight (< 2^29, top < 2^24);
//   general       fr_dot.h's: four products of such operands are < 112 r^2 < 121 r^2, a partial is < 2r, the FrDot holds
//                 at most FR_DOT_MAX_PARTIALS of them (< 120 r) and folds itself back to one partial when full;
//   unit, +       unit + X grows by less than 5.3 r, carry-normalised by add();
//   unit, -       unit - X + 6r (fr29_sub6r): 6r > 2^256 > X keeps the value non-negative whatever unit >= 0 is, and it
//                 grows by at most 6r; signed carries, every limb difference fits an int32 (|.| < 2^30);
//   unit sum      after t unit terms unit <= 6 t r.  FR_SPARSE_UNIT_MAX = 20 terms: unit <= 120 r < 2^261 (the top limb stays
//                 below 2^29) and unit * (2^256 mod r) < 120 r * r < 121 r^2, mul()'s precondition.  When a 21st unit term
//                 arrives the sum is first brought down: joined into the FrDot as above, and unit starts again at zero;
//   joined        the partial mul(unit, 2^256 mod r) is < 2r, tight: pushed exactly as fr_dot_push pushes a reduced group
//                 (the FrDot is folded first when it already holds FR_DOT_MAX_PARTIALS), so sum < 120 r holds throughout;
//   result        fr_dot_finish: sum < 120 r times 2^266 mod r < r, below 121 r^2; canonical2() of a value < 2r.  A row without
//                 general entries skips the join: unit <= 120 r times 2^261 mod r < r is below 121 r^2 and the product is
//                 unit 2^261 / 2^261, the sum in form 2^256, < 2r; canonical2() as before.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fp.h"
#include "fr29.h"
#include "fr_dot.h"

namespace lsa {

constexpr unsigned FR_SPARSE_UNIT_MAX = 20;    // unit terms (<= 6r each) the second accumulator takes before it is joined: 6 * 20 r < 121 r

constexpr uint8_t FR_SPARSE_GENERAL = 0, FR_SPARSE_PLUS = 1, FR_SPARSE_MINUS = 2;

// the class of a stored coefficient: a unit only for the exact canonical words of +1 or -1
LSA_HD uint8_t fr_sparse_class(const Fr &v) {
    const Fr one = Fr::one();
    if (v == one) return FR_SPARSE_PLUS;
    if (v == Fr::zero() - one) return FR_SPARSE_MINUS;
    return FR_SPARSE_GENERAL;
}

// 2^256 mod r: the product by it takes the unit sum (form 2^256) to the partials' form 2^251
LSA_HD Fr29 fr_sparse_down() {
    constexpr uint32_t C[9] = {0x0ffffffbu, 0x04b1a0e2u, 0x18334a6bu, 0x18ed2b3eu, 0x1462e36fu,
                               0x11b7bc3cu, 0x1cbd99bau, 0x183340fbu, 0x000e0a77u};
    Fr29 o;
#pragma unroll
    for (int i = 0; i < 9; i++) o.l[i] = C[i];
    return o;
}

// a - b + 6r for b < 6r (any 256-bit pattern is), carry-normalised.  [a + 6r; tight]
LSA_HD Fr29 fr29_sub6r(const Fr29 &a, const Fr29 &b) {
    Fr29 o;
    int32_t c = 0;
    uint32_t rc = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        rc += Fr29::r(i) * 6u;
        const uint32_t rl = (i < 8) ? (rc & Fr29::MASK) : rc;
        rc >>= 29;
        const int32_t v = (int32_t)a.l[i] - (int32_t)b.l[i] + (int32_t)rl + c;
        if (i < 8) { o.l[i] = (uint32_t)v & Fr29::MASK; c = v >> 29; }
        else o.l[i] = (uint32_t)v;
    }
    return o;
}

struct FrSparseAcc {
    FrDot d;             // general products and joined unit sums, form 2^251
    Fr29Wide w;          // the open group: pending <= FR_DOT_GROUP products
    uint32_t pending;
    Fr29 unit;           // <= 6 * units * r, tight; form 2^256
    uint32_t units;      // <= FR_SPARSE_UNIT_MAX
};
LSA_HD FrSparseAcc fr_sparse_zero() {
    FrSparseAcc a;
    a.d = fr_dot_zero();
    a.w = fr29_wide_zero();
    a.pending = 0;
    a.unit = Fr29::zero();
    a.units = 0;
    return a;
}
// d += p for a reduced p < 2r: fr_dot_push after its reduction
LSA_HD void fr_sparse_push_reduced(FrDot &d, const Fr29 &p) {
    if (d.partials == FR_DOT_MAX_PARTIALS) {
        d.sum = mul(d.sum, Fr29::one());
        d.partials = 1;
    }
    d.sum = add(d.sum, p);
    d.partials++;
}
// the unit sum into the FrDot; the second accumulator starts again
LSA_HD void fr_sparse_join(FrSparseAcc &a) {
    fr_sparse_push_reduced(a.d, mul(a.unit, fr_sparse_down()));
    a.unit = Fr29::zero();
    a.units = 0;
}
// a += (+-1) * x
LSA_HD void fr_sparse_add_unit(FrSparseAcc &a, bool minus, const Fr29 &x) {
    if (a.units == FR_SPARSE_UNIT_MAX) fr_sparse_join(a);
    a.unit = minus ? fr29_sub6r(a.unit, x) : add(a.unit, x);
    a.units++;
}
// a += v * x
LSA_HD void fr_sparse_add_general(FrSparseAcc &a, const Fr29 &v, const Fr29 &x) {
    fr29_wide_mac(a.w, v, x);
    if (++a.pending == FR_DOT_GROUP) {
        fr_dot_push(a.d, a.w);
        a.w = fr29_wide_zero();
        a.pending = 0;
    }
}
// the value as libff's canonical words
LSA_HD Fr fr_sparse_finish(FrSparseAcc &a) {
    // units alone (most rows of a gadget library's system): unit <= 120 r is already in libff's form 2^256, ONE product by
    // 2^261 mod r (the same residue, < 2r) instead of the join and the closing product
    if (a.pending == 0 && a.d.partials == 0) return mul(a.unit, Fr29::one()).canonical2().to_words();
    if (a.pending) { fr_dot_push(a.d, a.w); a.pending = 0; }
    if (a.units) fr_sparse_join(a);
    return fr_dot_finish(a.d);
}

struct FrSparseLoadPlain {
    LSA_HD Fr operator()(const Fr *p) const { return *p; }
};

// out = sum over e = lo, lo + stride, ... < hi of vals[e] * x[idx[e]].  cls[e] is fr_sparse_class(vals[e]); vals[e] is read
// only where it is general.  Every idx[e] must be a valid index into x (the creator of the matrix checks it).  load(p): the 32
// bytes at p.  No entries: zero.
template <class Load>
LSA_HD Fr fr_sparse_row(const Fr *vals, const uint8_t *cls, const uint32_t *idx, const Fr *x, size_t lo, size_t hi, size_t stride, Load load) {
    FrSparseAcc a = fr_sparse_zero();
    for (size_t e = lo; e < hi; e += stride) {
        const uint8_t k = cls[e];
        const Fr29 xe = Fr29::from_words(load(x + idx[e]));
        if (k == FR_SPARSE_GENERAL) fr_sparse_add_general(a, Fr29::from_words(load(vals + e)), xe);
        else fr_sparse_add_unit(a, k == FR_SPARSE_MINUS, xe);
    }
    return fr_sparse_finish(a);
}

}  // namespace lsa
