// legosnark_amd/csrc/fr_dot.h -- one output's dot product sum_k a_k b_k over Fr on fr29.h's limbs: what every lane of the
// matrix kernels (fr_matrix.hip) runs per output, written so that the host compiles the same code (tests/cpp/test_fr_dot.cc).
//
// Form of the values (fr29.h's header comment; k_mle_dot / k_mle_finish in fr_vec.hip).  Operands are libff's words
// X = x 2^256 mod r read as limbs without conversion.  Up to FOUR schoolbook products share one Montgomery reduction
// (fr29_wide_mac / fr29_wide_reduce), which divides by 2^261: a reduced partial stands for (sum of <= 4 products) 2^251.
// The partials are added on limbs; ONE product by 2^266 mod r (fr_dot_up()) turns the sum into (sum) 2^256, libff's form
// again, and canonical2() brings it below r: the bytes of the reference's loop, whatever the order of summation.
//
// Bounds, every intermediate:
//   operand       any 256-bit word pattern (canonical inputs are < r; 2^256 - 1 < 5.3 r), limbs tight (< 2^29, top < 2^24);
//   column sums   4 products x 9 limb products x (2^29 - 1)^2 < 36 * 2^58, the reduction adds < 9 * 2^58 + a carry: < 2^64;
//   wide value    4 * (2^256 - 1)^2 < 112 r^2 < 121 r^2, fr29_wide_reduce's precondition, so a partial is < 2r, tight;
//   running sum   the sum of p partials is < 2 p r, carry-normalised by add() (the top limb takes the rest: 120 r < 2^261
//                 keeps it below 2^29).  A product mul(s, c) needs s * c < 121 r^2; the closing constant c = 2^266 mod r is
//                 < r, so s < 121 r: at most FR_DOT_MAX_PARTIALS = 60 partials (s < 120 r), that is 240 products;
//   longer sums   when a 61st partial arrives the running sum is first multiplied by Fr29::one() (2^261 mod r < r: the same
//                 value, back below 2r) and counts as ONE partial from then on: < 2r + 59 * 2r = 120 r again.  Any length.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fp.h"
#include "fr29.h"

namespace lsa {

constexpr unsigned FR_DOT_MAX_PARTIALS = 60;   // partials (< 2r each) a running sum may hold: 2 * 60 r < 121 r
constexpr unsigned FR_DOT_GROUP = 4;           // products per reduction (Fr29Wide)

// 2^266 mod r: the product by it closes a dot product (shifted form 2^251 -> libff's 2^256)
LSA_HD Fr29 fr_dot_up() {
    constexpr uint32_t C[9] = {0x0fffead7u, 0x1d5444f4u, 0x04438aa5u, 0x03b4d096u, 0x134c84dau,
                               0x0e92d304u, 0x14cb95b3u, 0x041b9d3du, 0x00058003u};
    Fr29 o;
#pragma unroll
    for (int i = 0; i < 9; i++) o.l[i] = C[i];
    return o;
}

struct FrDot {
    Fr29 sum;            // < 2 * partials * r, tight
    uint32_t partials;   // <= FR_DOT_MAX_PARTIALS
};
LSA_HD FrDot fr_dot_zero() {
    FrDot d;
    d.sum = Fr29::zero();
    d.partials = 0;
    return d;
}
// d += the <= 4 products gathered in w (w < 121 r^2 in value)
LSA_HD void fr_dot_push(FrDot &d, const Fr29Wide &w) {
    if (d.partials == FR_DOT_MAX_PARTIALS) {               // < 120 r  ->  < 2r, the same residue
        d.sum = mul(d.sum, Fr29::one());
        d.partials = 1;
    }
    d.sum = add(d.sum, fr29_wide_reduce(w));               // < 2 (partials + 1) r <= 120 r
    d.partials++;
}
// d += sum_{j < n} a[j] b[j], n <= FR_DOT_GROUP operands in limbs: ONE reduction.  The one place products are gathered and
// pushed: the matrix kernels call it with the operands of a group in registers, the two routines below with gathered ones.
LSA_HD void fr_dot_group(FrDot &d, const Fr29 *a, const Fr29 *b, unsigned n) {
    Fr29Wide w = fr29_wide_zero();
#pragma unroll
    for (unsigned j = 0; j < FR_DOT_GROUP; j++)
        if (j < n) fr29_wide_mac(w, a[j], b[j]);
    fr_dot_push(d, w);
}
// d += sum_{k < n} a[k * sa] * b[k * sb], operands already in limbs; groups of four, the last one shorter
LSA_HD void fr_dot_span(FrDot &d, const Fr29 *a, size_t sa, const Fr29 *b, size_t sb, size_t n) {
    for (size_t k = 0; k < n; k += FR_DOT_GROUP) {
        const unsigned m = n - k < FR_DOT_GROUP ? (unsigned)(n - k) : FR_DOT_GROUP;
        Fr29 ga[FR_DOT_GROUP], gb[FR_DOT_GROUP];
        for (unsigned j = 0; j < m; j++) { ga[j] = a[(k + j) * sa]; gb[j] = b[(k + j) * sb]; }
        fr_dot_group(d, ga, gb, m);
    }
}
// the value as libff's canonical words: (sum 2^251) * 2^266 / 2^261 = sum 2^256.  sum < 120 r, the constant < r.
LSA_HD Fr fr_dot_finish(const FrDot &d) { return mul(d.sum, fr_dot_up()).canonical2().to_words(); }

// the whole thing on words: out = sum_{k < n} a[k * sa] * b[k * sb]  (n = 0: zero)
LSA_HD Fr fr_dot_words(const Fr *a, size_t sa, const Fr *b, size_t sb, size_t n) {
    FrDot d = fr_dot_zero();
    for (size_t k = 0; k < n; k += FR_DOT_GROUP) {
        const unsigned m = n - k < FR_DOT_GROUP ? (unsigned)(n - k) : FR_DOT_GROUP;
        Fr29 ga[FR_DOT_GROUP], gb[FR_DOT_GROUP];
        for (unsigned j = 0; j < m; j++) { ga[j] = Fr29::from_words(a[(k + j) * sa]); gb[j] = Fr29::from_words(b[(k + j) * sb]); }
        fr_dot_group(d, ga, gb, m);
    }
    return fr_dot_finish(d);
}

}  // namespace lsa
