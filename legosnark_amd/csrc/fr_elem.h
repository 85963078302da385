// legosnark_amd/csrc/fr_elem.h -- the per-element and per-run arithmetic of the Fr vector calls (lsa_fr_vec_mul,
// lsa_fr_vec_lincomb, lsa_fr_powers, lsa_fr_batch_inverse, lsa_fr_poly_eval; kernels: fr_elem.hip), written so that the host
// compiles the same code (tests/cpp/test_fr_elem.cc).
//
// Form of the values (fr29.h's header comment).  A vector element is libff's words X = x 2^256 mod r, read as limbs without
// conversion; ANY 256-bit pattern is accepted and counts as its value mod r (X <= 2^256 - 1 < 5.3 r, limbs tight: < 2^29,
// the top limb < 2^24).  A Montgomery product on the limbs divides by 2^261, so a constant that is to multiply an element and
// leave libff's form behind is held as c 2^261 mod r ("form 2^261": the words of c * 32), and the constant that closes a product
// of TWO elements (X Y / 2^261 = x y 2^251) as c 2^266 ("form 2^266": the words of c * 1024).  The one-element arguments of
// the calls (scale, coeffs, base, first, x) are host values: the entry points bring them below r (fr_elem_canon) and into
// these forms once per call (fr_elem_c261, fr_elem_c266), so every constant a kernel sees is canonical.  No element of a
// vector is canonicalised on load except by lsa_fr_batch_inverse, whose zero test and prefix chain (fp.h's operators: operands
// below r) need the canonical value: one product by 2^261 mod r per element.
//
// Bounds, every intermediate (mul(a, b) needs a * b < 121 r^2 and tight limbs, and returns a tight value < 2r):
//   canon        X * (2^261 mod r) < 5.3 r^2;  the product is X mod r below 2r, canonical2() below r;
//   vec_mul      X Y < 28.1 r^2;  the product (< 2r) times the closing constant (< r) < 2 r^2;
//   lincomb      a group of FR_DOT_GROUP = 4 products element x constant shares one reduction (fr_dot.h): the column sums
//                are fr29.h's four-product bound, the value 4 * 5.3 r * r < 22 r^2;  each group's partial is made canonical
//                (< r), and the two partials of k > 4 add up below 2r: canonical2() once more;
//   powers       the running power stays below 2r: (< 2r)(base < r) < 2 r^2;  fr29_pow_u64 squares values < 2r: < 4 r^2;
//   horner       acc < 2r + X < 7.3 r after every step, times x (< r) < 7.3 r^2;  the closing product by the offset power
//                (< 2r) < 14.6 r^2;
//   sums         reduced values (< 2r) are added up as fr_dot.h adds its partials: at most FR_DOT_MAX_PARTIALS = 60 before a
//                product by 2^261 mod r brings the running sum back below 2r (fr_elem_sum_push).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fp.h"
#include "fr29.h"
#include "fr_batch_inv.h"
#include "fr_dot.h"

namespace lsa {

constexpr unsigned FR_VEC_LINCOMB_MAX = 8;             // vectors per lsa_fr_vec_lincomb call: two groups of FR_DOT_GROUP
static_assert(FR_VEC_LINCOMB_MAX == 2 * FR_DOT_GROUP, "fr_elem_lincomb_point adds exactly two partials");
// elements per lane of lsa_fr_batch_inverse and lsa_fr_powers: the run of fr_batch_inv.h (its measurements: 16 leaves
// 2^16 lanes at n = 2^20 and pays one inversion, or one starting power, per 16 elements)
#ifndef FR_ELEM_INV_RUN
#define FR_ELEM_INV_RUN 16
#endif
#ifndef FR_ELEM_POWERS_RUN
#define FR_ELEM_POWERS_RUN 16
#endif
// coefficients per lane of lsa_fr_poly_eval
#ifndef FR_ELEM_EVAL_ITEMS
#define FR_ELEM_EVAL_ITEMS 16
#endif
static_assert(FR_ELEM_INV_RUN >= 1 && FR_ELEM_INV_RUN <= 32, "the zero mask of a run is one 32-bit word");

// any 256-bit word pattern -> the canonical words of its value mod r
LSA_HD Fr fr_elem_canon(const Fr &x) { return mul(Fr29::from_words(x), Fr29::one()).canonical2().to_words(); }
// a host scalar s (any pattern) as the words of s 2^261 / of s 2^266 (s == nullptr: one); canonical
LSA_HD Fr fr_elem_c261(const Fr &s) { return fr_elem_canon(s) * Fr::from_u32(32); }
LSA_HD Fr fr_elem_c266(const Fr *s) { return (s ? fr_elem_canon(*s) : Fr::one()) * Fr::from_u32(1024); }

// base^e for base in form 2^261 (canonical or < 2r), in form 2^261 and below 2r; e == 0: one, also for base zero
LSA_HD Fr29 fr29_pow_u64(const Fr29 &base261, uint64_t e) {
    Fr29 acc = Fr29::one(), b = base261;
    while (e) {
        if (e & 1) acc = mul(acc, b);
        e >>= 1;
        if (e) b = mul(b, b);
    }
    return acc;
}

// ---- lsa_fr_vec_mul: scale * a * b as canonical words; c266 = the scale in form 2^266
LSA_HD Fr fr_elem_mul_point(const Fr29 &a, const Fr29 &b, const Fr29 &c266) { return mul(mul(a, b), c266).canonical2().to_words(); }

// ---- lsa_fr_vec_lincomb: sum_{t < k} c[t] x[t] as canonical words, 1 <= k <= FR_VEC_LINCOMB_MAX; c261: the coefficients in form
// 2^261.  One reduction per FR_DOT_GROUP products.  (k is a compile-time constant in the kernels: the tests below fold.)
LSA_HD Fr fr_elem_lincomb_point(const Fr29 *x, const Fr29 *c261, unsigned k) {
    if (k == 1) return mul(x[0], c261[0]).canonical2().to_words();       // one product: no column accumulators to hold
    Fr29 part[2] = {Fr29::zero(), Fr29::zero()};
#pragma unroll
    for (unsigned g = 0; g < 2; g++) {
        if (g * FR_DOT_GROUP < k) {
            Fr29Wide w = fr29_wide_zero();
#pragma unroll
            for (unsigned j = 0; j < FR_DOT_GROUP; j++)
                if (g * FR_DOT_GROUP + j < k) fr29_wide_mac(w, x[g * FR_DOT_GROUP + j], c261[g * FR_DOT_GROUP + j]);
            part[g] = fr29_wide_reduce(w).canonical2();
        }
    }
    if (k <= FR_DOT_GROUP) return part[0].to_words();
    return add(part[0], part[1]).canonical2().to_words();
}

// ---- lsa_fr_powers: out[j] = first * base^(lo + j), j < len, as canonical words.  base261: the base in form 2^261; first:
// canonical words read as limbs.  One product per element after the starting power; nothing is read from out.
LSA_HD void fr_elem_powers_run(const Fr29 &base261, const Fr29 &first, uint64_t lo, unsigned len, Fr *out) {
    Fr29 cur = mul(first, fr29_pow_u64(base261, lo));
    for (unsigned j = 0; j < len; j++) {
        out[j] = cur.canonical2().to_words();
        cur = mul(cur, base261);
    }
}

// ---- lsa_fr_batch_inverse: out[j] = 1 / x[j], j < len <= FR_ELEM_INV_RUN; an element that is 0 mod r (whatever its words) is
// replaced by one in the prefix chain of fr_batch_inv_run and gives 0.  Returns the number of such elements.  Every x[j] is
// read before any out[j] is written: out may be x.
LSA_HD unsigned fr_elem_inv_run(const Fr *x, Fr *out, unsigned len) {
    Fr v[FR_ELEM_INV_RUN], pre[FR_ELEM_INV_RUN];
    uint32_t zmask = 0;
    unsigned zeros = 0;
    for (unsigned j = 0; j < len; j++) {
        Fr c = fr_elem_canon(x[j]);
        if (c.is_zero()) { zmask |= 1u << j; zeros++; c = Fr::one(); }
        v[j] = c;
    }
    fr_batch_inv_run(v, pre, len);
    for (unsigned j = 0; j < len; j++) out[j] = ((zmask >> j) & 1u) ? Fr::zero() : v[j];
    return zeros;
}

// ---- lsa_fr_poly_eval: (sum_{j < len} c[j] x^j) * x^lo in libff's form, below 2r, tight; x261: x in form 2^261, xlo261: the
// offset power x^lo in form 2^261 (< 2r).  Horner's rule from the top coefficient down.  len == 0: zero.
LSA_HD Fr29 fr_elem_horner_run(const Fr *c, unsigned len, const Fr29 &x261, const Fr29 &xlo261) {
    if (len == 0) return Fr29::zero();
    Fr29 acc = Fr29::from_words(c[len - 1]);
    for (unsigned j = len - 1; j-- > 0;) acc = add(mul(acc, x261), Fr29::from_words(c[j]));
    return mul(acc, xlo261);
}

// the constants of a call for a canonical point x, `items` coefficients per lane and `lanes` lanes per workgroup: x and
// x^items in form 2^261, and the words of x^(items * lanes), the factor between neighbouring workgroups' offsets
struct FrEvalConsts { Fr x261, xi261, xb; };
LSA_HD FrEvalConsts fr_elem_eval_consts(const Fr &x, unsigned items, unsigned lanes) {
    const Fr xi = fr_pow_u64(x, items), up5 = Fr::from_u32(32);
    return {x * up5, xi * up5, fr_pow_u64(xi, lanes)};
}

// a running sum of reduced values (< 2r each, libff's form), any number of them: FrDot's bookkeeping without its products
LSA_HD void fr_elem_sum_push(FrDot &d, const Fr29 &p) {
    if (d.partials == FR_DOT_MAX_PARTIALS) {               // < 120 r  ->  < 2r, the same residue
        d.sum = mul(d.sum, Fr29::one());
        d.partials = 1;
    }
    d.sum = add(d.sum, p);
    d.partials++;
}
// the sum as canonical words: sum < 120 r times 2^261 mod r < r
LSA_HD Fr fr_elem_sum_finish(const FrDot &d) { return mul(d.sum, Fr29::one()).canonical2().to_words(); }

}  // namespace lsa
