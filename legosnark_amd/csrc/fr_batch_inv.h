// legosnark_amd/csrc/fr_batch_inv.h -- run-wise batch inversion over Fr and the rows built on it (fr_poly.hip), written so
// that the host compiles the same code (tests/cpp/test_fr_batch_inv.cc).
//
// A vector of m values is inverted in runs of FR_BATCH_INV_RUN consecutive elements, one run per lane: prefix products
// forward, ONE Fr::inverse() (Fermat on the device: ~380 products), peel backward -- three products per element and the
// inversion shared by the run.  No chain crosses a run: m = 2^20 is 2^16 independent lanes.
//
// Every row fr_poly.hip needs has the shape
//     out[i] = k [w^i] / ((t - w^i) (a v^i - c)),      either factor of the denominator optional,
// (the Lagrange coefficients of a radix-2 domain: k w^i / (t - w^i); those of the big part of a step domain: the same times
// the other part's vanishing factor 1 / (x_i^small - omega^small); the inverse values of Z on a coset of the step domain:
// k / (g^small v^i - omega^small)), so one routine generates a run's denominators from two geometric sequences, inverts
// them and applies the numerators: fr_geom_row_run.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fp.h"
#include "fr29.h"

namespace lsa {

// elements per lane.  One lane's cost is ~100 products for its two starting powers + 380 for the inversion + 7 per element,
// so a short run pays more inversions and a long one leaves too few lanes for the chip (m = 2^20: a run of 16 is 1024
// wavefronts).  Measured on an MI355X, lsa_fr_lagrange, median of 21 (profiles/lipmaa_quotient.txt):
//     m = 2^20:         run 8: 0.82 ms   run 16: 0.63-0.65 ms   run 32: 0.75 ms
//     m = 2^20 + 2^19:  run 8: 1.34 ms   run 16: 1.27 ms        run 32: 1.57 ms
// (-DFR_BATCH_INV_RUN=n builds another length.)  The prefix products live in a per-lane array indexed by a run-time
// length (576 B of scratch per lane in k_fr_geom_row) and the denominators pass through out[]: the figures above are for
// that code.
#ifndef FR_BATCH_INV_RUN
#define FR_BATCH_INV_RUN 16
#endif

LSA_HD Fr fr_pow_u64(const Fr &base, uint64_t e) {
    Fr acc = Fr::one();
    bool started = false;
    for (int i = 63; i >= 0; --i) {
        if (started) acc = acc * acc;
        if ((e >> i) & 1) { acc = started ? acc * base : base; started = true; }
    }
    return acc;
}

// x[i] <- 1 / x[i], i < len; pre: len elements of scratch.  No x[i] is zero.
LSA_HD void fr_batch_inv_run(Fr *x, Fr *pre, unsigned len) {
    Fr acc = Fr::one();
    for (unsigned i = 0; i < len; i++) { pre[i] = acc; acc = acc * x[i]; }
    Fr inv = acc.inverse();
    for (unsigned i = len; i-- > 0;) {
        const Fr d = x[i];
        x[i] = inv * pre[i];
        inv = inv * d;
    }
}

struct FrGeomRow {
    Fr w, t;            // first factor of the denominator: t - w^i              (use_t)
    Fr v, a, c;         // second factor: a v^i - c                              (use_v)
    Fr k;               // numerator: k, or k w^i                                (num_w)
    int use_t, use_v, num_w;
};

// entries lo .. lo + len - 1 of the row, len <= FR_BATCH_INV_RUN, written to out[lo ..] (which also holds the denominators
// in between).  No denominator is zero: the callers rule that out beforehand (t outside the domain, Z without a root on the coset).
LSA_HD void fr_geom_row_run(const FrGeomRow &r, size_t lo, unsigned len, Fr *out) {
    Fr pre[FR_BATCH_INV_RUN];
    const Fr W0 = (r.use_t || r.num_w) ? fr_pow_u64(r.w, lo) : Fr::one();
    Fr W = W0, V = r.use_v ? r.a * fr_pow_u64(r.v, lo) : Fr::one();
    for (unsigned j = 0; j < len; j++) {
        Fr den = r.use_t ? r.t - W : Fr::one();
        if (r.use_v) den = r.use_t ? den * (V - r.c) : V - r.c;
        out[lo + j] = den;
        if (r.use_t) W = W * r.w;
        if (r.use_v) V = V * r.v;
    }
    fr_batch_inv_run(out + lo, pre, len);
    W = W0;
    for (unsigned j = 0; j < len; j++) {
        out[lo + j] = out[lo + j] * (r.num_w ? r.k * W : r.k);
        if (r.num_w) W = W * r.w;
    }
}

// the Lagrange coefficients at t of the radix-2 domain {w^i, i < 2^log_n}, times `scale`: scale (t^n - 1) / n * w^i / (t - w^i)
// (libfqfft _basic_radix2_evaluate_all_lagrange_polynomials; n = 1: the single coefficient 1).  t is not in the domain.
LSA_HD FrGeomRow fr_lagrange_row(unsigned log_n, const Fr &w, const Fr &t, const Fr &scale) {
    FrGeomRow r;
    r.w = w; r.t = t;
    r.v = r.a = r.c = Fr::one();
    Fr tn = t;
    for (unsigned i = 0; i < log_n; i++) tn = tn * tn;
    r.k = scale * (tn - Fr::one()) * fr_pow_u64(Fr::from_u32(2), log_n).inverse();
    r.use_t = 1; r.use_v = 0; r.num_w = 1;
    return r;
}

// ---- the step radix-2 domain, m = big + small = 2^big_log + 2^small_log, omega a primitive 2 big-th root of unity:
// points omega^(2i) (i < big) and omega sigma^j (j < small), sigma = omega^(2 big / small);
// Z(x) = (x^big - 1)(x^small - omega^small).
LSA_HD Fr fr_step_sigma(unsigned big_log, unsigned small_log, const Fr &omega) { return fr_pow_u64(omega, (uint64_t)1 << (big_log + 1 - small_log)); }

// 1 / Z(g x) * scale over the points x of the domain: on the big part x^big = 1 and x^small runs through the big / small
// powers of omega^(2 small), so entry i is table[i mod (big / small)], table = the row below; on the small part x^big = -1 and
// x^small = omega^small: the one constant `small_part`.  Z has no root on the coset (fr_coset_meets_roots).
struct FrStepZinv {
    FrGeomRow table;
    size_t period;
    Fr small_part;
};
LSA_HD FrStepZinv fr_step_zinv(unsigned big_log, unsigned small_log, const Fr &omega, const Fr &g, const Fr &scale) {
    const uint64_t big = (uint64_t)1 << big_log, small = (uint64_t)1 << small_log;
    const Fr one = Fr::one(), c = fr_pow_u64(omega, small), g_big = fr_pow_u64(g, big), g_small = fr_pow_u64(g, small);
    FrStepZinv z;
    z.period = (size_t)(big / small);
    z.table.w = z.table.t = one;
    z.table.v = fr_pow_u64(omega, 2 * small);
    z.table.a = g_small;
    z.table.c = c;
    z.table.k = scale * (g_big - one).inverse();
    z.table.use_t = 0; z.table.use_v = 1; z.table.num_w = 0;
    // (g omega)^big = -g^big, (g omega)^small = g^small omega^small
    z.small_part = scale * ((Fr::zero() - g_big - one) * (g_small * c - c)).inverse();
    return z;
}

// Does Z vanish somewhere on g * domain?  Basic domain (small_log < 0): Z(g x) = g^m - 1.  Step domain: every factor of
// Z(g x) that can vanish does so only if g^big = +-1 or g^small = omega^small x^-small, an element whose (2 big / small)-th
// power is 1: in all cases g^(2 big) = 1, and a g with g^(2 big) = 1 is refused whether or not it hits a root.
LSA_HD bool fr_coset_meets_roots(unsigned big_log, int small_log, const Fr &g) {
    Fr x = g;
    for (unsigned i = 0; i < big_log + (small_log < 0 ? 0u : 1u); i++) x = x * x;
    return x == Fr::one();
}

// 1 / Z(g x) * scale on the basic domain of 2^log_m points: the one constant 1 / (g^m - 1)
LSA_HD Fr fr_basic_zinv(unsigned log_m, const Fr &g, const Fr &scale) {
    Fr gm = g;
    for (unsigned i = 0; i < log_m; i++) gm = gm * gm;
    return scale * (gm - Fr::one()).inverse();
}

// The monomials of -d3 + d1 d2 Z, as up to four (index, value) pairs with distinct indices; set: the entry has no earlier
// value (index m).  Z = x^m - 1 on the basic domain (small_log < 0), x^m - c x^big - x^small + c with c = omega^small on
// the step domain (add_poly_Z of either domain, and coefficients_for_H[0] -= d3).
struct FrHqFix { size_t idx[4]; Fr val[4]; int set[4]; int n; };
LSA_HD FrHqFix fr_hq_fix(unsigned big_log, int small_log, const Fr &omega, const Fr d[3]) {
    const size_t big = (size_t)1 << big_log, small = small_log < 0 ? 0 : (size_t)1 << small_log, m = big + small;
    const Fr d12 = d[0] * d[1], zero = Fr::zero();
    FrHqFix f;
    for (int j = 0; j < 4; j++) { f.idx[j] = 0; f.val[j] = zero; f.set[j] = 0; }
    if (small_log < 0) {
        f.n = 2;
        f.idx[0] = 0; f.val[0] = zero - d[2] - d12;
        f.idx[1] = m; f.val[1] = d12; f.set[1] = 1;
    } else {
        const Fr d12c = d12 * fr_pow_u64(omega, small);
        f.n = 4;
        f.idx[0] = 0; f.val[0] = d12c - d[2];
        f.idx[1] = small; f.val[1] = zero - d12;
        f.idx[2] = big; f.val[2] = zero - d12c;
        f.idx[3] = m; f.val[3] = d12; f.set[3] = 1;
    }
    return f;
}

// evaluate_all_lagrange_polynomials(t) of either domain as at most two rows (the step domain: its big part, then its
// small part -- the radix-2 row of either part times the other part's vanishing factor, normalised at the point, as in
// shim/libfqfft/evaluation_domain/get_evaluation_domain.hpp).  unit: t is a point of the domain and part j of the row is
// [p_j w_j^i == t]; else part j is row[j] (fr_geom_row_run).
struct FrLagrangePlan {
    int parts, unit;
    size_t count[2];
    FrGeomRow row[2];
    Fr unit_w[2], unit_p[2];
};
LSA_HD FrLagrangePlan fr_lagrange_plan(unsigned big_log, int small_log, const Fr &omega, const Fr &t) {
    const Fr one = Fr::one();
    FrLagrangePlan p;
    p.count[0] = (size_t)1 << big_log;
    p.count[1] = 0;
    Fr t_big = t;
    for (unsigned i = 0; i < big_log; i++) t_big = t_big * t_big;
    if (small_log < 0) {
        p.parts = 1;
        p.unit = t_big == one;
        p.unit_w[0] = p.unit_w[1] = omega;
        p.unit_p[0] = p.unit_p[1] = one;
        p.row[0] = p.row[1] = fr_lagrange_row(big_log, omega, t, one);
        return p;
    }
    const size_t small = (size_t)1 << small_log;
    const Fr big_omega = omega * omega, sigma = fr_step_sigma(big_log, (unsigned)small_log, omega), ts = t * omega.inverse();
    const Fr c = fr_pow_u64(omega, small);
    Fr t_small = t, ts_small = ts;
    for (int i = 0; i < small_log; i++) { t_small = t_small * t_small; ts_small = ts_small * ts_small; }
    p.parts = 2;
    p.count[1] = small;
    p.unit = t_big == one || ts_small == one;                      // t is a point of the big / of the small part
    p.unit_w[0] = big_omega; p.unit_p[0] = one;
    p.unit_w[1] = sigma; p.unit_p[1] = omega;
    // big part: k w^i / ((t - w^i)(v^i - c)), w = omega^2, v = w^small, k = (t^big - 1) / big * (t^small - c)
    p.row[0] = fr_lagrange_row(big_log, big_omega, t, t_small - c);
    p.row[0].v = fr_pow_u64(big_omega, small); p.row[0].a = one; p.row[0].c = c; p.row[0].use_v = 1;
    // small part: the radix-2 row of {sigma^j} at t / omega, times (t^big - 1) / (omega^big - 1) = (t^big - 1) / -2
    p.row[1] = fr_lagrange_row((unsigned)small_log, sigma, ts, (t_big - one) * (Fr::zero() - Fr::from_u32(2)).inverse());
    return p;
}

// ---- the quotient's pointwise step on fr29.h's limbs: (a b - c) zinv + d2 a + d1 b, every word in and out libff's x 2^256.
// The words are read as limbs without conversion, so a (x) b stands for a b 2^512; with neg = the words of -1 (-2^256) the
// first reduction gives q = (a b - c) 2^251 (< 2r, tight); zinv carries 2^266 and d1, d2 carry 2^261 (fr_hq_consts), so the
// second reduction gives (...) 2^256 again.  Five schoolbook products, two reductions.
struct FrHqConsts { Fr zinv, d1, d2, neg; };
LSA_HD FrHqConsts fr_hq_consts(const Fr &zinv_times_1024, const Fr &d1, const Fr &d2) {
    const Fr up5 = Fr::from_u32(32);
    return {zinv_times_1024, d1 * up5, d2 * up5, Fr::zero() - Fr::one()};
}
LSA_HD Fr fr_hq_point(const Fr29 &a, const Fr29 &b, const Fr29 &c, const Fr29 &zinv, const Fr29 &d1, const Fr29 &d2, const Fr29 &neg) {
    Fr29Wide w = fr29_wide_zero();
    fr29_wide_mac(w, a, b);
    fr29_wide_mac(w, c, neg);
    const Fr29 q = fr29_wide_reduce(w);
    w = fr29_wide_zero();
    fr29_wide_mac(w, q, zinv);
    fr29_wide_mac(w, a, d2);
    fr29_wide_mac(w, b, d1);
    return fr29_wide_reduce(w).canonical2().to_words();
}

}  // namespace lsa
