// Host unit test of the paired products of csrc/fp29.h: on the host mul2 / sqr2 call the single forms (the fallback the
// LSA_HD code compiles to), and the column stepper behind the device forms (f29_chain2 over MulTerms / SqrTerms, its step
// plain C++ here) must enumerate the same limb products: both are compared limb for limb with mul / sqr on the stated
// extremes of each form and on random tight operands.  Build: g++ -std=c++17 -O2 -I legosnark_amd/csrc
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "ec.h"
#include "fp29.h"

using namespace lsa;
static std::mt19937_64 rng(20261019);
static int fails = 0;
#define CHECK(c, msg) do { if (!(c)) { printf("FAIL %s (line %d)\n", msg, __LINE__); fails++; } } while (0)

static bool eq(const F29 &a, const F29 &b) { return memcmp(a.l, b.l, sizeof a.l) == 0; }
static F29 k_times_p(uint32_t k, int minus) {          // k*p - minus in tight limbs
    F29 r;
    uint64_t c = 0;
    for (int i = 0; i < 9; i++) { c += (uint64_t)F29::p(i) * k; r.l[i] = i < 8 ? (uint32_t)c & F29::MASK : (uint32_t)c; c >>= 29; }
    int64_t b = -minus;
    for (int i = 0; i < 9 && b != 0; i++) { int64_t v = (int64_t)r.l[i] + b; if (i < 8) { r.l[i] = (uint32_t)v & F29::MASK; b = v >> 29; } else r.l[i] = (uint32_t)v; }
    return r;
}
static F29 all_limbs(uint32_t v) { F29 r; for (int i = 0; i < 9; i++) r.l[i] = v; return r; }
static F29 rand_tight() { F29 r; for (int i = 0; i < 9; i++) r.l[i] = (uint32_t)rng() & (i == 8 ? 0x3fffffu : F29::MASK); return r; }

static void check_mul(const F29 &a0, const F29 &b0, const F29 &a1, const F29 &b1) {
    const F29 w0 = mul(a0, b0), w1 = mul(a1, b1);
    const F29Pair f = mul2(a0, b0, a1, b1), s = f29_chain2<MacPaired>(MulTerms{a0, b0}, MulTerms{a1, b1});
    CHECK(eq(f.a, w0) && eq(f.b, w1), "mul2 (host form) against mul");
    CHECK(eq(s.a, w0) && eq(s.b, w1), "column stepper over MulTerms against mul");
}
static void check_sqr(const F29 &a0, const F29 &a1) {
    const F29 w0 = sqr(a0), w1 = sqr(a1);
    uint32_t d0[9], d1[9];
    f29_doubled(a0, d0);
    f29_doubled(a1, d1);
    const F29Pair f = sqr2(a0, a1), s = f29_chain2<MacPaired>(SqrTerms{a0, d0}, SqrTerms{a1, d1});
    CHECK(eq(f.a, w0) && eq(f.b, w1), "sqr2 (host form) against sqr");
    CHECK(eq(s.a, w0) && eq(s.b, w1), "column stepper over SqrTerms against sqr");
}

int main() {
    // values 0, 1, p - 1, p, 2p - 1, the largest operand of mul (11p), every limb 2^29 - 1
    const std::vector<F29> tight = {F29::zero(), k_times_p(0, -1), k_times_p(1, 1), k_times_p(1, 0), k_times_p(2, 1), k_times_p(11, 0), all_limbs(F29::MASK)};
    const F29 loose = all_limbs((1u << 30) - 1);       // sqr only
    for (const F29 &a : tight) for (const F29 &b : tight) { check_mul(a, b, b, a); check_sqr(a, b); }
    for (const F29 &a : tight) { check_sqr(loose, a); check_sqr(a, loose); }
    check_sqr(loose, loose);
    for (int i = 0; i < 4096; i++) {
        const F29 a0 = rand_tight(), b0 = rand_tight(), a1 = rand_tight(), b1 = rand_tight();
        check_mul(a0, b0, a1, b1);
        check_sqr(a0, b1);
    }
    // the paired general addition is, on the host, the single forms in another order: the same limbs as xyzz29_add
    {
        const Aff29 g{F29::from_mont256(Fq::from_u32(1)).canonical(), F29::from_mont256(Fq::from_u32(2)).canonical()};
        XYZZ29 a = xyzz29_dbl_affine(g), b = xyzz29_madd(a, g);         // 2G, 3G
        for (int i = 0; i < 64; i++) {
            const XYZZ29 w = xyzz29_add(a, b), v = xyzz29_add_paired(a, b);
            CHECK(eq(w.X, v.X) && eq(w.Y, v.Y) && eq(w.ZZ, v.ZZ) && eq(w.ZZZ, v.ZZZ), "xyzz29_add_paired against xyzz29_add");
            a = b; b = w;
        }
        const XYZZ29 d = xyzz29_add_paired(a, a), n = xyzz29_add_paired(a, xyzz29_neg(a)), i0 = xyzz29_add_paired(XYZZ29::inf(), a);
        const XYZZ29 dw = xyzz29_dbl(a);
        CHECK(eq(d.X, dw.X) && eq(d.Y, dw.Y) && eq(d.ZZ, dw.ZZ) && eq(d.ZZZ, dw.ZZZ), "doubling");
        CHECK(n.is_inf(), "cancellation");
        CHECK(eq(i0.X, a.X) && eq(i0.ZZZ, a.ZZZ), "infinity + a");
    }
    // the number of limb products per column is that of the single forms
    int nm = 0, ns = 0;
    for (int k = 0; k < 17; k++) { nm += MulTerms::count(k); ns += SqrTerms::count(k); }
    CHECK(nm == 81 && ns == 45, "81 limb products in a product, 45 in a square");
    printf(fails ? "FAIL (%d)\n" : "PASS\n", fails);
    return fails ? 1 : 0;
}
