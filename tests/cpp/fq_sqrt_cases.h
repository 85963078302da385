// tests/cpp/fq_sqrt_cases.h -- the operand list of csrc/fq_sqrt.h's tests, built on the host: tests/cpp/test_fq_sqrt.cc
// checks every entry against Euler's criterion / [r]P == O, tools/fq_sqrt_check.hip runs the same list through the device
// compilation and compares with the host compilation.  Runs on the host.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "fq_sqrt.h"

// (under hipcc the device pass parses these host functions too, and there fp.h's product is a __device__ function)
#if defined(__HIPCC__)
#define FQC_FN inline __host__ __device__
#else
#define FQC_FN inline
#endif

namespace fqcases {
using namespace lsa;

struct Rng {
    uint64_t s;
    FQC_FN uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    FQC_FN Fq fq() {
        uint32_t w[8];
        for (int i = 0; i < 8; i += 2) { const uint64_t v = next(); w[i] = (uint32_t)v; w[i + 1] = (uint32_t)(v >> 32); }
        w[7] &= 0x1fffffffu;                                     // < 2^253 < p
        return Fq::from_canonical(w);
    }
    FQC_FN Fq2 fq2() { Fq a = fq(); Fq b = fq(); return {a, b}; }
};

#define FQC_REQUIRE(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

// plain square-and-multiply over the bits of a 256-bit exponent (independent of fq_sqrt.h's window schedule)
FQC_FN Fq fq_pow(const Fq &a, const uint32_t e[8]) {
    Fq acc = Fq::one();
    for (int i = 255; i >= 0; --i) {
        acc = acc.sqr();
        if ((e[i >> 5] >> (i & 31)) & 1) acc = acc * a;
    }
    return acc;
}
// Euler's criterion: a^((p-1)/2) == 1  (0 counts as a square)
FQC_FN bool fq_is_square(const Fq &a) {
    if (a.is_zero()) return true;
    uint32_t e[8];
    for (int i = 0; i < 8; i++) e[i] = (LSA_P[i] >> 1) | (i < 7 ? LSA_P[i + 1] << 31 : 0u);   // (p - 1) / 2: p is odd
    return fq_pow(a, e) == Fq::one();
}
// a != 0 is a square in Fq2 iff its norm is a square in Fq
FQC_FN bool fq2_is_square(const Fq2 &a) { return fq_is_square(a.c0.sqr() + a.c1.sqr()); }

// plain double-and-add, any point of the twist
FQC_FN Jac<Fq2> g2_ladder(const Jac<Fq2> &p, const uint32_t e[8]) {
    Jac<Fq2> acc = Jac<Fq2>::inf();
    for (int i = 255; i >= 0; --i) {
        acc = jac_dbl(acc);
        if ((e[i >> 5] >> (i & 31)) & 1) acc = jac_add(acc, p);
    }
    return acc;
}
FQC_FN Jac<Fq2> g2_small(const Jac<Fq2> &p, uint32_t k) {
    const uint32_t e[8] = {k, 0, 0, 0, 0, 0, 0, 0};
    return g2_ladder(p, e);
}
FQC_FN bool g2_on_curve(const Jac<Fq2> &p) {
    if (p.is_inf()) return true;
    const Fq2 z2 = p.Z.sqr(), z6 = z2.sqr() * z2;
    return p.Y.sqr() == p.X.sqr() * p.X + fq2_const(LSA_TWIST_B) * z6;
}
// the same point with another Z
FQC_FN Jac<Fq2> g2_rescale(const Jac<Fq2> &p, const Fq2 &z) {
    if (p.is_inf()) return p;
    const Fq2 z2 = z.sqr();
    return {p.X * z2, p.Y * (z2 * z), p.Z * z};
}

// #E'(Fq2) = r c, c = 2p - r = 10069 * 5864401 * ...
static const uint32_t ORDER_R[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
static const uint32_t COFACTOR[8] = {0xc0f9fa8du, 0x345f2299u, 0x572a2489u, 0x06ceecdau, 0x8181585eu, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
static const uint32_t COFACTOR_DIV_10069[8] = {0x915f1659u, 0x6c3cd334u, 0x671af448u, 0x207142f7u, 0x5b5681dau, 0x9e28bcf6u, 0xa58fce69u, 0x00013af7u};
static const uint32_t COFACTOR_DIV_5864401[8] = {0x56710dfdu, 0xd3865bedu, 0x679e3e75u, 0xd47f2c69u, 0x0434f091u, 0x67a5f866u, 0x712e2645u, 0x0000008au};

struct Cases {
    std::vector<Fq> fq;            // operands of fq_sqrt
    std::vector<Fq2> fq2;          // operands of fq2_sqrt
    std::vector<Jac<Fq2>> pts;     // points of the twist, operands of g2_in_subgroup
    size_t fq2_second = 0;         // fq2 operands (squares, a1 != 0) whose first candidate (a0 + sn)/2 is a non-residue
};

FQC_FN Jac<Fq2> g2_generator() { return {fq2_const(LSA_G2_GEN_X), fq2_const(LSA_G2_GEN_Y), Fq2::one()}; }

FQC_FN Cases build(int n_random) {
    Cases c;
    Rng rng{0x9e3779b97f4a7c15ull};
    // ---- Fq
    c.fq.push_back(Fq::zero());
    c.fq.push_back(Fq::one());
    c.fq.push_back(Fq::zero() - Fq::one());                      // p - 1: a non-residue (p = 3 mod 4)
    for (uint32_t k = 2; k < 20; k++) c.fq.push_back(Fq::from_u32(k));
    for (int i = 0; i < 16; i++) { const Fq x = rng.fq(); c.fq.push_back(x.sqr()); c.fq.push_back(x.sqr().neg()); }
    for (int i = 0; i < n_random; i++) c.fq.push_back(rng.fq());
    // ---- Fq2
    c.fq2.push_back(Fq2::zero());
    c.fq2.push_back(Fq2::one());
    c.fq2.push_back(Fq2{Fq::zero(), Fq::one()});
    c.fq2.push_back(Fq2{Fq::zero() - Fq::one(), Fq::zero()});
    c.fq2.push_back(Fq2{Fq::zero(), Fq::zero() - Fq::one()});
    for (int i = 0; i < 8; i++) {                                // (t, 0): t a residue, t a non-residue
        const Fq s = rng.fq().sqr();
        c.fq2.push_back(Fq2{s, Fq::zero()});
        c.fq2.push_back(Fq2{s.neg(), Fq::zero()});
        c.fq2.push_back(Fq2{Fq::zero(), s});                     // a0 == 0, a1 != 0
    }
    for (int i = 0; i < n_random; i++) {
        const Fq2 z = rng.fq2();
        const Fq2 a = (i & 1) ? z.sqr() : z;                     // half of them squares for certain
        c.fq2.push_back(a);
        if (!a.c1.is_zero() && fq2_is_square(a)) {
            Fq sn;
            FQC_REQUIRE(fq_sqrt(a.c0.sqr() + a.c1.sqr(), &sn));
            if (!fq_is_square((a.c0 + sn) * fq_words(LSA_FQ_TWO_INV))) c.fq2_second++;
        }
    }
    // ---- points of the twist
    const Jac<Fq2> G = g2_generator();
    c.pts.push_back(Jac<Fq2>::inf());
    const uint32_t ks[] = {1, 2, 3, 12345, 1000003};
    for (uint32_t k : ks) c.pts.push_back(g2_small(G, k));
    std::vector<Jac<Fq2>> twist;
    for (uint32_t i = 1; twist.size() < 4; i++) {                // twist points found by trying x = i + u
        const Fq2 x{Fq::from_u32(i), Fq::one()};
        Fq2 y;
        if (!fq2_sqrt(x.sqr() * x + fq2_const(LSA_TWIST_B), &y)) continue;
        twist.push_back({x, y, Fq2::one()});
    }
    for (const auto &T : twist) {
        FQC_REQUIRE(g2_on_curve(T));
        c.pts.push_back(T);
        c.pts.push_back(g2_ladder(T, COFACTOR));                 // [c]T lies in G2
    }
    const Jac<Fq2> T = twist[0];
    const Jac<Fq2> rT = g2_ladder(T, ORDER_R);
    const Jac<Fq2> s1 = g2_ladder(rT, COFACTOR_DIV_10069), s2 = g2_ladder(rT, COFACTOR_DIV_5864401);
    FQC_REQUIRE(!s1.is_inf() && g2_small(s1, 10069).is_inf());   // order exactly 10069 (a prime)
    FQC_REQUIRE(!s2.is_inf() && g2_small(s2, 5864401).is_inf());
    c.pts.push_back(s1);
    c.pts.push_back(s2);
    c.pts.push_back(jac_neg(s1));
    c.pts.push_back(g2_small(s1, 2));
    c.pts.push_back(jac_add(g2_small(G, 7), s1));
    c.pts.push_back(jac_add(g2_small(G, 12345), s2));
    c.pts.push_back(jac_add(g2_ladder(T, COFACTOR), jac_add(s1, s2)));
    // every point again with a Z outside Fq (psi conjugates Z)
    const size_t n0 = c.pts.size();
    for (size_t i = 0; i < n0; i++) c.pts.push_back(g2_rescale(c.pts[i], rng.fq2()));
    for (const auto &p : c.pts) FQC_REQUIRE(g2_on_curve(p));
    return c;
}

}  // namespace fqcases
