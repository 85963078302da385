// Host unit test of csrc/smul_g2.h (the per-item body of k_smul_g2, instantiated with the one-lane Fq2 type F29x2): [s]P by
// signed 4-bit digits over the whole scalar against plain double-and-add with the generic Jacobian formulas of ec.h on
// fp.h's Jac<Fq2>, compared after normalisation; and the recoding identity sum digit_j 16^j = s.
//
// Arguments (tests/test_smul_g2_host.py computes them with oracle/pymodel): eight hexadecimal integers, the affine
// coordinates x.c0 x.c1 y.c0 y.c1 of a twist point OUTSIDE the order-r subgroup and of a twist point of small order.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <random>
#include <vector>
#include "ec.h"
#include "tower.h"
#include "smul_g2.h"
using namespace lsa;

using Scalar = std::array<uint32_t, 8>;

static bool less_than(const Scalar &a, const uint32_t b[8]) {
    for (int i = 7; i >= 0; --i)
        if (a[i] != b[i]) return a[i] < b[i];
    return false;
}
static Scalar small(uint32_t v) { return Scalar{v, 0, 0, 0, 0, 0, 0, 0}; }
static Scalar sub(const Scalar &a, const Scalar &b) {
    Scalar r;
    uint64_t borrow = 0;
    for (int i = 0; i < 8; i++) {
        const uint64_t d = (uint64_t)a[i] - b[i] - borrow;
        r[i] = (uint32_t)d;
        borrow = (d >> 32) & 1;
    }
    return r;
}
static Scalar add(const Scalar &a, const Scalar &b) {
    Scalar r;
    uint64_t c = 0;
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)a[i] + b[i];
        r[i] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}
static Scalar half(const Scalar &a) {
    Scalar r;
    for (int i = 0; i < 8; i++) r[i] = (a[i] >> 1) | (i < 7 ? a[i + 1] << 31 : 0);
    return r;
}
static Scalar pow2(int k) {
    Scalar r = small(0);
    r[k >> 5] = 1u << (k & 31);
    return r;
}
static Scalar modulus() {
    Scalar r;
    for (int i = 0; i < 8; i++) r[i] = FrParams::MOD[i];
    return r;
}
static Scalar reduced(Scalar a) {
    while (!less_than(a, FrParams::MOD)) a = sub(a, modulus());
    return a;
}
static Scalar filled(uint32_t nibble) { Scalar r; r.fill(nibble * 0x11111111u); return r; }

static Jac<Fq2> plain_mul(const Jac<Fq2> &P, const Scalar &k) {
    Jac<Fq2> acc = Jac<Fq2>::inf();
    for (int i = 255; i >= 0; --i) {
        acc = jac_dbl(acc);
        if ((k[i >> 5] >> (i & 31)) & 1) acc = jac_add(acc, P);
    }
    return acc;
}
static Aff29x2 to_affine29(const Jac<Fq2> &P) {
    if (P.is_inf()) return {F29x2::zero(), F29x2::zero()};
    const Jac<Fq2> n = jac_normalize(P);
    return {f29x2_from_mont256(n.X).canonical(), f29x2_from_mont256(n.Y).canonical()};
}
static bool same_point(const Jac<Fq2> &a, const Jac<Fq2> &b) {
    if (a.is_inf() || b.is_inf()) return a.is_inf() && b.is_inf();
    const Jac<Fq2> x = jac_normalize(a), y = jac_normalize(b);
    return x.X == y.X && x.Y == y.Y;
}

// sum digit_j 16^j == s, digits in [-8, 7], the top one in [0, 4]; every prefix of the digit string is >= 0
static bool recoding_ok(const Scalar &s) {
    uint32_t dg[8];
    recode_nibbles_256(s.data(), dg);
    Scalar acc = small(0);
    for (int j = SMUL_G2_DIGITS - 1; j >= 0; --j) {
        const int d = smul_g2_digit(dg, j);
        if (d < -8 || d > 7) return false;
        if (j == SMUL_G2_DIGITS - 1 && (d < 0 || d > 4)) return false;
        if (acc[7] >> 28) return false;                                          // the shift below must not lose bits
        for (int i = 7; i >= 0; --i) acc[i] = (acc[i] << 4) | (i ? acc[i - 1] >> 28 : 0);
        if (d >= 0) acc = add(acc, small((uint32_t)d));
        else {
            if (less_than(acc, small((uint32_t)-d).data())) return false;       // a negative prefix
            acc = sub(acc, small((uint32_t)-d));
        }
    }
    return acc == s;
}

static int check(const Jac<Fq2> &P, const Scalar &s, const char *what, size_t idx) {
    static int reported = 0;
    XYZZ29x2 T[SMUL_G2_TBL];
    const Jac<Fq2> got = g2_to_jac(smul_g2<F29x2>(to_affine29(P), s.data(), T));
    const Jac<Fq2> want = plain_mul(P, s);
    if (same_point(got, want)) return 0;
    if (reported++ < 8) printf("mismatch: %s, scalar %zu\n", what, idx);
    return 1;
}

static Fq fq_from_hex(const char *h) {
    if (h[0] == '0' && (h[1] == 'x' || h[1] == 'X')) h += 2;
    const size_t len = strlen(h);
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < len && i < 64; i++) {
        const char c = h[len - 1 - i];
        const uint32_t v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : 0;
        w[i >> 3] |= v << ((i & 7) * 4);
    }
    return Fq::from_canonical(w);
}
static Jac<Fq2> point_from_args(char **a) { return {{fq_from_hex(a[0]), fq_from_hex(a[1])}, {fq_from_hex(a[2]), fq_from_hex(a[3])}, Fq2::one()}; }
static bool on_twist(const Jac<Fq2> &p) {                    // affine (Z = 1): y^2 = x^3 + 3/xi
    return p.Y.sqr() == p.X.sqr() * p.X + fq2_const(LSA_TWIST_B);
}

int main(int argc, char **argv) {
    if (argc != 9) { printf("usage: test_smul_g2 <outside: x0 x1 y0 y1> <small order: x0 x1 y0 y1>  (hexadecimal)\n"); return 2; }
    const Jac<Fq2> G = {fq2_const(LSA_G2_GEN_X), fq2_const(LSA_G2_GEN_Y), Fq2::one()};
    const Jac<Fq2> outside = point_from_args(argv + 1), tiny = point_from_args(argv + 5);
    int fails = 0;
    if (!on_twist(outside) || !on_twist(tiny) || !on_twist(G)) { printf("an argument is not a point of the twist\n"); return 2; }
    const Scalar r = modulus();
    if (plain_mul(outside, r).is_inf()) { printf("the 'outside' point is in the subgroup\n"); return 2; }

    std::vector<Scalar> edge;
    for (uint32_t v : {0u, 1u, 2u, 7u, 8u, 9u, 15u, 16u, 17u}) edge.push_back(small(v));
    edge.push_back(sub(r, small(1)));
    edge.push_back(sub(r, small(2)));
    edge.push_back(half(sub(r, small(1))));
    edge.push_back(half(add(r, small(1))));
    for (uint32_t nib : {7u, 8u, 15u}) edge.push_back(reduced(filled(nib)));
    for (int k : {4, 124, 125, 126, 127, 128, 129, 130, 131, 132, 252, 253}) {
        edge.push_back(pow2(k));
        edge.push_back(sub(pow2(k), small(1)));
    }
    std::mt19937_64 rng(2024);
    std::vector<Scalar> random;
    while (random.size() < 2000) {
        Scalar k;
        for (int i = 0; i < 4; i++) { const uint64_t x = rng(); k[2 * i] = (uint32_t)x; k[2 * i + 1] = (uint32_t)(x >> 32); }
        k[7] &= 0x3fffffffu;
        if (less_than(k, FrParams::MOD)) random.push_back(k);
    }

    // the recoding, over the same scalars
    for (size_t i = 0; i < edge.size(); i++)
        if (!recoding_ok(edge[i])) { printf("recoding wrong at edge scalar %zu\n", i); fails++; }
    for (size_t i = 0; i < random.size(); i++)
        if (!recoding_ok(random[i])) { if (fails < 8) printf("recoding wrong at random scalar %zu\n", i); fails++; }

    // edge scalars on every kind of base
    const Jac<Fq2> walked = jac_add(jac_dbl(jac_add(jac_dbl(G), G)), G);                        // 7G, Z != 1
    const Jac<Fq2> outside3 = jac_add(jac_dbl(outside), outside);                               // Z != 1
    struct { const char *name; Jac<Fq2> p; } bases[] = {{"generator", G}, {"7G (Z != 1)", walked}, {"infinity", Jac<Fq2>::inf()},
                                                         {"outside the subgroup", outside}, {"3 * outside (Z != 1)", outside3},
                                                         {"small order", tiny}, {"2 * small order", jac_dbl(tiny)}};
    for (auto &b : bases)
        for (size_t i = 0; i < edge.size(); i++) fails += check(b.p, edge[i], b.name, i);
    if (!same_point(plain_mul(G, edge[9]), jac_neg(G))) { printf("(r - 1) G != -G in the reference ladder\n"); fails++; }

    // random scalars on a walk of un-normalised bases, in and out of the subgroup
    Jac<Fq2> P = G, Q = outside, S = tiny;
    for (size_t i = 0; i < random.size(); i++) {
        const int kind = (int)(i % 4);
        fails += check(kind == 3 ? S : kind == 2 ? Q : P, random[i], kind == 3 ? "small-order walk" : kind == 2 ? "outside walk" : "subgroup walk", i);
        if (kind == 3) S = jac_add(jac_dbl(S), tiny);
        else if (kind == 2) Q = jac_add(jac_dbl(Q), outside);
        else P = jac_add(jac_dbl(P), G);                                                          // next base: 2P + G
    }
    printf("%zu edge scalars x %zu bases, %zu random scalars\n", edge.size(), sizeof(bases) / sizeof(bases[0]), random.size());
    printf(fails ? "FAILED (%d)\n" : "PASS\n", fails);
    return fails ? 1 : 0;
}
