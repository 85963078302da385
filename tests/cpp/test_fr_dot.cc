// Host unit test of csrc/fr_dot.h, the per-output dot product every lane of csrc/fr_matrix.hip runs, against big-integer
// arithmetic that shares nothing with it (64 x 64 -> 128-bit schoolbook product, reduction mod r by shift and subtract):
//   (1) fr_dot_words at lengths 0 .. 9, at FR_DOT_MAX_PARTIALS * FR_DOT_GROUP - 1, +0, +1 (where the running sum is first
//       brought back below 2r) and past a second such point, with strides 1 and 3;
//   (2) operands: random canonical residues; every operand r - 1; every operand the word pattern 2^256 - 1, which puts all
//       nine limbs of both factors at their maxima (fr_dot.h states its bounds for any 256-bit words);
//   (3) the way the matrix product calls it: limbs staged in steps of 16 with zero padding, four products per push -- and
//       after every push the stated invariants of the running sum (partials <= the maximum, limbs 0..7 below 2^29, the top
//       limb below 2^29, the value below 2 * partials * r);
//   (4) fr_dot_up() is 2^266 mod r.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "fp.h"
#include "fr29.h"
#include "fr_dot.h"
using namespace lsa;

static std::mt19937_64 rng(2025);
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { printf("FAIL "); printf(__VA_ARGS__); printf(" (line %d)\n", __LINE__); } fails++; } } while (0)

// ---- the reference: little-endian 64-bit limbs
typedef unsigned __int128 u128;
struct U256 { uint64_t w[4]; };
static const U256 RMOD = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
static const U256 INV256 = {{0xdc5ba0056db1194eull, 0x090ef5a9e111ec87ull, 0xc8260de4aeb85d5dull, 0x15ebf95182c5551cull}};   // 2^-256 mod r

static bool geq(const U256 &a, const U256 &b) {
    for (int i = 3; i >= 0; --i) if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
    return true;
}
static void sub_in_place(U256 &a, const U256 &b) {
    uint64_t borrow = 0;
    for (int i = 0; i < 4; i++) {
        const u128 d = (u128)a.w[i] - b.w[i] - borrow;
        a.w[i] = (uint64_t)d;
        borrow = (uint64_t)(d >> 64) & 1;
    }
}
// (a * b) mod r for any 256-bit a, b: the 512-bit product, then one bit at a time
static U256 mulmod(const U256 &a, const U256 &b) {
    uint64_t p[8] = {0};
    for (int i = 0; i < 4; i++) {
        uint64_t carry = 0;
        for (int j = 0; j < 4; j++) {
            const u128 t = (u128)a.w[i] * b.w[j] + p[i + j] + carry;
            p[i + j] = (uint64_t)t;
            carry = (uint64_t)(t >> 64);
        }
        p[i + 4] = carry;
    }
    U256 rem = {{0, 0, 0, 0}};
    for (int bit = 511; bit >= 0; --bit) {
        for (int i = 3; i > 0; --i) rem.w[i] = (rem.w[i] << 1) | (rem.w[i - 1] >> 63);      // rem < r < 2^254: no bit is lost
        rem.w[0] = (rem.w[0] << 1) | ((p[bit >> 6] >> (bit & 63)) & 1);
        if (geq(rem, RMOD)) sub_in_place(rem, RMOD);
    }
    return rem;
}
static U256 addmod(const U256 &a, const U256 &b) {                                           // a, b < r
    U256 s;
    uint64_t carry = 0;
    for (int i = 0; i < 4; i++) {
        const u128 t = (u128)a.w[i] + b.w[i] + carry;
        s.w[i] = (uint64_t)t;
        carry = (uint64_t)(t >> 64);
    }
    if (geq(s, RMOD)) sub_in_place(s, RMOD);
    return s;
}
static U256 words_of(const Fr &x) {
    U256 u;
    for (int i = 0; i < 4; i++) u.w[i] = (uint64_t)x.l[2 * i] | ((uint64_t)x.l[2 * i + 1] << 32);
    return u;
}
static Fr fr_of(const U256 &u) {
    Fr x;
    for (int i = 0; i < 4; i++) { x.l[2 * i] = (uint32_t)u.w[i]; x.l[2 * i + 1] = (uint32_t)(u.w[i] >> 32); }
    return x;
}
// libff's words of sum_k a_k b_k: (sum_k A_k B_k) 2^-256 mod r on the words A_k, B_k
static Fr expected_dot(const Fr *a, size_t sa, const Fr *b, size_t sb, size_t n) {
    U256 acc = {{0, 0, 0, 0}};
    for (size_t k = 0; k < n; k++) acc = addmod(acc, mulmod(words_of(a[k * sa]), words_of(b[k * sb])));
    return fr_of(mulmod(acc, INV256));
}

static Fr rand_fr() {
    for (;;) {
        U256 u;
        for (int i = 0; i < 4; i++) u.w[i] = rng();
        u.w[3] &= 0x3fffffffffffffffull;
        if (!geq(u, RMOD)) return fr_of(u);
    }
}
static Fr pattern(int kind) {
    if (kind == 0) return rand_fr();
    U256 u = RMOD;
    if (kind == 1) u.w[0] -= 1;                                   // r - 1
    else for (int i = 0; i < 4; i++) u.w[i] = ~(uint64_t)0;       // 2^256 - 1: limbs 0..7 at 2^29 - 1, the top limb at 2^24 - 1
    return fr_of(u);
}
static const char *KIND[3] = {"random", "r - 1", "2^256 - 1"};
static const size_t EDGE = (size_t)FR_DOT_MAX_PARTIALS * FR_DOT_GROUP;

static std::vector<size_t> lengths() {
    std::vector<size_t> v;
    for (size_t n = 0; n <= 9; n++) v.push_back(n);
    for (size_t n : {EDGE - 1, EDGE, EDGE + 1, 2 * EDGE - FR_DOT_GROUP + 1, 2 * EDGE + 5}) v.push_back(n);
    return v;
}

static void test_words() {
    for (int kind = 0; kind < 3; kind++)
        for (size_t n : lengths())
            for (size_t stride : {(size_t)1, (size_t)3}) {
                std::vector<Fr> a(n * stride + 1), b(n + 1);
                for (auto &x : a) x = pattern(kind);
                for (auto &x : b) x = pattern(kind);
                const Fr got = fr_dot_words(a.data(), stride, b.data(), 1, n), want = expected_dot(a.data(), stride, b.data(), 1, n);
                CHECK(got == want, "fr_dot_words %s n %zu stride %zu", KIND[kind], n, stride);
                CHECK(!geq(words_of(got), RMOD), "not canonical: %s n %zu", KIND[kind], n);
            }
}

// the value of tight limbs as 320 bits, compared with 2 * partials * r
static bool below_2pr(const Fr29 &s, uint32_t partials) {
    uint64_t v[5] = {0}, bound[5] = {0};
    for (int i = 0; i < 9; i++) {
        const int bit = 29 * i, j = bit >> 6, sh = bit & 63;
        v[j] += (uint64_t)s.l[i] << sh;                            // limbs do not overlap: a sum of disjoint bit fields
        if (sh > 35 && j + 1 < 5) v[j + 1] += (uint64_t)s.l[i] >> (64 - sh);
    }
    uint64_t carry = 0;
    for (int i = 0; i < 4; i++) {
        const u128 t = (u128)RMOD.w[i] * (2ull * partials) + carry;
        bound[i] = (uint64_t)t;
        carry = (uint64_t)(t >> 64);
    }
    bound[4] = carry;
    for (int i = 4; i >= 0; --i) if (v[i] != bound[i]) return v[i] < bound[i];
    return false;
}

static void test_staged_like_the_matrix_product() {
    const size_t STEP = 16;
    for (int kind = 0; kind < 3; kind++)
        for (size_t n : lengths()) {
            std::vector<Fr> a(n), b(n);
            for (auto &x : a) x = pattern(kind);
            for (auto &x : b) x = pattern(kind);
            FrDot d = fr_dot_zero();
            bool ok = true;
            for (size_t k0 = 0; k0 < n; k0 += STEP) {
                Fr29 la[STEP], lb[STEP];
                for (size_t k = 0; k < STEP; k++) {
                    la[k] = k0 + k < n ? Fr29::from_words(a[k0 + k]) : Fr29::zero();
                    lb[k] = k0 + k < n ? Fr29::from_words(b[k0 + k]) : Fr29::zero();
                }
                for (size_t g = 0; g < STEP; g += FR_DOT_GROUP) {
                    fr_dot_span(d, la + g, 1, lb + g, 1, FR_DOT_GROUP);
                    ok = ok && d.partials >= 1 && d.partials <= FR_DOT_MAX_PARTIALS && below_2pr(d.sum, d.partials) && d.sum.l[8] < (1u << 29);
                    for (int i = 0; i < 8; i++) ok = ok && d.sum.l[i] < (1u << 29);
                }
            }
            CHECK(ok, "invariants of the running sum: %s n %zu", KIND[kind], n);
            CHECK(fr_dot_finish(d) == expected_dot(a.data(), 1, b.data(), 1, n), "staged dot %s n %zu", KIND[kind], n);
        }
}

static void test_constant() {
    // 2^266 = 2^256 * 1024: libff's words of the value 1024
    const Fr k = Fr::from_u32(1024);
    const Fr29 up = fr_dot_up(), want = Fr29::from_words(k);
    bool same = true;
    for (int i = 0; i < 9; i++) same = same && up.l[i] == want.l[i];
    CHECK(same, "fr_dot_up() is not 2^266 mod r");
    CHECK(FR_DOT_GROUP == 4, "Fr29Wide holds four products");
    // 2 * MAX * r < 121 r and one more partial would not be: the stated count is the largest the bound allows
    CHECK(2 * FR_DOT_MAX_PARTIALS < 121 && 2 * (FR_DOT_MAX_PARTIALS + 1) > 121, "FR_DOT_MAX_PARTIALS against 121 r");
}

int main() {
    test_constant();
    test_words();
    test_staged_like_the_matrix_product();
    if (fails) { printf("%d FAILED\n", fails); return 1; }
    printf("PASS fr_dot (max partials %u, group %u)\n", FR_DOT_MAX_PARTIALS, FR_DOT_GROUP);
    return 0;
}
