// Host unit test of csrc/fr_sparse.h, the per-row routine every lane of csrc/fr_sparse.hip runs, against big-integer
// arithmetic that shares nothing with it (64 x 64 -> 128-bit schoolbook product, reduction mod r by shift and subtract):
//   (1) rows of lengths 0 .. 5, one past FR_DOT_MAX_PARTIALS * FR_DOT_GROUP general entries, one past FR_SPARSE_UNIT_MAX unit
//       entries (and past a second such point), with strides 1 and 64 (a lane of the chunk kernel);
//   (2) coefficient mixes: only general, only +1, only -1, alternating +-1, units mixed with general, an explicit zero
//       coefficient among them; a -1 row whose sum is 0;
//   (3) operands: random canonical residues, every operand 0, the word 1, r - 1, the word pattern 2^256 - 1;
//   (4) after every entry the stated invariants of the two accumulators (counts within their maxima, limbs tight, the unit
//       sum at most 6 * units * r, the running sum below 2 * partials * r);
//   (5) classification: the canonical words of +1 and of r - 1 are units, nothing else is -- 0, the word 1, r - 1 as a
//       word, and the non-canonical spellings (2^256 mod r) + r, ... of the value 1 are general; the constants.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "fp.h"
#include "fr29.h"
#include "fr_dot.h"
#include "fr_sparse.h"
using namespace lsa;

static std::mt19937_64 rng(2026);
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { printf("FAIL "); printf(__VA_ARGS__); printf(" (line %d)\n", __LINE__); } fails++; } } while (0)

// ---- the reference: little-endian 64-bit limbs
typedef unsigned __int128 u128;
struct U256 { uint64_t w[4]; };
static const U256 RMOD = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
static const U256 INV256 = {{0xdc5ba0056db1194eull, 0x090ef5a9e111ec87ull, 0xc8260de4aeb85d5dull, 0x15ebf95182c5551cull}};   // 2^-256 mod r
static const U256 MONT1 = {{0xac96341c4ffffffbull, 0x36fc76959f60cd29ull, 0x666ea36f7879462eull, 0x0e0a77c19a07df2full}};    // 2^256 mod r

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
static U256 add_plain(const U256 &a, const U256 &b) {                                        // (no overflow at the callers)
    U256 s;
    uint64_t carry = 0;
    for (int i = 0; i < 4; i++) {
        const u128 t = (u128)a.w[i] + b.w[i] + carry;
        s.w[i] = (uint64_t)t;
        carry = (uint64_t)(t >> 64);
    }
    return s;
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
    U256 s = add_plain(a, b);
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
static U256 minus_one_words() { U256 u = RMOD; sub_in_place(u, MONT1); return u; }

// libff's words of sum_e v_e x_{idx e}: (sum_e V_e X_{idx e}) 2^-256 mod r on the words, every entry as a product
static Fr expected_row(const std::vector<Fr> &vals, const std::vector<uint32_t> &idx, const std::vector<Fr> &x, size_t lo, size_t hi, size_t stride) {
    U256 acc = {{0, 0, 0, 0}};
    for (size_t e = lo; e < hi; e += stride) acc = addmod(acc, mulmod(words_of(vals[e]), words_of(x[idx[e]])));
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
enum { OP_RANDOM, OP_ZERO, OP_WORD1, OP_RM1, OP_ALL_ONES, OP_KINDS };
static const char *OP[OP_KINDS] = {"random", "0", "word 1", "r - 1", "2^256 - 1"};
static Fr operand(int kind) {
    U256 u = {{0, 0, 0, 0}};
    switch (kind) {
    case OP_RANDOM: return rand_fr();
    case OP_ZERO: break;
    case OP_WORD1: u.w[0] = 1; break;
    case OP_RM1: u = RMOD; u.w[0] -= 1; break;
    default: for (int i = 0; i < 4; i++) u.w[i] = ~(uint64_t)0;      // limbs 0..7 at 2^29 - 1, the top limb at 2^24 - 1
    }
    return fr_of(u);
}
enum { MIX_GENERAL, MIX_PLUS, MIX_MINUS, MIX_ALTERNATE, MIX_MIXED, MIX_KINDS };
static const char *MIX[MIX_KINDS] = {"general", "+1", "-1", "+-1", "mixed"};
static Fr coefficient(int mix, size_t e, int op) {
    const Fr plus = fr_of(MONT1), minus = fr_of(minus_one_words());
    switch (mix) {
    case MIX_GENERAL: return operand(op);
    case MIX_PLUS: return plus;
    case MIX_MINUS: return minus;
    case MIX_ALTERNATE: return e & 1 ? minus : plus;
    default:
        switch (rng() % 5) {
        case 0: return plus;
        case 1: return minus;
        case 2: return Fr::zero();                                    // an explicit zero coefficient
        default: return operand(op);
        }
    }
}

static const size_t DOT_EDGE = (size_t)FR_DOT_MAX_PARTIALS * FR_DOT_GROUP, UNIT_EDGE = FR_SPARSE_UNIT_MAX;

static std::vector<size_t> lengths() {
    std::vector<size_t> v;
    for (size_t n = 0; n <= 5; n++) v.push_back(n);
    for (size_t n : {UNIT_EDGE - 1, UNIT_EDGE, UNIT_EDGE + 1, 2 * UNIT_EDGE + 1, DOT_EDGE, DOT_EDGE + 1, 2 * DOT_EDGE + 5,
                     UNIT_EDGE * FR_DOT_MAX_PARTIALS + UNIT_EDGE + 1}) v.push_back(n);    // (the last: the joined sums alone fill the FrDot)
    return v;
}

// the value of tight limbs as 320 bits, compared with factor * r (or_equal: <=)
static bool below(const Fr29 &s, uint64_t factor, bool or_equal = false) {
    uint64_t v[5] = {0}, bound[5] = {0};
    for (int i = 0; i < 9; i++) {
        const int bit = 29 * i, j = bit >> 6, sh = bit & 63;
        v[j] += (uint64_t)s.l[i] << sh;                                // limbs do not overlap: a sum of disjoint bit fields
        if (sh > 35 && j + 1 < 5) v[j + 1] += (uint64_t)s.l[i] >> (64 - sh);
    }
    uint64_t carry = 0;
    for (int i = 0; i < 4; i++) {
        const u128 t = (u128)RMOD.w[i] * factor + carry;
        bound[i] = (uint64_t)t;
        carry = (uint64_t)(t >> 64);
    }
    bound[4] = carry;
    for (int i = 4; i >= 0; --i) if (v[i] != bound[i]) return v[i] < bound[i];
    return or_equal;
}
static bool tight(const Fr29 &s) {
    for (int i = 0; i < 9; i++) if (s.l[i] >= (1u << 29)) return false;
    return true;
}
static bool invariants(const FrSparseAcc &a) {
    return a.units <= FR_SPARSE_UNIT_MAX && a.pending < FR_DOT_GROUP && a.d.partials <= FR_DOT_MAX_PARTIALS && tight(a.unit) && tight(a.d.sum) &&
           below(a.unit, 6ull * a.units, true) && (a.d.partials == 0 || below(a.d.sum, 2ull * a.d.partials));
}

static void test_rows() {
    for (int mix = 0; mix < MIX_KINDS; mix++)
        for (int op = 0; op < OP_KINDS; op++)
            for (size_t n : lengths())
                for (size_t stride : {(size_t)1, (size_t)64}) {
                    if (stride > 1 && n > 2 * UNIT_EDGE + 1) continue;                // (a lane's share of a chunk is short)
                    const size_t ncols = 7, lo = 3, hi = lo + n * stride;
                    std::vector<Fr> vals(hi + 1), x(ncols);
                    std::vector<uint32_t> idx(hi + 1);
                    std::vector<uint8_t> cls(hi + 1);
                    for (auto &v : x) v = operand(op);
                    for (size_t e = 0; e <= hi; e++) {
                        vals[e] = coefficient(mix, e, op);
                        idx[e] = (uint32_t)(rng() % ncols);                           // duplicates within a row are the rule
                        cls[e] = fr_sparse_class(vals[e]);
                    }
                    const Fr want = expected_row(vals, idx, x, lo, hi, stride);
                    const Fr got = fr_sparse_row(vals.data(), cls.data(), idx.data(), x.data(), lo, hi, stride, FrSparseLoadPlain());
                    CHECK(got == want, "fr_sparse_row %s x %s n %zu stride %zu", MIX[mix], OP[op], n, stride);
                    CHECK(!geq(words_of(got), RMOD), "not canonical: %s x %s n %zu", MIX[mix], OP[op], n);
                    // the same entries one by one, the invariants after each
                    FrSparseAcc a = fr_sparse_zero();
                    bool ok = invariants(a);
                    for (size_t e = lo; e < hi; e += stride) {
                        const Fr29 xe = Fr29::from_words(x[idx[e]]);
                        if (cls[e] == FR_SPARSE_GENERAL) fr_sparse_add_general(a, Fr29::from_words(vals[e]), xe);
                        else fr_sparse_add_unit(a, cls[e] == FR_SPARSE_MINUS, xe);
                        ok = ok && invariants(a);
                    }
                    CHECK(ok, "invariants of the accumulators: %s x %s n %zu", MIX[mix], OP[op], n);
                    CHECK(fr_sparse_finish(a) == want, "entry by entry: %s x %s n %zu", MIX[mix], OP[op], n);
                }
}

// a row of -1 whose sum is zero: operands a, r - a (as words), and all-zero operands
static void test_minus_row_summing_to_zero() {
    for (size_t pairs : {(size_t)1, (size_t)2, (size_t)UNIT_EDGE / 2 + 1, (size_t)UNIT_EDGE + 3}) {
        std::vector<Fr> x(2 * pairs), vals(2 * pairs, fr_of(minus_one_words()));
        std::vector<uint32_t> idx(2 * pairs);
        std::vector<uint8_t> cls(2 * pairs, FR_SPARSE_MINUS);
        for (size_t p = 0; p < pairs; p++) {
            const Fr a = rand_fr();
            U256 neg = RMOD;
            sub_in_place(neg, words_of(a));
            x[2 * p] = a;
            x[2 * p + 1] = fr_of(neg);
        }
        for (size_t e = 0; e < 2 * pairs; e++) idx[e] = (uint32_t)e;
        const Fr got = fr_sparse_row(vals.data(), cls.data(), idx.data(), x.data(), 0, 2 * pairs, 1, FrSparseLoadPlain());
        CHECK(got == Fr::zero(), "-1 row over a, r - a: %zu pairs", pairs);
        for (auto &v : x) v = Fr::zero();
        const Fr z = fr_sparse_row(vals.data(), cls.data(), idx.data(), x.data(), 0, 2 * pairs, 1, FrSparseLoadPlain());
        CHECK(z == Fr::zero(), "-1 row over zeros: %zu pairs", pairs);
    }
}

static void test_classes_and_constants() {
    const U256 minus = minus_one_words();
    CHECK(fr_sparse_class(fr_of(MONT1)) == FR_SPARSE_PLUS, "+1");
    CHECK(fr_sparse_class(fr_of(minus)) == FR_SPARSE_MINUS, "the words of r - 1 are -1");
    CHECK(fr_of(MONT1) == Fr::one() && fr_of(minus) == Fr::zero() - Fr::one(), "the reference's words of +-1");
    // the value r - 1 the long way: (r - 1) * 2^256 mod r
    U256 rm1 = RMOD;
    rm1.w[0] -= 1;
    CHECK(geq(mulmod(rm1, MONT1), minus) && geq(minus, mulmod(rm1, MONT1)), "(r - 1) 2^256 mod r");
    U256 ones;
    for (int i = 0; i < 4; i++) ones.w[i] = ~(uint64_t)0;
    U256 word1 = {{1, 0, 0, 0}};
    std::vector<U256> general = {U256{{0, 0, 0, 0}}, word1, rm1, ones, RMOD};
    // every non-canonical spelling of +1 and of -1 that fits 256 bits
    for (const U256 &base : {MONT1, minus}) {
        U256 v = base;
        for (;;) {
            const U256 next = add_plain(v, RMOD);
            if (!geq(next, v)) break;                                      // wrapped past 2^256
            v = next;
            general.push_back(v);
        }
    }
    CHECK(general.size() >= 5 + 4 + 4, "non-canonical spellings: %zu patterns", general.size());
    for (const U256 &u : general) CHECK(fr_sparse_class(fr_of(u)) == FR_SPARSE_GENERAL, "a pattern that is no canonical unit: top word %016llx", (unsigned long long)u.w[3]);
    // ... and they still count as their value: coefficient (2^256 mod r) + r times x is x
    {
        std::vector<Fr> vals = {fr_of(add_plain(MONT1, RMOD))}, x = {rand_fr()};
        std::vector<uint32_t> idx = {0};
        std::vector<uint8_t> cls = {fr_sparse_class(vals[0])};
        CHECK(fr_sparse_row(vals.data(), cls.data(), idx.data(), x.data(), 0, 1, 1, FrSparseLoadPlain()) == x[0], "a non-canonical 1 as a product");
    }
    const Fr29 down = fr_sparse_down(), want = Fr29::from_words(Fr::one());
    bool same = true;
    for (int i = 0; i < 9; i++) same = same && down.l[i] == want.l[i];
    CHECK(same, "fr_sparse_down() is not 2^256 mod r");
    // 6r exceeds every 256-bit pattern, 5r does not; 6 * MAX * r < 121 r and one more term would not be
    U256 r5 = RMOD;
    for (int k = 0; k < 4; k++) r5 = add_plain(r5, RMOD);
    CHECK(!geq(add_plain(r5, RMOD), r5), "6r wraps past 2^256 while 5r does not");
    CHECK(6 * FR_SPARSE_UNIT_MAX < 121 && 6 * (FR_SPARSE_UNIT_MAX + 1) > 121, "FR_SPARSE_UNIT_MAX against 121 r");
    // fr29_sub6r at its corners: 0 - (2^256 - 1) + 6r, and the largest unit sum minus zero
    const Fr29 z = fr29_sub6r(Fr29::zero(), Fr29::from_words(fr_of(ones)));
    CHECK(tight(z) && below(z, 1), "0 - (2^256 - 1) + 6r is 6r - 2^256 + 1 < r");
}

int main() {
    test_classes_and_constants();
    test_rows();
    test_minus_row_summing_to_zero();
    if (fails) { printf("%d FAILED\n", fails); return 1; }
    printf("PASS fr_sparse (unit max %u, dot max partials %u, group %u)\n", FR_SPARSE_UNIT_MAX, FR_DOT_MAX_PARTIALS, FR_DOT_GROUP);
    return 0;
}
