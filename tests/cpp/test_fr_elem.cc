// Host unit test of csrc/fr_elem.h, the per-element and per-run arithmetic every lane of csrc/fr_elem.hip runs, against fp.h's
// plain Fr operators (the 64-bit-limb Montgomery code of the host side, which shares nothing with the 29-bit limbs under test)
// on operands brought below r by plain subtraction:
//   (1) fr_elem_canon and the constant forms over the edge patterns 0, the words of 1, r - 1, r, r + 1, 2r, 2^256 - 1 and random
//       256-bit patterns;
//   (2) fr_elem_mul_point over every pair of operand kinds and every kind of scale (none included);
//   (3) fr_elem_lincomb_point for k = 1 .. FR_VEC_LINCOMB_MAX, every vector and coefficient of one kind (r - 1 and 2^256 - 1: the
//       widest accumulator) and mixed kinds;
//   (4) fr29_pow_u64 and fr_elem_powers_run: bases 0, 1, -1, a root of unity, random; offsets 0, around a run, 2^20 + 5, 2^40 + 3;
//       every run length; first given and one; 0^0 = 1;
//   (5) fr_elem_inv_run: every run length, no zero, a zero in the first and in the last slot, nothing but zeros, zeros spelled
//       0, r and 2r, in place and out of place (the input untouched), the count;
//   (6) fr_elem_horner_run with an offset power, every length up to FR_ELEM_EVAL_ITEMS, and a whole evaluation the way the
//       kernels cut it (lanes, workgroups, the finishing sum over more than FR_DOT_MAX_PARTIALS partials).
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "fp.h"
#include "fr29.h"
#include "fr_batch_inv.h"
#include "fr_dot.h"
#include "fr_elem.h"
using namespace lsa;

static std::mt19937_64 rng(2027);
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { printf("FAIL "); printf(__VA_ARGS__); printf(" (line %d)\n", __LINE__); } fails++; } } while (0)

struct U256 { uint64_t w[4]; };
static const U256 RMOD = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
static bool geq(const U256 &a, const U256 &b) {
    for (int i = 3; i >= 0; --i) if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
    return true;
}
static void sub_in_place(U256 &a, const U256 &b) {
    unsigned __int128 borrow = 0;
    for (int i = 0; i < 4; i++) {
        const unsigned __int128 d = (unsigned __int128)a.w[i] - b.w[i] - borrow;
        a.w[i] = (uint64_t)d;
        borrow = (d >> 64) & 1;
    }
}
static U256 add_plain(const U256 &a, const U256 &b) {
    U256 s;
    unsigned __int128 carry = 0;
    for (int i = 0; i < 4; i++) {
        const unsigned __int128 t = (unsigned __int128)a.w[i] + b.w[i] + carry;
        s.w[i] = (uint64_t)t;
        carry = t >> 64;
    }
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
// the reference's way below r: subtract r while it fits (at most five times)
static Fr canon_ref(const Fr &x) {
    U256 u = words_of(x);
    while (geq(u, RMOD)) sub_in_place(u, RMOD);
    return fr_of(u);
}
static bool canonical(const Fr &x) { return !geq(words_of(x), RMOD); }

static Fr rand_fr() {
    for (;;) {
        U256 u;
        for (int i = 0; i < 4; i++) u.w[i] = rng();
        u.w[3] &= 0x3fffffffffffffffull;
        if (!geq(u, RMOD)) return fr_of(u);
    }
}
enum { OP_RANDOM, OP_ZERO, OP_ONE, OP_MINUS_ONE, OP_RM1, OP_R, OP_RP1, OP_2R, OP_ALL_ONES, OP_ANY, OP_KINDS };
static const char *OP[OP_KINDS] = {"random", "0", "one", "-1", "r - 1", "r", "r + 1", "2r", "2^256 - 1", "any 256 bits"};
static Fr operand(int kind) {
    U256 u = {{0, 0, 0, 0}};
    switch (kind) {
    case OP_RANDOM: return rand_fr();
    case OP_ZERO: break;
    case OP_ONE: return Fr::one();
    case OP_MINUS_ONE: return Fr::zero() - Fr::one();
    case OP_RM1: u = RMOD; u.w[0] -= 1; break;
    case OP_R: u = RMOD; break;
    case OP_RP1: u = RMOD; u.w[0] += 1; break;
    case OP_2R: u = add_plain(RMOD, RMOD); break;
    case OP_ALL_ONES: for (int i = 0; i < 4; i++) u.w[i] = ~(uint64_t)0; break;
    default: for (int i = 0; i < 4; i++) u.w[i] = rng();
    }
    return fr_of(u);
}
static bool tight(const Fr29 &s) {
    for (int i = 0; i < 9; i++) if (s.l[i] >= (1u << 29)) return false;
    return true;
}

static void test_canon_and_forms() {
    for (int k = 0; k < OP_KINDS; k++)
        for (int rep = 0; rep < (k == OP_RANDOM || k == OP_ANY ? 200 : 1); rep++) {
            const Fr x = operand(k), c = fr_elem_canon(x);
            CHECK(c == canon_ref(x) && canonical(c), "fr_elem_canon %s", OP[k]);
            // the forms: a product on limbs with the form-2^261 constant is the field product, in libff's words
            const Fr y = operand((k + rep + 3) % OP_KINDS);
            const Fr got = mul(Fr29::from_words(y), Fr29::from_words(fr_elem_c261(x))).canonical2().to_words();
            CHECK(got == canon_ref(y) * canon_ref(x), "fr_elem_c261 %s", OP[k]);
        }
    CHECK(fr_elem_c266(nullptr) == Fr::from_u32(1024), "the closing constant of a product without a scale is 2^266 mod r");
}

static void test_mul_point() {
    for (int ka = 0; ka < OP_KINDS; ka++)
        for (int kb = 0; kb < OP_KINDS; kb++)
            for (int ks = -1; ks < OP_KINDS; ks++) {
                const Fr a = operand(ka), b = operand(kb), s = ks < 0 ? Fr::one() : operand(ks);
                const Fr got = fr_elem_mul_point(Fr29::from_words(a), Fr29::from_words(b), Fr29::from_words(fr_elem_c266(ks < 0 ? nullptr : &s)));
                CHECK(got == canon_ref(a) * canon_ref(b) * canon_ref(s) && canonical(got), "mul_point %s x %s, scale %s", OP[ka], OP[kb], ks < 0 ? "none" : OP[ks]);
            }
    const Fr a = rand_fr();
    CHECK(fr_elem_mul_point(Fr29::from_words(a), Fr29::from_words(a), Fr29::from_words(fr_elem_c266(nullptr))) == a * a, "squares");
}

static void test_lincomb_point() {
    for (unsigned k = 1; k <= FR_VEC_LINCOMB_MAX; k++)
        for (int kx = 0; kx <= OP_KINDS; kx++)              // OP_KINDS: a different kind per term
            for (int kc = 0; kc <= OP_KINDS; kc++) {
                Fr x[FR_VEC_LINCOMB_MAX], c[FR_VEC_LINCOMB_MAX];
                Fr29 xl[FR_VEC_LINCOMB_MAX], cl[FR_VEC_LINCOMB_MAX];
                Fr want = Fr::zero();
                for (unsigned t = 0; t < k; t++) {
                    x[t] = operand(kx < OP_KINDS ? kx : (int)((t + k) % OP_KINDS));
                    c[t] = operand(kc < OP_KINDS ? kc : (int)((3 * t + 1) % OP_KINDS));
                    xl[t] = Fr29::from_words(x[t]);
                    cl[t] = Fr29::from_words(fr_elem_c261(c[t]));
                    want = want + canon_ref(c[t]) * canon_ref(x[t]);
                }
                const Fr got = fr_elem_lincomb_point(xl, cl, k);
                CHECK(got == want && canonical(got), "lincomb_point k %u, %s x %s", k, kx < OP_KINDS ? OP[kx] : "mixed", kc < OP_KINDS ? OP[kc] : "mixed");
            }
    // coefficients (1, -1): the difference, also of equal operands
    const Fr a = rand_fr(), b = rand_fr();
    const Fr29 cl[2] = {Fr29::from_words(fr_elem_c261(Fr::one())), Fr29::from_words(fr_elem_c261(Fr::zero() - Fr::one()))};
    const Fr29 ab[2] = {Fr29::from_words(a), Fr29::from_words(b)}, aa[2] = {Fr29::from_words(a), Fr29::from_words(a)};
    CHECK(fr_elem_lincomb_point(ab, cl, 2) == a - b, "a - b");
    CHECK(fr_elem_lincomb_point(aa, cl, 2) == Fr::zero(), "a - a");
}

static Fr root_of_unity_16() {                             // 5^((r - 1) / 16): 5 generates the multiplicative group
    U256 e = RMOD;
    e.w[0] -= 1;
    for (int s = 0; s < 4; s++) {
        for (int i = 0; i < 3; i++) e.w[i] = (e.w[i] >> 1) | (e.w[i + 1] << 63);
        e.w[3] >>= 1;
    }
    Fr acc = Fr::one();
    const Fr five = Fr::from_u32(5);
    for (int i = 255; i >= 0; --i) {
        acc = acc * acc;
        if ((e.w[i >> 6] >> (i & 63)) & 1) acc = acc * five;
    }
    return acc;
}

static void test_powers() {
    const Fr root = root_of_unity_16();
    CHECK(fr_pow_u64(root, 16) == Fr::one() && fr_pow_u64(root, 8) == Fr::zero() - Fr::one(), "the root of unity");
    std::vector<Fr> bases = {rand_fr(), rand_fr(), root};
    for (int k = 1; k < OP_KINDS; k++) bases.push_back(operand(k));
    const uint64_t los[] = {0, 1, 2, FR_ELEM_POWERS_RUN - 1, FR_ELEM_POWERS_RUN, FR_ELEM_POWERS_RUN + 1, 255, 256, ((uint64_t)1 << 20) + 5, ((uint64_t)1 << 40) + 3, ~(uint64_t)0};
    for (const Fr &b : bases) {
        const Fr bc = canon_ref(b);
        const Fr29 b261 = Fr29::from_words(fr_elem_c261(b));
        for (uint64_t lo : los) {
            const Fr29 p = fr29_pow_u64(b261, lo);
            CHECK(tight(p) && mul(p, Fr29::from_words(Fr::one())).canonical2().to_words() == fr_pow_u64(bc, lo), "fr29_pow_u64, exponent %llu", (unsigned long long)lo);
            for (int with_first = 0; with_first < 2; with_first++) {
                const Fr first = with_first ? fr_elem_canon(operand((int)(lo % OP_KINDS))) : Fr::one();
                for (unsigned len = 0; len <= FR_ELEM_POWERS_RUN; len++) {
                    if (lo > ((uint64_t)1 << 41) && len > 1) break;                   // (the offset may not wrap)
                    Fr out[FR_ELEM_POWERS_RUN + 1];
                    const Fr guard = rand_fr();
                    out[len] = guard;
                    fr_elem_powers_run(b261, Fr29::from_words(first), lo, len, out);
                    Fr want = first * fr_pow_u64(bc, lo);
                    bool ok = out[len] == guard;
                    for (unsigned j = 0; j < len; j++) { ok = ok && out[j] == want && canonical(out[j]); want = want * bc; }
                    CHECK(ok, "powers_run lo %llu len %u first %d", (unsigned long long)lo, len, with_first);
                }
            }
        }
    }
    Fr out[4];
    fr_elem_powers_run(Fr29::from_words(fr_elem_c261(Fr::zero())), Fr29::from_words(Fr::one()), 0, 4, out);
    CHECK(out[0] == Fr::one() && out[1].is_zero() && out[2].is_zero() && out[3].is_zero(), "0^0 = 1, then zeros");
}

static void test_inv_run() {
    const int zero_kinds[3] = {OP_ZERO, OP_R, OP_2R};
    for (unsigned len = 0; len <= FR_ELEM_INV_RUN; len++)
        for (int pattern = 0; pattern < 6; pattern++)
            for (int zk = 0; zk < 3; zk++)
                for (int in_place = 0; in_place < 2; in_place++) {
                    if (pattern == 0 && zk) continue;
                    Fr x[FR_ELEM_INV_RUN + 1] = {}, out[FR_ELEM_INV_RUN + 1] = {};
                    unsigned zeros = 0;
                    for (unsigned j = 0; j < len; j++) {
                        bool z = false;
                        switch (pattern) {
                        case 1: z = j == 0; break;
                        case 2: z = j == len - 1; break;
                        case 3: z = j == 0 || j == len - 1; break;
                        case 4: z = true; break;
                        case 5: z = rng() % 3 == 0; break;
                        }
                        x[j] = z ? operand(zero_kinds[zk]) : operand(pattern == 5 ? (int)(rng() % OP_KINDS) : OP_RANDOM);
                        if (canon_ref(x[j]).is_zero()) zeros++;
                    }
                    const Fr guard = rand_fr();
                    Fr keep[FR_ELEM_INV_RUN + 1];
                    memcpy(keep, x, sizeof keep);
                    Fr *dst = in_place ? x : out;
                    dst[len] = guard;
                    const unsigned got = fr_elem_inv_run(x, dst, len);
                    bool ok = got == zeros && dst[len] == guard;
                    for (unsigned j = 0; j < len; j++) {
                        const Fr c = canon_ref(keep[j]);
                        ok = ok && canonical(dst[j]) && (c.is_zero() ? dst[j].is_zero() : dst[j] * c == Fr::one() && dst[j] == c.inverse());
                        if (!in_place) ok = ok && x[j] == keep[j];
                    }
                    CHECK(ok, "inv_run len %u pattern %d zero %s in_place %d (zeros %u, got %u)", len, pattern, OP[zero_kinds[zk]], in_place, zeros, got);
                }
}

static Fr horner_ref(const std::vector<Fr> &c, const Fr &x) {
    Fr acc = Fr::zero();
    for (size_t j = c.size(); j-- > 0;) acc = acc * x + canon_ref(c[j]);
    return acc;
}

static void test_horner() {
    for (int kx = 0; kx < OP_KINDS; kx++)
        for (int kc = 0; kc <= OP_KINDS; kc++)
            for (unsigned len = 0; len <= FR_ELEM_EVAL_ITEMS; len++)
                for (uint64_t lo : {(uint64_t)0, (uint64_t)1, (uint64_t)FR_ELEM_EVAL_ITEMS, (uint64_t)255 * FR_ELEM_EVAL_ITEMS}) {
                    const Fr x = fr_elem_canon(operand(kx));
                    std::vector<Fr> c(len);
                    for (unsigned j = 0; j < len; j++) c[j] = operand(kc < OP_KINDS ? kc : (int)((j + len) % OP_KINDS));
                    const Fr29 x261 = Fr29::from_words(fr_elem_c261(x));
                    const Fr29 got = fr_elem_horner_run(c.data(), len, x261, fr29_pow_u64(x261, lo));
                    CHECK(tight(got) && got.canonical2().to_words() == horner_ref(c, x) * fr_pow_u64(x, lo), "horner_run x %s c %s len %u lo %llu", OP[kx],
                          kc < OP_KINDS ? OP[kc] : "mixed", len, (unsigned long long)lo);
                }
}

// a whole evaluation cut the way the kernels cut it: `lanes` lanes per workgroup, the lane's offset as a power of x^items,
// the workgroup's as a power of x^(items lanes) applied after the lanes' sum, the finishing sum on limbs
static void test_whole_evaluation() {
    const unsigned lanes = 4, items = FR_ELEM_EVAL_ITEMS;
    for (int kx : {OP_RANDOM, OP_ZERO, OP_ONE, OP_MINUS_ONE})
        for (int kc : {OP_RANDOM, OP_RM1, OP_ALL_ONES, OP_KINDS})
            for (size_t n : {(size_t)1, (size_t)items * lanes, (size_t)items * lanes + 1, (size_t)items * lanes * (FR_DOT_MAX_PARTIALS + 1) + 3, (size_t)items * lanes * (2 * FR_DOT_MAX_PARTIALS + 7)}) {
                const Fr x = fr_elem_canon(operand(kx));
                std::vector<Fr> c(n);
                for (size_t j = 0; j < n; j++) c[j] = operand(kc < OP_KINDS ? kc : (int)(rng() % OP_KINDS));
                const FrEvalConsts k = fr_elem_eval_consts(x, items, lanes);
                const size_t blocks = (n + (size_t)items * lanes - 1) / ((size_t)items * lanes);
                FrDot d = fr_dot_zero();
                bool within = true;
                for (size_t blk = 0; blk < blocks; blk++) {
                    Fr sum = Fr::zero();
                    for (unsigned lane = 0; lane < lanes; lane++) {
                        const size_t lo = (blk * lanes + lane) * items;
                        if (lo >= n) continue;
                        const size_t left = n - lo;
                        const Fr29 v = fr_elem_horner_run(c.data() + lo, (unsigned)(left < items ? left : items), Fr29::from_words(k.x261), fr29_pow_u64(Fr29::from_words(k.xi261), lane));
                        sum = sum + v.canonical2().to_words();
                    }
                    const Fr partial = blk ? sum * fr_pow_u64(k.xb, blk) : sum;
                    fr_elem_sum_push(d, Fr29::from_words(partial));
                    within = within && d.partials <= FR_DOT_MAX_PARTIALS && tight(d.sum);
                }
                const Fr got = fr_elem_sum_finish(d);
                CHECK(within && got == horner_ref(c, x) && canonical(got), "whole evaluation x %s c %s n %zu", OP[kx], kc < OP_KINDS ? OP[kc] : "mixed", n);
            }
    // the running sum alone, far past the fold: t copies of r - 1 (as words) and of 2^256 - 1 would not be reduced values, so
    // copies of canonical r - 1
    FrDot d = fr_dot_zero();
    const Fr top = operand(OP_RM1);
    Fr want = Fr::zero();
    for (unsigned t = 0; t < 5 * FR_DOT_MAX_PARTIALS + 1; t++) { fr_elem_sum_push(d, Fr29::from_words(top)); want = want + top; }
    CHECK(fr_elem_sum_finish(d) == want, "a long running sum of r - 1");
}

int main() {
    test_canon_and_forms();
    test_mul_point();
    test_lincomb_point();
    test_powers();
    test_inv_run();
    test_horner();
    test_whole_evaluation();
    if (fails) { printf("%d FAILED\n", fails); return 1; }
    printf("PASS fr_elem (lincomb max %u, inv run %d, powers run %d, eval items %d, dot max partials %u, group %u)\n", FR_VEC_LINCOMB_MAX, FR_ELEM_INV_RUN,
           FR_ELEM_POWERS_RUN, FR_ELEM_EVAL_ITEMS, FR_DOT_MAX_PARTIALS, FR_DOT_GROUP);
    return 0;
}
