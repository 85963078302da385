// Host unit test of csrc/fr_batch_inv.h, the code the kernels of csrc/fr_poly.hip run one lane at a time:
//   (1) fr_batch_inv_run against Fr::inverse() element by element, run lengths 1, L-1, L, L+1 (as two runs), 3L+2 (as four),
//       with the values 1 and r - 1 among the random ones;
//   (2) fr_geom_row_run / fr_lagrange_row: the Lagrange coefficients of a radix-2 domain against the definition
//       L_i(t) = prod_(j != i) (t - x_j) / (x_i - x_j), cut into runs the way the kernel cuts them;
//   (3) fr_step_zinv: the step domain's table of 1 / Z(g x) and its small-part constant against direct evaluation of
//       Z(x) = (x^big - 1)(x^small - omega^small) at every point of the coset;
//   (4) fr_coset_meets_roots: whenever Z has a root on g * domain the coset is refused (g running through roots of unity and
//       generic values), and the reference's coset generator 5 is accepted;
//   (5) fr_hq_point, the quotient's pointwise step on 29-bit limbs, against the same expression on fp.h's Fr, the values
//       0, 1 and r - 1 in every position;
//   (6) fr_hq_fix / fr_basic_zinv against Z written out, and fr_lagrange_plan (both domains, t outside the domain and at
//       points of either part) against the definition of the Lagrange coefficients.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "fp.h"
#include "fr_batch_inv.h"
using namespace lsa;

static std::mt19937_64 rng(77);
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { printf("FAIL "); printf(__VA_ARGS__); printf(" (line %d)\n", __LINE__); } fails++; } } while (0)

static Fr rand_fr() {
    for (;;) {
        Fr x;
        for (int i = 0; i < 4; i++) { uint64_t v = rng(); x.l[2 * i] = (uint32_t)v; x.l[2 * i + 1] = (uint32_t)(v >> 32); }
        x.l[7] &= 0x3fffffffu;
        bool lt = false;
        for (int i = 7; i >= 0; --i) if (x.l[i] != FrParams::MOD[i]) { lt = x.l[i] < FrParams::MOD[i]; break; }
        if (lt && !x.is_zero()) return x;
    }
}
// primitive 2^L-th root of unity: 5^((r - 1) / 2^28) squared down
static Fr root_of_unity(unsigned L) {
    uint32_t e[8], rm1[8];
    for (int i = 0; i < 8; i++) rm1[i] = FrParams::MOD[i];
    rm1[0] -= 1;
    for (int i = 0; i < 8; i++) e[i] = (uint32_t)(((uint64_t)rm1[i] >> 28) | ((uint64_t)(i + 1 < 8 ? rm1[i + 1] : 0) << 4));
    Fr acc = Fr::one(), five = Fr::from_u32(5);
    for (int i = 255; i >= 0; --i) { acc = acc * acc; if ((e[i >> 5] >> (i & 31)) & 1) acc = acc * five; }
    for (unsigned i = 28; i > L; --i) acc = acc * acc;
    return acc;
}

// a vector inverted the way the kernel cuts it: runs of FR_BATCH_INV_RUN, the last one shorter
static void invert_in_runs(std::vector<Fr> &x) {
    Fr pre[FR_BATCH_INV_RUN];
    for (size_t lo = 0; lo < x.size(); lo += FR_BATCH_INV_RUN) {
        const size_t left = x.size() - lo;
        fr_batch_inv_run(x.data() + lo, pre, (unsigned)(left < FR_BATCH_INV_RUN ? left : FR_BATCH_INV_RUN));
    }
}
static std::vector<Fr> row_in_runs(const FrGeomRow &r, size_t count) {
    std::vector<Fr> out(count);
    for (size_t lo = 0; lo < count; lo += FR_BATCH_INV_RUN) {
        const size_t left = count - lo;
        fr_geom_row_run(r, lo, (unsigned)(left < FR_BATCH_INV_RUN ? left : FR_BATCH_INV_RUN), out.data());
    }
    return out;
}

static void test_batch_inversion() {
    const unsigned L = FR_BATCH_INV_RUN;
    const Fr one = Fr::one(), top = Fr::zero() - one;                       // r - 1
    for (size_t len : {(size_t)1, (size_t)L - 1, (size_t)L, (size_t)L + 1, (size_t)3 * L + 2}) {
        for (int variant = 0; variant < 3; variant++) {
            std::vector<Fr> x(len);
            for (auto &v : x) v = rand_fr();
            if (variant == 1) { x[0] = one; x[len - 1] = top; x[len / 2] = one; }
            if (variant == 2) for (size_t i = 0; i < len; i++) x[i] = (i & 1) ? top : one;
            const std::vector<Fr> keep = x;
            invert_in_runs(x);
            for (size_t i = 0; i < len; i++) {
                CHECK(x[i] == keep[i].inverse(), "batch inverse len %zu variant %d entry %zu", len, variant, i);
                CHECK(x[i] * keep[i] == one, "x * 1/x len %zu variant %d entry %zu", len, variant, i);
            }
        }
    }
}

static void test_lagrange_row() {
    const Fr one = Fr::one();
    for (unsigned log_n : {0u, 1u, 3u, 5u, 6u}) {
        const size_t n = (size_t)1 << log_n;
        const Fr w = root_of_unity(log_n);
        for (int which = 0; which < 2; which++) {
            const Fr t = which ? Fr::zero() : rand_fr(), scale = which ? one : rand_fr();
            const std::vector<Fr> got = row_in_runs(fr_lagrange_row(log_n, w, t, scale), n);
            std::vector<Fr> x(n);
            Fr p = one;
            for (size_t i = 0; i < n; i++) { x[i] = p; p = p * w; }
            for (size_t i = 0; i < n; i++) {
                Fr num = scale, den = one;
                for (size_t j = 0; j < n; j++) if (j != i) { num = num * (t - x[j]); den = den * (x[i] - x[j]); }
                CHECK(got[i] == num * den.inverse(), "lagrange row log_n %u entry %zu", log_n, i);
            }
        }
    }
}

static Fr step_Z(unsigned big_log, unsigned small_log, const Fr &omega, const Fr &x) {
    const uint64_t big = (uint64_t)1 << big_log, small = (uint64_t)1 << small_log;
    return (fr_pow_u64(x, big) - Fr::one()) * (fr_pow_u64(x, small) - fr_pow_u64(omega, small));
}
static std::vector<Fr> step_points(unsigned big_log, unsigned small_log, const Fr &omega) {
    const size_t big = (size_t)1 << big_log, small = (size_t)1 << small_log;
    std::vector<Fr> x(big + small);
    const Fr sigma = fr_step_sigma(big_log, small_log, omega);
    for (size_t i = 0; i < big; i++) x[i] = fr_pow_u64(omega, 2 * i);
    for (size_t j = 0; j < small; j++) x[big + j] = omega * fr_pow_u64(sigma, j);
    return x;
}

static void test_step_zinv_table() {
    const unsigned cases[][2] = {{1, 0}, {2, 1}, {3, 0}, {5, 2}, {6, 0}, {7, 6}, {8, 3}};
    for (const auto &bs : cases) {
        const unsigned big_log = bs[0], small_log = bs[1];
        const size_t big = (size_t)1 << big_log;
        const Fr omega = root_of_unity(big_log + 1);
        const std::vector<Fr> x = step_points(big_log, small_log, omega);
        for (int which = 0; which < 2; which++) {
            const Fr g = which ? rand_fr() : Fr::from_u32(5), scale = which ? rand_fr() : Fr::one();
            CHECK(!fr_coset_meets_roots(big_log, (int)small_log, g), "generic coset refused (%u, %u)", big_log, small_log);
            const FrStepZinv z = fr_step_zinv(big_log, small_log, omega, g, scale);
            CHECK(z.period == big >> small_log, "period (%u, %u)", big_log, small_log);
            const std::vector<Fr> tab = row_in_runs(z.table, z.period);
            for (size_t i = 0; i < x.size(); i++) {
                const Fr want = scale * step_Z(big_log, small_log, omega, g * x[i]).inverse();
                const Fr got = i < big ? tab[i % z.period] : z.small_part;
                CHECK(got == want, "1/Z on the coset (%u, %u) point %zu", big_log, small_log, i);
            }
        }
    }
}

static void test_coset_rule() {
    const Fr one = Fr::one();
    // step domains: g through every 2^k-th root of unity up to 4 big, their products with generic values, and generic values
    const unsigned cases[][2] = {{1, 0}, {2, 1}, {3, 0}, {4, 2}, {5, 4}};
    for (const auto &bs : cases) {
        const unsigned big_log = bs[0], small_log = bs[1];
        const Fr omega = root_of_unity(big_log + 1);
        const std::vector<Fr> x = step_points(big_log, small_log, omega);
        std::vector<Fr> gs;
        const Fr w4 = root_of_unity(big_log + 2);
        Fr p = one;
        for (size_t k = 0; k < ((size_t)4 << big_log); k++) { gs.push_back(p); p = p * w4; }
        for (int k = 0; k < 8; k++) gs.push_back(rand_fr());
        gs.push_back(Fr::from_u32(5));
        size_t refused = 0;
        for (const Fr &g : gs) {
            bool root = false;
            for (const Fr &xi : x) root = root || step_Z(big_log, small_log, omega, g * xi).is_zero();
            const bool no = fr_coset_meets_roots(big_log, (int)small_log, g);
            CHECK(!root || no, "Z has a root on an accepted coset (%u, %u)", big_log, small_log);
            CHECK(no == (fr_pow_u64(g, (uint64_t)2 << big_log) == one), "rule is g^(2 big) = 1 (%u, %u)", big_log, small_log);
            refused += no;
        }
        CHECK(refused == ((size_t)2 << big_log), "2 big roots of unity refused (%u, %u): %zu", big_log, small_log, refused);
    }
    // basic domains: Z(g x) = g^m - 1
    for (unsigned log_m : {1u, 2u, 5u}) {
        const Fr w2 = root_of_unity(log_m + 1);
        Fr p = one;
        for (size_t k = 0; k < ((size_t)2 << log_m); k++) {
            const bool root = fr_pow_u64(p, (uint64_t)1 << log_m) == one;
            CHECK(fr_coset_meets_roots(log_m, -1, p) == root, "basic rule log_m %u k %zu", log_m, k);
            p = p * w2;
        }
        CHECK(!fr_coset_meets_roots(log_m, -1, Fr::from_u32(5)), "generator refused on the basic domain");
        CHECK(fr_coset_meets_roots(log_m, -1, one), "g = 1 accepted on the basic domain");
    }
}

// the Lagrange plan of either domain against the definition, t outside and inside the domain
static void test_lagrange_plan() {
    const Fr one = Fr::one();
    const int cases[][2] = {{1, -1}, {3, -1}, {5, -1}, {1, 0}, {2, 1}, {3, 0}, {5, 2}, {5, 4}};
    for (const auto &bs : cases) {
        const unsigned big_log = (unsigned)bs[0];
        const int small_log = bs[1];
        const Fr omega = root_of_unity(small_log < 0 ? big_log : big_log + 1);
        std::vector<Fr> x;
        if (small_log < 0) { Fr p = one; for (size_t i = 0; i < ((size_t)1 << big_log); i++) { x.push_back(p); p = p * omega; } }
        else x = step_points(big_log, (unsigned)small_log, omega);
        std::vector<Fr> ts = {rand_fr(), Fr::zero(), x[0], x[x.size() - 1], x[((size_t)1 << big_log) - 1], x[x.size() / 2]};
        if (small_log >= 0) ts.push_back(x[(size_t)1 << big_log]);
        for (const Fr &t : ts) {
            const FrLagrangePlan p = fr_lagrange_plan(big_log, small_log, omega, t);
            std::vector<Fr> got;
            for (int j = 0; j < p.parts; j++) {
                if (p.unit) { Fr y = p.unit_p[j]; for (size_t i = 0; i < p.count[j]; i++) { got.push_back(y == t ? one : Fr::zero()); y = y * p.unit_w[j]; } }
                else { const std::vector<Fr> part = row_in_runs(p.row[j], p.count[j]); got.insert(got.end(), part.begin(), part.end()); }
            }
            CHECK(got.size() == x.size(), "plan size (%u, %d)", big_log, small_log);
            for (size_t i = 0; i < x.size() && i < got.size(); i++) {
                Fr num = one, den = one;
                for (size_t j = 0; j < x.size(); j++) if (j != i) { num = num * (t - x[j]); den = den * (x[i] - x[j]); }
                CHECK(got[i] == num * den.inverse(), "lagrange plan (%u, %d) entry %zu", big_log, small_log, i);
            }
        }
    }
}

// fr_hq_fix and fr_basic_zinv against Z written out: sum of the monomials = d1 d2 Z(x) - d3 at a random x
static void test_hq_fix() {
    const int cases[][2] = {{1, -1}, {4, -1}, {1, 0}, {3, 0}, {5, 2}, {5, 4}};
    for (const auto &bs : cases) {
        const unsigned big_log = (unsigned)bs[0];
        const int small_log = bs[1];
        const Fr omega = root_of_unity(small_log < 0 ? big_log : big_log + 1), x = rand_fr();
        const Fr d[3] = {rand_fr(), rand_fr(), rand_fr()};
        const FrHqFix f = fr_hq_fix(big_log, small_log, omega, d);
        const size_t m = ((size_t)1 << big_log) + (small_log < 0 ? 0 : (size_t)1 << small_log);
        Fr sum = Fr::zero();
        for (int j = 0; j < f.n; j++) {
            sum = sum + f.val[j] * fr_pow_u64(x, f.idx[j]);
            CHECK(f.idx[j] <= m && (f.set[j] != 0) == (f.idx[j] == m), "fix index (%u, %d)", big_log, small_log);
            for (int k = 0; k < j; k++) CHECK(f.idx[k] != f.idx[j], "fix indices distinct (%u, %d)", big_log, small_log);
        }
        const Fr Z = small_log < 0 ? fr_pow_u64(x, m) - Fr::one() : step_Z(big_log, (unsigned)small_log, omega, x);
        CHECK(sum == d[0] * d[1] * Z - d[2], "d1 d2 Z - d3 (%u, %d)", big_log, small_log);
        if (small_log < 0) CHECK(fr_basic_zinv(big_log, x, d[0]) * Z == d[0], "basic 1/Z log_m %u", big_log);
    }
}

static void test_hq_point() {
    const Fr one = Fr::one(), top = Fr::zero() - one, up10 = Fr::from_u32(1024);
    for (int it = 0; it < 2000; it++) {
        Fr v[6];
        for (auto &x : v) x = rand_fr();
        // the extremes: every combination of 0, 1, r - 1 in the first 729 rounds
        if (it < 729) { int k = it; for (auto &x : v) { x = (k % 3 == 0) ? Fr::zero() : (k % 3 == 1) ? one : top; k /= 3; } }
        const Fr &a = v[0], &b = v[1], &c = v[2], &zinv = v[3], &d1 = v[4], &d2 = v[5];
        const FrHqConsts k = fr_hq_consts(zinv * up10, d1, d2);
        const Fr got = fr_hq_point(Fr29::from_words(a), Fr29::from_words(b), Fr29::from_words(c), Fr29::from_words(k.zinv), Fr29::from_words(k.d1),
                                   Fr29::from_words(k.d2), Fr29::from_words(k.neg));
        CHECK(got == (a * b - c) * zinv + d2 * a + d1 * b, "hq point round %d", it);
    }
}

int main() {
    test_hq_point();
    test_hq_fix();
    test_lagrange_plan();
    test_batch_inversion();
    test_lagrange_row();
    test_step_zinv_table();
    test_coset_rule();
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("PASS (run length %d)\n", (int)FR_BATCH_INV_RUN);
    return 0;
}
