// Host unit test of csrc/ecntt.h (the stage geometry and the per-butterfly body of the k_ecntt_* kernels, G2 instantiated
// with the one-lane Fq2 type F29x2):
//   1. geometry, log_n <= 10: every stage's butterflies partition the elements and the slots, the pairs and twiddle indices
//      are those of the textbook decimation-in-time network, stage s writes where stage s + 1 reads, stage 1 reads the
//      bit-reversed input, the last stage writes natural order, and the butterflies are ordered j-first;
//   2. whole transforms of n = 1, 2, 4, 16 run through ecntt_bfly / ecntt_twiddled / ecntt_combine exactly as ecntt.hip
//      runs them (twiddle table w^t, second operands normalised before each stage, the inverse's 1/n on the inputs), G1 and
//      G2, forward and inverse, on a_i G with un-normalised representatives, against [(naive O(n^2) Fr transform of a)_k] G
//      by plain double-and-add with ec.h's Jacobian formulas; the same on the degenerate inputs of a commitment key: all
//      inputs equal, (P, O, ..., O), and the pure frequencies w^(-i k0) P.
#include <cstdio>
#include <cstdint>
#include <random>
#include <vector>
#include "ec.h"
#include "tower.h"
#include "ecntt.h"
using namespace lsa;

// ---------------------------------------------------------------- Fr helpers
static Fr fr_pow_words(const Fr &b, const uint32_t e[8]) {
    Fr acc = Fr::one();
    for (int i = 255; i >= 0; --i) {
        acc = acc.sqr();
        if ((e[i >> 5] >> (i & 31)) & 1) acc = acc * b;
    }
    return acc;
}
static Fr fr_pow_u(Fr b, uint64_t e) {
    Fr acc = Fr::one();
    for (; e; e >>= 1, b = b.sqr())
        if (e & 1) acc = acc * b;
    return acc;
}
// a primitive 2^log_n-th root of unity: 5 generates Fr*, r - 1 = 2^28 * odd
static Fr root_of_unity(unsigned log_n) {
    uint32_t e[8];
    for (int i = 0; i < 8; i++) e[i] = FrParams::MOD[i];
    e[0] -= 1;                                                          // r - 1 (r is odd)
    for (int i = 0; i < 8; i++) e[i] = (e[i] >> 28) | (i < 7 ? e[i + 1] << 4 : 0);
    Fr w = fr_pow_words(Fr::from_u32(5), e);
    for (unsigned i = log_n; i < 28; i++) w = w.sqr();
    return w;
}
// out[k] = sum_i w^(ik) a[i]
static std::vector<Fr> naive_transform(const std::vector<Fr> &a, const Fr &w) {
    const size_t n = a.size();
    std::vector<Fr> out(n, Fr::zero());
    for (size_t k = 0; k < n; k++)
        for (size_t i = 0; i < n; i++) out[k] = out[k] + fr_pow_u(w, (uint64_t)i * k) * a[i];
    return out;
}

// ---------------------------------------------------------------- per-group glue
template <class F>
static Jac<F> plain_mul(const Jac<F> &P, const Fr &k) {
    uint32_t w[8];
    k.to_canonical(w);
    Jac<F> acc = Jac<F>::inf();
    for (int i = 255; i >= 0; --i) {
        acc = jac_dbl(acc);
        if ((w[i >> 5] >> (i & 31)) & 1) acc = jac_add(acc, P);
    }
    return acc;
}
template <class F>
static bool same_point(const Jac<F> &a, const Jac<F> &b) {
    if (a.is_inf() || b.is_inf()) return a.is_inf() && b.is_inf();
    const Jac<F> x = jac_normalize(a), y = jac_normalize(b);
    return x.X == y.X && x.Y == y.Y;
}
struct G1 {
    using F = Fq;
    using Aff = Aff29;
    using Acc = XYZZ29;
    static constexpr int TBL = SMUL_TBL;
    static const char *name() { return "G1"; }
    static Jac<Fq> gen() { const Fq one = Fq::one(); return {one, one + one, one}; }
    static Aff to_affine(const Jac<Fq> &P) {                           // what prepare_bases hands the stage kernel
        if (P.is_inf()) return {F29::zero(), F29::zero()};
        const Jac<Fq> n = jac_normalize(P);
        return {F29::from_mont256(n.X).canonical(), F29::from_mont256(n.Y).canonical()};
    }
    static Jac<Fq> to_jac(const Acc &a) { return xyzz29_to_jac(a); }
};
struct G2 {
    using F = Fq2;
    using Aff = Aff29x2;
    using Acc = XYZZ29x2;
    static constexpr int TBL = SMUL_G2_TBL;
    static const char *name() { return "G2"; }
    static Jac<Fq2> gen() { return {fq2_const(LSA_G2_GEN_X), fq2_const(LSA_G2_GEN_Y), Fq2::one()}; }
    static Aff to_affine(const Jac<Fq2> &P) {
        if (P.is_inf()) return {F29x2::zero(), F29x2::zero()};
        const Jac<Fq2> n = jac_normalize(P);
        return {f29x2_from_mont256(n.X).canonical(), f29x2_from_mont256(n.Y).canonical()};
    }
    static Jac<Fq2> to_jac(const Acc &a) { return g2_to_jac(a); }
};

// the transform as ecntt.hip's ecntt_device runs it
template <class G>
static std::vector<Jac<typename G::F>> run_transform(const std::vector<Jac<typename G::F>> &in, unsigned log_n, const Fr &omega, bool inverse) {
    using P = Jac<typename G::F>;
    const size_t n = (size_t)1 << log_n, half_n = n / 2;
    if (log_n == 0) return in;
    typename G::Acc T[G::TBL];
    const Fr w = inverse ? omega.inverse() : omega;
    std::vector<Fr> tw(half_n ? half_n : 1, Fr::one());
    for (size_t t = 1; t < half_n; t++) tw[t] = tw[t - 1] * w;
    std::vector<P> src = in, dst(n);
    if (inverse) {
        uint32_t c[8];
        Fr::from_u32((uint32_t)n).inverse().to_canonical(c);
        for (size_t i = 0; i < n; i++) src[i] = G::to_jac(ecntt_twiddled(G::to_affine(in[i]), c, false, T));
    }
    for (unsigned s = 1; s <= log_n; s++) {
        for (size_t b = 0; b < half_n; b++) {
            const EcnttBfly f = ecntt_bfly(log_n, s, b);
            typename G::Acc t, sum, diff;
            if (s == 1) t = ecntt_from_jac(src[f.src_b]);
            else {
                uint32_t k[8];
                tw[f.tw].to_canonical(k);
                t = ecntt_twiddled(G::to_affine(src[f.src_b]), k, f.tw == 0, T);
            }
            ecntt_combine(ecntt_from_jac(src[f.src_a]), t, sum, diff);
            dst[f.dst_a] = G::to_jac(sum);
            dst[f.dst_b] = G::to_jac(diff);
        }
        src.swap(dst);
    }
    return src;
}

template <class G>
static int check_transform(const std::vector<Fr> &a, unsigned log_n, const char *what, std::mt19937_64 &rng) {
    using F = typename G::F;
    const size_t n = a.size();
    const Fr omega = root_of_unity(log_n);
    int fails = 0;
    std::vector<Jac<F>> in(n);
    for (size_t i = 0; i < n; i++) {
        in[i] = plain_mul(G::gen(), a[i]);
        if (!in[i].is_inf() && (rng() & 1)) in[i] = jac_add(jac_dbl(in[i]), jac_neg(in[i]));   // the same point, Z != 1
    }
    for (int inverse = 0; inverse < 2; inverse++) {
        std::vector<Fr> want = naive_transform(a, inverse ? omega.inverse() : omega);
        if (inverse) for (auto &x : want) x = x * Fr::from_u32((uint32_t)n).inverse();
        const std::vector<Jac<F>> got = run_transform<G>(in, log_n, omega, inverse != 0);
        for (size_t k = 0; k < n; k++)
            if (!same_point(got[k], plain_mul(G::gen(), want[k]))) {
                if (fails < 8) printf("%s %s n=%zu %s: wrong point at k=%zu\n", G::name(), what, n, inverse ? "inverse" : "forward", k);
                fails++;
            }
    }
    return fails;
}

template <class G>
static int check_group(std::mt19937_64 &rng) {
    int fails = 0, transforms = 0;
    for (unsigned log_n : {0u, 1u, 2u, 4u}) {
        const size_t n = (size_t)1 << log_n;
        const Fr omega = root_of_unity(log_n);
        std::vector<Fr> a(n);
        for (auto &x : a) {
            uint32_t w[8];
            for (int i = 0; i < 8; i++) w[i] = (uint32_t)rng();
            w[7] &= 0x0fffffffu;                                        // < 2^252 < r
            x = Fr::from_canonical(w);
        }
        if (n >= 4) { a[1] = Fr::zero(); a[n - 1] = Fr::one(); a[2] = Fr::zero() - Fr::one(); }
        fails += check_transform<G>(a, log_n, "random", rng);
        // the degenerate inputs: all equal (stage 1 doubles and cancels in every butterfly), one point, pure frequencies
        const Fr c = Fr::from_u32(7);
        fails += check_transform<G>(std::vector<Fr>(n, c), log_n, "all equal", rng);
        std::vector<Fr> one(n, Fr::zero());
        one[0] = c;
        fails += check_transform<G>(one, log_n, "(P, O, ..., O)", rng);
        transforms += 3;
        if (n >= 4)
            for (size_t k0 : {(size_t)1, n / 2, n - 1}) {
                std::vector<Fr> f(n);
                const Fr winv = omega.inverse();
                for (size_t i = 0; i < n; i++) f[i] = c * fr_pow_u(winv, (uint64_t)i * k0);
                fails += check_transform<G>(f, log_n, "pure frequency", rng);
                transforms++;
            }
    }
    printf("%s: %d inputs, forward and inverse, n = 1, 2, 4, 16\n", G::name(), transforms);
    return fails;
}

// ---------------------------------------------------------------- geometry
static int check_geometry() {
    int fails = 0;
    auto bad = [&](unsigned log_n, unsigned s, const char *what) { if (fails++ < 10) printf("geometry log_n=%u stage %u: %s\n", log_n, s, what); };
    for (unsigned log_n = 1; log_n <= 10; log_n++) {
        const size_t n = (size_t)1 << log_n, half_n = n / 2;
        std::vector<size_t> where(n), next(n);                        // slot -> element, as the previous stage wrote it
        for (unsigned s = 1; s <= log_n; s++) {
            const size_t half = (size_t)1 << (s - 1), groups = n >> s;
            std::vector<char> seen_e(n, 0), seen_src(n, 0), seen_dst(n, 0);
            size_t prev_tw = 0;
            for (size_t b = 0; b < half_n; b++) {
                const EcnttBfly f = ecntt_bfly(log_n, s, b);
                if (f.ea >= n || f.eb >= n || f.src_a >= n || f.src_b >= n || f.dst_a >= n || f.dst_b >= n || f.tw >= (half_n ? half_n : 1)) { bad(log_n, s, "index out of range"); continue; }
                if (f.eb != f.ea + half || ((f.ea >> (s - 1)) & 1)) bad(log_n, s, "not a pair of the network");
                if (f.tw != (f.ea & (half - 1)) * groups) bad(log_n, s, "twiddle index is not j n / 2^s");
                if (seen_e[f.ea]++ || seen_e[f.eb]++) bad(log_n, s, "an element is used twice");
                if (seen_src[f.src_a]++ || seen_src[f.src_b]++) bad(log_n, s, "a source slot is read twice");
                if (seen_dst[f.dst_a]++ || seen_dst[f.dst_b]++) bad(log_n, s, "a destination slot is written twice");
                if (s == 1) {
                    if (f.src_a != ecntt_bitrev(f.ea, log_n) || f.src_b != ecntt_bitrev(f.eb, log_n)) bad(log_n, s, "stage 1 does not read the bit-reversed input");
                } else {
                    if (f.src_a != b || f.src_b != half_n + b) bad(log_n, s, "operands are not at b and n/2 + b");
                    if (where[f.src_a] != f.ea || where[f.src_b] != f.eb) bad(log_n, s, "reads what the previous stage did not write there");
                    if (f.src_a != ecntt_slot(log_n, s, f.ea) || f.src_b != ecntt_slot(log_n, s, f.eb)) bad(log_n, s, "ecntt_slot disagrees");
                }
                if (s == log_n && (f.dst_a != f.ea || f.dst_b != f.eb)) bad(log_n, s, "the last stage does not write natural order");
                if (f.tw < prev_tw) bad(log_n, s, "butterflies are not ordered by j");
                if ((f.tw == 0) != (b < groups)) bad(log_n, s, "the twiddle-1 butterflies are not the first n / 2^s");
                prev_tw = f.tw;
                next[f.dst_a] = f.ea;
                next[f.dst_b] = f.eb;
            }
            for (size_t i = 0; i < n; i++)
                if (!seen_e[i] || !seen_src[i] || !seen_dst[i]) { bad(log_n, s, "not a partition"); break; }
            where.swap(next);
        }
    }
    for (unsigned log_n = 1; log_n <= 10; log_n++)
        for (size_t e = 0; e < ((size_t)1 << log_n); e++)
            if (ecntt_bitrev(ecntt_bitrev(e, log_n), log_n) != e) { bad(log_n, 0, "bitrev is not an involution"); break; }
    printf("geometry: log_n = 1 .. 10\n");
    return fails;
}

int main() {
    int fails = 0;
    for (unsigned log_n : {0u, 1u, 2u, 4u, 10u, 24u}) {                 // the roots themselves
        Fr w = root_of_unity(log_n);
        for (unsigned i = 1; i < log_n; i++) w = w.sqr();
        if (log_n == 0 ? w != Fr::one() : w != Fr::zero() - Fr::one()) { printf("root_of_unity(%u) is not primitive\n", log_n); fails++; }
    }
    fails += check_geometry();
    std::mt19937_64 rng(2025);
    fails += check_group<G1>(rng);
    fails += check_group<G2>(rng);
    printf(fails ? "FAILED (%d)\n" : "PASS\n", fails);
    return fails ? 1 : 0;
}
