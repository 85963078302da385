// tools/paired_check.hip -- the paired products of fp29.h (mul2, sqr2) and the G1 point formulas built on them
// (xyzz29_madd_signed, xyzz29_add_affine, xyzz29_add_paired) run on the device and compared on the host: the products limb for limb with
// mul / sqr, the points limb for limb with the host's own evaluation of the same formula (which runs the single forms)
// and, as canonical affine points, with the plain xyzz29_madd on an explicitly negated base / the plain xyzz29_add.
// Prints one line per group and "PASS" or "FAIL"; exit status 0 only when everything agrees.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I legosnark_amd/csrc tools/paired_check.hip -o paired_check
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <random>
#include <vector>
#include "fp29.h"
#include "inv29.h"

using namespace lsa;

#define HIP_OK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { printf("FAIL %s: %s (line %d)\n", #e, hipGetErrorString(e_), __LINE__); return 2; } } while (0)

struct MadCase { XYZZ29 acc; Aff29 base; uint32_t neg; };
struct HeadCase { Aff29 a, b; uint32_t neg; };
struct AddCase { XYZZ29 a, b; };

// in: 4 operands per item (a0, b0, a1, b1); out: 4 results per item (mul2.a, mul2.b, sqr2(a0, a1).a, sqr2(a0, a1).b)
__global__ __launch_bounds__(64) void k_fields(const F29 *__restrict__ in, F29 *__restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const F29 a0 = in[4 * (size_t)t], b0 = in[4 * (size_t)t + 1], a1 = in[4 * (size_t)t + 2], b1 = in[4 * (size_t)t + 3];
    const F29Pair m = mul2(a0, b0, a1, b1), s = sqr2(a0, a1);
    out[4 * (size_t)t] = m.a; out[4 * (size_t)t + 1] = m.b; out[4 * (size_t)t + 2] = s.a; out[4 * (size_t)t + 3] = s.b;
}
__global__ __launch_bounds__(64) void k_madd(const MadCase *__restrict__ in, XYZZ29 *__restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    out[t] = xyzz29_madd_signed(in[t].acc, in[t].base, lsa_mask(in[t].neg ? ~0u : 0u));
}
__global__ __launch_bounds__(64) void k_add(const AddCase *__restrict__ in, XYZZ29 *__restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    out[t] = xyzz29_add_paired(in[t].a, in[t].b);
}
__global__ __launch_bounds__(64) void k_head(const HeadCase *__restrict__ in, XYZZ29 *__restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    out[t] = xyzz29_add_affine(in[t].a, in[t].b, lsa_mask(in[t].neg ? ~0u : 0u));
}

static std::mt19937_64 rng(20261019);
static bool eq(const F29 &a, const F29 &b) { return memcmp(a.l, b.l, sizeof a.l) == 0; }
static bool eq(const XYZZ29 &a, const XYZZ29 &b) { return eq(a.X, b.X) && eq(a.Y, b.Y) && eq(a.ZZ, b.ZZ) && eq(a.ZZZ, b.ZZZ); }
// canonical affine coordinates (X / ZZ, Y / ZZZ, each in [0, p)) of a finite point
static Aff29 affine(const XYZZ29 &a) { return {mul(a.X, f29_inverse(a.ZZ)).canonical(), mul(a.Y, f29_inverse(a.ZZZ)).canonical()}; }
// equal as points: both infinity, or the same canonical affine coordinates
static bool same_point(const XYZZ29 &a, const XYZZ29 &b) {
    if (a.is_inf() || b.is_inf()) return a.is_inf() && b.is_inf();
    const Aff29 p = affine(a), q = affine(b);
    return eq(p.x, q.x) && eq(p.y, q.y);
}
static F29 k_times_p(uint32_t k, int minus) {          // k*p - minus in tight limbs (k*p >= minus)
    F29 r;
    uint64_t c = 0;
    for (int i = 0; i < 9; i++) { c += (uint64_t)F29::p(i) * k; r.l[i] = i < 8 ? (uint32_t)c & F29::MASK : (uint32_t)c; c >>= 29; }
    int64_t b = -minus;
    for (int i = 0; i < 9 && b != 0; i++) { int64_t v = (int64_t)r.l[i] + b; if (i < 8) { r.l[i] = (uint32_t)v & F29::MASK; b = v >> 29; } else r.l[i] = (uint32_t)v; }
    return r;
}
static F29 all_limbs(uint32_t v) { F29 r; for (int i = 0; i < 9; i++) r.l[i] = v; return r; }
static F29 rand_tight() { F29 r; for (int i = 0; i < 9; i++) r.l[i] = (uint32_t)rng() & (i == 8 ? 0x3fffffu : F29::MASK); return r; }
static Aff29 rand_base() {                             // k*G by double-and-add from G = (1, 2), canonical
    const Aff29 g{F29::from_mont256(Fq::from_u32(1)).canonical(), F29::from_mont256(Fq::from_u32(2)).canonical()};
    const uint64_t k = rng() | (1ull << 63);
    XYZZ29 acc = XYZZ29::inf();
    for (int i = 63; i >= 0; i--) { acc = xyzz29_dbl(acc); if ((k >> i) & 1) acc = xyzz29_madd(acc, g); }
    return affine(acc);
}
static Aff29 negated(const Aff29 &b) { return {b.x, sub_k<1>(F29::zero(), b.y)}; }
// an accumulator with ZZ, ZZZ != 1 that equals the affine point q: 2q + (-q)
static XYZZ29 acc_equal_to(const Aff29 &q) { return xyzz29_madd(xyzz29_dbl_affine(q), negated(q)); }

int main() {
    int fails = 0;
    // ---- products ----
    std::vector<F29> tight = {F29::zero(), k_times_p(0, -1), k_times_p(1, 1), k_times_p(1, 0), k_times_p(2, 1), k_times_p(11, 0), all_limbs(F29::MASK)};
    std::vector<F29> in;
    for (const F29 &a : tight) for (const F29 &b : tight) {              // every pair of the extremes, beside its mirror
        in.push_back(a); in.push_back(b); in.push_back(b); in.push_back(a);
    }
    // limbs 2^30 - 1, the loose bound of sqr, beside every tight extreme and beside itself (mul takes such limbs too: its
    // limb products stay <= 2^60; only its value bound is exceeded, and the comparison is of the same integers)
    const F29 loose = all_limbs((1u << 30) - 1);
    for (const F29 &a : tight) { in.push_back(loose); in.push_back(a); in.push_back(a); in.push_back(loose); in.push_back(a); in.push_back(loose); in.push_back(loose); in.push_back(a); }
    in.push_back(loose); in.push_back(loose); in.push_back(loose); in.push_back(loose);
    const size_t n_ext = in.size() / 4;
    for (int i = 0; i < 4096; i++) for (int j = 0; j < 4; j++) in.push_back(rand_tight());
    const uint32_t nf = (uint32_t)(in.size() / 4);
    {
        F29 *d_in, *d_out;
        std::vector<F29> out(in.size());
        HIP_OK(hipMalloc(&d_in, in.size() * sizeof(F29))); HIP_OK(hipMalloc(&d_out, in.size() * sizeof(F29)));
        HIP_OK(hipMemcpy(d_in, in.data(), in.size() * sizeof(F29), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_fields, dim3((nf + 63) / 64), dim3(64), 0, 0, d_in, d_out, nf);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(out.data(), d_out, in.size() * sizeof(F29), hipMemcpyDeviceToHost));
        int bad_mul = 0, bad_sqr = 0;
        for (uint32_t t = 0; t < nf; t++) {
            const F29 &a0 = in[4 * t], &b0 = in[4 * t + 1], &a1 = in[4 * t + 2], &b1 = in[4 * t + 3];
            if (!(eq(out[4 * t], mul(a0, b0)) && eq(out[4 * t + 1], mul(a1, b1)))) bad_mul++;
            if (!(eq(out[4 * t + 2], sqr(a0)) && eq(out[4 * t + 3], sqr(a1)))) bad_sqr++;
        }
        printf("products: %u items (%zu extremes, 4096 random): mul2 differs in %d, sqr2 in %d\n", nf, n_ext, bad_mul, bad_sqr);
        fails += bad_mul + bad_sqr;
        HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_out));
    }
    // ---- the mixed addition ----
    {
        std::vector<MadCase> c;
        for (int i = 0; i < 64 * 8; i++) {                               // random accumulators and bases, both signs
            XYZZ29 acc = xyzz29_madd(xyzz29_dbl_affine(rand_base()), rand_base());
            if (i & 2) acc = xyzz29_madd(acc, rand_base());
            c.push_back({acc, rand_base(), (uint32_t)(i & 1)});
        }
        const size_t n_rand = c.size();
        for (int s = 0; s < 2; s++) {                                    // the degenerate lanes, both signs
            const Aff29 q = rand_base();
            c.push_back({XYZZ29::inf(), q, (uint32_t)s});                                    // accumulator at infinity
            c.push_back({acc_equal_to(s ? negated(q) : q), q, (uint32_t)s});                 // doubling
            c.push_back({acc_equal_to(s ? q : negated(q)), q, (uint32_t)s});                 // cancellation
            c.push_back({{q.x, s ? negated(q).y : q.y, F29::one(), F29::one()}, q, (uint32_t)s});   // doubling, ZZ = 1
        }
        const uint32_t n = (uint32_t)c.size();
        MadCase *d_in; XYZZ29 *d_out;
        std::vector<XYZZ29> out(n);
        HIP_OK(hipMalloc(&d_in, n * sizeof(MadCase))); HIP_OK(hipMalloc(&d_out, n * sizeof(XYZZ29)));
        HIP_OK(hipMemcpy(d_in, c.data(), n * sizeof(MadCase), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_madd, dim3((n + 63) / 64), dim3(64), 0, 0, d_in, d_out, n);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(out.data(), d_out, n * sizeof(XYZZ29), hipMemcpyDeviceToHost));
        int bad_limbs = 0, bad_point = 0, inf = 0;
        for (uint32_t t = 0; t < n; t++) {
            if (!eq(out[t], xyzz29_madd_signed(c[t].acc, c[t].base, c[t].neg ? ~0u : 0u))) bad_limbs++;
            if (!same_point(out[t], xyzz29_madd(c[t].acc, c[t].neg ? negated(c[t].base) : c[t].base))) bad_point++;
            inf += out[t].is_inf();
        }
        printf("mixed addition: %u lanes (%zu random, %zu degenerate, %d results at infinity): limbs differ in %d, points in %d\n",
               n, n_rand, c.size() - n_rand, inf, bad_limbs, bad_point);
        if (inf != 2) { printf("FAIL expected exactly the two cancellations at infinity\n"); fails++; }
        fails += bad_limbs + bad_point;
        HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_out));
    }
    // ---- the head: affine + affine ----
    {
        std::vector<HeadCase> c;
        for (int i = 0; i < 64 * 8; i++) {
            Aff29 a = rand_base();
            if (i & 2) a = negated(a);                                   // the first entry carries its own sign
            c.push_back({a, rand_base(), (uint32_t)(i & 1)});
        }
        const size_t n_rand = c.size();
        for (int s = 0; s < 2; s++) {
            const Aff29 q = rand_base();
            c.push_back({s ? negated(q) : q, q, (uint32_t)s});           // doubling
            c.push_back({s ? q : negated(q), q, (uint32_t)s});           // cancellation
        }
        const uint32_t n = (uint32_t)c.size();
        HeadCase *d_in; XYZZ29 *d_out;
        std::vector<XYZZ29> out(n);
        HIP_OK(hipMalloc(&d_in, n * sizeof(HeadCase))); HIP_OK(hipMalloc(&d_out, n * sizeof(XYZZ29)));
        HIP_OK(hipMemcpy(d_in, c.data(), n * sizeof(HeadCase), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_head, dim3((n + 63) / 64), dim3(64), 0, 0, d_in, d_out, n);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(out.data(), d_out, n * sizeof(XYZZ29), hipMemcpyDeviceToHost));
        int bad_limbs = 0, bad_point = 0, inf = 0;
        for (uint32_t t = 0; t < n; t++) {
            if (!eq(out[t], xyzz29_add_affine(c[t].a, c[t].b, c[t].neg ? ~0u : 0u))) bad_limbs++;
            const XYZZ29 a1{c[t].a.x, c[t].a.y, F29::one(), F29::one()};
            if (!same_point(out[t], xyzz29_madd(a1, c[t].neg ? negated(c[t].b) : c[t].b))) bad_point++;
            inf += out[t].is_inf();
        }
        printf("head: %u lanes (%zu random, %zu degenerate, %d results at infinity): limbs differ in %d, points in %d\n",
               n, n_rand, c.size() - n_rand, inf, bad_limbs, bad_point);
        if (inf != 2) { printf("FAIL expected exactly the two cancellations at infinity\n"); fails++; }
        fails += bad_limbs + bad_point;
        HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_out));
    }
    // ---- the general addition of the tail ----
    {
        std::vector<AddCase> c;
        auto rand_acc = [&](int i) {
            XYZZ29 acc = xyzz29_madd(xyzz29_dbl_affine(rand_base()), rand_base());
            if (i & 1) acc = xyzz29_add(acc, xyzz29_dbl(acc));
            return acc;
        };
        for (int i = 0; i < 64 * 8; i++) c.push_back({rand_acc(i), rand_acc(i >> 1)});
        const size_t n_rand = c.size();
        for (int s = 0; s < 2; s++) {
            const Aff29 q = rand_base();
            const XYZZ29 a = acc_equal_to(q), a1{q.x, q.y, F29::one(), F29::one()}, na = xyzz29_neg(a);
            c.push_back({XYZZ29::inf(), a});                             // either side at infinity, both
            c.push_back({a, XYZZ29::inf()});
            c.push_back({XYZZ29::inf(), XYZZ29::inf()});
            c.push_back({a, a1});                                        // doubling: the same point in two representations
            c.push_back({a1, a});
            c.push_back({a, a});
            c.push_back({na, a1});                                       // cancellation
            c.push_back({a, na});
        }
        const uint32_t n = (uint32_t)c.size();
        AddCase *d_in; XYZZ29 *d_out;
        std::vector<XYZZ29> out(n);
        HIP_OK(hipMalloc(&d_in, n * sizeof(AddCase))); HIP_OK(hipMalloc(&d_out, n * sizeof(XYZZ29)));
        HIP_OK(hipMemcpy(d_in, c.data(), n * sizeof(AddCase), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_add, dim3((n + 63) / 64), dim3(64), 0, 0, d_in, d_out, n);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(out.data(), d_out, n * sizeof(XYZZ29), hipMemcpyDeviceToHost));
        int bad_limbs = 0, bad_point = 0, inf = 0;
        for (uint32_t t = 0; t < n; t++) {
            const XYZZ29 want = xyzz29_add(c[t].a, c[t].b);
            if (!eq(out[t], want) || !eq(out[t], xyzz29_add_paired(c[t].a, c[t].b))) bad_limbs++;
            if (!same_point(out[t], want)) bad_point++;
            inf += out[t].is_inf();
        }
        printf("general addition: %u lanes (%zu random, %zu degenerate, %d results at infinity): limbs differ in %d, points in %d\n",
               n, n_rand, c.size() - n_rand, inf, bad_limbs, bad_point);
        if (inf != 6) { printf("FAIL expected infinity + infinity and the two cancellations, twice\n"); fails++; }
        fails += bad_limbs + bad_point;
        HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_out));
    }
    printf(fails ? "FAIL\n" : "PASS\n");
    return fails ? 1 : 0;
}
