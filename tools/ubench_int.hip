// tools/ubench_int.hip -- instruction-throughput microbenchmark that decides how the
// 254-bit field multiplication is built on gfx950 (DESIGN.md "field multiplication").
// Measures wave-level issue rates of the candidate building blocks:
//   v_mad_u64_u32 (32x32+64), v_mul_lo_u32 / v_mul_hi_u32, v_mad_u32_u24,
//   v_add_co/v_addc, v_lshl_add_u64, v_fma_f64, and the library's Fq product;
//   and N products stepped side by side in one accumulator chain each, against N calls of mul() (DESIGN.md,
//   "Paired single-chain products": the form fp29.h uses was chosen here).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I legosnark_amd/csrc tools/ubench_int.hip -o /tmp/ubench_int
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <utility>
#include <vector>
#include "fp.h"
#include "fp29.h"

using namespace lsa;

#define CHAINS 8

template <int OP>
__global__ __launch_bounds__(256) void k_op(uint32_t *out, uint32_t seed, int iters) {
    uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t a[CHAINS];
    uint32_t b = seed * 2654435761u + tid * 40503u + 1u;
    double d[CHAINS];
#pragma unroll
    for (int c = 0; c < CHAINS; c++) { a[c] = (uint64_t)(tid + c) * 0x9E3779B97F4A7C15ull + seed; d[c] = 1.0 + (double)(tid + c) * 1e-9; }
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int c = 0; c < CHAINS; c++) {
            if (OP == 0) {            // v_mad_u64_u32
                a[c] = (uint64_t)(uint32_t)a[c] * b + a[c];
            } else if (OP == 1) {     // v_mul_lo_u32
                a[c] = (uint32_t)a[c] * b;
            } else if (OP == 2) {     // v_mul_hi_u32
                a[c] = __umulhi((uint32_t)a[c], b);
            } else if (OP == 3) {     // v_mad_u32_u24
                a[c] = __umul24((uint32_t)a[c], b) + (uint32_t)(a[c] >> 3);
            } else if (OP == 4) {     // 64-bit add (v_lshl_add_u64 or add_co/addc)
                a[c] = a[c] + ((uint64_t)b << 7) + it;
            } else if (OP == 5) {     // v_fma_f64
                d[c] = __builtin_fma(d[c], 1.0000001, 1e-7);
            } else if (OP == 6) {     // 32-bit add3
                a[c] = (uint32_t)a[c] + b + (uint32_t)it;
            }
        }
    }
    uint64_t s = 0;
#pragma unroll
    for (int c = 0; c < CHAINS; c++) s += a[c] + (uint64_t)d[c];
    out[tid] = (uint32_t)s ^ (uint32_t)(s >> 32);
}

template <bool INLINE>
__global__ __launch_bounds__(256) void k_fqmul(Fq *out, const Fq *in, int iters) {
    uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    Fq x = in[tid], y = in[tid + 1];
    for (int it = 0; it < iters; it++) {
        if (INLINE) { x = Fq::mul_inline(x, y); y = Fq::mul_inline(y, x); }
        else { x = x * y; y = y * x; }
    }
    out[tid] = x + y;
}

template <int ILP>
__global__ __launch_bounds__(256) void k_mul29(F29 *out, const F29 *in, int iters) {
    uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    F29 x[ILP], y = in[tid + 1];
#pragma unroll
    for (int j = 0; j < ILP; j++) { x[j] = in[tid]; x[j].l[0] ^= j; }
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int j = 0; j < ILP; j++) x[j] = mul(x[j], y);      // ILP independent dependent-chains
    }
    F29 r = x[0];
#pragma unroll
    for (int j = 1; j < ILP; j++) r = add_lazy(r, x[j]);
    out[tid] = r;
}

// ---- N products stepped column by column side by side, each in ONE 64-bit accumulator chain ----
// mul() as compiled opens every column in a fresh accumulator and re-adds the shifted carry (16 v_lshl_add_u64 per
// product); a single chain has no re-adds.  The multiply-add step of a chain, in the candidate forms:
// (a) inline v_mad_u64_u32, carry-out to vcc (a constant limb of p in an SGPR, as the compiler keeps it)
struct MacAsmVcc {
    static LSA_HD void mac(uint64_t &acc, uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b) : "vcc");
#endif
    }
    static LSA_HD void mac_c(uint64_t &acc, uint32_t a, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(a), "s"(c) : "vcc");
#endif
    }
};
// (b) the same with the carry-out to an SGPR pair
struct MacAsmSgpr {
    static LSA_HD void mac(uint64_t &acc, uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
        uint64_t co;
        asm volatile("v_mad_u64_u32 %0, %1, %2, %3, %0" : "+v"(acc), "=s"(co) : "v"(a), "v"(b));
#endif
    }
    static LSA_HD void mac_c(uint64_t &acc, uint32_t a, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
        uint64_t co;
        asm volatile("v_mad_u64_u32 %0, %1, %2, %3, %0" : "+v"(acc), "=s"(co) : "v"(a), "s"(c));
#endif
    }
};
// (c) plain C++ with an opaque barrier behind every step: source order is the interleaving
struct MacBarrier {
    static LSA_HD void mac(uint64_t &acc, uint32_t a, uint32_t b) {
        acc += (uint64_t)a * b;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(acc));
#endif
    }
    static LSA_HD void mac_c(uint64_t &acc, uint32_t a, uint32_t c) { mac(acc, a, c); }
};
// (c) without "volatile": every chain keeps its order, the scheduler places the chains against each other
struct MacBarrierFree {
    static LSA_HD void mac(uint64_t &acc, uint32_t a, uint32_t b) {
        acc += (uint64_t)a * b;
#if defined(__HIP_DEVICE_COMPILE__)
        asm("" : "+v"(acc));
#endif
    }
    static LSA_HD void mac_c(uint64_t &acc, uint32_t a, uint32_t c) { mac(acc, a, c); }
};
// (c) with the scheduler pinned as well.  The hazard recognizer takes an asm statement, an empty one too, for a producer whose
// result the next VALU instruction may not read without a wait state, and the scheduler is free to move the multiply-adds past
// the empty statements: it emits A, B, asm, asm, s_nop, A, ...  With a scheduling barrier behind every step the order is the
// source's -- A, asm, B, asm, A -- and the neighbour's step is the wait state.
struct MacBarrierPinned {
    static LSA_HD void mac(uint64_t &acc, uint32_t a, uint32_t b) {
        acc += (uint64_t)a * b;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(acc));
        __builtin_amdgcn_sched_barrier(0);
#endif
    }
    static LSA_HD void mac_c(uint64_t &acc, uint32_t a, uint32_t c) { mac(acc, a, c); }
};
// x[j] = x[j] * y for j < N, the same column sums as mul() (so the same limbs).  The column index is a template parameter:
// every limb index is a constant before anything is unrolled.
template <class Mac, int N>
struct ChainN {
    uint64_t acc[N];
    uint32_t m[N][9];
    template <int K>
    LSA_HD void column(const F29 (&x)[N], const F29 &y, F29 (&r)[N]) {
#pragma unroll
        for (int i = (K < 9 ? 0 : K - 8); i < (K < 9 ? K + 1 : 9); i++)
#pragma unroll
            for (int j = 0; j < N; j++) Mac::mac(acc[j], x[j].l[i], y.l[K - i]);
#pragma unroll
        for (int i = (K < 9 ? 0 : K - 8); i < (K < 9 ? K : 9); i++)
#pragma unroll
            for (int j = 0; j < N; j++) Mac::mac_c(acc[j], m[j][i], F29::p(K - i));
#pragma unroll
        for (int j = 0; j < N; j++) {
            if (K < 9) m[j][K < 9 ? K : 0] = ((uint32_t)acc[j] * F29::PINV) & F29::MASK;
            else r[j].l[K < 9 ? 0 : K - 9] = (uint32_t)acc[j] & F29::MASK;
        }
        if (K < 9) {
#pragma unroll
            for (int j = 0; j < N; j++) Mac::mac_c(acc[j], m[j][K < 9 ? K : 0], F29::p(0));
        }
#pragma unroll
        for (int j = 0; j < N; j++) acc[j] >>= 29;
    }
    template <int... K>
    LSA_HD void run(F29 (&x)[N], const F29 &y, std::integer_sequence<int, K...>) {
#pragma unroll
        for (int j = 0; j < N; j++) acc[j] = 0;
        F29 r[N];
        (column<K>(x, y, r), ...);
#pragma unroll
        for (int j = 0; j < N; j++) { r[j].l[8] = (uint32_t)acc[j]; x[j] = r[j]; }
    }
};
// the loop of k_mul29<N> with the N products of an iteration stepped together
template <class Mac, int N>
__global__ __launch_bounds__(256) void k_mul29_chains(F29 *out, const F29 *in, int iters) {
    uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    F29 x[N], y = in[tid + 1];
#pragma unroll
    for (int j = 0; j < N; j++) { x[j] = in[tid]; x[j].l[0] ^= j; }
    for (int it = 0; it < iters; it++) {
        ChainN<Mac, N> c;
        c.run(x, y, std::make_integer_sequence<int, 17>{});
    }
    F29 r = x[0];
#pragma unroll
    for (int j = 1; j < N; j++) r = add_lazy(r, x[j]);
    out[tid] = r;
}

template <class Fn>
static float time_ms(Fn fn, int reps = 3) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    fn();
    hipDeviceSynchronize();
    float best = 1e30f;
    for (int r = 0; r < reps; r++) {
        hipEventRecord(e0);
        fn();
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        if (ms < best) best = ms;
    }
    return best;
}

int main() {
    hipDeviceProp_t prop;
    hipGetDeviceProperties(&prop, 0);
    printf("device: %s, CUs=%d, clock=%d kHz\n", prop.gcnArchName, prop.multiProcessorCount, prop.clockRate);
    const int blocks = prop.multiProcessorCount * 8, threads = 256, iters = 4096;
    uint32_t *d_out;
    hipMalloc(&d_out, (size_t)blocks * threads * 4);
    const char *names[] = {"v_mad_u64_u32", "v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u32_u24", "add_u64", "v_fma_f64", "add3_u32"};
    double total = (double)blocks * threads * iters * CHAINS;
#define RUN(OP) { float ms = time_ms([&] { hipLaunchKernelGGL((k_op<OP>), dim3(blocks), dim3(threads), 0, 0, d_out, 7u, iters); }); \
                  printf("%-16s %8.3f ms  %8.2f Gop/s  (%.2f lane-ops/clk/CU at %.2f GHz)\n", names[OP], ms, total / ms * 1e-6, \
                         total / (ms * 1e-3) / prop.multiProcessorCount / (prop.clockRate * 1e3), prop.clockRate * 1e-6); }
    RUN(0) RUN(1) RUN(2) RUN(3) RUN(4) RUN(5) RUN(6)
    // field multiplication
    {
        size_t n = (size_t)blocks * threads;
        std::vector<Fq> h(n + 1);
        for (size_t i = 0; i <= n; i++) for (int j = 0; j < 8; j++) h[i].l[j] = (uint32_t)(i * 2654435761u + j * 40503u + 12345u) & (j == 7 ? 0x0fffffffu : 0xffffffffu);
        Fq *d_in, *d_o;
        hipMalloc(&d_in, (n + 1) * sizeof(Fq)); hipMalloc(&d_o, n * sizeof(Fq));
        hipMemcpy(d_in, h.data(), (n + 1) * sizeof(Fq), hipMemcpyHostToDevice);
        const int fi = 512;
        for (int occ = 1; occ <= 8; occ *= 2) {
            int bl = prop.multiProcessorCount * occ;
            double muls = (double)bl * threads * fi * 2;
            float ms1 = time_ms([&] { hipLaunchKernelGGL((k_fqmul<true>), dim3(bl), dim3(threads), 0, 0, d_o, d_in, fi); });
            float ms2 = time_ms([&] { hipLaunchKernelGGL((k_fqmul<false>), dim3(bl), dim3(threads), 0, 0, d_o, d_in, fi); });
            printf("Fq mul, %d blocks/CU: inline %8.3f ms = %7.2f Gmul/s | call %8.3f ms = %7.2f Gmul/s\n", occ, ms1, muls / ms1 * 1e-6, ms2, muls / ms2 * 1e-6);
        }
    }
    // 29-bit-limb multiplication: throughput vs occupancy and per-lane ILP
    {
        size_t n = (size_t)prop.multiProcessorCount * 8 * 256;
        std::vector<F29> h(n + 1);
        for (size_t i = 0; i <= n; i++) for (int j = 0; j < 9; j++) h[i].l[j] = (uint32_t)(i * 2654435761u + j * 40503u + 12345u) & (j == 8 ? 0x3fffffu : 0x1fffffffu);
        F29 *d_in, *d_o;
        hipMalloc(&d_in, (n + 1) * sizeof(F29)); hipMalloc(&d_o, n * sizeof(F29));
        hipMemcpy(d_in, h.data(), (n + 1) * sizeof(F29), hipMemcpyHostToDevice);
        const int fi = 512;
        for (int occ = 1; occ <= 8; occ *= 2) {
            int bl = prop.multiProcessorCount * occ;
            double muls = (double)bl * threads * fi;
            float m1 = time_ms([&] { hipLaunchKernelGGL((k_mul29<1>), dim3(bl), dim3(threads), 0, 0, d_o, d_in, fi); });
            float m2 = time_ms([&] { hipLaunchKernelGGL((k_mul29<2>), dim3(bl), dim3(threads), 0, 0, d_o, d_in, fi); });
            float m4 = time_ms([&] { hipLaunchKernelGGL((k_mul29<4>), dim3(bl), dim3(threads), 0, 0, d_o, d_in, fi); });
            printf("F29 mul, %d waves/SIMD: ILP1 %7.2f Gmul/s | ILP2 %7.2f Gmul/s | ILP4 %7.2f Gmul/s\n", occ, muls / m1 * 1e-6, 2 * muls / m2 * 1e-6, 4 * muls / m4 * 1e-6);
        }
    }
    // N products side by side in single chains against N calls of mul(): G products/s, slowest and fastest of 7 timed
    // launches (the spread of the benchmark itself); every form first checked limb for limb against mul()
    {
        size_t n = (size_t)prop.multiProcessorCount * 8 * 256;
        std::vector<F29> h(n + 1), want(n), got(n);
        for (size_t i = 0; i <= n; i++) for (int j = 0; j < 9; j++) h[i].l[j] = (uint32_t)(i * 2654435761u + j * 40503u + 12345u) & (j == 8 ? 0x3fffffu : 0x1fffffffu);
        F29 *d_in, *d_o;
        hipMalloc(&d_in, (n + 1) * sizeof(F29)); hipMalloc(&d_o, n * sizeof(F29));
        hipMemcpy(d_in, h.data(), (n + 1) * sizeof(F29), hipMemcpyHostToDevice);
        const int fi = 512, bl8 = prop.multiProcessorCount * 8;
        auto result = [&](auto kernel, std::vector<F29> &dst) {
            hipLaunchKernelGGL(kernel, dim3(bl8), dim3(threads), 0, 0, d_o, d_in, 5);
            hipMemcpy(dst.data(), d_o, n * sizeof(F29), hipMemcpyDeviceToHost);
        };
        auto same = [&](auto kernel) { result(kernel, got); return memcmp(got.data(), want.data(), n * sizeof(F29)) == 0; };
        result(k_mul29<2>, want);
        bool ok = same(k_mul29_chains<MacAsmVcc, 2>) && same(k_mul29_chains<MacAsmSgpr, 2>) && same(k_mul29_chains<MacBarrier, 2>) && same(k_mul29_chains<MacBarrierFree, 2>) && same(k_mul29_chains<MacBarrierPinned, 2>);
        result(k_mul29<3>, want);
        ok = ok && same(k_mul29_chains<MacBarrier, 3>) && same(k_mul29_chains<MacAsmVcc, 3>) && same(k_mul29_chains<MacBarrierPinned, 3>);
        printf("single-chain forms against mul(), 5 iterations, %zu lanes: %s\n", n, ok ? "identical" : "DIFFERENT");
        if (!ok) return 1;
        auto spread = [&](auto kernel, int bl, double muls) {
            float lo = 1e30f, hi = 0.f;
            for (int r = 0; r < 7; r++) {
                float ms = time_ms([&] { hipLaunchKernelGGL(kernel, dim3(bl), dim3(threads), 0, 0, d_o, d_in, fi); }, 1);
                lo = ms < lo ? ms : lo; hi = ms > hi ? ms : hi;
            }
            printf(" %6.2f-%6.2f", muls / hi * 1e-6, muls / lo * 1e-6);
        };
        printf("two products: two mul() | (a) asm, vcc | (b) asm, SGPR pair | (c) barrier | (c) barrier, not volatile | (c) barrier, scheduler pinned\n");
        for (int occ : {1, 2, 3, 4, 8}) {
            int bl = prop.multiProcessorCount * occ;
            double muls = 2.0 * bl * threads * fi;
            printf("  %d waves/SIMD:", occ);
            spread(k_mul29<2>, bl, muls); printf(" |");
            spread(k_mul29_chains<MacAsmVcc, 2>, bl, muls); printf(" |");
            spread(k_mul29_chains<MacAsmSgpr, 2>, bl, muls); printf(" |");
            spread(k_mul29_chains<MacBarrier, 2>, bl, muls); printf(" |");
            spread(k_mul29_chains<MacBarrierFree, 2>, bl, muls); printf(" |");
            spread(k_mul29_chains<MacBarrierPinned, 2>, bl, muls); printf("\n");
        }
        printf("three products: three mul() | (c) barrier | (a) asm, vcc | (c) barrier, scheduler pinned\n");
        for (int occ : {1, 2, 3, 4, 8}) {
            int bl = prop.multiProcessorCount * occ;
            double muls = 3.0 * bl * threads * fi;
            printf("  %d waves/SIMD:", occ);
            spread(k_mul29<3>, bl, muls); printf(" |");
            spread(k_mul29_chains<MacBarrier, 3>, bl, muls); printf(" |");
            spread(k_mul29_chains<MacAsmVcc, 3>, bl, muls); printf(" |");
            spread(k_mul29_chains<MacBarrierPinned, 3>, bl, muls); printf("\n");
        }
    }
    return 0;
}
