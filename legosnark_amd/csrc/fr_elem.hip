// legosnark_amd/csrc/fr_elem.hip -- element-wise algebra on device-resident Fr vectors: products, linear combinations,
// geometric sequences, batch inversion and the evaluation of a coefficient vector at a point (lsa_fr_vec_mul,
// lsa_fr_vec_lincomb, lsa_fr_powers, lsa_fr_batch_inverse, lsa_fr_poly_eval; the entry points are in capi_fr.hip, the
// arithmetic of an element and of a run in fr_elem.h).
//
// Replaces the host loops between the library's other Fr calls: the Hadamard witness c = a o b (hadamard.cc:130-135), the
// key generator's gamma * L_i(chi) and chi^i (lipmaa.h:50-52, 98-102), the Groth16 key scalars (beta At + alpha Bt + Ct) / delta,
// PolyT::eval (polytools.h:92-100).
//
//   k_fr_vec_mul, k_fr_vec_lincomb<K>   HBM streams shaped like k_scale_upper (fr_vec.hip): 16-byte non-temporal loads, a lane
//       takes U elements a grid stride apart and issues all their loads before the first product.  U * (vectors read) is
//       held at eight elements in flight per lane at most (lincomb: U = 4 for one or two vectors, 2 up to four, 1 beyond; vec_mul: 2), and the grid
//       is sized so that one trip of the loop covers fr_elem_pass_elems() elements whatever U is.  The constants arrive as
//       kernel arguments in the form they are used in (fr_elem.h) and live in scalar registers.  out may be exactly an input:
//       a lane reads every element it owns before it writes one, and no lane touches another's.
//   k_fr_powers, k_fr_batch_inverse     one run of consecutive elements per lane (fr_elem.h), 64-lane workgroups as k_fr_geom_row.
//   k_fr_poly_eval, k_fr_poly_finish    a lane evaluates FR_ELEM_EVAL_ITEMS consecutive coefficients by Horner's rule; its
//       offset power x^lo is factored as (x^ITEMS)^lane * (x^(256 ITEMS))^block: the first factor is a power with an exponent
//       below 256 per lane, the second is applied ONCE per workgroup, after the tree sum of its lanes.  The finishing kernel
//       adds the workgroups' partials (fr_elem_sum_push).  No atomics on field elements.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capi_internal.h"
#include "fr29.h"
#include "fr_elem.h"
#include "fr_stream.h"

namespace lsa {

constexpr unsigned ELEM_BLOCK = 256;          // lanes of a streaming workgroup and of k_fr_poly_eval
constexpr unsigned ELEM_UNROLL_MAX = 4;       // elements per lane and trip at most (k_scale_upper's STREAM_UNROLL)
// workgroups per CU of a streaming launch, at the widest unroll (-DFR_ELEM_BLOCKS_PER_CU=n builds another grid).  32 is
// k_scale_upper's 8192 workgroups on 256 CUs; measured at n = 2^24 against that kernel in the same process (bytes/s over
// its own): 8 per CU 0.95 (vec_mul) / 0.955 (lincomb k = 1) / 1.01 (k = 2) / 1.05 (k = 3), 32 per CU 0.99-1.0 / 1.0 / 1.06 / 1.12-1.13
#ifndef FR_ELEM_BLOCKS_PER_CU
#define FR_ELEM_BLOCKS_PER_CU 32
#endif
// elements per lane and trip of k_fr_vec_mul (two loads each): 2 or 4.  Measured at n = 2^24: 0.341 ms with 2, 0.347 ms with 4
#ifndef FR_ELEM_MUL_UNROLL
#define FR_ELEM_MUL_UNROLL 2
#endif
constexpr unsigned RUN_BLOCK = 64;            // few, long-running lanes: small workgroups spread them over the CUs

struct FrVecPtrs { const Fr *x[FR_VEC_LINCOMB_MAX]; };
struct FrVecCoefs { Fr c[FR_VEC_LINCOMB_MAX]; };
constexpr unsigned lincomb_unroll(unsigned k) { return k <= 2 ? 4 : (k <= 4 ? 2 : 1); }

// out[i] = scale * a[i] * b[i]; c266: the scale in form 2^266.  out may be a and / or b.
__global__ __launch_bounds__(ELEM_BLOCK) void k_fr_vec_mul(const Fr *a, const Fr *b, Fr c266, size_t n, Fr *out) {
    constexpr int U = FR_ELEM_MUL_UNROLL;
    const Fr29 c = Fr29::from_words(c266);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t p0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p0 < n; p0 += stride * U) {
        Fr x[U][2];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t p = p0 + u * stride;
            if (p < n) { x[u][0] = fr_stream_load(a + p); x[u][1] = fr_stream_load(b + p); }
        }
        // (written out: left as a loop, the compiler keeps this one rolled and the loaded elements in scratch)
        auto emit = [&](int u) {
            const size_t p = p0 + u * stride;
            if (p < n) fr_stream_store(out + p, fr_elem_mul_point(Fr29::from_words(x[u][0]), Fr29::from_words(x[u][1]), c));
        };
        static_assert(U == 2 || U == 4, "emit() is called once per element of the trip");
        emit(0); emit(1);
        if constexpr (U == 4) { emit(2); emit(3); }
    }
}

// out[i] = sum_{t < K} c[t] xs[t][i]; cs: the coefficients in form 2^261.  out may be any of the xs.
template <unsigned K>
__global__ __launch_bounds__(ELEM_BLOCK) void k_fr_vec_lincomb(FrVecPtrs xs, FrVecCoefs cs, size_t n, Fr *out) {
    constexpr int U = (int)lincomb_unroll(K);
    Fr29 c[K];
#pragma unroll
    for (unsigned t = 0; t < K; t++) c[t] = Fr29::from_words(cs.c[t]);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t p0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p0 < n; p0 += stride * U) {
        Fr x[U][K];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t p = p0 + u * stride;
            if (p < n) {
#pragma unroll
                for (unsigned t = 0; t < K; t++) x[u][t] = fr_stream_load(xs.x[t] + p);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t p = p0 + u * stride;
            if (p < n) {
                Fr29 l[K];
#pragma unroll
                for (unsigned t = 0; t < K; t++) l[t] = Fr29::from_words(x[u][t]);
                fr_stream_store(out + p, fr_elem_lincomb_point(l, c, K));
            }
        }
    }
}

// out[i] = first * base^i, i < n: run `lane` is elements lane * FR_ELEM_POWERS_RUN ..; no chain across lanes
__global__ __launch_bounds__(RUN_BLOCK) void k_fr_powers(Fr base261, Fr first, size_t n, Fr *out) {
    const size_t lo = ((size_t)blockIdx.x * RUN_BLOCK + threadIdx.x) * FR_ELEM_POWERS_RUN;
    if (lo >= n) return;
    const size_t left = n - lo;
    fr_elem_powers_run(Fr29::from_words(base261), Fr29::from_words(first), lo, (unsigned)(left < FR_ELEM_POWERS_RUN ? left : FR_ELEM_POWERS_RUN), out + lo);
}

// out[i] = 1 / x[i] (0 for an element that is 0 mod r), runs of FR_ELEM_INV_RUN; *zeros += the number of such elements
__global__ __launch_bounds__(RUN_BLOCK) void k_fr_batch_inverse(const Fr *x, size_t n, Fr *out, unsigned long long *zeros) {
    const size_t lo = ((size_t)blockIdx.x * RUN_BLOCK + threadIdx.x) * FR_ELEM_INV_RUN;
    if (lo >= n) return;
    const size_t left = n - lo;
    const unsigned z = fr_elem_inv_run(x + lo, out + lo, (unsigned)(left < FR_ELEM_INV_RUN ? left : FR_ELEM_INV_RUN));
    if (z) atomicAdd(zeros, (unsigned long long)z);
}

// partial[block] = sum over the block's lanes of (their FR_ELEM_EVAL_ITEMS coefficients at x) * x^(first coefficient's index).
// x261, xi261: x and x^ITEMS in form 2^261; xb: the words of x^(256 ITEMS).
__global__ __launch_bounds__(ELEM_BLOCK) void k_fr_poly_eval(const Fr *__restrict__ c, size_t n, Fr x261, Fr xi261, Fr xb, Fr *__restrict__ partial) {
    __shared__ Fr s_red[ELEM_BLOCK];
    const size_t lo = ((size_t)blockIdx.x * ELEM_BLOCK + threadIdx.x) * FR_ELEM_EVAL_ITEMS;
    Fr v = Fr::zero();
    if (lo < n) {
        const size_t left = n - lo;
        const Fr29 lane_pow = fr29_pow_u64(Fr29::from_words(xi261), threadIdx.x);
        v = fr_elem_horner_run(c + lo, (unsigned)(left < FR_ELEM_EVAL_ITEMS ? left : FR_ELEM_EVAL_ITEMS), Fr29::from_words(x261), lane_pow).canonical2().to_words();
    }
    s_red[threadIdx.x] = v;
    __syncthreads();
    for (unsigned sft = ELEM_BLOCK / 2; sft >= 1; sft >>= 1) {
        if (threadIdx.x < sft) s_red[threadIdx.x] = s_red[threadIdx.x] + s_red[threadIdx.x + sft];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = blockIdx.x ? s_red[0] * fr_pow_u64(xb, blockIdx.x) : s_red[0];
}
// out = sum of n canonical partials (one workgroup): a lane adds its share on limbs, then a tree
__global__ __launch_bounds__(ELEM_BLOCK) void k_fr_poly_finish(const Fr *__restrict__ partial, size_t n, Fr *__restrict__ out) {
    __shared__ Fr s_red[ELEM_BLOCK];
    FrDot d = fr_dot_zero();
    for (size_t b = threadIdx.x; b < n; b += ELEM_BLOCK) fr_elem_sum_push(d, Fr29::from_words(partial[b]));
    s_red[threadIdx.x] = fr_elem_sum_finish(d);
    __syncthreads();
    for (unsigned sft = ELEM_BLOCK / 2; sft >= 1; sft >>= 1) {
        if (threadIdx.x < sft) s_red[threadIdx.x] = s_red[threadIdx.x] + s_red[threadIdx.x + sft];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s_red[0];
}

// ---------------------------------------------------------------- host side
// elements one trip of the streaming kernels' loop covers: FR_ELEM_BLOCKS_PER_CU workgroups per CU at the widest unroll
size_t fr_elem_pass_elems() {
    static size_t cus = 0;
    if (!cus) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
            (void)hipGetLastError();
            return 0;
        }
        cus = (size_t)n;
    }
    return cus * FR_ELEM_BLOCKS_PER_CU * ELEM_BLOCK * ELEM_UNROLL_MAX;
}
static unsigned elem_blocks(size_t n, unsigned unroll) {
    const size_t cap = fr_elem_pass_elems() / ((size_t)ELEM_BLOCK * unroll), b = (n + ELEM_BLOCK - 1) / ELEM_BLOCK;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}
static unsigned run_blocks(size_t n, unsigned run) { return (unsigned)(((n + run - 1) / run + RUN_BLOCK - 1) / RUN_BLOCK); }

int fr_vec_mul_device(const Fr *d_a, const Fr *d_b, const Fr &c266, size_t n, Fr *d_out, hipStream_t st) {
    if (n == 0) return LSA_OK;
    if (!fr_elem_pass_elems()) { set_error("fr_vec_mul: no device"); return LSA_ERR_HIP; }
    hipLaunchKernelGGL(k_fr_vec_mul, dim3(elem_blocks(n, FR_ELEM_MUL_UNROLL)), dim3(ELEM_BLOCK), 0, st, d_a, d_b, c266, n, d_out);
    HIPCHK(hipGetLastError());
    return LSA_OK;
}

template <unsigned K>
static void launch_lincomb(const FrVecPtrs &xs, const FrVecCoefs &cs, size_t n, Fr *d_out, hipStream_t st) {
    hipLaunchKernelGGL((k_fr_vec_lincomb<K>), dim3(elem_blocks(n, lincomb_unroll(K))), dim3(ELEM_BLOCK), 0, st, xs, cs, n, d_out);
}
// c261: the k coefficients in form 2^261 (host)
int fr_vec_lincomb_device(const Fr *const *d_xs, const Fr *c261, size_t k, size_t n, Fr *d_out, hipStream_t st) {
    if (k == 0 || k > FR_VEC_LINCOMB_MAX) { set_error("fr_vec_lincomb: k = %zu not in 1..%u", k, FR_VEC_LINCOMB_MAX); return LSA_ERR_INVALID; }
    if (n == 0) return LSA_OK;
    if (!fr_elem_pass_elems()) { set_error("fr_vec_lincomb: no device"); return LSA_ERR_HIP; }
    FrVecPtrs xs;
    FrVecCoefs cs;
    for (unsigned t = 0; t < FR_VEC_LINCOMB_MAX; t++) {
        xs.x[t] = t < k ? d_xs[t] : nullptr;
        cs.c[t] = t < k ? c261[t] : Fr::zero();
    }
    switch (k) {
    case 1: launch_lincomb<1>(xs, cs, n, d_out, st); break;
    case 2: launch_lincomb<2>(xs, cs, n, d_out, st); break;
    case 3: launch_lincomb<3>(xs, cs, n, d_out, st); break;
    case 4: launch_lincomb<4>(xs, cs, n, d_out, st); break;
    case 5: launch_lincomb<5>(xs, cs, n, d_out, st); break;
    case 6: launch_lincomb<6>(xs, cs, n, d_out, st); break;
    case 7: launch_lincomb<7>(xs, cs, n, d_out, st); break;
    default: launch_lincomb<8>(xs, cs, n, d_out, st); break;
    }
    HIPCHK(hipGetLastError());
    return LSA_OK;
}

// base261: the base in form 2^261; first: canonical words
int fr_powers_device(const Fr &base261, const Fr &first, size_t n, Fr *d_out, hipStream_t st) {
    if (n == 0) return LSA_OK;
    hipLaunchKernelGGL(k_fr_powers, dim3(run_blocks(n, FR_ELEM_POWERS_RUN)), dim3(RUN_BLOCK), 0, st, base261, first, n, d_out);
    HIPCHK(hipGetLastError());
    return LSA_OK;
}

// d_zeros: one 64-bit counter, zeroed here on the stream
int fr_batch_inverse_device(const Fr *d_x, size_t n, Fr *d_out, unsigned long long *d_zeros, hipStream_t st) {
    HIPCHK(hipMemsetAsync(d_zeros, 0, sizeof(unsigned long long), st));
    if (n == 0) return LSA_OK;
    hipLaunchKernelGGL(k_fr_batch_inverse, dim3(run_blocks(n, FR_ELEM_INV_RUN)), dim3(RUN_BLOCK), 0, st, d_x, n, d_out, d_zeros);
    HIPCHK(hipGetLastError());
    return LSA_OK;
}

size_t fr_poly_eval_partials(size_t n) { return (n + (size_t)ELEM_BLOCK * FR_ELEM_EVAL_ITEMS - 1) / ((size_t)ELEM_BLOCK * FR_ELEM_EVAL_ITEMS); }
size_t fr_poly_eval_block_items() { return (size_t)ELEM_BLOCK * FR_ELEM_EVAL_ITEMS; }
// x: canonical words (host).  d_partial: fr_poly_eval_partials(n) elements.  n >= 1.
int fr_poly_eval_device(const Fr *d_c, size_t n, const Fr &x, Fr *d_partial, Fr *d_out, hipStream_t st) {
    const size_t blocks = fr_poly_eval_partials(n);
    const FrEvalConsts k = fr_elem_eval_consts(x, FR_ELEM_EVAL_ITEMS, ELEM_BLOCK);
    hipLaunchKernelGGL(k_fr_poly_eval, dim3((unsigned)blocks), dim3(ELEM_BLOCK), 0, st, d_c, n, k.x261, k.xi261, k.xb, d_partial);
    hipLaunchKernelGGL(k_fr_poly_finish, dim3(1), dim3(ELEM_BLOCK), 0, st, (const Fr *)d_partial, blocks, d_out);
    HIPCHK(hipGetLastError());
    return LSA_OK;
}

}  // namespace lsa
