// legosnark_amd/csrc/msm_reduce.h -- stages 5-6 of the MSM pipeline (msm.hip): the tail.
// Bucket reduction (quad and lane levels, bit trees), the Horner fold / emit, and the publication of a slot's result.
// Device code only, compiled by msm.hip (launch_tail).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "curves.h"
#include "msm_quad.h"

namespace lsa {

// ------------------------------------------------------------------------------------
// kernel 5: bucket reduction  sum_b (b+1) * S_b  per window.  Pure latency (a few thousand
// point additions on an otherwise idle chip), so every point is shared by a QUAD of lanes
// (quad29.h: one field product per lane per dependency level, ~2.7x shorter per addition than a
// lane-private one) and a wavefront holds 16 points.
//
// For quads j = 0..15 of a wavefront holding (acc_j, run_j) the helper returns in quad 0
//   ACC = sum_j acc_j + 2^log_mult * sum_j j*run_j      RUN = sum_j run_j
// using an inclusive suffix scan of run over the quads (4 shuffle steps), then two tree sums.
// ------------------------------------------------------------------------------------
template <class A>
__device__ __forceinline__ A select_acc(uint32_t mask, const A &a, const A &b) {   // mask all ones: a, zero: b
    A r;
    const uint32_t *pa = reinterpret_cast<const uint32_t *>(&a), *pb = reinterpret_cast<const uint32_t *>(&b);
    uint32_t *pr = reinterpret_cast<uint32_t *>(&r);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(A) / 4); i++) pr[i] = (pa[i] & mask) | (pb[i] & ~mask);
    return r;
}
// One call site of quad_add and one of quad_dbl for the whole helper (a loop of nine trips whose
// operands are selected with opaque masks, as in k_reduce1_lane below): the kernels built on it
// run ONE wavefront through their code once, so an unrolled version (13 inlined additions, 122 KB
// for k_reduce2) spent more time fetching instructions than executing them.  Order of work: the
// suffix scan of run (4 additions), then every quad scales its own suffix sum (log_mult
// doublings, all quads side by side) and adds it to its acc, then ONE tree sum (4 additions):
// 9 + log_mult sequential operations instead of 13 + log_mult.
template <class A>
__device__ __forceinline__ void quadwave_weighted(A &acc, A &run, unsigned log_mult, unsigned lane) {
    const unsigned q = lane & 3, qi = lane >> 2;
    A s = A::inf();
#pragma unroll 1
    for (unsigned step = 0; step < 9; step++) {
        // steps 0-3: run_j <- run_j + run_(j+d), d = 1, 2, 4, 8 (suffix scan); step 4: acc_j <- acc_j +
        // 2^log_mult * Suf_j (j >= 1); steps 5-8: acc_j <- acc_j + acc_(j+d), d = 8, 4, 2, 1
        if (step == 4) {
            s = (qi == 0) ? A::inf() : run;
#pragma unroll 1
            for (unsigned i = 0; i < log_mult; i++) s = quad_dbl(s, q);
        }
        uint32_t m_run = step < 4 ? 0xffffffffu : 0u, m_s = step == 4 ? 0xffffffffu : 0u;
        asm volatile("" : "+v"(m_run), "+v"(m_s));
        const unsigned d = step < 4 ? (1u << step) : (step == 4 ? 0u : (8u >> (step - 5)));
        const A lhs = select_acc(m_run, run, acc);
        const A rhs = select_acc(m_s, s, shfl_down_acc(lhs, 4 * d));
        A r = lhs;
        if (qi + d < 16) r = quad_add(lhs, rhs, q);
        run = select_acc(m_run, r, run);
        acc = select_acc(m_run, acc, r);
    }
}

// Wide path, level 1: ONE bucket space of B = 2^19 .. 2^21 buckets (every window gathers from its
// own pre-shifted copy of the bases, so bucket b has weight b+1 whatever the window).  That many
// buckets are throughput, not latency: one LANE per segment of L buckets with lane-private
// additions, writing the (ACC, RUN) pair the quad levels (k_reduce2) continue from.
// The kernel holds ONE inlined copy of the general addition (~40 KB of code with its doubling
// and infinity paths): written with two call sites (RUN += bucket; ACC += RUN) the loop body was
// 83 KB for G1 -- more than the 64-KB instruction cache two CUs share -- and every kernel that
// ran beside it on another stream (the next call's first sort kernels) spent its time on
// instruction fetches: k_hist_wide 35 -> 124 us, k_tile_scan_rows 6 -> 80 us.  The two additions of
// a bucket are therefore two trips through the same call site; which operands a trip takes is
// selected word by word with a mask the compiler cannot see through (it would unswitch the loop
// into two copies again).
template <class C>
__global__ __launch_bounds__(64) void k_reduce1_lane(const typename C::Acc *__restrict__ buckets, uint32_t B, uint32_t L, uint32_t split,
                                                     typename C::Acc *__restrict__ out) {
    using A = typename C::Acc;
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if ((uint64_t)t * L >= B) return;
    A acc = A::inf(), run = A::inf();
    const A *bk = buckets + (size_t)t * L * split;
    // trips per bucket: `split` of "RUN += part h", then one of "ACC += RUN"
    const uint32_t per = split + 1;
#pragma unroll 1
    for (int i = (int)L - 1; i >= 0; i--) {
#pragma unroll 1
        for (uint32_t h = 0; h < per; h++) {
            uint32_t m = h < split ? 0xffffffffu : 0u;       // all ones: RUN += bucket part
            asm volatile("" : "+v"(m));
            A rhs = run;
            if (h < split) rhs = bk[(size_t)i * split + h];
            const A lhs = select_acc(m, run, acc);
            const A r = C::template add<PairedAdd<C, TAIL_REDUCE1_LANE>::value>(lhs, rhs);
            run = select_acc(m, r, run);
            acc = select_acc(m, acc, r);
        }
    }
    out[2 * (size_t)t] = acc;
    out[2 * (size_t)t + 1] = run;
}

// The first 16-ary level over the 65536 (ACC, RUN) pairs of k_reduce1_lane, ONE LANE per group of sixteen (wide path, calls
// whose tail hides under the next call's front).  The quad version of this level (k_reduce2) is the shortest chain --
// 9 + log_mult quad operations -- but every quad operation keeps four lanes busy for one addition and carries ~40 % of
// selects and broadcasts: 4096 wavefronts x ~20 000 instructions = 82 M wavefront-instructions per MSM, as much as a
// sixth of the accumulate kernel, on a chip whose issue slots are the bottleneck of a pipelined step.  A lane-private
// running sum does the same arithmetic in 48 general additions per lane: 64 wavefronts x ~190 000 instructions = 12 M.
// Seven times less work, 0.2 ms more latency -- the right trade exactly when nobody waits for this call alone.
//   ACC = sum_j acc_j + 2^log_mult * sum_j j * run_j,  RUN = sum_j run_j   (j = 0 .. 15, as quadwave_weighted)
template <class C>
__global__ __launch_bounds__(64) void k_reduce2_lane(const typename C::Acc *__restrict__ in, uint32_t m_in, uint32_t m_out, uint32_t log_mult,
                                                     typename C::Acc *__restrict__ out) {
    using A = typename C::Acc;
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= m_out) return;
    A acc = A::inf(), run = A::inf(), wsum = A::inf();
    // trips per input pair through ONE addition site (see k_reduce1_lane): acc += acc_j; run += run_j; wsum += run (j >= 1)
#pragma unroll 1
    for (int j = 15; j >= 0; j--) {
        const uint32_t idx = 16 * t + (uint32_t)j;
        const bool have = idx < m_in;
        const uint32_t trips = j ? 3u : 2u;
#pragma unroll 1
        for (uint32_t h = 0; h < trips; h++) {
            uint32_t m0 = h == 0 ? 0xffffffffu : 0u, m1 = h == 1 ? 0xffffffffu : 0u;
            asm volatile("" : "+v"(m0), "+v"(m1));
            A rhs = run;                                                    // h == 2: wsum += run
            if (h < 2) rhs = have ? in[2 * (size_t)idx + h] : A::inf();
            const A lhs = select_acc(m0, acc, select_acc(m1, run, wsum));
            const A r = C::template add<PairedAdd<C, TAIL_REDUCE2_LANE>::value>(lhs, rhs);
            acc = select_acc(m0, r, acc);
            run = select_acc(m1, r, run);
            wsum = select_acc(~(m0 | m1), r, wsum);
        }
    }
#pragma unroll 1
    for (uint32_t i = 0; i < log_mult; i++) wsum = C::dbl(wsum);
    out[2 * (size_t)t] = C::template add<PairedAdd<C, TAIL_REDUCE2_LANE>::value>(acc, wsum);
    out[2 * (size_t)t + 1] = run;
}

// Level 1: T = B/L quads per window; quad t owns buckets [t*L, (t+1)*L) (their `split` partial
// sums are folded in here).  Writes one (ACC,RUN) pair per wavefront (16 quads = 16*L buckets).
template <class C>
__global__ __launch_bounds__(64) void k_reduce1(const typename C::Acc *__restrict__ buckets, uint32_t B, uint32_t L, uint32_t logL,
                                                uint32_t waves_per_window, uint32_t split, typename C::Acc *__restrict__ wave_out) {
    using A = typename C::Acc;
    uint32_t wave = blockIdx.x;                 // global wave id = k*waves_per_window + w
    uint32_t k = wave / waves_per_window, w = wave % waves_per_window;
    const unsigned lane = threadIdx.x, q = lane & 3;
    uint32_t t = w * 16 + (lane >> 2);
    A acc = A::inf(), run = A::inf();
    if ((uint64_t)t * L < B) {
        const A *bk = buckets + ((size_t)k * B + (size_t)t * L) * split;
        const uint32_t per = split + 1;              // trips per bucket through ONE addition site (see k_reduce1_lane)
#pragma unroll 1
        for (int i = (int)L - 1; i >= 0; i--) {
#pragma unroll 1
            for (uint32_t h = 0; h < per; h++) {
                uint32_t m = h < split ? 0xffffffffu : 0u;   // all ones: RUN += bucket part h; zero: ACC += RUN
                asm volatile("" : "+v"(m));
                A rhs = run;
                if (h < split) rhs = bk[(size_t)i * split + h];
                const A lhs = select_acc(m, run, acc);
                const A r = quad_add(lhs, rhs, q);
                run = select_acc(m, r, run);
                acc = select_acc(m, acc, r);
            }
        }
    }
    quadwave_weighted(acc, run, logL, lane);
    if (lane == 0) {
        wave_out[2 * (size_t)wave] = acc;
        wave_out[2 * (size_t)wave + 1] = run;
    }
}

// Level >= 2: per window, every wavefront folds 16 consecutive (ACC,RUN) pairs of the previous
// level (each covering 2^log_mult buckets) into one; the last level (m_out == 1) leaves the
// window sum in out[2*k].
template <class C>
__global__ __launch_bounds__(64) void k_reduce2(const typename C::Acc *__restrict__ in, uint32_t m_in, uint32_t m_out, uint32_t log_mult,
                                                typename C::Acc *__restrict__ out) {
    using A = typename C::Acc;
    const uint32_t k = blockIdx.x / m_out, w = blockIdx.x % m_out;
    const unsigned lane = threadIdx.x;
    const uint32_t j = w * 16 + (lane >> 2);
    A acc = A::inf(), run = A::inf();
    if (j < m_in) {
        acc = in[2 * ((size_t)k * m_in + j)];
        run = in[2 * ((size_t)k * m_in + j) + 1];
    }
    quadwave_weighted(acc, run, log_mult, lane);
    if (lane == 0) {
        out[2 * ((size_t)k * m_out + w)] = acc;
        out[2 * ((size_t)k * m_out + w) + 1] = run;
    }
}

// ------------------------------------------------------------------------------------
// kernel 6: Horner fold over windows -> Jacobian (libff layout)
// ------------------------------------------------------------------------------------
// Keep a value in VGPRs: without this the compiler proves the single active lane's data
// wave-uniform and moves the whole fold onto the scalar ALU (3x slower).
template <class A>
__device__ __forceinline__ void pin_vgpr(A &a) {
    uint32_t *w = reinterpret_cast<uint32_t *>(&a);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(A) / 4); i++) asm volatile("" : "+v"(w[i]));
}

// ------------------------------------------------------------------------------------
// kernel 6b (G1): the same Horner fold with each point shared by a QUAD of lanes.  The 240
// doublings are inherently sequential, so the lever is latency per doubling: the 9 field
// products of an XYZZ doubling have only 3 dependency levels, and the 14 of a general add
// have 4.  Lane q of the quad computes the q-th product of each level; results are
// replicated with DPP quad_perm broadcasts (v_mov_b32_dpp, no LDS).  ~2.7x shorter chain.
// ------------------------------------------------------------------------------------
template <class A, class J>
__device__ __forceinline__ void fold_quad_body(const A *__restrict__ window_sums, unsigned nwin, unsigned c, J *__restrict__ out) {
    // EVERY quad of the wavefront runs the same fold (one of them would do): with four lanes on, a lone wavefront executes
    // the chain 1.1-2.1x slower, depending on the CU it landed on (tools/ubench_exec_mask.hip); lane 0 stores
    if (blockIdx.x != 0) return;
    const unsigned q = threadIdx.x & 3;
    // window_sums holds (ACC,RUN) pairs of the last reduction level: window k at index 2k
    A r = window_sums[2 * (nwin - 1)];
    pin_vgpr(r);
    for (int k = (int)nwin - 2; k >= 0; k--) {
        for (unsigned i = 0; i < c; i++) r = quad_dbl(r, q);
        A w = window_sums[2 * k];
        pin_vgpr(w);
        r = quad_add(r, w, q);
    }
    J res;
    if constexpr (std::is_same<A, XYZZ29>::value) res = xyzz29_to_jac(r);
    else res = g2_to_jac(r);
    pin_vgpr(res);
    if (threadIdx.x == 0) *out = res;
}
__global__ __launch_bounds__(64) void k_fold_quad(const XYZZ29 *__restrict__ window_sums, unsigned nwin, unsigned c, Jac<Fq> *__restrict__ out) {
    fold_quad_body(window_sums, nwin, c, out);
}
__global__ __launch_bounds__(64) void k_fold_quad_g2(const XYZZ29x2 *__restrict__ window_sums, unsigned nwin, unsigned c, Jac<Fq2> *__restrict__ out) {
    fold_quad_body(window_sums, nwin, c, out);
}

// segmented calls: window j's sum (slot 2j of the last reduction level) -> result j
template <class A, class J>
__device__ __forceinline__ void emit_body(const A *__restrict__ window_sums, J *__restrict__ out) {
    if (threadIdx.x != 0) return;
    A r = window_sums[2 * (size_t)blockIdx.x];
    if constexpr (std::is_same<A, XYZZ29>::value) out[blockIdx.x] = xyzz29_to_jac(r);
    else out[blockIdx.x] = g2_to_jac(r);
}
__global__ __launch_bounds__(64) void k_emit_g1(const XYZZ29 *__restrict__ window_sums, Jac<Fq> *__restrict__ out) { emit_body(window_sums, out); }
__global__ __launch_bounds__(64) void k_emit_g2(const XYZZ29x2 *__restrict__ window_sums, Jac<Fq2> *__restrict__ out) { emit_body(window_sums, out); }

// ------------------------------------------------------------------------------------
// The upper reduction levels as bit trees (wide path, one bucket space).  After the first k_reduce2 level m = 4096
// (ACC, RUN) pairs are left, pair t covering 2^lm buckets:  total = sum_t ACC_t + 2^lm * sum_t t * RUN_t.  Three more
// 16-ary levels are three dependent chains of 9 + log_mult quad operations each (53 + 61 + 67 us of a lone call's
// 1.55 ms); written as  sum_t t * RUN_t = sum_j 2^j * T_j,  T_j = sum of the RUN_t whose index has bit j,  the twelve
// T_j and the sum of the ACC_t are thirteen INDEPENDENT tree sums (k_reduce_bits_a: eight wavefronts per 512 pairs,
// 7 + 3 quad additions), each weighted by its own lm + j doublings (k_reduce_bits_b: one wavefront per tree) and added
// up by one wavefront that also converts the result (k_reduce_bits_c): ~75 us.  Same quad arithmetic (quad29.h); 13 x
// the reads of the level it replaces, but that level is 4096 pairs: 832 short wavefronts against the 4096 of the level
// before it.
// ------------------------------------------------------------------------------------
template <class C>
__global__ __launch_bounds__(512) void k_reduce_bits_a(const typename C::Acc *__restrict__ pairs, uint32_t m, uint32_t nbits, uint32_t G,
                                                       typename C::Acc *__restrict__ part) {
    using A = typename C::Acc;
    constexpr uint32_t AW = sizeof(A) / 4;
    __shared__ uint32_t wave_sum[8][AW];
    const uint32_t bit = blockIdx.x, g = blockIdx.y;
    const unsigned tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, sub = lane & 3, qd = lane >> 2;
    A a = A::inf();
#pragma unroll 1
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t t = g * 512 + wv * 64 + qd + 16 * j;
        A o = A::inf();
        if (t < m) {
            if (bit == nbits) o = pairs[2 * (size_t)t];                              // the ACC tree
            else if ((t >> bit) & 1u) o = pairs[2 * (size_t)t + 1];                  // RUN_t into T_bit
        }
        a = quad_add(a, o, sub);
    }
    a = bits_quad_tree(a, lane, 8);
    if (lane == 0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(&a);
#pragma unroll
        for (uint32_t w = 0; w < AW; w++) wave_sum[wv][w] = src[w];
    }
    __syncthreads();
    if (wv != 0) return;
    a = A::inf();
    if (qd < 8) a = *reinterpret_cast<const A *>(&wave_sum[qd][0]);
    a = bits_quad_tree(a, lane, 4);
    if (lane == 0) part[bit * G + g] = a;
}
// one wavefront per tree: the G <= 16 partials of tree `bit`, then its weight 2^(lm + bit) (the ACC tree: none)
template <class C>
__global__ __launch_bounds__(64) void k_reduce_bits_b(const typename C::Acc *__restrict__ part, uint32_t nbits, uint32_t G, uint32_t lm,
                                                      typename C::Acc *__restrict__ weighted) {
    using A = typename C::Acc;
    const uint32_t bit = blockIdx.x;
    const unsigned lane = threadIdx.x, sub = lane & 3, qd = lane >> 2;
    A a = A::inf();
    if (qd < G) a = part[bit * G + qd];
    a = bits_quad_tree(a, lane, 8);
    const uint32_t dbl = bit == nbits ? 0u : lm + bit;
#pragma unroll 1
    for (uint32_t i = 0; i < dbl; i++) a = quad_dbl(a, sub);
    if (lane == 0) weighted[bit] = a;
}
// the sum of the nbits + 1 <= 16 weighted trees, as libff's Jacobian point
template <class C>
__global__ __launch_bounds__(64) void k_reduce_bits_c(const typename C::Acc *__restrict__ weighted, uint32_t count, Jac<typename C::Field> *__restrict__ out) {
    using A = typename C::Acc;
    const unsigned lane = threadIdx.x, qd = lane >> 2;
    A a = A::inf();
    if (qd < count) a = weighted[qd];
    a = bits_quad_tree(a, lane, 8);
    if (lane == 0) *out = C::to_jac(a);
}

// publishes a slot's result(s) into the caller's buffer (a 96/192-byte hipMemcpyAsync costs ~30 us
// as a runtime copy kernel; this is one small workgroup)
__global__ __launch_bounds__(256) void k_publish(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, unsigned words) {
    for (unsigned i = threadIdx.x; i < words; i += 256) dst[i] = src[i];
}

}  // namespace lsa
