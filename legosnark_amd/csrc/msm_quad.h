// legosnark_amd/csrc/msm_quad.h -- what the kernels of msm_accumulate.h, msm_reduce.h and msm_compact.hip share: an
// accumulator moved word by word (across lanes, out of memory) and the tree sum over the 16 quads of a wavefront
// (quad29.h: one point per quad of lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quad29.h"

namespace lsa {

template <class A>
__device__ __forceinline__ A shfl_down_acc(const A &p, unsigned delta) {
    A r;
    constexpr int NW = sizeof(A) / 4;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&p);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&r);
#pragma unroll
    for (int i = 0; i < NW; i++) dst[i] = __shfl_down(src[i], delta, 64);
    return r;
}

// the sum of the 16 quads' points, valid in quad 0 (four dependent quad additions from first_d = 8; one call site)
template <class A>
__device__ __forceinline__ A bits_quad_tree(A a, unsigned lane, unsigned first_d = 8) {
    const unsigned sub = lane & 3, qd = lane >> 2;
#pragma unroll 1
    for (unsigned d = first_d; d >= 1; d >>= 1) {
        A o = shfl_down_acc(a, 4 * d);
        if (qd + d >= 16) o = A::inf();
        a = quad_add(a, o, sub);
    }
    return a;
}

template <class A>
__device__ __forceinline__ A cmp_load(const A *p) {
    A r;
    constexpr int NW = sizeof(A) / 4;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(p);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&r);
#pragma unroll
    for (int w = 0; w < NW; w++) dst[w] = src[w];
    return r;
}

}  // namespace lsa
