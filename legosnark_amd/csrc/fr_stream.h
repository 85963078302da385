// legosnark_amd/csrc/fr_stream.h -- the 16-byte non-temporal loads and stores of the Fr streaming kernels (fr_vec.hip,
// fr_elem.hip): every byte of such a stream is touched once.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fp.h"

namespace lsa {

// (stream kernels: their loads and stores are marked non-temporal -- every byte is touched once; round 6: pushRandomness at half = 2^23
// 0.181 -> 0.177 ms, the suffix update equal; -DLSA_STREAM_TEMPORAL: plain accesses; profiles/r06_w9_stream_kernels_nontemporal.txt)
typedef uint32_t lsa_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ Fr fr_stream_load(const Fr *p) {
#if !defined(LSA_STREAM_TEMPORAL)
    const lsa_u32x4 lo = __builtin_nontemporal_load(reinterpret_cast<const lsa_u32x4 *>(p)), hi = __builtin_nontemporal_load(reinterpret_cast<const lsa_u32x4 *>(p) + 1);
    Fr x;
    x.l[0] = lo.x; x.l[1] = lo.y; x.l[2] = lo.z; x.l[3] = lo.w; x.l[4] = hi.x; x.l[5] = hi.y; x.l[6] = hi.z; x.l[7] = hi.w;
    return x;
#else
    return *p;
#endif
}
__device__ __forceinline__ void fr_stream_store(Fr *p, const Fr &x) {
#if !defined(LSA_STREAM_TEMPORAL)
    lsa_u32x4 lo, hi;
    lo.x = x.l[0]; lo.y = x.l[1]; lo.z = x.l[2]; lo.w = x.l[3]; hi.x = x.l[4]; hi.y = x.l[5]; hi.z = x.l[6]; hi.w = x.l[7];
    __builtin_nontemporal_store(lo, reinterpret_cast<lsa_u32x4 *>(p));
    __builtin_nontemporal_store(hi, reinterpret_cast<lsa_u32x4 *>(p) + 1);
#else
    *p = x;
#endif
}

}  // namespace lsa
