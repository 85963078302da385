// legosnark_amd/csrc/curves.h -- curve traits shared by the MSM pipeline (msm.hip and its stage headers) and the
// fixed-base batch exponentiation (batch_exp.hip): which representation a group's device
// kernels compute in, how a device-resident base is stored, and the point operations.
#pragma once
#include "ec.h"
#include "fp29.h"
#include "fp29x2.h"
#include "quad29.h"

namespace lsa {

// G1 on 9 x 29-bit unsaturated limbs (fp29.h); bases packed to 64 B.
struct CurveG1 {
    using Field = Fq;
    using Base = AffPacked;
    using Acc = XYZZ29;
    static constexpr bool GLV = true;     // scalars split as k1 + k2*lambda (glv.h)
    static __device__ __forceinline__ Acc inf() { return Acc::inf(); }
    // acc + (+-)[phi](b): the sign goes into the addition's own carry pass, never into a negated copy of the base
    // (fp29.h: xyzz29_madd_signed).  ENDO = false: a caller whose entries never carry the endo bit.
    template <bool ENDO = true>
    static __device__ __forceinline__ Acc madd(const Acc &a, const Base &b, bool negate, bool endo) {
        return g1_madd_packed<ENDO>(a, b, negate, endo);
    }
    // the head of a bucket list, two finite bases, as affine + affine (4M + 2S instead of two mixed additions from infinity)
    static constexpr bool HEAD = true;
    static __device__ __forceinline__ bool head_ok(const Base &b0, const Base &b1) { return !packed_is_inf(b0) && !packed_is_inf(b1); }
    template <bool ENDO = true>
    static __device__ __forceinline__ Acc madd_head(const Base &b0, bool neg0, bool endo0, const Base &b1, bool neg1, bool endo1) {
        return g1_madd_head<ENDO>(b0, neg0, endo0, b1, neg1, endo1);
    }
    // PAIRED: the general addition with its products in pairs (fp29.h: xyzz29_add_paired), for the kernels whose registers
    // allow it -- msm_accumulate.h names them through PairedAdd
    template <bool PAIRED = false>
    static __device__ __forceinline__ Acc add(const Acc &a, const Acc &b) {
        if constexpr (PAIRED) return xyzz29_add_paired(a, b);
        else return xyzz29_add(a, b);
    }
    static __device__ __forceinline__ Acc dbl(const Acc &a) { return xyzz29_dbl(a); }
    static __device__ __forceinline__ Jac<Fq> to_jac(const Acc &a) { return xyzz29_to_jac(a); }
    static __device__ __forceinline__ Acc from_jac(const Jac<Fq> &p) {          // ZZ = Z^2, ZZZ = Z^3
        if (p.Z.is_zero()) return Acc::inf();
        F29 z = F29::from_mont256(p.Z), zz = sqr(z);
        return {F29::from_mont256(p.X), F29::from_mont256(p.Y), zz, mul(zz, z)};
    }
    static __device__ __forceinline__ Base from_affine(const Aff<Fq> &a) {
        Base r;
        if (a.is_inf()) {
#pragma unroll
            for (int i = 0; i < 8; i++) { r.x[i] = 0; r.y[i] = 0; }
        } else {
            F29::from_mont256(a.x).canonical().pack256(r.x);
            F29::from_mont256(a.y).canonical().pack256(r.y);
        }
        return r;
    }
};
// G2 on the same 29-bit-limb field (fp29x2.h): Fq2 products with fused reductions; bases
// packed to 128 B.  No GLV (the G2 endomorphism needs a 4-dimensional split): 16 windows.
struct CurveG2 {
    using Field = Fq2;
    using Base = AffPackedG2;
    using Acc = XYZZ29x2;
    static constexpr bool GLV = false;
    static __device__ __forceinline__ Acc inf() { return Acc::inf(); }
    static constexpr bool HEAD = false;      // no affine + affine head of a bucket list (CurveG1 has one)
    // ENDO is unused here (G2 has no endomorphism entries): it only lets accumulate_body write C::template madd<ENDO> for both curves
    template <bool ENDO = true>
    static __device__ __forceinline__ Acc madd(const Acc &a, const Base &b, bool negate, bool /*endo*/) {
        Aff29x2 q = unpack_affine(b);
        if (q.is_inf()) return a;
        if (negate) q.y = sub_k<1>(F29x2::zero(), q.y);                // p - y per component
        return g2_madd(a, q);
    }
    template <bool PAIRED = false>      // unused: G2 has one general addition
    static __device__ __forceinline__ Acc add(const Acc &a, const Acc &b) { return g2_add(a, b); }
    static __device__ __forceinline__ Acc dbl(const Acc &a) { return g2_dbl(a); }
    static __device__ __forceinline__ Jac<Fq2> to_jac(const Acc &a) { return g2_to_jac(a); }
    static __device__ __forceinline__ Acc from_jac(const Jac<Fq2> &p) {
        if (p.Z.is_zero()) return Acc::inf();
        F29x2 z = f29x2_from_mont256(p.Z), zz = sqr<2>(z);
        return {f29x2_from_mont256(p.X), f29x2_from_mont256(p.Y), zz, mul<2>(zz, z)};
    }
    static __device__ __forceinline__ Base from_affine(const Aff<Fq2> &a) { return pack_affine_g2(a); }
};
template <class F> struct CurveOf;
template <> struct CurveOf<Fq> { using type = CurveG1; };
template <> struct CurveOf<Fq2> { using type = CurveG2; };


}  // namespace lsa
