// legosnark_amd/csrc/msm_bases.h -- stage 0 of the MSM pipeline (msm.hip): base preparation.
// Jacobian points in libff layout -> the device-resident base formats, and the step from one pre-shifted copy of a
// table to the next.  Device code only, compiled by msm.hip; the host side (prepare_bases, precompute_windows) is there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "curves.h"
#include "fs29.h"

namespace lsa {

// ------------------------------------------------------------------------------------
// kernel 0: Jacobian (libff layout) -> affine, per-lane Montgomery batch inversion
// ------------------------------------------------------------------------------------
template <class F, int K>
__global__ __launch_bounds__(256) void k_normalize(const Jac<F> *__restrict__ in, Aff<F> *__restrict__ out, size_t n) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t base = t * K;
    if (base >= n) return;
    F prod[K];
    F acc = F::one();
    const F one = F::one();
    bool need_inv = false;
#pragma unroll
    for (int i = 0; i < K; i++) {
        if (base + i < n) {
            F z = in[base + i].Z;
            if (!z.is_zero() && z != one) { acc = acc * z; need_inv = true; }
        }
        prod[i] = acc;
    }
    F inv = need_inv ? acc.inverse() : one;
#pragma unroll
    for (int i = K - 1; i >= 0; i--) {
        if (base + i < n) {
            Jac<F> p = in[base + i];
            Aff<F> a;
            if (p.Z.is_zero()) {
                a = Aff<F>::inf();
            } else if (p.Z == one) {
                a.x = p.X; a.y = p.Y;
            } else {
                F before = (i == 0) ? one : prod[i - 1];
                F zi = inv * before;          // 1 / Z_i
                inv = inv * p.Z;
                F zi2 = zi.sqr();
                a.x = p.X * zi2;
                a.y = p.Y * (zi2 * zi);
            }
            out[base + i] = a;
        }
    }
}

// affine (libff Montgomery limbs) -> the curve's device-resident base format
template <class C>
__global__ __launch_bounds__(256) void k_convert_bases(const Aff<typename C::Field> *__restrict__ in, typename C::Base *__restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = C::from_affine(in[i]);
}

// G1: Jacobian (libff layout) -> packed affine bases in ONE kernel, on the 29-bit-limb field: a third
// of the instructions per product of the 32-bit-limb Fq, no 64-byte staging array, and the same
// canonical coordinates as k_normalize + k_convert_bases (affine coordinates are unique).  Per lane K
// points share one Fermat inversion (Montgomery's trick).
template <int K>
__global__ __launch_bounds__(256) void k_prepare_g1(const Jac<Fq> *__restrict__ in, AffPacked *__restrict__ out, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, base = t * K;
    if (base >= n) return;
    const Fq one256 = Fq::one();
    F29 prod[K];
    F29 acc = F29::one();
    bool need_inv = false;
#pragma unroll
    for (int i = 0; i < K; i++) {
        if (base + i < n) {
            const Fq z = in[base + i].Z;
            if (!z.is_zero() && z != one256) { acc = mul(acc, F29::from_mont256(z)); need_inv = true; }
        }
        prod[i] = acc;
    }
    F29 inv = need_inv ? Fs{acc}.inverse().v : F29::one();
#pragma unroll
    for (int i = K - 1; i >= 0; i--) {
        if (base + i >= n) continue;
        const Jac<Fq> p = in[base + i];
        AffPacked r;
        if (p.Z.is_zero()) {
#pragma unroll
            for (int w = 0; w < 8; w++) { r.x[w] = 0; r.y[w] = 0; }
        } else {
            F29 x = F29::from_mont256(p.X), y = F29::from_mont256(p.Y);
            if (p.Z != one256) {
                const F29 zi = mul(inv, i == 0 ? F29::one() : prod[i - 1]);      // 1 / Z_i
                inv = mul(inv, F29::from_mont256(p.Z));
                const F29 zi2 = sqr(zi);
                x = mul(x, zi2);
                y = mul(y, mul(zi2, zi));
            }
            x.canonical().pack256(r.x);
            y.canonical().pack256(r.y);
        }
        out[base + i] = r;
    }
}

// G2: the same on Fq2 over the 29-bit limbs (fp29x2.h), K points per inversion (through the norm: one Fq inversion).
// k_normalize<Fq2, 8> + k_convert_bases, which this replaces, kept 656 bytes of scratch per lane: 344 MB for a full
// grid, far above what the runtime keeps allocated between dispatches, so EVERY launch paid a scratch allocation --
// 1-10 ms per launch depending on the box, twelve launches per streamed first-sight G2 vector.
template <int K>
__global__ __launch_bounds__(256) void k_prepare_g2(const Jac<Fq2> *__restrict__ in, AffPackedG2 *__restrict__ out, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, base = t * K;
    if (base >= n) return;
    const Fq2 one256 = Fq2::one();
    F29x2 prod[K];
    F29x2 acc = F29x2::one();
    bool need_inv = false;
#pragma unroll
    for (int i = 0; i < K; i++) {
        if (base + i < n) {
            const Fq2 z = in[base + i].Z;
            if (!z.is_zero() && z != one256) { acc = mul<2>(acc, f29x2_from_mont256(z)); need_inv = true; }   // [< 2]
        }
        prod[i] = acc;
    }
    F29x2 inv = need_inv ? f29x2_inverse(acc) : F29x2::one();
#pragma unroll
    for (int i = K - 1; i >= 0; i--) {
        if (base + i >= n) continue;
        const Jac<Fq2> p = in[base + i];
        AffPackedG2 r;
        if (p.Z.is_zero()) {
#pragma unroll
            for (int c = 0; c < 4; c++)
#pragma unroll
                for (int w = 0; w < 8; w++) r.w[c][w] = 0;
        } else {
            F29x2 x = f29x2_from_mont256(p.X), y = f29x2_from_mont256(p.Y);
            if (p.Z != one256) {
                const F29x2 zi = mul<2>(inv, i == 0 ? F29x2::one() : prod[i - 1]);      // 1 / Z_i
                inv = mul<2>(inv, f29x2_from_mont256(p.Z));
                const F29x2 zi2 = sqr<2>(zi);
                x = mul<2>(x, zi2);
                y = mul<2>(y, mul<2>(zi2, zi));
            }
            const F29x2 xc = x.canonical(), yc = y.canonical();
            xc.c0.pack256(r.w[0]);
            xc.c1.pack256(r.w[1]);
            yc.c0.pack256(r.w[2]);
            yc.c1.pack256(r.w[3]);
        }
        out[base + i] = r;
    }
}

// copy k of a table of pre-shifted bases from copy k - 1: c doublings per point (precompute_windows, msm.hip)
template <class C>
__global__ __launch_bounds__(256) void k_shift_window(const typename C::Base *__restrict__ prev, Jac<typename C::Field> *__restrict__ out,
                                                      size_t n, unsigned c) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typename C::Acc p = C::madd(C::inf(), prev[i], false, false);   // infinity stays infinity
    for (unsigned j = 0; j < c; j++) p = C::dbl(p);
    out[i] = C::to_jac(p);
}

}  // namespace lsa
