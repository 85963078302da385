// legosnark_amd/csrc/ecntt.hip -- the discrete Fourier transform on group elements: lsa_g1_ecntt, lsa_g2_ecntt,
// lsa_ecntt_param (include/legosnark_amd.h).  out[k] = sum_i [w^(ik)] in[i]: lsa_fr_ntt's transform with points for data and
// scalars for twiddles -- what turns a powers string chi^i G into the Lagrange-basis key L_i(chi) G without the trapdoor.
//
// A radix-2 network of log_n stages (geometry and per-butterfly body: ecntt.h) over two library-owned buffers of n
// Jacobian points.  Per call:
//   twiddles          one table w^t, t < n/2 (w^-1 for the inverse), by lsa_fr_powers' kernel; stage s reads it with stride n / 2^s
//   inverse only      prepare_bases over all n inputs, then k_ecntt_scale_*: [1/n] in[i], one ladder per point, every lane
//                     on the same scalar (no divergence), before stage 1
//   stage 1           k_ecntt_first_*: the twiddle is 1 everywhere -- two complete additions per butterfly, no ladder; the
//                     bit reversal is in its loads
//   stage s >= 2      prepare_bases over the upper half of the source buffer (the second operands: one batch inversion
//                     per stage), then the fused k_ecntt_stage_*: T = [w] B by the ladder body of k_smul_g1 / k_smul_g2
//                     (smul_glv on one lane; smul_g2 on a lane pair, one Fq2 component each), THEN the load of A, then
//                     A + T and A - T with the complete XYZZ additions.  T never goes to memory.  The first n / 2^s
//                     butterflies of a stage (twiddle 1) skip the ladder.  The last stage writes the caller's array.
// Ladders: forward (n/2)(log_n - 1) - (n/2 - 1) = (n/2)(log_n - 2) + 1; the inverse n more.
// Every intermediate point is in libff's Jacobian layout, so prepare_bases reads a stage's output as it is.
// Nothing is allocated after the first call of a size (StageBuf), and nothing waits for the device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "capi_internal.h"
#include "ecntt.h"
#include "fp29x2l.h"
#include "fr_elem.h"

namespace lsa {

static constexpr unsigned ECNTT_BLOCKS = 512;      // persistent grid of the ladder kernels: 2 blocks (8 waves) per CU, as k_smul_g1 / k_smul_g2
static constexpr unsigned ECNTT_G2_LANES = 2;      // lanes per G2 butterfly: one Fq2 component each

struct EcnttScalar { uint32_t w[8]; };             // canonical words of a scalar known to the host (1/n)

// ---------------------------------------------------------------- G1: one lane per butterfly
__global__ __launch_bounds__(256) void k_ecntt_first_g1(const Jac<Fq> *__restrict__ src, unsigned log_n, Jac<Fq> *__restrict__ dst) {
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= ((size_t)1 << (log_n - 1))) return;
    const EcnttBfly f = ecntt_bfly(log_n, 1, b);
    XYZZ29 sum, diff;
    ecntt_combine(ecntt_from_jac(src[f.src_a]), ecntt_from_jac(src[f.src_b]), sum, diff);
    dst[f.dst_a] = xyzz29_to_jac(sum);
    dst[f.dst_b] = xyzz29_to_jac(diff);
}

// src: the stage's source buffer (first operands in slots [0, n/2)); aff: its upper half, normalised (n/2 entries)
__global__ __launch_bounds__(256) void k_ecntt_stage_g1(const Jac<Fq> *__restrict__ src, const AffPacked *__restrict__ aff,
                                                        const Fr *__restrict__ tw, unsigned log_n, unsigned s,
                                                        XYZZ29 *__restrict__ tbl, Jac<Fq> *__restrict__ dst) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256, half_n = (size_t)1 << (log_n - 1);
    XYZZ29 *T = tbl + gid * SMUL_TBL;
    for (size_t b = gid; b < half_n; b += stride) {
        const EcnttBfly f = ecntt_bfly(log_n, s, b);
        const Aff29 B = unpack_affine(aff[b]);
        uint32_t w[8];
        tw[f.tw].to_canonical(w);
        const XYZZ29 t = ecntt_twiddled(B, w, f.tw == 0, T);
        XYZZ29 sum, diff;
        ecntt_combine(ecntt_from_jac(src[f.src_a]), t, sum, diff);     // (A is loaded after the ladder)
        dst[f.dst_a] = xyzz29_to_jac(sum);
        dst[f.dst_b] = xyzz29_to_jac(diff);
    }
}

// dst[i] = [c] aff[i], i < n
__global__ __launch_bounds__(256) void k_ecntt_scale_g1(const AffPacked *__restrict__ aff, EcnttScalar c, size_t n,
                                                        XYZZ29 *__restrict__ tbl, Jac<Fq> *__restrict__ dst) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    XYZZ29 *T = tbl + gid * SMUL_TBL;
    for (size_t i = gid; i < n; i += stride) dst[i] = xyzz29_to_jac(smul_glv(unpack_affine(aff[i]), c.w, T));
}

// ---------------------------------------------------------------- G2: a lane pair per butterfly (fp29x2l.h)
// (a pair shares its butterfly index, so its two lanes always stay or leave together)
__global__ __launch_bounds__(256) void k_ecntt_first_g2(const Jac<Fq2> *__restrict__ src, unsigned log_n, Jac<Fq2> *__restrict__ dst) {
    const size_t b = ((size_t)blockIdx.x * 256 + threadIdx.x) / ECNTT_G2_LANES;
    const unsigned part = threadIdx.x & 1u;
    if (b >= ((size_t)1 << (log_n - 1))) return;
    const EcnttBfly f = ecntt_bfly(log_n, 1, b);
    XYZZ29h sum, diff;
    ecntt_combine(g2h_from_jac(src[f.src_a], part), g2h_from_jac(src[f.src_b], part), sum, diff);
    g2h_store_jac(sum, part, &dst[f.dst_a]);
    g2h_store_jac(diff, part, &dst[f.dst_b]);
}

__global__ __launch_bounds__(256) void k_ecntt_stage_g2(const Jac<Fq2> *__restrict__ src, const AffPackedG2 *__restrict__ aff,
                                                        const Fr *__restrict__ tw, unsigned log_n, unsigned s,
                                                        XYZZ29h *__restrict__ tbl, Jac<Fq2> *__restrict__ dst) {
    const size_t lane = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * (256 / ECNTT_G2_LANES);
    const size_t half_n = (size_t)1 << (log_n - 1);
    const unsigned part = threadIdx.x & 1u;
    XYZZ29h *T = tbl + lane * SMUL_G2_TBL;
    for (size_t b = lane / ECNTT_G2_LANES; b < half_n; b += stride) {
        const EcnttBfly f = ecntt_bfly(log_n, s, b);
        const AffE<F29h> B = unpack_affine_half(aff[b], part);
        uint32_t w[8];
        tw[f.tw].to_canonical(w);
        const XYZZ29h t = ecntt_twiddled(B, w, f.tw == 0, T);
        XYZZ29h sum, diff;
        ecntt_combine(g2h_from_jac(src[f.src_a], part), t, sum, diff); // (A is loaded after the ladder)
        g2h_store_jac(sum, part, &dst[f.dst_a]);
        g2h_store_jac(diff, part, &dst[f.dst_b]);
    }
}

__global__ __launch_bounds__(256) void k_ecntt_scale_g2(const AffPackedG2 *__restrict__ aff, EcnttScalar c, size_t n,
                                                        XYZZ29h *__restrict__ tbl, Jac<Fq2> *__restrict__ dst) {
    const size_t lane = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * (256 / ECNTT_G2_LANES);
    const unsigned part = threadIdx.x & 1u;
    XYZZ29h *T = tbl + lane * SMUL_G2_TBL;
    for (size_t i = lane / ECNTT_G2_LANES; i < n; i += stride)
        g2h_store_jac(smul_g2(unpack_affine_half(aff[i], part), c.w, T), part, &dst[i]);
}

// ---------------------------------------------------------------- host side
namespace {
template <class F> struct EcnttOf;
template <> struct EcnttOf<Fq> {
    using Aff = AffPacked;
    using Tbl = XYZZ29;
    static constexpr unsigned LANES = 1, TBL = SMUL_TBL;
    static constexpr const char *NAME = "g1_ecntt";
    static void first(unsigned blocks, hipStream_t st, const Jac<Fq> *src, unsigned log_n, Jac<Fq> *dst) {
        hipLaunchKernelGGL(k_ecntt_first_g1, dim3(blocks), dim3(256), 0, st, src, log_n, dst);
    }
    static void stage(unsigned blocks, hipStream_t st, const Jac<Fq> *src, const Aff *aff, const Fr *tw, unsigned log_n, unsigned s, Tbl *tbl, Jac<Fq> *dst) {
        hipLaunchKernelGGL(k_ecntt_stage_g1, dim3(blocks), dim3(256), 0, st, src, aff, tw, log_n, s, tbl, dst);
    }
    static void scale(unsigned blocks, hipStream_t st, const Aff *aff, const EcnttScalar &c, size_t n, Tbl *tbl, Jac<Fq> *dst) {
        hipLaunchKernelGGL(k_ecntt_scale_g1, dim3(blocks), dim3(256), 0, st, aff, c, n, tbl, dst);
    }
};
template <> struct EcnttOf<Fq2> {
    using Aff = AffPackedG2;
    using Tbl = XYZZ29h;
    static constexpr unsigned LANES = ECNTT_G2_LANES, TBL = SMUL_G2_TBL;
    static constexpr const char *NAME = "g2_ecntt";
    static void first(unsigned blocks, hipStream_t st, const Jac<Fq2> *src, unsigned log_n, Jac<Fq2> *dst) {
        hipLaunchKernelGGL(k_ecntt_first_g2, dim3(blocks), dim3(256), 0, st, src, log_n, dst);
    }
    static void stage(unsigned blocks, hipStream_t st, const Jac<Fq2> *src, const Aff *aff, const Fr *tw, unsigned log_n, unsigned s, Tbl *tbl, Jac<Fq2> *dst) {
        hipLaunchKernelGGL(k_ecntt_stage_g2, dim3(blocks), dim3(256), 0, st, src, aff, tw, log_n, s, tbl, dst);
    }
    static void scale(unsigned blocks, hipStream_t st, const Aff *aff, const EcnttScalar &c, size_t n, Tbl *tbl, Jac<Fq2> *dst) {
        hipLaunchKernelGGL(k_ecntt_scale_g2, dim3(blocks), dim3(256), 0, st, aff, c, n, tbl, dst);
    }
};

// workgroups for `items` ladders: one trip each up to the persistent grid
template <class F>
unsigned ladder_blocks(size_t items) {
    const size_t per_block = 256 / EcnttOf<F>::LANES, want = (items + per_block - 1) / per_block;
    return (unsigned)(want < ECNTT_BLOCKS ? want : ECNTT_BLOCKS);
}

// the working memory of a call, for host and device callers alike, and the staged operands of host callers; shared by the
// two groups (every user is ordered on lsa_stream())
StageBuf g_stage_ec_ping[2], g_stage_ec_aff, g_stage_ec_tw, g_stage_ec_tbl, g_stage_ec_in, g_stage_ec_out;
}  // namespace

// Bytes of working memory for a transform of 2^log_n points, log_n >= 1: the two stage buffers, the normalised operands
// (all n for the inverse's scaling), the twiddles, the ladders' tables.
template <class F>
struct EcnttPlan {
    size_t ping, aff, tw, tbl;
    EcnttPlan(unsigned log_n, bool inverse) {
        const size_t n = (size_t)1 << log_n, ladders = inverse ? n : n / 2;
        ping = n * sizeof(Jac<F>);
        aff = ladders * sizeof(typename EcnttOf<F>::Aff);
        tw = (n / 2) * sizeof(Fr);
        tbl = (size_t)ladder_blocks<F>(ladders) * 256 * EcnttOf<F>::TBL * sizeof(typename EcnttOf<F>::Tbl);
    }
};

// d_out[k] = sum_i [w^(ik)] d_in[i] over 2^log_n points, log_n >= 1; w: omega, or its inverse for the inverse transform;
// inv_n != nullptr: every point is also multiplied by that scalar (1/n, canonical words).  d_out == d_in is allowed.
// buf0 / buf1 / d_aff / d_tw / d_tbl: EcnttPlan's sizes.  Asynchronous on st.
template <class F>
int ecntt_device(const Jac<F> *d_in, Jac<F> *d_out, unsigned log_n, const Fr &w, const EcnttScalar *inv_n, Jac<F> *buf0, Jac<F> *buf1,
                 void *d_aff, Fr *d_tw, void *d_tbl, hipStream_t st) {
    using K = EcnttOf<F>;
    const size_t n = (size_t)1 << log_n, half_n = n / 2;
    auto *aff = (typename K::Aff *)d_aff;
    auto *tbl = (typename K::Tbl *)d_tbl;
    Jac<F> *buf[2] = {buf0, buf1};
    int rc;
    if (log_n >= 2) {
        rc = fr_powers_device(fr_elem_c261(w), Fr::one(), half_n, d_tw, st);
        if (rc) return rc;
    }
    const Jac<F> *src = d_in;
    if (inv_n) {
        rc = prepare_bases<F>(d_in, aff, n, st);
        if (rc) return rc;
        K::scale(ladder_blocks<F>(n), st, aff, *inv_n, n, tbl, buf[0]);
        src = buf[0];
    }
    // stage s writes buf[s & 1], but for the last one (the caller's array); a transform of two points has only stage 1,
    // which may not write the array it reads
    K::first((unsigned)((half_n * K::LANES + 255) / 256), st, src, log_n, buf[1]);
    for (unsigned s = 2; s <= log_n; s++) {
        const Jac<F> *from = buf[(s - 1) & 1];
        rc = prepare_bases<F>(from + half_n, aff, half_n, st);
        if (rc) return rc;
        K::stage(ladder_blocks<F>(half_n), st, from, aff, d_tw, log_n, s, tbl, s == log_n ? d_out : buf[s & 1]);
    }
    if (log_n == 1) HIPCHK(hipMemcpyAsync(d_out, buf[1], n * sizeof(Jac<F>), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipGetLastError());
    return LSA_OK;
}

namespace {
// omega must be a primitive 2^log_n-th root of unity: omega^(n/2) == -1 (omega == 1 for one point)
bool primitive_root(Fr w, size_t log_n) {
    if (log_n == 0) return w == Fr::one();
    for (size_t i = 1; i < log_n; i++) w = w.sqr();
    return w == Fr::zero() - Fr::one();
}

// the body of lsa_g1_ecntt / lsa_g2_ecntt.  Every refusal comes before the library is asked for a device.
template <class F>
int ecntt(const void *in_jac, void *out_jac, size_t log_n, const void *omega, int inverse, int on_device) {
    const char *who = EcnttOf<F>::NAME;
    if (!in_jac || !out_jac || !omega) { set_error("%s: null argument", who); return LSA_ERR_INVALID; }
    if (log_n > ECNTT_MAX_LOG) { set_error("%s: log_n = %zu exceeds the limit of %u", who, log_n, ECNTT_MAX_LOG); return LSA_ERR_INVALID; }
    const size_t n = (size_t)1 << log_n, bytes = n * sizeof(Jac<F>);
    if (in_jac != out_jac && overlap(in_jac, bytes, out_jac, bytes)) {
        set_error("%s: out overlaps in without being exactly in", who);
        return LSA_ERR_INVALID;
    }
    if (on_device && (misaligned(in_jac) || misaligned(out_jac))) { set_error("%s: device pointers must be 16-byte aligned", who); return LSA_ERR_INVALID; }
    Fr w;
    memcpy(&w, omega, sizeof w);
    w = fr_elem_canon(w);
    if (!primitive_root(w, log_n)) { set_error("%s: omega is not a primitive 2^%zu-th root of unity", who, log_n); return LSA_ERR_INVALID; }
    int rc = require_ready();
    if (rc) return rc;
    rc = msm_join(g.stream);
    if (rc) return rc;

    OperandFrame f(who, on_device);
    const Jac<F> *d_in = f.in<Jac<F>>(g_stage_ec_in, in_jac, bytes);
    Jac<F> *d_out = f.out<Jac<F>>(g_stage_ec_out, out_jac, bytes);
    if (log_n == 0) {
        if (f.rc()) return f.rc();
        if (d_in != d_out) HIPCHK(hipMemcpyAsync(d_out, d_in, bytes, hipMemcpyDeviceToDevice, g.stream));
        return f.download();
    }
    const EcnttPlan<F> plan((unsigned)log_n, inverse != 0);
    Jac<F> *b0 = f.scratch<Jac<F>>(g_stage_ec_ping[0], plan.ping);
    Jac<F> *b1 = f.scratch<Jac<F>>(g_stage_ec_ping[1], plan.ping);
    void *d_aff = f.scratch(g_stage_ec_aff, plan.aff);
    Fr *d_tw = f.scratch<Fr>(g_stage_ec_tw, plan.tw);
    void *d_tbl = f.scratch(g_stage_ec_tbl, plan.tbl);
    if (f.rc()) return f.rc();
    EcnttScalar inv_n;
    if (inverse) {
        w = w.inverse();
        Fr nn = Fr::one();
        for (size_t i = 0; i < log_n; i++) nn = nn.dbl();
        nn.inverse().to_canonical(inv_n.w);
    }
    rc = ecntt_device<F>(d_in, d_out, (unsigned)log_n, w, inverse ? &inv_n : nullptr, b0, b1, d_aff, d_tw, d_tbl, g.stream);
    if (rc) return rc;
    return f.download();
}
}  // namespace

}  // namespace lsa

using namespace lsa;

extern "C" {
int lsa_g1_ecntt(const void *in_jac, void *out_jac, size_t log_n, const void *omega, int inverse, int on_device) {
    LSA_TRACE_CALL("g1_ecntt", (size_t)1 << (log_n & 31));
    return ecntt<Fq>(in_jac, out_jac, log_n, omega, inverse, on_device);
}
int lsa_g2_ecntt(const void *in_jac, void *out_jac, size_t log_n, const void *omega, int inverse, int on_device) {
    LSA_TRACE_CALL("g2_ecntt", (size_t)1 << (log_n & 31));
    return ecntt<Fq2>(in_jac, out_jac, log_n, omega, inverse, on_device);
}
size_t lsa_ecntt_param(int which) {
    switch (which) {
    case LSA_ECNTT_PARAM_G1_RESIDENT_BUTTERFLIES: return (size_t)ECNTT_BLOCKS * 256;
    case LSA_ECNTT_PARAM_G2_RESIDENT_BUTTERFLIES: return (size_t)ECNTT_BLOCKS * (256 / ECNTT_G2_LANES);
    case LSA_ECNTT_PARAM_G2_LANES_PER_BUTTERFLY: return ECNTT_G2_LANES;
    case LSA_ECNTT_PARAM_MAX_LOG_N: return ECNTT_MAX_LOG;
    }
    return 0;
}
}  // extern "C"
