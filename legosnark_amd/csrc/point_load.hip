// legosnark_amd/csrc/point_load.hip -- reading and writing keys: batch decompression of libff's compressed points (is_zero, X,
// one bit of Y), the curve check of uncompressed ones, the G2 subgroup test, and the compressed form of result vectors
// (lsa_gN_decompress / lsa_gN_validate / lsa_gN_compress; the shim's lsa_load_points / lsa_dump_points sit on top).
//
// One lane per point, 256-lane workgroups, no LDS and no barriers.  All arithmetic is fp.h's canonical Fq / Fq2 (the bytes that
// cross the C-ABI are libff's Montgomery words, so nothing is converted); the roots and the subgroup chain are csrc/fq_sqrt.h.
//   k_decompress<F>   range check of the words, rhs = x^3 + b, the root, the sign rule, the point (or (0, 1, 0) and a status)
//   k_validate<F>     range check, Z == 0, Y^2 == X^3 + b Z^6
//   k_subgroup_g2     psi(P) == [6u^2]P for the lanes whose status is still LSA_PT_OK (a kernel of its own: launched only when
//                     the caller asks for the test; 127 doublings + 39 additions over Fq2 per point)
//   k_compress<F>     from the affine form of msm_bases.h's batch normalisation: X and the flag byte
//   k_count_rejected  statuses >= 2, one atomic per wavefront that holds any
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>

#include "capi_internal.h"
#include "fq_sqrt.h"

namespace lsa {
namespace {

// raw words < p
LSA_HD bool fq_in_range(const Fq &a) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) br = (((uint64_t)a.l[i] - LSA_P[i] - br) >> 32) & 1;
    return br != 0;
}
LSA_HD unsigned fq_parity(const Fq &a) {
    uint32_t w[8];
    a.to_canonical(w);
    return w[0] & 1u;
}

template <class F> struct PointField;
template <> struct PointField<Fq> {
    static LSA_HD Fq b() { return fq_words(LSA_FQ_B); }
    static LSA_HD bool in_range(const Fq &a) { return fq_in_range(a); }
    static LSA_HD bool sqrt(const Fq &a, Fq *r) { return fq_sqrt(a, r); }
    static LSA_HD unsigned parity(const Fq &y) { return fq_parity(y); }
};
template <> struct PointField<Fq2> {
    static LSA_HD Fq2 b() { return fq2_const(LSA_TWIST_B); }
    static LSA_HD bool in_range(const Fq2 &a) { return fq_in_range(a.c0) && fq_in_range(a.c1); }
    static LSA_HD bool sqrt(const Fq2 &a, Fq2 *r) { return fq2_sqrt(a, r); }
    static LSA_HD unsigned parity(const Fq2 &y) { return fq_parity(y.c0); }
};

template <class F>
__global__ __launch_bounds__(256) void k_decompress(const F *__restrict__ x, const uint8_t *__restrict__ flags, size_t n, Jac<F> *__restrict__ out,
                                                    uint8_t *__restrict__ status) {
    using PF = PointField<F>;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned f = flags[i];
    Jac<F> P = Jac<F>::inf();
    uint8_t st = LSA_PT_OK;
    if (f & ~3u) st = LSA_PT_MALFORMED;
    else if (f & 2u) st = LSA_PT_INFINITY;                       // X is ignored, as libff ignores it
    else {
        const F X = x[i];
        F Y;
        if (!PF::in_range(X)) st = LSA_PT_MALFORMED;
        else if (!PF::sqrt(X.sqr() * X + PF::b(), &Y)) st = LSA_PT_NOT_ON_CURVE;
        else {
            if (PF::parity(Y) != (f & 1u)) Y = Y.neg();          // (a G2 root (0, r2) has parity 0 either way: bit 0 set negates it)
            P = Jac<F>{X, Y, F::one()};
        }
    }
    out[i] = P;
    status[i] = st;
}

template <class F>
__global__ __launch_bounds__(256) void k_validate(const Jac<F> *__restrict__ pts, size_t n, uint8_t *__restrict__ status) {
    using PF = PointField<F>;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Jac<F> P = pts[i];
    uint8_t st = LSA_PT_OK;
    if (!PF::in_range(P.X) || !PF::in_range(P.Y) || !PF::in_range(P.Z)) st = LSA_PT_MALFORMED;
    else if (P.Z.is_zero()) st = LSA_PT_INFINITY;
    else {
        const F z2 = P.Z.sqr(), z6 = z2.sqr() * z2;
        if (P.Y.sqr() != P.X.sqr() * P.X + PF::b() * z6) st = LSA_PT_NOT_ON_CURVE;
    }
    status[i] = st;
}

// out: where a point that fails is replaced by (0, 1, 0) (decompression: out == pts), or null (validation)
__global__ __launch_bounds__(256) void k_subgroup_g2(const Jac<Fq2> *pts, size_t n, uint8_t *__restrict__ status, Jac<Fq2> *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || status[i] != LSA_PT_OK) return;
    if (g2_in_subgroup(pts[i])) return;
    status[i] = LSA_PT_NOT_IN_SUBGROUP;
    if (out) out[i] = Jac<Fq2>::inf();
}

template <class F>
__global__ __launch_bounds__(256) void k_compress(const Aff<F> *__restrict__ aff, size_t n, F *__restrict__ x, uint8_t *__restrict__ flags) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Aff<F> a = aff[i];
    if (a.is_inf()) {                                            // libff's zero() is (0, 1, 0): X = 0, and Y = 1 is odd
        x[i] = F::zero();
        flags[i] = 3;
        return;
    }
    x[i] = a.x;
    flags[i] = (uint8_t)PointField<F>::parity(a.y);
}

__global__ __launch_bounds__(256) void k_count_rejected(const uint8_t *__restrict__ status, size_t n, unsigned long long *count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool bad = i < n && status[i] >= LSA_PT_MALFORMED;
    const unsigned long long m = __ballot(bad);
    if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(count, (unsigned long long)__popcll(m));
}

// grow-only staging of the host-buffer calls and the affine form behind lsa_gN_compress (released by lsa_shutdown)
StageBuf g_pl_in, g_pl_flags, g_pl_out, g_pl_status, g_pl_aff, g_pl_count;

// n points of `each` bytes: the byte count fits size_t and the grid fits 2^31 - 1 workgroups
bool sizes_ok(const char *what, size_t n, size_t each, size_t *bytes) {
    if (!bytes_of(n, each, bytes) || (n + 255) / 256 > 0x7fffffffu) {
        set_error("%s: %zu points of %zu bytes overflow", what, n, each);
        return false;
    }
    return true;
}
unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

// d_status holds the statuses (queued on the stream): count the rejected ones into *n_rejected (blocking)
int count_rejected(const uint8_t *d_status, size_t n, uint64_t *n_rejected) {
    if (g_pl_count.ensure(sizeof(unsigned long long))) { set_error("point_load: hipMalloc failed"); return LSA_ERR_NOMEM; }
    HIPCHK(hipMemsetAsync(g_pl_count.p, 0, sizeof(unsigned long long), g.stream));
    hipLaunchKernelGGL(k_count_rejected, dim3(blocks_of(n)), dim3(256), 0, g.stream, d_status, n, (unsigned long long *)g_pl_count.p);
    HIPCHK(hipGetLastError());
    unsigned long long c = 0;
    HIPCHK(hipMemcpyAsync(&c, g_pl_count.p, sizeof c, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    *n_rejected = c;
    return LSA_OK;
}

template <class F>
int decompress_any(const char *what, const void *x, const uint8_t *flags, size_t n, int check_subgroup, void *out, uint8_t *status, uint64_t *n_rejected,
                   int on_device) {
    LSA_TRACE_CALL(what, n);
    int rc = require_ready();
    if (rc) return rc;
    size_t x_bytes, out_bytes;
    if (!sizes_ok(what, n, sizeof(F), &x_bytes) || !sizes_ok(what, n, sizeof(Jac<F>), &out_bytes)) return LSA_ERR_INVALID;
    if (n == 0) { if (n_rejected) *n_rejected = 0; return LSA_OK; }
    if (!x || !flags || !out || !status) { set_error("%s: null argument", what); return LSA_ERR_INVALID; }
    if (overlap(out, out_bytes, x, x_bytes) || overlap(out, out_bytes, flags, n) || overlap(status, n, x, x_bytes) || overlap(status, n, flags, n) ||
        overlap(out, out_bytes, status, n)) { set_error("%s: an output overlaps an input or the other output", what); return LSA_ERR_INVALID; }
    OperandFrame f(what, on_device);
    const F *d_x = f.in<F>(g_pl_in, x, x_bytes);
    const uint8_t *d_flags = f.in<uint8_t>(g_pl_flags, flags, n);
    Jac<F> *d_out = f.out<Jac<F>>(g_pl_out, out, out_bytes);
    uint8_t *d_status = f.out<uint8_t>(g_pl_status, status, n);
    if (f.rc()) return f.rc();
    hipLaunchKernelGGL((k_decompress<F>), dim3(blocks_of(n)), dim3(256), 0, g.stream, d_x, d_flags, n, d_out, d_status);
    if constexpr (std::is_same<F, Fq2>::value) {
        if (check_subgroup) hipLaunchKernelGGL(k_subgroup_g2, dim3(blocks_of(n)), dim3(256), 0, g.stream, (const Jac<Fq2> *)d_out, n, d_status, d_out);
    }
    HIPCHK(hipGetLastError());
    if (n_rejected) { rc = count_rejected(d_status, n, n_rejected); if (rc) return rc; }
    return f.download();
}

template <class F>
int validate_any(const char *what, const void *pts, size_t n, int check_subgroup, uint8_t *status, uint64_t *n_rejected, int on_device) {
    LSA_TRACE_CALL(what, n);
    int rc = require_ready();
    if (rc) return rc;
    size_t in_bytes;
    if (!sizes_ok(what, n, sizeof(Jac<F>), &in_bytes)) return LSA_ERR_INVALID;
    if (n == 0) { if (n_rejected) *n_rejected = 0; return LSA_OK; }
    if (!pts || !status) { set_error("%s: null argument", what); return LSA_ERR_INVALID; }
    if (overlap(status, n, pts, in_bytes)) { set_error("%s: status overlaps the points", what); return LSA_ERR_INVALID; }
    OperandFrame f(what, on_device);
    const Jac<F> *d_pts = f.in<Jac<F>>(g_pl_out, pts, in_bytes);
    uint8_t *d_status = f.out<uint8_t>(g_pl_status, status, n);
    if (f.rc()) return f.rc();
    hipLaunchKernelGGL((k_validate<F>), dim3(blocks_of(n)), dim3(256), 0, g.stream, d_pts, n, d_status);
    if constexpr (std::is_same<F, Fq2>::value) {
        if (check_subgroup) hipLaunchKernelGGL(k_subgroup_g2, dim3(blocks_of(n)), dim3(256), 0, g.stream, d_pts, n, d_status, (Jac<Fq2> *)nullptr);
    }
    HIPCHK(hipGetLastError());
    if (n_rejected) { rc = count_rejected(d_status, n, n_rejected); if (rc) return rc; }
    return f.download();
}

template <class F>
int compress_any(const char *what, const void *pts, size_t n, void *x, uint8_t *flags, int on_device) {
    LSA_TRACE_CALL(what, n);
    int rc = require_ready();
    if (rc) return rc;
    size_t in_bytes, x_bytes, aff_bytes;
    if (!sizes_ok(what, n, sizeof(Jac<F>), &in_bytes) || !sizes_ok(what, n, sizeof(F), &x_bytes) || !sizes_ok(what, n, sizeof(Aff<F>), &aff_bytes)) return LSA_ERR_INVALID;
    if (n == 0) return LSA_OK;
    if (!pts || !x || !flags) { set_error("%s: null argument", what); return LSA_ERR_INVALID; }
    if (overlap(x, x_bytes, pts, in_bytes) || overlap(flags, n, pts, in_bytes) || overlap(x, x_bytes, flags, n)) {
        set_error("%s: an output overlaps the points or the other output", what);
        return LSA_ERR_INVALID;
    }
    OperandFrame f(what, on_device);
    Aff<F> *d_aff = f.scratch<Aff<F>>(g_pl_aff, aff_bytes);
    const Jac<F> *d_pts = f.in<Jac<F>>(g_pl_out, pts, in_bytes);
    F *d_x = f.out<F>(g_pl_in, x, x_bytes);
    uint8_t *d_flags = f.out<uint8_t>(g_pl_flags, flags, n);
    if (f.rc()) return f.rc();
    rc = normalize_to_affine<F>(d_pts, d_aff, n, g.stream);
    if (rc) return rc;
    hipLaunchKernelGGL((k_compress<F>), dim3(blocks_of(n)), dim3(256), 0, g.stream, (const Aff<F> *)d_aff, n, d_x, d_flags);
    HIPCHK(hipGetLastError());
    return f.download();
}

}  // namespace

}  // namespace lsa

using namespace lsa;

extern "C" {
int lsa_g1_decompress(const void *x_mont, const uint8_t *flags, size_t n, void *out_jac, uint8_t *status, uint64_t *n_rejected, int on_device) {
    return decompress_any<Fq>("g1_decompress", x_mont, flags, n, 0, out_jac, status, n_rejected, on_device);
}
int lsa_g2_decompress(const void *x_mont, const uint8_t *flags, size_t n, int check_subgroup, void *out_jac, uint8_t *status, uint64_t *n_rejected,
                      int on_device) {
    return decompress_any<Fq2>("g2_decompress", x_mont, flags, n, check_subgroup, out_jac, status, n_rejected, on_device);
}
int lsa_g1_validate(const void *pts_jac, size_t n, uint8_t *status, uint64_t *n_rejected, int on_device) {
    return validate_any<Fq>("g1_validate", pts_jac, n, 0, status, n_rejected, on_device);
}
int lsa_g2_validate(const void *pts_jac, size_t n, int check_subgroup, uint8_t *status, uint64_t *n_rejected, int on_device) {
    return validate_any<Fq2>("g2_validate", pts_jac, n, check_subgroup, status, n_rejected, on_device);
}
int lsa_g1_compress(const void *pts_jac, size_t n, void *x_mont, uint8_t *flags, int on_device) {
    return compress_any<Fq>("g1_compress", pts_jac, n, x_mont, flags, on_device);
}
int lsa_g2_compress(const void *pts_jac, size_t n, void *x_mont, uint8_t *flags, int on_device) {
    return compress_any<Fq2>("g2_compress", pts_jac, n, x_mont, flags, on_device);
}
}  // extern "C"
