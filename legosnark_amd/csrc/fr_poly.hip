// legosnark_amd/csrc/fr_poly.hip -- the Lipmaa Hadamard prover's polynomial work between its transforms and its MSM, and the
// key generator's Lagrange row, on device-resident vectors (lsa_fr_hadamard_quotient, lsa_fr_lagrange).
//
// Replaces, for the reference's src/gadgets/lipmaa.cc:103-176 and src/prototools/interp.h:68-71, the host loops of the shim's
// evaluation domains (shim/libfqfft/evaluation_domain/get_evaluation_domain.hpp): the three pointwise loops of
// CPHadL::prove, divide_by_Z_on_coset, add_poly_Z and evaluate_all_lagrange_polynomials, over the basic radix-2 domain and
// the step radix-2 domain.  The seven transforms are ntt.hip's (fr_ntt_device / fr_ntt_step_device).
//
// Quotient.  H = d2 A + d1 B - d3 + d1 d2 Z + (A B - C) / Z.  Everything but the three monomial corrections has degree < m,
// so it is interpolated from its values on the coset g * domain in ONE inverse transform:
//     iFFT a, b, c;  cosetFFT A, B, C;  h[i] = (A B - C)(g x_i) / Z(g x_i) + d2 A(g x_i) + d1 B(g x_i)   (k_hq_point);
//     icosetFFT h (in h_out itself);  then -d3 - d1 d2 Z's monomials onto at most four entries, h[m] among them (k_hq_fix).
// The reference adds d2 A + d1 B in coefficient form (a pass over three vectors before the coset transforms and one after
// the last): the same polynomial, and Fr values are canonical residues, so the same bytes.
//
// k_hq_point runs on fr29.h's limbs (fr_batch_inv.h: fr_hq_point): 5 schoolbook products and 2 reductions per element
// (3.5 products), 4 vectors of traffic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "capi_internal.h"
#include "fr29.h"
#include "fr_batch_inv.h"
#include "ntt_core.h"

namespace lsa {

// ---------------------------------------------------------------- rows (fr_batch_inv.h): one run per lane
constexpr unsigned ROW_BLOCK = 64;            // few, long-running lanes: small workgroups spread them over the CUs
__global__ __launch_bounds__(ROW_BLOCK) void k_fr_geom_row(FrGeomRow r, size_t count, Fr *out) {
    const size_t lo = ((size_t)blockIdx.x * ROW_BLOCK + threadIdx.x) * FR_BATCH_INV_RUN;
    if (lo >= count) return;
    const size_t left = count - lo;
    fr_geom_row_run(r, lo, (unsigned)(left < FR_BATCH_INV_RUN ? left : FR_BATCH_INV_RUN), out);
}
// out[i] = (p w^i == t) ? 1 : 0: the Lagrange row at a point OF the domain
__global__ __launch_bounds__(ROW_BLOCK) void k_fr_unit_row(Fr w, Fr p, Fr t, size_t count, Fr *out) {
    const size_t lo = ((size_t)blockIdx.x * ROW_BLOCK + threadIdx.x) * FR_BATCH_INV_RUN;
    if (lo >= count) return;
    Fr x = p * fr_pow_u64(w, lo);
    for (size_t i = lo; i < lo + FR_BATCH_INV_RUN && i < count; i++) {
        out[i] = x == t ? Fr::one() : Fr::zero();
        x = x * w;
    }
}

// ---------------------------------------------------------------- the quotient's two pointwise kernels
// h[i] = (A[i] B[i] - C[i]) Zinv_i + d2 A[i] + d1 B[i], i < m (fr_hq_point).  Zinv_i 2^10: ztab[i & zmask] for i < zbig, k.zinv
// elsewhere (zbig = 0 on the basic domain).  h may be A (each lane reads its elements before it writes them).
__global__ __launch_bounds__(256) void k_hq_point(const Fr *A, const Fr *__restrict__ B, const Fr *__restrict__ C, Fr *h, size_t m,
                                                  const Fr *__restrict__ ztab, size_t zbig, size_t zmask, FrHqConsts k) {
    const size_t T = (size_t)gridDim.x * blockDim.x;
    const Fr29 zc = Fr29::from_words(k.zinv), d1 = Fr29::from_words(k.d1), d2 = Fr29::from_words(k.d2), neg = Fr29::from_words(k.neg);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += T) {
        const Fr29 a = Fr29::from_words(A[i]), b = Fr29::from_words(B[i]), c = Fr29::from_words(C[i]);
        h[i] = fr_hq_point(a, b, c, i < zbig ? Fr29::from_words(ztab[i & zmask]) : zc, d1, d2, neg);
    }
}
// the monomials of -d3 + d1 d2 Z onto at most four entries (fr_hq_fix)
__global__ __launch_bounds__(64) void k_hq_fix(Fr *h, FrHqFix f) {
    const int j = (int)threadIdx.x;
    if (j >= f.n) return;
    h[f.idx[j]] = f.set[j] ? f.val[j] : h[f.idx[j]] + f.val[j];
}

// ---------------------------------------------------------------- host side
namespace {
// (every field operation of the host side is inside fr_batch_inv.h's __host__ __device__ helpers: fp.h's operator* is
// another function in the device pass)
// grow-only staging (released by lsa_shutdown): two working vectors, the transforms' second buffer, the step domain's
// table of Zinv, and for host callers the result
StageBuf g_poly_b, g_poly_c, g_poly_tmp, g_poly_h, g_poly_ztab;
// (what g_poly_ztab holds; a released table has cap 0, and lsa_fr_hadamard_quotient drops the key whenever the table is too small)
struct ZtabKey { bool valid = false; unsigned big_log = 0, small_log = 0; Fr omega, g; } g_ztab_key;

unsigned row_blocks(size_t count) { return (unsigned)(((count + FR_BATCH_INV_RUN - 1) / FR_BATCH_INV_RUN + ROW_BLOCK - 1) / ROW_BLOCK); }
int launch_row(const FrGeomRow &r, size_t count, Fr *out, hipStream_t st) {
    hipLaunchKernelGGL(k_fr_geom_row, dim3(row_blocks(count)), dim3(ROW_BLOCK), 0, st, r, count, out);
    HIPCHK(hipGetLastError());
    return LSA_OK;
}
int launch_unit(const Fr &w, const Fr &p, const Fr &t, size_t count, Fr *out, hipStream_t st) {
    hipLaunchKernelGGL(k_fr_unit_row, dim3(row_blocks(count)), dim3(ROW_BLOCK), 0, st, w, p, t, count, out);
    HIPCHK(hipGetLastError());
    return LSA_OK;
}

// the domain arguments of both entry points (those of lsa_fr_ntt / lsa_fr_ntt_step, and m >= 2)
int check_domain(const char *who, size_t big_log, int small_log) {
    if (small_log < 0) {
        if (big_log < 1 || big_log > 28) { set_error("%s: need 1 <= big_log <= 28 on the basic domain (got %zu): m >= 2, and Fr has 2-adicity 28", who, big_log); return LSA_ERR_INVALID; }
    } else if (big_log > 27 || (size_t)small_log >= big_log) {
        set_error("%s: need small_log < big_log <= 27 on the step domain (got %d, %zu): omega is a 2^(big_log + 1)-th root of unity of a field of 2-adicity 28", who, small_log, big_log);
        return LSA_ERR_INVALID;
    }
    return LSA_OK;
}
}  // namespace

// d_h: m + 1 elements holding a (n values, the rest zero) on entry and H on return; d_b, d_c: m elements holding b and c,
// destroyed; d_tmp: the transforms' second buffer.  Asynchronous on st.
static int hadamard_quotient_device(Fr *d_h, Fr *d_b, Fr *d_c, unsigned big_log, int small_log, const Fr &omega, const Fr &g, const Fr d[3],
                                    Fr *d_tmp, hipStream_t st) {
    const bool step = small_log >= 0;
    const size_t big = (size_t)1 << big_log, small = step ? (size_t)1 << small_log : 0, m = big + small;
    Fr *v[3] = {d_h, d_b, d_c};
    int rc;
    for (int inverse = 1; inverse >= 0; inverse--)
        for (int j = 0; j < 3; j++) {
            rc = step ? fr_ntt_step_device(v[j], big_log, (unsigned)small_log, omega, inverse != 0, inverse ? nullptr : &g, d_tmp, st)
                      : fr_ntt_device(v[j], big_log, omega, inverse != 0, inverse ? nullptr : &g, d_tmp, st);
            if (rc) return rc;
        }
    const Fr up10 = Fr::from_u32(1024);                    // 1 / Z carries 2^10 into the kernel (fr_hq_point)
    FrHqConsts k = fr_hq_consts(Fr::one(), d[0], d[1]);
    const Fr *ztab = nullptr;
    size_t zbig = 0, zmask = 0;
    if (!step) {
        k.zinv = fr_basic_zinv(big_log, g, up10);
    } else {
        const FrStepZinv z = fr_step_zinv(big_log, (unsigned)small_log, omega, g, up10);
        k.zinv = z.small_part;
        ZtabKey &key = g_ztab_key;
        if (!(key.valid && key.big_log == big_log && key.small_log == (unsigned)small_log && memcmp(&key.omega, &omega, sizeof(Fr)) == 0 &&
              memcmp(&key.g, &g, sizeof(Fr)) == 0)) {
            key.valid = false;
            rc = launch_row(z.table, z.period, (Fr *)g_poly_ztab.p, st);
            if (rc) return rc;
            key.valid = true; key.big_log = big_log; key.small_log = (unsigned)small_log; key.omega = omega; key.g = g;
        }
        ztab = (const Fr *)g_poly_ztab.p;
        zbig = big;
        zmask = z.period - 1;
    }
    const size_t blocks = (m + 4 * 256 - 1) / (4 * 256);
    hipLaunchKernelGGL(k_hq_point, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, (const Fr *)d_h, (const Fr *)d_b, (const Fr *)d_c, d_h, m,
                       ztab, zbig, zmask, k);
    HIPCHK(hipGetLastError());
    rc = step ? fr_ntt_step_device(d_h, big_log, (unsigned)small_log, omega, true, &g, d_tmp, st) : fr_ntt_device(d_h, big_log, omega, true, &g, d_tmp, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_hq_fix, dim3(1), dim3(64), 0, st, d_h, fr_hq_fix(big_log, small_log, omega, d));
    HIPCHK(hipGetLastError());
    return LSA_OK;
}

// out: m elements.  Asynchronous on st.
static int lagrange_device(Fr *d_out, unsigned big_log, int small_log, const Fr &omega, const Fr &t, hipStream_t st) {
    const FrLagrangePlan p = fr_lagrange_plan(big_log, small_log, omega, t);
    size_t at = 0;
    for (int j = 0; j < p.parts; j++) {
        const int rc = p.unit ? launch_unit(p.unit_w[j], p.unit_p[j], t, p.count[j], d_out + at, st) : launch_row(p.row[j], p.count[j], d_out + at, st);
        if (rc) return rc;
        at += p.count[j];
    }
    return LSA_OK;
}

}  // namespace lsa

using namespace lsa;

extern "C" {
int lsa_fr_hadamard_quotient(const void *a, const void *b, const void *c, size_t n, size_t big_log, int small_log, const void *omega,
                             const void *coset_g, const void *d123, void *h_out, int on_device) {
    int rc = require_ready();
    if (rc) return rc;
    rc = check_domain("fr_hadamard_quotient", big_log, small_log);
    if (rc) return rc;
    LSA_TRACE_CALL("fr_hadamard_quotient", ((size_t)1 << big_log) + (small_log >= 0 ? (size_t)1 << small_log : 0));
    // (a, b, c may be null when n == 0: an empty device tensor has no address)
    if ((n && (!a || !b || !c)) || !omega || !coset_g || !d123 || !h_out) { set_error("fr_hadamard_quotient: null argument"); return LSA_ERR_INVALID; }
    const bool step = small_log >= 0;
    const size_t big = (size_t)1 << big_log, m = big + (step ? (size_t)1 << small_log : 0);
    if (n > m) { set_error("fr_hadamard_quotient: n = %zu values on a domain of m = %zu points", n, m); return LSA_ERR_INVALID; }
    Fr w, cg, d[3];
    memcpy(&w, omega, sizeof w);
    memcpy(&cg, coset_g, sizeof cg);
    memcpy(d, d123, sizeof d);
    if (fr_coset_meets_roots((unsigned)big_log, small_log, cg)) {
        set_error("fr_hadamard_quotient: coset_g^%s = 1: the vanishing polynomial may have a root on this coset of the domain", step ? "(2 * 2^big_log)" : "m");
        return LSA_ERR_INVALID;
    }
    const size_t tmp_elems = step ? big : (big_log > NTT_TILE_LOG ? m : 0), period = step ? big >> small_log : 0;
    OperandFrame f("fr_hadamard_quotient", on_device);
    Fr *d_b = f.scratch<Fr>(g_poly_b, m * sizeof(Fr)), *d_c = f.scratch<Fr>(g_poly_c, m * sizeof(Fr));
    Fr *d_tmp = f.scratch<Fr>(g_poly_tmp, tmp_elems * sizeof(Fr));
    Fr *d_h = f.out<Fr>(g_poly_h, h_out, (m + 1) * sizeof(Fr));
    if (period * sizeof(Fr) > g_poly_ztab.cap) g_ztab_key.valid = false;
    f.scratch(g_poly_ztab, period * sizeof(Fr));
    if (f.rc()) return f.rc();
    // a, b, c into the working vectors, zero-padded to the domain (not operands of the frame: a device caller's are copied too)
    Fr *dv[3] = {d_h, d_b, d_c};
    const void *src[3] = {a, b, c};
    for (int j = 0; j < 3; j++) {
        if (n) {
            if (on_device) HIPCHK(hipMemcpyAsync(dv[j], src[j], n * sizeof(Fr), hipMemcpyDeviceToDevice, g.stream));
            else LSA_UPLOAD(dv[j], src[j], n * sizeof(Fr));
        }
        if (n < m) HIPCHK(hipMemsetAsync(dv[j] + n, 0, (m - n) * sizeof(Fr), g.stream));
    }
    rc = hadamard_quotient_device(d_h, d_b, d_c, (unsigned)big_log, small_log, w, cg, d, d_tmp, g.stream);
    if (rc) return rc;
    return f.download();              // (host callers: enqueued behind the kernels, as in lsa_fr_ntt)
}

int lsa_fr_lagrange(size_t big_log, int small_log, const void *omega, const void *t, void *out, int on_device) {
    int rc = require_ready();
    if (rc) return rc;
    rc = check_domain("fr_lagrange", big_log, small_log);
    if (rc) return rc;
    const size_t m = ((size_t)1 << big_log) + (small_log >= 0 ? (size_t)1 << small_log : 0);
    LSA_TRACE_CALL("fr_lagrange", m);
    if (!omega || !t || !out) { set_error("fr_lagrange: null argument"); return LSA_ERR_INVALID; }
    Fr w, tt;
    memcpy(&w, omega, sizeof w);
    memcpy(&tt, t, sizeof tt);
    OperandFrame f("fr_lagrange", on_device);
    Fr *d_out = f.out<Fr>(g_poly_h, out, m * sizeof(Fr));
    if (f.rc()) return f.rc();
    rc = lagrange_device(d_out, (unsigned)big_log, small_log, w, tt, g.stream);
    if (rc) return rc;
    return f.download();
}
}  // extern "C"
