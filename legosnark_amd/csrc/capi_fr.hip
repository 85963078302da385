// legosnark_amd/csrc/capi_fr.hip -- the Fr-vector and NTT entry points of include/legosnark_amd.h (the kernels are in
// fr_vec.hip and ntt.hip).  No kernels here.
#include <hip/hip_runtime.h>
#include <string.h>

#include "capi_internal.h"
#include "fr_elem.h"
#include "ntt_core.h"

using namespace lsa;

// grow-only device staging buffers (StageBuf, staging.h)
namespace {
StageBuf g_stage_ntt_a, g_stage_ntt_tmp;         // lsa_fr_ntt: the data of host callers, the second buffer of the passes
// the Fr recursions (lsa_fr_cppoly_witness, lsa_fr_eval_mle): scratch, and for host callers v / r / w -- grow-only like the
// others (round 5; before, every call paid a hipMalloc + hipFree pair per buffer, and the recursions' cached hipGraphs
// (fr_vec.hip) are keyed by these pointers)
StageBuf g_stage_fr_tmp, g_stage_fr_v, g_stage_fr_r, g_stage_fr_w;
StageBuf g_stage_sc_partial, g_stage_sc_out;     // lsa_fr_sumcheck_round: block partials and the coefficients (one call per round of a prover)
// the element-wise calls (fr_elem.hip): for host callers the operands and the result; for every caller the block partials of
// lsa_fr_poly_eval and the zero counter of lsa_fr_batch_inverse
StageBuf g_stage_el_x[FR_VEC_LINCOMB_MAX], g_stage_el_out, g_stage_el_partial, g_stage_el_count;
constexpr size_t FR_VEC_MAX_N = (size_t)1 << 40;   // elements per call: the run kernels' grids stay below 2^31 workgroups

// The checks the element-wise calls share, before any device work: every vector non-null, n * 32 within size_t, n within
// FR_VEC_MAX_N, device pointers 16-byte aligned, and out either exactly an input (when `in_place` allows it) or apart from it.
int vec_args(const char *who, const void *const *ins, size_t nin, const void *out, size_t out_elems, size_t n, bool in_place, int on_device, size_t *bytes) {
    if (!fr_bytes_of(n, 1, bytes) || n > FR_VEC_MAX_N) { set_error("%s: n = %zu exceeds the limit of 2^40 elements per call", who, n); return LSA_ERR_INVALID; }
    if (!out) { set_error("%s: null argument", who); return LSA_ERR_INVALID; }
    if (on_device && misaligned(out)) { set_error("%s: device pointers must be 16-byte aligned", who); return LSA_ERR_INVALID; }
    for (size_t t = 0; t < nin; t++) {
        if (!ins[t]) { set_error("%s: null argument", who); return LSA_ERR_INVALID; }
        if (on_device && misaligned(ins[t])) { set_error("%s: device pointers must be 16-byte aligned", who); return LSA_ERR_INVALID; }
        if (in_place && ins[t] == out) continue;
        if (overlap(ins[t], *bytes, out, out_elems * sizeof(Fr))) {
            set_error("%s: out overlaps an input%s", who, in_place ? " without being exactly that input" : "");
            return LSA_ERR_INVALID;
        }
    }
    return LSA_OK;
}
Fr load_fr(const void *p) {
    Fr x;
    memcpy(&x, p, sizeof x);
    return x;
}
}  // namespace

// ---------------------------------------------------------------- Fr vectors
extern "C" {
int lsa_fr_cppoly_witness(const void *v, size_t d, const void *r, void *w, int on_device) {
    LSA_TRACE_CALL("fr_cppoly_witness", (size_t)1 << d);
    int rc = require_ready();
    if (rc) return rc;
    if (d > 40) { set_error("cppoly_witness: d = %zu too large", d); return LSA_ERR_INVALID; }
    if (!v || !w || (d && !r)) { set_error("cppoly_witness: null argument"); return LSA_ERR_INVALID; }
    const size_t N = (size_t)1 << d;
    OperandFrame f("cppoly_witness", on_device);
    Fr *d_tmp = f.scratch<Fr>(g_stage_fr_tmp, (N / 2 + N / 4 + 1) * sizeof(Fr));
    const Fr *d_v = f.in<Fr>(g_stage_fr_v, v, N * sizeof(Fr));
    const Fr *d_r = f.in<Fr>(g_stage_fr_r, r, d * sizeof(Fr), (d + 1) * sizeof(Fr));
    Fr *d_w = f.out<Fr>(g_stage_fr_w, w, N * sizeof(Fr));
    if (f.rc()) return f.rc();
    rc = fr_cppoly_fold_device(d_v, d, d_r, d_w, d_tmp, g.stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));   // (device callers read w from their own streams)
    return f.download();
}

int lsa_fr_eval_mle(const void *v, size_t d, const void *r, void *out, int on_device) {
    LSA_TRACE_CALL("fr_eval_mle", (size_t)1 << d);
    int rc = require_ready();
    if (rc) return rc;
    if (d > 40) { set_error("eval_mle: d = %zu too large", d); return LSA_ERR_INVALID; }
    if (!v || !out || (d && !r)) { set_error("eval_mle: null argument"); return LSA_ERR_INVALID; }
    const size_t N = (size_t)1 << d;
    OperandFrame f("eval_mle", on_device);
    Fr *d_tmp = f.scratch<Fr>(g_stage_fr_tmp, (N / 2 + N / 4 + 1) * sizeof(Fr));
    const Fr *d_v = f.in<Fr>(g_stage_fr_v, v, N * sizeof(Fr));
    const Fr *d_r = f.in<Fr>(g_stage_fr_r, r, d * sizeof(Fr), (d + 1) * sizeof(Fr));
    Fr *d_o = f.out<Fr>(g_stage_fr_w, out, sizeof(Fr));
    if (f.rc()) return f.rc();
    rc = fr_eval_mle_device(d_v, d, d_r, d_tmp, d_o, g.stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return f.download();
}

int lsa_fr_sumcheck_round(const void *suff, const void *const *tables, size_t m, size_t half, const void *pre, const void *rho_j,
                          void *out_coeffs, int on_device) {
    int rc = require_ready();
    if (rc) return rc;
    if (!tables || !out_coeffs || m == 0 || m > 4 || half == 0) { set_error("sumcheck_round: invalid argument (1 <= m <= 4, half > 0)"); return LSA_ERR_INVALID; }
    if (rho_j && !pre) { set_error("sumcheck_round: rho_j without pre"); return LSA_ERR_INVALID; }
    for (size_t t = 0; t < m; t++) if (!tables[t]) { set_error("sumcheck_round: null table"); return LSA_ERR_INVALID; }
    const size_t ncoef = m + (rho_j ? 2 : 1);
    DevBuf d_suff, d_tab[4];
    OperandFrame f("sumcheck_round", on_device);
    Fr *d_partial = f.scratch<Fr>(g_stage_sc_partial, fr_sumcheck_scratch_elems() * sizeof(Fr));
    Fr *d_out = f.scratch<Fr>(g_stage_sc_out, 8 * sizeof(Fr));       // (the coefficients go to host memory for every caller)
    const Fr *tabs[4] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t t = 0; t < m; t++) tabs[t] = f.in<Fr>(d_tab[t], tables[t], 2 * half * sizeof(Fr));
    const Fr *sf = suff ? f.in<Fr>(d_suff, suff, half * sizeof(Fr)) : nullptr;
    if (f.rc()) return f.rc();
    rc = fr_sumcheck_round_device(sf, tabs, m, half, (const Fr *)pre, (const Fr *)rho_j, d_partial, d_out, g.stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    LSA_DOWNLOAD(out_coeffs, d_out, ncoef * sizeof(Fr));
    return LSA_OK;
}

int lsa_fr_scale_upper(const void *old, size_t half, const void *k, void *cur, int on_device) {
    LSA_TRACE_CALL("fr_scale_upper", half);
    int rc = require_ready();
    if (rc) return rc;
    if (half == 0) return LSA_OK;
    if (!old || !cur || !k) { set_error("fr_scale_upper: null argument"); return LSA_ERR_INVALID; }
    Fr kk;
    memcpy(&kk, k, sizeof kk);
    DevBuf d_v;
    OperandFrame f("fr_scale_upper", on_device);
    const Fr *d_old = f.in<Fr>(d_v, old, 2 * half * sizeof(Fr));
    Fr *d_cur = f.out_in<Fr>(d_old, cur, half * sizeof(Fr));          // (host callers: in place in the staged copy)
    if (f.rc()) return f.rc();
    rc = fr_scale_upper_device(d_old, half, kk, d_cur, g.stream);
    if (rc) return rc;
    if (!on_device) HIPCHK(hipStreamSynchronize(g.stream));
    return f.download();
}

int lsa_fr_eq_table(const void *r, size_t d, int variant, void *out, int on_device) {
    LSA_TRACE_CALL("fr_eq_table", (size_t)1 << (d & 63));
    int rc = require_ready();
    if (rc) return rc;
    if (d == 0 || d > 30) { set_error("fr_eq_table: need 1 <= d <= 30 (got %zu)", d); return LSA_ERR_INVALID; }
    if (!out || (d && !r)) { set_error("fr_eq_table: null argument"); return LSA_ERR_INVALID; }
    if (variant != 0 && variant != 1) { set_error("fr_eq_table: variant %d (0: the reference's loop, 1: the eq monomials)", variant); return LSA_ERR_INVALID; }
    const size_t N = (size_t)1 << d;
    OperandFrame f("fr_eq_table", on_device);
    Fr *d_tmp = f.scratch<Fr>(g_stage_fr_tmp, fr_eq_table_scratch_elems(d) * sizeof(Fr));
    const Fr *d_r = f.in<Fr>(g_stage_fr_r, r, d * sizeof(Fr), (d + 1) * sizeof(Fr));
    Fr *d_o = f.out<Fr>(g_stage_fr_w, out, N * sizeof(Fr));
    if (f.rc()) return f.rc();
    rc = fr_eq_table_device(d_r, d, variant, d_tmp, d_o, g.stream);
    if (rc) return rc;
    if (!on_device) HIPCHK(hipStreamSynchronize(g.stream));
    return f.download();
}

int lsa_fr_ntt(void *a, size_t log_n, const void *omega, int inverse, const void *coset_g, int on_device) {
    LSA_TRACE_CALL("fr_ntt", (size_t)1 << log_n);
    int rc = require_ready();
    if (rc) return rc;
    if (log_n > 28) { set_error("fr_ntt: log_n = %zu exceeds the 2-adicity of Fr (28)", log_n); return LSA_ERR_INVALID; }
    if (!a || !omega) { set_error("fr_ntt: null argument"); return LSA_ERR_INVALID; }
    if (log_n == 0) return LSA_OK;
    const size_t n = (size_t)1 << log_n;
    Fr w, gco;
    memcpy(&w, omega, sizeof w);
    if (coset_g) memcpy(&gco, coset_g, sizeof gco);
    // grow-only staging (released by lsa_shutdown, like every other staging buffer) for the second buffer of the passes
    // and, for host callers, the data: two hipMalloc / hipFree pairs per call cost a 2^20-point transform of an unchanged
    // prover more than its kernels (the shim's evaluation_domain calls this 7 times per Lipmaa proof).  The twiddle
    // tables are cached per domain inside ntt.hip.
    OperandFrame f("fr_ntt", on_device);
    if (log_n > NTT_TILE_LOG) f.scratch(g_stage_ntt_tmp, n * sizeof(Fr));
    Fr *d_a = f.inout<Fr>(g_stage_ntt_a, a, n * sizeof(Fr));
    if (f.rc()) return f.rc();
    rc = fr_ntt_device(d_a, (unsigned)log_n, w, inverse != 0, coset_g ? &gco : nullptr, (Fr *)g_stage_ntt_tmp.p, g.stream);
    if (rc) return rc;
    // (The download is enqueued BEHIND the kernels, not after a wait for them: the first device -> host copy a process
    // issues on an idle stream costs it 8 ms of copy-engine set-up on this stack.)
    if (on_device) HIPCHK(hipStreamSynchronize(g.stream));
    return f.download();
}

int lsa_fr_ntt_step(void *a, size_t big_log, size_t small_log, const void *omega, int inverse, const void *coset_g, int on_device) {
    LSA_TRACE_CALL("fr_ntt_step", ((size_t)1 << (big_log & 31)) + ((size_t)1 << (small_log & 31)));
    int rc = require_ready();
    if (rc) return rc;
    if (big_log > 27 || small_log >= big_log) {
        set_error("fr_ntt_step: need small_log < big_log <= 27 (got %zu, %zu): omega is a 2^(big_log + 1)-th root of unity of a field of 2-adicity 28", small_log, big_log);
        return LSA_ERR_INVALID;
    }
    if (!a || !omega) { set_error("fr_ntt_step: null argument"); return LSA_ERR_INVALID; }
    const size_t big = (size_t)1 << big_log, m = big + ((size_t)1 << small_log);
    Fr w, gco;
    memcpy(&w, omega, sizeof w);
    if (coset_g) memcpy(&gco, coset_g, sizeof gco);
    OperandFrame f("fr_ntt_step", on_device);
    Fr *d_tmp = f.scratch<Fr>(g_stage_ntt_tmp, big * sizeof(Fr));
    Fr *d_a = f.inout<Fr>(g_stage_ntt_a, a, m * sizeof(Fr));
    if (f.rc()) return f.rc();
    rc = fr_ntt_step_device(d_a, (unsigned)big_log, (unsigned)small_log, w, inverse != 0, coset_g ? &gco : nullptr, d_tmp, g.stream);
    if (rc) return rc;
    if (on_device) HIPCHK(hipStreamSynchronize(g.stream));
    return f.download();
}

int lsa_fr_fold(const void *old, size_t half, const void *r, void *cur, int on_device) {
    LSA_TRACE_CALL("fr_fold", half);
    int rc = require_ready();
    if (rc) return rc;
    if (half == 0) return LSA_OK;
    if (!old || !cur || !r) { set_error("fr_fold: null argument"); return LSA_ERR_INVALID; }
    DevBuf d_v, d_rr;
    OperandFrame f("fr_fold", on_device);
    const Fr *d_old = f.in<Fr>(d_v, old, 2 * half * sizeof(Fr));
    const Fr *d_r = f.in<Fr>(d_rr, r, sizeof(Fr));
    Fr *d_cur = f.out_in<Fr>(d_old, cur, half * sizeof(Fr));          // (host callers: in place in the staged copy)
    if (f.rc()) return f.rc();
    rc = fr_fold_halves_device(d_old, half, d_r, d_cur, g.stream);
    if (rc) return rc;
    if (!on_device) HIPCHK(hipStreamSynchronize(g.stream));
    return f.download();
}

// ---------------------------------------------------------------- element-wise vector algebra (fr_elem.hip)
int lsa_fr_vec_mul(const void *a, const void *b, const void *scale, size_t n, void *out, int on_device) {
    LSA_TRACE_CALL("fr_vec_mul", n);
    int rc = require_ready();
    if (rc) return rc;
    if (n == 0) return LSA_OK;
    size_t bytes;
    const void *ins[2] = {a, b};
    rc = vec_args("fr_vec_mul", ins, 2, out, n, n, true, on_device, &bytes);
    if (rc) return rc;
    Fr s;
    if (scale) s = load_fr(scale);
    const Fr c266 = fr_elem_c266(scale ? &s : nullptr);
    OperandFrame f("fr_vec_mul", on_device);
    const Fr *d_a = f.in<Fr>(g_stage_el_x[0], a, bytes);
    const Fr *d_b = (a == b) ? d_a : f.in<Fr>(g_stage_el_x[1], b, bytes);
    Fr *d_out = f.out<Fr>(g_stage_el_out, out, bytes);
    if (f.rc()) return f.rc();
    rc = fr_vec_mul_device(d_a, d_b, c266, n, d_out, g.stream);
    if (rc) return rc;
    return f.download();
}

int lsa_fr_vec_lincomb(const void *const *xs, const void *coeffs, size_t k, size_t n, void *out, int on_device) {
    LSA_TRACE_CALL("fr_vec_lincomb", n);
    int rc = require_ready();
    if (rc) return rc;
    if (k == 0 || k > FR_VEC_LINCOMB_MAX) { set_error("fr_vec_lincomb: k = %zu not in 1..%u", k, FR_VEC_LINCOMB_MAX); return LSA_ERR_INVALID; }
    if (n == 0) return LSA_OK;
    if (!xs || !coeffs) { set_error("fr_vec_lincomb: null argument"); return LSA_ERR_INVALID; }
    size_t bytes;
    rc = vec_args("fr_vec_lincomb", xs, k, out, n, n, true, on_device, &bytes);
    if (rc) return rc;
    Fr c261[FR_VEC_LINCOMB_MAX];
    for (size_t t = 0; t < k; t++) c261[t] = fr_elem_c261(load_fr((const char *)coeffs + t * sizeof(Fr)));
    OperandFrame f("fr_vec_lincomb", on_device);
    const Fr *d_xs[FR_VEC_LINCOMB_MAX];
    for (size_t t = 0; t < k; t++) {
        size_t same = t;                                   // a vector given twice is staged once
        for (size_t u = 0; u < t; u++) if (xs[u] == xs[t]) { same = u; break; }
        d_xs[t] = same < t ? d_xs[same] : f.in<Fr>(g_stage_el_x[t], xs[t], bytes);
    }
    Fr *d_out = f.out<Fr>(g_stage_el_out, out, bytes);
    if (f.rc()) return f.rc();
    rc = fr_vec_lincomb_device(d_xs, c261, k, n, d_out, g.stream);
    if (rc) return rc;
    return f.download();
}

int lsa_fr_powers(const void *base, const void *first, size_t n, void *out, int on_device) {
    LSA_TRACE_CALL("fr_powers", n);
    int rc = require_ready();
    if (rc) return rc;
    if (n == 0) return LSA_OK;
    if (!base) { set_error("fr_powers: null argument"); return LSA_ERR_INVALID; }
    size_t bytes;
    rc = vec_args("fr_powers", nullptr, 0, out, n, n, false, on_device, &bytes);
    if (rc) return rc;
    const Fr base261 = fr_elem_c261(load_fr(base)), f0 = first ? fr_elem_canon(load_fr(first)) : Fr::one();
    OperandFrame f("fr_powers", on_device);
    Fr *d_out = f.out<Fr>(g_stage_el_out, out, bytes);
    if (f.rc()) return f.rc();
    rc = fr_powers_device(base261, f0, n, d_out, g.stream);
    if (rc) return rc;
    return f.download();
}

int lsa_fr_batch_inverse(const void *x, size_t n, void *out, uint64_t *n_zero, int on_device) {
    LSA_TRACE_CALL("fr_batch_inverse", n);
    int rc = require_ready();
    if (rc) return rc;
    if (n == 0) { if (n_zero) *n_zero = 0; return LSA_OK; }
    size_t bytes;
    rc = vec_args("fr_batch_inverse", &x, 1, out, n, n, true, on_device, &bytes);
    if (rc) return rc;
    OperandFrame f("fr_batch_inverse", on_device);
    unsigned long long *d_zeros = f.scratch<unsigned long long>(g_stage_el_count, sizeof(unsigned long long));
    const Fr *d_x = f.in<Fr>(g_stage_el_x[0], x, bytes);
    Fr *d_out = f.out<Fr>(g_stage_el_out, out, bytes);
    if (f.rc()) return f.rc();
    rc = fr_batch_inverse_device(d_x, n, d_out, d_zeros, g.stream);
    if (rc) return rc;
    rc = f.download();
    if (rc) return rc;
    if (n_zero) LSA_DOWNLOAD(n_zero, d_zeros, sizeof(uint64_t));       // (blocking, behind the kernel: device callers too)
    return LSA_OK;
}

int lsa_fr_poly_eval(const void *coeffs, size_t n, const void *x, void *out, int on_device) {
    LSA_TRACE_CALL("fr_poly_eval", n);
    int rc = require_ready();
    if (rc) return rc;
    if (!out || !x) { set_error("fr_poly_eval: null argument"); return LSA_ERR_INVALID; }
    if (on_device && misaligned(out)) { set_error("fr_poly_eval: device pointers must be 16-byte aligned"); return LSA_ERR_INVALID; }
    if (n == 0) {                                          // the empty sum
        if (on_device) HIPCHK(hipMemsetAsync(out, 0, sizeof(Fr), g.stream));
        else memset(out, 0, sizeof(Fr));
        return LSA_OK;
    }
    size_t bytes;
    rc = vec_args("fr_poly_eval", &coeffs, 1, out, 1, n, false, on_device, &bytes);
    if (rc) return rc;
    const Fr xc = fr_elem_canon(load_fr(x));
    OperandFrame f("fr_poly_eval", on_device);
    Fr *d_partial = f.scratch<Fr>(g_stage_el_partial, fr_poly_eval_partials(n) * sizeof(Fr));
    const Fr *d_c = f.in<Fr>(g_stage_el_x[0], coeffs, bytes);
    Fr *d_out = f.out<Fr>(g_stage_el_out, out, sizeof(Fr));
    if (f.rc()) return f.rc();
    rc = fr_poly_eval_device(d_c, n, xc, d_partial, d_out, g.stream);
    if (rc) return rc;
    return f.download();
}

size_t lsa_fr_vec_param(int which) {
    switch (which) {
    case LSA_FR_VEC_PARAM_LINCOMB_MAX: return FR_VEC_LINCOMB_MAX;
    case LSA_FR_VEC_PARAM_INV_RUN: return FR_ELEM_INV_RUN;
    case LSA_FR_VEC_PARAM_POWERS_RUN: return FR_ELEM_POWERS_RUN;
    case LSA_FR_VEC_PARAM_EVAL_ITEMS: return FR_ELEM_EVAL_ITEMS;
    case LSA_FR_VEC_PARAM_PASS_ELEMS: return g.ready ? fr_elem_pass_elems() : 0;
    case LSA_FR_VEC_PARAM_EVAL_BLOCK: return fr_poly_eval_block_items();
    default: return 0;
    }
}
}  // extern "C"
