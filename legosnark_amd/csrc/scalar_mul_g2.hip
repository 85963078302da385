// legosnark_amd/csrc/scalar_mul_g2.hip -- variable-base batch scalar multiplication on the twist (G2) and the
// column-sparse "matrix in the exponent" product built on it: the G2 twins of scalar_mul.hip.
//
// Every commitment of the reference is a pair Comm{c in G1, kc in G2}, and every operation on commitments runs on both
// halves: out[i] = k_i * P_i on distinct G2 bases, and out[j] = sum over the non-zeros e of column j of k[row(e)] * M[e].
//
//   k_smul_g2     a lane PAIR per (point, scalar) item, persistent grid-stride loop: the even lane carries the c0
//                 components, the odd lane the c1 components of every Fq2 value (fp29x2l.h, F29h), both run smul_g2<F29h>
//                 (smul_g2.h): signed 4-bit digits over the whole 254-bit scalar, NO endomorphism (the result is the
//                 integer multiple for every point of the twist, in or out of the order-r subgroup); a table {1..8}*P in
//                 XYZZ coordinates in a global-memory slot per lane (8 x 144 B = 1152 B, contiguous, as in k_smul_g1);
//                 63 x 4 doublings + at most 64 complete XYZZ additions.  Predicates are uniform over a pair, and a pair
//                 shares its item index, so the two lanes of a pair always leave the loop together.
//   k_col_sum_g2  a lane pair per column: complete XYZZ additions over the column's segment; an empty column: infinity.
// Results are group elements in libff's Jacobian layout; they agree with the reference after affine normalisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "curves.h"
#include "fp29x2l.h"
#include "smul_g2.h"
#include "msm.h"

namespace lsa {

static constexpr unsigned SMUL_G2_LANES = 2;     // lanes per item: one Fq2 component each
static constexpr unsigned SMUL_G2_BLOCKS = 512;  // persistent grid: 2 blocks (8 waves) per CU

// (XYZZ29h, g2h_from_jac, g2h_store_jac: fp29x2l.h, shared with ecntt.hip)

__global__ __launch_bounds__(256) void k_smul_g2(const AffPackedG2 *__restrict__ pts, const Fr *__restrict__ scalars,
                                                 const uint32_t *__restrict__ sidx, size_t n, XYZZ29h *__restrict__ tbl,
                                                 Jac<Fq2> *__restrict__ out) {
    const size_t lane = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * (256 / SMUL_G2_LANES);
    const unsigned part = threadIdx.x & 1u;
    XYZZ29h *T = tbl + lane * SMUL_G2_TBL;
    for (size_t i = lane / SMUL_G2_LANES; i < n; i += stride) {        // (i is the pair's: both lanes stay or leave)
        const AffE<F29h> P = unpack_affine_half(pts[i], part);
        uint32_t s[8];
        scalars[sidx ? sidx[i] : i].to_canonical(s);
        g2h_store_jac(smul_g2(P, s, T), part, &out[i]);
    }
}

// out[j] = sum of items[col_ptr[j] .. col_ptr[j+1])
__global__ __launch_bounds__(256) void k_col_sum_g2(const Jac<Fq2> *__restrict__ items, const uint64_t *__restrict__ col_ptr, size_t ncols,
                                                    Jac<Fq2> *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, j = t / SMUL_G2_LANES;
    const unsigned part = threadIdx.x & 1u;
    if (j >= ncols) return;                                            // (both lanes of a pair leave together)
    XYZZ29h acc = XYZZ29h::inf();
#pragma unroll 1
    for (uint64_t e = col_ptr[j]; e < col_ptr[j + 1]; e++) acc = g2_add(acc, g2h_from_jac(items[e], part));
    g2h_store_jac(acc, part, &out[j]);
}

// d_out[i] = d_scalars[d_sidx ? d_sidx[i] : i] * d_pts[i]; d_pts: libff Jacobian, device.
// Synchronises the stream before returning (temporary buffers are freed).
int g2_scalar_mul_device(const Jac<Fq2> *d_pts, const Fr *d_scalars, const uint32_t *d_sidx, size_t n, Jac<Fq2> *d_out, hipStream_t st) {
    if (n == 0) return LSA_OK;
    constexpr size_t PER_BLOCK = 256 / SMUL_G2_LANES;
    const unsigned blocks = (unsigned)((n + PER_BLOCK - 1) / PER_BLOCK < SMUL_G2_BLOCKS ? (n + PER_BLOCK - 1) / PER_BLOCK : SMUL_G2_BLOCKS);
    AffPackedG2 *d_aff = nullptr;
    XYZZ29h *d_tbl = nullptr;
    if (hipMalloc(&d_aff, n * sizeof(AffPackedG2)) != hipSuccess ||
        hipMalloc(&d_tbl, (size_t)blocks * 256 * SMUL_G2_TBL * sizeof(XYZZ29h)) != hipSuccess) {
        if (d_aff) (void)hipFree(d_aff);
        set_error("g2 scalar_mul: workspace allocation failed");
        return LSA_ERR_NOMEM;
    }
    int rc = prepare_bases<Fq2>(d_pts, d_aff, n, st);
    if (!rc) hipLaunchKernelGGL(k_smul_g2, dim3(blocks), dim3(256), 0, st, d_aff, d_scalars, d_sidx, n, d_tbl, d_out);
    hipError_t e = hipStreamSynchronize(st);
    (void)hipFree(d_aff);
    (void)hipFree(d_tbl);
    if (rc) return rc;
    if (e != hipSuccess) { set_error("g2 scalar_mul: %s", hipGetErrorString(e)); return LSA_ERR_HIP; }
    return LSA_OK;
}

int g2_column_sums_device(const Jac<Fq2> *d_items, const uint64_t *d_col_ptr, size_t ncols, Jac<Fq2> *d_out, hipStream_t st) {
    if (ncols == 0) return LSA_OK;
    const size_t lanes = ncols * SMUL_G2_LANES;
    hipLaunchKernelGGL(k_col_sum_g2, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, d_items, d_col_ptr, ncols, d_out);
    HIPCHK(hipGetLastError());
    return LSA_OK;
}

// lsa_smul_param: 0 = window width in bits, 1 = items resident in one pass of the persistent grid, 2 = lanes per item
size_t g2_smul_param(int which) {
    return which == 0 ? (size_t)SMUL_G2_WINDOW : which == 1 ? (size_t)SMUL_G2_BLOCKS * (256 / SMUL_G2_LANES) : which == 2 ? (size_t)SMUL_G2_LANES : 0;
}

}  // namespace lsa
