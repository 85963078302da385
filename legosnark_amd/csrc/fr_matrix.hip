// legosnark_amd/csrc/fr_matrix.hip -- an Fr vector as a row-major matrix: the product C = A B (lsa_fr_matmul) and the weighted
// sums of rows / of columns (lsa_fr_matvec), for the matrix-product gadget CPMat / CPmmp of the reference.
//
// Replaces the schoolbook triple loop of src/examples/matrixsc.cc:83-91 (the witness C) and the contraction in DPMatrixMle's
// constructor, src/prototools/mle.h:241-258 (v[r] = sum_l A[(l << d) + r] eqTbl[l]: lsa_fr_matvec side 0 with w = the table of
// lsa_fr_eq_table(rho, d, 0)).  The rest of CPSumcheckMatrix::prove is fr_vec.hip's.
//
// Every output is one dot product on fr29.h's limbs, fr_dot.h: four schoolbook products per Montgomery reduction, the reduced
// partials summed lazily, one closing product, canonical words out -- the bytes of the reference's loops.
//
// k_fr_matmul     a workgroup of 256 lanes owns a 32 x 32 tile of C, a lane a 2 x 2 register tile of it (rows ty, ty + 16; columns
//                 tx, tx + 16).  Per K-step of 16 the 32 x 16 tile of A and the 16 x 32 tile of B are turned into limbs ONCE and
//                 kept in LDS limb-major (37 KiB), so a wavefront's reads of B are 16 consecutive words and its reads of A four
//                 broadcasts; the next step's words are already in flight while this one is multiplied.  Edges are predicated: an
//                 element outside A or B enters LDS as zero, an output outside C is not stored.
// k_fr_matvec_cols  side 0: a lane owns a column, a workgroup 256 of them and a slice of the rows; a wavefront's loads of a row
//                 are 2 KiB contiguous, w[r] is the same for every lane (limbs read through the scalar cache).
// k_fr_matvec_rows  side 1: a wavefront owns a row (four rows per workgroup) and a slice of the columns, its lanes 64 apart along
//                 the row; the 64 lane sums meet in LDS.
// Both read M once and w from a limb-major copy (k_fr_to_limbs); when the outputs alone give fewer workgroups than the chip
// needs, the summed dimension is cut into slices (matvec_plan) whose canonical partial sums k_fr_matvec_finish adds up.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "capi_internal.h"
#include "fr29.h"
#include "fr_dot.h"

namespace lsa {

typedef uint32_t mat_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ Fr fr_words(const mat_u32x4 &lo, const mat_u32x4 &hi) {
    Fr x;
    x.l[0] = lo.x; x.l[1] = lo.y; x.l[2] = lo.z; x.l[3] = lo.w; x.l[4] = hi.x; x.l[5] = hi.y; x.l[6] = hi.z; x.l[7] = hi.w;
    return x;
}
__device__ __forceinline__ Fr fr_load(const Fr *p) {
    const mat_u32x4 *q = reinterpret_cast<const mat_u32x4 *>(p);
    return fr_words(q[0], q[1]);
}
// (M is touched once: non-temporal, as fr_vec.hip's stream kernels)
__device__ __forceinline__ Fr fr_load_once(const Fr *p) {
    const mat_u32x4 *q = reinterpret_cast<const mat_u32x4 *>(p);
    return fr_words(__builtin_nontemporal_load(q), __builtin_nontemporal_load(q + 1));
}
__device__ __forceinline__ void fr_store(Fr *p, const Fr &x) {
    mat_u32x4 lo, hi;
    lo.x = x.l[0]; lo.y = x.l[1]; lo.z = x.l[2]; lo.w = x.l[3]; hi.x = x.l[4]; hi.y = x.l[5]; hi.z = x.l[6]; hi.w = x.l[7];
    reinterpret_cast<mat_u32x4 *>(p)[0] = lo;
    reinterpret_cast<mat_u32x4 *>(p)[1] = hi;
}

// ---------------------------------------------------------------- C = A B
constexpr unsigned MM_TILE = 32;        // edge of a workgroup's tile of C
constexpr unsigned MM_KSTEP = 16;       // elements of the summed dimension staged per step: four reductions per output and step
constexpr unsigned MM_LANES = 16;       // lanes along either edge; each owns outputs MM_LANES apart: 2 x 2 per lane
constexpr unsigned MM_REG = MM_TILE / MM_LANES;
constexpr unsigned MM_PER_LANE = MM_TILE * MM_KSTEP / 256;      // elements of either staged tile a lane loads
static_assert(MM_KSTEP % FR_DOT_GROUP == 0 && MM_LANES * MM_LANES == 256 && MM_PER_LANE * 256 == MM_TILE * MM_KSTEP, "tile shape");

// d += sum_{g <= k < g + 4} a[row][k] b[k][col] from the staged limbs: one reduction
__device__ __forceinline__ void mm_group(FrDot &d, const uint32_t (&s_a)[9][MM_TILE][MM_KSTEP + 1], const uint32_t (&s_b)[9][MM_KSTEP][MM_TILE], unsigned row,
                                         unsigned col, unsigned g) {
    Fr29 a[FR_DOT_GROUP], b[FR_DOT_GROUP];
#pragma unroll
    for (unsigned k = 0; k < FR_DOT_GROUP; k++)
#pragma unroll
        for (int l = 0; l < 9; l++) {
            a[k].l[l] = s_a[l][row][g + k];
            b[k].l[l] = s_b[l][g + k][col];
        }
    fr_dot_group(d, a, b, FR_DOT_GROUP);
}

__global__ __launch_bounds__(256) void k_fr_matmul(const Fr *__restrict__ A, const Fr *__restrict__ B, size_t rows_a, size_t inner, size_t cols_b,
                                                   size_t tiles_x, size_t tiles, Fr *__restrict__ C) {
    // limb-major: s_a[limb][row][k] (a row padded by one word: the lanes that write a column of k are 17 words apart),
    // s_b[limb][k][column]
    __shared__ uint32_t s_a[9][MM_TILE][MM_KSTEP + 1];
    __shared__ uint32_t s_b[9][MM_KSTEP][MM_TILE];
    const unsigned t = threadIdx.x, tx = t % MM_LANES, ty = t / MM_LANES;
    const Fr zero = Fr::zero();
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t row0 = (tile / tiles_x) * MM_TILE, col0 = (tile % tiles_x) * MM_TILE;
        FrDot acc[MM_REG][MM_REG];
#pragma unroll
        for (unsigned i = 0; i < MM_REG; i++)
#pragma unroll
            for (unsigned j = 0; j < MM_REG; j++) acc[i][j] = fr_dot_zero();
        // this lane's elements of the staged tiles: A (row e / KSTEP, k e % KSTEP), B (k e / TILE, column e % TILE), e = t + 256 q
        Fr ra[MM_PER_LANE], rb[MM_PER_LANE];
        auto fetch = [&](size_t k0) {
#pragma unroll
            for (unsigned q = 0; q < MM_PER_LANE; q++) {
                const unsigned e = t + 256 * q;
                const size_t ar = row0 + e / MM_KSTEP, ak = k0 + e % MM_KSTEP, bk = k0 + e / MM_TILE, bc = col0 + e % MM_TILE;
                ra[q] = (ar < rows_a && ak < inner) ? fr_load(A + ar * inner + ak) : zero;
                rb[q] = (bk < inner && bc < cols_b) ? fr_load(B + bk * cols_b + bc) : zero;
            }
        };
        if (inner) fetch(0);
        for (size_t k0 = 0; k0 < inner; k0 += MM_KSTEP) {
#pragma unroll
            for (unsigned q = 0; q < MM_PER_LANE; q++) {
                const unsigned e = t + 256 * q;
                const Fr29 la = Fr29::from_words(ra[q]), lb = Fr29::from_words(rb[q]);
#pragma unroll
                for (int l = 0; l < 9; l++) {
                    s_a[l][e / MM_KSTEP][e % MM_KSTEP] = la.l[l];
                    s_b[l][e / MM_TILE][e % MM_TILE] = lb.l[l];
                }
            }
            __syncthreads();
            if (k0 + MM_KSTEP < inner) fetch(k0 + MM_KSTEP);          // in flight under the products below
#pragma unroll 1
            for (unsigned g = 0; g < MM_KSTEP; g += FR_DOT_GROUP) {
                static_assert(MM_REG == 2, "the four outputs of a lane are written out");
                mm_group(acc[0][0], s_a, s_b, ty, tx, g);
                mm_group(acc[0][1], s_a, s_b, ty, tx + MM_LANES, g);
                mm_group(acc[1][0], s_a, s_b, ty + MM_LANES, tx, g);
                mm_group(acc[1][1], s_a, s_b, ty + MM_LANES, tx + MM_LANES, g);
            }
            __syncthreads();
        }
#pragma unroll
        for (unsigned i = 0; i < MM_REG; i++)
#pragma unroll
            for (unsigned j = 0; j < MM_REG; j++) {
                const size_t r = row0 + ty + MM_LANES * i, c = col0 + tx + MM_LANES * j;
                if (r < rows_a && c < cols_b) fr_store(C + r * cols_b + c, fr_dot_finish(acc[i][j]));
            }
    }
}

// ---------------------------------------------------------------- weighted sums of rows and of columns
// wl[l * n + i] = limb l of w[i]
__global__ __launch_bounds__(256) void k_fr_to_limbs(const Fr *__restrict__ w, size_t n, uint32_t *__restrict__ wl) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Fr29 x = Fr29::from_words(fr_load(w + i));
#pragma unroll
    for (int l = 0; l < 9; l++) wl[(size_t)l * n + i] = x.l[l];
}
__device__ __forceinline__ Fr29 limbs_at(const uint32_t *__restrict__ wl, size_t n, size_t i) {
    Fr29 x;
#pragma unroll
    for (int l = 0; l < 9; l++) x.l[l] = wl[(size_t)l * n + i];
    return x;
}

constexpr unsigned MV_COLS_PER_BLOCK = 256;      // side 0: a column per lane
constexpr unsigned MV_ROWS_PER_BLOCK = 4;        // side 1: a row per wavefront

// side 0.  part[s * cols + c] = sum over the rows r of slice s (chunk rows each) of w[r] M[r][c]; grid (column blocks, slices)
__global__ __launch_bounds__(256) void k_fr_matvec_cols(const Fr *__restrict__ M, size_t rows, size_t cols, const uint32_t *__restrict__ wl, size_t chunk,
                                                        Fr *__restrict__ part) {
    const size_t r_lo = (size_t)blockIdx.y * chunk, r_hi = r_lo + chunk < rows ? r_lo + chunk : rows;
    const Fr zero = Fr::zero();
    for (size_t c0 = (size_t)blockIdx.x * MV_COLS_PER_BLOCK; c0 < cols; c0 += (size_t)gridDim.x * MV_COLS_PER_BLOCK) {
        const size_t c = c0 + threadIdx.x, cc = c < cols ? c : cols - 1;     // lanes past the edge redo the last column: no divergence
        const Fr *in = M + cc;
        FrDot d = fr_dot_zero();
        size_t r = r_lo;
#pragma unroll 1
        for (; r + FR_DOT_GROUP <= r_hi; r += FR_DOT_GROUP) {            // whole groups: four loads in flight, no guards
            Fr x[FR_DOT_GROUP];
#pragma unroll
            for (unsigned j = 0; j < FR_DOT_GROUP; j++) x[j] = fr_load_once(in + (r + j) * cols);
            Fr29 m[FR_DOT_GROUP], w[FR_DOT_GROUP];
#pragma unroll
            for (unsigned j = 0; j < FR_DOT_GROUP; j++) {
                m[j] = Fr29::from_words(x[j]);
                w[j] = limbs_at(wl, rows, r + j);
            }
            fr_dot_group(d, m, w, FR_DOT_GROUP);
        }
        if (r < r_hi) {                                                   // the last one to three rows
            Fr29 m[FR_DOT_GROUP], w[FR_DOT_GROUP];
#pragma unroll
            for (unsigned j = 0; j < FR_DOT_GROUP; j++) {
                const bool in_range = r + j < r_hi;
                m[j] = Fr29::from_words(in_range ? fr_load_once(in + (r + j) * cols) : zero);
                w[j] = limbs_at(wl, rows, in_range ? r + j : r);          // (a zero operand: which weight it meets does not matter)
            }
            fr_dot_group(d, m, w, FR_DOT_GROUP);
        }
        if (c < cols) fr_store(part + (size_t)blockIdx.y * cols + c, fr_dot_finish(d));
    }
}

// side 1.  part[s * rows + r] = sum over the columns c of slice s (chunk columns each) of M[r][c] w[c]; grid (row blocks, slices)
__global__ __launch_bounds__(256) void k_fr_matvec_rows(const Fr *__restrict__ M, size_t rows, size_t cols, const uint32_t *__restrict__ wl, size_t chunk,
                                                        Fr *__restrict__ part) {
    __shared__ Fr s_red[256];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t c_lo = (size_t)blockIdx.y * chunk, c_hi = c_lo + chunk < cols ? c_lo + chunk : cols;
    const Fr zero = Fr::zero();
    for (size_t r0 = (size_t)blockIdx.x * MV_ROWS_PER_BLOCK; r0 < rows; r0 += (size_t)gridDim.x * MV_ROWS_PER_BLOCK) {
        const size_t r = r0 + wave, rr = r < rows ? r : rows - 1;
        const Fr *in = M + rr * cols;
        FrDot d = fr_dot_zero();
#pragma unroll 1
        for (size_t c = c_lo + lane; c < c_hi; c += 64 * FR_DOT_GROUP) {
            Fr x[FR_DOT_GROUP];
#pragma unroll
            for (unsigned j = 0; j < FR_DOT_GROUP; j++) x[j] = c + 64 * j < c_hi ? fr_load_once(in + c + 64 * j) : zero;
            Fr29 m[FR_DOT_GROUP], w[FR_DOT_GROUP];
#pragma unroll
            for (unsigned j = 0; j < FR_DOT_GROUP; j++) {
                m[j] = Fr29::from_words(x[j]);
                w[j] = limbs_at(wl, cols, c + 64 * j < c_hi ? c + 64 * j : c);        // (a zero operand: which weight it meets does not matter)
            }
            fr_dot_group(d, m, w, FR_DOT_GROUP);
        }
        s_red[threadIdx.x] = fr_dot_finish(d);
        __syncthreads();
        for (unsigned s = 32; s >= 1; s >>= 1) {
            if (lane < s) s_red[threadIdx.x] = s_red[threadIdx.x] + s_red[threadIdx.x + s];
            __syncthreads();
        }
        if (lane == 0 && r < rows) fr_store(part + (size_t)blockIdx.y * rows + r, s_red[threadIdx.x]);
        __syncthreads();
    }
}

// out[i] = sum_{s < slices} part[s * n + i]
__global__ __launch_bounds__(256) void k_fr_matvec_finish(const Fr *__restrict__ part, size_t slices, size_t n, Fr *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Fr acc = fr_load(part + i);
    for (size_t s = 1; s < slices; s++) acc = acc + fr_load(part + s * n + i);
    fr_store(out + i, acc);
}

// ---------------------------------------------------------------- host side
namespace {
// How lsa_fr_matvec cuts its work.  blocks: workgroups along the outputs; slices: parts of the summed dimension (1: the
// kernel writes `out` itself, no finishing kernel); chunk: summed elements per slice.
//   a matrix of at most MV_SMALL elements: ONE workgroup walks all outputs;
//   outputs that give MV_FILL_BLOCKS workgroups or more, or fewer than MV_SPLIT_MIN_SUM summed elements: no slices;
//   else about 2 * MV_FILL_BLOCKS workgroups in all, a slice never shorter than MV_CHUNK_MIN[side].
constexpr size_t MV_SMALL = 4096, MV_SPLIT_MIN_SUM = 256, MV_FILL_BLOCKS = 512, MV_MAX_BLOCKS = 65535;
constexpr size_t MV_CHUNK_MIN[2] = {64, 256};
struct MatvecPlan { size_t blocks, slices, chunk; };
MatvecPlan matvec_plan(size_t rows, size_t cols, int side) {
    const size_t nout = side ? rows : cols, nsum = side ? cols : rows, per = side ? MV_ROWS_PER_BLOCK : MV_COLS_PER_BLOCK;
    MatvecPlan p;
    p.blocks = (nout + per - 1) / per;
    p.slices = 1;
    p.chunk = nsum;
    if (nout == 0) return p;
    if (nsum == 0 || rows <= MV_SMALL / cols) {          // (rows * cols <= MV_SMALL, without the product)
        if (nsum) p.blocks = 1;
        return p;
    }
    if (p.blocks < MV_FILL_BLOCKS && nsum >= MV_SPLIT_MIN_SUM) {
        size_t want = (2 * MV_FILL_BLOCKS + p.blocks - 1) / p.blocks;
        const size_t most = nsum / MV_CHUNK_MIN[side];
        if (want > most) want = most;
        if (want > 1) {
            const size_t unit = side ? 64 * FR_DOT_GROUP : FR_DOT_GROUP;        // whole groups of four per lane in every slice but the last
            p.chunk = ((nsum + want - 1) / want + unit - 1) / unit * unit;
            p.slices = (nsum + p.chunk - 1) / p.chunk;
        }
    }
    if (p.blocks > MV_MAX_BLOCKS) p.blocks = MV_MAX_BLOCKS;                     // (the kernels stride over the rest)
    return p;
}

// grow-only staging (released by lsa_shutdown): the limbs of w, the slices' partial sums, and for host callers the three operands
StageBuf g_mat_limbs, g_mat_part, g_mat_a, g_mat_b, g_mat_c;
}  // namespace

// All device pointers, 16-byte aligned.  d_limbs: 9 * (side ? cols : rows) words; d_part: slices * outputs elements when the plan
// has slices.  Asynchronous on st.
static int fr_matvec_device(const Fr *d_m, size_t rows, size_t cols, const Fr *d_w, int side, Fr *d_out, uint32_t *d_limbs, Fr *d_part,
                            const MatvecPlan &p, hipStream_t st) {
    const size_t nout = side ? rows : cols, nsum = side ? cols : rows;
    if (nsum) hipLaunchKernelGGL(k_fr_to_limbs, dim3((unsigned)((nsum + 255) / 256)), dim3(256), 0, st, d_w, nsum, d_limbs);
    Fr *dst = p.slices > 1 ? d_part : d_out;
    const dim3 grid((unsigned)p.blocks, (unsigned)p.slices);
    if (side) hipLaunchKernelGGL(k_fr_matvec_rows, grid, dim3(256), 0, st, d_m, rows, cols, (const uint32_t *)d_limbs, p.chunk, dst);
    else hipLaunchKernelGGL(k_fr_matvec_cols, grid, dim3(256), 0, st, d_m, rows, cols, (const uint32_t *)d_limbs, p.chunk, dst);
    if (p.slices > 1) hipLaunchKernelGGL(k_fr_matvec_finish, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, (const Fr *)d_part, p.slices, nout, d_out);
    HIPCHK(hipGetLastError());
    return LSA_OK;
}

static int fr_matmul_device(const Fr *d_a, const Fr *d_b, size_t rows_a, size_t inner, size_t cols_b, Fr *d_c, hipStream_t st) {
    const size_t tiles_x = (cols_b + MM_TILE - 1) / MM_TILE, tiles = tiles_x * ((rows_a + MM_TILE - 1) / MM_TILE);
    const size_t grid = tiles < ((size_t)1 << 20) ? tiles : (size_t)1 << 20;       // (the kernel strides over the rest)
    hipLaunchKernelGGL(k_fr_matmul, dim3((unsigned)grid), dim3(256), 0, st, d_a, d_b, rows_a, inner, cols_b, tiles_x, tiles, d_c);
    HIPCHK(hipGetLastError());
    return LSA_OK;
}

}  // namespace lsa

using namespace lsa;

extern "C" {
size_t lsa_fr_matrix_param(int which) {
    switch (which) {
    case LSA_FR_PARAM_MATMUL_TILE: return MM_TILE;
    case LSA_FR_PARAM_MATMUL_KSTEP: return MM_KSTEP;
    case LSA_FR_PARAM_DOT_MAX_PARTIALS: return FR_DOT_MAX_PARTIALS;
    case LSA_FR_PARAM_DOT_GROUP: return FR_DOT_GROUP;
    case LSA_FR_PARAM_MATVEC_SMALL: return MV_SMALL;
    default: return 0;
    }
}

size_t lsa_fr_matvec_slices(size_t rows, size_t cols, int side) {
    size_t bytes;
    if ((side != 0 && side != 1) || !fr_bytes_of(rows, cols, &bytes)) return 0;
    return matvec_plan(rows, cols, side).slices;
}

int lsa_fr_matvec(const void *m, size_t rows, size_t cols, const void *w, int side, void *out, int on_device) {
    LSA_TRACE_CALL("fr_matvec", rows < cols ? cols : rows);
    int rc = require_ready();
    if (rc) return rc;
    if (side != 0 && side != 1) { set_error("fr_matvec: side %d (0: out[c] = sum_r w[r] M[r][c], 1: out[r] = sum_c M[r][c] w[c])", side); return LSA_ERR_INVALID; }
    size_t m_bytes;
    if (!fr_bytes_of(rows, cols, &m_bytes)) { set_error("fr_matvec: %zu x %zu elements of 32 bytes overflow size_t", rows, cols); return LSA_ERR_INVALID; }
    const size_t nout = side ? rows : cols, nsum = side ? cols : rows, out_bytes = nout * sizeof(Fr), w_bytes = nsum * sizeof(Fr);
    if (nout == 0) return LSA_OK;
    if (!out || (m_bytes && !m) || (w_bytes && !w)) { set_error("fr_matvec: null argument"); return LSA_ERR_INVALID; }
    if (overlap(out, out_bytes, m, m_bytes) || overlap(out, out_bytes, w, w_bytes)) { set_error("fr_matvec: out overlaps an input"); return LSA_ERR_INVALID; }
    if (on_device && (misaligned(m) || misaligned(w) || misaligned(out))) { set_error("fr_matvec: device pointers must be 16-byte aligned"); return LSA_ERR_INVALID; }
    const MatvecPlan p = matvec_plan(rows, cols, side);
    size_t part_bytes = 0;
    if (p.slices > 1 && !fr_bytes_of(p.slices, nout, &part_bytes)) { set_error("fr_matvec: %zu x %zu partial sums overflow size_t", p.slices, nout); return LSA_ERR_INVALID; }
    size_t limb_bytes;
    if (__builtin_mul_overflow(nsum, 9 * sizeof(uint32_t), &limb_bytes)) { set_error("fr_matvec: the limbs of %zu weights overflow size_t", nsum); return LSA_ERR_INVALID; }
    OperandFrame f("fr_matvec", on_device);
    uint32_t *d_limbs = f.scratch<uint32_t>(g_mat_limbs, limb_bytes);
    Fr *d_part = f.scratch<Fr>(g_mat_part, part_bytes);
    const Fr *d_m = f.in<Fr>(g_mat_a, m, m_bytes);
    const Fr *d_w = f.in<Fr>(g_mat_b, w, w_bytes);
    Fr *d_out = f.out<Fr>(g_mat_c, out, out_bytes);
    if (f.rc()) return f.rc();
    rc = fr_matvec_device(d_m, rows, cols, d_w, side, d_out, d_limbs, d_part, p, g.stream);
    if (rc) return rc;
    return f.download();
}

int lsa_fr_matmul(const void *a, const void *b, size_t rows_a, size_t inner, size_t cols_b, void *c, int on_device) {
    LSA_TRACE_CALL("fr_matmul", rows_a < cols_b ? cols_b : rows_a);
    int rc = require_ready();
    if (rc) return rc;
    size_t a_bytes, b_bytes, c_bytes;
    if (!fr_bytes_of(rows_a, inner, &a_bytes) || !fr_bytes_of(inner, cols_b, &b_bytes) || !fr_bytes_of(rows_a, cols_b, &c_bytes)) {
        set_error("fr_matmul: (%zu x %zu) (%zu x %zu) elements of 32 bytes overflow size_t", rows_a, inner, inner, cols_b);
        return LSA_ERR_INVALID;
    }
    if (c_bytes == 0) return LSA_OK;
    if (!c || (a_bytes && (!a || !b))) { set_error("fr_matmul: null argument"); return LSA_ERR_INVALID; }
    if (overlap(c, c_bytes, a, a_bytes) || overlap(c, c_bytes, b, b_bytes)) { set_error("fr_matmul: c overlaps an input"); return LSA_ERR_INVALID; }
    if (on_device && (misaligned(a) || misaligned(b) || misaligned(c))) { set_error("fr_matmul: device pointers must be 16-byte aligned"); return LSA_ERR_INVALID; }
    OperandFrame f("fr_matmul", on_device);
    const Fr *d_a = f.in<Fr>(g_mat_a, a, a_bytes);           // (inner == 0: both inputs are empty and may be null)
    const Fr *d_b = f.in<Fr>(g_mat_b, b, b_bytes);
    Fr *d_c = f.out<Fr>(g_mat_c, c, c_bytes);
    if (f.rc()) return f.rc();
    rc = fr_matmul_device(d_a, d_b, rows_a, inner, cols_b, d_c, g.stream);
    if (rc) return rc;
    return f.download();
}
}  // extern "C"
