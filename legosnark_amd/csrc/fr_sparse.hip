// legosnark_amd/csrc/fr_sparse.hip -- sparse Fr matrices resident on the device: y = M x and y = M^T x for a CSR matrix
// (lsa_fr_sparse_create / lsa_fr_sparse_matvec), and on top of them the witness map of a Groth16-style prover,
// H = (A z . B z - C z) / Z (lsa_fr_qap_witness: three products, then lsa_fr_hadamard_quotient).
//
// Serves the R1CS of src/examples/legogrothmatrix.cc:79-117 (n^3 inner-product constraints of one to three entries a row
// over about 2 n^2 + n^3 variables) and the key generator's A^T L(t) (side 0 with the row of lsa_fr_lagrange).
//
// Every output is fr_sparse.h's row routine: coefficients that are exactly +1 or -1 (nearly all of a gadget library's) are
// limb additions of the gathered operand, the rest go four to a Montgomery reduction through fr_dot.h; canonical words out.
//
// The work is cut by nonzeros, not by rows.  At creation the rows are grouped by length (thresholds: lsa_fr_sparse_param):
//   k_sp_short   rows of at most SP_SHORT_MAX entries, empty ones included: a lane per row (up to SP_LANE_MAX entries when the
//                matrix has enough such rows to fill the chip with lanes).  The list of short rows keeps the matrix's order,
//                so neighbouring lanes read neighbouring stretches of vals / cols;
//   k_sp_chunk   longer rows are cut into chunks of SP_CHUNK entries; a wavefront owns a chunk, its lanes 64 entries apart
//                (consecutive coefficients and indices per load), the 64 lane sums meet in LDS; one partial sum per chunk;
//   k_sp_finish  a wavefront per long row adds the row's partial sums (they are consecutive), k_fr_matvec_finish's step.
// Every row is in exactly one group, so `out` is written once and never cleared.  The transposed orientation is a second CSR
// copy made on the host at creation (counting sort by column); the same kernels serve both sides.
//
// Every index a kernel uses is checked on the host when the handle is created: column indices against the column count, the
// row pointers for monotony and their end against nnz; the row lists, chunk bounds and partial-sum slots are derived from
// those.  The caller's x must hold as many elements as the side says.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "capi_internal.h"
#include "fr29.h"
#include "fr_dot.h"
#include "fr_sparse.h"

namespace lsa {

// Measured on one MI355X (tools/bench_fr_sparse.py, profiles/fr_sparse.txt; builds with -DLSA_SP_SHORT_MAX / -DLSA_SP_CHUNK loaded
// through LSA_LIB_VARIANT).  Rows of 33 .. 128 entries go either way: 2^16 rows of 1 .. 96 entries take 0.188 / 0.252 ms (side 1 /
// side 0) with a lane up to 32 entries and 0.140 / 0.111 ms with a lane up to 128 -- a wavefront on such a row pays 64 closing
// products and the LDS sum for one or two entries a lane -- but the 4096 rows of 64 entries of the matrix-product system's A^T
// take 0.025 ms as wavefronts and 0.039 ms as lanes, which are then 64 wavefronts on a chip of 256 CUs.  So such rows are
// lanes only when there are at least SP_LANE_FILL of them, a wavefront of lanes for every CU; the two measurements bracket
// that count, nothing in between was timed.  One row of 2^16 entries beside 2^18 short ones takes 0.057 / 0.047 / 0.042 /
// 0.040 ms in chunks of 1024 / 512 / 256 / 128.
#ifndef LSA_SP_SHORT_MAX
#define LSA_SP_SHORT_MAX 32
#endif
#ifndef LSA_SP_LANE_MAX
#define LSA_SP_LANE_MAX 128
#endif
#ifndef LSA_SP_CHUNK
#define LSA_SP_CHUNK 256
#endif
constexpr unsigned SP_SHORT_MAX = LSA_SP_SHORT_MAX;     // entries up to which a row is always one lane's
constexpr unsigned SP_LANE_MAX = LSA_SP_LANE_MAX;       // ... and up to which it is when the matrix has SP_LANE_FILL rows between the two
constexpr size_t SP_LANE_FILL = 256 * 64;
constexpr unsigned SP_CHUNK = LSA_SP_CHUNK;             // entries of a long row per wavefront: four per lane
constexpr unsigned SP_WAVES = 4;           // chunks (wavefronts) per workgroup
static_assert(SP_SHORT_MAX <= SP_LANE_MAX && SP_LANE_MAX < SP_CHUNK, "a row a lane may take is shorter than a chunk");

namespace {
typedef uint32_t sp_u32x4 __attribute__((ext_vector_type(4)));
struct SpLoad {
    __device__ __forceinline__ Fr operator()(const Fr *p) const {
        const sp_u32x4 *q = reinterpret_cast<const sp_u32x4 *>(p);
        const sp_u32x4 lo = q[0], hi = q[1];
        Fr x;
        x.l[0] = lo.x; x.l[1] = lo.y; x.l[2] = lo.z; x.l[3] = lo.w; x.l[4] = hi.x; x.l[5] = hi.y; x.l[6] = hi.z; x.l[7] = hi.w;
        return x;
    }
};
__device__ __forceinline__ void sp_store(Fr *p, const Fr &x) {
    sp_u32x4 lo, hi;
    lo.x = x.l[0]; lo.y = x.l[1]; lo.z = x.l[2]; lo.w = x.l[3]; hi.x = x.l[4]; hi.y = x.l[5]; hi.z = x.l[6]; hi.w = x.l[7];
    reinterpret_cast<sp_u32x4 *>(p)[0] = lo;
    reinterpret_cast<sp_u32x4 *>(p)[1] = hi;
}
}  // namespace

// One orientation on the device.  rows: the outputs; x has `xlen` elements and every cols[e] < xlen.
struct SpView {
    const Fr *vals;              // nnz coefficients (read where cls is general)
    const uint8_t *cls;          // nnz classes (fr_sparse_class)
    const uint32_t *cols;        // nnz indices into x
    const uint64_t *row_ptr;     // rows + 1
    const uint32_t *short_rows;  // nshort rows a lane each (at most SP_SHORT_MAX or SP_LANE_MAX entries), ascending
    const uint64_t *chunk_lo;    // nchunks: entries [chunk_lo, chunk_hi) of vals / cls / cols, at most SP_CHUNK
    const uint64_t *chunk_hi;
    const uint32_t *long_row;    // nlong: the other rows
    const uint64_t *long_first;  // nlong: the row's first chunk; its chunks are consecutive
    const uint32_t *long_parts;  // nlong: how many
    size_t rows, xlen, nnz, nshort, nchunks, nlong;
};

__global__ __launch_bounds__(256) void k_sp_short(SpView m, const Fr *__restrict__ x, Fr *__restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < m.nshort; i += (size_t)gridDim.x * 256) {
        const uint32_t r = m.short_rows[i];
        sp_store(out + r, fr_sparse_row(m.vals, m.cls, m.cols, x, m.row_ptr[r], m.row_ptr[r + 1], 1, SpLoad()));
    }
}

// the 64 lane values of every wavefront of the workgroup summed in place: s_red[wave * 64] holds the wavefront's sum
__device__ __forceinline__ void sp_reduce(Fr *s_red, unsigned lane) {
    __syncthreads();
    for (unsigned s = 32; s >= 1; s >>= 1) {
        if (lane < s) s_red[threadIdx.x] = s_red[threadIdx.x] + s_red[threadIdx.x + s];
        __syncthreads();
    }
}

// part[c] = the sum over chunk c
__global__ __launch_bounds__(256) void k_sp_chunk(SpView m, const Fr *__restrict__ x, Fr *__restrict__ part) {
    __shared__ Fr s_red[64 * SP_WAVES];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (size_t c0 = (size_t)blockIdx.x * SP_WAVES; c0 < m.nchunks; c0 += (size_t)gridDim.x * SP_WAVES) {
        const size_t c = c0 + wave;
        size_t lo = 0, hi = 0;                                  // (a wavefront past the last chunk sums nothing)
        if (c < m.nchunks) { lo = m.chunk_lo[c]; hi = m.chunk_hi[c]; }
        s_red[threadIdx.x] = fr_sparse_row(m.vals, m.cls, m.cols, x, lo + lane, hi, 64, SpLoad());
        sp_reduce(s_red, lane);
        if (lane == 0 && c < m.nchunks) sp_store(part + c, s_red[threadIdx.x]);
        __syncthreads();
    }
}

// out[long_row[i]] = the sum of the row's partial sums: a wavefront per long row, its lanes 64 partial sums apart (a row of
// 2^16 entries has 128 of them: one lane would wait for 128 loads one after the other)
__global__ __launch_bounds__(256) void k_sp_finish(SpView m, const Fr *__restrict__ part, Fr *__restrict__ out) {
    __shared__ Fr s_red[64 * SP_WAVES];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (size_t i0 = (size_t)blockIdx.x * SP_WAVES; i0 < m.nlong; i0 += (size_t)gridDim.x * SP_WAVES) {
        const size_t i = i0 + wave;
        Fr acc = Fr::zero();
        if (i < m.nlong) {
            const Fr *p = part + m.long_first[i];
            const uint32_t n = m.long_parts[i];
            for (uint32_t s = lane; s < n; s += 64) acc = acc + SpLoad()(p + s);
        }
        s_red[threadIdx.x] = acc;
        sp_reduce(s_red, lane);
        if (lane == 0 && i < m.nlong) sp_store(out + m.long_row[i], s_red[threadIdx.x]);
        __syncthreads();
    }
}

// ---------------------------------------------------------------- host side
struct SpSide {
    SpView v;
    std::vector<void *> owned;       // the device allocations behind v
    bool present = false;
};

namespace {
constexpr size_t SP_MAX_BLOCKS = (size_t)1 << 20;        // (the kernels stride over the rest)

// grow-only staging (released by lsa_shutdown): the chunks' partial sums; for host callers x and the result; for the witness
// map a, b, c and for its host callers H
StageBuf g_sp_part, g_sp_x, g_sp_out, g_sp_abc[3], g_sp_h;

void sp_free(SpSide &s) {
    for (void *p : s.owned) (void)hipFree(p);
    s.owned.clear();
    s.present = false;
}
// a device copy of `bytes` host bytes (nullptr for none), owned by s
int sp_copy(SpSide &s, const void *h, size_t bytes, const void **d) {
    *d = nullptr;
    if (!bytes) return LSA_OK;
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { set_error("fr_sparse_create: hipMalloc of %zu bytes failed", bytes); return LSA_ERR_NOMEM; }
    s.owned.push_back(p);
    HIPCHK(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
    *d = p;
    return LSA_OK;
}

// One orientation from checked CSR arrays: classes, the row groups, the copies.
int sp_build(SpSide &s, const Fr *vals, const uint32_t *cols, const uint64_t *row_ptr, size_t rows, size_t xlen, size_t nnz) {
    std::vector<uint8_t> cls(nnz);
    for (size_t e = 0; e < nnz; e++) cls[e] = fr_sparse_class(vals[e]);
    std::vector<uint32_t> short_rows, long_row, long_parts;
    std::vector<uint64_t> chunk_lo, chunk_hi, long_first;
    size_t middling = 0;
    for (size_t r = 0; r < rows; r++) middling += row_ptr[r + 1] - row_ptr[r] > SP_SHORT_MAX && row_ptr[r + 1] - row_ptr[r] <= SP_LANE_MAX;
    const uint64_t lane_max = middling >= SP_LANE_FILL ? SP_LANE_MAX : SP_SHORT_MAX;
    for (size_t r = 0; r < rows; r++) {
        const uint64_t lo = row_ptr[r], hi = row_ptr[r + 1];
        if (hi - lo <= lane_max) { short_rows.push_back((uint32_t)r); continue; }
        long_row.push_back((uint32_t)r);
        long_first.push_back(chunk_lo.size());
        uint32_t parts = 0;
        for (uint64_t at = lo; at < hi; at += SP_CHUNK, parts++) {
            chunk_lo.push_back(at);
            chunk_hi.push_back(hi - at < SP_CHUNK ? hi : at + SP_CHUNK);
        }
        long_parts.push_back(parts);
    }
    SpView &v = s.v;
    memset(&v, 0, sizeof v);
    v.rows = rows; v.xlen = xlen; v.nnz = nnz;
    v.nshort = short_rows.size(); v.nchunks = chunk_lo.size(); v.nlong = long_row.size();
    s.present = true;
    if (rows == 0) return LSA_OK;
    int rc;
    if ((rc = sp_copy(s, vals, nnz * sizeof(Fr), (const void **)&v.vals)) || (rc = sp_copy(s, cls.data(), nnz, (const void **)&v.cls)) ||
        (rc = sp_copy(s, cols, nnz * sizeof(uint32_t), (const void **)&v.cols)) ||
        (rc = sp_copy(s, row_ptr, (rows + 1) * sizeof(uint64_t), (const void **)&v.row_ptr)) ||
        (rc = sp_copy(s, short_rows.data(), short_rows.size() * sizeof(uint32_t), (const void **)&v.short_rows)) ||
        (rc = sp_copy(s, chunk_lo.data(), chunk_lo.size() * sizeof(uint64_t), (const void **)&v.chunk_lo)) ||
        (rc = sp_copy(s, chunk_hi.data(), chunk_hi.size() * sizeof(uint64_t), (const void **)&v.chunk_hi)) ||
        (rc = sp_copy(s, long_row.data(), long_row.size() * sizeof(uint32_t), (const void **)&v.long_row)) ||
        (rc = sp_copy(s, long_first.data(), long_first.size() * sizeof(uint64_t), (const void **)&v.long_first)) ||
        (rc = sp_copy(s, long_parts.data(), long_parts.size() * sizeof(uint32_t), (const void **)&v.long_parts)))
        return rc;
    return LSA_OK;
}

unsigned sp_grid(size_t items, size_t per_block) {
    const size_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < SP_MAX_BLOCKS ? b : SP_MAX_BLOCKS);
}

// d_x: v.xlen elements, d_out: v.rows, d_part: v.nchunks.  Asynchronous on st.
int sp_matvec_device(const SpView &v, const Fr *d_x, Fr *d_out, Fr *d_part, hipStream_t st) {
    if (v.rows == 0) return LSA_OK;
    if (v.nnz == 0) {                                            // the words of zero are zero bytes
        HIPCHK(hipMemsetAsync(d_out, 0, v.rows * sizeof(Fr), st));
        return LSA_OK;
    }
    if (v.nshort) hipLaunchKernelGGL(k_sp_short, dim3(sp_grid(v.nshort, 256)), dim3(256), 0, st, v, d_x, d_out);
    if (v.nchunks) {
        hipLaunchKernelGGL(k_sp_chunk, dim3(sp_grid(v.nchunks, SP_WAVES)), dim3(256), 0, st, v, d_x, d_part);
        hipLaunchKernelGGL(k_sp_finish, dim3(sp_grid(v.nlong, SP_WAVES)), dim3(256), 0, st, v, (const Fr *)d_part, d_out);
    }
    HIPCHK(hipGetLastError());
    return LSA_OK;
}
}  // namespace

}  // namespace lsa

using namespace lsa;

struct lsa_fr_sparse {
    SpSide side[2];                  // [1]: as given (a result per row); [0]: the transpose (a result per column), if kept
    size_t nrows = 0, ncols = 0, nnz = 0;
};

static int fr_sparse_create_checked(const Fr *vals, const uint32_t *cols, const uint64_t *row_ptr, size_t nrows, size_t ncols, size_t nnz,
                                    int keep_transpose, lsa_fr_sparse *m) {
    m->nrows = nrows; m->ncols = ncols; m->nnz = nnz;
    const uint64_t zero_ptr = 0;
    int rc = sp_build(m->side[1], vals, cols, nrows ? row_ptr : &zero_ptr, nrows, ncols, nnz);
    if (rc || !keep_transpose) return rc;
    // the transpose by a counting sort on the column: the entries of a column keep the order of their rows
    std::vector<uint64_t> tptr(ncols + 1, 0);
    for (size_t e = 0; e < nnz; e++) tptr[cols[e] + 1]++;
    for (size_t c = 0; c < ncols; c++) tptr[c + 1] += tptr[c];
    std::vector<uint64_t> next(tptr.begin(), tptr.end() - 1);
    std::vector<Fr> tvals(nnz);
    std::vector<uint32_t> trows(nnz);
    for (size_t r = 0; r < nrows; r++)
        for (uint64_t e = row_ptr[r]; e < row_ptr[r + 1]; e++) {
            const uint64_t at = next[cols[e]]++;
            tvals[at] = vals[e];
            trows[at] = (uint32_t)r;
        }
    return sp_build(m->side[0], tvals.data(), trows.data(), tptr.data(), ncols, nrows, nnz);
}

extern "C" {
size_t lsa_fr_sparse_param(int which) {
    switch (which) {
    case LSA_FR_SPARSE_PARAM_SHORT_MAX: return SP_SHORT_MAX;
    case LSA_FR_SPARSE_PARAM_CHUNK: return SP_CHUNK;
    case LSA_FR_SPARSE_PARAM_UNIT_MAX: return FR_SPARSE_UNIT_MAX;
    case LSA_FR_SPARSE_PARAM_LANE_MAX: return SP_LANE_MAX;
    case LSA_FR_SPARSE_PARAM_LANE_FILL: return SP_LANE_FILL;
    default: return 0;
    }
}

int lsa_fr_sparse_create(const void *vals, const uint32_t *cols, const uint64_t *row_ptr, size_t nrows, size_t ncols, size_t nnz,
                         int keep_transpose, lsa_fr_sparse **out) {
    LSA_TRACE_CALL("fr_sparse_create", nnz);
    if (out) *out = nullptr;
    int rc = require_ready();
    if (rc) return rc;
    if (!out) { set_error("fr_sparse_create: null out"); return LSA_ERR_INVALID; }
    if (nrows > 0xffffffffull || ncols > 0xffffffffull) {
        set_error("fr_sparse_create: %zu x %zu: row and column indices are 32 bits wide (at most 2^32 - 1 of either)", nrows, ncols);
        return LSA_ERR_INVALID;
    }
    size_t val_bytes;
    if (__builtin_mul_overflow(nnz, sizeof(Fr), &val_bytes)) { set_error("fr_sparse_create: %zu entries of 32 bytes overflow size_t", nnz); return LSA_ERR_INVALID; }
    if ((nrows && !row_ptr) || (nnz && (!vals || !cols))) { set_error("fr_sparse_create: null argument"); return LSA_ERR_INVALID; }
    if (nrows == 0) {
        if (nnz) { set_error("fr_sparse_create: %zu entries in a matrix without rows", nnz); return LSA_ERR_INVALID; }
    } else {
        if (row_ptr[0] != 0) { set_error("fr_sparse_create: row_ptr[0] = %llu, not 0", (unsigned long long)row_ptr[0]); return LSA_ERR_INVALID; }
        for (size_t r = 0; r < nrows; r++)
            if (row_ptr[r + 1] < row_ptr[r]) {
                set_error("fr_sparse_create: row_ptr decreases at row %zu (%llu -> %llu)", r, (unsigned long long)row_ptr[r], (unsigned long long)row_ptr[r + 1]);
                return LSA_ERR_INVALID;
            }
        if (row_ptr[nrows] != nnz) {
            set_error("fr_sparse_create: row_ptr[nrows] = %llu, nnz = %zu", (unsigned long long)row_ptr[nrows], nnz);
            return LSA_ERR_INVALID;
        }
    }
    for (size_t e = 0; e < nnz; e++)
        if (cols[e] >= ncols) { set_error("fr_sparse_create: entry %zu has column %u of %zu", e, cols[e], ncols); return LSA_ERR_INVALID; }
    lsa_fr_sparse *m = nullptr;
    try {
        m = new lsa_fr_sparse();
        rc = fr_sparse_create_checked((const Fr *)vals, cols, row_ptr, nrows, ncols, nnz, keep_transpose, m);
    } catch (const std::bad_alloc &) {
        set_error("fr_sparse_create: out of host memory");
        rc = LSA_ERR_NOMEM;
    }
    if (rc) {
        if (m) { sp_free(m->side[0]); sp_free(m->side[1]); delete m; }
        return rc;
    }
    *out = m;
    return LSA_OK;
}

void lsa_fr_sparse_destroy(lsa_fr_sparse *m) {
    if (!m) return;
    if (g.ready) (void)hipStreamSynchronize(g.stream);          // (a product of this matrix may still be running)
    sp_free(m->side[0]);
    sp_free(m->side[1]);
    delete m;
}

size_t lsa_fr_sparse_rows(const lsa_fr_sparse *m) { return m ? m->nrows : 0; }
size_t lsa_fr_sparse_cols(const lsa_fr_sparse *m) { return m ? m->ncols : 0; }
size_t lsa_fr_sparse_nnz(const lsa_fr_sparse *m) { return m ? m->nnz : 0; }

int lsa_fr_sparse_matvec(const lsa_fr_sparse *m, const void *x, int side, void *out, int on_device) {
    int rc = require_ready();
    if (rc) return rc;
    if (!m) { set_error("fr_sparse_matvec: null matrix"); return LSA_ERR_INVALID; }
    LSA_TRACE_CALL("fr_sparse_matvec", m->nnz);
    if (side != 0 && side != 1) { set_error("fr_sparse_matvec: side %d (0: out[c] = sum_r x[r] M[r][c], 1: out[r] = sum_c M[r][c] x[c])", side); return LSA_ERR_INVALID; }
    const SpSide &s = m->side[side];
    if (!s.present) { set_error("fr_sparse_matvec: side 0 needs a matrix created with keep_transpose"); return LSA_ERR_INVALID; }
    const SpView &v = s.v;
    const size_t out_bytes = v.rows * sizeof(Fr), x_bytes = v.xlen * sizeof(Fr);
    if (v.rows == 0) return LSA_OK;
    if (!out || (x_bytes && v.nnz && !x)) { set_error("fr_sparse_matvec: null argument"); return LSA_ERR_INVALID; }
    if (overlap(out, out_bytes, x, x_bytes)) { set_error("fr_sparse_matvec: out overlaps x"); return LSA_ERR_INVALID; }
    if (on_device && (misaligned(x) || misaligned(out))) { set_error("fr_sparse_matvec: device pointers must be 16-byte aligned"); return LSA_ERR_INVALID; }
    OperandFrame f("fr_sparse_matvec", on_device);
    Fr *d_part = f.scratch<Fr>(g_sp_part, v.nchunks * sizeof(Fr));
    const Fr *d_x = f.in<Fr>(g_sp_x, x, v.nnz ? x_bytes : 0, x_bytes);       // (a matrix without entries reads no x: it may be null)
    Fr *d_out = f.out<Fr>(g_sp_out, out, out_bytes);
    if (f.rc()) return f.rc();
    rc = sp_matvec_device(v, d_x, d_out, d_part, g.stream);
    if (rc) return rc;
    return f.download();
}

int lsa_fr_qap_witness(const lsa_fr_sparse *A, const lsa_fr_sparse *B, const lsa_fr_sparse *C, const void *z, size_t big_log, int small_log,
                       const void *omega, const void *coset_g, const void *d123, void *h_out, int on_device) {
    int rc = require_ready();
    if (rc) return rc;
    if (!A || !B || !C || !omega || !coset_g || !h_out) { set_error("fr_qap_witness: null argument"); return LSA_ERR_INVALID; }
    LSA_TRACE_CALL("fr_qap_witness", A->nnz + B->nnz + C->nnz);
    if (A->nrows != B->nrows || A->nrows != C->nrows || A->ncols != B->ncols || A->ncols != C->ncols) {
        set_error("fr_qap_witness: A is %zu x %zu, B %zu x %zu, C %zu x %zu: one constraint system has one shape", A->nrows, A->ncols, B->nrows, B->ncols,
                  C->nrows, C->ncols);
        return LSA_ERR_INVALID;
    }
    const size_t n = A->nrows, nvars = A->ncols;
    if (nvars && !z) { set_error("fr_qap_witness: null argument"); return LSA_ERR_INVALID; }
    static const uint32_t no_blinding[3 * 8] = {0};              // three zeros
    if (!d123) d123 = no_blinding;
    // a domain lsa_fr_hadamard_quotient refuses: its refusal, before any work here (the same conditions as its check)
    const bool domain_ok = small_log < 0 ? (big_log >= 1 && big_log <= 28) : (big_log <= 27 && (size_t)small_log < big_log);
    if (!domain_ok) return lsa_fr_hadamard_quotient(omega, omega, omega, 0, big_log, small_log, omega, coset_g, d123, h_out, on_device);
    const size_t points = ((size_t)1 << big_log) + (small_log >= 0 ? (size_t)1 << small_log : 0);
    if (n > points) { set_error("fr_qap_witness: %zu constraints on a domain of m = %zu points", n, points); return LSA_ERR_INVALID; }
    const size_t z_bytes = nvars * sizeof(Fr), h_bytes = (points + 1) * sizeof(Fr);
    if (overlap(h_out, h_bytes, z, z_bytes)) { set_error("fr_qap_witness: h_out overlaps z"); return LSA_ERR_INVALID; }
    if (on_device && (misaligned(z) || misaligned(h_out))) { set_error("fr_qap_witness: device pointers must be 16-byte aligned"); return LSA_ERR_INVALID; }
    const lsa_fr_sparse *mats[3] = {A, B, C};
    size_t chunks = 0;
    for (const lsa_fr_sparse *m : mats) chunks = m->side[1].v.nchunks > chunks ? m->side[1].v.nchunks : chunks;
    OperandFrame f("fr_qap_witness", on_device);
    Fr *d_part = f.scratch<Fr>(g_sp_part, chunks * sizeof(Fr));
    const Fr *d_z = f.in<Fr>(g_sp_x, z, z_bytes);
    void *d_h = f.out(g_sp_h, h_out, h_bytes);
    Fr *d_abc[3];
    for (int j = 0; j < 3; j++) d_abc[j] = f.scratch<Fr>(g_sp_abc[j], (n ? n : 1) * sizeof(Fr));     // (never null: n == 0 passes them on unread)
    if (f.rc()) return f.rc();
    for (int j = 0; j < 3; j++) {
        rc = sp_matvec_device(mats[j]->side[1].v, d_z, d_abc[j], d_part, g.stream);
        if (rc) return rc;
    }
    rc = lsa_fr_hadamard_quotient(d_abc[0], d_abc[1], d_abc[2], n, big_log, small_log, omega, coset_g, d123, d_h, 1);
    if (rc) return rc;
    return f.download();
}
}  // extern "C"
