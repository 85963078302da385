/* include/legosnark_amd.h -- C-ABI of the MI355X (gfx950) implementation of LegoSNARK's
 * elliptic-curve hot path: alt_bn128 G1/G2 multi-scalar multiplication, fixed-base
 * batch exponentiation, and batched Miller-loop / final-exponentiation.
 *
 * The reference has no FFI layer: its gadgets call libff's C++ templates directly
 * (SURVEY.md section 8b).  This header is the boundary a libff-compatible shim binds
 * (legosnark_amd/shim/libff/...; INTEGRATION.md shows the forwarding wrappers).  Every
 * entry point names the reference interface it replaces (file:line under
 * /root/reference).
 *
 * Conventions
 *  - Plain pointers and sizes only; all buffers caller-owned.
 *  - Byte layout = libff's in-memory layout: Fr/Fq = 32 B, 4 x u64 little-endian limbs in
 *    Montgomery form (R = 2^256); G1 = {X,Y,Z} Jacobian 96 B (Z == 0 <=> infinity);
 *    Fq2 = {c0,c1} 64 B; G2 = 192 B; GT = Fq12 = {c0:{c0,c1,c2}, c1:{..}} 384 B.
 *  - Return 0 on success, negative lsa_status on failure; lsa_last_error() gives text.
 *    No exceptions cross the boundary.  There is NO CPU fallback: without a usable
 *    gfx950 device every compute entry point fails with LSA_ERR_NO_DEVICE.
 *  - One process drives one GPU (lsa_init(device)); calls are issued from one host
 *    thread at a time, matching the reference (single caller thread).
 *  - Results are the same group / field elements libff computes.  Jacobian outputs are
 *    valid representatives (compare with libff operator== or after
 *    to_affine_coordinates()); field outputs (GT) are canonical, hence bit-identical.
 */
#ifndef LEGOSNARK_AMD_H
#define LEGOSNARK_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden (it is meant to be linked beside libsnark / libff builds and other
 * C++ code): the entry points declared in this header are its ONLY dynamic symbols (tests/test_capi_symbols.py). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef enum {
    LSA_OK = 0,
    LSA_ERR_NO_DEVICE = -1,   /* no HIP device / wrong arch / lsa_init not called */
    LSA_ERR_INVALID = -2,     /* bad argument */
    LSA_ERR_HIP = -3,         /* HIP runtime error, see lsa_last_error() */
    LSA_ERR_NOMEM = -4
} lsa_status;

/* ---- lifecycle -------------------------------------------------------------------- */
/* Replaces default_ec_pp::init_public_params() as the one-time setup call
 * (src/examples/cplink.cc:81).  Selects `device`, creates the library's HIP stream, and pays here what the first calls
 * of a prover would otherwise pay inside themselves: the code object, the internal streams and their copy-engine queues,
 * the pinned slots of the host-copy path, and workspaces / staging buffers sized for 2^20 pairs of G1 or G2 (about 1 GB
 * of device memory; LSA_WARM=0: everything lazily, LSA_WARM_MB=m: another size) -- a hipFree + hipMalloc pair inside a
 * call costs 0.5 to 10+ ms depending on the box.  A failed warm-up is reported and leaves the library shut down. */
int lsa_init(int device);
void lsa_shutdown(void);
int lsa_device_count(void);
const char *lsa_last_error(void);
/* hipStream_t on which every kernel of this library is launched (for HIP-event timing). */
void *lsa_stream(void);
/* Block until all work queued by this library has finished. */
int lsa_synchronize(void);
/* The tail of an lsa_msm_run_async call (bucket reduction + fold) runs on an internal stream so
 * that it overlaps the next call's front phase.  lsa_stream_join() makes lsa_stream() wait for
 * every tail issued so far: call it before ordering foreign work (another stream's wait, a
 * collective) after lsa_stream().  All synchronous entry points and lsa_*_sum_async join
 * implicitly. */
int lsa_stream_join(void);
/* The same for a stream of the caller's (hipStream_t): it waits for the tails issued so far,
 * lsa_stream() does not -- the next MSM's front keeps overlapping them.  With LSA_NO_OVERLAP=1
 * there are no internal streams and the caller must order `stream` after lsa_stream() itself. */
int lsa_stream_join_to(void *stream);

/* ---- variable-base MSM from host buffers ------------------------------------------- */
/* out = sum_i scalars[i] * bases[i], i < n.
 * Replaces libff::multi_exp_with_mixed_addition<G1<pp>,Fr<pp>,multi_exp_method_BDLO12>
 * (src/utils/globl.h:74-77, multiExpMA) and libff::multi_exp<..BDLO12>
 * (src/utils/sparsemexp.h:58,89).  `chunks` is libff's CPU work split
 * (src/utils/globl.h:67-71; omp_get_max_threads() in the reference's -DMULTICORE=ON build); it does not change the
 * result and is accepted for signature compatibility only.  bases: n x 96 B (G1) / 192 B (G2); scalars: n x 32 B;
 * out: one Jacobian point.
 * Host buffers the library has not been handed before travel through its own pinned slots (a range is copied directly
 * by the runtime only from its third sighting on): the first call on a 2^20-point G1 vector is ~7 ms whatever pages
 * the caller's allocator uses.  Callers should not free large buffers right before a call: unmapping memory the HIP
 * runtime has touched stalls the next submission by 15-25 ms (the libff-compatible shim keeps vectors on the heap). */
int lsa_g1_msm(const void *bases_jac, const void *scalars_mont, size_t n, size_t chunks, void *out_jac);
int lsa_g2_msm(const void *bases_jac, const void *scalars_mont, size_t n, size_t chunks, void *out_jac);

/* CRS cache behind lsa_g1_msm / lsa_g2_msm.  The reference passes the SAME std::vector<G> on
 * every call of a prover (crs->P, src/gadgets/subspace.cc:82; g1s/g2s, src/prototools/commit.h:
 * 154-155; prefixes of g1s, src/gadgets/poly.h:77-86), so vectors of >= 1024 points stay
 * resident on the GPU in prepared form, keyed by host pointer and verified by content before
 * every use.  mode 2 (default; env LSA_CRS_CACHE=full): every byte of the n points passed is
 * fingerprinted (64-point units, host thread pool, overlapped with the scalar upload) -- a
 * vector modified in place is a miss, never a stale result.  mode 1 (LSA_CRS_CACHE=sampled):
 * ~3*log2(n) sampled points are compared; for callers that do not modify CRS vectors in place.
 * mode 0 (LSA_CRS_CACHE=0): every call uploads and normalises its bases.  Vectors below 1024 points are not kept,
 * but are recognised as prefixes of a kept one (whole 64-point units, or fewer than 64 points) and then served from it.  Entries are evicted
 * least-recently-used beyond max_bytes of device memory (0 keeps the current budget; default
 * min(1/4 of the device, 64 GiB), env LSA_CRS_CACHE_MB).  The first re-use of an entry of at
 * least the table threshold that has been hit often enough also STARTS building its pre-shifted window copies
 * (lsa_crs_cache_table_after). */
int lsa_crs_cache_configure(int mode, size_t max_bytes);
/* The pre-shifted copies of an entry are built in the BACKGROUND (a low-priority stream, 26 copies ~ 27 ms of GPU time
 * at 2^20 G1 points, 64 ms for G2) once the entry has been hit `hits` times (default 23, the break-even of 27 ms
 * against the ~1.2 ms a 2^20-pair MSM saves with them; 0: never; env LSA_CRS_TABLE_AFTER): the call that starts the
 * build and the calls during it run at plain-pipeline speed, the entry switches to the copies when they are complete
 * -- results are the same point either way.  They hold 26 x 64 B per G1 point (128 B per G2 point).  A prover that
 * knows it will re-use a key many times sets 1. */
int lsa_crs_cache_table_after(unsigned hits);
/* Blocks until every background build has finished and its entry has switched (tests, benchmarks). */
int lsa_crs_cache_wait_tables(void);
void lsa_crs_cache_clear(void);
int lsa_crs_cache_stats(uint64_t *hits, uint64_t *misses, uint64_t *resident_bytes, uint64_t *entries);
/* Host-side wall-clock split of the most recent lsa_g1_msm / lsa_g2_msm call, as the caller of
 * multiExpMA experiences it (SURVEY.md 8e "Host staging": H2D reported separately). */
typedef struct {
    size_t n;
    int cache_hit;               /* 1: bases were resident */
    int table;                   /* 1: the call used the entry's pre-shifted window copies; 2: the copies of the entry's first
                                  * points only (a G1 entry without full copies serving a request of <= 2^16 pairs: built in one
                                  * kernel on the first such request, LSA_CRS_PREFIX_TABLE) */
    double h2d_scalars_ms;       /* pageable host -> device copy of n x 32 B */
    double fingerprint_wait_ms;  /* what was left of the fingerprint pass after that copy */
    double bases_prepare_ms;     /* miss: upload + normalise (+ table on first re-use); hit: lookup */
    double msm_ms;               /* kernels + 96/192-byte result copy */
    double total_ms;
    int table_building;          /* 1: the entry's pre-shifted copies are being built in the background */
} lsa_host_stats;
int lsa_msm_host_stats(lsa_host_stats *out);

/* ---- device-resident bases (CRS) ---------------------------------------------------- */
/* The CRS vectors passed to multiExpMA are fixed per key (crs->P at
 * src/gadgets/subspace.cc:82, g1s/g2s at src/prototools/commit.h:154-155), so they are
 * uploaded once, batch-normalised to affine in HBM (64 B / 128 B per point) and reused.
 * `bases_jac` may be a host pointer or (src_on_device != 0) a device pointer.
 * Handles of >= 2^19 points (LSA_PRECOMPUTE_MIN, lsa_msm_set_table_threshold) also keep 26 (24) pre-shifted copies of
 * every point (lsa_bases_has_table); so do G1 handles of up to 2^16 points -- their copies come from ONE kernel, ~1.2 ms --
 * unless a threshold was set explicitly.  G1 MSMs of up to 2^17 pairs over such a handle take a four-launch pipeline
 * (csrc/msm_compact.hip: 0.12-0.25 ms blocking for n <= 2^14). */
typedef struct lsa_bases lsa_bases;
int lsa_g1_bases_create(const void *bases_jac, size_t n, int src_on_device, lsa_bases **out);
int lsa_g2_bases_create(const void *bases_jac, size_t n, int src_on_device, lsa_bases **out);
void lsa_bases_destroy(lsa_bases *b);
size_t lsa_bases_size(const lsa_bases *b);
/* Resident vectors of at least 2^19 points (env LSA_PRECOMPUTE_MIN) also keep 26 pre-shifted
 * copies 2^(pos_j)*P_i at bit positions about 10 apart (24 copies about 11 apart from 6*2^20
 * points on; G1 64 B, G2 128 B per point and copy; LSA_PRECOMPUTE=0 disables).  Every MSM on such a handle then runs over ONE bucket space shared by
 * all windows: 13 (12) bucket additions per pair instead of 16 and no GLV beta-multiplications for
 * n >= 2^16, 26 narrow digits and only 512 buckets to reduce below; one bucket reduction, no
 * Horner fold.  lsa_msm_set_table_threshold(t), t != 0: vectors of at least t points get the
 * copies and only MSMs of at least t pairs use them (tests); 0 restores the defaults.
 * lsa_bases_has_table() tells whether a handle carries the copies. */
void lsa_msm_set_table_threshold(size_t threshold);
int lsa_bases_has_table(const lsa_bases *b);
unsigned lsa_bases_table_windows(const lsa_bases *b);   /* 0 without the copies */
/* Field multiplications per point-scalar pair in the bucket-accumulation kernel for an MSM of n
 * pairs on this handle (NULL: host-buffer path) -- the operation count behind bench.py's
 * integer-throughput roofline: 10 per bucket addition (XYZZ mixed add, 8M + 2S), plus one
 * beta-multiplication per GLV half on the plain path. */
unsigned lsa_msm_field_mults_per_pair(const lsa_bases *b, size_t n);
/* Device pointer to the normalised affine array (n x 64 B / 128 B), for inspection. */
const void *lsa_bases_device_ptr(const lsa_bases *b);

/* MSM over bases[first .. first+n) with scalars already resident in HBM
 * (d_scalars_mont: device pointer, n x 32 B, Montgomery Fr).  out_jac is a HOST buffer
 * (96 B / 192 B); the call returns after the result has landed there (the whole call runs on lsa_stream() and its last
 * kernel writes into pinned host memory: no cross-stream hand-over, no copy command behind the kernels). */
int lsa_msm_run(const lsa_bases *bases, size_t first, const void *d_scalars_mont, size_t n, void *out_jac);
/* Same, asynchronous: result is written to the DEVICE buffer d_out_jac; it is ordered on
 * lsa_stream() after lsa_stream_join() (or any synchronous call). */
int lsa_msm_run_async(const lsa_bases *bases, size_t first, const void *d_scalars_mont, size_t n, void *d_out_jac);

/* Several independent MSMs over PREFIXES of the same resident bases in one pass -- the ladder
 * of CPPoly::prove (src/gadgets/poly.h:77-86: witness[i] = multiExpMA(g1s, w[start_i ..
 * start_i + 2^(d-1-i))), whose scalar slices are consecutive in one array):
 *   d_out_jac[j] = sum_i d_scalars[seg_offsets[j] + i] * bases[first + i],
 *                  i < seg_offsets[j+1] - seg_offsets[j],      j < nseg <= 64.
 * seg_offsets: HOST array of nseg + 1 non-decreasing element offsets into d_scalars_mont (device).
 * d_out_jac: DEVICE, nseg points (infinity for an empty segment).  The bases must carry the
 * pre-shifted copies (lsa_bases_has_table).  Meant for segments of up to about 2^16 pairs (each
 * is cut into 26 ten-bit digits over 512 buckets of its own); longer ones are better issued
 * through lsa_msm_run_async.  Asynchronous like lsa_msm_run_async. */
int lsa_msm_run_segments_async(const lsa_bases *bases, size_t first, const void *d_scalars_mont, const uint64_t *seg_offsets, size_t nseg,
                               void *d_out_jac);

/* CommScheme::commit (src/prototools/commit.h:149-158; CPPoly::commitPoly, src/gadgets/poly.h:30-32):
 *   c = multiExpMA<LG1>(g1s, v),   kc = multiExpMA<LG2>(g2s, v)
 * -- a G1 and a G2 MSM over the SAME scalar vector.  The scalar sort (digits, ranks, scatter) does
 * not depend on the bases, so it runs once for both when the two handles carry pre-shifted copies
 * over the same number of points (otherwise this is two lsa_msm_run_async calls).  bases[0 .. n)
 * of both handles; d_scalars_mont, d_out_g1 (96 B), d_out_g2 (192 B): DEVICE.  Asynchronous like
 * lsa_msm_run_async. */
int lsa_commit_run_async(const lsa_bases *g1_bases, const lsa_bases *g2_bases, const void *d_scalars_mont, size_t n, void *d_out_g1,
                         void *d_out_g2);

/* Window width (bits) the MSM uses for n pairs -- exposed for DESIGN.md / tests. */
unsigned lsa_msm_window_bits(size_t n);

/* ---- per-stage timing (HIP events on lsa_stream()) ----------------------------------- */
#define LSA_MSM_STAGES 8
/* 0 digits+histogram, 1 scan, 2 scatter (+ fine sort), 3 bucket accumulate (dominant; the
 * accumulate kernels alone), 4 bucket reduce, 5 window fold, 6 ordering of the buckets by
 * population (between scatter and accumulate), 7 total */
int lsa_profile_enable(int on);   /* also resets the recorded-call counter */
/* Average milliseconds per stage over the MSM calls (at most 64) recorded since
 * lsa_profile_enable(1); synchronises on their events; returns the number of calls. */
int lsa_profile_last_msm(float ms[LSA_MSM_STAGES]);

/* ---- fixed-base batch exponentiation ------------------------------------------------ */
/* out[i] = scalars[i] * base, i < n.  Replaces libff get_window_table + batch_exp as used
 * by cputil::simpleBatchExp (src/utils/util.h:119-134) and Interpolator::mkG1Exp/mkG2Exp
 * (src/prototools/interp.h:36-59).  base: one HOST Jacobian point; scalars: n x 32 B
 * Montgomery Fr; out: n Jacobian points (valid representatives, not normalised).
 * `on_device` != 0: scalars and out are device pointers, else host pointers.
 * libff builds the window table once per base and calls batch_exp many times over it; this interface takes the base
 * with every call, so the device tables of the last four bases are kept (keyed by the base's bytes and the window
 * width, LSA_BEXP_TABLES): the first call on a base pays its 254 dependent doublings (~1.0 ms G1 / 2.6 ms G2),
 * later ones ~0.08 / 0.15 ms for a handful of scalars.  The result is complete when the call returns. */
int lsa_g1_batch_exp(const void *base_jac, const void *scalars_mont, size_t n, void *out_jac, int on_device);
int lsa_g2_batch_exp(const void *base_jac, const void *scalars_mont, size_t n, void *out_jac, int on_device);

/* ---- sum of points --------------------------------------------------------------------- */
/* out = sum_i pts[i]; pts: n Jacobian points on the DEVICE, d_out_jac: DEVICE (async on
 * lsa_stream()).  Folds the per-GPU MSM partials after the RCCL all-gather that replaces
 * libff's `final = final + partial[i]` loop over chunks (multi_exp). */
int lsa_g1_sum_async(const void *d_pts_jac, size_t n, void *d_out_jac);
int lsa_g2_sum_async(const void *d_pts_jac, size_t n, void *d_out_jac);
/* The same on a stream of the caller's (hipStream_t) instead of lsa_stream(). */
int lsa_g1_sum_on(const void *d_pts_jac, size_t n, void *d_out_jac, void *stream);
int lsa_g2_sum_on(const void *d_pts_jac, size_t n, void *d_out_jac, void *stream);

/* ---- variable-base batch scalar multiplication / sparse matrix in the exponent ---------- */
/* out[i] = scalars[i] * pts[i], i < n: the independent 254-bit scalar multiplications of
 * CPlink key generation -- `acc*one` and the one- and two-term multi_exp calls of sparsemexpG
 * (src/utils/sparsemexp.h:62-90) -- and of init_as_random-style input generation
 * (src/examples/cplink.cc:51-58) when the bases differ.  pts: libff G1 (96 B), scalars: Fr
 * (32 B), out: libff G1.  on_device != 0: device pointers, else host pointers. */
int lsa_g1_scalar_mul_batch(const void *pts_jac, const void *scalars_mont, size_t n, void *out_jac, int on_device);
/* mtxmultiexp(out, exps, M) for a column-major sparse matrix of G1 elements
 * (src/gadgets/subspace.cc:18-25 -> simplesparsemexp, src/utils/sparsemexp.cc:15-24):
 *   out[j] = sum_{e = col_ptr[j]}^{col_ptr[j+1]-1} exps[rows[e]] * vals[e],   j < ncols.
 * CSC layout: vals (nnz x 96 B libff G1) and rows (nnz x u32, the CoeffPos::pos of
 * src/utils/matrix.h:35-42) ordered by column, col_ptr (ncols+1 x u64, col_ptr[0] = 0,
 * col_ptr[ncols] = nnz).  exps: nrows x Fr.  out: ncols x libff G1 (infinity for an empty
 * column).  Host pointers.  Row indices >= nrows are rejected (LSA_ERR_INVALID). */
int lsa_g1_sparse_matrix_msm(const void *vals_jac, const uint32_t *rows, const uint64_t *col_ptr, size_t ncols,
                             const void *exps_mont, size_t nrows, void *out_jac);
/* The same two calls on G2 (the kc halves of Comm{c, kc}: Comm::operator*, src/prototools/commit.h:25-53; evalAsPolyOn over
 * commitments, src/prototools/polytools.h:104-113): points are 192 B libff G2; argument checks, error codes, n == 0 / ncols == 0,
 * host / device modes and blocking behaviour are those of the G1 calls.  What is new for G2: the result is the INTEGER
 * multiple of the point by the canonical value of the scalar (0 <= s < r) for ANY point of the twist, in or out of the
 * order-r subgroup -- no endomorphism is used (csrc/smul_g2.h).  The input is not checked for being on the curve;
 * lsa_g2_validate does that. */
int lsa_g2_scalar_mul_batch(const void *pts_jac, const void *scalars_mont, size_t n, void *out_jac, int on_device);
int lsa_g2_sparse_matrix_msm(const void *vals_jac, const uint32_t *rows, const uint64_t *col_ptr, size_t ncols,
                             const void *exps_mont, size_t nrows, void *out_jac);
/* Test and tool support, not needed to use the calls above: the compiled shape of the two ladders, so that tests and
 * benchmarks follow a retune.  0 for an unknown selector. */
#define LSA_SMUL_PARAM_G1_WINDOW_BITS 0     /* -> bits per signed digit, G1 */
#define LSA_SMUL_PARAM_G2_WINDOW_BITS 1     /* -> bits per signed digit, G2 */
#define LSA_SMUL_PARAM_G1_RESIDENT_ITEMS 2  /* -> items in flight in one pass of the persistent grid, G1 */
#define LSA_SMUL_PARAM_G2_RESIDENT_ITEMS 3  /* -> the same, G2 */
#define LSA_SMUL_PARAM_G2_LANES_PER_ITEM 4  /* -> lanes that share one G2 item */
size_t lsa_smul_param(int which);

/* ---- the discrete Fourier transform on group elements ------------------------------------ */
/* out[k] = sum_{i < n} omega^(ik) * in[i], n = 2^log_n, natural order in and out: lsa_fr_ntt's transform (no coset) with
 * group elements for data.  inverse != 0: omega^-1 in place of omega, then every out[k] multiplied by n^-1 mod r.
 * in[i] = a_i * G for all i  =>  out[k] = (lsa_fr_ntt(a))[k] * G.  The inverse transform of a powers string chi^i * G is
 * the Lagrange-basis key L_i(chi) * G of InterpCommScheme (src/gadgets/lipmaa.h:38-53) without the trapdoor: INTEGRATION.md,
 * "Lipmaa keys from a powers string (no trapdoor)".
 *
 * Points are libff Jacobian (96 B for G1, 192 B for G2; Z == 0: infinity), need not be normalised on input and are valid
 * representatives, not normalised, on output.  omega: a HOST pointer to one Fr (Montgomery form, as for lsa_fr_ntt) in
 * both modes.  on_device != 0: in and out are device pointers (16-byte aligned) and the call is asynchronous on
 * lsa_stream(): no host synchronisation inside, working memory is library-owned and grow-only, so only the first call of
 * a larger size waits for the device.  Otherwise host pointers, and the call blocks.  out == in exactly is legal (in
 * place).  log_n == 0 copies the one point.
 *
 * LSA_ERR_INVALID, before any device work and before the library is asked for a device: a null pointer; out overlapping in
 * without being in; log_n > 24; an omega that is not a primitive 2^log_n-th root of unity (omega^(n/2) != -1; omega != 1
 * for log_n == 0).
 *
 * Not checked: that the inputs are on the curve (as for lsa_g1_scalar_mul_batch).  For G2 the twiddles compose mod r, so
 * the result is the transform only for points of the order-r subgroup -- lsa_g2_validate checks that; points of the twist
 * outside the subgroup give some point of the twist (every ladder returns the integer multiple) and never a fault.
 *
 * Cost: a radix-2 network of log_n stages, each butterfly one 254-bit scalar multiplication and two complete additions.
 * Stage 1 and every butterfly whose twiddle is 1 run no ladder: (n/2)(log_n - 2) + 1 ladders forward (fewer than
 * (n/2)(log_n - 1)), n more for the inverse's factor n^-1 (applied to the inputs, one scalar for every lane).
 *
 * Out of scope: sizes that are not powers of two (libfqfft's step domain), coset variants, more than one GPU, and the
 * libff shim (the reference knows its trapdoor: none of its call sites changes). */
int lsa_g1_ecntt(const void *in_jac, void *out_jac, size_t log_n, const void *omega_mont, int inverse, int on_device);
int lsa_g2_ecntt(const void *in_jac, void *out_jac, size_t log_n, const void *omega_mont, int inverse, int on_device);
/* Test and tool support, like lsa_smul_param; 0 for an unknown selector. */
#define LSA_ECNTT_PARAM_G1_RESIDENT_BUTTERFLIES 0  /* -> butterflies in flight in one pass of the stage kernel's grid, G1 */
#define LSA_ECNTT_PARAM_G2_RESIDENT_BUTTERFLIES 1  /* -> the same, G2 */
#define LSA_ECNTT_PARAM_G2_LANES_PER_BUTTERFLY 2   /* -> lanes that share one G2 butterfly */
#define LSA_ECNTT_PARAM_MAX_LOG_N 3                /* -> the largest log_n the calls accept */
size_t lsa_ecntt_param(int which);

/* ---- Fr vectors around the MSMs --------------------------------------------------------- */
/* Witness coefficients of CPPoly::prove (src/gadgets/poly.h:55-67): with v of length 2^d and the
 * evaluation point r of length d, round i = 0..d-1 over m = 2^(d-1-i) pairs writes
 *   w[start + p] = v[2p+1] - v[2p],   v'[p] = -v[2p]*(r[i]-1) + v[2p+1]*r[i],   start += m.
 * w has 2^d entries (the last one stays zero, as in the reference's value-initialised vector);
 * w[start .. start+m) is the scalar vector of the i-th MSM of the proof (poly.h:77-86) and can
 * be passed to lsa_msm_run_async without leaving the device.  v is not modified.
 * on_device != 0: v, r, w are device pointers; else host pointers. */
int lsa_fr_cppoly_witness(const void *v_mont, size_t d, const void *r_mont, void *w_mont, int on_device);
/* out = evalMLE(v, r) (MultiVPolyT::evalMLE, src/prototools/polytools.h:207-234): the
 * multilinear extension of v (2^d entries, index bit i pairs with r[i]) at r.  One Fr.
 * on_device != 0: v, r, out are device pointers; else host pointers. */
int lsa_fr_eval_mle(const void *v_mont, size_t d, const void *r_mont, void *out_mont, int on_device);
/* DPMle::pushRandomness (src/prototools/mle.h:199-210): cur[p] = old[p]*(1-r) + old[p+half]*r,
 * p < half; old has 2*half entries, r is ONE Fr; cur may alias old.  on_device != 0: all three
 * are device pointers and the call is asynchronous on lsa_stream(); else host pointers. */
int lsa_fr_fold(const void *old_mont, size_t half, const void *r_mont, void *cur_mont, int on_device);

/* One round polynomial of the sumcheck prover (CPSumcheck::make_new_h_poly,
 * src/gadgets/sumcheck.h:85-106):
 *   h_j(X) = sum_{p < half} betaPoly(j,p)(X) * prod_{t < m} mlePoly_t(j,p)(X),
 * mlePoly_t(j,p) = tables[t][p]*(1-X) + tables[t][p+half]*X (DPMle::getMLEPoly, mle.h:217-226; the
 * tables are the DPMle curVTable's, 2*half entries each), betaPoly(j,p) =
 * eqbit_poly(rho_j) * pre * suff[p] (DPBeta::getBetaPoly, mle.h:74-82: pre = getBetaPre(j-1),
 * suff = beta_suff_rho_cur, half entries, NULL = all ones as for j+1 > d-1).  rho_j == NULL drops
 * the beta factor altogether (DPBetaDummy, mle.h:148-166).  1 <= m <= 4.
 * out_coeffs (HOST): m+2 coefficients of h_j, lowest degree first (m+1 when rho_j == NULL).
 * pre, rho_j: HOST pointers to one Fr each.  on_device != 0: suff and tables[t] are device
 * pointers (the array `tables` itself is a host array of m pointers); else host pointers. */
int lsa_fr_sumcheck_round(const void *suff_mont, const void *const *tables, size_t m, size_t half, const void *pre_mont,
                          const void *rho_j_mont, void *out_coeffs_mont, int on_device);
/* DPBeta::pushRandomness, suffix table (src/prototools/mle.h:46-53): cur[p] = old[half + p] * k,
 * p < half (k = rhoInvs[j+1], ONE Fr, HOST pointer); cur may alias old.  on_device != 0: old,
 * cur are device pointers, asynchronous on lsa_stream(); else host pointers. */
int lsa_fr_scale_upper(const void *old_mont, size_t half, const void *k_mont, void *cur_mont, int on_device);
/* DPBeta::compute_eq_tbl (src/prototools/mle.h:93-105), the table DPBeta::precomputeAll (mle.h:121-137) starts from;
 * 2^d entries, 1 <= d <= 30, eqbit(1, x) = x, eqbit(0, x) = 1 - x (mle.cc:12-15).
 *   variant 0 -- what the reference's loop computes: its doubling step reads dst[p >> 1], so every factor is selected by
 *                the TOP bit of p:  out[p] = prod_j (1 - r[j]) for p < 2^(d-1),  prod_j r[j] above.  Use this one to
 *                reproduce the reference's proofs.
 *   variant 1 -- the table the loop's comment describes:  out[p] = prod_{j < d} eqbit(bit j of p, r[j]).
 * The prover's first suffix table is then lsa_fr_scale_upper(out, 2^(d-1), rhoInvs[0], suff) (mle.h:132-137).
 * on_device != 0: r (d entries) and out are device pointers and the call is asynchronous on lsa_stream(); else host
 * pointers. */
int lsa_fr_eq_table(const void *r_mont, size_t d, int variant, void *out_mont, int on_device);

/* In-place radix-2 NTT of 2^log_n Fr values, natural order in and out: replaces libfqfft
 * basic_radix2_domain<Fr>::FFT / iFFT / cosetFFT / icosetFFT as used by the Lipmaa gadget
 * (src/gadgets/lipmaa.cc:68-81,102-175).  omega: a primitive 2^log_n-th root of unity (HOST, one
 * Fr; libff::get_root_of_unity).  inverse == 0: a[k] <- sum_i a[i] omega^(ik), after a[i] *= g^i
 * when coset_g != NULL (cosetFFT).  inverse != 0: the same with omega^-1, then a[k] *= 1/n and,
 * with coset_g, *= g^-k (iFFT / icosetFFT).  coset_g: HOST, one Fr, or NULL.
 * on_device != 0: a is a device pointer; else a host pointer.  log_n <= 28.
 * At most three passes over the data (csrc/ntt.hip); the twiddle tables of the last eight domains (log_n, omega,
 * direction; each up to one vector's size while that is at most LSA_NTT_T1_MB = 512 MB) and of the last eight coset
 * generators stay on the device, least recently used first out once they hold more than LSA_NTT_CACHE_MB (default
 * 2048) together; a second vector of the same size is kept as scratch. */
int lsa_fr_ntt(void *a_mont, size_t log_n, const void *omega_mont, int inverse, const void *coset_g_mont, int on_device);

/* The same four transforms on libfqfft's step_radix2_domain<Fr> of m = 2^big_log + 2^small_log points, small_log <
 * big_log <= 27: the domain libfqfft's get_evaluation_domain selects for every size that is not a power of two
 * (src/prototools/interp.h:62, src/gadgets/lipmaa.cc:102 with such an n) [upstream, recalled:
 * libfqfft/evaluation_domain/domains/step_radix2_domain.tcc].  Evaluation points: omega^(2k) for k < 2^big_log, then
 * omega sigma^j for j < 2^small_log, sigma = omega^(2^(big_log + 1 - small_log)).  a: m Fr values, in place, coefficients
 * <-> values in that order.  omega: a primitive 2^(big_log + 1)-th root of unity (HOST, one Fr: the domain's `omega`,
 * libff::get_root_of_unity(2^(big_log + 1))).  inverse / coset_g / on_device as for lsa_fr_ntt. */
int lsa_fr_ntt_step(void *a_mont, size_t big_log, size_t small_log, const void *omega_mont, int inverse, const void *coset_g_mont, int on_device);
/* Test and tool support, like lsa_ecntt_param: the state of the table cache the two calls above (and the quotient and the
 * witness map through them) share, and the budgets the process runs under.  0 for an unknown selector. */
#define LSA_FR_NTT_PARAM_RESIDENT_BYTES 0   /* -> bytes of twiddle and coset tables on the device now */
#define LSA_FR_NTT_PARAM_DOMAIN_TABLES 1    /* -> cached domains (log_n, omega, direction) */
#define LSA_FR_NTT_PARAM_COSET_TABLES 2     /* -> cached coset generators (log_n, g, direction) */
#define LSA_FR_NTT_PARAM_CACHE_BUDGET 3     /* -> LSA_NTT_CACHE_MB in bytes */
#define LSA_FR_NTT_PARAM_T1_BUDGET 4        /* -> LSA_NTT_T1_MB in bytes (the coset powers: a quarter of it) */
size_t lsa_fr_ntt_param(int which);

/* The Lipmaa Hadamard prover's quotient polynomial (CPHadL::prove, src/gadgets/lipmaa.cc:103-176: coefficients_for_H, the
 * scalar vector of its MSM) from the three committed vectors, all on the device:
 *     H = d2 A + d1 B - d3 + d1 d2 Z + (A B - C) / Z,       equivalently  H Z = (A + d1 Z)(B + d2 Z) - (C + d3 Z),
 * A, B, C the interpolants of a, b, c on the domain and Z the domain's monic vanishing polynomial.
 *   Domain: small_log < 0 -- the basic radix-2 domain, m = 2^big_log, 1 <= big_log <= 28, omega as for lsa_fr_ntt,
 *           Z = x^m - 1;  otherwise libfqfft's step radix-2 domain, m = 2^big_log + 2^small_log, omega and the limits as
 *           for lsa_fr_ntt_step, Z = (x^(2^big_log) - 1)(x^(2^small_log) - omega^(2^small_log)).
 *   a, b, c: n <= m values each on the domain's points in the domain's order; entries n .. m-1 count as zero (the
 *           reference's zero-filled vectors).  Not modified.  With n == 0 they are not read and may be null (an empty device
 *           tensor has no address).
 *   d123:   HOST, three Fr: the commitment randomness d1, d2, d3 of a, b, c.
 *   coset_g: HOST, one Fr: the coset on which the division by Z happens (the reference: Fr::multiplicative_generator).  A
 *           coset on which Z may vanish is refused before any device work: coset_g^m = 1 on the basic domain,
 *           coset_g^(2 * 2^big_log) = 1 on the step domain.
 *   h_out:  m + 1 Fr, lowest degree first; must not overlap the inputs.
 * NOTE: the reference fills aB from aPts (lipmaa.cc:121), so ITS proofs are those of this call with b == a; b is a
 * separate argument here.
 * Three iFFTs, three coset FFTs, one pointwise kernel, one inverse coset FFT (csrc/fr_poly.hip), on grow-only staging
 * owned by the library (two vectors, the transforms' scratch; for host callers a third): no allocation per call after
 * the first of a size.  Fr values are canonical, so the bytes are those of the reference's schedule.
 * on_device != 0: a, b, c, h_out are device pointers and the call is asynchronous on lsa_stream(), with no host
 * synchronisation inside: h_out can go straight to lsa_msm_run_async as the scalar vector.  (Two things the call shares
 * with lsa_fr_ntt do wait for the device when they happen: the first call of a larger size grows the staging, and a
 * domain whose twiddle tables were evicted from ntt.hip's cache frees the evicted ones -- a prover that keeps to its
 * sizes and domains meets neither after its first proof.)  Else host pointers and a
 * blocking call.  LSA_ERR_INVALID: null argument, n > m, big_log / small_log out of range, refused coset. */
int lsa_fr_hadamard_quotient(const void *a_mont, const void *b_mont, const void *c_mont, size_t n, size_t big_log, int small_log,
                             const void *omega_mont, const void *coset_g_mont, const void *d123_mont, void *h_out_mont, int on_device);

/* out[i] = L_i(t), i < m: evaluation_domain::evaluate_all_lagrange_polynomials(t) of the same two domains (the key
 * generator's row, src/prototools/interp.h:68-71); big_log, small_log, omega as above.  For t a point of the domain the
 * unit vector.  omega, t: HOST, one Fr each.  The m denominators are inverted in runs of consecutive elements, one run and
 * one field inversion per GPU lane (csrc/fr_batch_inv.h; 16 elements: the fastest of 8, 16 and 32 measured at m = 2^20 and
 * 2^20 + 2^19): no serial chain over the vector.
 * on_device != 0: out is a device pointer and the call is asynchronous on lsa_stream(); else a host pointer, blocking. */
int lsa_fr_lagrange(size_t big_log, int small_log, const void *omega_mont, const void *t_mont, void *out_mont, int on_device);

/* ---- element-wise algebra on Fr vectors: what a prover or key generator does between the calls above ----------------- */
/* Common to the five calls below.  Vectors are libff Montgomery words, 32 bytes each; any 256-bit word pattern, in a vector or
 * in a one-element argument, counts as its value mod r (no canonicalising step on load is needed for the products and sums:
 * the limb arithmetic of csrc/fr29.h takes any 256-bit pattern; lsa_fr_batch_inverse alone canonicalises every element,
 * because its zero test and its prefix chain need the canonical value).  Outputs are always canonical (< r): the bytes of the
 * reference's host loop.  The one-element arguments (scale, coeffs, base, first, x) are HOST pointers in both modes.
 * on_device != 0: the vector pointers are device pointers, 16-byte aligned, and the call is asynchronous on lsa_stream() with no
 * host synchronisation inside (any staging is grow-only and owned by the library: only the first call of a larger size waits
 * for the device).  Else host pointers and a blocking call.  n == 0 is LSA_OK without a launch.  An output vector may be
 * EXACTLY an input (out == a: in place; every GPU lane reads what it owns before it writes it); any other overlap is refused.
 * LSA_ERR_INVALID, before any device work: a null pointer with n > 0, a partial overlap, a misaligned device pointer, n * 32
 * overflowing size_t or n above 2^40, and the limits stated per call. */
/* out[i] = scale * a[i] * b[i]; scale == NULL: 1.  a == b is legal (squares).  The Hadamard witness c = a o b of
 * src/gadgets/hadamard.cc:130-135.  Two limb products per element (the second brings libff's form back and carries the scale). */
int lsa_fr_vec_mul(const void *a_mont, const void *b_mont, const void *scale_mont, size_t n, void *out_mont, int on_device);
/* out[i] = sum_{t<k} coeffs[t] * xs[t][i], 1 <= k <= LSA_FR_VEC_PARAM_LINCOMB_MAX (8).  xs: HOST array of k vector pointers (as
 * `tables` of lsa_fr_sumcheck_round); the same vector may appear twice; coeffs: k Fr.  Covers scale (mulByGamma, lipmaa.h:50-52),
 * add, sub (coefficients 1, r - 1), axpy, and the Groth16 key scalars (beta At + alpha Bt + Ct) / delta in one pass.  Four
 * products share one Montgomery reduction (csrc/fr_dot.h). */
int lsa_fr_vec_lincomb(const void *const *xs, const void *coeffs_mont, size_t k, size_t n, void *out_mont, int on_device);
/* out[i] = first * base^i, i < n; first == NULL: 1.  0^0 = 1.  The chiPows loop of lipmaa.h:98-102 is (base = chi, first = chi)
 * or (first = NULL, n = m + 1).  Runs of LSA_FR_VEC_PARAM_POWERS_RUN elements, one per GPU lane, each from its own starting power:
 * no chain across lanes. */
int lsa_fr_powers(const void *base_mont, const void *first_mont, size_t n, void *out_mont, int on_device);
/* out[i] = 1 / x[i]; an element that is 0 mod r (the words of 0, r, 2r, ... included) gives 0.  n_zero: HOST, may be NULL; receives
 * the number of such elements; in device mode a non-null n_zero makes the call blocking (as n_rejected of lsa_g1_decompress).
 * Runs of LSA_FR_VEC_PARAM_INV_RUN elements with one field inversion each (csrc/fr_batch_inv.h). */
int lsa_fr_batch_inverse(const void *x_mont, size_t n, void *out_mont, uint64_t *n_zero, int on_device);
/* out = sum_{i<n} coeffs[i] x^i (one Fr; 0 for n == 0; out must not overlap coeffs): PolyT::eval (polytools.h:92-100),
 * check_correctness (lipmaa.cc:43-58).  A GPU lane takes LSA_FR_VEC_PARAM_EVAL_ITEMS consecutive coefficients by Horner's rule;
 * workgroup sums, then a finishing kernel: no atomics on field elements, the same bytes whatever the order. */
int lsa_fr_poly_eval(const void *coeffs_mont, size_t n, const void *x_mont, void *out_mont, int on_device);
/* Test and tool support, like lsa_fr_matrix_param: the compiled shape of the five calls.  0 for an unknown selector. */
#define LSA_FR_VEC_PARAM_LINCOMB_MAX 0   /* -> vectors per lsa_fr_vec_lincomb call at most */
#define LSA_FR_VEC_PARAM_INV_RUN 1       /* -> elements per lane and inversion of lsa_fr_batch_inverse */
#define LSA_FR_VEC_PARAM_POWERS_RUN 2    /* -> elements per lane of lsa_fr_powers */
#define LSA_FR_VEC_PARAM_EVAL_ITEMS 3    /* -> coefficients per lane of lsa_fr_poly_eval */
#define LSA_FR_VEC_PARAM_PASS_ELEMS 4    /* -> elements one trip of the streaming kernels' grid-stride loop covers on the current device
                                          *    (grid x block x unroll; 0 before lsa_init) */
#define LSA_FR_VEC_PARAM_EVAL_BLOCK 5    /* -> coefficients per workgroup (and block partial) of lsa_fr_poly_eval */
size_t lsa_fr_vec_param(int which);

/* ---- Fr vectors as row-major matrices: the matrix-product gadget (CPMat / CPmmp, src/examples/matrixsc.cc) ---------- */
/* Weighted sums of the rows or of the columns of a rows x cols matrix M (row-major, M[r * cols + c]):
 *   side 0: out[c] = sum_r w[r] * M[r * cols + c]   (cols results; w has rows entries)
 *           -- the contraction in DPMatrixMle's constructor (src/prototools/mle.h:241-258, v[r] = sum_l A[(l << d) + r] eqTbl[l])
 *           with M = A, rows = cols = 2^d and w = the table of lsa_fr_eq_table(rho, d, 0);
 *   side 1: out[r] = sum_c M[r * cols + c] * w[c]   (rows results; w has cols entries).
 * Any dimensions; a summed dimension of zero gives zeros, no outputs is a successful no-op.  Inputs are libff Montgomery
 * words; the outputs are canonical (< r), so the bytes are those of the reference's loop whatever the order of summation
 * (csrc/fr_dot.h: four products per Montgomery reduction on 29-bit limbs).  M is read once; when the outputs alone cannot
 * fill the device the summed dimension is cut into lsa_fr_matvec_slices(rows, cols, side) slices and a finishing kernel
 * adds their partial sums (csrc/fr_matrix.hip).
 * on_device != 0: m, w, out are device pointers (16-byte aligned) and the call is asynchronous on lsa_stream(), with no host
 * synchronisation inside (the staging -- the limbs of w, the slices' partial sums -- is grow-only and owned by the library:
 * only the first call of a larger size waits for the device).  Else host pointers and a blocking call.
 * LSA_ERR_INVALID, before any device work: side not 0 or 1, rows * cols * 32 overflows size_t, a null pointer with a
 * non-empty extent, out overlapping m or w, a misaligned device pointer. */
int lsa_fr_matvec(const void *m_mont, size_t rows, size_t cols, const void *w_mont, int side, void *out_mont, int on_device);

/* C (rows_a x cols_b) = A (rows_a x inner) * B (inner x cols_b), all row-major: the witness of the matrix-product gadget
 * (the triple loop of src/examples/matrixsc.cc:83-91).  Any dimensions; inner == 0 gives zeros, an empty C is a successful
 * no-op.  Values, modes and refusals as for lsa_fr_matvec (c must not overlap a or b).  A workgroup owns a 32 x 32 tile of C
 * and stages the tiles of A and B in LDS as limbs, 16 of the summed dimension at a time; edge tiles are predicated, the
 * caller's buffers are never padded (csrc/fr_matrix.hip). */
int lsa_fr_matmul(const void *a_mont, const void *b_mont, size_t rows_a, size_t inner, size_t cols_b, void *c_mont, int on_device);

/* Test and tool support, not needed to use the two calls above: their compiled shape, so that tests and benchmarks follow a
 * retune.  `which` is one of the selectors below (the comment names the value returned); 0 for an unknown selector. */
#define LSA_FR_PARAM_MATMUL_TILE 0        /* -> edge of a workgroup's tile of C */
#define LSA_FR_PARAM_MATMUL_KSTEP 1       /* -> elements of the summed dimension staged per step */
#define LSA_FR_PARAM_DOT_MAX_PARTIALS 2   /* -> reduced partial sums added up before a product brings them back below 2r (csrc/fr_dot.h) */
#define LSA_FR_PARAM_DOT_GROUP 3          /* -> products per partial sum */
#define LSA_FR_PARAM_MATVEC_SMALL 4       /* -> lsa_fr_matvec: a matrix of at most this many elements is one workgroup's */
size_t lsa_fr_matrix_param(int which);
/* (Test and tool support.)  Slices of the summed dimension lsa_fr_matvec cuts a rows x cols matrix into: 1 = the kernel writes out itself, more =
 * partial sums and the finishing kernel.  0 for arguments the call refuses. */
size_t lsa_fr_matvec_slices(size_t rows, size_t cols, int side);

/* ---- sparse Fr matrices resident on the device: R1CS products and the QAP witness map (src/examples/legogrothmatrix.cc) ---- */
/* A sparse matrix over Fr kept on the device, made from host CSR arrays: vals_mont nnz x 32 bytes (libff Montgomery words; any
 * 256-bit pattern counts as its value mod r), cols nnz column indices, row_ptr nrows + 1 offsets (row r is the entries
 * row_ptr[r] .. row_ptr[r + 1] - 1).  Duplicate column indices inside a row are legal and summed (libsnark's linear combinations
 * are not merged); empty rows are legal.  keep_transpose != 0 also keeps the transposed copy (built on the host by a counting
 * sort), which side 0 of lsa_fr_sparse_matvec needs; it doubles the device memory of the handle.
 * Every stored coefficient gets a class here: exactly the canonical words of +1 or of -1 (r - 1), or general.  Units cost a limb
 * addition per entry instead of a product and their coefficient is never read (csrc/fr_sparse.h).
 * The arrays are copied: the caller's may go after the call.  Blocking.  *out is null after any failure.
 * LSA_ERR_INVALID, before any device work: row_ptr[0] != 0, a decreasing row_ptr, row_ptr[nrows] != nnz, a column index >= ncols,
 * a null pointer with a non-empty extent (or a null out), nrows or ncols above 2^32 - 1.  Because every index is checked here, no
 * kernel gathers out of bounds as long as x has the length the side says. */
typedef struct lsa_fr_sparse lsa_fr_sparse;
int lsa_fr_sparse_create(const void *vals_mont, const uint32_t *cols, const uint64_t *row_ptr, size_t nrows, size_t ncols, size_t nnz,
                         int keep_transpose, lsa_fr_sparse **out);
/* Waits for the library's stream (a product of the matrix may still be running), then frees the device copies.  Null: no-op. */
void lsa_fr_sparse_destroy(lsa_fr_sparse *m);
size_t lsa_fr_sparse_rows(const lsa_fr_sparse *m);
size_t lsa_fr_sparse_cols(const lsa_fr_sparse *m);
size_t lsa_fr_sparse_nnz(const lsa_fr_sparse *m);

/* side 1: out[r] = sum_c M[r][c] x[c] (nrows results; x has ncols entries); side 0: out[c] = sum_r x[r] M[r][c] (ncols results; x
 * has nrows entries; needs keep_transpose, else LSA_ERR_INVALID).  The sides are those of lsa_fr_matvec, and so are the bytes:
 * canonical words, whatever the order of summation.  An empty row gives zero; a matrix without entries gives zeros without a
 * launch over entries; no results is a successful no-op.
 * Work is cut by nonzeros: rows of at most LSA_FR_SPARSE_PARAM_SHORT_MAX entries are one lane's each (of at most _LANE_MAX
 * entries when the matrix has at least _LANE_FILL rows between the two: enough lanes for the whole device), longer rows are cut into
 * chunks of LSA_FR_SPARSE_PARAM_CHUNK entries, a wavefront each, and a finishing kernel adds a row's partial sums (csrc/fr_sparse.hip).
 * on_device != 0: x, out are device pointers (16-byte aligned) and the call is asynchronous on lsa_stream(), with no host
 * synchronisation inside (the staging -- the chunks' partial sums, x and out for host callers -- is grow-only and owned by the
 * library: only the first call of a larger size waits for the device).  Else host pointers and a blocking call.  x is not modified.
 * LSA_ERR_INVALID, before any device work: a null matrix, side not 0 or 1, side 0 without the transpose, a null pointer with a
 * non-empty extent, out overlapping x, a misaligned device pointer. */
int lsa_fr_sparse_matvec(const lsa_fr_sparse *m, const void *x_mont, int side, void *out_mont, int on_device);

/* H of the R1CS (A, B, C) at the assignment z (z[0] = 1): a = A z, b = B z, c = C z into library staging, then
 * lsa_fr_hadamard_quotient on them: H Z = (a + d1 Z)(b + d2 Z) - (c + d3 Z), libsnark's r1cs_to_qap_witness_map; with zero d123
 * Groth16's H.  n = the common row count <= m; big_log, small_log, omega, coset_g, d123, h_out (m + 1 Fr) and the refusals exactly
 * as documented for lsa_fr_hadamard_quotient; d123 == NULL: zeros.  z: as many Fr as the matrices have columns.
 * libsnark's extra input-consistency rows (one constraint 1 * z[i] = 0 appended to A per public input) need no special case:
 * they are ordinary rows of A with one unit entry and empty rows of B and C.
 * on_device != 0: z, h_out are device pointers (16-byte aligned), asynchronous on lsa_stream() as lsa_fr_hadamard_quotient is;
 * h_out can go straight to lsa_msm_run_async as the scalar vector.  Else host pointers, blocking.
 * LSA_ERR_INVALID also: a null matrix, differing row or column counts among A, B and C, more rows than the domain has points,
 * h_out overlapping z, a misaligned device pointer. */
int lsa_fr_qap_witness(const lsa_fr_sparse *A, const lsa_fr_sparse *B, const lsa_fr_sparse *C, const void *z_mont, size_t big_log,
                       int small_log, const void *omega_mont, const void *coset_g_mont, const void *d123_mont, void *h_out_mont, int on_device);

/* Test and tool support: the compiled shape of the sparse kernels, so that tests and benchmarks follow a retune.  0 for an
 * unknown selector. */
#define LSA_FR_SPARSE_PARAM_SHORT_MAX 0   /* -> entries up to which a row is summed by one lane */
#define LSA_FR_SPARSE_PARAM_CHUNK 1       /* -> entries of a longer row per wavefront and partial sum */
#define LSA_FR_SPARSE_PARAM_UNIT_MAX 2    /* -> +-1 terms the unit accumulator takes before it is joined (csrc/fr_sparse.h) */
#define LSA_FR_SPARSE_PARAM_LANE_MAX 3    /* -> entries up to which a row is one lane's when the matrix has LANE_FILL rows of SHORT_MAX + 1 .. LANE_MAX entries */
#define LSA_FR_SPARSE_PARAM_LANE_FILL 4   /* -> that number of rows */
size_t lsa_fr_sparse_param(int which);

/* ---- pairing ---------------------------------------------------------------------------- */
/* out[i] = miller_loop(precompute_G1(P_i), precompute_G2(Q_i)), i < n: replaces libff
 * alt_bn128_pp::precompute_G1 / precompute_G2 / miller_loop (src/utils/globl.h:96-102,
 * src/gadgets/subspace.cc:142-160, src/gadgets/poly.h:105-119).  P_i: libff G1 (96 B),
 * Q_i: libff G2 (192 B), out: n x Fq12 (384 B).  on_device != 0: all three are device
 * pointers, else host pointers. */
int lsa_miller_loop(const void *g1_jac, const void *g2_jac, size_t n, void *out_fq12, int on_device);
/* out = prod_i miller_loop(P_i, Q_i) (one Fq12, HOST): n = 2 is libff double_miller_loop
 * (src/gadgets/subspace.cc:147-163, src/gadgets/lipmaa.cc:187-207). Host pointers. */
int lsa_miller_loop_product(const void *g1_jac, const void *g2_jac, size_t n, void *out_fq12);
/* out = prod_i in[i] (one Fq12, HOST; 1 for n = 0): the GT/Fqk operator* chain of the verifiers
 * (src/gadgets/subspace.cc:163-166, src/gadgets/poly.h:108-110) and the fold of the per-GPU
 * partial products when a pairing batch is split across ranks.  Host pointers. */
int lsa_fq12_product(const void *in_fq12, size_t n, void *out_fq12);
/* out[i] = final_exponentiation(in[i]): replaces alt_bn128_pp::final_exponentiation
 * (src/utils/globl.h:103, src/gadgets/subspace.cc:166, src/gadgets/poly.h:110,122). */
int lsa_final_exponentiation(const void *in_fq12, size_t n, void *out_fq12, int on_device);
/* out = final_exponentiation(prod_i miller_loop(P_i, Q_i)) (one GT element, HOST).  n = 1 is
 * reduced_pairing (src/gadgets/subspace.cc:88-102,123-124); the batched form is the CPhad /
 * CPsc verifier shape (BASELINE.json configs[4]).  Host pointers.
 * Wherever a final exponentiation follows inside the library (this call, lsa_pairing_terms / _segments / _sharded with
 * final_exp) the Miller loops of pairs without a resident line table may walk the SIGNED digits of 6u + 2 (65 doubling and
 * 21 addition steps instead of 64 and 36): their Miller values differ from libff's by vertical lines, which the final
 * exponent kills, so every GT value returned is libff's bit for bit -- for every input: workgroups that hold a point at
 * infinity in G2 or a pair off its curve (where libff's loop is still defined, as the value of its formulas, and the identity
 * is not) keep libff's binary loop.  Raw Miller values (lsa_miller_loop*, final_exp == 0) always come from the binary loop.
 * Env LSA_MILLER_NAF=0 switches the signed-digit loop off. */
int lsa_pairing_product(const void *g1_jac, const void *g2_jac, size_t n, void *out_gt);

/* ---- G2 precomputation (libff G2_precomp) ------------------------------------------------- */
/* libff's alt_bn128_ate_G2_precomp as bytes: QX, QY (the affine point), then the coefficient triple
 * {ell_0, ell_VW, ell_VV} of each of the 102 steps of the ate loop (64 doublings, 36 additions, 2
 * Frobenius steps), 308 Fq2 of 64 B in libff's layout. */
#define LSA_ATE_NUM_COEFFS 102
#define LSA_G2_PRECOMP_BYTES ((2 + 3 * LSA_ATE_NUM_COEFFS) * 64)
size_t lsa_g2_precomp_bytes(void);   /* == LSA_G2_PRECOMP_BYTES */
/* out_precomp[i] = precompute_G2(Q_i), i < n: replaces libff alt_bn128_pp::precompute_G2 where the
 * reference keeps the result in a key and re-uses it in every verification (src/gadgets/subspace.cc:48,
 * 66-70: C_precomp, a_precomp; src/gadgets/lipmaa.h:95-96: gammazg2_precomp; src/gadgets/poly.h:97-98).
 * Q_i: libff G2 (192 B), out: n x LSA_G2_PRECOMP_BYTES.  Host pointers. */
int lsa_g2_precompute(const void *g2_jac, size_t n, void *out_precomp);
/* out[i] = miller_loop(precompute_G1(P_i), *q_precomp[i]), i < n, over precomputed G2 values
 * (src/gadgets/subspace.cc:152-166 verifyLin3or4, src/gadgets/lipmaa.cc:194-200): only the Fq12 chain
 * f <- f^2 * line(P) runs, 166 dependent rounds instead of 344.  q_precomp: n host pointers to
 * LSA_G2_PRECOMP_BYTES each (equal pointers / equal contents share one device table).  Host pointers. */
int lsa_miller_loop_precomp(const void *g1_jac, const void *const *q_precomp, size_t n, void *out_fq12);
/* The general form every pairing entry point is a shape of:
 *   out[j] = [final_exponentiation] ( prod_{i = seg_offsets[j]}^{seg_offsets[j+1]-1} m_i ),  j < nseg,
 *   m_i = miller_loop(P_i, Q_i), or its conjugate (libff unitary_inverse) when flags[i] & 1.
 * Q_i is *q_precomp[i] when q_precomp and q_precomp[i] are non-null, else the point g2_jac[i].
 * flags may be null (no conjugates).  A verifier's whole check
 *   final_exponentiation(lhs * rhs.unitary_inverse()) == GT::one()
 * (src/utils/globl.h:94-105, src/gadgets/subspace.cc:166, src/gadgets/lipmaa.cc:203, src/gadgets/poly.h:110,122)
 * is ONE product here: the pairs of a product share accumulators on the device, conjugated terms run as
 * Miller loops on -P (the same Fq12 element).  Host pointers. */
int lsa_pairing_terms(const void *g1_jac, const void *g2_jac, const void *const *q_precomp, const uint8_t *flags,
                      const uint64_t *seg_offsets, size_t nseg, void *out_fq12, int final_exp);
/* The device keeps one line table (22 KB) per distinct Q it has seen -- keyed by a 128-bit fingerprint of
 * the bytes passed (the 192-byte point, or the precomp blob) -- so that a CRS element costs its G2
 * arithmetic once.  max_tables: capacity (LRU; default 4096, env LSA_G2_TABLES); 0 turns the cache off
 * (every call recomputes its tables).  Calls with more than 1024 terms or device-resident points bypass
 * it.  stats: hits, misses, resident tables, evictions. */
int lsa_g2_table_cache(size_t max_tables);
/* Promises the tables of the points the cache does not hold yet and returns without waiting (they are built in one
 * launch when the next Miller call arrives, or earlier once LSA_G2_PREFETCH_BATCH = 60 of them are waiting): what
 * libff's precompute_G2 costs the caller when the result is only ever handed back to miller_loop
 * (src/gadgets/poly.h:116-118: precompute_G2(pts[i] * g2) inside a host loop).  Host pointer. */
int lsa_g2_tables_prefetch(const void *g2_jac, size_t n);
/* Pairs of one product that share an accumulator f <- f^2 * prod_i line_i (1..4; 0 = chosen from the
 * batch size: 1 up to 8192 terms, so that every pair has its own lanes while the chip is not full).
 * The value of a product does not depend on it. */
int lsa_pairing_set_chunk(unsigned pairs_per_accumulator);
int lsa_g2_table_cache_stats(uint64_t out[4]);

/* ---- multi-GPU: one process per GPU, one exchange step per MSM (RCCL over xGMI) --------------- */
/* libff's multi_exp splits [0, n) into `chunks` contiguous ranges, runs multi_exp_inner on each
 * and sums the partials; multiExpMA forwards `chunks` (src/utils/globl.h:67-77).  Here a chunk is
 * a GPU and a rank is a process: every rank runs the single-GPU pipeline on its slice and the
 * 96-byte (G1) / 192-byte (G2) Jacobian partials are combined with ONE ncclAllGather + a sum in
 * rank order (RCCL has no elliptic-curve reduce op).  Every rank ends up with the same point.
 *
 * lsa_comm_unique_id: rank 0 fills 128 bytes (an ncclUniqueId) that the caller distributes to
 * the other ranks over its own transport (MPI, a torch.distributed broadcast, a file ...).
 * lsa_comm_init: collective over all ranks; binds the communicator to the device of lsa_init.
 * lsa_comm_init_file: single-node bootstrap without a transport: rank 0 writes the id to `path`,
 * the others poll for it (timeout_s <= 0: 60 s).  The file must not exist beforehand. */
#define LSA_COMM_ID_BYTES 128
int lsa_comm_unique_id(void *out_id128);
int lsa_comm_init(int rank, int world, const void *id128);
int lsa_comm_init_file(int rank, int world, const char *path, int timeout_s);
void lsa_comm_destroy(void);
int lsa_comm_rank(void);    /* 0 without a communicator */
int lsa_comm_world(void);   /* 1 without a communicator */
/* libff's chunk split: one = n / world, the last rank takes the remainder (n < world: rank 0
 * takes everything).  The range of (base, scalar) pairs rank `rank` owns. */
void lsa_shard_range(size_t n, int world, int rank, size_t *lo, size_t *hi);
/* This rank's part of a sharded MSM over its resident bases[first .. first+n) (device scalars),
 * then the exchange step on an internal side stream; d_out_jac (DEVICE) receives the sum over
 * all ranks.  Asynchronous: lsa_stream() may start the next call's front meanwhile;
 * lsa_comm_join() orders every exchange issued so far on lsa_stream(). */
int lsa_msm_run_sharded_async(const lsa_bases *bases, size_t first, const void *d_scalars_mont, size_t n, void *d_out_jac);
int lsa_comm_join(void);
/* The same, blocking, result in a HOST buffer. */
int lsa_msm_run_sharded(const lsa_bases *bases, size_t first, const void *d_scalars_mont, size_t n, void *out_jac);
/* multiExpMA for an SPMD prover: every rank passes ITS slice of the vectors (host buffers, the
 * range lsa_shard_range gives it; the CRS cache applies) and receives the sum over all ranks.
 * Without a communicator (world 1) identical to lsa_g1_msm / lsa_g2_msm. */
int lsa_g1_msm_sharded(const void *bases_jac, const void *scalars_mont, size_t n_local, void *out_jac);
int lsa_g2_msm_sharded(const void *bases_jac, const void *scalars_mont, size_t n_local, void *out_jac);
/* final_exponentiation(prod over all ranks' pairs): per-rank Miller product, all-gather of the
 * 384-byte Fq12 partials, product in rank order, one final exponentiation on every rank. */
int lsa_pairing_product_sharded(const void *g1_jac, const void *g2_jac, size_t n_local, void *out_gt);
/* Building block: all-gather of one device-resident partial per rank (kind 1: G1 point, 2: G2
 * point, 12: Fq12) into d_gathered (world x the same), ordered on lsa_stream(). */
int lsa_comm_all_gather(const void *d_partial, void *d_gathered, int kind);

/* Many independent pairing products in one pass -- a verifier's shape (CPPoly::verify,
 * src/gadgets/poly.h:105-122: d products of two or three Miller values, each followed by a final
 * exponentiation; CPhad verify at d = 20: 181 Miller loops in 62 products):
 *   out[j] = [final_exponentiation] ( prod_{i = seg_offsets[j]}^{seg_offsets[j+1]-1} miller_loop(P_i, Q_i) ),  j < nseg
 * (Fq12 one for an empty segment).  seg_offsets: nseg + 1 non-decreasing offsets, the first 0.
 * One upload, one Miller launch over all pairs, one product workgroup per segment, one batched
 * final exponentiation, one download.  final_exp == 0 leaves the Miller products
 * (double_miller_loop values).  Host pointers. */
int lsa_pairing_product_segments(const void *g1_jac, const void *g2_jac, const uint64_t *seg_offsets, size_t nseg, void *out_gt, int final_exp);

/* ---- point helpers ------------------------------------------------------------------- */
/* Jacobian -> libff "special" form (affine with Z = 1, or (0,1,0)), n points, host
 * buffers; replaces G::to_affine_coordinates()/batch_to_special on result vectors. */
int lsa_g1_normalize(const void *in_jac, size_t n, void *out_jac);
int lsa_g2_normalize(const void *in_jac, size_t n, void *out_jac);

/* ---- loading and writing keys ---------------------------------------------------------- */
/* Batch forms of what libff's operator>> / operator<< do per point (compressed format: is_zero, X, one bit of Y), plus the
 * checks they leave out: the range of the words, the curve equation of uncompressed points, membership in G2.
 *
 * Layouts.  x_mont: libff words of X, Montgomery form (32 B for G1, 64 B = c0, c1 for G2).  flags: one byte per point, bit 0 =
 * libff's Y_lsb (the parity of the canonical Y; of Y.c0 for G2), bit 1 = is_zero.  Points are libff Jacobian (96 B / 192 B).
 * status: one byte per point, below; a call returns LSA_OK whatever the statuses are.  Precedence: MALFORMED before NOT_ON_CURVE
 * before NOT_IN_SUBGROUP. */
#define LSA_PT_OK              0
#define LSA_PT_INFINITY        1   /* accepted: the flag says zero / Z == 0 */
#define LSA_PT_MALFORMED       2   /* a coordinate's words spell a value >= p, or a flag byte has a bit other than 0, 1 set */
#define LSA_PT_NOT_ON_CURVE    3
#define LSA_PT_NOT_IN_SUBGROUP 4   /* G2 only */
/* out_jac[i] = (X, Y, one), Y the root of X^3 + b whose parity equals bit 0 -- the point libff's operator>> returns.  (G2: a
 * root with c0 == 0 exists only when X^3 + b' lies in Fq and is a non-residue there; both roots then have parity 0, and the result
 * is (0, r2) for bit 0 == 0 and (0, p - r2) for bit 0 == 1, r2 = (-rhs.c0)^((p+1)/4); libff accepts that mismatch silently, so
 * does this call.)  With is_zero set X is ignored, as libff ignores it: (0, 1, 0), LSA_PT_INFINITY.  A point with status >= 2 is
 * written as (0, 1, 0): a caller who ignores the status never feeds an off-curve point to an MSM.  check_subgroup != 0 (G2):
 * points on the twist are tested with psi(P) == [6u^2]P, which holds exactly on G2 (csrc/fq_sqrt.h) -- 127 doublings and 39
 * additions per point, in a kernel of its own.
 * n_rejected: a HOST pointer, may be NULL; receives the number of statuses >= 2.  on_device != 0: every other pointer is a device
 * pointer, and with n_rejected == NULL the call is asynchronous on lsa_stream(); with n_rejected it blocks.  Host mode blocks.
 * LSA_ERR_INVALID, before any device work: a null pointer with n > 0, an output that overlaps an input (or the other output), a
 * byte count that overflows size_t.  n == 0 is LSA_OK (*n_rejected = 0). */
int lsa_g1_decompress(const void *x_mont, const uint8_t *flags, size_t n, void *out_jac, uint8_t *status, uint64_t *n_rejected, int on_device);
int lsa_g2_decompress(const void *x_mont, const uint8_t *flags, size_t n, int check_subgroup, void *out_jac, uint8_t *status, uint64_t *n_rejected, int on_device);
/* The checks alone, on Jacobian points (any Z; what arrives under NO_PT_COMPRESSION): words >= p in any coordinate give
 * LSA_PT_MALFORMED, then Z == 0 gives LSA_PT_INFINITY, any other point is tested with Y^2 = X^3 + b Z^6 and, for G2 when asked
 * for, the subgroup test.  The points are not modified.  Modes and refusals as above. */
int lsa_g1_validate(const void *pts_jac, size_t n, uint8_t *status, uint64_t *n_rejected, int on_device);
int lsa_g2_validate(const void *pts_jac, size_t n, int check_subgroup, uint8_t *status, uint64_t *n_rejected, int on_device);
/* Jacobian -> compressed form, VALID points assumed: x_mont[i] = the canonical affine X in Montgomery words, flags as above.
 * Infinity: X = 0 and flags = 3 (libff prints its zero() = (0, 1, 0): is_zero set, and Y = 1 is odd).  One batch inversion per
 * eight points.  on_device != 0: device pointers, asynchronous on lsa_stream().  Refusals as above. */
int lsa_g1_compress(const void *pts_jac, size_t n, void *x_mont, uint8_t *flags, int on_device);
int lsa_g2_compress(const void *pts_jac, size_t n, void *x_mont, uint8_t *flags, int on_device);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
