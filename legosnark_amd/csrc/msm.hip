// legosnark_amd/csrc/msm.hip -- variable-base multi-scalar multiplication on gfx950.
//
// Replaces libff::multi_exp_with_mixed_addition / multi_exp<BDLO12> as called by
// multiExpMA (/root/reference/src/utils/globl.h:63-78) and sparsemexp
// (/root/reference/src/utils/sparsemexp.h:58,89).  Same sum, different schedule:
//
//   1 digits     scalars (Montgomery Fr, 32 B, coalesced) -> canonical -> signed c-bit digits,
//                recomputed by both sort passes instead of stored.  Resident bases with
//                pre-shifted copies (the usual case, "wide" path below): per tile of 2048 scalars
//                a histogram of 768 population-balanced bucket segments in LDS; plain path: per
//                (tile of 32768 scalars, window) a bucket histogram in LDS that ranks every entry.
//                A prefix over the tiles gives populations and run starts.  No global atomics.
//   2/3 sort     wide path: k_partition stages a tile's records per segment in LDS and copies
//                them out as whole runs; k_fine_sort_part (one workgroup per segment) orders a
//                segment in LDS from registers and writes it out linearly, with the per-bucket
//                populations and offsets.  Plain path: exclusive scan over the bucket populations,
//                then entry (point index | sign) written to offs[bucket] + tile_base + rank.
//   3b order     buckets ordered by population (largest first) so a wavefront's 64 lanes
//                walk equally long lists.
//   4 accumulate one lane per bucket walks its entry list, gathers 64-B affine points
//                and accumulates in XYZZ (8M+2S mixed add, 29-bit limbs for G1) -- the
//                dominant kernel.  Buckets above a population threshold are split across
//                workgroups (skewed scalars, e.g. the u[i]=i inputs of
//                /root/reference/src/examples/hadamard.cc:130-135).
//   5 reduce     sum_b (b+1)*S_b per window: per-lane running sums over L buckets,
//                then wavefront suffix-scan + tree reductions with cross-lane shuffles.
//   6 fold       Horner over the windows (c doublings + 1 add each) -> one Jacobian point;
//                for G1 each point is shared by a quad of lanes (quad29.h).
//
// Signed digits halve the bucket count (2^(c-1)); the zero/one filter of libff's
// multi_exp_with_mixed_addition needs no special case (0 contributes nothing, 1 lands in
// bucket 1 of window 0) and gives the same group element.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <type_traits>
#include <vector>

#include "curves.h"
#include "msm.h"
#include "msm_plan.h"
#include "msm_slots.h"
// The kernels, stage by stage.  This file stays the only one that compiles them: one code object, which msm_warmup loads
// with its one k_publish launch.
#include "msm_bases.h"         // 0       k_normalize, k_convert_bases, k_prepare_g1/g2, k_shift_window
#include "msm_sort.h"          // 1-3     k_digits .. k_fine_sort
#include "msm_accumulate.h"    // 3b, 4   k_size_*, k_accumulate*, k_heavy_plan, k_accumulate_heavy, k_heavy_finish
#include "msm_reduce.h"        // 5, 6    k_reduce*, k_fold_quad*, k_emit_*, k_reduce_bits_*, k_publish

namespace lsa {

// (window choice, tile sizes, SegList, CoarseMap and every other size the host derives: msm_plan.h)

// ------------------------------------------------------------------------------------
// host orchestration
// ------------------------------------------------------------------------------------
static Workspace g_ws;        // front phase (digits .. accumulate): reused by every call, ordered on the caller's stream
static Workspace g_prep_ws;   // prepare_bases staging

// Per-stage HIP events on the library stream.  A ring of EV_POOL call slots so that
// profiling never synchronises inside the timed loop; msm_profile_last() harvests.
static constexpr int EV_POOL = 64;
static constexpr int EV_MARKS = 8;   // 0..3 sort stage (caller's stream), 4..5 accumulate kernels (internal stream), 6..7 tail
static hipEvent_t g_ev[EV_POOL][EV_MARKS];
static bool g_ev_ready = false;
static bool g_profile = false;
static int g_ev_calls = 0;

void msm_release_workspace() {
    msm_slots_release();
    g_ws.release();
    g_prep_ws.release();
    if (g_ev_ready) { for (auto &row : g_ev) for (auto &e : row) (void)hipEventDestroy(e); g_ev_ready = false; }
}
void msm_profile_enable(bool on) { g_profile = on; g_ev_calls = 0; }
// Average per-stage milliseconds over the (up to EV_POOL) MSM calls recorded since
// profiling was enabled; returns the number of calls averaged.
int msm_profile_last(float ms[LSA_MSM_STAGES]) {
    for (int s = 0; s < LSA_MSM_STAGES; s++) ms[s] = 0.f;
    int cnt = g_ev_calls < EV_POOL ? g_ev_calls : EV_POOL;
    if (!g_ev_ready || cnt == 0) return 0;
    for (int c = 0; c < cnt; c++) {
        if (hipEventSynchronize(g_ev[c][EV_MARKS - 1]) != hipSuccess) return 0;
        // stage -> (from mark, to mark); stage 6 = hand-over from the sort to the accumulate kernel
        // (waiting for the previous call's accumulate + ordering the buckets by population)
        static const int span[7][2] = {{0, 1}, {1, 2}, {2, 3}, {4, 5}, {5, 6}, {6, 7}, {3, 4}};
        for (int s = 0; s < 7; s++) { float t = 0.f; (void)hipEventElapsedTime(&t, g_ev[c][span[s][0]], g_ev[c][span[s][1]]); ms[s] += t; }
        float t = 0.f; (void)hipEventElapsedTime(&t, g_ev[c][0], g_ev[c][EV_MARKS - 1]); ms[7] += t;
    }
    for (int s = 0; s < LSA_MSM_STAGES; s++) ms[s] /= (float)cnt;
    return cnt;
}

static int msm_func_attrs() {
    static bool lds_attr_set = false;
    if (!lds_attr_set) {   // > 64 KiB of dynamic LDS needs an explicit opt-in (the limits: msm_plan.h, where plan_pipeline's requests are checked against them)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_scatter), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX_BIN_WORDS));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_scatter_wide<0>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX_BIN_WORDS));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_scatter_wide<1>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX_BIN_WORDS));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_scatter_wide<2>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX_BIN_WORDS));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_rank), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX_BIN_HALVES));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_hist_wide), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX_BIN_HALVES));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_partition), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX_PARTITION));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fine_sort_part), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX_FINE_SORT_PART));
        lds_attr_set = true;
    }
    return LSA_OK;
}

// What the first MSM of a process used to pay inside its own call (17-20 ms whatever its size: the library's code object
// loaded on the first kernel launch, eight streams and their events, the function attributes, the first workspace
// allocations) is paid by lsa_init instead -- a prover's init_public_params(), not its first multiExpMA.  The workspaces
// are sized for the first G1 and G2 MSMs of 2^20 pairs: 400 MB of front workspace + 360 MB for tail slot 0 here, 34 + 202 MB of
// staging in capi.hip (warm_stage_buffers) -- about 1 GB of the 288 GB per process; LSA_WARM=0 skips all of it (everything
// is then allocated by the first call that needs it), LSA_WARM_MB sets the size for processes that share a GPU or never see
// 2^20 pairs (a verifier, a check program: LSA_WARM_MB=16).
bool msm_warm_mb(size_t *mb) {
    const char *w = getenv("LSA_WARM"), *m = getenv("LSA_WARM_MB");
    *mb = m ? (size_t)atoll(m) : 400;
    return !(w && w[0] == '0');
}
int msm_warmup(hipStream_t st) {
    size_t warm_mb = 0;
    if (!msm_warm_mb(&warm_mb)) return LSA_OK;
    int rc = msm_slots_ready();
    if (rc) return rc;
    rc = msm_func_attrs();
    if (rc) return rc;
    // Workspaces for the first calls of a process at the BASELINE scale (2^20 pairs, G1 and G2, plain layout and copies):
    // the front workspace and tail slot 0 as large as those calls need (377 MB / 343 MB, LSA_TRACE=2 prints every growth),
    // so that a prover's first multiExpMA does not start with hipFree + hipMalloc pairs -- 0.5 ms each on one box, 10 ms and
    // more on another (the first G2 MSM of a process: 11.6 ms on a good box with them, 26 ms of them on a slow one).
    // One tail slot: a caller that only ever blocks -- the reference's provers and verifiers -- never leaves slot 0; queued
    // callers grow the other slots on first use.  LSA_WARM_MB=m: front = m MB, tail = 0.9 m (0: nothing).
    const size_t front = warm_mb << 20, tailb = front / 10 * 9;
    if (front) {
        // (no memory: the first call that needs the workspace will say so; LSA_TRACE reports it here)
        if (g_ws.ensure(front) != 0) { (void)hipGetLastError(); if (getenv("LSA_TRACE")) fprintf(stderr, "[lsa]   warm-up: front workspace of %zu MB not allocated\n", front >> 20); }
        if (msm_slots_warm(tailb) != 0) { (void)hipGetLastError(); if (getenv("LSA_TRACE")) fprintf(stderr, "[lsa]   warm-up: tail workspace of %zu MB not allocated\n", tailb >> 20); }
    }
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, st, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u);      // loads the code object
    for (int i = 0; i < MSM_NTAIL; i++)
        if (hipStream_t ts = msm_slot_stream(i)) hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, ts, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u);
    HIPCHK(hipDeviceSynchronize());
    return LSA_OK;
}

size_t msm_base_bytes(int group) { return group == 1 ? sizeof(CurveG1::Base) : sizeof(CurveG2::Base); }

// Jacobian (libff layout, device) -> device-resident bases of the curve's pipeline:
// batch-normalise to affine, then convert to the curve's base format.
template <class F>
int prepare_bases(const Jac<F> *d_in, void *d_out, size_t n, hipStream_t st) {
    using C = typename CurveOf<F>::type;
    if (n == 0) return LSA_OK;
    constexpr int K = 8;
    size_t threads = (n + K - 1) / K;
    unsigned blocks = (unsigned)((threads + 255) / 256);
    if (std::is_same<typename C::Base, Aff<F>>::value) {
        hipLaunchKernelGGL((k_normalize<F, K>), dim3(blocks), dim3(256), 0, st, d_in, (Aff<F> *)d_out, n);
        HIPCHK(hipGetLastError());
        return LSA_OK;
    }
    if constexpr (std::is_same<F, Fq>::value) {
        constexpr int KG = 16;                               // points per inversion (16 x 9 registers of prefix products)
        const unsigned gblocks = (unsigned)(((n + KG - 1) / KG + 255) / 256);
        hipLaunchKernelGGL((k_prepare_g1<KG>), dim3(gblocks), dim3(256), 0, st, d_in, (AffPacked *)d_out, n);
        HIPCHK(hipGetLastError());
        return LSA_OK;
    }
    if constexpr (std::is_same<F, Fq2>::value) {
        static const bool old_path = getenv("LSA_G2_PREPARE_OLD") != nullptr;      // A/B: k_normalize + k_convert_bases
        if (!old_path) {
            constexpr int KG = 4;
            const unsigned gblocks = (unsigned)(((n + KG - 1) / KG + 255) / 256);
            hipLaunchKernelGGL((k_prepare_g2<KG>), dim3(gblocks), dim3(256), 0, st, d_in, (AffPackedG2 *)d_out, n);
            HIPCHK(hipGetLastError());
            return LSA_OK;
        }
    }
    // staging buffer for the normalised affine points: grow-only, reused across calls
    // (every user is ordered on the same stream)
    if (g_prep_ws.ensure(n * sizeof(Aff<F>)) != 0) { set_error("prepare_bases: staging allocation failed"); return LSA_ERR_NOMEM; }
    Aff<F> *tmp = (Aff<F> *)g_prep_ws.ptr;
    hipLaunchKernelGGL((k_normalize<F, K>), dim3(blocks), dim3(256), 0, st, d_in, tmp, n);
    hipLaunchKernelGGL((k_convert_bases<C>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tmp, (typename C::Base *)d_out, n);
    HIPCHK(hipGetLastError());
    return LSA_OK;
}
template int prepare_bases<Fq>(const Jac<Fq> *, void *, size_t, hipStream_t);
template int prepare_bases<Fq2>(const Jac<Fq2> *, void *, size_t, hipStream_t);

template <class F>
int normalize_to_affine(const Jac<F> *d_in, Aff<F> *d_out, size_t n, hipStream_t st) {
    if (n == 0) return LSA_OK;
    constexpr int K = 8;
    size_t threads = (n + K - 1) / K;
    unsigned blocks = (unsigned)((threads + 255) / 256);
    hipLaunchKernelGGL((k_normalize<F, K>), dim3(blocks), dim3(256), 0, st, d_in, d_out, n);
    HIPCHK(hipGetLastError());
    return LSA_OK;
}
template int normalize_to_affine<Fq>(const Jac<Fq> *, Aff<Fq> *, size_t, hipStream_t);
template int normalize_to_affine<Fq2>(const Jac<Fq2> *, Aff<Fq2> *, size_t, hipStream_t);

// ------------------------------------------------------------------------------------
// Wide windows over pre-shifted bases.  A resident CRS can carry, next to P_i, the multiples
// 2^(pos_j) * P_i for 26 (24) bit positions pos_j (window-major: entry j*N + i; table_grid()).
// A digit that starts at pos_j gathers from copy j, so a digit d of ANY window is "add d * (its
// copy's point)": all windows share ONE bucket space in which bucket b has weight b+1.
// Consequences:
//   * the digit width is no longer tied to the per-window bucket count.  Large inputs
//     (n >= 2^16) use every other position: 13 (12) digits of 20/19 (22/21) bits per scalar instead
//     of 16 -- 13 mixed additions per pair -- and no GLV (its only gain, fewer windows to reduce
//     and fold, is moot), so no beta-multiplications either: 130 field products per pair instead
//     of 168.  Smaller inputs use every position: 26 digits, but only 512 (1024) buckets to reduce.
//   * one reduction over 2^(c-1) buckets instead of nwin reductions, and no Horner fold
//     (c*(nwin-1) sequential doublings: 0.3 ms G1 / 1.8 ms G2 of pure latency).
//   * several independent MSMs over prefixes of the same bases (CPPoly::prove's ladder,
//     /root/reference/src/gadgets/poly.h:77-86) run as ONE pass: segment j owns the bins
//     [j*B, (j+1)*B) of one sorted entry array (msm_segments_device).
// Price: 26 (24) x the base memory (G1 64 B, G2 128 B per point and copy) and one pass of 255
// doublings + 25 batch normalisations per key.
// ------------------------------------------------------------------------------------
// The switches of the plan (msm_plan.h: MsmSwitches), read from the environment once per process.
static MsmSwitches &switches() {
    static MsmSwitches sw = [] {
        const auto is_one = [](const char *name) { const char *e = getenv(name); return e && e[0] == '1'; };
        MsmSwitches v;
        v.no_rec32 = getenv("LSA_NO_REC32") != nullptr;
        v.no_part = getenv("LSA_NO_PART") != nullptr;
        if (const char *e = getenv("LSA_WIDE_SPLIT")) v.wide_split = (uint32_t)atoi(e);
        v.g2_pair = is_one("LSA_G2_PAIR");
        v.no_reduce_bits = getenv("LSA_NO_REDUCE_BITS") != nullptr;
        v.no_lane_l1 = getenv("LSA_NO_LANE_L1") != nullptr;
        v.g2_lane_l1 = is_one("LSA_G2_LANE_L1");
        if (const char *e = getenv("LSA_WIDE_BIG_MIN")) v.wide_big_min = (size_t)atoll(e);
        return v;
    }();
    return sw;
}
unsigned msm_table_windows(int /*group*/, size_t n) { return table_copies(n); }

static size_t g_merge_min = 0;
static bool g_merge_min_explicit = false;
// n != 0: vectors of at least n points get the copies and MSMs of at least n pairs use them;
// 0: defaults (copies from LSA_PRECOMPUTE_MIN / 2^19 points on, used by MSMs of every size)
void msm_set_merge_min(size_t n) {
    g_merge_min = n;
    g_merge_min_explicit = n != 0;
    switches().table_use_min = n ? n : 1;
}
size_t msm_merge_min() {
    if (g_merge_min == 0) {
        const char *e = getenv("LSA_PRECOMPUTE_MIN");
        g_merge_min = e && atoll(e) > 0 ? (size_t)atoll(e) : (size_t)1 << 19;
    }
    return g_merge_min;
}
bool msm_merge_min_is_explicit() { return g_merge_min_explicit; }
bool msm_precompute_off() { const char *pe = getenv("LSA_PRECOMPUTE"); return pe && pe[0] == '0'; }
// whether an MSM of n pairs on a handle that carries the copies runs over them (the wide-window pipeline)
bool msm_uses_table(size_t n) { return n >= switches().table_use_min; }

// d_table: msm_table_windows(group, n) * n entries, copy 0 (= the bases) already filled.
template <class F>
int precompute_windows(void *d_table, size_t n, hipStream_t st) {
    using C = typename CurveOf<F>::type;
    if (n == 0) return LSA_OK;
    const TableGrid grid = table_grid(n);
    Jac<F> *tmp = nullptr;
    if (hipMalloc(&tmp, n * sizeof(Jac<F>)) != hipSuccess) { set_error("precompute_windows: hipMalloc failed"); return LSA_ERR_NOMEM; }
    typename C::Base *tbl = (typename C::Base *)d_table;
    int rc = LSA_OK;
    for (unsigned k = 1; k < grid.ncopies && !rc; k++) {
        hipLaunchKernelGGL((k_shift_window<C>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tbl + (size_t)(k - 1) * n, tmp, n, grid.pos[k] - grid.pos[k - 1]);
        rc = prepare_bases<F>(tmp, tbl + (size_t)k * n, n, st);
    }
    hipError_t e = hipStreamSynchronize(st);
    (void)hipFree(tmp);
    if (rc) return rc;
    if (e != hipSuccess) { set_error("precompute_windows: %s", hipGetErrorString(e)); return LSA_ERR_HIP; }
    return LSA_OK;
}
// One copy of the same: copy k (1 <= k < msm_table_windows) from copy k - 1, no allocation, no synchronisation; d_tmp
// holds n Jacobian points.  The background builder of the CRS cache issues the copies one at a time.
template <class F>
int precompute_window_step(void *d_table, size_t n, void *d_tmp, unsigned k, hipStream_t st) {
    using C = typename CurveOf<F>::type;
    const TableGrid grid = table_grid(n);
    if (n == 0 || k == 0 || k >= grid.ncopies) return LSA_OK;
    typename C::Base *tbl = (typename C::Base *)d_table;
    hipLaunchKernelGGL((k_shift_window<C>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tbl + (size_t)(k - 1) * n, (Jac<F> *)d_tmp, n, grid.pos[k] - grid.pos[k - 1]);
    return prepare_bases<F>((const Jac<F> *)d_tmp, tbl + (size_t)k * n, n, st);
}
template int precompute_window_step<Fq>(void *, size_t, void *, unsigned, hipStream_t);
template int precompute_window_step<Fq2>(void *, size_t, void *, unsigned, hipStream_t);
template int precompute_windows<Fq>(void *, size_t, hipStream_t);
template int precompute_windows<Fq2>(void *, size_t, hipStream_t);

// field multiplications per point-scalar pair in the accumulate kernel (bench.py's VALU roofline)
unsigned msm_field_mults_per_pair(size_t n, size_t table_n) {
    if (table_n && n >= switches().table_use_min) return wide_plan(table_n, n, 1, switches()).nwin * 10;   // mixed XYZZ addition: 8M + 2S
    return 16 * 10 + 8;                                                                // 16 additions + 8 beta-multiplications (GLV)
}

// ------------------------------------------------------------------------------------
// The general pipeline.  plan_pipeline (msm_plan.h) decides everything a call's shape decides; msm_pipeline
// gets the workspaces and the slot, binds the pointers and issues the three stages below.
// ------------------------------------------------------------------------------------
// The buffers of one call, bound in one place from the plan's two layouts.
template <class A>
struct MsmBuffers {
    // front workspace (g_ws): sort and accumulate, reused by every call, ordered on the caller's stream
    uint32_t *hist, *heavy_count, *offs, *bsum, *bin_count, *bin_start, *bin_cursor, *perm;
    int32_t *digits;
    uint16_t *rank, *tile_hist;
    uint32_t *tile_base, *entries, *heavy_list, *chunk_off;
    A *hpart;
    void *recs;                      // coarse-sorted records, u32 or u64
    uint32_t *hist_c, *offs_c;       // populations and offsets of the first pass's bins
    // the slot's workspace: what the tail reads
    A *buckets, *wave_out, *window_sums;
    void *res;                       // Jac[nseg]

    MsmBuffers(const PipelinePlan &p, void *front_ws, void *tail_ws) {
        char *ws = (char *)front_ws, *tws = (char *)tail_ws;
        hist = (uint32_t *)(ws + p.front[F_HIST]);
        heavy_count = hist + p.nb;
        offs = (uint32_t *)(ws + p.front[F_OFFS]);
        bsum = (uint32_t *)(ws + p.front[F_BSUM]);
        bin_count = (uint32_t *)(ws + p.front[F_BINS]);
        bin_start = bin_count + SIZE_BINS;
        bin_cursor = bin_start + SIZE_BINS;
        perm = (uint32_t *)(ws + p.front[F_PERM]);
        digits = (int32_t *)(ws + p.front[F_DIGITS]);
        rank = (uint16_t *)(ws + p.front[F_RANK]);
        tile_hist = (uint16_t *)(ws + p.front[F_THIST]);
        tile_base = (uint32_t *)(ws + p.front[F_TBASE]);
        entries = (uint32_t *)(ws + p.front[F_ENTRIES]);
        heavy_list = (uint32_t *)(ws + p.front[F_HEAVY]);
        chunk_off = (uint32_t *)(ws + p.front[F_CHOFF]);
        hpart = (A *)(ws + p.front[F_HPART]);
        recs = ws + p.front[F_RECS];
        hist_c = p.fine ? (uint32_t *)(ws + p.front[F_CHIST]) : hist;       // one pass: the bins ARE the buckets
        offs_c = p.fine ? (uint32_t *)(ws + p.front[F_COFFS]) : offs;
        buckets = (A *)(tws + p.tail[T_BUCKETS]);
        wave_out = (A *)(tws + p.tail[T_WAVE]);
        window_sums = (A *)(tws + p.tail[T_WIN]);
        res = tws + p.tail[T_RES];
    }
};

// The call's row of profiling events (EV_MARKS of them), null when profiling is off.
struct Marks {
    hipEvent_t *ev;
    void operator()(int i, hipStream_t s) const { if (ev) (void)hipEventRecord(ev[i], s); }
};

// ---- sort stage (marks 1..3): entries ordered by bucket, populations in hist, offsets in offs
template <class C>
static void launch_sort(const PipelinePlan &p, const MsmBuffers<typename C::Acc> &b, const Fr *d_scalars, const SegList &segs, hipStream_t st,
                        const Marks &mark) {
    const size_t n = p.n;
    if (p.wide) {
        hipLaunchKernelGGL(k_hist_wide, dim3(p.wtiles), dim3(1024), p.lds_hist_wide, st, d_scalars, n, segs, p.pl, p.B, p.Bc, p.cm, p.pitch, p.wtile, b.tile_hist);
        mark(1, st);
        // (also clears heavy_count and the three bin arrays for launch_accumulate)
        hipLaunchKernelGGL(k_tile_scan_rows, dim3((p.Bc + 31) / 32), dim3(1024), 0, st, b.tile_hist, p.Bc, p.wtiles, p.pitch, b.tile_base, b.hist_c, b.heavy_count,
                           b.bin_count, (uint32_t)(3 * SIZE_BINS));
        mark(2, st);
        if (p.part) {
            hipLaunchKernelGGL(k_partition, dim3(p.wtiles), dim3(1024), p.lds_partition, st, d_scalars, n, segs, p.pl, p.B, p.Bc, p.cm, p.pitch,
                               b.tile_hist, b.hist_c, b.offs_c, b.tile_base, (uint32_t *)b.recs);
            hipLaunchKernelGGL(k_fine_sort_part, dim3(p.Bc), dim3(1024), p.lds_fine_sort_part, st, (const uint32_t *)b.recs, b.offs_c, b.hist_c,
                               b.tile_base, p.pitch, p.wtiles, p.cm, segs, p.win_stride, p.stage_cap, b.entries, b.hist, b.offs);
        } else if (p.rec32) {
            hipLaunchKernelGGL(k_scatter_wide<2>, dim3(p.wtiles), dim3(1024), p.lds_scatter_wide, st, d_scalars, n, segs, p.pl, p.B, p.Bc, p.pitch, p.wtile, b.hist_c, b.offs_c, b.tile_base, b.recs, p.win_stride);
            hipLaunchKernelGGL(k_fine_sort<uint32_t>, dim3(p.Bc), dim3(1024), 0, st, (const uint32_t *)b.recs, b.offs_c, b.hist_c, b.entries, b.hist, b.offs);
        } else if (p.fine) {
            hipLaunchKernelGGL(k_scatter_wide<1>, dim3(p.wtiles), dim3(1024), p.lds_scatter_wide, st, d_scalars, n, segs, p.pl, p.B, p.Bc, p.pitch, p.wtile, b.hist_c, b.offs_c, b.tile_base, b.recs, p.win_stride);
            hipLaunchKernelGGL(k_fine_sort<uint64_t>, dim3(p.Bc), dim3(1024), 0, st, (const uint64_t *)b.recs, b.offs_c, b.hist_c, b.entries, b.hist, b.offs);
        } else {
            hipLaunchKernelGGL(k_scatter_wide<0>, dim3(p.wtiles), dim3(1024), p.lds_scatter_wide, st, d_scalars, n, segs, p.pl, p.B, p.Bc, p.pitch, p.wtile, b.hist_c, b.offs_c, b.tile_base, (void *)b.entries, p.win_stride);
        }
        mark(3, st);
    } else {
        hipLaunchKernelGGL((k_digits<C::GLV>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_scalars, n, p.c, p.nwin, b.digits);
        hipLaunchKernelGGL(k_rank, dim3(p.ntiles, p.nwin), dim3(1024), p.lds_rank, st, b.digits, p.nv, p.B, p.ntiles, b.rank, b.tile_hist, 0u);
        hipLaunchKernelGGL(k_tile_scan, dim3((p.nb + 255) / 256), dim3(256), 0, st, b.tile_hist, p.B, p.ntiles, p.nb, b.tile_base, b.hist);
        mark(1, st);
        hipLaunchKernelGGL(k_scan_sums, dim3(p.scan_blocks), dim3(256), 0, st, b.hist, p.nb, b.bsum);
        hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(256), 0, st, b.bsum, p.scan_blocks);
        hipLaunchKernelGGL(k_scan_final, dim3(p.scan_blocks), dim3(256), 0, st, b.hist, b.bsum, p.nb, b.offs);
        mark(2, st);
        hipLaunchKernelGGL(k_scatter, dim3(p.ntiles, p.nwin), dim3(1024), p.lds_scatter, st, b.digits, b.rank, b.offs, b.tile_base, p.nv, n, p.B, p.ntiles, b.entries, 0u);
        mark(3, st);
    }
}

// ---- accumulate stage (marks 4, 5): bucket order, accumulation, heavy buckets
template <class C>
static int launch_accumulate(const PipelinePlan &p, const MsmBuffers<typename C::Acc> &b, const typename C::Base *d_bases, hipStream_t st, const Marks &mark) {
    constexpr bool g2 = std::is_same<C, CurveG2>::value;
    // the counters of the ordering stage: a wide sort's k_tile_scan_rows has cleared them (two memset launches less);
    // a shared sort launched nothing
    if (!p.wide || p.reuse_sort) {
        HIPCHK(hipMemsetAsync(b.heavy_count, 0, 4, st));
        HIPCHK(hipMemsetAsync(b.bin_count, 0, (size_t)3 * SIZE_BINS * 4, st));
    }
    const unsigned sb = (p.nb + 2047) / 2048;
    const uint32_t gsz = 0u, ngroups = 1;
    hipLaunchKernelGGL((k_size_hist<C>), dim3(sb), dim3(256), 0, st, b.hist, p.nb, p.heavy_threshold, b.bin_count, gsz, p.bin_shift);
    hipLaunchKernelGGL(k_size_scan, dim3(1), dim3(256), 0, st, b.bin_count, b.bin_start, ngroups);
    hipLaunchKernelGGL((k_size_scatter<C>), dim3(sb), dim3(256), 0, st, b.hist, p.nb, p.heavy_threshold, b.bin_start, b.bin_cursor, b.perm, b.heavy_list, b.heavy_count, b.buckets, gsz, p.bin_shift, p.split);
    mark(4, st);
    const dim3 one_lane((p.nb + 255) / 256), two_lanes((p.nb * 2 + 255) / 256);
    // (measured equal: 3.18 ms for the pair kernel -- 160 VGPRs, no scratch, three wavefronts per SIMD, ~18 % more
    // instructions per addition -- against 3.09 ms for the one-lane kernel at 2^20 pairs: both are instruction-issue
    // bound, the 316 B of scratch were never the cost.  LSA_G2_PAIR=1 selects the pair kernel.)
    if (g2 && p.g2_pair) {
        if constexpr (g2) hipLaunchKernelGGL(k_accumulate_g2_pair, two_lanes, dim3(256), 0, st, d_bases, b.entries, b.offs, b.hist, b.perm, b.bin_start, b.buckets);
    } else if (g2 && p.split == 1) {       // (the generic one-lane kernel at full occupancy -- LSA_G2_OCC1 -- lost to this one in rounds 2-4)
        if constexpr (g2) hipLaunchKernelGGL(k_accumulate_g2_occ2, one_lane, dim3(256), 0, st, d_bases, b.entries, b.offs, b.hist, b.perm, b.bin_start, b.buckets);
    } else if (p.split == 1) {
        hipLaunchKernelGGL((k_accumulate<C, 1u>), one_lane, dim3(256), 0, st, d_bases, b.entries, b.offs, b.hist, b.perm, b.bin_start, b.buckets);
    } else {
        hipLaunchKernelGGL((k_accumulate<C, 2u>), two_lanes, dim3(256), 0, st, d_bases, b.entries, b.offs, b.hist, b.perm, b.bin_start, b.buckets);
    }
    hipLaunchKernelGGL(k_heavy_plan, dim3(1), dim3(256), 0, st, b.hist, b.heavy_list, b.heavy_count, b.chunk_off);
    hipLaunchKernelGGL((k_accumulate_heavy<C>), dim3(4096), dim3(64), 0, st, d_bases, b.entries, b.offs, b.hist,
                       b.heavy_list, b.heavy_count, b.chunk_off, b.hpart);
    hipLaunchKernelGGL((k_heavy_finish<C>), dim3(256), dim3(64), 0, st, b.heavy_list, b.heavy_count, b.chunk_off, b.hpart, b.buckets, p.split);
    mark(5, st);
    return LSA_OK;
}

// ---- tail (marks 6, 7) on the slot's stream: bucket reduction, the point, its publication in d_out
// lane_l1: the first 16-ary level lane-private (plan.lane_l1_shape and the call sequence, see msm_pipeline)
template <class C>
static int launch_tail(const PipelinePlan &p, const MsmBuffers<typename C::Acc> &b, Jac<typename C::Field> *d_out, hipStream_t tail, bool inline_tail,
                       bool lane_l1, MsmSlot &slot, const Marks &mark) {
    using A = typename C::Acc;
    using J = Jac<typename C::Field>;
    constexpr bool g1 = std::is_same<C, CurveG1>::value;
    if (p.big)
        hipLaunchKernelGGL((k_reduce1_lane<C>), dim3(p.kw * ((p.T + 63) / 64)), dim3(64), 0, tail, b.buckets, p.B, p.L, p.split, b.wave_out);
    else
        hipLaunchKernelGGL((k_reduce1<C>), dim3(p.kw * p.wpw), dim3(64), 0, tail, b.buckets, p.B, p.L, p.logL, p.wpw, p.split, b.wave_out);
    A *lvl_in = b.wave_out, *lvl_out = b.window_sums;
    uint32_t m = p.wpw, lm = p.big ? p.logL : p.logL + 4;    // m pairs per window, each covering 2^lm buckets
    J *res = inline_tail ? d_out : (J *)b.res;
    const auto level = [&](bool lane) {              // one 16-ary level: m -> ceil(m / 16) pairs per window
        const uint32_t m_out = (m + 15) / 16;
        if (lane) hipLaunchKernelGGL((k_reduce2_lane<C>), dim3((m_out + 63) / 64), dim3(64), 0, tail, lvl_in, m, m_out, lm, lvl_out);
        else hipLaunchKernelGGL((k_reduce2<C>), dim3(p.kw * m_out), dim3(64), 0, tail, lvl_in, m, m_out, lm, lvl_out);
        std::swap(lvl_in, lvl_out);
        m = m_out;
        lm += 4;
    };
    level(lane_l1);                                  // at least one level (it leaves the sum in slot 0)
    if (p.bits_tail) {
        // one bucket space of 2^19 and more buckets: after the first 16-ary level (m >= 256 left) the rest are bit trees,
        // which end in the Jacobian point
        uint32_t nbits = 0;
        while ((1u << nbits) < m) nbits++;           // indices 0 .. m - 1
        const uint32_t G = (m + 511) / 512;          // <= 16
        A *part = lvl_out;                           // (the level just consumed: (nbits + 1) * G + 16 values fit its m_in * 2)
        A *weighted = part + (size_t)(nbits + 1) * G;
        hipLaunchKernelGGL((k_reduce_bits_a<C>), dim3(nbits + 1, G), dim3(512), 0, tail, lvl_in, m, nbits, G, part);
        hipLaunchKernelGGL((k_reduce_bits_b<C>), dim3(nbits + 1), dim3(64), 0, tail, part, nbits, G, lm, weighted);
        mark(6, tail);
        hipLaunchKernelGGL((k_reduce_bits_c<C>), dim3(1), dim3(64), 0, tail, weighted, nbits + 1, res);
    } else {
        while (m > 1) level(false);
        mark(6, tail);
        // lvl_in[2*k] = sum of window k (pairs of (ACC,RUN): stride 2)
        if (p.wide && p.nseg > 1) {   // every segment's bucket space is a finished sum: convert
            if constexpr (g1) hipLaunchKernelGGL(k_emit_g1, dim3(p.nseg), dim3(64), 0, tail, lvl_in, res);
            else hipLaunchKernelGGL(k_emit_g2, dim3(p.nseg), dim3(64), 0, tail, lvl_in, res);
        } else if constexpr (g1) {   // (wide, one segment: kw = 1, the fold only converts -- with a quad of lanes)
            hipLaunchKernelGGL(k_fold_quad, dim3(1), dim3(64), 0, tail, lvl_in, p.kw, p.c, res);
        } else {
            hipLaunchKernelGGL(k_fold_quad_g2, dim3(1), dim3(64), 0, tail, lvl_in, p.kw, p.c, res);
        }
    }
    if (!inline_tail) {
        int rc = msm_slot_publish_order(&slot);
        if (rc) return rc;
        hipLaunchKernelGGL(k_publish, dim3(1), dim3(256), 0, tail, (const uint32_t *)res, (uint32_t *)d_out, (unsigned)(p.nseg * sizeof(J) / 4));
    }
    mark(7, tail);
    return LSA_OK;
}

static int plan_error(const PipelinePlan &p) {
    switch (p.status) {
    case PLAN_OK: return LSA_OK;
    case PLAN_N_TOO_LARGE: set_error("msm: n too large (%zu)", p.n); break;
    case PLAN_SEGMENTS_NEED_COPIES: set_error("msm: segmented calls need bases with pre-shifted copies"); break;
    case PLAN_TABLE_TOO_LARGE: set_error("msm: base table too large for 30-bit entries"); break;
    case PLAN_BIN_SPACE: set_error("msm: %u segments of %u buckets exceed the bin space", p.nseg, p.B); break;
    }
    return LSA_ERR_INVALID;
}

// The whole pipeline.  segs.nseg == 1: one MSM over n = segs.off[1] pairs.  segs.nseg > 1 (wide path
// only): segment j multiplies scalars[off[j] .. off[j+1]) with bases[first .. first + len_j) and
// d_out receives nseg points.
template <class F>
static int msm_pipeline(const void *d_bases_v, size_t first, const Fr *d_scalars, const SegList &segs, Jac<F> *d_out, hipStream_t st,
                        size_t table_stride, bool reuse_sort = false, bool blocking = false) {
    using C = typename CurveOf<F>::type;
    using A = typename C::Acc;
    const typename C::Base *d_bases = (const typename C::Base *)d_bases_v + first;
    const MsmShape shape = {std::is_same<C, CurveG1>::value ? 1 : 2, sizeof(A), sizeof(Jac<F>), C::GLV, segs.off[segs.nseg], segs.nseg,
                            table_stride, blocking, reuse_sort};
    const PipelinePlan p = plan_pipeline(shape, switches());
    int rc = plan_error(p);
    if (rc) return rc;
    if (g_ws.ensure(p.front.total) != 0) { set_error("msm: workspace allocation of %zu bytes failed", p.front.total); return LSA_ERR_NOMEM; }
    // (Running the sort of call i+1 beside the accumulate of call i on a third stream was measured
    // and rejected: with enough hardware queues for real concurrency both kernels slow each other
    // down by more than the overlap gains -- 1.87 ms per step against 1.70 -- because the
    // accumulate kernel alone already fills every SIMD's issue slots and register file.)
    if (!blocking && (rc = msm_slots_grow_all(p.tail.total)) != 0) return rc;      // growth: a queued call grows every slot, a blocking one its own
    MsmSlot slot;
    rc = msm_slot_begin(st, p.tail.total, d_out, &slot, blocking);
    if (rc) return rc;
    const hipStream_t tail = slot.tail;
    const MsmBuffers<A> b(p, g_ws.ptr, slot.ws);

    if (g_profile && !g_ev_ready) {
        for (auto &row : g_ev) for (auto &e : row) HIPCHK(hipEventCreate(&e));
        g_ev_ready = true;
    }
    const Marks mark = {g_profile ? g_ev[g_ev_calls % EV_POOL] : nullptr};
    mark(0, st);
    rc = msm_func_attrs();
    if (rc) return rc;
    if (reuse_sort) {
        // second MSM of a commitment pair: the entries, populations and offsets of the call just
        // issued on this stream (same scalars, same digit plan, same table stride) are still in the
        // workspace -- the sort does not depend on the bases
        if (!p.wide) { set_error("msm: a shared sort needs bases with pre-shifted copies"); return LSA_ERR_INVALID; }
        mark(1, st); mark(2, st); mark(3, st);
    } else {
        launch_sort<C>(p, b, d_scalars, segs, st, mark);
    }
    rc = launch_accumulate<C>(p, b, d_bases, st, mark);
    if (rc) return rc;
    rc = msm_slot_continue(&slot, st);
    if (rc) return rc;
    // The lane-private first level only when calls are queued back to back: the previous call's tail has not been joined by
    // the caller since it was issued.  Decided from the CALL SEQUENCE alone -- not from whether that tail happens to be running
    // still -- so that the same calls always add in the same order and return the same Jacobian bytes.
    const bool lane_l1 = p.lane_l1_shape && tail != st && msm_slot_follows_unjoined(&slot);
    rc = launch_tail<C>(p, b, d_out, tail, tail == st, lane_l1, slot, mark);
    if (rc) return rc;
    // a blocking caller waits for this tail before it calls again: its next call can take the same slot (and its workspace)
    rc = msm_slot_finish(&slot, st, /*advance=*/!blocking);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    if (g_profile) g_ev_calls++;
    return LSA_OK;
}

template <class F>
int msm_device(const void *d_bases_v, size_t first, const Fr *d_scalars, size_t n, Jac<F> *d_out, hipStream_t st, size_t table_stride, bool blocking) {
    if (n == 0) {
        int jr = msm_join(st);
        if (jr) return jr;
        Jac<F> inf = Jac<F>::inf();
        HIPCHK(hipMemcpyAsync(d_out, &inf, sizeof inf, hipMemcpyDefault, st));       // (d_out may be pinned host memory: blocking callers)
        HIPCHK(hipStreamSynchronize(st));
        return LSA_OK;
    }
    {
        // small and medium calls over a table: the four-launch pipeline of msm_compact.hip (LSA_NO_COMPACT=1: never;
        // LSA_NO_COMPACT_G2=1: G1 only, the round-4 state)
        static const bool allow_compact = getenv("LSA_NO_COMPACT") == nullptr;
        static const bool allow_g2 = getenv("LSA_NO_COMPACT_G2") == nullptr;
        const size_t cmax = std::is_same<F, Fq>::value ? msm_compact_max() : msm_compact_max_g2();
        if (allow_compact && (std::is_same<F, Fq>::value || allow_g2) && table_stride != 0 && n >= switches().table_use_min && n <= cmax)
            return msm_compact_device<F>(d_bases_v, first, d_scalars, n, d_out, st, table_stride, blocking);
    }
    SegList segs;
    segs.nseg = 1;
    segs.off[0] = 0;
    segs.off[1] = (uint32_t)n;
    return msm_pipeline<F>(d_bases_v, first, d_scalars, segs, d_out, st, table_stride, false, blocking);
}

// nseg independent MSMs in one pass: result j = sum_i scalars[off[j] + i] * bases[first + i],
// i < off[j+1] - off[j] (every segment multiplies a PREFIX of the same bases).  Needs the
// pre-shifted copies; at most MSM_MAX_SEGMENTS segments; empty segments give infinity.
template <class F>
int msm_segments_device(const void *d_bases_v, size_t first, const Fr *d_scalars, const uint64_t *seg_off, size_t nseg, Jac<F> *d_out,
                        hipStream_t st, size_t table_stride) {
    if (nseg == 0) return LSA_OK;
    if (nseg > MSM_MAX_SEGMENTS) { set_error("msm_segments: at most %u segments per call", MSM_MAX_SEGMENTS); return LSA_ERR_INVALID; }
    SegList segs;
    segs.nseg = (uint32_t)nseg;
    for (size_t j = 0; j <= nseg; j++) {
        if (seg_off[j] >= (uint64_t(1) << 27) || (j && seg_off[j] < seg_off[j - 1])) { set_error("msm_segments: bad offsets"); return LSA_ERR_INVALID; }
        segs.off[j] = (uint32_t)(seg_off[j] - seg_off[0]);
    }
    if (segs.off[nseg] == 0) {          // nothing but empty segments
        int jr = msm_join(st);
        if (jr) return jr;
        std::vector<Jac<F>> inf(nseg, Jac<F>::inf());
        HIPCHK(hipMemcpyAsync(d_out, inf.data(), nseg * sizeof(Jac<F>), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        return LSA_OK;
    }
    return msm_pipeline<F>(d_bases_v, first, d_scalars + seg_off[0], segs, d_out, st, table_stride);
}
// CommScheme::commit (/root/reference/src/prototools/commit.h:154-155): a G1 and a G2 MSM over the
// SAME scalar vector.  The sort (digits, ranks, scatter, fine sort: a third of a G1 call) depends on
// the scalars and the digit plan only, so it runs once: the G2 pipeline goes first (its workspace
// is the larger one), the G1 pipeline re-uses the sorted entries.  Both tables must have the same
// number of points (the same plan and copy stride); the caller checks that.
int msm_commit_pair_device(const void *d_g1_bases, const void *d_g2_bases, const Fr *d_scalars, size_t n, Jac<Fq> *d_out1,
                           Jac<Fq2> *d_out2, hipStream_t st, size_t table_stride) {
    SegList segs;
    segs.nseg = 1;
    segs.off[0] = 0;
    segs.off[1] = (uint32_t)n;
    int rc = msm_pipeline<Fq2>(d_g2_bases, 0, d_scalars, segs, d_out2, st, table_stride, false);
    if (rc) return rc;
    return msm_pipeline<Fq>(d_g1_bases, 0, d_scalars, segs, d_out1, st, table_stride, true);
}

template int msm_segments_device<Fq>(const void *, size_t, const Fr *, const uint64_t *, size_t, Jac<Fq> *, hipStream_t, size_t);
template int msm_segments_device<Fq2>(const void *, size_t, const Fr *, const uint64_t *, size_t, Jac<Fq2> *, hipStream_t, size_t);

template int msm_device<Fq>(const void *, size_t, const Fr *, size_t, Jac<Fq> *, hipStream_t, size_t, bool);
template int msm_device<Fq2>(const void *, size_t, const Fr *, size_t, Jac<Fq2> *, hipStream_t, size_t, bool);

}  // namespace lsa
