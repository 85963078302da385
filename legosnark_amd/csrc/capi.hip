// legosnark_amd/csrc/capi.hip -- implementation of the C-ABI in include/legosnark_amd.h: library state, bases and the
// MSM, normalise / batch_exp / sum and scalar-multiplication entry points (Fr vectors: capi_fr.hip; pairings:
// capi_pairing.hip; host <-> device copies: host_copy.hip; the CRS cache behind lsa_g1_msm / lsa_g2_msm: crs_cache.hip).
// No CPU fallback: every compute entry point requires lsa_init() to have found a gfx950
// device and fails with LSA_ERR_NO_DEVICE otherwise.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <vector>

#include "capi_internal.h"
#include "crs_cache.h"
#include "tower.h"

namespace lsa {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

State g;

int require_ready() {
    if (!g.ready) {
        set_error("legosnark_amd: no initialised gfx950 device (call lsa_init first; there is no CPU fallback)");
        return LSA_ERR_NO_DEVICE;
    }
    return LSA_OK;
}

}  // namespace lsa

using namespace lsa;

static void warm_stage_buffers();

extern "C" {

int lsa_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *lsa_last_error(void) { return g_err; }
}  // extern "C"
namespace lsa {
bool trace_on() {
    static const bool on = getenv("LSA_TRACE") && (getenv("LSA_TRACE")[0] == '1' || getenv("LSA_TRACE")[0] == '2');
    return on;
}
double CallTrace::now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace lsa
extern "C" {

int lsa_init(int device) {
    if (g.ready && g.device == device) return LSA_OK;
    if (g.ready) lsa_shutdown();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("lsa_init: no HIP device visible (there is no CPU fallback)");
        return LSA_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) {
        set_error("lsa_init: device %d out of range (%d visible)", device, n);
        return LSA_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("lsa_init: device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
        return LSA_ERR_NO_DEVICE;
    }
    HIPCHK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    HIPCHK(hipMalloc(&g.d_result, 512));
    HIPCHK(hipHostMalloc(&g.h_result, 512, hipHostMallocDefault));
    g.device = device;
    upload_prepare();
    const int wrc = msm_warmup(g.stream);
    warm_stage_buffers();
    g.ready = true;                                  // (lsa_shutdown releases what the steps above created)
    if (wrc) { lsa_shutdown(); return wrc; }         // a library whose warm-up failed is not handed out as ready
    return LSA_OK;
}

void lsa_shutdown(void) {
    if (!g.ready) return;
    (void)hipStreamSynchronize(g.stream);
    comm_release();
    crs_shutdown();
    msm_release_workspace();
    batch_exp_release();
    stage_release_all();                             // every StageBuf of every translation unit (staging.h)
    ntt_release();                                   // the per-domain twiddle tables (ntt.hip)
    fr_vec_release();                                // the cached hipGraphs of the Fr recursions (fr_vec.hip)
    pairing_release();
    upload_release();
    (void)hipFree(g.d_result);
    (void)hipHostFree(g.h_result);
    (void)hipStreamDestroy(g.stream);
    g = State();
}

void *lsa_stream(void) { return g.ready ? (void *)g.stream : nullptr; }

int lsa_stream_join(void) {
    int rc = require_ready();
    if (rc) return rc;
    return msm_join(g.stream);
}

int lsa_synchronize(void) {
    int rc = require_ready();
    if (rc) return rc;
    rc = msm_join(g.stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return LSA_OK;
}

unsigned lsa_msm_window_bits(size_t n) { return msm_window_bits(2 * n); }   // G1 (GLV: 2n virtual scalars)

int lsa_profile_enable(int on) { msm_profile_enable(on != 0); return LSA_OK; }
int lsa_profile_last_msm(float ms[LSA_MSM_STAGES]) { return msm_profile_last(ms); }

}  // extern "C"

// grow-only device staging buffers of the host-buffer entry points (StageBuf, staging.h: lsa_shutdown frees every one)
namespace {
StageBuf g_stage_jac, g_stage_bases, g_stage_scalars;
}  // namespace
namespace lsa { StageBuf g_stage_gather; }

// ---------------------------------------------------------------- bases
template <class F>
static int bases_create(const void *bases_jac, size_t n, int src_on_device, int group, lsa_bases **out, bool allow_table = true) {
    int rc = require_ready();
    if (rc) return rc;
    if (!out || (n && !bases_jac)) { set_error("bases_create: null argument"); return LSA_ERR_INVALID; }
    lsa_bases *b = new lsa_bases();
    b->n = n;
    b->group = group;
    if (n) {
        const Jac<F> *d_in = nullptr;
        void *tmp = nullptr;
        // Large resident CRS vectors also keep the pre-shifted windows (msm.hip, "merged
        // windows"): nwin x the memory, no Horner fold per MSM.  LSA_PRECOMPUTE=0 opts out; a
        // table that does not fit falls back to the plain layout.
        const bool may_table = allow_table && !msm_precompute_off();
        bool table = may_table && n >= msm_merge_min();
        // G1 handles of up to 2^16 points: all copies in ONE kernel (msm_compact.hip: one inversion per point instead
        // of 25, ~1.2 ms whatever n) -- cheap enough that every such handle carries them unless a threshold was set
        // explicitly, and their MSMs of up to msm_compact_max() pairs take the four-launch pipeline
        // (G2 handles too since round 5: CommScheme::commit's second half, src/prototools/commit.h:155)
        const bool fast_build = n <= ((size_t)1 << 16) && may_table && (table || !msm_merge_min_is_explicit());
        if (fast_build) table = true;
        const size_t tw = msm_table_windows(group, n);
        if (table && (uint64_t)n * tw >= (1u << 30)) table = false;
        if (table && hipMalloc(&b->d_aff, tw * n * msm_base_bytes(group)) != hipSuccess) { (void)hipGetLastError(); b->d_aff = nullptr; table = false; }
        if (!table && hipMalloc(&b->d_aff, n * msm_base_bytes(group)) != hipSuccess) {
            delete b;
            set_error("bases_create: hipMalloc of %zu bytes failed", n * msm_base_bytes(group));
            return LSA_ERR_NOMEM;
        }
        bool prepared = false;
        if (src_on_device) {
            d_in = (const Jac<F> *)bases_jac;
        } else {
            // the Jacobian staging area: the library's grow-only buffer up to 512 MiB (no hipMalloc / hipFree -- each an
            // implicit device synchronisation and 0.5-2 ms -- inside a prover's first MSM), a temporary beyond
            const size_t jbytes = n * sizeof(Jac<F>);
            void *d_stage = nullptr;
            if (jbytes <= ((size_t)512 << 20)) {
                if (!g_stage_jac.ensure(jbytes)) d_stage = g_stage_jac.p;
            }
            if (!d_stage) {
                if (hipMalloc(&tmp, jbytes) != hipSuccess) {
                    (void)hipFree(b->d_aff); delete b;
                    set_error("bases_create: hipMalloc of %zu bytes failed", jbytes);
                    return LSA_ERR_NOMEM;
                }
                d_stage = tmp;
            }
            d_in = (const Jac<F> *)d_stage;
            // In waves: while the host threads fill the pinned slots of wave k + 1, the copy engine moves wave k and
            // the normalisation kernel of wave k - 1 runs (affine coordinates are unique: the same bytes as one
            // prepare_bases over the whole vector).  One wave for short vectors.
            // A vector the runtime has pinned by now (seen several times) goes as one direct copy, as before.
            const bool slots = upload_takes_slots(bases_jac, jbytes);
            const size_t wave_pts = slots ? ((((size_t)16 << 20) / sizeof(Jac<F>)) & ~(size_t)4095) : n;
            int urc = LSA_OK;
            for (size_t lo = 0; lo < n && !urc; lo += wave_pts) {
                const size_t cnt = n - lo < wave_pts ? n - lo : wave_pts;
                urc = upload_host_as((char *)d_stage + lo * sizeof(Jac<F>), (const char *)bases_jac + lo * sizeof(Jac<F>), cnt * sizeof(Jac<F>), slots, lo == 0);
                if (!urc) urc = prepare_bases<F>(d_in + lo, (char *)b->d_aff + lo * msm_base_bytes(group), cnt, g.stream);
            }
            if (urc) { (void)hipStreamSynchronize(g.stream); if (tmp) (void)hipFree(tmp); (void)hipFree(b->d_aff); delete b; return urc; }
            prepared = true;
        }
        if (!prepared) rc = prepare_bases<F>(d_in, b->d_aff, n, g.stream);
        void *scratch = nullptr;
        if (!rc && table && fast_build) {
            if (hipMalloc(&scratch, table_build_scratch_bytes(n, group)) != hipSuccess) { (void)hipGetLastError(); scratch = nullptr; set_error("bases_create: scratch allocation failed"); rc = LSA_ERR_NOMEM; }
            if (!rc) rc = group == 1 ? table_build_g1_device(b->d_aff, n, n, scratch, g.stream) : table_build_g2_device(b->d_aff, n, n, scratch, g.stream);
            if (!rc) b->table_stride = n;
        } else if (!rc && table) {
            rc = precompute_windows<F>(b->d_aff, n, g.stream);
            if (!rc) b->table_stride = n;
        }
        hipError_t e = hipStreamSynchronize(g.stream);
        if (tmp) (void)hipFree(tmp);
        if (scratch) (void)hipFree(scratch);
        if (rc || e != hipSuccess) {
            if (!rc) { set_error("bases_create: kernel failed: %s", hipGetErrorString(e)); rc = LSA_ERR_HIP; }
            (void)hipFree(b->d_aff); delete b;
            return rc;
        }
    }
    *out = b;
    return LSA_OK;
}

int lsa::bases_create_plain(const void *bases_jac, size_t n, int group, lsa_bases **out) {
    return group == 1 ? bases_create<Fq>(bases_jac, n, 0, 1, out, false) : bases_create<Fq2>(bases_jac, n, 0, 2, out, false);
}

extern "C" {
int lsa_g1_bases_create(const void *bases_jac, size_t n, int src_on_device, lsa_bases **out) {
    return bases_create<Fq>(bases_jac, n, src_on_device, 1, out);
}
int lsa_g2_bases_create(const void *bases_jac, size_t n, int src_on_device, lsa_bases **out) {
    return bases_create<Fq2>(bases_jac, n, src_on_device, 2, out);
}
void lsa_bases_destroy(lsa_bases *b) {
    if (!b) return;
    if (b->d_aff) (void)hipFree(b->d_aff);
    delete b;
}
size_t lsa_bases_size(const lsa_bases *b) { return b ? b->n : 0; }
int lsa_bases_has_table(const lsa_bases *b) { return b && b->table_stride ? 1 : 0; }
void lsa_msm_set_table_threshold(size_t n) { msm_set_merge_min(n); }
unsigned lsa_msm_field_mults_per_pair(const lsa_bases *b, size_t n) { return msm_field_mults_per_pair(n, b ? b->table_stride : 0); }
unsigned lsa_bases_table_windows(const lsa_bases *b) { return b && b->table_stride ? msm_table_windows(b->group, b->n) : 0; }
const void *lsa_bases_device_ptr(const lsa_bases *b) { return b ? b->d_aff : nullptr; }

// ---------------------------------------------------------------- MSM
int lsa_msm_run_async(const lsa_bases *bases, size_t first, const void *d_scalars, size_t n, void *d_out_jac) {
    int rc = require_ready();
    if (rc) return rc;
    if (!bases || !d_out_jac || (n && !d_scalars)) { set_error("msm_run: null argument"); return LSA_ERR_INVALID; }
    if (first > bases->n || n > bases->n - first) { set_error("msm_run: range [%zu,%zu) exceeds %zu bases", first, first + n, bases->n); return LSA_ERR_INVALID; }
    if (bases->group == 1)
        return msm_device<Fq>(bases->d_aff, first, (const Fr *)d_scalars, n, (Jac<Fq> *)d_out_jac, g.stream, bases->table_stride);
    return msm_device<Fq2>(bases->d_aff, first, (const Fr *)d_scalars, n, (Jac<Fq2> *)d_out_jac, g.stream, bases->table_stride);
}

int lsa_msm_run_segments_async(const lsa_bases *bases, size_t first, const void *d_scalars, const uint64_t *seg_offsets, size_t nseg,
                               void *d_out_jac) {
    int rc = require_ready();
    if (rc) return rc;
    if (nseg == 0) return LSA_OK;
    if (!bases || !d_out_jac || !seg_offsets || !d_scalars) { set_error("msm_run_segments: null argument"); return LSA_ERR_INVALID; }
    if (!bases->table_stride) { set_error("msm_run_segments: the bases carry no pre-shifted copies (lsa_bases_has_table)"); return LSA_ERR_INVALID; }
    for (size_t j = 0; j < nseg; j++) {
        if (seg_offsets[j + 1] < seg_offsets[j]) { set_error("msm_run_segments: offsets must not decrease"); return LSA_ERR_INVALID; }
        const size_t len = seg_offsets[j + 1] - seg_offsets[j];
        if (first > bases->n || len > bases->n - first) { set_error("msm_run_segments: segment %zu of %zu pairs exceeds the %zu bases", j, len, bases->n); return LSA_ERR_INVALID; }
    }
    if (bases->group == 1)
        return msm_segments_device<Fq>(bases->d_aff, first, (const Fr *)d_scalars, seg_offsets, nseg, (Jac<Fq> *)d_out_jac, g.stream, bases->table_stride);
    return msm_segments_device<Fq2>(bases->d_aff, first, (const Fr *)d_scalars, seg_offsets, nseg, (Jac<Fq2> *)d_out_jac, g.stream, bases->table_stride);
}

int lsa_commit_run_async(const lsa_bases *g1_bases, const lsa_bases *g2_bases, const void *d_scalars, size_t n, void *d_out_g1, void *d_out_g2) {
    int rc = require_ready();
    if (rc) return rc;
    if (!g1_bases || !g2_bases || !d_out_g1 || !d_out_g2 || (n && !d_scalars)) { set_error("commit_run: null argument"); return LSA_ERR_INVALID; }
    if (g1_bases->group != 1 || g2_bases->group != 2) { set_error("commit_run: needs a G1 and a G2 handle, in that order"); return LSA_ERR_INVALID; }
    if (n > g1_bases->n || n > g2_bases->n) { set_error("commit_run: %zu pairs exceed the bases (%zu, %zu)", n, g1_bases->n, g2_bases->n); return LSA_ERR_INVALID; }
    // one shared sort when both handles carry copies over the same number of points AND an MSM of n pairs runs
    // over them (an explicit table threshold above n sends both to the plain pipeline); else two calls
    if (n && g1_bases->table_stride && g1_bases->table_stride == g2_bases->table_stride && msm_uses_table(n))
        return msm_commit_pair_device(g1_bases->d_aff, g2_bases->d_aff, (const Fr *)d_scalars, n, (Jac<Fq> *)d_out_g1, (Jac<Fq2> *)d_out_g2, g.stream,
                                      g1_bases->table_stride);
    rc = msm_device<Fq>(g1_bases->d_aff, 0, (const Fr *)d_scalars, n, (Jac<Fq> *)d_out_g1, g.stream, g1_bases->table_stride);
    if (rc) return rc;
    return msm_device<Fq2>(g2_bases->d_aff, 0, (const Fr *)d_scalars, n, (Jac<Fq2> *)d_out_g2, g.stream, g2_bases->table_stride);
}

// Blocking: the tail runs on lsa_stream() itself and the last kernel writes the point straight into pinned host memory
// (no cross-stream hand-over, no copy command behind the kernels: ~35 us of a small call's latency).
int lsa_msm_run(const lsa_bases *bases, size_t first, const void *d_scalars, size_t n, void *out_jac) {
    int rc = require_ready();
    if (rc) return rc;
    if (!bases || !out_jac || (n && !d_scalars)) { set_error("msm_run: null argument"); return LSA_ERR_INVALID; }
    if (first > bases->n || n > bases->n - first) { set_error("msm_run: range [%zu,%zu) exceeds %zu bases", first, first + n, bases->n); return LSA_ERR_INVALID; }
    rc = msm_join(g.stream);                       // earlier asynchronous calls publish before this one (call order)
    if (rc) return rc;
    if (bases->group == 1)
        rc = msm_device<Fq>(bases->d_aff, first, (const Fr *)d_scalars, n, (Jac<Fq> *)g.h_result, g.stream, bases->table_stride, true);
    else
        rc = msm_device<Fq2>(bases->d_aff, first, (const Fr *)d_scalars, n, (Jac<Fq2> *)g.h_result, g.stream, bases->table_stride, true);
    if (rc) return rc;
    size_t bytes = bases->group == 1 ? sizeof(Jac<Fq>) : sizeof(Jac<Fq2>);
    HIPCHK(hipStreamSynchronize(g.stream));
    memcpy(out_jac, g.h_result, bytes);
    return LSA_OK;
}

}  // extern "C"
// lsa_init: the staging buffers of the host-vector entry points at the BASELINE scale (2^20 scalars, 2^20 G2 points in
// Jacobian form), beside msm_warmup's workspaces: no allocation inside a prover's first multiExpMA (LSA_WARM=0: lazy)
static void warm_stage_buffers() {
    // (LSA_WARM_MB scales these with the MSM workspaces: 400 is the default there)
    size_t scale = 0;
    if (!msm_warm_mb(&scale) || scale == 0) return;
    const int e1 = g_stage_scalars.ensure(((size_t)34 << 20) * scale / 400), e2 = g_stage_jac.ensure(((size_t)202 << 20) * scale / 400);
    if ((e1 || e2) && trace_on()) fprintf(stderr, "[lsa]   warm-up: staging buffers not allocated\n");
    (void)hipGetLastError();
}

// ---------------------------------------------------------------- MSM over host vectors
static lsa_host_stats g_host_stats = {};

static inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// this process's MSM into g.d_result (stream-ordered, tails joined); the host-side wall-clock split in `st`
template <class F>
static int msm_host_local(const void *bases_jac, const void *scalars, size_t n, int group, lsa_host_stats &st,
                          std::chrono::steady_clock::time_point &t_msm, bool to_host) {
    int rc = LSA_OK;
    const bool cached = crs_wanted(n);
    if (g_stage_scalars.ensure(n * sizeof(Fr))) { set_error("msm: staging allocation failed"); return LSA_ERR_NOMEM; }
    const void *d_bases = nullptr;
    size_t table_stride = 0;
    // the bases: a resident entry of the CRS cache (crs_cache.hip), a prefix of one, or uploaded for this call alone
    if (cached) {
        // the fingerprint of the bases is computed by the cache's threads while this thread uploads the scalars
        crs_fingerprint_begin(bases_jac, n, sizeof(Jac<F>));
        auto t0 = std::chrono::steady_clock::now();
        const int ce = upload_host(g_stage_scalars.p, scalars, n * sizeof(Fr));
        st.h2d_scalars_ms = ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        crs_fingerprint_finish();                       // also on the error path: the workers read the caller's buffer
        if (ce) return ce;
        st.fingerprint_wait_ms = ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        CrsEntry *e = nullptr;
        bool hit = false;
        rc = crs_lookup_or_insert(bases_jac, n, group, &e, &hit);
        if (rc) return rc;
        st.bases_prepare_ms = ms_since(t0);
        st.cache_hit = hit ? 1 : 0;
        rc = crs_bases_for(e, n, &d_bases, &table_stride, st);
        if (rc) return rc;
    } else if (CrsEntry *pe = crs_lookup_small(bases_jac, n, group)) {
        auto t0 = std::chrono::steady_clock::now();
        rc = upload_host(g_stage_scalars.p, scalars, n * sizeof(Fr));
        if (rc) return rc;
        st.h2d_scalars_ms = ms_since(t0);
        st.cache_hit = 1;
        rc = crs_bases_for(pe, n, &d_bases, &table_stride, st);
        if (rc) return rc;
    } else {
        if (g_stage_jac.ensure(n * sizeof(Jac<F>)) || g_stage_bases.ensure(n * msm_base_bytes(group))) {
            set_error("msm: staging allocation failed");
            return LSA_ERR_NOMEM;
        }
        if (n) {
            auto t0 = std::chrono::steady_clock::now();
            rc = upload_host(g_stage_jac.p, bases_jac, n * sizeof(Jac<F>));
            if (rc) return rc;
            st.bases_prepare_ms = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            rc = upload_host(g_stage_scalars.p, scalars, n * sizeof(Fr));
            if (rc) return rc;
            st.h2d_scalars_ms = ms_since(t0);
            rc = prepare_bases<F>((const Jac<F> *)g_stage_jac.p, g_stage_bases.p, n, g.stream);
            if (rc) return rc;
        }
        d_bases = g_stage_bases.p;
    }
    t_msm = std::chrono::steady_clock::now();
    rc = msm_join(g.stream);
    if (rc) return rc;
    // blocking call: tail on lsa_stream(); unless the partials still have to be exchanged, the result lands in pinned host memory
    return msm_device<F>(d_bases, 0, (const Fr *)g_stage_scalars.p, n, (Jac<F> *)(to_host ? g.h_result : g.d_result), g.stream, table_stride, true);
}

template <class F>
static int msm_host(const void *bases_jac, const void *scalars, size_t n, void *out_jac, int group, bool sharded = false) {
    LSA_TRACE_CALL(group == 1 ? "msm_g1" : "msm_g2", n);
    int rc = require_ready();
    if (rc) return rc;
    if (sharded && lsa_comm_world() <= 1) sharded = false;
    if (!out_jac || (n && (!bases_jac || !scalars))) { set_error("msm: null argument"); return LSA_ERR_INVALID; }
    const auto t_all = std::chrono::steady_clock::now();
    lsa_host_stats st = {};
    st.n = n;
    auto t0 = std::chrono::steady_clock::now();
    rc = msm_host_local<F>(bases_jac, scalars, n, group, st, t0, !sharded);
    if (sharded) {
        // this rank's slice is one libff chunk: all-gather the partials, sum them in rank order.  A rank whose
        // local part failed still takes part (with the point at infinity: all-zero bytes) and reports its error
        // afterwards -- the other ranks must not be left blocking in ncclAllGather.
        const int local = rc;
        const size_t world = (size_t)lsa_comm_world();
        if (local) (void)hipMemsetAsync(g.d_result, 0, sizeof(Jac<F>), g.stream);
        if (g_stage_gather.ensure(world * sizeof(Jac<F>))) { set_error("msm: staging allocation failed"); return LSA_ERR_NOMEM; }
        rc = lsa_comm_all_gather(g.d_result, g_stage_gather.p, group);
        if (local) return local;
        if (rc) return rc;
        rc = sum_points_device<F>((const Jac<F> *)g_stage_gather.p, world, (Jac<F> *)g.d_result, g.stream);
    }
    if (rc) return rc;
    if (sharded) HIPCHK(hipMemcpyAsync(g.h_result, g.d_result, sizeof(Jac<F>), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    memcpy(out_jac, g.h_result, sizeof(Jac<F>));
    crs_after_drain();                                     // lsa_stream() has just drained
    st.msm_ms = ms_since(t0);
    st.total_ms = ms_since(t_all);
    g_host_stats = st;
    if (trace_on())
        fprintf(stderr, "[lsa]   msm_split                  h2d_scalars=%.3f fingerprint_wait=%.3f bases_prepare=%.3f kernels=%.3f hit=%d table=%d\n",
                st.h2d_scalars_ms, st.fingerprint_wait_ms, st.bases_prepare_ms, st.msm_ms, st.cache_hit, st.table);
    return LSA_OK;
}

extern "C" {
int lsa_g1_msm(const void *bases_jac, const void *scalars, size_t n, size_t chunks, void *out_jac) {
    (void)chunks;
    return msm_host<Fq>(bases_jac, scalars, n, out_jac, 1);
}
int lsa_g2_msm(const void *bases_jac, const void *scalars, size_t n, size_t chunks, void *out_jac) {
    (void)chunks;
    return msm_host<Fq2>(bases_jac, scalars, n, out_jac, 2);
}
int lsa_g1_msm_sharded(const void *bases_jac, const void *scalars, size_t n_local, void *out_jac) {
    return msm_host<Fq>(bases_jac, scalars, n_local, out_jac, 1, true);
}
int lsa_g2_msm_sharded(const void *bases_jac, const void *scalars, size_t n_local, void *out_jac) {
    return msm_host<Fq2>(bases_jac, scalars, n_local, out_jac, 2, true);
}
int lsa_msm_host_stats(lsa_host_stats *out) {
    if (!out) return LSA_ERR_INVALID;
    *out = g_host_stats;
    return LSA_OK;
}

// ---------------------------------------------------------------- normalisation
}  // extern "C"
template <class F>
static int normalize_host(const void *in_jac, size_t n, void *out_jac) {
    LSA_TRACE_CALL("normalize", n);
    int rc = require_ready();
    if (rc) return rc;
    if (n == 0) return LSA_OK;
    if (!in_jac || !out_jac) { set_error("normalize: null argument"); return LSA_ERR_INVALID; }
    void *d_in = nullptr, *d_aff = nullptr;
    if (hipMalloc(&d_in, n * sizeof(Jac<F>)) != hipSuccess || hipMalloc(&d_aff, n * sizeof(Aff<F>)) != hipSuccess) {
        if (d_in) (void)hipFree(d_in);
        set_error("normalize: hipMalloc failed");
        return LSA_ERR_NOMEM;
    }
    rc = upload_host(d_in, in_jac, n * sizeof(Jac<F>));
    if (!rc) rc = normalize_to_affine<F>((const Jac<F> *)d_in, (Aff<F> *)d_aff, n, g.stream);
    std::vector<Aff<F>> host(n);
    if (!rc) rc = download_host(host.data(), d_aff, n * sizeof(Aff<F>));
    const hipError_t e = hipStreamSynchronize(g.stream);
    (void)hipFree(d_in);
    (void)hipFree(d_aff);
    if (rc) return rc;
    if (e != hipSuccess) { set_error("normalize: %s", hipGetErrorString(e)); return LSA_ERR_HIP; }
    Jac<F> *o = (Jac<F> *)out_jac;
    for (size_t i = 0; i < n; i++) {
        if (host[i].is_inf()) o[i] = Jac<F>::inf();
        else o[i] = Jac<F>{host[i].x, host[i].y, F::one()};
    }
    return LSA_OK;
}
extern "C" {
int lsa_g1_normalize(const void *in_jac, size_t n, void *out_jac) { return normalize_host<Fq>(in_jac, n, out_jac); }
int lsa_g2_normalize(const void *in_jac, size_t n, void *out_jac) { return normalize_host<Fq2>(in_jac, n, out_jac); }

}  // extern "C"

// ---------------------------------------------------------------- batch_exp / sum
template <class F>
static int batch_exp_any(const void *base_jac, const void *scalars, size_t n, void *out_jac, int on_device) {
    LSA_TRACE_CALL("batch_exp", n);
    int rc = require_ready();
    if (rc) return rc;
    if (n == 0) return LSA_OK;
    if (!base_jac || !scalars || !out_jac) { set_error("batch_exp: null argument"); return LSA_ERR_INVALID; }
    Jac<F> base;
    memcpy(&base, base_jac, sizeof base);
    if (on_device) return batch_exp_device<F>(base, (const Fr *)scalars, n, (Jac<F> *)out_jac, g.stream);
    // grow-only staging (the shim calls this with anything from one scalar to a whole key vector)
    if (g_stage_scalars.ensure(n * sizeof(Fr)) || g_stage_jac.ensure(n * sizeof(Jac<F>))) { set_error("batch_exp: staging allocation failed"); return LSA_ERR_NOMEM; }
    void *d_sc = g_stage_scalars.p, *d_out = g_stage_jac.p;
    rc = upload_host(d_sc, scalars, n * sizeof(Fr));
    if (!rc) rc = batch_exp_device<F>(base, (const Fr *)d_sc, n, (Jac<F> *)d_out, g.stream);
    if (!rc) rc = download_host(out_jac, d_out, n * sizeof(Jac<F>));
    const hipError_t e = hipStreamSynchronize(g.stream);
    if (rc) return rc;
    if (e != hipSuccess) { set_error("batch_exp: %s", hipGetErrorString(e)); return LSA_ERR_HIP; }
    return LSA_OK;
}

extern "C" {
int lsa_g1_batch_exp(const void *base_jac, const void *scalars, size_t n, void *out_jac, int on_device) {
    return batch_exp_any<Fq>(base_jac, scalars, n, out_jac, on_device);
}
int lsa_g2_batch_exp(const void *base_jac, const void *scalars, size_t n, void *out_jac, int on_device) {
    return batch_exp_any<Fq2>(base_jac, scalars, n, out_jac, on_device);
}
// the same on a caller-supplied stream, without touching lsa_stream(): lets the collective and
// the fold of step i run beside the MSM front of step i+1
}  // extern "C"
template <class F>
static int sum_on_any(const void *d_pts, size_t n, void *d_out, void *stream) {
    int rc = require_ready();
    if (rc) return rc;
    if (!d_out || (n && !d_pts)) { set_error("sum: null argument"); return LSA_ERR_INVALID; }
    return sum_points_device<F>((const Jac<F> *)d_pts, n, (Jac<F> *)d_out, (hipStream_t)stream);
}
extern "C" {
int lsa_g1_sum_on(const void *d_pts, size_t n, void *d_out, void *stream) { return sum_on_any<Fq>(d_pts, n, d_out, stream); }
int lsa_g2_sum_on(const void *d_pts, size_t n, void *d_out, void *stream) { return sum_on_any<Fq2>(d_pts, n, d_out, stream); }
int lsa_stream_join_to(void *stream) {
    int rc = require_ready();
    if (rc) return rc;
    return msm_join_to((hipStream_t)stream);
}
int lsa_g1_sum_async(const void *d_pts, size_t n, void *d_out) {
    int rc = require_ready();
    if (rc) return rc;
    if (!d_out || (n && !d_pts)) { set_error("sum: null argument"); return LSA_ERR_INVALID; }
    rc = msm_join(g.stream);
    if (rc) return rc;
    return sum_points_device<Fq>((const Jac<Fq> *)d_pts, n, (Jac<Fq> *)d_out, g.stream);
}
int lsa_g2_sum_async(const void *d_pts, size_t n, void *d_out) {
    int rc = require_ready();
    if (rc) return rc;
    if (!d_out || (n && !d_pts)) { set_error("sum: null argument"); return LSA_ERR_INVALID; }
    rc = msm_join(g.stream);
    if (rc) return rc;
    return sum_points_device<Fq2>((const Jac<Fq2> *)d_pts, n, (Jac<Fq2> *)d_out, g.stream);
}
}  // extern "C"

// ---------------------------------------------------------------- variable-base scalar mul / sparse matrix
namespace {
inline int smul_device(const Jac<Fq> *p, const Fr *s, const uint32_t *idx, size_t n, Jac<Fq> *o, hipStream_t st) { return g1_scalar_mul_device(p, s, idx, n, o, st); }
inline int smul_device(const Jac<Fq2> *p, const Fr *s, const uint32_t *idx, size_t n, Jac<Fq2> *o, hipStream_t st) { return g2_scalar_mul_device(p, s, idx, n, o, st); }
inline int colsum_device(const Jac<Fq> *it, const uint64_t *cp, size_t ncols, Jac<Fq> *o, hipStream_t st) { return g1_column_sums_device(it, cp, ncols, o, st); }
inline int colsum_device(const Jac<Fq2> *it, const uint64_t *cp, size_t ncols, Jac<Fq2> *o, hipStream_t st) { return g2_column_sums_device(it, cp, ncols, o, st); }

// the body of lsa_g1_scalar_mul_batch / lsa_g2_scalar_mul_batch (F = Fq / Fq2)
template <class F>
int scalar_mul_batch(const void *pts_jac, const void *scalars, size_t n, void *out_jac, int on_device) {
    int rc = require_ready();
    if (rc) return rc;
    if (n == 0) return LSA_OK;
    if (!pts_jac || !scalars || !out_jac) { set_error("scalar_mul_batch: null argument"); return LSA_ERR_INVALID; }
    rc = msm_join(g.stream);
    if (rc) return rc;
    DevBuf d_p, d_s, d_o;
    OperandFrame f("scalar_mul_batch", on_device);
    const Jac<F> *p = f.in<Jac<F>>(d_p, pts_jac, n * sizeof(Jac<F>));
    const Fr *s = f.in<Fr>(d_s, scalars, n * sizeof(Fr));
    Jac<F> *o = f.out<Jac<F>>(d_o, out_jac, n * sizeof(Jac<F>));
    if (f.rc()) return f.rc();
    rc = smul_device(p, s, nullptr, n, o, g.stream);
    if (rc) return rc;
    return f.download();
}

// the body of lsa_g1_sparse_matrix_msm / lsa_g2_sparse_matrix_msm
template <class F>
int sparse_matrix_msm(const void *vals_jac, const uint32_t *rows, const uint64_t *col_ptr, size_t ncols, const void *exps, size_t nrows,
                      void *out_jac) {
    int rc = require_ready();
    if (rc) return rc;
    if (ncols == 0) return LSA_OK;
    if (!col_ptr || !out_jac) { set_error("sparse_matrix_msm: null argument"); return LSA_ERR_INVALID; }
    const uint64_t nnz = col_ptr[ncols];
    if (col_ptr[0] != 0) { set_error("sparse_matrix_msm: col_ptr[0] must be 0"); return LSA_ERR_INVALID; }
    for (size_t j = 0; j < ncols; j++)
        if (col_ptr[j] > col_ptr[j + 1]) { set_error("sparse_matrix_msm: col_ptr not monotone at column %zu", j); return LSA_ERR_INVALID; }
    if (nnz && (!vals_jac || !rows || !exps)) { set_error("sparse_matrix_msm: null argument"); return LSA_ERR_INVALID; }
    for (uint64_t e = 0; e < nnz; e++)
        if (rows[e] >= nrows) { set_error("sparse_matrix_msm: row index %u out of range (%zu rows)", rows[e], nrows); return LSA_ERR_INVALID; }
    rc = msm_join(g.stream);
    if (rc) return rc;
    DevBuf d_v, d_r, d_c, d_e, d_items, d_o;
    OperandFrame f("sparse_matrix_msm", /*on_device=*/0);            // (host buffers only; the exponents go up only with entries to use them)
    const Jac<F> *v = f.in<Jac<F>>(d_v, vals_jac, nnz * sizeof(Jac<F>));
    const uint32_t *r = f.in<uint32_t>(d_r, rows, nnz * sizeof(uint32_t));
    const Fr *e = f.in<Fr>(d_e, exps, nnz ? nrows * sizeof(Fr) : 0, nrows * sizeof(Fr));
    const uint64_t *c = f.in<uint64_t>(d_c, col_ptr, (ncols + 1) * sizeof(uint64_t));
    Jac<F> *items = f.scratch<Jac<F>>(d_items, nnz * sizeof(Jac<F>));
    Jac<F> *o = f.out<Jac<F>>(d_o, out_jac, ncols * sizeof(Jac<F>));
    if (f.rc()) return f.rc();
    rc = smul_device(v, e, r, nnz, items, g.stream);
    if (rc) return rc;
    rc = colsum_device(items, c, ncols, o, g.stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return f.download();
}
}  // namespace

extern "C" {
int lsa_g1_scalar_mul_batch(const void *pts_jac, const void *scalars, size_t n, void *out_jac, int on_device) {
    LSA_TRACE_CALL("g1_scalar_mul_batch", n);
    return scalar_mul_batch<Fq>(pts_jac, scalars, n, out_jac, on_device);
}
int lsa_g2_scalar_mul_batch(const void *pts_jac, const void *scalars, size_t n, void *out_jac, int on_device) {
    LSA_TRACE_CALL("g2_scalar_mul_batch", n);
    return scalar_mul_batch<Fq2>(pts_jac, scalars, n, out_jac, on_device);
}
int lsa_g1_sparse_matrix_msm(const void *vals_jac, const uint32_t *rows, const uint64_t *col_ptr, size_t ncols,
                             const void *exps, size_t nrows, void *out_jac) {
    return sparse_matrix_msm<Fq>(vals_jac, rows, col_ptr, ncols, exps, nrows, out_jac);
}
int lsa_g2_sparse_matrix_msm(const void *vals_jac, const uint32_t *rows, const uint64_t *col_ptr, size_t ncols,
                             const void *exps, size_t nrows, void *out_jac) {
    return sparse_matrix_msm<Fq2>(vals_jac, rows, col_ptr, ncols, exps, nrows, out_jac);
}
size_t lsa_smul_param(int which) {
    switch (which) {
    case LSA_SMUL_PARAM_G1_WINDOW_BITS: return g1_smul_param(0);
    case LSA_SMUL_PARAM_G2_WINDOW_BITS: return g2_smul_param(0);
    case LSA_SMUL_PARAM_G1_RESIDENT_ITEMS: return g1_smul_param(1);
    case LSA_SMUL_PARAM_G2_RESIDENT_ITEMS: return g2_smul_param(1);
    case LSA_SMUL_PARAM_G2_LANES_PER_ITEM: return g2_smul_param(2);
    }
    return 0;
}
}  // extern "C"
