// legosnark_amd/csrc/crs_cache.hip -- the CRS cache behind lsa_g1_msm / lsa_g2_msm (interface: crs_cache.h) and the
// lsa_crs_cache_* entry points.  The one part of the C-ABI layer that owns threads and decides the lifetime of device
// buffers; its host-only pieces are keyed_hash.h, hash_pool.h and crs_index.h.
//
// multiExpMA hands libff the same std::vector<G> on every call of a prover: crs->P in
// SubspaceSnark::prove (src/gadgets/subspace.cc:82), g1s/g2s in CommScheme::commit
// (src/prototools/commit.h:154-155), prefixes of g1s in CPPoly::prove (src/gadgets/poly.h:77-86).
// Uploading 96 B/point over PCIe and normalising it each time costs more than the MSM, so the
// host-buffer entry points keep the prepared (affine, packed; after the first re-use also the
// pre-shifted window copies) bases of recently seen vectors resident, keyed by host pointer and
// VERIFIED by content before every use:
//   mode 2 "full" (default): a 64-bit fingerprint of every 64-point unit, computed by a small
//          host thread pool while the caller thread uploads the scalars; any change of any byte
//          of the vector is a miss (a single changed word always changes its unit's fingerprint).
//          Never reads past the n points the caller passed.
//   mode 1 "sampled": only ~3*log2(n) sampled points are compared -- for callers that promise
//          not to modify a CRS vector in place.
//   mode 0: off.  Env LSA_CRS_CACHE = full | sampled | 0, LSA_CRS_CACHE_MB = budget (LRU by bytes).
// A request (ptr, n) also hits an entry (ptr, n' > n) when n is a multiple of 64: the prefix is
// verified unit-wise (CPPoly::prove's ladder of prefixes 2^k of g1s).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <deque>
#include <list>
#include <memory>

#include "capi_internal.h"
#include "crs_cache.h"
#include "hash_pool.h"    // (and with it <atomic>, <condition_variable>, <mutex>, <thread>, <vector>)
#include "tower.h"

namespace lsa {

namespace {

constexpr unsigned CRS_TABLE_AFTER_DEFAULT = 23;

// One background build: allocates the table, fills copy 0 from the entry's prepared bases and derives the other copies
// one at a time on a low-priority stream, each time waiting (at most 2 ms) for lsa_stream() to be idle first -- an MSM
// issued meanwhile overlaps with at most one copy step (~1 ms of the GPU at 2^20 points).
struct TableBuild {
    std::atomic<int> state{0};                      // 0: queued / running, 1: table complete, 2: failed or cancelled (buffers freed)
    std::atomic<bool> cancel{false};
    const void *bases = nullptr;                    // the entry's prepared bases (read-only)
    void *big = nullptr, *tmp = nullptr;
    size_t n = 0;
    int group = 1;
};
class TableBuilder {
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<std::shared_ptr<TableBuild>> q_;
    bool stop_ = false;
    std::atomic<bool> abandon_{false};              // process exit: no more HIP calls from this thread (the runtime may be gone)
    hipStream_t stream_ = nullptr;

    void run(TableBuild &j) {
        const size_t tw = msm_table_windows(j.group, j.n), per = msm_base_bytes(j.group);
        const size_t jac = j.group == 1 ? sizeof(Jac<Fq>) : sizeof(Jac<Fq2>);
        // the call that asked for the build is still running its own MSM: let it finish first (it is the "second call")
        {
            const auto t0 = std::chrono::steady_clock::now();
            std::this_thread::sleep_for(std::chrono::microseconds(200));
            while (hipStreamQuery(g.stream) == hipErrorNotReady && !j.cancel.load() &&
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() < 6.0)
                std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
        bool ok = hipMalloc(&j.big, tw * j.n * per) == hipSuccess && hipMalloc(&j.tmp, j.n * jac) == hipSuccess;
        ok = ok && hipMemcpyAsync(j.big, j.bases, j.n * per, hipMemcpyDeviceToDevice, stream_) == hipSuccess;
        for (unsigned k = 1; ok && k < tw && !j.cancel.load() && !abandon_.load(); k++) {
            const auto t0 = std::chrono::steady_clock::now();
            while (hipStreamQuery(g.stream) == hipErrorNotReady && !j.cancel.load() &&
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() < 2.0)
                std::this_thread::sleep_for(std::chrono::microseconds(30));
            const int rc = j.group == 1 ? precompute_window_step<Fq>(j.big, j.n, j.tmp, k, stream_) : precompute_window_step<Fq2>(j.big, j.n, j.tmp, k, stream_);
            ok = rc == LSA_OK && hipStreamSynchronize(stream_) == hipSuccess;
        }
        if (abandon_.load()) { j.state.store(2); return; }
        if (ok && !j.cancel.load() && hipStreamSynchronize(stream_) == hipSuccess) { j.state.store(1); return; }
        (void)hipGetLastError();
        (void)hipStreamSynchronize(stream_);
        if (j.big) (void)hipFree(j.big);
        if (j.tmp) (void)hipFree(j.tmp);
        j.big = j.tmp = nullptr;
        j.state.store(2);
    }
    void loop(int device) {
        (void)hipSetDevice(device);
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (hipStreamCreateWithPriority(&stream_, hipStreamNonBlocking, least) != hipSuccess) stream_ = nullptr;
        for (;;) {
            std::shared_ptr<TableBuild> j;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
                if (stop_ && q_.empty()) break;
                j = q_.front();
                q_.pop_front();
            }
            if (!stream_ || j->cancel.load()) { j->state.store(2); continue; }
            run(*j);
        }
        if (stream_ && !abandon_.load()) (void)hipStreamDestroy(stream_);
        stream_ = nullptr;
    }

  public:
    ~TableBuilder() { abandon_.store(true); shutdown(); }
    void submit(std::shared_ptr<TableBuild> j) {
        std::lock_guard<std::mutex> lk(m_);
        if (!th_.joinable()) { stop_ = false; th_ = std::thread([this, d = g.device] { loop(d); }); }
        q_.push_back(std::move(j));
        cv_.notify_all();
    }
    // after this every submitted build has state != 0
    void shutdown() {
        {
            std::lock_guard<std::mutex> lk(m_);
            for (auto &j : q_) j->cancel.store(true);
            stop_ = true;
        }
        cv_.notify_all();
        if (th_.joinable()) th_.join();
    }
};

}  // namespace

struct CrsEntry {
    const void *ptr = nullptr;
    size_t n = 0;
    int group = 1;
    std::vector<uint64_t> unit_fp;                  // mode 2: one fingerprint per 64-point unit (the last may be short)
    std::vector<uint64_t> head_fp;                  // mode 2: one fingerprint per point of the first unit (prefixes shorter than a unit)
    std::vector<size_t> sample_pos;                 // mode 1
    std::vector<uint8_t> sample;
    lsa_bases *b = nullptr;
    size_t bytes = 0;
    uint64_t tick = 0;
    unsigned hits = 0;
    // the pre-shifted window copies are built by a background thread (TableBuilder): the entry keeps serving the
    // plain layout until the build has finished, then switches; nobody ever waits for the 26 copies
    std::shared_ptr<TableBuild> build;
    void *small = nullptr;                          // the plain bases after the switch (an MSM queued earlier may still read them)
    // G1: pre-shifted copies of the entry's first prefix_n points only, built in one kernel on lsa_stream() when the first
    // request that fits arrives (crs_bases_for): the tails of the reference's prefix ladders run over them
    void *prefix = nullptr;
    size_t prefix_n = 0;
    unsigned prefix_asks = 0;                       // G2: requests a prefix table would have served (it is built at the second)
    unsigned build_attempts = 0;                    // table builds handed to the builder thread (a failed one is retried once)
    bool building() const { return build && build->state.load() == 0; }
};

namespace {

struct CrsCache {
    int mode = -1;                                  // -1: read the environment on first use
    size_t budget = 0, bytes = 0;
    uint64_t tick = 0, hits = 0, misses = 0;
    std::list<CrsEntry> entries;                    // in insertion order (the first match wins); an entry stays where it is while others go
    HashPool pool;
    std::vector<uint64_t> scratch_fp;
    TableBuilder builder;
    // hits before an entry's copies are built (0: never; LSA_CRS_TABLE_AFTER).  The copies of 2^20 G1 points cost ~27 ms of
    // GPU time and save ~1.2 ms per MSM: building them at the 23rd hit is the break-even rule (never more than twice the
    // cost of the better choice in hindsight); a key that proves a handful of times never pays for them
    unsigned table_after = CRS_TABLE_AFTER_DEFAULT;
    // (Round 6 tried an adaptive rule -- build at the second hit when the caller leaves the GPU idle most of the time, as the
    // unchanged examples do -- and measured a LOSS on `hadamard 20`: 7 more of its 126 G1 MSMs ran over copies, but the two
    // background builds ran beside its foreground kernels: msm_g1 76.8-79.6 -> 82.3-86.3 ms.  The break-even rule stays.)
    std::vector<void *> garbage;                    // device buffers to free once the device is idle
} g_crs;

StageBuf g_stage_prefix_scratch;                    // (staging.h: lsa_shutdown frees it)

void crs_configure_from_env() {
    if (g_crs.mode >= 0) return;
    const char *e = getenv("LSA_CRS_CACHE");
    g_crs.mode = 2;
    if (e) {
        if (e[0] == '0' || !strcmp(e, "off")) g_crs.mode = 0;
        else if (!strcmp(e, "sampled") || e[0] == '1') g_crs.mode = 1;
    }
    if (const char *ta = getenv("LSA_CRS_TABLE_AFTER")) g_crs.table_after = (unsigned)atoi(ta);
    const char *mb = getenv("LSA_CRS_CACHE_MB");
    if (mb && atoll(mb) > 0) g_crs.budget = (size_t)atoll(mb) << 20;
    if (g_crs.budget == 0) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) tot = (size_t)64 << 30;
        g_crs.budget = std::min<size_t>(tot / 4, (size_t)64 << 30);
    }
}

size_t bases_device_bytes(const lsa_bases *b) {
    size_t per = msm_base_bytes(b->group);
    return b->n * per * (b->table_stride ? msm_table_windows(b->group, b->n) : 1);
}

// The one way an entry goes.  No MSM may still read it; a build in flight is cancelled and waited for (it reads the
// entry's bases).  Returns the entry after it.
std::list<CrsEntry>::iterator crs_drop(std::list<CrsEntry>::iterator it) {
    CrsEntry &e = *it;
    (void)msm_join(g.stream);
    (void)hipStreamSynchronize(g.stream);
    g_crs.bytes -= e.bytes;
    if (e.build) {
        e.build->cancel.store(true);
        while (e.build->state.load() == 0) std::this_thread::sleep_for(std::chrono::microseconds(50));
        if (e.build->state.load() == 1) {              // complete but never adopted
            if (e.build->big) (void)hipFree(e.build->big);
            if (e.build->tmp) (void)hipFree(e.build->tmp);
        }
    }
    if (e.small) (void)hipFree(e.small);
    if (e.prefix) (void)hipFree(e.prefix);
    lsa_bases_destroy(e.b);
    return g_crs.entries.erase(it);
}

void crs_evict_to(size_t budget) {
    while (g_crs.bytes > budget && !g_crs.entries.empty()) crs_drop(crs_lru_victim(g_crs.entries.begin(), g_crs.entries.end()));
}

// evicts least-recently-used entries beyond the budget, never the entry with tick `keep`
void crs_trim(uint64_t keep) {
    while (g_crs.bytes > g_crs.budget && g_crs.entries.size() > 1) {
        const auto victim = crs_lru_victim(g_crs.entries.begin(), g_crs.entries.end(), keep);
        if (victim == g_crs.entries.end()) break;
        crs_drop(victim);
    }
}

// Background build of an entry's pre-shifted copies.  After `table_after` hits the entry's build is handed to the
// builder thread (allocation, copy 0, the 25 shift + normalise steps -- all off this thread): this MSM and the
// following ones keep using the plain layout.  Once the build has finished, the handle switches to the table (the
// plain buffer is kept until the entry goes: an MSM queued earlier may still read it).
int crs_table_progress(CrsEntry &e) {
    lsa_bases *b = e.b;
    if (b->table_stride || b->n < msm_merge_min() || msm_precompute_off() || g_crs.table_after == 0) return LSA_OK;
    if (e.build) {
        const int st = e.build->state.load();
        if (st == 0) return LSA_OK;                                    // not yet
        if (st == 1) {
            e.small = b->d_aff;
            b->d_aff = e.build->big;
            b->table_stride = b->n;
            g_crs.garbage.push_back(e.build->tmp);
            e.bytes += bases_device_bytes(b);                          // the plain copy stays resident too
            g_crs.bytes += bases_device_bytes(b);
        }
        e.build.reset();                                               // a failed build (no memory) leaves a plain entry
        return LSA_OK;
    }
    if (e.hits < g_crs.table_after || e.build_attempts >= 2) return LSA_OK;              // (no endless retries after a failed build)
    e.build_attempts++;
    const size_t tw = msm_table_windows(b->group, b->n);
    if ((uint64_t)b->n * tw >= (1u << 30)) return LSA_OK;
    auto j = std::make_shared<TableBuild>();
    j->bases = b->d_aff; j->n = b->n; j->group = b->group;
    e.build = j;
    g_crs.builder.submit(j);
    return LSA_OK;
}

// The one way a large request is served by a resident entry.  rekey_to: the entry follows the vector to this address.
int crs_serve_hit(CrsEntry &e, const void *rekey_to, CrsEntry **out) {
    if (rekey_to) e.ptr = rekey_to;
    e.tick = ++g_crs.tick;
    e.hits++;
    g_crs.hits++;
    if (!e.b->table_stride) {                         // re-used: worth the pre-shifted copies -- built in the background
        int rc = crs_table_progress(e);
        if (rc) return rc;
    }
    crs_trim(e.tick);
    *out = &e;
    return LSA_OK;
}

// The copies of the first points of a G1 entry that has no full table (yet): CPPoly::prove asks for MSMs over prefixes
// 2^(d-1) .. 1 of its key vector (src/gadgets/poly.h:76-88) and most of those calls are small.  On the plain layout
// such an MSM is 0.9 ms (a fold over 127 dependent doublings, ~25 launches); over copies of the prefix it takes the
// four-launch pipeline of msm_compact.hip.  One kernel, ~1.2 ms, on lsa_stream() ahead of the MSM that asked for it;
// paid back by the second small call.  LSA_CRS_PREFIX_TABLE=0 turns it off.
size_t crs_prefix_max() {
    static const size_t v = [] {
        const char *e = getenv("LSA_CRS_PREFIX_TABLE");
        const size_t want = e ? (size_t)atoll(e) : (size_t)1 << 16;
        return want > ((size_t)1 << 16) ? (size_t)1 << 16 : want;
    }();
    return v;
}
// G2 entries (CommScheme::commit's second MSM, src/prototools/commit.h:155; InterpCommScheme::commit, src/gadgets/lipmaa.cc:27)
// get theirs at the SECOND request that could use one (LSA_CRS_PREFIX_AFTER_G2 requests are served from the plain layout
// first; the G2 builder's 255 Fq2 doublings per point are ~3x the G1 kernel, and a vector used once never pays for them).
unsigned crs_prefix_after_g2() {
    static const unsigned v = [] { const char *e = getenv("LSA_CRS_PREFIX_AFTER_G2"); return e ? (unsigned)atoi(e) : 1u; }();
    return v;
}
int crs_prefix_table(CrsEntry &e, size_t n_req, const void **d_bases, size_t *stride) {
    const lsa_bases *b = e.b;
    const int grp = b->group;
    if (b->table_stride || n_req == 0 || n_req > crs_prefix_max() || n_req > (grp == 1 ? msm_compact_max() : msm_compact_max_g2()) ||
        msm_precompute_off() || msm_merge_min_is_explicit())
        return LSA_OK;
    if (!e.prefix) {
        if (grp == 2 && e.prefix_asks++ < crs_prefix_after_g2()) return LSA_OK;
        const size_t pn = std::min(e.n, crs_prefix_max());
        const size_t bytes = (size_t)msm_table_windows(grp, pn) * pn * msm_base_bytes(grp);
        void *t = nullptr;
        if (hipMalloc(&t, bytes) != hipSuccess) { (void)hipGetLastError(); return LSA_OK; }          // no memory: the plain layout serves
        if (g_stage_prefix_scratch.ensure(table_build_scratch_bytes(pn, grp))) { (void)hipFree(t); return LSA_OK; }
        if (hipMemcpyAsync(t, b->d_aff, pn * msm_base_bytes(grp), hipMemcpyDeviceToDevice, g.stream) != hipSuccess) {
            set_error("crs_prefix_table: copy failed: %s", hipGetErrorString(hipGetLastError()));
            (void)hipFree(t);
            return LSA_ERR_HIP;
        }
        const int rc = grp == 1 ? table_build_g1_device(t, pn, pn, g_stage_prefix_scratch.p, g.stream)
                                : table_build_g2_device(t, pn, pn, g_stage_prefix_scratch.p, g.stream);
        if (rc) { (void)hipStreamSynchronize(g.stream); (void)hipFree(t); return rc; }
        e.prefix = t;
        e.prefix_n = pn;
        e.bytes += bytes;
        g_crs.bytes += bytes;
    }
    if (n_req <= e.prefix_n) { *d_bases = e.prefix; *stride = e.prefix_n; }
    return LSA_OK;
}

}  // namespace

bool crs_wanted(size_t n) {
    crs_configure_from_env();
    return g_crs.mode != 0 && n >= CRS_MIN_POINTS;
}

void crs_fingerprint_begin(const void *bases_jac, size_t n, size_t point_bytes) {
    if (g_crs.mode != 2) return;
    g_crs.scratch_fp.resize((n + CRS_UNIT_POINTS - 1) / CRS_UNIT_POINTS);
    g_crs.pool.begin(bases_jac, n * point_bytes, CRS_UNIT_POINTS * point_bytes, CRS_TASK_UNITS, g_crs.scratch_fp.data());
}
void crs_fingerprint_finish() {
    if (g_crs.mode == 2) g_crs.pool.finish();
}

int crs_lookup_or_insert(const void *bases_jac, size_t n, int group, CrsEntry **out, bool *hit) {
    const size_t psz = group == 1 ? sizeof(Jac<Fq>) : sizeof(Jac<Fq2>);
    const size_t nun = (n + CRS_UNIT_POINTS - 1) / CRS_UNIT_POINTS;
    const std::vector<uint64_t> &fp = g_crs.scratch_fp;
    *hit = false;
    for (auto &e : g_crs.entries) {
        if (e.ptr != bases_jac || e.group != group || e.n < n) continue;
        bool same = true;
        if (g_crs.mode == 2) {
            if (!crs_comparable(e.n, n)) continue;
            for (size_t u = 0; u < nun && same; u++) same = fp[u] == e.unit_fp[u];
        } else {
            for (size_t k = 0; k < e.sample_pos.size() && same; k++) {
                size_t i = e.sample_pos[k];
                if (i >= n) continue;
                same = memcmp((const uint8_t *)bases_jac + i * psz, e.sample.data() + k * psz, psz) == 0;
            }
        }
        if (!same) continue;
        *hit = true;
        return crs_serve_hit(e, nullptr, out);
    }
    // Not under this pointer -- but maybe under another one: the reference hands multiExpMA COPIES of its key vectors
    // (CommScheme::getBases1() returns g1s by value, src/prototools/commit.h:145-147, and CPPoly::prove
    // calls it once per proof, src/gadgets/poly.h:73), so the same bytes arrive at a new address with every proof.
    // With full fingerprints the cache is content-addressed: an entry of the same group whose unit fingerprints equal
    // the request's is the same vector (or, prefix rule as above, starts with it); it is re-keyed to the new pointer.
    if (g_crs.mode == 2) {
        for (auto &e : g_crs.entries) {
            if (e.group != group || e.ptr == bases_jac || !crs_comparable(e.n, n)) continue;
            if (memcmp(fp.data(), e.unit_fp.data(), nun * sizeof(uint64_t)) != 0) continue;
            *hit = true;                              // a whole-vector match follows the copy; a prefix match leaves the entry where it is
            return crs_serve_hit(e, e.n == n ? bases_jac : nullptr, out);
        }
    }
    // miss: drop stale entries for this pointer, upload + normalise (no table yet), insert
    for (auto it = g_crs.entries.begin(); it != g_crs.entries.end();) {
        if (it->ptr == bases_jac && it->group == group && it->n <= n) it = crs_drop(it);
        else ++it;
    }
    g_crs.misses++;
    CrsEntry e;
    e.ptr = bases_jac; e.n = n; e.group = group;
    int rc = bases_create_plain(bases_jac, n, group, &e.b);
    if (rc) return rc;
    if (g_crs.mode == 2) {
        e.unit_fp.assign(fp.begin(), fp.begin() + nun);
        const size_t head = n < CRS_UNIT_POINTS ? n : CRS_UNIT_POINTS;
        e.head_fp.resize(head);
        for (size_t i = 0; i < head; i++) e.head_fp[i] = hash_words((const uint64_t *)((const uint8_t *)bases_jac + i * psz), psz / 8);
    } else {
        e.sample_pos = sample_positions(n);
        e.sample.resize(e.sample_pos.size() * psz);
        for (size_t k = 0; k < e.sample_pos.size(); k++) memcpy(e.sample.data() + k * psz, (const uint8_t *)bases_jac + e.sample_pos[k] * psz, psz);
    }
    e.bytes = bases_device_bytes(e.b);
    e.tick = ++g_crs.tick;
    g_crs.bytes += e.bytes;
    g_crs.entries.push_back(std::move(e));
    *out = &g_crs.entries.back();
    crs_trim((*out)->tick);
    return LSA_OK;
}

// Vectors below CRS_MIN_POINTS are not worth an entry of their own -- but the reference asks for them as PREFIXES of its
// key vector: CPPoly::prove's ladder ends with multiExpMA(g1s, 512 .. 1 scalars) (src/gadgets/poly.h:77-86, globl.h:66).
// Such a request is looked up (never inserted): whole 64-point units against the entries' unit fingerprints, fewer than
// 64 points against the per-point fingerprints of an entry's first unit.  A hit saves the upload and normalisation of
// the points and runs on the entry's pre-shifted copies when it has them (0.3 ms instead of 0.9-1.0 for an MSM this small:
// no fold over 127 doublings).  Every byte the request covers is verified, as for large vectors.
// Not through crs_serve_hit, on purpose: a small hit does not count towards the entry's table (no e.hits++), never trims
// (nothing was inserted), and a table step that fails makes it no hit instead of an error.
CrsEntry *crs_lookup_small(const void *bases_jac, size_t n, int group) {
    if (g_crs.mode != 2 || g_crs.entries.empty()) return nullptr;
    const size_t psz = group == 1 ? sizeof(Jac<Fq>) : sizeof(Jac<Fq2>);
    bool by_point = false;
    const size_t cnt = crs_small_fingerprints(n, &by_point);
    if (cnt == 0) return nullptr;
    const uint8_t *p = (const uint8_t *)bases_jac;
    uint64_t fp[CRS_MIN_POINTS / CRS_UNIT_POINTS > CRS_UNIT_POINTS ? CRS_MIN_POINTS / CRS_UNIT_POINTS : CRS_UNIT_POINTS];
    for (size_t i = 0; i < cnt; i++)
        fp[i] = by_point ? hash_words((const uint64_t *)(p + i * psz), psz / 8)
                         : hash_words((const uint64_t *)(p + i * CRS_UNIT_POINTS * psz), CRS_UNIT_POINTS * psz / 8);
    for (auto &e : g_crs.entries) {
        if (e.group != group || e.n <= n) continue;
        const std::vector<uint64_t> &have = by_point ? e.head_fp : e.unit_fp;
        if (have.size() < cnt || memcmp(fp, have.data(), cnt * sizeof(uint64_t)) != 0) continue;
        e.tick = ++g_crs.tick;
        g_crs.hits++;
        if (!e.b->table_stride && crs_table_progress(e) != LSA_OK) return nullptr;      // (a finished build switches the entry)
        return &e;
    }
    return nullptr;
}

int crs_bases_for(CrsEntry *e, size_t n, const void **d_bases, size_t *table_stride, lsa_host_stats &st) {
    const lsa_bases *b = e->b;
    st.table = b->table_stride ? 1 : 0;
    st.table_building = e->building() ? 1 : 0;
    *d_bases = b->d_aff;
    *table_stride = b->table_stride;
    const int rc = crs_prefix_table(*e, n, d_bases, table_stride);
    if (rc) return rc;
    if (*table_stride && !b->table_stride) st.table = 2;              // the entry's prefix table
    return LSA_OK;
}

void crs_after_drain() {
    for (void *p : g_crs.garbage) (void)hipFree(p);
    g_crs.garbage.clear();
}

void crs_shutdown() {
    crs_evict_to(0);
    crs_after_drain();
    g_crs.builder.shutdown();
    g_crs.pool.stop();
    g_crs.bytes = 0;
}

}  // namespace lsa

using namespace lsa;

extern "C" {
int lsa_crs_cache_configure(int mode, size_t max_bytes) {
    int rc = require_ready();
    if (rc) return rc;
    if (mode < 0 || mode > 2) { set_error("crs_cache_configure: mode must be 0 (off), 1 (sampled) or 2 (full)"); return LSA_ERR_INVALID; }
    crs_configure_from_env();
    if (mode != g_crs.mode) crs_evict_to(0);          // fingerprints of the two modes are not comparable
    g_crs.mode = mode;
    if (max_bytes) g_crs.budget = max_bytes;
    crs_evict_to(g_crs.budget);
    return LSA_OK;
}
void lsa_crs_cache_clear(void) { if (g.ready) crs_evict_to(0); }
int lsa_crs_cache_stats(uint64_t *hits, uint64_t *misses, uint64_t *resident_bytes, uint64_t *entries) {
    if (hits) *hits = g_crs.hits;
    if (misses) *misses = g_crs.misses;
    if (resident_bytes) *resident_bytes = g_crs.bytes;
    if (entries) *entries = g_crs.entries.size();
    return LSA_OK;
}
int lsa_crs_cache_table_after(unsigned hits) {
    crs_configure_from_env();
    g_crs.table_after = hits;
    return LSA_OK;
}
// blocks until every background table build has finished and its entry has switched (tests, benchmarks)
int lsa_crs_cache_wait_tables(void) {
    int rc = require_ready();
    if (rc) return rc;
    for (auto &e : g_crs.entries) {
        if (!e.build) continue;
        while (e.build->state.load() == 0) std::this_thread::sleep_for(std::chrono::microseconds(100));
        rc = crs_table_progress(e);
        if (rc) return rc;
    }
    return LSA_OK;
}
}  // extern "C"
