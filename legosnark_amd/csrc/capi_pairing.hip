// legosnark_amd/csrc/capi_pairing.hip -- the pairing entry points of the C-ABI (include/legosnark_amd.h).
//
// Every entry point is one shape of the same job: n terms (P_i, Q_i), grouped into products, each
// product optionally followed by a final exponentiation.  Q_i arrives either as a point (libff
// precompute_G2 is then done here) or as libff's alt_bn128_ate_G2_precomp bytes (lsa_g2_precompute),
// the form the reference's keys hold and re-use in every verification
// (/root/reference/src/gadgets/subspace.cc:48,66-70,152-166; src/gadgets/lipmaa.h:95-96;
// src/gadgets/poly.h:97-121).  The device works on line tables (tmiller.h): a table is built once per
// distinct Q, kept resident in a cache keyed by a 128-bit fingerprint of the bytes the caller passed (the
// point, or the precomp blob), and every Miller loop over it runs the Fq12 chain only.  Products share
// accumulators (f <- f^2 * prod line_i) when there are more pairs than the chip has lanes for.
// No CPU arithmetic: the host only fingerprints, deduplicates and lays out index arrays.
//
// What is a pure function of host data lives in two headers that the host tests compile without HIP:
//   pairing_plan.h    -- plan_pairing: the route of a job, M, the accumulators and the layout of its pinned index block
//                        (tests/cpp/test_pairing_plan.cc);
//   g2_table_index.h  -- the cache's rules: keys, slots, LRU with pinned slots, the call guard, the promises of a
//                        prefetch (tests/cpp/test_g2_table_index.cc).
// This file owns the device memory behind the slots, the staging buffers and the order of the launches.
// (These entry points do not go through OperandFrame, staging.h: their operands are one pinned index block per call and
// the on_device calls return without synchronising, which a frame of per-operand copies does not express.)
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <unordered_map>
#include <vector>

#include "capi_internal.h"
#include "g2_table_index.h"
#include "pairing_plan.h"
#include "tower.h"

namespace lsa {
// pairing.hip
size_t g2_table_words();
size_t g2_precomp_public_bytes();
int g2_precomp_device(const void *d_g2, size_t n, uint32_t *const *d_tabs, hipStream_t st);
int g2_table_export_device(const uint32_t *const *d_tabs, size_t n, void *d_public, hipStream_t st);
int g2_table_import_device(const void *d_public, size_t n, uint32_t *const *d_tabs, hipStream_t st);
int g2_table_identity_device(uint32_t *d_tab, hipStream_t st);
unsigned miller_tab_max_pairs();
void miller_split_release();
int miller_tab_device(const void *d_g1, const uint32_t *const *d_tabs, const uint8_t *d_flags, const uint32_t *d_acc_off, size_t nacc, unsigned M,
                      const uint32_t *d_ident, void *d_out, hipStream_t st);
int miller_fused_device(const void *d_g1, const void *d_g2, const uint8_t *d_flags, uint32_t *const *d_tabs, size_t n, void *d_out, hipStream_t st, bool gt_only);
}  // namespace lsa

using namespace lsa;

namespace {

static_assert(sizeof(Jac<Fq>) == PAIRING_G1_BYTES, "pairing_plan.h lays out the inline G1 points of a job");

StageBuf g_pair_p, g_pair_q, g_pair_f, g_pair_s, g_pair_o;     // points, Miller values, product scratch, results
StageBuf g_pair_meta, g_pair_scratch_tabs, g_pair_pub;         // index arrays, uncached tables, public-form staging

// Pinned host staging for the small arrays of a call (one H2D copy each), and the one rule about it: a pinned block is
// not rewritten before its copy has run.  An on_device call returns without synchronising, so mark() records an event
// after the uploads of a call and wait() waits for it before the next call writes.
struct PinnedStaging {
    struct Buf {
        void *p = nullptr;
        size_t cap = 0;
        int ensure(size_t bytes) {
            if (bytes <= cap) return 0;
            if (p) { (void)hipStreamSynchronize(g.stream); (void)hipHostFree(p); }
            p = nullptr; cap = 0;
            size_t want = bytes < 65536 ? 65536 : bytes + bytes / 4;
            if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr; return -1; }
            cap = want;
            return 0;
        }
        void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    };
    Buf meta, q;                           // the index block of a call; points and destinations of the tables to build
    hipEvent_t uploaded = nullptr;
    bool pending = false;
    int wait() {
        if (pending) { HIPCHK(hipEventSynchronize(uploaded)); pending = false; }
        return LSA_OK;
    }
    int mark() {
        if (!uploaded) HIPCHK(hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
        HIPCHK(hipEventRecord(uploaded, g.stream));
        pending = true;
        return LSA_OK;
    }
    void release() {
        meta.release(); q.release();
        if (uploaded) { (void)hipEventDestroy(uploaded); uploaded = nullptr; }
        pending = false;
    }
} g_pin;

// ---------------------------------------------------------------- G2 line-table cache: the device memory behind
// the slots of g2_table_index.h
struct TableCache {
    static constexpr size_t BLOCK = 128;                  // tables per device allocation
    G2TableIndex ix;                                      // capacity: LSA_G2_TABLES / lsa_g2_table_cache
    std::vector<void *> blocks;
    uint32_t *ident = nullptr;                            // the table of a pair that is not there
    bool env_read = false;

    uint32_t *ptr(uint32_t slot) const { return (uint32_t *)((char *)blocks[slot / BLOCK] + (size_t)(slot % BLOCK) * g2_table_words() * 4); }
    void read_env() {
        if (env_read) return;
        env_read = true;
        if (const char *e = getenv("LSA_G2_TABLES")) ix.set_capacity((size_t)strtoull(e, nullptr, 10));
    }
    int ensure_ident() {
        if (ident) return 0;
        if (hipMalloc((void **)&ident, g2_table_words() * 4) != hipSuccess) { ident = nullptr; return -1; }
        return g2_table_identity_device(ident, g.stream);
    }
    // ix.insert with memory behind the slot: the block of a slot the index is about to create is allocated BEFORE the key
    // enters the map, so a failed allocation is a plain miss (-1)
    long insert(const Key128 &key, bool pending = false) {
        if (ix.slot_to_create() == (long)(blocks.size() * BLOCK)) {
            void *b = nullptr;
            if (hipMalloc(&b, BLOCK * g2_table_words() * 4) != hipSuccess) { (void)hipGetLastError(); return -1; }
            blocks.push_back(b);
        }
        return ix.insert(key, pending);
    }
    void clear() {
        for (void *b : blocks) (void)hipFree(b);
        blocks.clear();
        ix.clear();
        if (ident) (void)hipFree(ident);
        ident = nullptr;
    }
} g_tabs;

// Tables lsa_g2_tables_prefetch has promised (g_tabs.ix.promised: their slots are taken, their keys resolve) but not yet
// built: built when a Miller call arrives or when `batch()` of them are waiting, whichever is first (ix.flush_due) --
// always before anything on lsa_stream() can read them.  One wavefront of k_g2_precomp holds five points and takes as
// long (0.65 ms) for five as for one; further wavefronts run beside it.  A verifier that derives twenty G2 points one
// after the other (CPPoly::verify, src/gadgets/poly.h:115-118) spends 0.45 ms of host time on them since the fixed-base
// tables of round 5, so ONE launch of four workgroups when its Miller call arrives (0.65 ms) beats four launches of one
// queued behind each other (2.6 ms: the round-4 setting, LSA_G2_PREFETCH_BATCH=5, which paid when a product took
// 0.27 ms of host time).
struct PendingTables {
    std::vector<Jac<Fq2>> pts;             // the points of g_tabs.ix.promised, in its order
    StageBuf dev;
    static size_t batch() {
        static const size_t b = G2TableIndex::clamp_batch(getenv("LSA_G2_PREFETCH_BATCH") ? atol(getenv("LSA_G2_PREFETCH_BATCH")) : 60);
        return b;
    }
    int build(const std::vector<char> &h, size_t m) {
        if (dev.ensure(h.size())) { set_error("g2_tables_prefetch: staging allocation failed"); return LSA_ERR_NOMEM; }
        LSA_UPLOAD(dev.p, h.data(), h.size());
        return g2_precomp_device(dev.p, m, (uint32_t *const *)((const char *)dev.p + m * sizeof(Jac<Fq2>)), g.stream);
    }
    int flush() {
        const size_t m = pts.size();
        if (m == 0) return LSA_OK;
        std::vector<char> h(m * (sizeof(Jac<Fq2>) + 8));
        memcpy(h.data(), pts.data(), m * sizeof(Jac<Fq2>));
        for (size_t k = 0; k < m; k++) {
            const uint64_t dst = (uint64_t)(uintptr_t)g_tabs.ptr(g_tabs.ix.promised[k].slot);
            memcpy(h.data() + m * sizeof(Jac<Fq2>) + k * 8, &dst, 8);
        }
        pts.clear();
        const int rc = build(h, m);
        g_tabs.ix.settle_promises(rc == LSA_OK);
        return rc;
    }
    void drop() { pts.clear(); g_tabs.ix.promised.clear(); }
} g_pending;

// ---------------------------------------------------------------- one job description
struct Terms {
    const void *g1 = nullptr;              // n Jacobian G1 points
    const void *g2 = nullptr;              // n Jacobian G2 points, or null
    const void *const *qpre = nullptr;     // n pointers to LSA_G2_PRECOMP_BYTES blobs (a null entry: use g2[i]), or null
    const uint8_t *flags = nullptr;        // bit 0: conjugate the term (libff unitary_inverse of its Miller value)
    const uint64_t *seg = nullptr;         // nseg + 1 offsets; null: every term is its own product
    size_t n = 0, nseg = 0;
    bool on_device = false;                // g1 / g2 are device pointers (no cache: nothing to fingerprint on the host)
    bool gt_only = false;                  // every value of this job goes through a final exponentiation before it leaves: Miller
                                           // values may differ from libff's by factors the final exponent kills (signed-digit loop)
};

unsigned g_force_m = 0;                    // lsa_pairing_set_chunk: pairs per accumulator, 0 = by batch size
inline int force_kernel() {
    static const int f = getenv("LSA_MILLER_KERNEL") ? atoi(getenv("LSA_MILLER_KERNEL")) : 0;   // 3: one lane per pairing (miller.h), 5: tables, 6: fused
    return f;
}

PairingShape shape_of(const Terms &t) {
    PairingShape s;
    s.n = t.n; s.seg = t.seg; s.nseg = t.nseg;
    s.flags = t.flags != nullptr; s.blobs = t.qpre != nullptr; s.on_device = t.on_device;
    s.force_m = g_force_m; s.force_kernel = force_kernel();
    s.capacity = g_tabs.ix.capacity; s.max_pairs = miller_tab_max_pairs();
    return s;
}

// ---------------------------------------------------------------- the pieces every route shares
// the points of a host job on the device (d_q null: the route does not read the G2 points as a whole)
int points_on_device(const Terms &t, const void **d_p, const void **d_q) {
    *d_p = t.g1;
    if (d_q) *d_q = t.g2;
    if (t.on_device) return LSA_OK;
    const size_t room = std::max<size_t>(t.n, 1);
    if (g_pair_p.ensure(room * sizeof(Jac<Fq>)) || (d_q && g_pair_q.ensure(room * sizeof(Jac<Fq2>)))) { set_error("pairing: hipMalloc failed"); return LSA_ERR_NOMEM; }
    if (t.n) {
        LSA_UPLOAD(g_pair_p.p, t.g1, t.n * sizeof(Jac<Fq>));
        if (d_q) LSA_UPLOAD(g_pair_q.p, t.g2, t.n * sizeof(Jac<Fq2>));
    }
    *d_p = g_pair_p.p;
    if (d_q) *d_q = g_pair_q.p;
    return LSA_OK;
}

// values -> products: g_pair_f holds nval values, product j is the product of the values [d_off[j], d_off[j+1]);
// one_each: the values ARE the products.  (d_off is not read for a single product.)
int products(size_t nval, bool one_each, const uint64_t *d_off, size_t nprod, void **d_res) {
    if (one_each) { *d_res = g_pair_f.p; return LSA_OK; }
    if (g_pair_s.ensure((nprod == 1 ? (nval + 7) / 8 + 1 : nprod) * fq12_bytes())) { set_error("pairing: hipMalloc failed"); return LSA_ERR_NOMEM; }
    if (nprod == 1 && nval) return fq12_product_device(g_pair_f.p, g_pair_s.p, nval, d_res, g.stream);
    *d_res = g_pair_s.p;
    if (nprod == 1) {                      // the empty product
        Fq12 one = Fq12::one();
        HIPCHK(hipMemcpyAsync(g_pair_s.p, &one, sizeof one, hipMemcpyHostToDevice, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
        return LSA_OK;
    }
    return fq12_segment_products_device(g_pair_f.p, d_off, nprod, g_pair_s.p, g.stream);
}

// one Fq12 to the caller through the pinned mirror g.h_result (d_val null: a kernel has written it there already)
int one_to_host(const void *d_val, void *out) {
    if (d_val) HIPCHK(hipMemcpyAsync(g.h_result, d_val, fq12_bytes(), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    memcpy(out, g.h_result, fq12_bytes());
    return LSA_OK;
}

// ---------------------------------------------------------------- the routes
// The job through the fused kernel (pairing.hip, k_miller_fused: G2 arithmetic and Fq12 chain side by side in one
// workgroup, one Miller value per term), then the products.  fill_tables: the caller has resolved the job and left, per
// term, the device table to fill on the way (0: none) at pl.off_tab of the pinned block -- the tables of points seen
// for the first time go into the cache while their first loop runs.
int run_fused(const Terms &t, const PairingShape &sh, const PairingPlan &pl, bool fill_tables, void **d_res) {
    int rc = g_pin.wait();
    if (rc) return rc;
    if (g_pin.meta.ensure(pl.meta_bytes) || g_pair_meta.ensure(pl.meta_bytes) || g_pair_f.ensure(std::max<size_t>(t.n, 1) * fq12_bytes())) {
        set_error("pairing: staging allocation failed");
        return LSA_ERR_NOMEM;
    }
    pl.fill(sh, t.flags, (char *)g_pin.meta.p);
    const void *d_p, *d_q;
    rc = points_on_device(t, &d_p, &d_q);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(g_pair_meta.p, g_pin.meta.p, pl.meta_bytes, hipMemcpyHostToDevice, g.stream));
    rc = g_pin.mark();
    if (rc) return rc;
    const char *dm = (const char *)g_pair_meta.p;
    rc = miller_fused_device(d_p, d_q, (const uint8_t *)(dm + pl.off_flag), fill_tables ? (uint32_t *const *)(dm + pl.off_tab) : nullptr, t.n, g_pair_f.p, g.stream, t.gt_only);
    if (rc) return rc;
    return products(t.n, !t.seg, (const uint64_t *)(dm + pl.off_prod), pl.nprod, d_res);
}

// the one-lane-per-pairing kernel of miller.h
int run_one_lane(const Terms &t, void **d_res) {
    const void *d_p, *d_q;
    int rc = points_on_device(t, &d_p, &d_q);
    if (rc) return rc;
    if (g_pair_f.ensure(std::max<size_t>(t.n, 1) * fq12_bytes())) { set_error("pairing: hipMalloc failed"); return LSA_ERR_NOMEM; }
    rc = miller_device(d_p, d_q, t.n, g_pair_f.p, g.stream);
    if (rc) return rc;
    if (t.seg && t.nseg > 1) {
        if (g_pair_meta.ensure((t.nseg + 1) * sizeof(uint64_t))) { set_error("pairing: hipMalloc failed"); return LSA_ERR_NOMEM; }
        LSA_UPLOAD(g_pair_meta.p, t.seg, (t.nseg + 1) * sizeof(uint64_t));
        HIPCHK(hipStreamSynchronize(g.stream));     // t.seg is pageable caller memory
    }
    return products(t.n, !t.seg, (const uint64_t *)g_pair_meta.p, t.nseg, d_res);
}

// Tables, stage 2: a device table for every term into h_tab; the terms whose table has to be computed from the point
// (need_pre) or imported from a precomp blob (need_imp).  The only code that talks to the index during a call.
int resolve_tables(const Terms &t, const PairingPlan &pl, uint64_t *h_tab, std::vector<uint32_t> &need_pre, std::vector<uint32_t> &need_imp) {
    const size_t n = t.n, TW = g2_table_words(), PUB = g2_precomp_public_bytes();
    // every term is validated BEFORE the cache is touched: a call that fails half-way must not leave keys behind
    for (size_t i = 0; i < n; i++)
        if (!(t.qpre && t.qpre[i]) && !t.g2) { set_error("pairing: term %zu has neither a point nor a precomputed table", i); return LSA_ERR_INVALID; }
    // Equal keys within the call share one table.  With the cache the key is the fingerprint; without it blobs are
    // keyed by their POINTER (verifyLin3or4 scaled up: 2^16 terms over a handful of key blobs are a handful of tables)
    // and points are not compared at all.
    std::unordered_map<Key128, uint64_t, Key128Hash> seen;
    auto key_of = [&](size_t i, const void *blob) {
        if (!pl.use_cache) return Key128{(uint64_t)(uintptr_t)blob, 0};
        return blob ? g2_fingerprint(blob, PUB, 2) : g2_fingerprint((const char *)t.g2 + i * sizeof(Jac<Fq2>), sizeof(Jac<Fq2>), 1);
    };
    // uncached terms take scratch tables: sized first (the scratch buffer must not move afterwards).  With the cache: at
    // worst all n (the cache full of this call's own tables, n <= 1024); without: one per point term and one per
    // distinct blob, entered into `seen` without a table yet
    size_t scratch_need = pl.scratch_max, scratch_used = 0;
    if (!pl.use_cache && t.qpre) {
        scratch_need = 0;
        for (size_t i = 0; i < n; i++)
            if (!t.qpre[i] || seen.emplace(key_of(i, t.qpre[i]), 0).second) scratch_need++;
    }
    if (g_pair_scratch_tabs.ensure(std::max<size_t>(scratch_need, 1) * TW * 4)) { set_error("pairing: table scratch allocation failed"); return LSA_ERR_NOMEM; }
    for (size_t i = 0; i < n; i++) {
        const void *blob = t.qpre ? t.qpre[i] : nullptr;
        const bool shared = pl.use_cache || blob;
        const Key128 key = key_of(i, blob);
        if (shared) {
            auto it = seen.find(key);
            if (it != seen.end() && it->second) { h_tab[i] = it->second; continue; }
        }
        long s = pl.use_cache ? g_tabs.ix.lookup(key) : -1;
        if (s < 0) {
            if (pl.use_cache) s = g_tabs.insert(key);
            (blob ? need_imp : need_pre).push_back((uint32_t)i);
        }
        h_tab[i] = (uint64_t)(uintptr_t)(s >= 0 ? g_tabs.ptr((uint32_t)s) : (uint32_t *)g_pair_scratch_tabs.p + scratch_used++ * TW);
        if (shared) seen[key] = h_tab[i];
    }
    return LSA_OK;
}

// Tables, stage 5: the tables of need_pre computed from their points, those of need_imp imported from their blobs
int build_missing(const Terms &t, const PairingPlan &pl, const uint64_t *h_tab, const std::vector<uint32_t> &need_pre, const std::vector<uint32_t> &need_imp) {
    const size_t PUB = g2_precomp_public_bytes();
    if (!need_pre.empty()) {
        const size_t m = need_pre.size();
        const void *d_q = t.g2;                                                              // on the device: all of them, in place
        const uint32_t *const *d_tp = (const uint32_t *const *)((const char *)g_pair_meta.p + pl.off_tab);
        if (t.on_device && m != t.n) { set_error("pairing: internal (device points need tables for all terms)"); return LSA_ERR_INVALID; }
        if (!t.on_device) {
            // the points and the destination pointers of the misses, gathered into pinned staging
            if (g_pin.q.ensure(m * (sizeof(Jac<Fq2>) + 8)) || g_pair_q.ensure(m * (sizeof(Jac<Fq2>) + 8))) { set_error("pairing: staging allocation failed"); return LSA_ERR_NOMEM; }
            char *hq = (char *)g_pin.q.p;
            uint64_t *hp = (uint64_t *)(hq + m * sizeof(Jac<Fq2>));
            for (size_t k = 0; k < m; k++) {
                memcpy(hq + k * sizeof(Jac<Fq2>), (const char *)t.g2 + (size_t)need_pre[k] * sizeof(Jac<Fq2>), sizeof(Jac<Fq2>));
                hp[k] = h_tab[need_pre[k]];
            }
            HIPCHK(hipMemcpyAsync(g_pair_q.p, hq, m * (sizeof(Jac<Fq2>) + 8), hipMemcpyHostToDevice, g.stream));
            d_q = g_pair_q.p;
            d_tp = (const uint32_t *const *)((const char *)g_pair_q.p + m * sizeof(Jac<Fq2>));
        }
        int rc = g2_precomp_device(d_q, m, (uint32_t *const *)d_tp, g.stream);
        if (rc) return rc;
    }
    if (!need_imp.empty()) {
        const size_t m = need_imp.size();
        if (g_pair_pub.ensure(m * (PUB + 8))) { set_error("pairing: staging allocation failed"); return LSA_ERR_NOMEM; }
        std::vector<uint64_t> hp(m);
        for (size_t k = 0; k < m; k++) {
            LSA_UPLOAD((char *)g_pair_pub.p + k * PUB, t.qpre[need_imp[k]], PUB);
            hp[k] = h_tab[need_imp[k]];
        }
        HIPCHK(hipMemcpyAsync((char *)g_pair_pub.p + m * PUB, hp.data(), m * 8, hipMemcpyHostToDevice, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));     // hp is a local
        int rc = g2_table_import_device(g_pair_pub.p, m, (uint32_t *const *)((char *)g_pair_pub.p + m * PUB), g.stream);
        if (rc) return rc;
    }
    return LSA_OK;
}

// Miller products of the job on the device: *d_res points at nseg (or n) Fq12 values when this returns (stream-ordered)
int run_miller(const Terms &t, void **d_res) {
    const size_t n = t.n;
    g_tabs.read_env();
    // ---- 1. plan
    const PairingShape sh = shape_of(t);
    const PairingPlan pl = plan_pairing(sh);
    if (pl.route == ROUTE_FUSED) return run_fused(t, sh, pl, false, d_res);
    if (pl.route == ROUTE_ONE_LANE) return run_one_lane(t, d_res);
    int rc = g_pin.wait();
    if (rc) return rc;
    rc = g_pending.flush();                 // promised tables: on the stream before anything reads them
    if (rc) return rc;
    if (g_tabs.ensure_ident()) { set_error("pairing: hipMalloc failed"); return LSA_ERR_NOMEM; }
    g_tabs.ix.tick++;
    if (g_pin.meta.ensure(pl.meta_bytes) || g_pair_meta.ensure(pl.meta_bytes)) { set_error("pairing: staging allocation failed"); return LSA_ERR_NOMEM; }
    char *hm = (char *)g_pin.meta.p;
    const char *dm = (const char *)g_pair_meta.p;
    uint64_t *h_tab = (uint64_t *)(hm + pl.off_tab);
    pl.fill(sh, t.flags, hm);
    // ---- 2. a device table for every term
    G2TableIndex::CallGuard guard(g_tabs.ix);
    std::vector<uint32_t> need_pre, need_imp;
    rc = resolve_tables(t, pl, h_tab, need_pre, need_imp);
    if (rc) return rc;
    // ---- 3. points seen for the first time and no precomputed tables among the terms: the fused kernel computes every
    // term (while the chip is not full a resident Q gains nothing from its table: the call waits for the new ones
    // anyway) and fills the new tables on the way.  h_tab stays where it is (as_fused) and keeps the new tables only.
    if (pl.may_fill && !need_pre.empty()) {
        for (size_t i = 0, k = 0; i < n; i++) {
            if (k < need_pre.size() && need_pre[k] == i) k++;
            else h_tab[i] = 0;
        }
        rc = run_fused(t, sh, pl.as_fused(n), true, d_res);
        if (rc == LSA_OK) guard.commit();
        return rc;
    }
    // ---- 4. uploads: a handful of host G1 points ride in the index block (one copy command for the whole call)
    const void *d_g1 = dm + pl.off_g1;
    if (pl.g1_in_meta) memcpy(hm + pl.off_g1, t.g1, n * sizeof(Jac<Fq>));
    else if ((rc = points_on_device(t, &d_g1, nullptr))) return rc;
    HIPCHK(hipMemcpyAsync(g_pair_meta.p, hm, pl.meta_bytes, hipMemcpyHostToDevice, g.stream));
    // ---- 5. missing tables
    rc = build_missing(t, pl, h_tab, need_pre, need_imp);
    if (rc) return rc;
    rc = g_pin.mark();
    if (rc) return rc;
    // ---- 6. Miller loops, one Fq12 per accumulator
    if (g_pair_f.ensure(std::max<size_t>(pl.nacc, 1) * fq12_bytes())) { set_error("pairing: hipMalloc failed"); return LSA_ERR_NOMEM; }
    rc = miller_tab_device(d_g1, (const uint32_t *const *)(dm + pl.off_tab), (const uint8_t *)(dm + pl.off_flag), (const uint32_t *)(dm + pl.off_acc), pl.nacc, pl.M,
                           g_tabs.ident, g_pair_f.p, g.stream);
    if (rc) return rc;
    guard.commit();            // every new table is on the stream, ahead of anything that reads it
    // ---- 7. products over the accumulators of each product
    return products(pl.nacc, pl.nacc == pl.nprod, (const uint64_t *)(dm + pl.off_prod), pl.nprod, d_res);
}

// the job with host results: out = nseg (or n) Fq12 values
int run_terms_host(const Terms &t_in, void *out, bool final_exp) {
    LSA_TRACE_CALL("pairing_terms", t_in.n);
    Terms t = t_in;
    t.gt_only = final_exp;
    int rc = require_ready();
    if (rc) return rc;
    const size_t nres = t.seg ? t.nseg : t.n;
    if (nres == 0) return LSA_OK;
    if (!out || (t.n && !t.g1)) { set_error("pairing: null argument"); return LSA_ERR_INVALID; }
    void *res = nullptr;
    rc = run_miller(t, &res);
    if (rc) return rc;
    if (final_exp && nres == 1) {
        // one check = one value: the final exponentiation writes it straight into pinned host memory (no copy command
        // behind the kernel: ~15 us of every blocking check of a verifier written call by call)
        rc = final_exp_device(res, 1, g.h_result, g.stream);
        return rc ? rc : one_to_host(nullptr, out);
    }
    if (final_exp) {
        if (g_pair_o.ensure(nres * fq12_bytes())) { set_error("pairing: hipMalloc failed"); return LSA_ERR_NOMEM; }
        rc = final_exp_device(res, nres, g_pair_o.p, g.stream);
        if (rc) return rc;
        res = g_pair_o.p;
    }
    LSA_DOWNLOAD(out, res, nres * fq12_bytes());
    HIPCHK(hipStreamSynchronize(g.stream));
    return LSA_OK;
}

int check_segments(const uint64_t *seg, size_t nseg, const char *who) {
    if (!seg) { set_error("%s: null argument", who); return LSA_ERR_INVALID; }
    if (seg[0] != 0) { set_error("%s: offsets must start at 0", who); return LSA_ERR_INVALID; }
    for (size_t j = 0; j < nseg; j++)
        if (seg[j + 1] < seg[j]) { set_error("%s: offsets must not decrease", who); return LSA_ERR_INVALID; }
    return LSA_OK;
}

}  // namespace

namespace lsa {
void pairing_release() {
    g_pin.release();                                   // (the StageBufs above: stage_release_all, staging.h)
    g_pending.drop();
    miller_split_release();
    g_tabs.clear();
}
}  // namespace lsa

extern "C" {

size_t lsa_g2_precomp_bytes(void) { return g2_precomp_public_bytes(); }

int lsa_g2_precompute(const void *g2_jac, size_t n, void *out_precomp) {
    LSA_TRACE_CALL("g2_precompute", n);
    int rc = require_ready();
    if (rc) return rc;
    if (n == 0) return LSA_OK;
    if (!g2_jac || !out_precomp) { set_error("g2_precompute: null argument"); return LSA_ERR_INVALID; }
    const size_t TW = g2_table_words(), PUB = g2_precomp_public_bytes();
    if (g_pair_q.ensure(n * sizeof(Jac<Fq2>)) || g_pair_scratch_tabs.ensure(n * TW * 4) || g_pair_pub.ensure(n * PUB) || g_pin.meta.ensure(n * 8) ||
        g_pair_meta.ensure(n * 8)) {
        set_error("g2_precompute: staging allocation failed");
        return LSA_ERR_NOMEM;
    }
    rc = g_pin.wait();
    if (rc) return rc;
    uint64_t *hp = (uint64_t *)g_pin.meta.p;
    for (size_t i = 0; i < n; i++) hp[i] = (uint64_t)(uintptr_t)((uint32_t *)g_pair_scratch_tabs.p + i * TW);
    HIPCHK(hipMemcpyAsync(g_pair_meta.p, hp, n * 8, hipMemcpyHostToDevice, g.stream));
    LSA_UPLOAD(g_pair_q.p, g2_jac, n * sizeof(Jac<Fq2>));
    rc = g2_precomp_device(g_pair_q.p, n, (uint32_t *const *)g_pair_meta.p, g.stream);
    if (rc) return rc;
    rc = g2_table_export_device((const uint32_t *const *)g_pair_meta.p, n, g_pair_pub.p, g.stream);
    if (rc) return rc;
    LSA_DOWNLOAD(out_precomp, g_pair_pub.p, n * PUB);
    HIPCHK(hipStreamSynchronize(g.stream));
    return LSA_OK;
}

// Builds the line tables of points the cache does not hold yet, asynchronously (no host synchronisation): a
// verifier that derives its G2 points one after the other on the host (CPPoly::verify: pts[i] * g2,
// /root/reference/src/gadgets/poly.h:116-118) overlaps the G2 arithmetic of point i with its own work on point i + 1.
int lsa_g2_tables_prefetch(const void *g2_jac, size_t n) {
    LSA_TRACE_CALL("g2_tables_prefetch", n);
    int rc = require_ready();
    if (rc) return rc;
    if (n == 0) return LSA_OK;
    if (!g2_jac) { set_error("g2_tables_prefetch: null argument"); return LSA_ERR_INVALID; }
    g_tabs.read_env();
    G2TableIndex &ix = g_tabs.ix;
    if (ix.capacity == 0 || n > PAIRING_CACHE_MAX_TERMS) return LSA_OK;         // nothing to keep them in
    ix.tick++;
    for (size_t i = 0; i < n; i++) {
        const char *q = (const char *)g2_jac + i * sizeof(Jac<Fq2>);
        const Key128 key = g2_fingerprint(q, sizeof(Jac<Fq2>), 1);
        if (ix.lookup(key) >= 0) continue;
        const long s = g_tabs.insert(key, true);                    // pending: no later insert may evict it before it is built
        if (s < 0) continue;                                        // full of tables of this very call: leave it to the Miller call
        Jac<Fq2> pt;
        memcpy(&pt, q, sizeof pt);
        g_pending.pts.push_back(pt);
        ix.promise(key, (uint32_t)s);
    }
    return ix.flush_due(PendingTables::batch()) ? g_pending.flush() : LSA_OK;
}

int lsa_pairing_set_chunk(unsigned pairs_per_accumulator) {
    if (pairs_per_accumulator > miller_tab_max_pairs()) { set_error("pairing_set_chunk: at most %u pairs share an accumulator", miller_tab_max_pairs()); return LSA_ERR_INVALID; }
    g_force_m = pairs_per_accumulator;
    return LSA_OK;
}
int lsa_g2_table_cache(size_t max_tables) {
    int rc = require_ready();
    if (rc) return rc;
    g_pending.drop();                                           // their slots go with the cache
    HIPCHK(hipStreamSynchronize(g.stream));
    g_tabs.env_read = true;
    g_tabs.clear();
    g_tabs.ix.set_capacity(max_tables);
    return LSA_OK;
}
int lsa_g2_table_cache_stats(uint64_t out[4]) {
    if (!out) return LSA_ERR_INVALID;
    const G2TableIndex &ix = g_tabs.ix;
    out[0] = ix.hits; out[1] = ix.misses; out[2] = ix.slots.size(); out[3] = ix.evictions;
    return LSA_OK;
}

int lsa_miller_loop(const void *g1, const void *g2, size_t n, void *out, int on_device) {
    int rc = require_ready();
    if (rc) return rc;
    if (n == 0) return LSA_OK;
    if (!g1 || !g2 || !out) { set_error("miller_loop: null argument"); return LSA_ERR_INVALID; }
    Terms t;
    t.g1 = g1; t.g2 = g2; t.n = n; t.on_device = on_device != 0;
    if (!on_device) return run_terms_host(t, out, false);
    void *res = nullptr;
    rc = run_miller(t, &res);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, res, n * fq12_bytes(), hipMemcpyDeviceToDevice, g.stream));
    return LSA_OK;
}
int lsa_miller_loop_precomp(const void *g1, const void *const *q_precomp, size_t n, void *out) {
    if (n && !q_precomp) { set_error("miller_loop_precomp: null argument"); return LSA_ERR_INVALID; }
    for (size_t i = 0; i < n; i++)
        if (!q_precomp[i]) { set_error("miller_loop_precomp: term %zu has no table", i); return LSA_ERR_INVALID; }
    Terms t;
    t.g1 = g1; t.qpre = q_precomp; t.n = n;
    return run_terms_host(t, out, false);
}
int lsa_pairing_terms(const void *g1, const void *g2, const void *const *q_precomp, const uint8_t *flags, const uint64_t *seg_offsets, size_t nseg,
                      void *out, int final_exp) {
    int rc = require_ready();
    if (rc) return rc;
    if (nseg == 0) return LSA_OK;
    rc = check_segments(seg_offsets, nseg, "pairing_terms");
    if (rc) return rc;
    Terms t;
    t.g1 = g1; t.g2 = g2; t.qpre = q_precomp; t.flags = flags; t.seg = seg_offsets; t.nseg = nseg; t.n = (size_t)seg_offsets[nseg];
    if (t.n && !g2 && !q_precomp) { set_error("pairing_terms: neither points nor tables"); return LSA_ERR_INVALID; }
    return run_terms_host(t, out, final_exp != 0);
}

static int product_host(const void *g1, const void *g2, size_t n, void *out, bool final_exp, bool sharded) {
    LSA_TRACE_CALL("pairing_product", n);
    int rc = require_ready();
    if (rc) return rc;
    if (!out || (n && (!g1 || !g2))) { set_error("pairing: null argument"); return LSA_ERR_INVALID; }
    const uint64_t seg[2] = {0, n};
    Terms t;
    t.g1 = g1; t.g2 = g2; t.seg = seg; t.nseg = 1; t.n = n;
    t.gt_only = final_exp;
    if (!(sharded && lsa_comm_world() > 1)) return run_terms_host(t, out, final_exp);
    // per-rank Miller product (1 for an empty slice), all-gather of the Fq12 partials, product in rank
    // order, one final exponentiation on every rank (SURVEY.md 8e "Pairings").  A rank whose local part
    // fails still takes part in the collective (with 1) and reports its error afterwards: the others
    // must not block in ncclAllGather.
    const size_t world = (size_t)lsa_comm_world();
    void *res = nullptr;
    int local = LSA_OK;
    if (g_pair_o.ensure(fq12_bytes()) || g_stage_gather.ensure(world * fq12_bytes()) || g_pair_s.ensure((world + 8) * fq12_bytes())) local = LSA_ERR_NOMEM;
    if (!local) local = run_miller(t, &res);
    if (local == LSA_ERR_NOMEM && !g_pair_o.p) { set_error("pairing: hipMalloc failed"); return local; }   // nothing to contribute from
    if (local) {
        Fq12 one = Fq12::one();
        (void)hipMemcpy(g_pair_o.p, &one, sizeof one, hipMemcpyHostToDevice);
    } else {
        HIPCHK(hipMemcpyAsync(g_pair_o.p, res, fq12_bytes(), hipMemcpyDeviceToDevice, g.stream));
    }
    rc = lsa_comm_all_gather(g_pair_o.p, g_stage_gather.p, 12);
    if (local) return local;
    if (rc) return rc;
    rc = fq12_product_device(g_stage_gather.p, g_pair_s.p, world, &res, g.stream);
    if (rc) return rc;
    if (final_exp) {
        rc = final_exp_device(res, 1, g_pair_o.p, g.stream);
        if (rc) return rc;
        res = g_pair_o.p;
    }
    return one_to_host(res, out);
}
int lsa_miller_loop_product(const void *g1, const void *g2, size_t n, void *out) { return product_host(g1, g2, n, out, false, false); }
int lsa_pairing_product(const void *g1, const void *g2, size_t n, void *out) { return product_host(g1, g2, n, out, true, false); }
int lsa_pairing_product_sharded(const void *g1, const void *g2, size_t n_local, void *out) { return product_host(g1, g2, n_local, out, true, true); }

// many independent products in one pass: one upload, one Miller launch over all pairs, one product
// workgroup per segment, one batched final exponentiation, one download
int lsa_pairing_product_segments(const void *g1, const void *g2, const uint64_t *seg_offsets, size_t nseg, void *out_gt, int final_exp) {
    int rc = require_ready();
    if (rc) return rc;
    if (nseg == 0) return LSA_OK;
    rc = check_segments(seg_offsets, nseg, "pairing_product_segments");
    if (rc) return rc;
    if (!out_gt) { set_error("pairing_product_segments: null argument"); return LSA_ERR_INVALID; }
    const size_t n = (size_t)seg_offsets[nseg];
    if (n && (!g1 || !g2)) { set_error("pairing_product_segments: null argument"); return LSA_ERR_INVALID; }
    Terms t;
    t.g1 = g1; t.g2 = g2; t.seg = seg_offsets; t.nseg = nseg; t.n = n;
    return run_terms_host(t, out_gt, final_exp != 0);
}

int lsa_fq12_product(const void *in, size_t n, void *out) {
    LSA_TRACE_CALL("fq12_product", n);
    int rc = require_ready();
    if (rc) return rc;
    if (!out || (n && !in)) { set_error("fq12_product: null argument"); return LSA_ERR_INVALID; }
    if (n == 0) {
        Fq12 one = Fq12::one();
        memcpy(out, &one, sizeof one);
        return LSA_OK;
    }
    void *res = nullptr;
    if (g_pair_f.ensure(n * fq12_bytes()) || g_pair_s.ensure(((n + 7) / 8 + 1) * fq12_bytes())) { set_error("fq12_product: hipMalloc failed"); return LSA_ERR_NOMEM; }
    LSA_UPLOAD(g_pair_f.p, in, n * fq12_bytes());
    rc = fq12_product_device(g_pair_f.p, g_pair_s.p, n, &res, g.stream);
    return rc ? rc : one_to_host(res, out);
}
int lsa_final_exponentiation(const void *in, size_t n, void *out, int on_device) {
    LSA_TRACE_CALL("final_exponentiation", n);
    int rc = require_ready();
    if (rc) return rc;
    if (n == 0) return LSA_OK;
    if (!in || !out) { set_error("final_exponentiation: null argument"); return LSA_ERR_INVALID; }
    if (on_device) return final_exp_device(in, n, out, g.stream);
    if (g_pair_f.ensure(n * fq12_bytes()) || g_pair_s.ensure(n * fq12_bytes())) { set_error("final_exponentiation: hipMalloc failed"); return LSA_ERR_NOMEM; }
    LSA_UPLOAD(g_pair_f.p, in, n * fq12_bytes());
    rc = final_exp_device(g_pair_f.p, n, g_pair_s.p, g.stream);
    if (rc) return rc;
    LSA_DOWNLOAD(out, g_pair_s.p, n * fq12_bytes());
    HIPCHK(hipStreamSynchronize(g.stream));
    return LSA_OK;
}
}  // extern "C"
