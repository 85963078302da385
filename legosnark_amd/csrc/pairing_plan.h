// legosnark_amd/csrc/pairing_plan.h -- the plan of one pairing job (capi_pairing.hip): everything its SHAPE decides,
// before a single table is resolved.  Which kernel family takes it, whether the line-table cache is asked, how many
// pairs share an accumulator, and the layout of the pinned index block that goes to the device in one copy.  Two
// steps, like plan_pipeline (msm_plan.h): sizes and offsets first, then fill() into the caller's block.  No HIP type,
// no getenv, no global state, no heap: tests/cpp/test_pairing_plan.cc checks on the host what the kernels rely on:
//   - accumulator a covers the terms [acc[a], acc[a+1]): the next accumulator starts where this one ends, except after
//     an empty product (same start), and acc[nacc] = n;
//   - an accumulator never crosses a product boundary and holds at most M pairs;
//   - an empty product owns exactly one accumulator without pairs (its value is one);
//   - the regions of the block do not overlap, lie inside meta_bytes, and are aligned for what they hold.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace lsa {

constexpr size_t PAIRING_G1_BYTES = 96;          // one Jacobian G1 point (capi_pairing.hip asserts it)
constexpr size_t PAIRING_CACHE_MAX_TERMS = 1024; // larger jobs are not fingerprinted
constexpr size_t PAIRING_G1_INLINE_MAX = 256;    // host G1 points of a job this small ride in the index block

enum PairingRoute {
    ROUTE_FUSED,      // k_miller_fused: G2 arithmetic and Fq12 chain side by side, one value per term, no table read
    ROUTE_ONE_LANE,   // miller.h, one lane per pairing (the family's fallback): only when forced
    ROUTE_TABLES,     // line tables, resolved per term; may still end in the fused kernel, which then FILLS the new
                      // tables (may_fill)
};

struct PairingShape {
    size_t n = 0;                    // terms
    const uint64_t *seg = nullptr;   // nseg + 1 offsets; null: every term is its own product
    size_t nseg = 0;
    bool flags = false, blobs = false, on_device = false;
    unsigned force_m = 0;            // lsa_pairing_set_chunk
    int force_kernel = 0;            // LSA_MILLER_KERNEL: 0, 3 (one lane), 5 (tables), 6 (fused)
    size_t capacity = 0;             // of the line-table cache
    unsigned max_pairs = 4;          // miller_tab_max_pairs()
};

struct PairingPlan {
    PairingRoute route = ROUTE_TABLES;
    bool use_cache = false;          // terms are fingerprinted and looked up
    bool may_fill = false;           // points seen for the first time go through the fused kernel, which fills their tables
    unsigned M = 1;                  // pairs per accumulator
    size_t nprod = 0, nacc = 0;      // products; Miller values the kernel writes (fused: one per term)
    bool g1_in_meta = false;
    // the index block.  ROUTE_TABLES: table pointers (u64 x n), accumulator offsets in terms (u32 x nacc + 1), product
    // offsets in accumulators (u64 x nprod + 1), flags (u8 x n), inline G1 points.  ROUTE_FUSED: tables to fill or 0
    // (u64 x n), product offsets in terms (u64 x nprod + 1), flags; no accumulator offsets, no points.
    size_t off_tab = 0, off_acc = 0, off_prod = 0, off_flag = 0, off_g1 = 0, meta_bytes = 0;
    size_t scratch_max = 0;          // tables the job may need outside the cache (without the cache the resolver
                                     // counts distinct blobs and takes fewer)

    void layout(size_t n) {
        const bool tables = route == ROUTE_TABLES;
        off_tab = 0;
        off_acc = off_tab + n * 8;
        off_prod = (off_acc + (tables ? (nacc + 1) * 4 : 0) + 7) & ~(size_t)7;
        off_flag = off_prod + (nprod + 1) * 8;
        off_g1 = (off_flag + n + 15) & ~(size_t)15;
        meta_bytes = off_g1 + (g1_in_meta ? n * PAIRING_G1_BYTES : 0) + 8;
    }
    // the same job through the fused kernel after all: the table pointers stay where the resolver wrote them (they
    // become the tables to fill), the block never grows
    PairingPlan as_fused(size_t n) const {
        PairingPlan p = *this;
        p.route = ROUTE_FUSED;
        p.M = 1;
        p.nacc = n;
        p.g1_in_meta = false;
        p.layout(n);
        return p;
    }
    // accumulator and product offsets and the flags into `block` (meta_bytes of it); the table pointers are the
    // resolver's
    void fill(const PairingShape &s, const uint8_t *flags, char *block) const {
        uint64_t *h_prod = (uint64_t *)(block + off_prod);
        if (route == ROUTE_TABLES) {
            uint32_t *h_acc = (uint32_t *)(block + off_acc);
            size_t a = 0;
            for (size_t j = 0; j < nprod; j++) {
                h_prod[j] = a;
                const size_t lo = s.seg ? (size_t)s.seg[j] : j, hi = s.seg ? (size_t)s.seg[j + 1] : j + 1;
                if (lo == hi) { h_acc[a++] = (uint32_t)lo; continue; }       // an empty product: one accumulator without pairs = 1
                for (size_t t = lo; t < hi; t += M) h_acc[a++] = (uint32_t)t;
            }
            h_prod[nprod] = a;
            h_acc[a] = (uint32_t)s.n;
        } else {
            for (size_t j = 0; j <= nprod; j++) h_prod[j] = s.seg ? s.seg[j] : j;
        }
        uint8_t *h_flag = (uint8_t *)(block + off_flag);
        for (size_t i = 0; i < s.n; i++) h_flag[i] = flags ? (uint8_t)(flags[i] & 1) : (uint8_t)0;
    }
};

inline PairingPlan plan_pairing(const PairingShape &s) {
    PairingPlan p;
    const size_t n = s.n;
    p.nprod = s.seg ? s.nseg : n;
    p.use_cache = !s.on_device && s.capacity > 0 && n <= PAIRING_CACHE_MAX_TERMS;
    p.scratch_max = n;
    // points the cache does not take (more than 1024 terms, device-resident, cache off) go through the fused kernel;
    // a forced chunk needs accumulators, which only the table kernels have
    if (!s.blobs && n && s.force_m == 0 && ((s.force_kernel == 0 && !p.use_cache) || s.force_kernel == 6)) p.route = ROUTE_FUSED;
    else if (!s.blobs && !s.flags && s.force_kernel == 3) p.route = ROUTE_ONE_LANE;
    if (p.route != ROUTE_TABLES) {
        p.nacc = n;
        if (p.route == ROUTE_FUSED) p.layout(n);
        return p;
    }
    p.may_fill = p.use_cache && !s.blobs && s.force_m == 0 && s.force_kernel != 5;
    // accumulators: a product of len pairs takes ceil(len / M) of them; M grows once the chip is full
    // (four accumulators per wavefront, 1024 SIMDs)
    while (p.M < s.max_pairs && n > (size_t)p.M * 8192) p.M++;
    if (s.force_m) p.M = s.force_m;
    if (s.seg) {
        for (size_t j = 0; j < p.nprod; j++) { const size_t len = (size_t)(s.seg[j + 1] - s.seg[j]); p.nacc += len ? (len + p.M - 1) / p.M : 1; }
    } else {
        p.nacc = n;
    }
    p.g1_in_meta = !s.on_device && n > 0 && n <= PAIRING_G1_INLINE_MAX;
    p.layout(n);
    return p;
}

}  // namespace lsa
