// Host unit test of the plan of a pairing job (csrc/pairing_plan.h; the launches: csrc/capi_pairing.hip).  Also built
// with the address + undefined-behaviour sanitizers (tests/test_host_cpp.py): every index block is allocated at exactly
// meta_bytes, so a write of fill() past the stated size is an error there.
// Over the cross product of
//   n in {0, 1, 2, 5, 41, 256, 257, 1024, 1025, 8192, 8193, 16385};
//   no segments / one segment / segments with an empty product first, in the middle and last / ragged products of
//   1 .. 9 terms / all products empty (n = 0);
//   M forced to 0 .. 4;  host / device points;  cache capacity 0 / 4096;  LSA_MILLER_KERNEL 0 / 3 / 5 / 6;
//   flags and blobs present or not:
//   (1) the route is the one the entry points took before plan_pairing existed (expected_route: a decision table written
//       from those conditions), and use_cache, M, g1_in_meta and scratch_max are what the shape says;
//   (2) table route: nacc = sum max(1, ceil(len / M)); acc[nacc] = n; accumulator a covers [acc[a], acc[a+1]); an
//       accumulator never crosses a product boundary; one of a non-empty product has 1 .. M pairs; an empty product owns
//       exactly one accumulator without pairs; every term is covered exactly once; prod[] counts accumulators;
//   (3) both layouts: the regions are disjoint, in the stated size, off_prod a multiple of 8 and off_g1 of 16; fill() writes
//       nothing outside its regions (the table pointers are the resolver's); the flags are bit 0 of the caller's;
//   (4) as_fused: the table pointers stay at the same offset and the block does not grow.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pairing_plan.h"
using namespace lsa;

static int fails = 0;
static long plans = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 30) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf(" (line %d)\n", __LINE__); } fails++; } } while (0)

struct Want { PairingRoute route; bool may_fill; };
// what run_miller did: the fused kernel for points the cache does not take, or when forced (6) -- never with blobs,
// without terms or under a forced chunk; the one-lane kernel only when forced (3) and the job is plain points; the
// tables otherwise, and there the fused kernel fills the tables of new points unless blobs, a forced chunk or
// LSA_MILLER_KERNEL=5 say otherwise
static Want expected_route(const PairingShape &s) {
    const bool no_cache = s.on_device || s.n > 1024 || s.capacity == 0;
    bool fused = false;
    switch (s.force_kernel) {
        case 0: fused = no_cache; break;
        case 6: fused = true; break;
        default: break;
    }
    if (s.blobs || s.n == 0 || s.force_m != 0) fused = false;
    if (fused) return Want{ROUTE_FUSED, false};
    if (s.force_kernel == 3 && !s.blobs && !s.flags) return Want{ROUTE_ONE_LANE, false};
    return Want{ROUTE_TABLES, !no_cache && !s.blobs && s.force_m == 0 && s.force_kernel != 5};
}

struct Region { const char *name; size_t off, bytes, align; };

static void check_regions(const Region *r, int count, size_t meta_bytes, const char *tag) {
    for (int i = 0; i < count; i++) {
        CHECK(r[i].off % r[i].align == 0, "%s: %s at %zu not aligned to %zu", tag, r[i].name, r[i].off, r[i].align);
        CHECK(r[i].off + r[i].bytes <= meta_bytes, "%s: %s ends at %zu of %zu", tag, r[i].name, r[i].off + r[i].bytes, meta_bytes);
        for (int k = 0; k < i; k++)
            CHECK(r[i].bytes == 0 || r[k].bytes == 0 || r[i].off >= r[k].off + r[k].bytes || r[k].off >= r[i].off + r[i].bytes, "%s: %s overlaps %s", tag, r[i].name, r[k].name);
    }
}

// fill() into a block of exactly meta_bytes, pre-set to a pattern: what lies outside `written` regions keeps it
static std::vector<char> filled(const PairingPlan &p, const PairingShape &s, const uint8_t *flags, const Region *written, int count, const char *tag) {
    std::vector<char> block(p.meta_bytes, (char)0xA5);
    p.fill(s, flags, block.data());
    std::vector<char> mine(p.meta_bytes, 0);
    for (int i = 0; i < count; i++)
        for (size_t b = written[i].off; b < written[i].off + written[i].bytes && b < p.meta_bytes; b++) mine[b] = 1;
    size_t touched = 0;
    for (size_t b = 0; b < p.meta_bytes; b++) touched += !mine[b] && block[b] != (char)0xA5;
    CHECK(touched == 0, "%s: fill wrote %zu bytes outside its regions", tag, touched);
    return block;
}

static void check_flags(const std::vector<char> &block, size_t off_flag, size_t n, const uint8_t *flags, const char *tag) {
    size_t bad = 0;
    for (size_t i = 0; i < n; i++) bad += (uint8_t)block[off_flag + i] != (flags ? (flags[i] & 1) : 0);
    CHECK(bad == 0, "%s: %zu flags differ", tag, bad);
}

static void check_fused_layout(const PairingPlan &p, const PairingShape &s, const uint8_t *flags, const char *tag) {
    const size_t n = s.n;
    CHECK(p.nacc == n && p.nprod == (s.seg ? s.nseg : n), "%s: fused counts %zu %zu", tag, p.nacc, p.nprod);
    const Region all[] = {{"tab", p.off_tab, n * 8, 8}, {"prod", p.off_prod, (p.nprod + 1) * 8, 8}, {"flag", p.off_flag, n, 1}};
    check_regions(all, 3, p.meta_bytes, tag);
    const std::vector<char> block = filled(p, s, flags, all + 1, 2, tag);
    const uint64_t *h_prod = (const uint64_t *)(block.data() + p.off_prod);
    size_t bad = 0;
    for (size_t j = 0; j <= p.nprod; j++) bad += h_prod[j] != (s.seg ? s.seg[j] : j);
    CHECK(bad == 0, "%s: %zu fused product offsets differ", tag, bad);
    check_flags(block, p.off_flag, n, flags, tag);
}

static void check_table_layout(const PairingPlan &p, const PairingShape &s, const uint8_t *flags, const char *tag) {
    const size_t n = s.n, M = p.M;
    const unsigned auto_m = n <= 8192 ? 1u : n <= 16384 ? 2u : n <= 24576 ? 3u : 4u;
    CHECK(p.M == (s.force_m ? s.force_m : auto_m) && p.M >= 1, "%s: M %u", tag, p.M);
    CHECK(p.nprod == (s.seg ? s.nseg : n), "%s: nprod %zu", tag, p.nprod);
    CHECK(p.g1_in_meta == (!s.on_device && n > 0 && n <= 256), "%s: g1_in_meta %d", tag, p.g1_in_meta);
    size_t want_nacc = 0;
    for (size_t j = 0; j < p.nprod; j++) {
        const size_t len = s.seg ? (size_t)(s.seg[j + 1] - s.seg[j]) : 1;
        want_nacc += len ? (len + M - 1) / M : 1;
    }
    CHECK(p.nacc == want_nacc, "%s: nacc %zu, want %zu", tag, p.nacc, want_nacc);
    const Region all[] = {{"tab", p.off_tab, n * 8, 8}, {"acc", p.off_acc, (p.nacc + 1) * 4, 4}, {"prod", p.off_prod, (p.nprod + 1) * 8, 8},
                          {"flag", p.off_flag, n, 1}, {"g1", p.off_g1, p.g1_in_meta ? n * PAIRING_G1_BYTES : 0, 16}};
    check_regions(all, 5, p.meta_bytes, tag);
    if (p.nacc != want_nacc) return;
    const std::vector<char> block = filled(p, s, flags, all + 1, 3, tag);
    const uint32_t *acc = (const uint32_t *)(block.data() + p.off_acc);
    const uint64_t *prod = (const uint64_t *)(block.data() + p.off_prod);
    check_flags(block, p.off_flag, n, flags, tag);
    CHECK(acc[p.nacc] == n && prod[0] == 0 && prod[p.nprod] == p.nacc, "%s: ends %u %llu %llu", tag, acc[p.nacc], (unsigned long long)prod[0], (unsigned long long)prod[p.nprod]);
    std::vector<uint8_t> covered(n, 0);
    size_t bad = 0;
    for (size_t j = 0; j < p.nprod && bad == 0; j++) {
        const size_t lo = s.seg ? (size_t)s.seg[j] : j, hi = s.seg ? (size_t)s.seg[j + 1] : j + 1;
        const size_t a0 = (size_t)prod[j], a1 = (size_t)prod[j + 1];
        if (a0 >= a1 || a1 > p.nacc) { bad++; break; }                      // every product owns at least one accumulator
        if (lo == hi) { bad += a1 - a0 != 1 || acc[a0] != lo || acc[a0 + 1] != lo; continue; }   // exactly one, without pairs
        bad += acc[a0] != lo || acc[a1] != hi;                             // first starts at the product, last ends with it
        for (size_t a = a0; a < a1; a++) {
            const size_t from = acc[a], to = acc[a + 1];                   // accumulator a covers [acc[a], acc[a+1])
            if (from < lo || to > hi || to <= from || to - from > M) { bad++; break; }
            for (size_t i = from; i < to; i++) covered[i]++;
        }
    }
    CHECK(bad == 0, "%s: accumulators do not partition the products", tag);
    size_t not_once = 0;
    for (size_t i = 0; i < n; i++) not_once += covered[i] != 1;
    CHECK(not_once == 0, "%s: %zu terms not covered exactly once", tag, not_once);
    // the same job through the fused kernel after resolution
    const PairingPlan f = p.as_fused(n);
    CHECK(f.route == ROUTE_FUSED && f.off_tab == p.off_tab && f.meta_bytes <= p.meta_bytes && f.use_cache == p.use_cache, "%s: as_fused moves or grows the block (%zu -> %zu)", tag, p.meta_bytes, f.meta_bytes);
    if (p.may_fill) check_fused_layout(f, s, flags, tag);
}

// segment offsets of the variants
static std::vector<uint64_t> segments(int variant, size_t n) {
    std::vector<uint64_t> off;
    switch (variant) {
        case 1: off = {0, n}; break;                                       // one product
        case 2: off = {0, 0, n / 3, n / 3, n, n}; break;                    // empty first, in the middle and last
        case 3: {                                                           // ragged: 1, 2, 3, 5, 9 terms in turn
            static const size_t len[] = {1, 2, 3, 5, 9};
            off.push_back(0);
            for (size_t at = 0, k = 0; at < n; k++) { at = at + len[k % 5] < n ? at + len[k % 5] : n; off.push_back(at); }
            break;
        }
        case 4: off = {0, 0, 0, 0}; break;                                  // all products empty
        default: break;
    }
    return off;
}

int main() {
    static const size_t ns[] = {0, 1, 2, 5, 41, 256, 257, 1024, 1025, 8192, 8193, 16385};
    static const int kernels[] = {0, 3, 5, 6};
    static const size_t caps[] = {0, 4096};
    std::vector<uint8_t> flag_bytes(16385);
    for (size_t i = 0; i < flag_bytes.size(); i++) flag_bytes[i] = (uint8_t)((i * 7 + i / 5) & 3);       // bits above bit 0 are ignored
    for (size_t n : ns)
        for (int variant = 0; variant < 5; variant++) {
            if (variant == 4 && n != 0) continue;
            const std::vector<uint64_t> off = segments(variant, n);
            for (unsigned force_m = 0; force_m <= 4; force_m++)
                for (int dev = 0; dev < 2; dev++)
                    for (size_t cap : caps)
                        for (int fk : kernels)
                            for (int fb = 0; fb < 4; fb++) {
                                PairingShape s;
                                s.n = n;
                                s.seg = variant ? off.data() : nullptr;
                                s.nseg = variant ? off.size() - 1 : 0;
                                s.flags = fb & 1; s.blobs = (fb & 2) != 0; s.on_device = dev != 0;
                                s.force_m = force_m; s.force_kernel = fk; s.capacity = cap; s.max_pairs = 4;
                                const uint8_t *flags = s.flags ? flag_bytes.data() : nullptr;
                                char tag[160];
                                snprintf(tag, sizeof tag, "n %zu variant %d M %u dev %d cap %zu kernel %d flags %d blobs %d", n, variant, force_m, dev, cap, fk, s.flags, s.blobs);
                                const PairingPlan p = plan_pairing(s);
                                plans++;
                                const Want w = expected_route(s);
                                CHECK(p.route == w.route && p.may_fill == w.may_fill, "%s: route %d fill %d, want %d %d", tag, p.route, p.may_fill, w.route, w.may_fill);
                                CHECK(p.use_cache == (!dev && cap > 0 && n <= 1024), "%s: use_cache %d", tag, p.use_cache);
                                CHECK(p.scratch_max == n, "%s: scratch_max %zu", tag, p.scratch_max);
                                if (p.route != w.route) continue;
                                if (p.route == ROUTE_TABLES) check_table_layout(p, s, flags, tag);
                                if (p.route == ROUTE_FUSED) check_fused_layout(p, s, flags, tag);
                            }
        }
    // M by batch size stops at max_pairs
    PairingShape big;
    big.n = 100000; big.blobs = true; big.max_pairs = 4;
    CHECK(plan_pairing(big).M == 4, "M stops at max_pairs");
    big.max_pairs = 2;
    CHECK(plan_pairing(big).M == 2, "M stops at max_pairs = 2");
    if (fails) { printf("%d FAILED (%ld plans)\n", fails, plans); return 1; }
    printf("PASS (%ld plans)\n", plans);
    return 0;
}
