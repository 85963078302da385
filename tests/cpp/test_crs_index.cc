// Host unit test of the CRS cache's host-only pieces (csrc/keyed_hash.h, hash_pool.h, crs_index.h; the cache itself:
// csrc/crs_cache.hip).  Also built with the address + undefined-behaviour sanitizers and with the thread sanitizer
// (tests/test_host_cpp.py): HashPool is the library's one piece of hand-written thread code.
//   (1) HashPool against the serial loop (hash_words per unit) at the sizes where its paths change: one unit, a short
//       last unit, fewer than 8 tasks (the caller alone), exactly 8 (workers start), a short last task; every buffer is
//       allocated at its exact size, so a read past the end is an error under the sanitizer;
//   (2) the same after stop(), three times over (lsa_shutdown -> lsa_init: workers started later must not see a phantom
//       generation), and in a pool that LSA_HASH_THREADS=0 leaves without workers;
//   (3) the keyed hash: a function of its input within the process; any single changed word of a 6144-byte unit, a changed
//       length and a changed tweak each change the value -- the last three except with probability about 2^-64 over the
//       process's random key, the bound the cache's verification rests on;
//   (4) sample_positions, the comparability rule, the small-request rule and the choice of the LRU victim.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>

#include "hash_pool.h"
using namespace lsa;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 30) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf(" (line %d)\n", __LINE__); } fails++; } } while (0)

static const size_t POINT_BYTES = 96, UNIT_BYTES = CRS_UNIT_POINTS * POINT_BYTES;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static void check_pool(HashPool &pool, size_t npoints, const char *tag) {
    const size_t bytes = npoints * POINT_BYTES, nunits = (npoints + CRS_UNIT_POINTS - 1) / CRS_UNIT_POINTS;
    uint64_t *buf = (uint64_t *)malloc(bytes);
    for (size_t i = 0; i < bytes / 8; i++) buf[i] = rng();
    std::vector<uint64_t> want(nunits), got(nunits, 0);
    for (size_t u = 0; u < nunits; u++) {
        const size_t lo = u * UNIT_BYTES, hi = lo + UNIT_BYTES < bytes ? lo + UNIT_BYTES : bytes;
        want[u] = hash_words(buf + lo / 8, (hi - lo) / 8);
    }
    pool.begin(buf, bytes, UNIT_BYTES, CRS_TASK_UNITS, got.data());
    pool.finish();
    CHECK(got == want, "%s: %zu points", tag, npoints);
    free(buf);
}

static void check_pool_sizes(HashPool &pool, const char *tag) {
    const size_t sizes[] = {1, 63, 64, 65, 7 * 4096 + 5, 8 * 4096, 9 * 4096 + 63, 100000};
    for (size_t n : sizes) check_pool(pool, n, tag);
}

static void check_keyed_hash() {
    const size_t nw = UNIT_BYTES / 8;
    std::vector<uint64_t> m(nw), c;
    for (auto &w : m) w = rng();
    c = m;
    const uint64_t h = keyed_hash64(m.data(), UNIT_BYTES, 0);
    uint64_t h128[2], c128[2];
    keyed_hash128(m.data(), UNIT_BYTES, 0, h128);
    keyed_hash128(c.data(), UNIT_BYTES, 0, c128);
    CHECK(keyed_hash64(c.data(), UNIT_BYTES, 0) == h && h128[0] == c128[0] && h128[1] == c128[1], "equal inputs");
    CHECK(hash_words(m.data(), nw) == h, "hash_words is keyed_hash64 with tweak 0");
    for (size_t i = 0; i < nw; i++) {
        const uint64_t keep = c[i];
        c[i] = 0x0123456789ABCDEFull;
        CHECK(keyed_hash64(c.data(), UNIT_BYTES, 0) != h, "word %zu", i);
        c[i] = keep;
    }
    std::vector<uint64_t> z(nw, 0);                      // two messages that differ only in length
    CHECK(keyed_hash64(z.data(), UNIT_BYTES, 0) != keyed_hash64(z.data(), UNIT_BYTES - 8, 0), "length");
    CHECK(keyed_hash64(z.data(), 96, 0) != keyed_hash64(z.data(), 88, 0), "length, short");
    CHECK(keyed_hash64(m.data(), UNIT_BYTES, 1) != h, "tweak");
    keyed_hash128(m.data(), UNIT_BYTES, 1, c128);
    CHECK(c128[0] != h128[0] || c128[1] != h128[1], "tweak, 128-bit");
}

static void check_sample_positions() {
    const size_t ns[] = {0, 1, 7, 8, 9, 1024, 5000};
    for (size_t n : ns) {
        const std::vector<size_t> pos = sample_positions(n);
        size_t log2n = 0;
        while (((size_t)1 << log2n) < n) log2n++;        // ceil(log2 n)
        CHECK(pos.size() <= 3 * log2n + 9, "n %zu: %zu positions", n, pos.size());
        for (size_t p : pos) CHECK(p < n, "n %zu: position %zu", n, p);
        auto has = [&](size_t p) { for (size_t q : pos) if (q == p) return true; return false; };
        for (size_t i = 0; i < 8 && i < n; i++) CHECK(has(i), "n %zu: head %zu", n, i);
        if (n) CHECK(has(n - 1), "n %zu: last", n);
    }
}

static void check_rules() {
    // (entry n, request n, comparable)
    const struct { size_t entry, req; bool yes; } cmp[] = {
        {5000, 4096, true}, {5000, 4097, false}, {5000, 5000, true}, {5000, 5001, false}, {5000, 64, true}, {5000, 4992, true},
        {5000, 4999, false}, {4096, 4096, true}, {4096, 8192, false}, {1088, 1024, true}, {1088, 1030, false}, {1000, 1000, true}};
    for (auto &c : cmp) CHECK(crs_comparable(c.entry, c.req) == c.yes, "entry %zu request %zu", c.entry, c.req);
    // (request n, fingerprints compared, by point): below one unit by point, above by unit, never a partial last unit
    const struct { size_t req, count; bool by_point; } small[] = {
        {63, 63, true}, {64, 1, false}, {96, 0, false}, {1, 1, true}, {0, 0, true}, {512, 8, false}, {960, 15, false}, {1000, 0, false}, {65, 0, false}};
    for (auto &s : small) {
        bool by_point = !s.by_point;
        CHECK(crs_small_fingerprints(s.req, &by_point) == s.count && by_point == s.by_point, "request %zu", s.req);
    }
    // the LRU victim: the oldest tick, never the kept one
    struct E { uint64_t tick; };
    std::list<E> l = {{5}, {2}, {9}, {3}};
    CHECK(crs_lru_victim(l.begin(), l.end())->tick == 2, "oldest");
    CHECK(crs_lru_victim(l.begin(), l.end(), 2)->tick == 3, "oldest but the kept one");
    CHECK(crs_lru_victim(l.begin(), l.end(), 9)->tick == 2, "kept one is not the oldest");
    std::list<E> one = {{7}};
    CHECK(crs_lru_victim(one.begin(), one.end(), 7) == one.end(), "only the kept entry: none");
    CHECK(crs_lru_victim(one.begin(), one.end())->tick == 7, "a single entry");
    CHECK(crs_lru_victim(one.end(), one.end()) == one.end(), "empty");
}

int main() {
    {
        HashPool pool;
        check_pool_sizes(pool, "fresh pool");
        for (int cycle = 0; cycle < 3; cycle++) {
            pool.stop();
            check_pool_sizes(pool, "after stop()");
        }
    }
    {
        setenv("LSA_HASH_THREADS", "0", 1);
        HashPool pool;
        check_pool_sizes(pool, "no workers");
        unsetenv("LSA_HASH_THREADS");
    }
    check_keyed_hash();
    check_sample_positions();
    check_rules();
    if (fails) { printf("%d FAILED\n", fails); return 1; }
    printf("PASS\n");
    return 0;
}
