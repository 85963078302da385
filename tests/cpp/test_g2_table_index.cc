// Host unit test of the G2 line-table cache's rules (csrc/g2_table_index.h; the device memory behind the slots:
// csrc/capi_pairing.hip).  Also built with the address + undefined-behaviour sanitizers (tests/test_host_cpp.py).
//   (a) scripted cases, one per rule: slots within one tick are never taken from each other, the next tick evicts the
//       older one, a promised (pending) slot is never the victim, erase makes a key miss and its slot is reused before a
//       new one is created, built() clears the pin, the call guard withdraws exactly what was inserted under it unless
//       committed, capacity 0 resolves nothing, and when promises are kept;
//   (b) a few thousand random sequences of lookup / insert / insert-pending / built / erase / new tick / set-capacity
//       over 12 keys and capacities 1, 2, 3, 8 against a deliberately naive model (a plain vector of records, linear
//       search, victim by sorting): after every step the returned slot, the four counters and the set of keys that
//       resolve agree, no two live keys share a slot, every slot is live, free or (beyond slots.size()) never used, and
//       no more slots are live than the capacity.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "g2_table_index.h"
using namespace lsa;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 30) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf(" (line %d)\n", __LINE__); } fails++; } } while (0)

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static Key128 K(uint64_t i) { return Key128{i * 0x9E3779B97F4A7C15ull + 1, ~i}; }

// ---------------------------------------------------------------- (a)
static void check_one_tick_and_the_next() {
    G2TableIndex ix;
    ix.set_capacity(2);
    ix.tick++;
    long got[6];
    for (int i = 0; i < 6; i++) { CHECK(ix.lookup(K(i)) < 0, "key %d unseen", i); got[i] = ix.insert(K(i)); }
    CHECK(got[0] == 0 && got[1] == 1, "two slots: %ld %ld", got[0], got[1]);
    for (int i = 2; i < 6; i++) CHECK(got[i] == -1, "key %d refused, got %ld", i, got[i]);
    CHECK(ix.evictions == 0 && ix.misses == 6 && ix.hits == 0 && ix.slots.size() == 2, "one tick: nothing evicted");
    // the next tick: key 1 is touched, key 0 is the older one and goes
    ix.tick++;
    CHECK(ix.lookup(K(1)) == 1, "key 1 resolves");
    CHECK(ix.insert(K(7)) == 0 && ix.evictions == 1, "the older slot goes");
    CHECK(ix.lookup(K(0)) < 0 && ix.lookup(K(7)) == 0 && ix.lookup(K(1)) == 1, "who resolves after the eviction");
    CHECK(ix.insert(K(8)) == -1 && ix.evictions == 1, "both slots belong to this tick");
    // ties go to the lowest slot: the scan is for a tick strictly below the best so far
    ix.tick++;
    CHECK(ix.insert(K(9)) == 0, "equal ticks: the first slot");
}

static void check_pending_is_never_the_victim() {
    G2TableIndex ix;
    ix.set_capacity(2);
    ix.tick++;
    CHECK(ix.insert(K(0), true) == 0 && ix.insert(K(1)) == 1, "two slots");
    ix.tick++;
    ix.lookup(K(1));                       // slot 1 is the younger one, slot 0 older but pending
    ix.tick++;
    CHECK(ix.insert(K(2)) == 1, "the built slot goes although the pending one is older");
    CHECK(ix.lookup(K(0)) == 0, "the promise still resolves");
    // no other candidate: none, rather than the pending slot
    G2TableIndex one;
    one.set_capacity(1);
    one.tick++;
    CHECK(one.insert(K(0), true) == 0, "slot");
    one.tick++;
    CHECK(one.insert(K(1)) == -1 && one.evictions == 0 && one.map.count(K(0)) == 1, "a pending slot is not chosen when it is the only one");
    // built() clears the pin
    one.built(K(0));
    CHECK(one.insert(K(1)) == 0 && one.evictions == 1 && one.map.count(K(0)) == 0, "built: evictable");
    one.built(K(5));                       // unknown key: nothing
}

static void check_erase() {
    G2TableIndex ix;
    ix.set_capacity(4);
    ix.tick++;
    for (int i = 0; i < 3; i++) ix.insert(K(i));
    ix.erase(K(1));
    const uint64_t m = ix.misses;
    CHECK(ix.lookup(K(1)) < 0 && ix.misses == m + 1, "an erased key misses");
    CHECK(ix.slots.size() == 3 && ix.free_slots.size() == 1, "the slot is released, not forgotten");
    CHECK(ix.insert(K(5)) == 1 && ix.slots.size() == 3, "a released slot is reused before a new one is created");
    CHECK(ix.insert(K(6)) == 3 && ix.slots.size() == 4, "then a new one");
    ix.erase(K(9));                        // unknown key: nothing
    CHECK(ix.free_slots.empty(), "erase of an unknown key");
    CHECK(ix.slot_to_create() == -1, "full: nothing to create");
    ix.erase(K(0));
    CHECK(ix.slot_to_create() == -1, "a free slot: nothing to create");
    ix.clear();
    CHECK(ix.slot_to_create() == 0 && ix.slots.empty() && ix.map.empty() && ix.misses == m + 1, "clear keeps the counters");
}

static void check_guard() {
    G2TableIndex ix;
    ix.set_capacity(8);
    ix.tick++;
    ix.insert(K(0));
    {
        G2TableIndex::CallGuard guard(ix);
        ix.insert(K(1));
        ix.insert(K(2));
    }                                      // not committed
    CHECK(ix.map.count(K(0)) == 1 && ix.map.count(K(1)) == 0 && ix.map.count(K(2)) == 0, "exactly the keys inserted under the guard are withdrawn");
    CHECK(ix.free_slots.size() == 2 && ix.slots.size() == 3, "their slots are released");
    {
        G2TableIndex::CallGuard guard(ix);
        ix.insert(K(3));
        guard.commit();
    }
    CHECK(ix.map.count(K(3)) == 1, "nothing is withdrawn after commit");
    ix.insert(K(4));                       // no guard armed: not journalled
    {
        G2TableIndex::CallGuard guard(ix);
    }
    CHECK(ix.map.count(K(4)) == 1 && ix.map.count(K(3)) == 1 && ix.journal.empty(), "a guard does not see earlier inserts");
    // a key evicted under the guard stays gone; the key that took its slot is withdrawn
    G2TableIndex two;
    two.set_capacity(1);
    two.tick++;
    two.insert(K(0));
    two.tick++;
    {
        G2TableIndex::CallGuard guard(two);
        CHECK(two.insert(K(1)) == 0, "evicts");
    }
    CHECK(two.map.empty() && two.free_slots.size() == 1, "neither key resolves to the half-written slot");
}

static void check_capacity_zero_and_promises() {
    G2TableIndex ix;
    ix.set_capacity(0);
    ix.tick++;
    for (int i = 0; i < 4; i++) CHECK(ix.lookup(K(i)) < 0 && ix.insert(K(i)) == -1 && ix.insert(K(i), true) == -1, "capacity 0: key %d", i);
    CHECK(ix.slots.empty() && ix.map.empty() && ix.misses == 4 && ix.slot_to_create() == -1, "no slot is created");
    // when promises are kept
    G2TableIndex small;
    small.set_capacity(8);
    CHECK(small.flush_due(60), "capacity 8, batch 60: at once");
    G2TableIndex big;
    big.set_capacity(240);
    big.tick++;
    for (int i = 0; i < 60; i++) {
        CHECK(!big.flush_due(60), "capacity 240, batch 60: %d promises wait", i);
        big.promise(K(i), (uint32_t)big.insert(K(i), true));
    }
    CHECK(big.flush_due(60), "the 60th promise");
    G2TableIndex edge;
    edge.set_capacity(239);
    CHECK(edge.flush_due(60), "below four batches: at once");
    // kept: the pins go; not kept: the keys go
    big.settle_promises(true);
    CHECK(big.promised.empty() && big.map.size() == 60 && !big.slots[7].pending, "kept");
    big.promise(K(100), (uint32_t)big.insert(K(100), true));
    big.settle_promises(false);
    CHECK(big.promised.empty() && big.map.count(K(100)) == 0 && big.map.size() == 60 && big.free_slots.size() == 1, "withdrawn");
    CHECK(G2TableIndex::clamp_batch(0) == 1 && G2TableIndex::clamp_batch(-5) == 1 && G2TableIndex::clamp_batch(60) == 60 && G2TableIndex::clamp_batch(5000) == 1024, "batch bounds");
    // the fingerprint: a function of bytes and kind
    uint64_t a[24], b[24];
    for (int i = 0; i < 24; i++) a[i] = b[i] = rng();
    CHECK(g2_fingerprint(a, sizeof a, 1) == g2_fingerprint(b, sizeof b, 1), "equal bytes");
    CHECK(!(g2_fingerprint(a, sizeof a, 1) == g2_fingerprint(a, sizeof a, 2)), "kind");
    b[23] ^= 1;
    CHECK(!(g2_fingerprint(a, sizeof a, 1) == g2_fingerprint(b, sizeof b, 1)), "one bit");
}

// ---------------------------------------------------------------- (b)
struct Model {
    struct Rec { int key; uint64_t tick; bool pending; long slot; };
    std::vector<Rec> live;                 // no order that matters
    std::vector<long> free_slots;          // released, last in first out
    long created = 0;
    size_t capacity = 0;
    uint64_t tick = 0, hits = 0, misses = 0, evictions = 0;

    Rec *find(int key) { for (Rec &r : live) if (r.key == key) return &r; return nullptr; }
    long lookup(int key) {
        Rec *r = find(key);
        if (!r) { misses++; return -1; }
        hits++;
        r->tick = tick;
        return r->slot;
    }
    long insert(int key, bool pending) {
        long s;
        if (!free_slots.empty()) { s = free_slots.back(); free_slots.pop_back(); }
        else if ((size_t)created < capacity) s = created++;
        else {
            // candidates: built, older than this tick; the victim is first by (tick, slot)
            std::vector<Rec> c;
            for (const Rec &r : live) if (!r.pending && r.tick < tick) c.push_back(r);
            if (c.empty()) return -1;
            std::sort(c.begin(), c.end(), [](const Rec &x, const Rec &y) { return x.tick != y.tick ? x.tick < y.tick : x.slot < y.slot; });
            s = c[0].slot;
            drop(c[0].key);
            evictions++;
        }
        live.push_back(Rec{key, tick, pending, s});
        return s;
    }
    void drop(int key) {
        for (size_t i = 0; i < live.size(); i++) if (live[i].key == key) { live.erase(live.begin() + (long)i); return; }
    }
    void erase(int key) { if (Rec *r = find(key)) { free_slots.push_back(r->slot); drop(key); } }
    void built(int key) { if (Rec *r = find(key)) r->pending = false; }
    void set_capacity(size_t k) { live.clear(); free_slots.clear(); created = 0; capacity = k; }
};

static void compare(G2TableIndex &ix, Model &m, int seq, int step, const char *op) {
    CHECK(ix.hits == m.hits && ix.misses == m.misses && ix.evictions == m.evictions && ix.slots.size() == (size_t)m.created,
          "seq %d step %d %s: counters %llu %llu %llu %zu, model %llu %llu %llu %ld", seq, step, op, (unsigned long long)ix.hits, (unsigned long long)ix.misses,
          (unsigned long long)ix.evictions, ix.slots.size(), (unsigned long long)m.hits, (unsigned long long)m.misses, (unsigned long long)m.evictions, m.created);
    // the keys that resolve, and to which slot (read from the map: a lookup would count)
    size_t live = 0;
    std::vector<int> owner(ix.slots.size(), -1);
    for (int k = 0; k < 12; k++) {
        auto it = ix.map.find(K(k));
        Model::Rec *r = m.find(k);
        CHECK((it != ix.map.end()) == (r != nullptr), "seq %d step %d %s: key %d resolves %d, model %d", seq, step, op, k, it != ix.map.end(), r != nullptr);
        if (it == ix.map.end() || !r) continue;
        live++;
        const uint32_t s = it->second;
        CHECK((long)s == r->slot && s < ix.slots.size(), "seq %d step %d %s: key %d slot %u, model %ld", seq, step, op, k, s, r->slot);
        if (s >= ix.slots.size()) continue;
        CHECK(owner[s] < 0, "seq %d step %d %s: keys %d and %d share slot %u", seq, step, op, owner[s], k, s);
        owner[s] = k;
        CHECK(ix.slots[s].used && ix.slots[s].key == K(k) && ix.slots[s].pending == r->pending && ix.slots[s].tick == r->tick, "seq %d step %d %s: slot %u of key %d", seq, step, op, s, k);
    }
    CHECK(ix.map.size() == live && live <= ix.capacity, "seq %d step %d %s: %zu live of %zu, map %zu", seq, step, op, live, ix.capacity, ix.map.size());
    // every slot in exactly one of live / free (never used: the slots beyond slots.size(), at most capacity in all)
    std::vector<int> in_free(ix.slots.size(), 0);
    for (uint32_t s : ix.free_slots) { CHECK(s < ix.slots.size(), "free slot %u", s); if (s < ix.slots.size()) in_free[s]++; }
    for (size_t s = 0; s < ix.slots.size(); s++)
        CHECK((owner[s] >= 0) + in_free[s] == 1 && ix.slots[s].used == (owner[s] >= 0), "seq %d step %d %s: slot %zu live %d free %d used %d", seq, step, op, s, owner[s] >= 0, in_free[s], ix.slots[s].used);
    CHECK(ix.slots.size() <= ix.capacity, "seq %d step %d %s: %zu slots of %zu", seq, step, op, ix.slots.size(), ix.capacity);
}

static void run(int seq) {
    static const size_t caps[] = {1, 2, 3, 8};
    G2TableIndex ix;
    Model m;
    ix.set_capacity(caps[seq % 4]);
    m.set_capacity(caps[seq % 4]);
    for (int step = 0; step < 60 && fails == 0; step++) {
        const int key = (int)(rng() % 12);
        const uint64_t r = rng() % 100;
        const char *op;
        if (r < 30) {
            op = "lookup";
            const long a = ix.lookup(K(key)), b = m.lookup(key);
            CHECK(a == b, "seq %d step %d lookup %d: %ld, model %ld", seq, step, key, a, b);
        } else if (r < 60) {
            // as the callers do: insert follows a lookup that missed
            const bool pending = r >= 50;
            op = pending ? "insert-pending" : "insert";
            const long a = ix.lookup(K(key)), b = m.lookup(key);
            CHECK(a == b, "seq %d step %d lookup before insert %d: %ld, model %ld", seq, step, key, a, b);
            if (a < 0 && b < 0) {
                const long c = ix.insert(K(key), pending), d = m.insert(key, pending);
                CHECK(c == d, "seq %d step %d %s %d: %ld, model %ld", seq, step, op, key, c, d);
            }
        } else if (r < 70) {
            op = "built";
            ix.built(K(key)); m.built(key);
        } else if (r < 80) {
            op = "erase";
            ix.erase(K(key)); m.erase(key);
        } else if (r < 97) {
            op = "tick";
            ix.tick++; m.tick++;
        } else {
            op = "set-capacity";
            const size_t c = caps[rng() % 4];
            ix.set_capacity(c); m.set_capacity(c);
        }
        compare(ix, m, seq, step, op);
    }
}

int main() {
    check_one_tick_and_the_next();
    check_pending_is_never_the_victim();
    check_erase();
    check_guard();
    check_capacity_zero_and_promises();
    for (int seq = 0; seq < 4000 && fails == 0; seq++) run(seq);
    if (fails) { printf("%d FAILED\n", fails); return 1; }
    printf("PASS\n");
    return 0;
}
