// legosnark_amd/csrc/g2_table_index.h -- the rules of the G2 line-table cache (capi_pairing.hip) that are pure functions
// of host data: which key resolves to which slot, which slot a new key takes, which keys are withdrawn when a call
// fails, and when promised tables are built.  The index hands out slot NUMBERS; the owner in capi_pairing.hip turns a
// slot into device memory.  Host code only, no HIP, no getenv: tests/cpp/test_g2_table_index.cc checks it against a
// naive model.
// The verifier-facing promise: a key never resolves to an unwritten or foreign line table.  A key enters the map only
// with a slot of its own; a slot changes hands only by eviction (never one the current tick touched, never one whose
// table is still promised) or after erase; whoever could not write a table it inserted a key for erases the key.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <unordered_map>
#include <vector>
#include "keyed_hash.h"

namespace lsa {

struct Key128 {
    uint64_t a, b;
    bool operator==(const Key128 &o) const { return a == o.a && b == o.b; }
};
struct Key128Hash { size_t operator()(const Key128 &k) const { return (size_t)(k.a ^ (k.b * 0x9E3779B97F4A7C15ull)); } };

// 128-bit KEYED fingerprint (keyed_hash.h: NH under a per-process random key): a verifier's results depend on which
// table a point resolves to, so the key of a table must not be something a prover can aim at -- for two distinct
// points (or blobs) the collision probability over the key is <= 2^-64 whatever their bytes are.
inline Key128 g2_fingerprint(const void *bytes, size_t nbytes, uint64_t kind) {
    uint64_t h[2];
    keyed_hash128(bytes, nbytes, kind, h);
    return Key128{h[0], h[1]};
}

struct G2TableIndex {
    struct Slot { Key128 key; uint64_t tick; bool used; bool pending; };      // pending: promised by a prefetch, not built yet
    struct Promise { Key128 key; uint32_t slot; };
    size_t capacity = 4096;                               // tables; 90 MB
    uint64_t tick = 0, hits = 0, misses = 0, evictions = 0;
    std::vector<Slot> slots;                              // every slot ever created, released ones included
    std::vector<uint32_t> free_slots;                     // released by erase, reused before a new slot is created
    std::unordered_map<Key128, uint32_t, Key128Hash> map;
    std::vector<Promise> promised;                        // slots taken, keys resolve, tables not yet built
    std::vector<Key128> journal;                          // keys inserted under the current CallGuard
    bool journaling = false;

    static size_t clamp_batch(long v) { return (size_t)(v < 1 ? 1 : v > 1024 ? 1024 : v); }

    // slot of `key`, -1 on a miss
    long lookup(const Key128 &key) {
        auto it = map.find(key);
        if (it == map.end()) { misses++; return -1; }
        hits++;
        slots[it->second].tick = tick;
        return (long)it->second;
    }
    // the slot insert() would CREATE next, -1 when it would reuse, evict or refuse: the owner allocates the memory of a
    // new block before the key enters the map, so a failed allocation leaves nothing behind
    long slot_to_create() const { return free_slots.empty() && slots.size() < capacity ? (long)slots.size() : -1; }
    // a slot for `key` (a released one, a new one, or the least recently used one that neither the current tick nor an
    // unbuilt promise refers to), -1 if none
    long insert(const Key128 &key, bool pending = false) {
        long s = -1;
        if (!free_slots.empty()) {
            s = (long)free_slots.back();
            free_slots.pop_back();
        } else if (slots.size() < capacity) {
            slots.push_back(Slot{});
            s = (long)slots.size() - 1;
        } else {
            uint64_t best = tick;
            for (size_t i = 0; i < slots.size(); i++)
                if (slots[i].used && !slots[i].pending && slots[i].tick < best) { best = slots[i].tick; s = (long)i; }
            if (s < 0) return -1;
            map.erase(slots[(size_t)s].key);
            evictions++;
        }
        slots[(size_t)s] = Slot{key, tick, true, pending};
        map[key] = (uint32_t)s;
        if (journaling) journal.push_back(key);
        return s;
    }
    // forgets `key` (a table that was promised or begun and never finished: a later lookup must miss, not read it)
    void erase(const Key128 &key) {
        auto it = map.find(key);
        if (it == map.end()) return;
        const uint32_t s = it->second;
        map.erase(it);
        slots[s].used = false; slots[s].pending = false; slots[s].tick = 0;
        free_slots.push_back(s);
    }
    void built(const Key128 &key) {
        auto it = map.find(key);
        if (it != map.end()) slots[it->second].pending = false;
    }
    // forgets every key, slot and promise; the counters and the tick run on
    void clear() { slots.clear(); free_slots.clear(); map.clear(); promised.clear(); journal.clear(); }
    void set_capacity(size_t tables) { clear(); capacity = tables; }

    // ---- keys a call inserts are withdrawn again unless the call commits: on any error return their tables would be
    // unwritten or partial, and the next call with the same Q would run its Miller loop over them
    struct CallGuard {
        G2TableIndex &ix;
        explicit CallGuard(G2TableIndex &index) : ix(index) { ix.journal.clear(); ix.journaling = true; }
        void commit() { ix.journal.clear(); }
        ~CallGuard() {
            ix.journaling = false;
            for (const Key128 &k : ix.journal) ix.erase(k);
            ix.journal.clear();
        }
        CallGuard(const CallGuard &) = delete;
        CallGuard &operator=(const CallGuard &) = delete;
    };

    // ---- promised tables: built in one launch when a Miller call arrives or when `batch` of them are waiting,
    // whichever is first.  A cache smaller than four batches could hand a promised slot to somebody else before it is
    // built (every other slot may belong to the current tick): it keeps its promises at once.
    void promise(const Key128 &key, uint32_t slot) { promised.push_back(Promise{key, slot}); }
    bool flush_due(size_t batch) const { return promised.size() >= batch || capacity < 4 * batch; }
    // the launch for the promises went out (kept) or failed: a promise that could not be kept is withdrawn -- its key
    // must miss from now on, not resolve to an unwritten table
    void settle_promises(bool kept) {
        for (const Promise &p : promised) { if (kept) built(p.key); else erase(p.key); }
        promised.clear();
    }
};

}  // namespace lsa
