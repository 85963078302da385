// legosnark_amd/csrc/crs_index.h -- the rules of the CRS cache (crs_cache.hip) that are pure functions of host data: what
// is fingerprinted, which requests can be compared with which entries, which entry goes first.  Host code only, no
// HIP: tests/cpp/test_crs_index.cc checks them.
#pragma once
#include <vector>
#include "keyed_hash.h"

namespace lsa {

constexpr size_t CRS_UNIT_POINTS = 64;          // fingerprint granularity (a prefix of k units can be verified against a longer entry)
constexpr size_t CRS_TASK_UNITS = 64;           // units per hashing task (4096 points)
constexpr size_t CRS_MIN_POINTS = 1024;         // smaller vectors are cheaper to re-upload than to look up

// the fingerprint of one unit (or one point): keyed, see keyed_hash.h
inline uint64_t hash_words(const uint64_t *w, size_t nwords) { return keyed_hash64(w, nwords * 8, 0); }

// sampled mode: the points of an n-point vector that are compared (~3 log2 n of them)
inline std::vector<size_t> sample_positions(size_t n) {
    std::vector<size_t> pos;
    for (size_t i = 0; i < 8 && i < n; i++) pos.push_back(i);
    for (size_t k = 8; k < n; k <<= 1) {
        pos.push_back(k - 1);
        pos.push_back(k);
        if (k + k / 2 < n) pos.push_back(k + k / 2);
    }
    if (n) pos.push_back(n - 1);
    return pos;
}

// a request of n points can be compared with an entry of entry_n points only when the request's units cover the same
// byte ranges as the entry's: the whole vector, or a prefix of whole units
inline bool crs_comparable(size_t entry_n, size_t n) { return entry_n >= n && (entry_n == n || n % CRS_UNIT_POINTS == 0); }

// a request below CRS_MIN_POINTS is compared point by point below one unit and unit by unit above; returns the number
// of fingerprints to compare, 0: not comparable (no points, or a partial last unit)
inline size_t crs_small_fingerprints(size_t n, bool *by_point) {
    *by_point = n < CRS_UNIT_POINTS;
    return *by_point ? n : (n % CRS_UNIT_POINTS == 0 ? n / CRS_UNIT_POINTS : 0);
}

// the least recently used entry of [first, last) by its .tick, never the one whose tick is `keep` (ticks start at 1:
// keep = 0 spares none); last: there is none
template <class It>
It crs_lru_victim(It first, It last, uint64_t keep = 0) {
    It victim = last;
    for (It i = first; i != last; ++i)
        if (i->tick != keep && (victim == last || i->tick < victim->tick)) victim = i;
    return victim;
}

}  // namespace lsa
