// tests/cpp/w12_edge_cases.h -- the operand classes of the pairing engines' contract ("operands < 2p, tight limbs"), shared by
// the host test of the host-compilable forms (tests/cpp/test_w12_edges.cc) and the device check of the row engine
// (tools/w12_rows_check.hip), so that both see the same cases.  Host code only.
//
// An element is twelve Fq components as RAW 29-bit limbs in the engine's slot order: component 2k + part is part (0: c0, 1: c1)
// of the coefficient of w^k.  Nothing here goes through from_mont256: the limbs are what the engine reads.
#pragma once
#include <array>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>
#include "w12.h"

namespace w12edge {
using namespace lsa;

enum Cls {
    C_ZERO,      // 0
    C_ONE,       // 1 in Montgomery form (2^261 mod p)
    C_PM1,       // p - 1
    C_P,         // p: zero, not canonical
    C_PP1,       // p + 1
    C_2PM1,      // 2p - 1: the top of the contract
    C_TMAX_P,    // low limbs all 2^29 - 1, top limb one under p's: the tight maximum below p
    C_TMAX_2P,   // the same below 2p
    C_RAND,      // random canonical v
    C_RAND_PP,   // the same v stored as v + p: the form condsub2 leaves behind
    N_CLS
};
static const char *const CLS_NAME[N_CLS] = {"0", "1", "p-1", "p", "p+1", "2p-1", "tmax<p", "tmax<2p", "v", "v+p"};

using Elt = std::array<F29, 12>;

// k*p - minus in tight limbs (k*p >= minus)
inline F29 kp_minus(uint32_t k, int minus) {
    F29 r;
    uint64_t c = 0;
    for (int i = 0; i < 9; i++) { c += (uint64_t)F29::p(i) * k; r.l[i] = i < 8 ? (uint32_t)c & F29::MASK : (uint32_t)c; c >>= 29; }
    int64_t b = -(int64_t)minus;
    for (int i = 0; i < 9 && b != 0; i++) {
        const int64_t v = (int64_t)r.l[i] + b;
        if (i < 8) { r.l[i] = (uint32_t)v & F29::MASK; b = v >> 29; } else { r.l[i] = (uint32_t)v; b = 0; }
    }
    return r;
}
// every low limb 2^29 - 1, top limb one under k*p's: the largest tight limbs of a value below k*p
inline F29 tight_max(uint32_t k) {
    F29 r = kp_minus(k, 0);
    for (int i = 0; i < 8; i++) r.l[i] = F29::MASK;
    r.l[8] -= 1u;
    return r;
}
// a < b as integers, both with tight limbs 0..7
inline bool less_than(const F29 &a, const F29 &b) {
    for (int i = 8; i >= 0; --i) if (a.l[i] != b.l[i]) return a.l[i] < b.l[i];
    return false;
}
// what the next chain link relies on: limbs 0..7 below 2^29 and the value below k*p as an integer
inline bool tight_below(const F29 &a, uint32_t k) {
    for (int i = 0; i < 8; i++) if (a.l[i] > F29::MASK) return false;
    return less_than(a, kp_minus(k, 0));
}
// the residue in [0, p) of a tight value below 64p, as a libff Fq (F29::canonical stops at 16p)
inline Fq residue(F29 t) {
    for (int s = 5; s >= 0; --s) {
        const F29 m = kp_minus(1u << s, 0);
        if (less_than(t, m)) continue;
        int64_t c = 0;
        for (int i = 0; i < 9; i++) {
            const int64_t v = (int64_t)t.l[i] - (int64_t)m.l[i] + c;
            if (i < 8) { t.l[i] = (uint32_t)v & F29::MASK; c = v >> 29; } else t.l[i] = (uint32_t)v;
        }
    }
    return t.to_mont256();
}
inline bool same_limbs(const F29 &a, const F29 &b) {
    for (int i = 0; i < 9; i++) if (a.l[i] != b.l[i]) return false;
    return true;
}

struct Gen {
    std::mt19937_64 rng;
    explicit Gen(uint64_t seed) : rng(seed) {}
    F29 rand_canonical() {
        const F29 p = kp_minus(1, 0);
        for (;;) {
            F29 r;
            for (int i = 0; i < 8; i++) r.l[i] = (uint32_t)rng() & F29::MASK;
            r.l[8] = (uint32_t)(rng() % (p.l[8] + 1u));
            if (less_than(r, p)) return r;
        }
    }
    F29 value(int cls) {
        switch (cls) {
        case C_ZERO: return F29::zero();
        case C_ONE: return F29::one();
        case C_PM1: return kp_minus(1, 1);
        case C_P: return kp_minus(1, 0);
        case C_PP1: return kp_minus(1, -1);
        case C_2PM1: return kp_minus(2, 1);
        case C_TMAX_P: return tight_max(1);
        case C_TMAX_2P: return tight_max(2);
        case C_RAND: return rand_canonical();
        default: return add_lazy(rand_canonical(), kp_minus(1, 0)).norm();
        }
    }
    Elt all_of(int cls) { Elt e; for (F29 &c : e) c = value(cls); return e; }
    // component `pos` of the class, the rest random canonical
    Elt single(int cls, int pos) { Elt e = all_of(C_RAND); e[pos] = value(cls); return e; }
    Elt mixed() { Elt e; for (F29 &c : e) c = value((int)(rng() % N_CLS)); return e; }
    // a single nonzero Fq component; the zeros as literal zeros or, p_zeros, stored as p
    Elt one_hot(int cls, int pos, bool p_zeros) { Elt e = all_of(p_zeros ? C_P : C_ZERO); e[pos] = value(cls); return e; }
};

struct Named { Elt e; char name[40]; };
// the elements every section draws from: each class in all twelve components, in one component beside random ones, mixed, one-hot
inline std::vector<Named> elements(uint64_t seed) {
    Gen g(seed);
    std::vector<Named> v;
    auto push = [&](const Elt &e, const char *fmt, const char *a, int b) { Named n; n.e = e; snprintf(n.name, sizeof n.name, fmt, a, b); v.push_back(n); };
    for (int c = 0; c < N_CLS; c++) push(g.all_of(c), "all %s", CLS_NAME[c], 0);
    for (int c = 0; c < N_CLS; c++) {
        push(g.single(c, (5 * c + 1) % 12), "single %s at %d", CLS_NAME[c], (5 * c + 1) % 12);
        push(g.single(c, (7 * c + 6) % 12), "single %s at %d", CLS_NAME[c], (7 * c + 6) % 12);
    }
    for (int t = 0; t < 8; t++) push(g.mixed(), "mixed%s %d", "", t);
    static const int HOT[8] = {C_ONE, C_PM1, C_PP1, C_2PM1, C_TMAX_P, C_TMAX_2P, C_RAND, C_RAND_PP};
    for (int pos = 0; pos < 12; pos++) push(g.one_hot(HOT[pos % 8], pos, false), "one-hot %s at %d", CLS_NAME[HOT[pos % 8]], pos);
    for (int pos = 0; pos < 12; pos += 3) push(g.one_hot(HOT[(pos + 3) % 8], pos, true), "one-hot %s at %d over p", CLS_NAME[HOT[(pos + 3) % 8]], pos);
    return v;
}
// the pairs of a product section: every class against every class in all components, and every element beside two others
inline std::vector<std::pair<int, int>> pairs(int n) {
    std::vector<std::pair<int, int>> r;
    for (int a = 0; a < N_CLS; a++) for (int b = 0; b < N_CLS; b++) r.push_back({a, b});      // (elements 0 .. N_CLS - 1: "all <class>")
    for (int i = N_CLS; i < n; i++) { r.push_back({i, (7 * i + 3) % n}); r.push_back({(11 * i + 5) % n, i}); }
    return r;
}

// the element as a tower value over canonical residues (the reference side of every comparison)
inline Fq12S to_tower(const Elt &e) {
    Fq12S t;
    for (int k = 0; k < 6; k++) w12_tower_ref(t, k) = Fq2S{Fs{e[2 * k].canonical()}, Fs{e[2 * k + 1].canonical()}};
    return t;
}
inline Elt from_slots(const Fq2S *s) {
    Elt e;
    for (int k = 0; k < 6; k++) { e[2 * k] = s[k].c0.v; e[2 * k + 1] = s[k].c1.v; }
    return e;
}
inline void to_slots(const Elt &e, Fq2S *s) {
    for (int k = 0; k < 6; k++) s[k] = Fq2S{Fs{e[2 * k]}, Fs{e[2 * k + 1]}};
}
// canonical 256-bit values equal, component by component
inline bool same_value(const Elt &got, Fq12S want) {
    for (int k = 0; k < 6; k++) {
        const Fq2S &w = w12_tower_ref(want, k);
        if (!(got[2 * k].to_mont256() == w.c0.to_mont256()) || !(got[2 * k + 1].to_mont256() == w.c1.to_mont256())) return false;
    }
    return true;
}
inline bool within_contract(const Elt &e) {
    for (const F29 &c : e) if (!tight_below(c, 2)) return false;
    return true;
}
// a line {ell_0, ell_VW, ell_VV} (the first three coefficients of `line`) as a full element: polynomial positions 0, 3, 4
inline Elt embed_line(const Elt &line) {
    Elt e;
    for (F29 &c : e) c = F29::zero();
    e[0] = line[0]; e[1] = line[1]; e[6] = line[2]; e[7] = line[3]; e[8] = line[4]; e[9] = line[5];
    return e;
}

}  // namespace w12edge
