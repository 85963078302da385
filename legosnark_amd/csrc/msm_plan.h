// legosnark_amd/csrc/msm_plan.h -- the digit plan of the wide-window MSM pipelines (msm.hip, msm_compact.hip):
// where the pre-shifted copies of a resident base table sit, which windows a call of a given size uses, and the
// signed-digit recoding of one scalar.  Shared so that every pipeline cuts a scalar the same way.
// Also the whole plan of msm.hip's general pipeline (plan_pipeline): every path flag, size, dynamic-LDS request and
// workspace offset of a call as a pure function of its shape and the LSA_* switches.  No HIP type, no getenv, no global
// state: tests/cpp/test_msm_plan.cc checks on the host what the kernels rely on.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "bn254_constants.h"
#include "fp.h"

namespace lsa {

struct WidePlan {
    unsigned nwin;        // digits per scalar
    unsigned c;           // widest window: 2^(c-1) buckets
    unsigned copy_step;   // window k gathers from table copy k * copy_step
    unsigned start[32];   // window k covers bits [start[k], start[k] + width[k])
    unsigned width[32];
};

// Copy j of the table holds 2^(pos[j]) * P.  The positions are the starts of 13 (12 from 6*2^20
// points on) wide windows that split the 255 scalar bits as evenly as possible (8 x 20 + 5 x 19
// bits; 3 x 22 + 9 x 21) plus the midpoint of each: wide digits use every other copy, narrow
// digits (10 or 9 bits; 11 or 10) all of them.  Even widths matter: a short window concentrates
// its digits on few buckets, and the longest bucket list bounds the accumulate kernel.
struct TableGrid {
    unsigned ncopies;
    unsigned pos[33];     // pos[ncopies] = 255
};
inline TableGrid table_grid(size_t n_table) {
    TableGrid t;
    const unsigned nbig = n_table >= ((size_t)6 << 20) ? 12u : 13u;
    const unsigned base = 255 / nbig, rem = 255 % nbig;
    unsigned bit = 0;
    for (unsigned k = 0; k < nbig; k++) {
        const unsigned w = base + (k < rem ? 1u : 0u);
        t.pos[2 * k] = bit;
        t.pos[2 * k + 1] = bit + (w + 1) / 2;
        bit += w;
    }
    t.ncopies = 2 * nbig;
    t.pos[t.ncopies] = 255;
    return t;
}

// big: 13 (12) wide digits over every other copy; otherwise all 26 (24) positions as narrow digits
inline WidePlan wide_plan_for(size_t n_table, bool big) {
    const TableGrid t = table_grid(n_table);
    WidePlan pl = {};
    pl.copy_step = big ? 2 : 1;
    pl.nwin = t.ncopies / pl.copy_step;
    pl.c = 0;
    for (unsigned k = 0; k < pl.nwin; k++) {
        pl.start[k] = t.pos[k * pl.copy_step];
        pl.width[k] = t.pos[(k + 1) * pl.copy_step] - pl.start[k];
        if (pl.width[k] > pl.c) pl.c = pl.width[k];
    }
    return pl;
}

// ------------------------------------------------------------------------------------
// Sizes the kernels of msm.hip (msm_sort.h .. msm_reduce.h) are written for, and what they pass between each other
// ------------------------------------------------------------------------------------
#define SORT_TILE 32768u        // plain path: scalars per workgroup of k_rank / k_scatter (u16 ranks)
#define SCAN_PER_BLOCK 2048     // counters per 256-lane block of the three scan kernels
#define WIDE_FINE_BITS 7u       // fine bits of a 64-bit record (k_scatter_wide<1> / k_fine_sort<u64>); 32-bit records: 6
#define MSM_MAX_SEGMENTS 64u
#define PART_TILE 2048u
#define PART_SEGS 768u          // at most: 512 bins of 2^9 buckets below B/2 and 256 of 2^10 above, at 2^19 buckets
#define PART_STAGE 28672u       // records the second pass can stage in LDS (a segment holds 26624 +- 160 at n = 2^20)
#define SIZE_BINS 1025          // bin 0 unused (total), bins 1..1024
#define HEAVY_CHUNK 512u

// Dynamic LDS above 64 KiB needs an opt-in per kernel (msm_func_attrs): the largest request each kernel may see.
constexpr uint32_t LDS_MAX_BIN_WORDS = 131072;                 // k_scatter, k_scatter_wide<0|1|2>: one u32 per bin
constexpr uint32_t LDS_MAX_BIN_HALVES = 65536;                 // k_rank, k_hist_wide: one u16 per bin
constexpr uint32_t LDS_MAX_PARTITION = 13 * PART_TILE * 4;     // k_partition: a tile's records, at most 13 windows
constexpr uint32_t LDS_MAX_FINE_SORT_PART = 155648;            // k_fine_sort_part: counters, tile bases and the record stage

// scalar slices of a segmented call: segment j = scalars[off[j] .. off[j+1]) against bases[0 .. len_j)
struct SegList {
    uint32_t nseg;
    uint32_t off[MSM_MAX_SEGMENTS + 1];
};

// Bucket -> coarse bin of the first sort pass.  Windows of the widest width c reach all 2^(c-1)
// buckets, windows one bit narrower (5 of the 13 at n = 2^20) only the lower half, so a bucket of
// the lower half holds more than twice as many entries as one of the upper half (36 against 16):
// bins of equal POPULATION take 2^sh_lo buckets below `half` and 2^sh_hi above.  half = 0 makes it a
// plain shift by sh_hi.
struct CoarseMap {
    uint32_t half, sh_lo, sh_hi, nlo;      // nlo = half >> sh_lo bins below `half`
    LSA_HD uint32_t bin(uint32_t b) const { return b < half ? b >> sh_lo : nlo + ((b - half) >> sh_hi); }
    LSA_HD uint32_t fine(uint32_t b) const { return b < half ? b & ((1u << sh_lo) - 1) : (b - half) & ((1u << sh_hi) - 1); }
    // bin -> its first bucket and its bucket count
    LSA_HD uint32_t first(uint32_t bin_) const { return bin_ < nlo ? bin_ << sh_lo : half + ((bin_ - nlo) << sh_hi); }
    LSA_HD uint32_t bits(uint32_t bin_) const { return bin_ < nlo ? sh_lo : sh_hi; }
};

// window width of the plain path (no pre-shifted copies)
inline unsigned msm_window_bits(size_t n) {
    unsigned lg = 0;
    while ((size_t(1) << (lg + 1)) <= n) lg++;   // floor(log2 n), 0 for n <= 1
    int c = (int)lg - 4;
    if (c < 8) c = 8;        // few, wide windows keep the latency-bound fold short for tiny inputs
    if (c > 16) c = 16;
    return (unsigned)c;
}

inline unsigned num_windows(unsigned c) { return (255 + c - 1) / c; }

// Scalars per workgroup of the wide path's ranking / scatter passes: a tile's entries (nwin per
// scalar) must fit the u16 counters even when every one of them lands in the same bin
// (all scalars equal, all their digits equal): 13 x 4096 or 26 x 2048 = 53248 < 65536.
// Small inputs get 256- or 1024-scalar tiles: a lone workgroup ranking
// 26 digits of 1024 scalars keeps ONE CU's LDS busy for 13 + 17 us (hist + scatter); with more
// tiles the LDS atomics of a call spread over several CUs.
inline uint32_t wide_tile(uint32_t nwin, size_t n) {
    if (n <= 4096) return 256u;
    if (n <= 16384) return 1024u;
    return nwin > 15 ? 2048u : 4096u;
}

// ------------------------------------------------------------------------------------
// The plan of one call of the general pipeline
// ------------------------------------------------------------------------------------
// What the LSA_* variables and lsa_msm_set_table_threshold decide; msm.hip fills one per process.
struct MsmSwitches {
    bool no_rec32 = false;            // LSA_NO_REC32: 64-bit records in the two-pass sort even where 32 bits do
    bool no_part = false;             // LSA_NO_PART: k_scatter_wide / k_fine_sort instead of the partitioned sort
    uint32_t wide_split = 1;          // LSA_WIDE_SPLIT=2: two lanes per bucket on the wide path too
    bool g2_pair = false;             // LSA_G2_PAIR=1: k_accumulate_g2_pair
    bool no_reduce_bits = false;      // LSA_NO_REDUCE_BITS: blocking calls reduce through 16-ary levels only
    bool no_lane_l1 = false;          // LSA_NO_LANE_L1: never the lane-private first 16-ary level
    bool g2_lane_l1 = false;          // LSA_G2_LANE_L1=1: ... for G2 as well
    size_t wide_big_min = (size_t)1 << 16;   // LSA_WIDE_BIG_MIN: calls of at least this many pairs take the wide digits
    size_t table_use_min = 1;         // lsa_msm_set_table_threshold(n != 0): smaller calls ignore a handle's copies
};

struct MsmShape {
    int group;                 // 1 | 2
    size_t acc_bytes;          // sizeof the curve's bucket accumulator (XYZZ, 29-bit limbs)
    size_t jac_bytes;          // sizeof a result point
    bool glv;                  // the curve's plain path splits scalars (G1)
    size_t n;                  // pairs, all segments together
    uint32_t nseg;
    size_t table_stride;       // points per copy of a table-carrying handle, 0: no copies
    bool blocking, reuse_sort;
};

enum PlanStatus {
    PLAN_OK = 0,
    PLAN_N_TOO_LARGE,             // n >= 2^27
    PLAN_SEGMENTS_NEED_COPIES,    // nseg > 1 on bases without pre-shifted copies
    PLAN_TABLE_TOO_LARGE,         // stride * copies does not fit the 30-bit point reference of an entry
    PLAN_BIN_SPACE,               // nseg * B > 2^21
};

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// A workspace is carved front to back, every region on a 256-byte boundary; `bytes` is what was asked for.
struct WsRegion { size_t off, bytes; };
enum FrontRegion {
    F_HIST,      // u32[nb] bucket populations, + the heavy_count word
    F_OFFS,      // u32[nb] bucket offsets into the entries
    F_BSUM,      // u32[scan_blocks]
    F_BINS,      // u32[3][SIZE_BINS]: bin_count | bin_start | bin_cursor
    F_PERM,      // u32[nb] buckets by population
    F_DIGITS,    // plain path: i32[ne]
    F_RANK,      // plain path: u16[ne] (the wide passes hand out positions with LDS atomics)
    F_THIST,     // u16[rows][pitch]
    F_TBASE,     // u32[rows][pitch]
    F_ENTRIES,   // u32[ne]
    F_HEAVY,     // u32[max_heavy]
    F_CHOFF,     // u32[max_heavy + 2]: chunk offsets, the chunk count, the chunk size
    F_HPART,     // Acc[max_chunks]
    F_RECS,      // two-pass sort: coarse-sorted records
    F_CHIST,     // two-pass sort: u32[Bc]
    F_COFFS,     // two-pass sort: u32[Bc]
    F_REGIONS
};
enum TailRegion {
    T_BUCKETS,   // Acc[nb * split]
    T_WAVE,      // Acc[kw * wpw * 2]: leaves the first reduction level
    T_WIN,       // Acc[kw * ceil(wpw / 16) * 2]: the 16-ary levels ping-pong between the two
    T_RES,       // Jac[nseg]: this call's result(s) before they are published
    T_REGIONS
};
template <int N>
struct WsLayout {
    WsRegion r[N];
    size_t total;
    size_t operator[](int i) const { return r[i].off; }
    void carve(int i, size_t bytes) {      // regions in enumeration order
        r[i].off = i == 0 ? 0 : total;
        r[i].bytes = bytes;
        total = align_up(r[i].off + bytes, 256);
    }
};

struct PipelinePlan {
    PlanStatus status;
    size_t n;                  // the shape, as given
    uint32_t nseg;
    bool reuse_sort;
    // path
    bool wide;                 // over the pre-shifted copies: all windows share one bucket space per segment
    bool glv;
    bool fine;                 // two-pass sort
    bool rec32;                // ... with 32-bit records (6 fine bits), else 64-bit ones (7 fine bits)
    bool part;                 // ... partitioned (k_partition / k_fine_sort_part)
    bool big;                  // throughput-shaped reduction
    // digits and buckets
    WidePlan pl;
    unsigned c, nwin;
    size_t nv, ne;             // virtual scalars, entries
    uint32_t B, nb;            // buckets per space, buckets
    uint32_t Bc;               // bins of the first sort pass
    CoarseMap cm;
    uint32_t fine_bits;        // (of the k_scatter_wide / k_fine_sort path)
    uint32_t win_stride;       // wide: entries of window k point into copy k * copy_step
    // sort geometry
    uint32_t ntiles, wtile, wtiles;
    size_t rows;
    uint32_t pitch;            // elements between rows of the tile arrays (see k_tile_scan_rows)
    uint32_t nscan, scan_blocks;
    // accumulate
    uint32_t split;            // lanes per bucket in k_accumulate
    bool g2_pair;              // G2, one lane per bucket: k_accumulate_g2_pair instead of k_accumulate_g2_occ2
    uint32_t heavy_threshold, bin_shift, max_heavy;
    size_t max_chunks;
    // reduction
    uint32_t L, logL, T, wpw, kw;
    bool bits_tail;            // bit trees after the first 16-ary level
    bool lane_l1_shape;        // the shape half of "first 16-ary level lane-private"; the other half is the previous slot's state
    // dynamic LDS, bytes
    size_t lds_hist_wide, lds_scatter_wide, lds_rank, lds_scatter, lds_partition, lds_fine_sort_part;
    uint32_t fixed_words, stage_cap;      // k_fine_sort_part
    // workspaces
    WsLayout<F_REGIONS> front;
    WsLayout<T_REGIONS> tail;
};

inline unsigned table_copies(size_t n_table) { return table_grid(n_table).ncopies; }
inline WidePlan wide_plan(size_t n_table, size_t n_call, unsigned nseg, const MsmSwitches &sw) {
    return wide_plan_for(n_table, nseg == 1 && n_call >= sw.wide_big_min);
}

inline PipelinePlan plan_pipeline(const MsmShape &sh, const MsmSwitches &sw) {
    PipelinePlan p = {};
    p.n = sh.n; p.nseg = sh.nseg; p.reuse_sort = sh.reuse_sort;
    const size_t n = sh.n, table_stride = sh.table_stride;
    const uint32_t nseg = sh.nseg;
    if (n >= (size_t(1) << 27)) { p.status = PLAN_N_TOO_LARGE; return p; }
    const bool wide = table_stride != 0 && (nseg > 1 || n >= sw.table_use_min);
    if (nseg > 1 && !wide) { p.status = PLAN_SEGMENTS_NEED_COPIES; return p; }
    WidePlan pl = {};
    if (wide) {
        pl = wide_plan(table_stride, n, nseg, sw);
        if ((uint64_t)table_stride * table_copies(table_stride) >= (1u << 30)) { p.status = PLAN_TABLE_TOO_LARGE; return p; }
    }
    const bool glv = sh.glv && !wide;
    const unsigned c = wide ? pl.c : msm_window_bits(glv ? 2 * n : n);       // plain path: sized by the virtual scalars
    const unsigned nwin = wide ? pl.nwin : (glv ? (128 + c - 1) / c : num_windows(c));   // |k1|,|k2| < 2^127 (glv.h)
    const size_t nv = glv ? 2 * n : n;                                       // virtual scalars
    const uint32_t B = 1u << (c - 1);
    const uint32_t nb = wide ? nseg * B : nwin * B;                          // wide: one bucket space per segment, shared by all windows
    if (wide && (uint64_t)nseg * B > (1u << 21)) { p.status = PLAN_BIN_SPACE; p.B = B; return p; }
    const bool fine = wide && nb > 32768;                                    // two-pass sort
    // 32-bit records (6 fine bits) when every point reference fits 25 bits, else 64-bit ones (7 fine bits)
    const bool rec32 = fine && !sw.no_rec32 && (uint64_t)table_stride * table_copies(table_stride) < (1u << 25) && (nb >> 6) <= 32768;
    // partitioned sort (k_partition / k_fine_sort_part): one large MSM whose tile count fits the second pass's LDS
    const bool part = fine && !sw.no_part && nseg == 1 && nwin <= 13 && n <= ((size_t)1 << 25) && (nb & (nb - 1)) == 0 && nb >= (1u << 19);
    const uint32_t fine_bits = rec32 ? 6u : WIDE_FINE_BITS;
    CoarseMap cm = {0u, 0u, fine ? fine_bits : 0u, 0u};
    uint32_t Bc = !wide ? B : (fine ? nb >> fine_bits : nb);
    if (part) {
        // 512 bins below B/2 and 256 above when some windows are a bit narrower than the widest
        // (they only reach the lower half of the buckets), 512 equal bins otherwise
        bool narrower = false;
        for (unsigned k = 0; k < nwin; k++) narrower |= pl.width[k] < c;
        unsigned lg = 0;
        while ((1u << lg) < B) lg++;
        if (narrower) { cm.half = B >> 1; cm.sh_lo = lg - 1 - 9; cm.sh_hi = lg - 1 - 8; cm.nlo = 512; Bc = 768; }
        else { cm.half = 0; cm.sh_lo = cm.sh_hi = lg - 9; cm.nlo = 0; Bc = 512; }
    }
    const size_t ne = nv * nwin;
    const bool big = wide && B > 4096;
    const uint32_t split = wide ? (sw.wide_split == 2 ? 2u : 1u) : 2u;
    // first reduction level: quads over L buckets (latency) or, for 2^19+ buckets, lanes over L buckets (throughput)
    // (a quad-shared first level over 2^19 buckets was measured too: 0.69 - 1.27 ms against 0.63 ms)
    // (G2, measured in round 6 with 32768 / 16384 / 8192 first-level lanes instead of 65536 -- longer lane-private chains, a half
    // to an eighth of the quad level's work behind them: pipelined 2^20-pair G2 MSMs 4.75-5.07 -> 4.80 / 5.41 / 6.78 ms.  65536 stays.)
    const uint32_t L = big ? (B / 65536 > 1 ? B / 65536 : 1) : (B > 4096 ? B / 4096 : 1);
    uint32_t logL = 0;
    while ((1u << logL) < L) logL++;
    const uint32_t T = B / L;                        // first-level segments per window
    const uint32_t wpw = big ? T : (T + 15) / 16;    // (ACC,RUN) pairs per window leaving level 1
    const uint32_t kw = wide ? nseg : nwin;          // bucket spaces ("windows") entering the reduction
    // Buckets far above the average population (skewed scalars; the partly filled top window)
    // are split across workgroups instead of being walked by their owner lanes.  With narrow
    // digits every bucket is long (26*n/512 entries), and the point of that path is latency:
    // anything above 4 entries is cut into chunks summed by a wavefront each.
    const uint32_t avg_pop = (uint32_t)(ne / nb + 1);
    // wide digits: the fullest buckets are those of the lower half, which every window reaches -- n / B
    // entries from each window of the widest width, twice that from each narrower one (36 at n = 2^20, 168
    // at n = 2^24); twice that expectation (6 sigma and more) separates them from skewed inputs, whose
    // long single-lane lists would otherwise bound the accumulate kernel (runs of equal scalars: 3.9 -> 3.2 ms)
    uint32_t pop_lo = avg_pop;
    if (wide && big) {
        unsigned nfull = 0;
        for (unsigned k = 0; k < nwin; k++) nfull += pl.width[k] == c;
        pop_lo = (uint32_t)(((uint64_t)n * (nfull + 2 * (nwin - nfull))) / B + 1);
    }
    const uint32_t pop = wide ? pop_lo : avg_pop;
    const uint32_t heavy_threshold = (wide && !big) ? 4u : (2 * pop + 32 > 64 ? 2 * pop + 32 : 64u);
    uint32_t bin_shift = 0;                          // populations above 1024 share bins (the order only balances wavefronts)
    while (((heavy_threshold - 1) >> bin_shift) + 1 > SIZE_BINS - 1) bin_shift++;
    const uint32_t max_heavy = (uint32_t)(ne / heavy_threshold + 1 < nb ? ne / heavy_threshold + 1 : nb);
    const size_t max_chunks = ne / HEAVY_CHUNK + max_heavy + 1;
    const uint32_t nscan = wide ? Bc : nb;           // counters the generic scan runs over
    const uint32_t scan_blocks = (nscan + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK;   // <= 1024 since nscan <= 2^20
    const uint32_t ntiles = (uint32_t)((nv + SORT_TILE - 1) / SORT_TILE);
    const uint32_t wtile = part ? PART_TILE : wide_tile(nwin, n);
    const uint32_t wtiles = (uint32_t)((n + wtile - 1) / wtile);             // wide path: one row per tile (all windows)
    const size_t rows = wide ? wtiles : (size_t)nwin * ntiles;
    const uint32_t pitch = wide ? Bc + 96 : Bc;

    p.status = PLAN_OK;
    p.wide = wide; p.glv = glv; p.fine = fine; p.rec32 = rec32; p.part = part; p.big = big;
    p.pl = pl; p.c = c; p.nwin = nwin; p.nv = nv; p.ne = ne; p.B = B; p.nb = nb; p.Bc = Bc; p.cm = cm; p.fine_bits = fine_bits;
    p.win_stride = wide ? (uint32_t)(table_stride * pl.copy_step) : 0u;
    p.ntiles = ntiles; p.wtile = wtile; p.wtiles = wtiles; p.rows = rows; p.pitch = pitch; p.nscan = nscan; p.scan_blocks = scan_blocks;
    p.split = split; p.g2_pair = sh.group == 2 && split == 1 && sw.g2_pair; p.heavy_threshold = heavy_threshold; p.bin_shift = bin_shift; p.max_heavy = max_heavy; p.max_chunks = max_chunks;
    p.L = L; p.logL = logL; p.T = T; p.wpw = wpw; p.kw = kw;
    // one bucket space of 2^19 and more buckets: after the first 16-ary level the rest are bit trees
    // (for blocking calls only: the trees are ~45 us shorter in latency and ~1 % more work than the levels they replace,
    // which is the wrong trade for calls whose tails hide under the next call's front)
    p.bits_tail = !sw.no_reduce_bits && sh.blocking && big && kw == 1 && nseg == 1 && wpw >= 4096 && (wpw / 16) <= 8192;
    // pipelined wide calls: the first 16-ary level lane-private (k_reduce2_lane: a seventh of the quad level's work)
    // (G1 only: 48 sequential G2 additions are 1.2 ms of latency.  The second half of a commitment pair (reuse_sort) is
    // waited for right away and would pay the lane kernel's 0.2 ms of extra latency: 6.0 -> 6.25 ms.)
    // (G2, measured in round 6: lane-private, this level is 64 wavefronts at 256 VGPRs + 228 B of scratch and runs longer than
    // the step it should hide under -- pipelined 2^20-pair G2 MSMs 4.76 -> 5.03 ms.  LSA_G2_LANE_L1=1 selects it all the same.)
    p.lane_l1_shape = !sw.no_lane_l1 && (sh.group == 1 || sw.g2_lane_l1) && !sh.blocking && !sh.reuse_sort && big && kw == 1 && nseg == 1 && wpw >= 16384;

    p.lds_hist_wide = (size_t)((Bc + 1) / 2) * 4;
    p.lds_scatter_wide = (size_t)Bc * 4;
    p.lds_rank = (size_t)B * 2;
    p.lds_scatter = (size_t)B * 4;
    p.lds_partition = (size_t)nwin * PART_TILE * 4;
    if (part) {
        p.fixed_words = 2 * (1u << cm.sh_hi) + wtiles + 1;
        p.stage_cap = p.fixed_words + PART_STAGE <= LDS_MAX_FINE_SORT_PART / 4 ? PART_STAGE : 0u;   // larger problems have larger segments anyway
    }
    p.lds_fine_sort_part = (size_t)(p.fixed_words + p.stage_cap) * 4;

    p.front.carve(F_HIST, (size_t)nb * 4 + 256);     // + heavy_count word
    p.front.carve(F_OFFS, (size_t)nb * 4);
    p.front.carve(F_BSUM, (size_t)scan_blocks * 4);
    p.front.carve(F_BINS, (size_t)3 * SIZE_BINS * 4);
    p.front.carve(F_PERM, (size_t)nb * 4);
    p.front.carve(F_DIGITS, wide ? 0 : ne * 4);
    p.front.carve(F_RANK, wide ? 0 : ne * 2);
    p.front.carve(F_THIST, rows * pitch * 2);
    p.front.carve(F_TBASE, rows * pitch * 4);
    p.front.carve(F_ENTRIES, ne * 4);
    p.front.carve(F_HEAVY, (size_t)max_heavy * 4);
    p.front.carve(F_CHOFF, (size_t)(max_heavy + 2) * 4);
    p.front.carve(F_HPART, max_chunks * sh.acc_bytes);
    p.front.carve(F_RECS, fine ? ne * (part || rec32 ? 4 : 8) : 0);
    p.front.carve(F_CHIST, fine ? (size_t)Bc * 4 : 0);
    p.front.carve(F_COFFS, fine ? (size_t)Bc * 4 : 0);

    p.tail.carve(T_BUCKETS, (size_t)nb * split * sh.acc_bytes);
    p.tail.carve(T_WAVE, (size_t)kw * wpw * 2 * sh.acc_bytes);
    p.tail.carve(T_WIN, (size_t)kw * ((wpw + 15) / 16) * 2 * sh.acc_bytes);
    p.tail.carve(T_RES, (size_t)nseg * sh.jac_bytes);
    return p;
}

#if defined(__HIPCC__)
// Signed digits of one scalar, produced one window at a time (the carry chain is sequential) and
// handed to `use(k, sd)` with sd = +-(segment * B + |digit|), 0 for a zero digit -- no digit
// array: the ranking pass and the scatter pass both recompute them from the scalar (a Montgomery
// reduction and a few shifts per scalar) instead of writing 4 B per digit to HBM and reading
// them back twice.
template <class Use>
__device__ __forceinline__ void wide_digits(const Fr &scalar, const WidePlan &pl, uint32_t seg_base, Use use) {
    uint32_t s[8];
    scalar.to_canonical(s);
    // balanced representative: s > (r-1)/2 is recoded as -(r - s), i.e. the digits of r - s with
    // every sign flipped.  Same sum; "small negative" scalars (r - 1, r - 2, ...: ten of their
    // thirteen digits would be the digits of r, the same ten buckets for every such scalar) become
    // small digits, and the top window never exceeds a quarter of its range.
    bool flip;
    {
        uint32_t t[8];
        uint64_t br = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {                  // t = r - s
            const uint64_t x = (uint64_t)LSA_R[i] - s[i] - br;
            t[i] = (uint32_t)x;
            br = (x >> 32) & 1;
        }
        br = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) br = (((uint64_t)t[i] - s[i] - br) >> 32) & 1;      // borrow out <=> t < s <=> 2 s > r
        flip = br != 0;
#pragma unroll
        for (int i = 0; i < 8; i++) s[i] = flip ? t[i] : s[i];
    }
    // consume the limbs through a 64-bit bit buffer (static limb index: no register-array indexing)
    uint64_t buf = 0;
    unsigned have = 0, k = 0;
    uint32_t carry = 0;
#pragma unroll
    for (int limb = 0; limb < 8; limb++) {
        buf |= (uint64_t)s[limb] << have;
        have += 32;
        while (k < pl.nwin && (have >= pl.width[k] || limb == 7)) {
            const unsigned width = pl.width[k];
            uint32_t d = (uint32_t)buf & ((1u << width) - 1);
            buf >>= width;
            have = have >= width ? have - width : 0;
            d += carry;
            int32_t sd;
            // the top window is never recoded: scalars are < 2^254 and the windows cover 255 bits, so
            // its raw value is < 2^(width-1) and the carry keeps it <= 2^(width-1) <= B
            if (k + 1 < pl.nwin && d >= (1u << (width - 1))) { sd = (int32_t)d - (int32_t)(1u << width); carry = 1; }
            else { sd = (int32_t)d; carry = 0; }
            if (sd != 0) { const int32_t m = (int32_t)seg_base + (sd < 0 ? -sd : sd); sd = (sd < 0) != flip ? -m : m; }
            use(k, sd);
            k++;
        }
    }
}

#endif

}  // namespace lsa
