// legosnark_amd/csrc/msm_sort.h -- stages 1-3 of the MSM pipeline (msm.hip): the three sort fronts.
// Scalars -> signed digits -> entries ordered by bucket, with the bucket populations and offsets: the plain path
// (k_digits .. k_scatter), the wide path (k_hist_wide, k_tile_scan_rows, k_scatter_wide + k_fine_sort) and its
// partitioned form (k_partition + k_fine_sort_part).  Device code only, compiled by msm.hip (launch_sort).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "curves.h"
#include "glv.h"
#include "msm_plan.h"

namespace lsa {

// ------------------------------------------------------------------------------------
// kernels 1a-1c: digits, LDS ranking, tile prefix.  No global atomics.
//   1a k_digits     scalars (Montgomery Fr, read once, coalesced) -> canonical -> signed
//                   c-bit digits, digits[k][i] (int16).
//   1b k_rank       one workgroup per (tile of TILE scalars, window): a bucket histogram of
//                   the tile lives in LDS (u16 counters packed in pairs, <= 64 KiB); each
//                   non-zero digit takes its rank inside (tile, bucket) with ONE returning
//                   LDS atomic.  rank[k][i] (u16) and the tile histogram go to HBM.
//   1c k_tile_scan  per (window, bucket): exclusive prefix over the tiles (u32) and the
//                   bucket population hist[k][b].
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void write_digits(const uint32_t *s, int nlimbs, bool negate, size_t col, size_t nv, unsigned c,
                                             unsigned nwin, int32_t *__restrict__ digits) {
    const uint32_t B = 1u << (c - 1);
    uint32_t carry = 0;
    for (unsigned k = 0; k < nwin; k++) {
        unsigned bit = k * c;
        int w = (int)(bit >> 5);
        unsigned sh = bit & 31;
        uint64_t two = (uint64_t)(w < nlimbs ? s[w] : 0) | ((uint64_t)(w + 1 < nlimbs ? s[w + 1] : 0) << 32);
        uint32_t d = (uint32_t)(two >> sh) & ((1u << c) - 1);
        d += carry;
        int32_t sd;
        if (k + 1 < nwin && d >= B) { sd = (int32_t)d - (int32_t)(1u << c); carry = 1; }
        else { sd = (int32_t)d; carry = 0; }
        digits[(size_t)k * nv + col] = negate ? -sd : sd;
    }
}
// GLV: scalar i yields two virtual scalars, columns i (k1, point i) and n+i (k2, phi(point i)).
template <bool GLV>
__global__ __launch_bounds__(256) void k_digits(const Fr *__restrict__ scalars, size_t n, unsigned c, unsigned nwin,
                                                int32_t *__restrict__ digits) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s[8];
    scalars[i].to_canonical(s);
    if (GLV) {
        GlvSplit g = glv_decompose(s);
        write_digits(g.k1, 4, g.neg1, i, 2 * n, c, nwin, digits);
        write_digits(g.k2, 4, g.neg2, n + i, 2 * n, c, nwin, digits);
    } else {
        write_digits(s, 8, false, i, n, c, nwin, digits);
    }
}

// `shift` != 0 (wide path): the histogram runs over the coarse bins b >> shift (B = number of bins).
__global__ __launch_bounds__(1024) void k_rank(const int32_t *__restrict__ digits, size_t n, uint32_t B, uint32_t ntiles,
                                               uint16_t *__restrict__ rank, uint16_t *__restrict__ tile_hist, uint32_t shift) {
    extern __shared__ __attribute__((aligned(16))) uint32_t cnt2[];   // B/2 words: two u16 counters each
    const uint32_t t = blockIdx.x, k = blockIdx.y;
    for (uint32_t x = threadIdx.x; x < B / 2; x += 1024) cnt2[x] = 0;
    __syncthreads();
    const size_t lo = (size_t)t * SORT_TILE;
    const size_t hi = lo + SORT_TILE < n ? lo + SORT_TILE : n;
    const int32_t *dg = digits + (size_t)k * n;
    uint16_t *rk = rank + (size_t)k * n;
    for (size_t i = lo + threadIdx.x; i < hi; i += 1024) {
        int32_t sd = dg[i];
        if (sd != 0) {
            uint32_t b = ((uint32_t)(sd < 0 ? -sd : sd) - 1) >> shift;
            uint32_t sh = (b & 1) * 16;
            uint32_t old = atomicAdd(&cnt2[b >> 1], 1u << sh);      // ds_add_rtn_u32
            rk[i] = (uint16_t)(old >> sh);
        }
    }
    __syncthreads();
    uint32_t *th = reinterpret_cast<uint32_t *>(tile_hist + ((size_t)k * ntiles + t) * B);
    for (uint32_t x = threadIdx.x; x < B / 2; x += 1024) th[x] = cnt2[x];
}

// (wide path: called with ntiles = nwin * ntiles and nb = B, i.e. every (window, tile) pair is a
// row of ONE bin space -- the pre-shifted copies make the windows interchangeable)
__global__ __launch_bounds__(256) void k_tile_scan(const uint16_t *__restrict__ tile_hist, uint32_t B, uint32_t ntiles, uint32_t nb,
                                                   uint32_t *__restrict__ tile_base, uint32_t *__restrict__ hist) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;      // g = k*B + b
    if (g >= nb) return;
    uint32_t k = g / B, b = g - k * B;
    uint32_t run = 0;
    for (uint32_t t = 0; t < ntiles; t++) {
        size_t idx = ((size_t)k * ntiles + t) * B + b;
        tile_base[idx] = run;
        run += tile_hist[idx];
    }
    hist[g] = run;
}

// ------------------------------------------------------------------------------------
// kernel 2: exclusive scan of `count` counters in three small launches:
//   a) per-block sums (2048 counters per 256-lane block, LDS-free wave shuffles)
//   b) one block scans the <= 1024 block sums
//   c) per-block exclusive scan seeded with the block offset
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t block_exclusive_scan_256(uint32_t v, uint32_t *lds, uint32_t *total) {
    // 256 lanes; wave-level shuffles then 4 wave totals through LDS
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(incl, d, 64);
        if ((int)lane >= d) incl += t;
    }
    if (lane == 63) lds[wv] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (unsigned w = 0; w < 4; w++) { uint32_t x = lds[w]; if (w < wv) base += x; tot += x; }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

__global__ __launch_bounds__(256) void k_scan_sums(const uint32_t *__restrict__ hist, uint32_t count, uint32_t *__restrict__ block_sums) {
    __shared__ uint32_t lds[4];
    const uint32_t base = blockIdx.x * SCAN_PER_BLOCK + threadIdx.x * 8;
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) if (base + j < count) s += hist[base + j];
    uint32_t tot;
    (void)block_exclusive_scan_256(s, lds, &tot);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_scan_blocks(uint32_t *__restrict__ block_sums, uint32_t nblocks) {
    __shared__ uint32_t lds[4];
    // nblocks <= 1024: 4 per lane
    uint32_t v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) { uint32_t idx = threadIdx.x * 4 + j; v[j] = idx < nblocks ? block_sums[idx] : 0; s += v[j]; }
    uint32_t tot;
    uint32_t run = block_exclusive_scan_256(s, lds, &tot);
#pragma unroll
    for (int j = 0; j < 4; j++) { uint32_t idx = threadIdx.x * 4 + j; if (idx < nblocks) block_sums[idx] = run; run += v[j]; }
}

__global__ __launch_bounds__(256) void k_scan_final(const uint32_t *__restrict__ hist, const uint32_t *__restrict__ block_sums,
                                                    uint32_t count, uint32_t *__restrict__ offs) {
    __shared__ uint32_t lds[4];
    const uint32_t base = blockIdx.x * SCAN_PER_BLOCK + threadIdx.x * 8;
    uint32_t v[8], s = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { v[j] = (base + j < count) ? hist[base + j] : 0; s += v[j]; }
    uint32_t tot;
    uint32_t run = block_sums[blockIdx.x] + block_exclusive_scan_256(s, lds, &tot);
#pragma unroll
    for (int j = 0; j < 8; j++) { if (base + j < count) offs[base + j] = run; run += v[j]; }
}

// ------------------------------------------------------------------------------------
// kernel 3: scatter.  One workgroup per (tile, window) loads base[b] = offs[k][b] +
// tile_base[k][t][b] into LDS (<= 128 KiB) and writes entry (point index | sign<<31) at
// base[b] + rank.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_scatter(const int32_t *__restrict__ digits, const uint16_t *__restrict__ rank,
                                                  const uint32_t *__restrict__ offs, const uint32_t *__restrict__ tile_base,
                                                  size_t n, size_t npoints, uint32_t B, uint32_t ntiles, uint32_t *__restrict__ entries,
                                                  uint32_t win_stride) {
    extern __shared__ __attribute__((aligned(16))) uint32_t base[];   // B words
    const uint32_t t = blockIdx.x, k = blockIdx.y;
    const uint32_t *of = offs + (size_t)k * B;
    const uint32_t *tb = tile_base + ((size_t)k * ntiles + t) * B;
    for (uint32_t x = threadIdx.x; x < B; x += 1024) base[x] = of[x] + tb[x];
    __syncthreads();
    const size_t lo = (size_t)t * SORT_TILE;
    const size_t hi = lo + SORT_TILE < n ? lo + SORT_TILE : n;
    const int32_t *dg = digits + (size_t)k * n;
    const uint16_t *rk = rank + (size_t)k * n;
    for (size_t i = lo + threadIdx.x; i < hi; i += 1024) {
        int32_t sd = dg[i];
        if (sd != 0) {
            uint32_t b = (uint32_t)(sd < 0 ? -sd : sd) - 1;
            // entry = point index | endo << 30 | sign << 31   (virtual scalar i >= npoints: phi(point))
            // win_stride != 0: window k reads its own pre-shifted copy of the bases (2^(c*k) * P)
            uint32_t pt = i < npoints ? (uint32_t)i : ((uint32_t)(i - npoints) | 0x40000000u);
            pt += k * win_stride;
            entries[base[b] + rk[i]] = pt | (sd < 0 ? 0x80000000u : 0u);
        }
    }
}

// Wide path: R = nwin * ntiles rows share ONE bin space of Bc bins; R is a few hundred, so a
// workgroup of 16 wavefronts takes 64 bins (one per lane, coalesced row reads) and splits the rows
// 16 ways: partial sums per wavefront, exclusive prefix across the wavefronts through LDS, then a
// second pass writes every row's base.
// Rows are `pitch` elements apart, pitch = Bc + 96, so that the rows of one bin are not a power of
// two apart.  (The kernel takes ~80 us for 2 MB whatever its shape -- one thread per bin over all
// rows, 64 bins x 16 row groups, this version, padded or not: it inherits the write-back of the
// 27 MB of ranks the preceding kernel left dirty in the L2s.)
__global__ __launch_bounds__(1024) void k_tile_scan_rows(const uint16_t *__restrict__ tile_hist, uint32_t Bc, uint32_t R, uint32_t pitch,
                                                         uint32_t *__restrict__ tile_base, uint32_t *__restrict__ hist,
                                                         uint32_t *__restrict__ zero1, uint32_t *__restrict__ zeron, uint32_t nzero) {
    __builtin_amdgcn_s_setprio(3);      // the sort runs beside the previous call's tail: do not starve behind its older wavefronts
    if (blockIdx.x == 0) {               // counters of the ordering stage (heavy_count; bin_count | bin_start | bin_cursor)
        if (threadIdx.x == 0) *zero1 = 0;
        for (uint32_t x = threadIdx.x; x < nzero; x += 1024) zeron[x] = 0;
    }
    // 32 bins x 32 row groups per workgroup: lane -> (bin = lane & 31, group = 2 * wavefront + (lane >> 5))
    __shared__ uint32_t part[32][33];
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned bl = lane & 31, grp = 2 * wv + (lane >> 5);
    const uint32_t b = blockIdx.x * 32 + bl;
    const uint32_t per = (R + 31) / 32, r0 = grp * per, r1 = r0 + per < R ? r0 + per : R;
    constexpr uint32_t MAXPER = 16;                  // rows held in registers (R <= 512: n <= 2^20 at 13 windows)
    uint32_t v[MAXPER];
    uint32_t sum = 0;
    const bool in_regs = per <= MAXPER;
    if (in_regs) {
#pragma unroll
        for (uint32_t j = 0; j < MAXPER; j++) {
            const uint32_t r = r0 + j;
            v[j] = (b < Bc && r < r1) ? tile_hist[(size_t)r * pitch + b] : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < MAXPER; j++) sum += v[j];
    } else if (b < Bc) {
        for (uint32_t r = r0; r < r1; r++) sum += tile_hist[(size_t)r * pitch + b];
    }
    part[grp][bl] = sum;
    __syncthreads();
    uint32_t run = 0, tot = 0;
#pragma unroll
    for (unsigned g2 = 0; g2 < 32; g2++) { uint32_t x = part[g2][bl]; if (g2 < grp) run += x; tot += x; }
    if (b < Bc) {
        if (in_regs) {
#pragma unroll
            for (uint32_t j = 0; j < MAXPER; j++) {
                const uint32_t r = r0 + j;
                if (r < r1) { tile_base[(size_t)r * pitch + b] = run; run += v[j]; }
            }
        } else {
            for (uint32_t r = r0; r < r1; r++) {
                const size_t idx = (size_t)r * pitch + b;
                tile_base[idx] = run;
                run += tile_hist[idx];
            }
        }
        if (grp == 0) hist[b] = tot;
    }
}

// ------------------------------------------------------------------------------------
// Wide-window path (resident bases with pre-shifted copies, see "Wide windows" below).
// Every entry is (bin, point reference): bin = segment * B + bucket.  With B = 2^(c-1) up to 2^21
// the bin space can be too large for an LDS histogram; then the sort runs in two passes:
// (A) k_hist_wide / k_tile_scan_rows / k_scatter_wide<1|2> partition all entries by the COARSE bin
// (bin >> 7, or bin >> 6 with 32-bit records; a tile's histogram fits LDS) into 64-bit records
// (fine bits | entry) or 32-bit ones (sign | fine bits | point reference); (B)
// k_fine_sort, one workgroup per coarse bin, counts its 128 (64) fine bins in LDS and places the
// 32-bit entries, writing the per-bin populations and offsets.  With at most 32768 bins (the
// narrow digits used for small inputs and for segmented calls) pass A alone (k_scatter_wide<0>)
// sorts completely.  (SegList, the tile sizes of these passes: msm_plan.h.)
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t segment_of(const SegList &segs, uint32_t i) {
    uint32_t seg = 0;
    for (uint32_t j = 1; j < segs.nseg; j++) if (i >= segs.off[j]) seg = j;
    return seg;
}

// Workgroup -> tile of the two wide-path passes.  Consecutive workgroup ids land on different
// XCDs (round-robin over the 8 dies, each with its own L2); a coarse bin's region of the record
// array is the concatenation of the tiles' runs in tile order, so giving every XCD a CONTIGUOUS
// range of tiles makes the short runs (a few records per tile and bin) of neighbouring tiles meet
// in the same L2 and leave it as whole lines instead of partial-line writes from eight dies.
__device__ __forceinline__ uint32_t xcd_tile(uint32_t bid, uint32_t ntiles) {
    const uint32_t q = ntiles >> 3, r = ntiles & 7u, x = bid & 7u, j = bid >> 3;
    return x * q + (x < r ? x : r) + j;
}

// One workgroup per tile of WIDE_TILE scalars, ALL windows: the histogram of the (coarse) bins of
// the tile's entries in LDS (u16 pairs, one ds_add_u32 per entry) -> the tile's row of tile_hist.
__global__ __launch_bounds__(1024) void k_hist_wide(const Fr *__restrict__ scalars, size_t n, SegList segs, WidePlan pl, uint32_t B,
                                                    uint32_t Bc, CoarseMap cm, uint32_t pitch, uint32_t tile,
                                                    uint16_t *__restrict__ tile_hist) {
    __builtin_amdgcn_s_setprio(3);      // the sort runs beside the previous call's tail: do not starve behind its older wavefronts
    extern __shared__ __attribute__((aligned(16))) uint32_t cnt2[];   // Bc/2 words: two u16 counters each
    for (uint32_t x = threadIdx.x; x < (Bc + 1) / 2; x += blockDim.x) cnt2[x] = 0;
    __syncthreads();
    const uint32_t t = xcd_tile(blockIdx.x, gridDim.x);
    const size_t lo = (size_t)t * tile;
    for (uint32_t il = threadIdx.x; il < tile; il += blockDim.x) {
        const size_t i = lo + il;
        if (i >= n) break;
        const uint32_t seg = segment_of(segs, (uint32_t)i);
        wide_digits(scalars[i], pl, seg * B, [&](unsigned, int32_t sd) {
            if (sd != 0) {
                const uint32_t b = cm.bin((uint32_t)(sd < 0 ? -sd : sd) - 1);
                atomicAdd(&cnt2[b >> 1], 1u << ((b & 1) * 16));                 // ds_add_u32
            }
        });
    }
    __syncthreads();
    uint16_t *th = tile_hist + (size_t)t * pitch;
    const uint16_t *c16 = reinterpret_cast<const uint16_t *>(cnt2);
    for (uint32_t x = threadIdx.x; x < Bc; x += blockDim.x) th[x] = c16[x];
}

// The same tiles again.  Every workgroup first rebuilds the exclusive prefix of the Bc bin
// populations in LDS (a few KB out of L2: cheaper than three scan launches), adds its tile's row
// of tile_base, and then hands out positions with one returning LDS atomic per entry: the order
// of a (tile, bin) run's records is whatever the atomics give -- bucket sums do not depend on it
// -- so no rank array travels between the passes.
// REC 0: the final 32-bit entries (one pass sorts completely); REC 1: 64-bit
// records (7 fine bits << 32 | entry) ordered by coarse bin; REC 2: 32-bit records
// (sign | 6 fine bits | 25-bit point reference) when every point reference fits 25 bits (tables of
// up to 2^20 points): half the bytes through the scatter and the fine sort.
// Entry = index inside the segment + copy * win_stride | sign << 31.
template <int REC>
__global__ __launch_bounds__(1024) void k_scatter_wide(const Fr *__restrict__ scalars, size_t n, SegList segs, WidePlan pl, uint32_t B,
                                                       uint32_t Bc, uint32_t pitch, uint32_t tile, const uint32_t *__restrict__ hist_c,
                                                       uint32_t *__restrict__ offs, const uint32_t *__restrict__ tile_base,
                                                       void *__restrict__ out, uint32_t win_stride) {
    extern __shared__ __attribute__((aligned(16))) uint32_t base[];   // Bc words
    __shared__ uint32_t wsum[16];
    const uint32_t t = xcd_tile(blockIdx.x, gridDim.x);
    const uint32_t *tb = tile_base + (size_t)t * pitch;
    {
        // exclusive scan of hist_c[0 .. Bc): thread x owns `per` consecutive bins
        const uint32_t per = (Bc + 1023) / 1024, b0 = threadIdx.x * per;
        uint32_t sum = 0;
        for (uint32_t q = 0; q < per; q++) if (b0 + q < Bc) sum += hist_c[b0 + q];
        uint32_t incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(incl, d, 64);
            if ((int)(threadIdx.x & 63) >= d) incl += u;
        }
        if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t run = incl - sum;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) run += wsum[w];
        for (uint32_t q = 0; q < per; q++) {
            const uint32_t b = b0 + q;
            if (b < Bc) {
                if (blockIdx.x == 0) offs[b] = run;
                base[b] = run + tb[b];
                run += hist_c[b];
            }
        }
    }
    __syncthreads();
    const size_t lo = (size_t)t * tile;
    for (uint32_t il = threadIdx.x; il < tile; il += 1024) {
        const size_t i = lo + il;
        if (i >= n) break;
        const uint32_t seg = segment_of(segs, (uint32_t)i);
        const uint32_t local = (uint32_t)i - segs.off[seg];
        wide_digits(scalars[i], pl, seg * B, [&](unsigned k, int32_t sd) {
            if (sd != 0) {
                const uint32_t b = (uint32_t)(sd < 0 ? -sd : sd) - 1;
                const uint32_t ent = (local + k * win_stride) | (sd < 0 ? 0x80000000u : 0u);   // window k reads its own copy of the bases
                if (REC == 1) ((uint64_t *)out)[atomicAdd(&base[b >> 7], 1u)] = ((uint64_t)(b & 127u) << 32) | ent;
                else if (REC == 2) ((uint32_t *)out)[atomicAdd(&base[b >> 6], 1u)] = (ent & 0x81ffffffu) | ((b & 63u) << 25);
                else ((uint32_t *)out)[atomicAdd(&base[b], 1u)] = ent;
            }
        });
    }
}

// ------------------------------------------------------------------------------------
// Partitioned two-pass sort (the large single-MSM shape: 2^19 .. 2^21 buckets).  The scatter of
// k_scatter_wide writes 13.6 M four-byte records at n = 2^20 in runs of ~6 (one run per tile and
// coarse bin, 8192 bins): 183 us, against 35 us for the same tiles without the stores
// (k_hist_wide).  Here the first pass cuts the bin space into at most PART_SEGS = 768 segments and
// stages a tile's records in LDS, so a tile leaves ~100-record runs behind (whole cache lines),
// and the second pass -- one workgroup per segment, 2^11 .. 2^13 fine buckets counted in LDS -- does
// its scattered stores inside the segment's own few hundred KB, which stay in one L2.
// A record is 32 bits: low bits of the tile number | fine bucket (10 .. 13 bits) << 16 | window << 12 | sign << 11 |
// index inside the tile; the rest of the tile number is implied by the record's position, because a
// segment's region is the concatenation of the tiles' runs in tile order (tile_base column of the
// segment): the second pass only has to find the block of 64 (.. 8) tiles a position falls into.
// ------------------------------------------------------------------------------------
// counter[idx]++ for every active lane, returning the lane's own old value.  When all active lanes of the
// wavefront name the SAME counter (few distinct scalar digits: every record of a segment in one
// bucket) the wavefront issues one atomic instead of 64 serialised ones.
__device__ __forceinline__ uint32_t lds_inc_rank(uint32_t *counters, uint32_t idx) {
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);
    const uint64_t active = __ballot(1), same = __ballot(idx == first);
    if (same == active) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(active >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)active, 0u));
        uint32_t base = 0;
        if (rank == 0) base = atomicAdd(&counters[first], (uint32_t)__popcll(active));
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)base) + rank;
    }
    return atomicAdd(&counters[idx], 1u);
}
__global__ __launch_bounds__(1024) void k_partition(const Fr *__restrict__ scalars, size_t n, SegList segs, WidePlan pl, uint32_t B, uint32_t Bc,
                                                    CoarseMap cm, uint32_t pitch, const uint16_t *__restrict__ tile_hist,
                                                    const uint32_t *__restrict__ hist_c, uint32_t *__restrict__ offs_c,
                                                    const uint32_t *__restrict__ tile_base, uint32_t *__restrict__ recs) {
    __builtin_amdgcn_s_setprio(3);      // the sort runs beside the previous call's tail: do not starve behind its older wavefronts
    extern __shared__ __attribute__((aligned(16))) uint32_t stage[];      // nwin * PART_TILE records
    __shared__ uint32_t lstart[PART_SEGS + 1], lcur[PART_SEGS], gdst[PART_SEGS], wtot[2][PART_SEGS / 64];
    const uint32_t t = xcd_tile(blockIdx.x, gridDim.x);
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    {
        // threads < Bc (<= 768: twelve wavefronts): exclusive prefix of the segment populations
        // (global: where a segment starts) and of this tile's row (where its run starts in LDS)
        uint32_t gv = 0, lv = 0;
        if (threadIdx.x < Bc) { gv = hist_c[threadIdx.x]; lv = tile_hist[(size_t)t * pitch + threadIdx.x]; }
        uint32_t gi = gv, li = lv;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t a = __shfl_up(gi, d, 64), b = __shfl_up(li, d, 64);
            if ((int)lane >= d) { gi += a; li += b; }
        }
        if (wv < PART_SEGS / 64 && lane == 63) { wtot[0][wv] = gi; wtot[1][wv] = li; }
        __syncthreads();
        if (threadIdx.x < Bc) {
            uint32_t gex = gi - gv, lex = li - lv;
            for (unsigned w = 0; w < wv; w++) { gex += wtot[0][w]; lex += wtot[1][w]; }
            lstart[threadIdx.x] = lex;
            lcur[threadIdx.x] = lex;
            gdst[threadIdx.x] = gex + tile_base[(size_t)t * pitch + threadIdx.x];
            if (blockIdx.x == 0) offs_c[threadIdx.x] = gex;
            if (threadIdx.x == Bc - 1) lstart[Bc] = lex + lv;
        }
    }
    __syncthreads();
    const size_t lo = (size_t)t * PART_TILE;
    const uint32_t fine_bits = cm.sh_hi;                               // (sh_lo <= sh_hi: the fine field is sh_hi bits wide)
    const uint32_t tlow = t & ((1u << (16 - fine_bits)) - 1);          // the record's spare high bits: low bits of the tile number
    for (uint32_t j = 0; j < PART_TILE / 1024; j++) {
        const uint32_t il = threadIdx.x + j * 1024;
        const size_t i = lo + il;
        if (i >= n) break;
        const uint32_t seg = segment_of(segs, (uint32_t)i);
        wide_digits(scalars[i], pl, seg * B, [&](unsigned k, int32_t sd) {
            if (sd != 0) {
                const uint32_t b = (uint32_t)(sd < 0 ? -sd : sd) - 1;
                const uint32_t pos = atomicAdd(&lcur[cm.bin(b)], 1u);
                stage[pos] = (tlow << (16 + fine_bits)) | (cm.fine(b) << 16) | (k << 12) | (sd < 0 ? 0x800u : 0u) | il;
            }
        });
    }
    __syncthreads();
    // half a wavefront moves one run (~50 records): consecutive lanes, consecutive words
    for (uint32_t sg = threadIdx.x >> 5; sg < Bc; sg += 32) {
        const uint32_t a = lstart[sg], e = lstart[sg + 1], g = gdst[sg];
        for (uint32_t x = a + (lane & 31); x < e; x += 32) recs[g + (x - a)] = stage[x];
    }
}

// Second pass: one workgroup per segment.  LDS: cnt[F] | cur[F] | col[T + 1] | stage[PART_STAGE] (F =
// 2^fine_bits fine buckets, T tiles; col[t] = start of tile t's run inside the segment).
__global__ __launch_bounds__(1024) void k_fine_sort_part(const uint32_t *__restrict__ recs, const uint32_t *__restrict__ offs_c,
                                                         const uint32_t *__restrict__ hist_c, const uint32_t *__restrict__ tile_base,
                                                         uint32_t pitch, uint32_t T, CoarseMap cm, SegList segs, uint32_t win_stride, uint32_t stage_cap,
                                                         uint32_t *__restrict__ entries, uint32_t *__restrict__ hist, uint32_t *__restrict__ offs) {
    __builtin_amdgcn_s_setprio(3);      // the sort runs beside the previous call's tail: do not starve behind its older wavefronts
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    __shared__ uint32_t wsum[16];
    const uint32_t sg = blockIdx.x, lo = offs_c[sg], ns = hist_c[sg];
    const uint32_t fine_bits = cm.sh_hi, FM = 1u << fine_bits, fmask = FM - 1, tbits = 16 - fine_bits;   // record layout (tbits low bits of the tile number ride in it)
    const uint32_t F = 1u << cm.bits(sg), bucket0 = cm.first(sg);      // this segment's buckets: [bucket0, bucket0 + F)
    uint32_t *cnt = sm, *cur = sm + FM, *col = sm + 2 * FM, *stage = col + T + 1;
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (uint32_t x = threadIdx.x; x < F; x += 1024) cnt[x] = 0;
    for (uint32_t x = threadIdx.x; x < T; x += 1024) col[x] = tile_base[(size_t)x * pitch + sg];
    if (threadIdx.x == 0) col[T] = ns;
    // exclusive scan of the F counters -> cur[], and this segment's slice of hist / offs
    auto scan_counters = [&]() {
        const uint32_t per = (F + 1023) >> 10, f0 = threadIdx.x * per;
        uint32_t sum = 0;
        for (uint32_t q = 0; q < per; q++) if (f0 + q < F) sum += cnt[f0 + q];
        uint32_t incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(incl, d, 64);
            if ((int)lane >= d) incl += u;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        uint32_t run = incl - sum;
        for (unsigned w = 0; w < wv; w++) run += wsum[w];
        for (uint32_t q = 0; q < per; q++) {
            if (f0 + q >= F) break;
            const uint32_t c = cnt[f0 + q];
            cur[f0 + q] = run;
            hist[(size_t)bucket0 + f0 + q] = c;
            offs[(size_t)bucket0 + f0 + q] = lo + run;
            run += c;
        }
    };
    // record at position p2 of the segment -> entry: it belongs to tile t with col[t] <= p2 < col[t + 1]
    // (runs may be empty): binary search for the last t with col[t] <= p2
    auto entry_of = [&](uint32_t r, uint32_t p2) {
        // block of 2^tbits tiles: the last j with col[j << tbits] <= p2 (few distinct addresses: cheap LDS reads)
        uint32_t a = 0, e = (T + (1u << tbits) - 1) >> tbits;   // invariant: col[a << tbits] <= p2, and p2 < col[e << tbits] (or e is the end)
        while (e - a > 1) {
            const uint32_t m = (a + e) >> 1;
            if (col[m << tbits] <= p2) a = m; else e = m;
        }
        const uint32_t i = ((a << tbits) | (r >> (16 + fine_bits))) * PART_TILE + (r & 0x7ffu);
        const uint32_t local = i - segs.off[segment_of(segs, i)];
        return (local + ((r >> 12) & 15u) * win_stride) | ((r & 0x800u) << 20);
    };
    if (ns <= stage_cap) {
        // The usual case (every segment, with uniformly distributed digits at n <= 2^20): the
        // segment's records are read ONCE, all loads of a thread in flight together, and stay in
        // registers across the count and the placement; the entries are ordered in LDS and leave
        // as one linear copy -- no scattered global stores at all.
        constexpr uint32_t NR = PART_STAGE / 1024;
        uint32_t r[NR];
#pragma unroll
        for (uint32_t u = 0; u < NR; u++) { const uint32_t p2 = threadIdx.x + u * 1024; r[u] = p2 < ns ? recs[lo + p2] : 0u; }
        __syncthreads();
        uint16_t rk[NR];                                     // rank inside the fine bucket, from the counting atomic
#pragma unroll
        for (uint32_t u = 0; u < NR; u++) {
            rk[u] = 0;
            if (threadIdx.x + u * 1024 < ns) rk[u] = (uint16_t)atomicAdd(&cnt[(r[u] >> 16) & fmask], 1u);
        }
        __syncthreads();
        scan_counters();
        __syncthreads();
#pragma unroll
        for (uint32_t u = 0; u < NR; u++) {
            const uint32_t p2 = threadIdx.x + u * 1024;
            if (p2 < ns) stage[cur[(r[u] >> 16) & fmask] + rk[u]] = entry_of(r[u], p2);
        }
        __syncthreads();
        for (uint32_t x = threadIdx.x; x < ns; x += 1024) entries[lo + x] = stage[x];
        return;
    }
    // A larger segment (skewed digits, or n > 2^20) is read twice and places its entries with
    // scattered stores inside its own region.
    __syncthreads();
    constexpr uint32_t UNR = 8;
    for (uint32_t p0 = threadIdx.x; p0 < ns; p0 += 1024 * UNR) {
        uint32_t r[UNR];
#pragma unroll
        for (uint32_t u = 0; u < UNR; u++) { const uint32_t p2 = p0 + u * 1024; r[u] = p2 < ns ? recs[lo + p2] : 0u; }
#pragma unroll
        for (uint32_t u = 0; u < UNR; u++) if (p0 + u * 1024 < ns) (void)lds_inc_rank(cnt, (r[u] >> 16) & fmask);
    }
    __syncthreads();
    scan_counters();
    __syncthreads();
    for (uint32_t p0 = threadIdx.x; p0 < ns; p0 += 1024 * UNR) {
        uint32_t r[UNR];
#pragma unroll
        for (uint32_t u = 0; u < UNR; u++) { const uint32_t p2 = p0 + u * 1024; r[u] = p2 < ns ? recs[lo + p2] : 0u; }
#pragma unroll
        for (uint32_t u = 0; u < UNR; u++) {
            const uint32_t p2 = p0 + u * 1024;
            if (p2 >= ns) break;
            entries[lo + lds_inc_rank(cur, (r[u] >> 16) & fmask)] = entry_of(r[u], p2);
        }
    }
}

template <class Rec>
struct RecOps;
template <>
struct RecOps<uint64_t> {          // 7 fine bits above a 32-bit entry
    static constexpr uint32_t NF = 128;
    static __device__ __forceinline__ uint32_t fine(uint64_t r) { return (uint32_t)(r >> 32); }
    static __device__ __forceinline__ uint32_t entry(uint64_t r) { return (uint32_t)r; }
};
template <>
struct RecOps<uint32_t> {          // sign | 6 fine bits | 25-bit point reference
    static constexpr uint32_t NF = 64;
    static __device__ __forceinline__ uint32_t fine(uint32_t r) { return (r >> 25) & 63u; }
    static __device__ __forceinline__ uint32_t entry(uint32_t r) { return r & 0x81ffffffu; }
};
template <class Rec>
__global__ __launch_bounds__(1024) void k_fine_sort(const Rec *__restrict__ recs, const uint32_t *__restrict__ offs_c,
                                                    const uint32_t *__restrict__ hist_c, uint32_t *__restrict__ entries,
                                                    uint32_t *__restrict__ hist, uint32_t *__restrict__ offs) {
    using O = RecOps<Rec>;
    constexpr uint32_t NF = O::NF;
    __shared__ uint32_t cnt[NF], cur[NF];
    const uint32_t bin = blockIdx.x, lo = offs_c[bin], n = hist_c[bin];
    if (threadIdx.x < NF) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < n; j += 1024) atomicAdd(&cnt[O::fine(recs[lo + j])], 1u);
    __syncthreads();
    if (threadIdx.x < 64) {          // exclusive scan of the NF counters by the first wavefront, NF/64 per lane
        constexpr uint32_t PER = NF / 64;
        uint32_t c[PER], tot = 0;
#pragma unroll
        for (uint32_t q = 0; q < PER; q++) { c[q] = cnt[PER * threadIdx.x + q]; tot += c[q]; }
        uint32_t incl = tot;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            uint32_t t = __shfl_up(incl, d, 64);
            if ((int)threadIdx.x >= d) incl += t;
        }
        uint32_t ex = incl - tot;
#pragma unroll
        for (uint32_t q = 0; q < PER; q++) {
            cur[PER * threadIdx.x + q] = ex;
            hist[(size_t)bin * NF + PER * threadIdx.x + q] = c[q];
            offs[(size_t)bin * NF + PER * threadIdx.x + q] = lo + ex;
            ex += c[q];
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < n; j += 1024) {
        const Rec r = recs[lo + j];
        const uint32_t pos = atomicAdd(&cur[O::fine(r)], 1u);
        entries[lo + pos] = O::entry(r);
    }
}

}  // namespace lsa
