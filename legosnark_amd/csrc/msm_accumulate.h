// legosnark_amd/csrc/msm_accumulate.h -- stages 3b-4 of the MSM pipeline (msm.hip): bucket order and accumulation.
// Buckets ordered by population, one lane (or two) per bucket walking its entry list, heavy buckets split across
// wavefronts.  Device code only, compiled by msm.hip (launch_accumulate).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "curves.h"
#include "fp29x2l.h"
#include "msm_plan.h"
#include "msm_quad.h"

namespace lsa {

// ------------------------------------------------------------------------------------
// kernel 3b: order buckets by population, largest first, so that the 64 lanes of a
// wavefront walk equally long entry lists (bucket sizes are ~Poisson(n/2^(c-1)); unsorted,
// a wavefront waits for its longest lane: ~1.45x the mean at n=2^20, c=16).
// Counting sort on min(count, SIZE_BINS-1) with LDS-aggregated histograms; empty buckets
// get their identity written here, over-threshold ones go to the heavy list.
// ------------------------------------------------------------------------------------
// lanes per bucket in k_accumulate: 2 on the plain path (GLV halves the bucket count; two lanes keep
// >= 2.5 wavefronts per SIMD slot in flight), 1 on the wide path (2^19 .. 2^21 buckets)
// population -> bin: ((cnt - 1) >> bin_shift) + 1 in [1, SIZE_BINS - 1] for cnt in [1, thr]
__device__ __forceinline__ uint32_t size_bin(uint32_t cnt, uint32_t bin_shift) { return ((cnt - 1) >> bin_shift) + 1; }
template <class C>
__global__ __launch_bounds__(256) void k_size_hist(const uint32_t *__restrict__ hist, uint32_t nb, uint32_t thr, uint32_t *__restrict__ bin_count,
                                                   uint32_t group_size, uint32_t bin_shift) {
    // group_size != 0: buckets are ordered group by group (a group = one window's 2^(c-1)
    // buckets, a multiple of this block's 2048), by population inside each group
    bin_count += (group_size ? (blockIdx.x * 2048u) / group_size : 0u) * SIZE_BINS;
    __shared__ uint32_t lcnt[SIZE_BINS];
    for (uint32_t t = threadIdx.x; t < SIZE_BINS; t += 256) lcnt[t] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * 2048 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint32_t g = base + j * 256;
        if (g < nb) { uint32_t cnt = hist[g]; if (cnt > 0 && cnt <= thr) atomicAdd(&lcnt[size_bin(cnt, bin_shift)], 1u); }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < SIZE_BINS; t += 256) if (lcnt[t]) atomicAdd(&bin_count[t], lcnt[t]);
}
// bin_start[g][b] = number of buckets ordered before population b of group g (groups ascending,
// populations descending); the total goes to bin_start[0][0]
__global__ __launch_bounds__(256) void k_size_scan(const uint32_t *__restrict__ bin_count, uint32_t *__restrict__ bin_start, uint32_t ngroups) {
    __shared__ uint32_t lds[4];
    uint32_t carry = 0;
    for (uint32_t gidx = 0; gidx < ngroups; gidx++) {
        const uint32_t *bc = bin_count + gidx * SIZE_BINS;
        uint32_t *bs = bin_start + gidx * SIZE_BINS;
        // lane t owns bins [SIZE_BINS-1-4t-3 .. SIZE_BINS-1-4t], visited from large to small
        uint32_t v[4], s = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int bin = (int)SIZE_BINS - 1 - (int)(threadIdx.x * 4 + j);
            v[j] = (bin >= 1) ? bc[bin] : 0;
            s += v[j];
        }
        uint32_t tot;
        uint32_t run = carry + block_exclusive_scan_256(s, lds, &tot);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int bin = (int)SIZE_BINS - 1 - (int)(threadIdx.x * 4 + j);
            if (bin >= 1) bs[bin] = run;
            run += v[j];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) bin_start[0] = carry;     // number of buckets in the permutation
}
template <class C>
__global__ __launch_bounds__(256) void k_size_scatter(const uint32_t *__restrict__ hist, uint32_t nb, uint32_t thr, const uint32_t *__restrict__ bin_start,
                                                      uint32_t *__restrict__ bin_cursor, uint32_t *__restrict__ perm,
                                                      uint32_t *__restrict__ heavy_list, uint32_t *__restrict__ heavy_count,
                                                      typename C::Acc *__restrict__ buckets, uint32_t group_size, uint32_t bin_shift,
                                                      uint32_t split) {
    const uint32_t goff = (group_size ? (blockIdx.x * 2048u) / group_size : 0u) * SIZE_BINS;
    bin_start += goff;
    bin_cursor += goff;
    __shared__ uint32_t lcnt[SIZE_BINS];
    for (uint32_t t = threadIdx.x; t < SIZE_BINS; t += 256) lcnt[t] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * 2048 + threadIdx.x;
    uint32_t cnt[8], rank[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint32_t g = base + j * 256;
        cnt[j] = 0; rank[j] = 0;
        if (g < nb) {
            cnt[j] = hist[g];
            if (cnt[j] == 0) { for (uint32_t h = 0; h < split; h++) buckets[(size_t)g * split + h] = C::inf(); }
            else if (cnt[j] > thr) heavy_list[atomicAdd(heavy_count, 1u)] = g;
            else rank[j] = atomicAdd(&lcnt[size_bin(cnt[j], bin_shift)], 1u);
        }
    }
    __syncthreads();
    // reserve this block's slice of every bin it touched (reuse lcnt as the slice base)
    for (uint32_t t = threadIdx.x; t < SIZE_BINS; t += 256) {
        uint32_t c = lcnt[t];
        lcnt[t] = c ? atomicAdd(&bin_cursor[t], c) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint32_t g = base + j * 256;
        if (g < nb && cnt[j] > 0 && cnt[j] <= thr) {
            const uint32_t bin = size_bin(cnt[j], bin_shift);
            perm[bin_start[bin] + lcnt[bin] + rank[j]] = g;
        }
    }
}

// ------------------------------------------------------------------------------------
// kernel 4: bucket accumulation (one lane per bucket); heavy buckets deferred.
// C = curve traits (CurveG1: 29-bit limbs, 64-B packed bases; CurveG2: Fq2 on the same limbs, 128-B bases).
// Loads (DESIGN.md "Bucket accumulation: loads"): the loop is rotated by one entry.  Iteration j holds entry word j+1
// already; at its top it issues, unconditionally, the load of entry word j+2 and the gather of base j+1, and it consumes
// that base only in iteration j+1 -- so the gather (an HBM round trip into a table of up to 872 MB) and the dependent
// index load before it have a whole mixed addition (G1: 2 293 instructions in the loop) to arrive in.  A lane past its end
// loads a clamped index, the last entry of its own part: no lane reads outside its list or a base its list does not name.
// (A load under `if (j + 1 < cnt)` made the compiler wait for it inside the branch, ahead of the addition.)
// ------------------------------------------------------------------------------------
// A packed base as 16-byte vectors.  The 64 / 128-B records lie on 64-B boundaries (whole records of a hipMalloc'd
// table); the structs only promise 4, and unpack256 reads overlapping 64-bit pairs of words, from which the compiler
// made overlapping x3 / x4 / x2 / x1 loads.  load_base16 requests the vectors; packed_base, called where the base is
// consumed, hands them over as the packed struct.  Its empty asm uses every vector whole, so the loads stay four (eight)
// global_load_dwordx4 and the wait for them stays at the use.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <class B> struct RawBase {
    static_assert(sizeof(B) % 16 == 0, "packed bases are whole 16-byte vectors");
    u32x4 q[sizeof(B) / 16];
};
template <class B>
__device__ __forceinline__ RawBase<B> load_base16(const B *__restrict__ p) {
    const u32x4 *src = reinterpret_cast<const u32x4 *>(p);
    RawBase<B> r;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(B) / 16); i++) r.q[i] = src[i];
    return r;
}
template <class B>
__device__ __forceinline__ B packed_base(RawBase<B> r) {
    B b;
    uint32_t *dst = reinterpret_cast<uint32_t *>(&b);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(B) / 16); i++) {
        asm("" : "+v"(r.q[i]));
        dst[4 * i] = r.q[i].x; dst[4 * i + 1] = r.q[i].y; dst[4 * i + 2] = r.q[i].z; dst[4 * i + 3] = r.q[i].w;
    }
    return b;
}
// Which curves take the rotated loop.  G2 keeps the loop it had: rotated, k_accumulate_g2_occ2 needs 368 B of scratch per
// lane instead of 316 at its 256 VGPRs and k_accumulate<CurveG2, 2> 256 + 48 registers instead of 256 + 43 (the extra
// entry word and eight 16-byte destinations on top of a register file that is full already).
template <class C> struct RotatedLoads { static constexpr bool value = true; };
template <> struct RotatedLoads<CurveG2> { static constexpr bool value = false; };
template <class C, uint32_t ACC_SPLIT, bool ROTATED = RotatedLoads<C>::value>
__device__ __forceinline__ void accumulate_body(const typename C::Base *__restrict__ bases, const uint32_t *__restrict__ entries,
                                                const uint32_t *__restrict__ offs, const uint32_t *__restrict__ hist,
                                                const uint32_t *__restrict__ perm, const uint32_t *__restrict__ nperm,
                                                typename C::Acc *__restrict__ buckets) {
    // ACC_SPLIT lanes per bucket take interleaved parts of its entry list; the parts are summed
    // when the bucket reduction loads them.
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= *nperm * ACC_SPLIT) return;
    const uint32_t g = perm[t / ACC_SPLIT], part = t % ACC_SPLIT;
    const uint32_t cnt = hist[g];           // 1 .. heavy_threshold
    const uint32_t *e = entries + offs[g];
    // One lane per bucket is the wide path only, whose entries never carry the endo bit: no beta multiplication in that loop.
    constexpr bool ENDO = ACC_SPLIT != 1;
    typename C::Acc acc = C::inf();
    if constexpr (!ROTATED) {
        if (part < cnt) {
            uint32_t v = e[part];
            typename C::Base cur = bases[v & 0x3fffffffu];
            static_assert(!C::HEAD || ROTATED, "the affine + affine head is written for the rotated loop only");
            for (uint32_t j = part; j < cnt; j += ACC_SPLIT) {
                uint32_t vn = v;
                typename C::Base nxt = cur;
                if (j + ACC_SPLIT < cnt) { vn = e[j + ACC_SPLIT]; nxt = bases[vn & 0x3fffffffu]; }
                acc = C::template madd<ENDO>(acc, cur, (v >> 31) != 0, ((v >> 30) & 1) != 0);
                v = vn;
                cur = nxt;
            }
        }
    } else if (part < cnt) {
        const uint32_t last = part + (cnt - 1 - part) / ACC_SPLIT * ACC_SPLIT;      // this lane's last entry
        auto word = [&](uint32_t k) { return e[k < last ? k : last]; };
        auto base = [&](uint32_t w) { return load_base16(bases + (w & 0x3fffffffu)); };
        uint32_t j = part;
        uint32_t v = word(j), vn = word(j + ACC_SPLIT);
        RawBase<typename C::Base> cur;
        if constexpr (C::HEAD) {
            // The first two entries as affine + affine.  A list of one entry, or an infinity base among the two, takes
            // the loop from the start: there an accumulator at infinity is the rare path of the mixed addition.
            // Entry words 0 .. 3 and the bases of entries 0 .. 2 are requested here, unconditionally; the compiler moves the
            // requests that only the head uses (words 2, 3, base 2) into its branch, in front of the head's arithmetic.
            const uint32_t v2 = word(j + 2 * ACC_SPLIT), v3 = word(j + 3 * ACC_SPLIT);
            const RawBase<typename C::Base> r0 = base(v), r1 = base(vn), r2 = base(v2);
            const typename C::Base b0 = packed_base(r0), b1 = packed_base(r1);
            cur = r0;
            if (j + ACC_SPLIT < cnt && C::head_ok(b0, b1)) {
                acc = C::template madd_head<ENDO>(b0, (v >> 31) != 0, ((v >> 30) & 1) != 0, b1, (vn >> 31) != 0, ((vn >> 30) & 1) != 0);
                j += 2 * ACC_SPLIT;
                v = v2;
                vn = v3;
                cur = r2;
            }
        } else {
            cur = base(v);
        }
        for (; j < cnt; j += ACC_SPLIT) {
            const uint32_t vnn = word(j + 2 * ACC_SPLIT);
            const RawBase<typename C::Base> nxt = base(vn);
            acc = C::template madd<ENDO>(acc, packed_base(cur), (v >> 31) != 0, ((v >> 30) & 1) != 0);
            v = vn;
            vn = vnn;
            cur = nxt;
        }
    }
    buckets[(size_t)g * ACC_SPLIT + part] = acc;
}
template <class C, uint32_t ACC_SPLIT>
__global__ __launch_bounds__(256) void k_accumulate(const typename C::Base *__restrict__ bases, const uint32_t *__restrict__ entries,
                                                    const uint32_t *__restrict__ offs, const uint32_t *__restrict__ hist,
                                                    const uint32_t *__restrict__ perm, const uint32_t *__restrict__ nperm,
                                                    typename C::Acc *__restrict__ buckets) {
    accumulate_body<C, ACC_SPLIT>(bases, entries, offs, hist, perm, nperm, buckets);
}
// The G2 kernel capped to the registers of two wavefronts per SIMD: 256 VGPRs + 316 B of scratch per
// lane instead of 256 + 42 AGPRs at one wavefront per SIMD -- 3.35 -> 3.16 ms at n = 2^20 on the
// wide path (the second wavefront hides the gathers the single one stalled on)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_accumulate_g2_occ2(
    const CurveG2::Base *__restrict__ bases, const uint32_t *__restrict__ entries, const uint32_t *__restrict__ offs,
    const uint32_t *__restrict__ hist, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ nperm, CurveG2::Acc *__restrict__ buckets) {
    accumulate_body<CurveG2, 1u>(bases, entries, offs, hist, perm, nperm, buckets);
}

// G2 with a PAIR of lanes per bucket, each lane on one Fq component of every coordinate (fp29x2l.h): the same entry
// walk and the same formulas as above, half the registers per lane.  A lane fetches its own halves of the next base
// (x.c, y.c of its component: 2 x 32 B of the 128-B record, so a pair still reads one contiguous record).
__global__ __launch_bounds__(256) void k_accumulate_g2_pair(const AffPackedG2 *__restrict__ bases, const uint32_t *__restrict__ entries,
                                                            const uint32_t *__restrict__ offs, const uint32_t *__restrict__ hist,
                                                            const uint32_t *__restrict__ perm, const uint32_t *__restrict__ nperm,
                                                            XYZZ29x2 *__restrict__ buckets) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, pr = t >> 1, part = t & 1;
    if (pr >= *nperm) return;                               // (both lanes of a pair leave together)
    const uint32_t g = perm[pr];
    const uint32_t cnt = hist[g];                           // 1 .. heavy_threshold
    const uint32_t *e = entries + offs[g];
    struct Half { uint32_t x[8], y[8]; };
    auto fetch = [&](uint32_t v) {
        const AffPackedG2 &b = bases[v & 0x3fffffffu];
        Half h;
#pragma unroll
        for (int i = 0; i < 8; i++) { h.x[i] = b.w[part][i]; h.y[i] = b.w[2 + part][i]; }
        return h;
    };
    XyzzE<F29h> acc = XyzzE<F29h>::inf();
    uint32_t v = e[0];
    Half cur = fetch(v);
    for (uint32_t j = 0; j < cnt; j++) {
        uint32_t vn = v;
        Half nxt = cur;
        if (j + 1 < cnt) { vn = e[j + 1]; nxt = fetch(vn); }
        AffE<F29h> q = {{F29::unpack256(cur.x)}, {F29::unpack256(cur.y)}};
        if (!q.is_inf()) {
            if (v >> 31) q.y = sub_k<1>(F29h::zero(), q.y);  // p - y per component
            acc = g2_madd(acc, q);
        }
        v = vn;
        cur = nxt;
    }
    F29 *o = reinterpret_cast<F29 *>(&buckets[g]);          // X.c0, X.c1, Y.c0, Y.c1, ZZ.c0, ...
    o[part] = acc.X.v;
    o[2 + part] = acc.Y.v;
    o[4 + part] = acc.ZZ.v;
    o[6 + part] = acc.ZZZ.v;
}

// (G1 capped to 128 VGPRs / four wavefronts per SIMD spills 208 B per lane and measured 2 % slower.)

// Which kernels of the tail run CurveG1's general addition with its products in pairs (curves.h: add<true>): those that keep
// their register limits with it -- three wavefronts per SIMD and no scratch for k_accumulate_heavy, the parent's 231 VGPRs
// for k_reduce1_lane, its 256 + 12 for k_reduce2_lane (profiles/r09_paired_products.txt has the compiled figures).
enum TailKernel { TAIL_HEAVY, TAIL_REDUCE1_LANE, TAIL_REDUCE2_LANE };
template <class C, TailKernel K> struct PairedAdd { static constexpr bool value = false; };
template <> struct PairedAdd<CurveG1, TAIL_HEAVY> { static constexpr bool value = true; };
template <> struct PairedAdd<CurveG1, TAIL_REDUCE1_LANE> { static constexpr bool value = true; };
// k_reduce2_lane compiles to 256 VGPRs + 14 AGPRs with it, against 256 + 12: it stays on xyzz29_add (the two AGPRs cost it
// 10 % once before, DESIGN.md "Bucket addition: instruction count")

// wavefront tree sum: result valid in lane 0
template <class C, bool PAIRED = false>
__device__ __forceinline__ typename C::Acc wave_sum(typename C::Acc v, unsigned lane) {
    for (unsigned d = 32; d >= 1; d >>= 1) {
        typename C::Acc t = shfl_down_acc(v, d);
        if (lane + d < 64) v = C::template add<PAIRED>(v, t);
    }
    return v;
}

// Heavy buckets (population > threshold): k_heavy_plan cuts every heavy bucket into chunks of
// HEAVY_CHUNK entries (exclusive scan of the chunk counts); k_accumulate_heavy gives each
// chunk one wavefront (8 sequential mixed adds per lane, then a shuffle tree);
// k_heavy_finish sums a bucket's chunk partials.  With uniformly random scalars and c | 128
// there are no heavy buckets and all three exit at once.
// Chunk size of this call: 512 entries, doubled (up to 4096) while that still leaves >= 2048 chunks.
// A chunk costs 6 general additions per lane (the shuffle tree) on top of its mixed additions --
// 8 per lane at 512 entries, i.e. 40 % overhead, which is right for a handful of heavy buckets
// (many short chunks = parallelism) and wasteful when most of the input sits in heavy buckets
// (few distinct scalars: 13.6 M heavy entries at n = 2^20, k_accumulate_heavy 2.0 -> 1.3 ms).
// Stored behind the chunk offsets: chunk_off[nh + 1].
__global__ __launch_bounds__(256) void k_heavy_plan(const uint32_t *__restrict__ hist, const uint32_t *__restrict__ heavy_list,
                                                    const uint32_t *__restrict__ heavy_count, uint32_t *__restrict__ chunk_off) {
    __shared__ uint32_t lds[4];
    __shared__ uint32_t s_chunk;
    const uint32_t nh = *heavy_count;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nh; base += 256) {           // total number of heavy entries
        uint32_t h = base + threadIdx.x;
        uint32_t tot;
        (void)block_exclusive_scan_256(h < nh ? hist[heavy_list[h]] : 0, lds, &tot);
        carry += tot;
    }
    if (threadIdx.x == 0) {
        uint32_t chunk = HEAVY_CHUNK;
        while (chunk < 4096u && carry / (2 * chunk) >= 2048u) chunk *= 2;
        s_chunk = chunk;
    }
    __syncthreads();
    const uint32_t chunk = s_chunk;
    carry = 0;
    for (uint32_t base = 0; base < nh; base += 256) {
        uint32_t h = base + threadIdx.x;
        uint32_t v = h < nh ? (hist[heavy_list[h]] + chunk - 1) / chunk : 0;
        uint32_t tot;
        uint32_t ex = block_exclusive_scan_256(v, lds, &tot);
        if (h < nh) chunk_off[h] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) { chunk_off[nh] = carry; chunk_off[nh + 1] = chunk; }      // total number of chunks; chunk size
}

template <class C>
__global__ __launch_bounds__(64) void k_accumulate_heavy(const typename C::Base *__restrict__ bases, const uint32_t *__restrict__ entries,
                                                         const uint32_t *__restrict__ offs, const uint32_t *__restrict__ hist,
                                                         const uint32_t *__restrict__ heavy_list, const uint32_t *__restrict__ heavy_count,
                                                         const uint32_t *__restrict__ chunk_off, typename C::Acc *__restrict__ partials) {
    const uint32_t nh = *heavy_count;
    if (nh == 0) return;
    const uint32_t total = chunk_off[nh], chunk = chunk_off[nh + 1];
    const unsigned lane = threadIdx.x;
    for (uint32_t v = blockIdx.x; v < total; v += gridDim.x) {
        uint32_t lo = 0, hi = nh;                       // largest h with chunk_off[h] <= v
        while (hi - lo > 1) { uint32_t mid = (lo + hi) >> 1; if (chunk_off[mid] <= v) lo = mid; else hi = mid; }
        const uint32_t g = heavy_list[lo];
        const uint32_t cnt = hist[g];
        const uint32_t start = (v - chunk_off[lo]) * chunk;
        const uint32_t end = start + chunk < cnt ? start + chunk : cnt;
        const uint32_t *e = entries + offs[g];
        typename C::Acc acc = C::inf();
        uint32_t j = start + lane;
        if constexpr (!RotatedLoads<C>::value) {
            for (; j < end; j += 64) {
                uint32_t w = e[j];
                acc = C::madd(acc, bases[w & 0x3fffffffu], (w >> 31) != 0, ((w >> 30) & 1) != 0);
            }
        } else if (j < end) {
            // the same rotation as accumulate_body, stride 64 inside the chunk, clamped to this lane's last entry of it
            const uint32_t last = j + (end - 1 - j) / 64 * 64;
            auto word = [&](uint32_t k) { return e[k < last ? k : last]; };
            uint32_t w = word(j), wn = word(j + 64);
            RawBase<typename C::Base> cur = load_base16(bases + (w & 0x3fffffffu));
            for (; j < end; j += 64) {
                const uint32_t wnn = word(j + 128);
                const RawBase<typename C::Base> nxt = load_base16(bases + (wn & 0x3fffffffu));
                acc = C::madd(acc, packed_base(cur), (w >> 31) != 0, ((w >> 30) & 1) != 0);
                w = wn;
                wn = wnn;
                cur = nxt;
            }
        }
        acc = wave_sum<C, PairedAdd<C, TAIL_HEAVY>::value>(acc, lane);
        if (lane == 0) partials[v] = acc;
    }
}

template <class C>
__global__ __launch_bounds__(64) void k_heavy_finish(const uint32_t *__restrict__ heavy_list, const uint32_t *__restrict__ heavy_count,
                                                     const uint32_t *__restrict__ chunk_off, const typename C::Acc *__restrict__ partials,
                                                     typename C::Acc *__restrict__ buckets, uint32_t split) {
    const uint32_t nh = *heavy_count;
    unsigned lane = threadIdx.x;
    for (uint32_t h = blockIdx.x; h < nh; h += gridDim.x) {
        typename C::Acc acc = C::inf();
        for (uint32_t v = chunk_off[h] + lane; v < chunk_off[h + 1]; v += 64) acc = C::add(acc, partials[v]);
        acc = wave_sum<C>(acc, lane);
        if (lane == 0) {
            buckets[(size_t)heavy_list[h] * split] = acc;
            for (uint32_t x = 1; x < split; x++) buckets[(size_t)heavy_list[h] * split + x] = C::inf();
        }
    }
}

}  // namespace lsa
