// Host unit test of csrc/msm_plan.h: plan_pipeline, the plan of one call of the general pipeline (msm.hip: msm_pipeline; kernels: msm_sort.h .. msm_reduce.h).
// What keeps the kernels inside their buffers exists nowhere else: the dynamic-LDS requests against the opt-ins of
// msm_func_attrs, the u16 tile counters, the 30/25-bit point references, k_partition's static arrays, the scratch of the
// bit-tree reduction, the CoarseMap's tiling of the buckets, and the two workspace layouts.
//   (1) a sweep over groups, table strides, sizes, segment counts, blocking / reuse_sort and the switches that change the
//       sort: every plan is accepted (no table of the sweep is too large) and satisfies all of the above;
//   (2) the four rejections;
//   (3) eight pinned plans (default switches, queued calls), derived by hand from the expressions of the pipeline before
//       they moved here.
#include <cstdio>
#include <cstring>

#include "msm_plan.h"
using namespace lsa;

static int fails = 0;
static long plans = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 30) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf(" (line %d)\n", __LINE__); } fails++; } } while (0)

static MsmShape shape_of(int group, size_t n, uint32_t nseg, size_t stride, bool blocking = false, bool reuse_sort = false) {
    return MsmShape{group, group == 1 ? (size_t)144 : (size_t)288, group == 1 ? (size_t)96 : (size_t)192, group == 1, n, nseg, stride, blocking, reuse_sort};
}

template <int N>
static void check_layout(const WsLayout<N> &l, const char *what, const char *tag) {
    size_t end = 0;
    for (int i = 0; i < N; i++) {
        CHECK(l.r[i].off % 256 == 0, "%s %s region %d at %zu", tag, what, i, l.r[i].off);
        CHECK(l.r[i].off >= end, "%s %s region %d at %zu overlaps the one before (ends %zu)", tag, what, i, l.r[i].off, end);
        CHECK(l.r[i].off == align_up(end, 256), "%s %s region %d at %zu does not follow the one before (ends %zu)", tag, what, i, l.r[i].off, end);
        CHECK(l[i] == l.r[i].off, "%s %s operator[] %d", tag, what, i);
        end = l.r[i].off + l.r[i].bytes;
    }
    CHECK(l.total == align_up(end, 256), "%s %s total %zu, last region ends %zu", tag, what, l.total, end);
}

static void check_plan(const MsmShape &sh, const PipelinePlan &p, const char *tag) {
    plans++;
    const size_t n = sh.n, A = sh.acc_bytes;
    CHECK(p.n == n && p.nseg == sh.nseg && p.reuse_sort == sh.reuse_sort, "%s shape", tag);
    CHECK(p.wide == (sh.table_stride != 0), "%s wide %d", tag, (int)p.wide);            // (table_use_min = 1 throughout)
    CHECK(p.B == 1u << (p.c - 1) && p.nb == (p.wide ? sh.nseg * p.B : p.nwin * p.B), "%s B %u nb %u", tag, p.B, p.nb);
    CHECK(p.ne == p.nv * p.nwin && p.nv == (p.glv ? 2 * n : n), "%s ne", tag);
    // ---- layouts
    check_layout(p.front, "front", tag);
    check_layout(p.tail, "tail", tag);
    CHECK(p.front.r[F_HIST].bytes >= (size_t)p.nb * 4 + 4, "%s heavy_count word", tag);
    CHECK(p.front.r[F_ENTRIES].bytes >= p.ne * 4 && p.front.r[F_HPART].bytes >= p.max_chunks * A, "%s entries / hpart", tag);
    CHECK(p.front.r[F_THIST].bytes >= p.rows * p.pitch * 2 && p.front.r[F_TBASE].bytes >= p.rows * p.pitch * 4, "%s tile arrays", tag);
    if (!p.wide) CHECK(p.front.r[F_DIGITS].bytes >= p.ne * 4 && p.front.r[F_RANK].bytes >= p.ne * 2, "%s digits / rank", tag);
    if (p.fine) CHECK(p.front.r[F_RECS].bytes >= p.ne * (p.part || p.rec32 ? 4 : 8) && p.front.r[F_CHIST].bytes >= (size_t)p.Bc * 4 && p.front.r[F_COFFS].bytes >= (size_t)p.Bc * 4, "%s records", tag);
    CHECK(p.tail.r[T_BUCKETS].bytes >= (size_t)p.nb * p.split * A && p.tail.r[T_RES].bytes >= sh.nseg * sh.jac_bytes, "%s buckets / res", tag);
    // ---- dynamic LDS against the opt-ins
    if (p.wide) {
        CHECK(p.lds_hist_wide == (size_t)((p.Bc + 1) / 2) * 4 && p.lds_hist_wide <= LDS_MAX_BIN_HALVES, "%s k_hist_wide %zu", tag, p.lds_hist_wide);
        CHECK(p.lds_scatter_wide == (size_t)p.Bc * 4 && p.lds_scatter_wide <= LDS_MAX_BIN_WORDS, "%s k_scatter_wide %zu", tag, p.lds_scatter_wide);
    } else {
        CHECK(p.lds_rank == (size_t)p.B * 2 && p.lds_rank <= LDS_MAX_BIN_HALVES, "%s k_rank %zu", tag, p.lds_rank);
        CHECK(p.lds_scatter == (size_t)p.B * 4 && p.lds_scatter <= LDS_MAX_BIN_WORDS, "%s k_scatter %zu", tag, p.lds_scatter);
    }
    if (p.part) {
        CHECK(p.lds_partition == (size_t)p.nwin * PART_TILE * 4 && p.lds_partition <= LDS_MAX_PARTITION, "%s k_partition %zu", tag, p.lds_partition);
        CHECK(p.fixed_words == 2 * (1u << p.cm.sh_hi) + p.wtiles + 1 && (p.stage_cap == 0 || p.stage_cap == PART_STAGE), "%s fixed_words %u stage_cap %u", tag, p.fixed_words, p.stage_cap);
        CHECK(p.lds_fine_sort_part == (size_t)(p.fixed_words + p.stage_cap) * 4 && p.lds_fine_sort_part <= LDS_MAX_FINE_SORT_PART, "%s k_fine_sort_part %zu", tag, p.lds_fine_sort_part);
    }
    // ---- partitioned sort
    CHECK(!p.part || (p.fine && p.wide), "%s part without fine", tag);
    CHECK(!p.rec32 || p.fine, "%s rec32 without fine", tag);
    if (p.part) {
        const CoarseMap &cm = p.cm;
        CHECK(p.Bc <= PART_SEGS && p.nwin <= 13 && cm.sh_lo <= cm.sh_hi && cm.sh_hi <= 16, "%s Bc %u nwin %u sh %u/%u", tag, p.Bc, p.nwin, cm.sh_lo, cm.sh_hi);
        CHECK(p.wtile == PART_TILE, "%s wtile %u", tag, p.wtile);
        CHECK(cm.first(0) == 0, "%s first(0)", tag);
        uint64_t sum = 0;
        for (uint32_t k = 0; k < p.Bc; k++) {
            if (k + 1 < p.Bc) CHECK(cm.first(k + 1) == cm.first(k) + (1u << cm.bits(k)), "%s bin %u does not end where bin %u starts", tag, k, k + 1);
            sum += (uint64_t)1 << cm.bits(k);
        }
        CHECK(sum == p.B, "%s the bins hold %llu buckets of %u", tag, (unsigned long long)sum, p.B);
        for (uint32_t i = 0; i < 4100; i++) {
            const uint32_t edge[4] = {0, cm.half ? cm.half - 1 : 0, cm.half, p.B - 1};
            const uint32_t b = i < 4 ? edge[i] : (uint32_t)(((uint64_t)i * 2654435761u) % p.B);
            CHECK(cm.bin(b) < p.Bc && cm.first(cm.bin(b)) + cm.fine(b) == b && cm.fine(b) < (1u << cm.bits(cm.bin(b))), "%s bucket %u -> bin %u fine %u", tag, b, cm.bin(b), cm.fine(b));
        }
    } else if (p.fine) {
        CHECK(p.Bc == p.nb >> p.fine_bits && p.cm.half == 0 && p.cm.sh_hi == p.fine_bits && p.fine_bits == (p.rec32 ? 6u : 7u), "%s plain coarse bins", tag);
        CHECK(((p.Bc << p.fine_bits) == p.nb), "%s the coarse bins do not tile %u buckets", tag, p.nb);
    } else {
        CHECK(p.Bc == (p.wide ? p.nb : p.B), "%s Bc %u", tag, p.Bc);
    }
    // ---- u16 tile counters, the scan
    if (p.wide) {
        CHECK((uint64_t)p.wtile * p.nwin <= 65535, "%s a tile holds %u x %u entries", tag, p.wtile, p.nwin);
        CHECK((uint64_t)p.wtiles * p.wtile >= n && p.rows == p.wtiles && p.pitch == p.Bc + 96, "%s tiles", tag);
    } else {
        CHECK(SORT_TILE <= 65535, "SORT_TILE");
        CHECK((uint64_t)p.ntiles * SORT_TILE >= p.nv && p.rows == (size_t)p.nwin * p.ntiles && p.pitch == p.Bc, "%s tiles", tag);
    }
    CHECK(p.nscan == (p.wide ? p.Bc : p.nb) && p.scan_blocks == (p.nscan + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK && p.scan_blocks <= 1024, "%s scan_blocks %u", tag, p.scan_blocks);
    CHECK(p.front.r[F_BSUM].bytes >= (size_t)p.scan_blocks * 4, "%s bsum", tag);
    // ---- entry widths
    if (p.wide) {
        const uint64_t refs = (uint64_t)sh.table_stride * table_grid(sh.table_stride).ncopies;
        CHECK(refs < (1u << 30) && p.nb <= (1u << 21), "%s %llu point references, %u buckets", tag, (unsigned long long)refs, p.nb);
        if (p.rec32) CHECK(refs < (1u << 25) && (p.nb >> 6) <= 32768, "%s rec32 with %llu point references", tag, (unsigned long long)refs);
        CHECK(p.win_stride == sh.table_stride * p.pl.copy_step, "%s win_stride", tag);
    }
    // ---- heavy buckets
    CHECK(p.heavy_threshold >= 1 && ((p.heavy_threshold - 1) >> p.bin_shift) + 1 <= SIZE_BINS - 1, "%s thr %u shift %u", tag, p.heavy_threshold, p.bin_shift);
    CHECK(p.max_heavy <= p.nb && p.max_chunks >= p.ne / HEAVY_CHUNK + p.max_heavy, "%s max_heavy %u max_chunks %zu", tag, p.max_heavy, p.max_chunks);
    CHECK(p.front.r[F_HEAVY].bytes >= (size_t)p.max_heavy * 4 && p.front.r[F_CHOFF].bytes >= ((size_t)p.max_heavy + 2) * 4, "%s heavy lists", tag);
    // ---- reduction levels: level 1 -> T_WAVE, then 16-ary levels ping-pong T_WIN, T_WAVE, ... down to one pair per window
    CHECK(p.L == 1u << p.logL && p.T * p.L == p.B && p.kw == (p.wide ? sh.nseg : p.nwin), "%s L %u T %u kw %u", tag, p.L, p.T, p.kw);
    CHECK(p.wpw == (p.big ? p.T : (p.T + 15) / 16), "%s wpw %u", tag, p.wpw);
    CHECK((size_t)p.kw * p.wpw * 2 * A <= p.tail.r[T_WAVE].bytes, "%s level 1 leaves %u x %u pairs", tag, p.kw, p.wpw);
    {
        uint32_t m = p.wpw;
        int out = T_WIN, levels = 0;
        do {
            const uint32_t m_in = m, m_out = (m + 15) / 16;
            CHECK((size_t)p.kw * m_out * 2 * A <= p.tail.r[out].bytes, "%s a level of %u x %u pairs into region %d", tag, p.kw, m_out, out);
            m = m_out;
            out = out == T_WIN ? T_WAVE : T_WIN;
            levels++;
            if (p.bits_tail && levels == 1) {
                CHECK(m > 1 && m <= 8192, "%s bit trees over %u pairs", tag, m);
                uint32_t nbits = 0;
                while ((1u << nbits) < m) nbits++;
                const uint32_t G = (m + 511) / 512;
                CHECK((size_t)(nbits + 1) * G + 16 <= 2 * (size_t)m_in, "%s bit-tree scratch (%u + 1) * %u + 16 in a level of %u pairs", tag, nbits, G, m_in);
                CHECK(((size_t)(nbits + 1) * G + 16) * A <= p.tail.r[out].bytes, "%s bit-tree scratch in region %d", tag, out);
                break;          // (the trees end in the point)
            }
        } while (m > 1 && levels < 10);
        CHECK(p.bits_tail || m == 1, "%s levels end at %u", tag, m);
    }
    if (p.bits_tail) CHECK(sh.blocking && p.big && p.kw == 1, "%s bits_tail", tag);
    if (p.lane_l1_shape) CHECK(!sh.blocking && !sh.reuse_sort && p.big && p.kw == 1 && p.wpw >= 16384, "%s lane_l1", tag);
    CHECK(!p.g2_pair || (sh.group == 2 && p.split == 1), "%s g2_pair", tag);
}

static void sweep() {
    const size_t strides[] = {0, 1, 3000, 70000, ((size_t)1 << 19) + 64, (size_t)1 << 20, ((size_t)6 << 20) - 1, (size_t)6 << 20, (size_t)1 << 24};
    const size_t ns[] = {1, 2, 255, 256, 257, 4096, 4097, 16384, 16385, 65535, 65536, 65537, (size_t)1 << 17, ((size_t)1 << 17) + 1, (size_t)1 << 20,
                         (size_t)1 << 25, ((size_t)1 << 25) + 1, ((size_t)1 << 27) - 1};
    const uint32_t nsegs[] = {1, 2, 3, 64};
    MsmSwitches sws[4];
    sws[1].no_rec32 = true;
    sws[2].no_part = true;
    sws[3].wide_split = 2;
    for (int group = 1; group <= 2; group++)
        for (size_t stride : strides)
            for (size_t n : ns)
                for (uint32_t nseg : nsegs) {
                    if (nseg > 1 && stride == 0) continue;
                    if (stride && n > nseg * stride) continue;
                    for (int flags = 0; flags < 4; flags++)
                        for (int s = 0; s < 4; s++) {
                            char tag[160];
                            snprintf(tag, sizeof tag, "[G%d n=%zu nseg=%u stride=%zu blocking=%d reuse=%d sw=%d]", group, n, nseg, stride, flags & 1, flags >> 1, s);
                            const MsmShape sh = shape_of(group, n, nseg, stride, flags & 1, flags >> 1);
                            const PipelinePlan p = plan_pipeline(sh, sws[s]);
                            const bool too_large = stride && (uint64_t)stride * table_grid(stride).ncopies >= (1u << 30);
                            CHECK(p.status == (too_large ? PLAN_TABLE_TOO_LARGE : PLAN_OK), "%s status %d", tag, (int)p.status);
                            if (p.status != PLAN_OK) continue;
                            check_plan(sh, p, tag);
                            if (s == 1) CHECK(!p.rec32, "%s rec32 with no_rec32", tag);
                            if (s == 2) CHECK(!p.part, "%s part with no_part", tag);
                            CHECK(p.split == (p.wide ? (s == 3 ? 2u : 1u) : 2u), "%s split %u", tag, p.split);
                        }
                }
}

static void rejections() {
    const MsmSwitches sw;
    CHECK(plan_pipeline(shape_of(1, (size_t)1 << 27, 1, 0), sw).status == PLAN_N_TOO_LARGE, "n = 2^27");
    CHECK(plan_pipeline(shape_of(2, (size_t)1 << 27, 1, (size_t)1 << 20), sw).status == PLAN_N_TOO_LARGE, "n = 2^27 over a table");
    CHECK(plan_pipeline(shape_of(1, 100, 2, 0), sw).status == PLAN_SEGMENTS_NEED_COPIES, "segments without copies");
    MsmSwitches thr;
    thr.table_use_min = 1000;            // a threshold keeps single calls off the copies, never segmented ones
    CHECK(plan_pipeline(shape_of(1, 100, 2, 5000), thr).status == PLAN_OK && plan_pipeline(shape_of(1, 100, 2, 5000), thr).wide, "segments below the threshold");
    CHECK(!plan_pipeline(shape_of(1, 100, 1, 5000), thr).wide && plan_pipeline(shape_of(1, 1000, 1, 5000), thr).wide, "table_use_min");
    CHECK(plan_pipeline(shape_of(1, 1000, 1, ((size_t)1 << 30) / 24), sw).status == PLAN_OK, "just below 2^30 point references");
    CHECK(plan_pipeline(shape_of(1, 1000, 1, ((size_t)1 << 30) / 24 + 1), sw).status == PLAN_TABLE_TOO_LARGE, "just above 2^30 point references");
    // (callers stop at MSM_MAX_SEGMENTS = 64 segments of 2^9 or 2^10 buckets; the pipeline's own limit is 2^21 bins)
    const PipelinePlan many = plan_pipeline(shape_of(1, 8192, 8192, (size_t)1 << 20), sw);
    CHECK(many.status == PLAN_BIN_SPACE && many.B == 512 && many.nseg == 8192, "8192 segments of 512 buckets");
    CHECK(plan_pipeline(shape_of(1, 8192, 4096, (size_t)1 << 20), sw).status == PLAN_OK, "4096 segments of 512 buckets");
}

struct Pin {
    int group; size_t n; uint32_t nseg; size_t stride;
    unsigned c, nwin; uint32_t B, nb;
    bool fine, rec32, part; uint32_t Bc;
    uint32_t L, T, wpw, kw, split, thr;
    uint32_t wtile, wtiles, pitch;         // wtile = 0: plain path, not looked at
    size_t front, tail;
};
static void pinned() {
    const Pin pins[] = {
        {1, (size_t)1 << 20, 1, (size_t)1 << 20, 20, 13, 1u << 19, 1u << 19, true, true, true, 768, 8, 65536, 65536, 1, 1, 106, 2048, 512, 864, 141398272, 95551744},
        {2, (size_t)1 << 20, 1, (size_t)1 << 20, 20, 13, 1u << 19, 1u << 19, true, true, true, 768, 8, 65536, 65536, 1, 1, 106, 2048, 512, 864, 163750400, 191103232},
        {1, (size_t)1 << 24, 1, (size_t)1 << 24, 22, 12, 1u << 21, 1u << 21, true, false, true, 768, 32, 65536, 65536, 1, 1, 370, 2048, 8192, 864, 1817595648, 322044160},
        {1, 70000, 1, 70000, 20, 13, 1u << 19, 1u << 19, true, true, true, 768, 8, 65536, 65536, 1, 1, 64, 2048, 35, 864, 16190464, 95551744},
        {1, 40000, 4, 20000, 10, 26, 512, 2048, false, false, false, 2048, 1, 512, 32, 4, 1, 4, 2048, 20, 2144, 5059072, 334592},
        {1, 4097, 1, 0, 9, 15, 256, 3840, false, false, false, 256, 1, 256, 16, 15, 2, 98, 0, 0, 256, 1537536, 1179648},
        {2, 4097, 1, 0, 8, 32, 128, 4096, false, false, false, 128, 1, 128, 8, 32, 2, 98, 0, 0, 128, 1868544, 2525440},
        {1, (size_t)1 << 20, 1, 0, 16, 8, 32768, 262144, false, false, false, 32768, 8, 4096, 256, 8, 2, 162, 0, 0, 32768, 292055552, 76124416},
    };
    const MsmSwitches sw;
    int row = 0;
    for (const Pin &e : pins) {
        row++;
        const PipelinePlan p = plan_pipeline(shape_of(e.group, e.n, e.nseg, e.stride), sw);
        CHECK(p.status == PLAN_OK, "pinned row %d status %d", row, (int)p.status);
        if (p.status != PLAN_OK) continue;
        CHECK(p.c == e.c && p.nwin == e.nwin && p.B == e.B && p.nb == e.nb, "pinned row %d: c %u nwin %u B %u nb %u", row, p.c, p.nwin, p.B, p.nb);
        CHECK(p.fine == e.fine && p.rec32 == e.rec32 && p.part == e.part && p.Bc == e.Bc, "pinned row %d: fine %d rec32 %d part %d Bc %u", row, (int)p.fine, (int)p.rec32, (int)p.part, p.Bc);
        CHECK(p.L == e.L && p.T == e.T && p.wpw == e.wpw && p.kw == e.kw && p.split == e.split, "pinned row %d: L %u T %u wpw %u kw %u split %u", row, p.L, p.T, p.wpw, p.kw, p.split);
        CHECK(p.heavy_threshold == e.thr, "pinned row %d: thr %u", row, p.heavy_threshold);
        if (e.wtile) CHECK(p.wtile == e.wtile && p.wtiles == e.wtiles, "pinned row %d: wtile %u wtiles %u", row, p.wtile, p.wtiles);
        CHECK(p.pitch == e.pitch, "pinned row %d: pitch %u", row, p.pitch);
        CHECK(p.front.total == e.front && p.tail.total == e.tail, "pinned row %d: front %zu tail %zu", row, p.front.total, p.tail.total);
    }
    // the CoarseMaps of rows 1 and 3
    const PipelinePlan a = plan_pipeline(shape_of(1, (size_t)1 << 20, 1, (size_t)1 << 20), sw);
    CHECK(a.cm.half == 1u << 18 && a.cm.sh_lo == 9 && a.cm.sh_hi == 10 && a.cm.nlo == 512, "CoarseMap at 2^19 buckets: half %u sh %u/%u nlo %u", a.cm.half, a.cm.sh_lo, a.cm.sh_hi, a.cm.nlo);
    CHECK(a.lane_l1_shape && !a.bits_tail && a.stage_cap == PART_STAGE, "2^20 queued: lane_l1 %d bits %d stage_cap %u", (int)a.lane_l1_shape, (int)a.bits_tail, a.stage_cap);
    const PipelinePlan ab = plan_pipeline(shape_of(1, (size_t)1 << 20, 1, (size_t)1 << 20, true), sw);
    CHECK(!ab.lane_l1_shape && ab.bits_tail, "2^20 blocking: lane_l1 %d bits %d", (int)ab.lane_l1_shape, (int)ab.bits_tail);
    CHECK(!plan_pipeline(shape_of(2, (size_t)1 << 20, 1, (size_t)1 << 20), sw).lane_l1_shape, "G2 lane_l1");
}

// The (shape, switches) pairs of tests/test_switch_paths_gpu.py.  Each variant there sets a switch in order to run a kernel the
// default plan of that shape does not; which kernel runs is a flag of the plan, so the plan must carry the flag the GPU test
// means -- with the switch, and not without it.  Handles of n points (table_stride = n), one segment.
static void switch_paths() {
    const size_t N16 = (size_t)1 << 16;
    const MsmSwitches def;
    const size_t wide_ns[2] = {N16, N16 + 1};
    char tag[96];
    // M1: LSA_NO_PART + LSA_NO_REC32 -> k_scatter_wide<1> / k_fine_sort<u64> (64-bit records, 7 fine bits), as n > 2^25 does by default
    MsmSwitches m1;
    m1.no_part = true;
    m1.no_rec32 = true;
    for (size_t n : wide_ns) {
        snprintf(tag, sizeof tag, "[M1 n=%zu]", n);
        const MsmShape sh = shape_of(1, n, 1, n, true);
        const PipelinePlan p = plan_pipeline(sh, m1), d = plan_pipeline(sh, def);
        CHECK(p.status == PLAN_OK && d.status == PLAN_OK, "%s status", tag);
        CHECK(p.wide && p.big && p.fine && !p.part && !p.rec32 && p.fine_bits == WIDE_FINE_BITS, "%s wide %d big %d fine %d part %d rec32 %d", tag, (int)p.wide, (int)p.big, (int)p.fine, (int)p.part, (int)p.rec32);
        CHECK(p.front.r[F_RECS].bytes >= p.ne * 8, "%s 64-bit records in %zu bytes", tag, p.front.r[F_RECS].bytes);
        CHECK(d.fine && d.part && d.rec32, "%s default: part %d rec32 %d", tag, (int)d.part, (int)d.rec32);
        check_plan(sh, p, tag);
    }
    {
        // the plan n > 2^25 takes without any switch is the same one
        const MsmShape sh = shape_of(1, ((size_t)1 << 25) + 1, 1, ((size_t)1 << 25) + 1);
        const PipelinePlan p = plan_pipeline(sh, def);
        CHECK(p.status == PLAN_OK && p.wide && p.big && p.fine && !p.part && !p.rec32, "[n=2^25+1 default] fine %d part %d rec32 %d", (int)p.fine, (int)p.part, (int)p.rec32);
    }
    // M3: LSA_NO_REDUCE_BITS -> blocking calls reduce through the 16-ary levels
    {
        MsmSwitches m3;
        m3.no_reduce_bits = true;
        const MsmShape sh = shape_of(1, N16, 1, N16, true);
        const PipelinePlan p = plan_pipeline(sh, m3), d = plan_pipeline(sh, def);
        CHECK(d.status == PLAN_OK && d.bits_tail, "[M3] default bits_tail %d", (int)d.bits_tail);
        CHECK(p.status == PLAN_OK && !p.bits_tail && p.big && p.wpw == d.wpw, "[M3] bits_tail %d", (int)p.bits_tail);
        check_plan(sh, p, "[M3]");
    }
    // M4: LSA_NO_LANE_L1 -> queued G1 calls keep the quad kernel in the first 16-ary level
    {
        MsmSwitches m4;
        m4.no_lane_l1 = true;
        const MsmShape sh = shape_of(1, N16, 1, N16, false);
        const PipelinePlan p = plan_pipeline(sh, m4), d = plan_pipeline(sh, def);
        CHECK(d.status == PLAN_OK && d.lane_l1_shape, "[M4] default lane_l1 %d", (int)d.lane_l1_shape);
        CHECK(p.status == PLAN_OK && !p.lane_l1_shape, "[M4] lane_l1 %d", (int)p.lane_l1_shape);
        check_plan(sh, p, "[M4]");
    }
    // M5: LSA_G2_LANE_L1=1 -> k_reduce2_lane<CurveG2> for queued G2 calls
    {
        MsmSwitches m5;
        m5.g2_lane_l1 = true;
        const MsmShape sh = shape_of(2, N16, 1, N16, false);
        const PipelinePlan p = plan_pipeline(sh, m5), d = plan_pipeline(sh, def);
        CHECK(d.status == PLAN_OK && !d.lane_l1_shape, "[M5] default lane_l1 %d", (int)d.lane_l1_shape);
        CHECK(p.status == PLAN_OK && p.lane_l1_shape && p.big, "[M5] lane_l1 %d", (int)p.lane_l1_shape);
        CHECK(!plan_pipeline(shape_of(2, N16, 1, N16, true), m5).lane_l1_shape, "[M5] blocking lane_l1");
        check_plan(sh, p, "[M5]");
    }
    // M6a: LSA_WIDE_BIG_MIN=1048576 -> 26 narrow digits at 2^16 pairs and beyond: 512 buckets, every one of them heavy
    MsmSwitches m6a;
    m6a.wide_big_min = 1048576;
    for (size_t n : wide_ns) {
        snprintf(tag, sizeof tag, "[M6a n=%zu]", n);
        const MsmShape sh = shape_of(1, n, 1, n, true);
        const PipelinePlan p = plan_pipeline(sh, m6a), d = plan_pipeline(sh, def);
        CHECK(d.status == PLAN_OK && d.big && d.nwin == 13, "%s default big %d nwin %u", tag, (int)d.big, d.nwin);
        CHECK(p.status == PLAN_OK && p.wide && !p.big && p.nwin == 26 && p.heavy_threshold == 4, "%s big %d nwin %u thr %u", tag, (int)p.big, p.nwin, p.heavy_threshold);
        CHECK(p.ne / p.nb > p.heavy_threshold, "%s %zu entries over %u buckets", tag, p.ne, p.nb);
        check_plan(sh, p, tag);
    }
    // M6b: LSA_WIDE_BIG_MIN=4096 -> 13 wide digits over 2^19 buckets at 4099 pairs
    {
        MsmSwitches m6b;
        m6b.wide_big_min = 4096;
        const MsmShape sh = shape_of(1, 4099, 1, 4099, true);
        const PipelinePlan p = plan_pipeline(sh, m6b), d = plan_pipeline(sh, def);
        CHECK(d.status == PLAN_OK && !d.big && d.nwin == 26, "[M6b] default big %d nwin %u", (int)d.big, d.nwin);
        CHECK(p.status == PLAN_OK && p.wide && p.big && p.nwin == 13 && p.nb == 1u << 19 && p.ne < p.nb / 8, "[M6b] big %d nwin %u nb %u", (int)p.big, p.nwin, p.nb);
        check_plan(sh, p, "[M6b]");
    }
}

int main() {
    sweep();
    rejections();
    pinned();
    switch_paths();
    printf("%ld plans checked\n", plans);
    if (fails) { printf("%d FAILURES\n", fails); return 1; }
    printf("PASS\n");
    return 0;
}
