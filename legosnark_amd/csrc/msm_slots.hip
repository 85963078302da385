// legosnark_amd/csrc/msm_slots.hip -- the tail slots of the MSM pipelines: their streams, events and workspaces, and
// the rules by which a front may overwrite a slot, a tail's result is published and a call counts as queued.  Host code
// only; one copy of the bookkeeping for both pipelines (msm.hip: msm_pipeline, msm_compact.hip) through msm_slots.h.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "msm.h"
#include "msm_slots.h"

namespace lsa {

// Pipelining of back-to-back MSMs: the tail (bucket reduction + fold, 0.4-0.8 ms of pure latency
// on a nearly idle chip) runs on an internal stream, so it overlaps the next calls'
// throughput-bound fronts (sort + accumulate).  The buffers a tail reads (buckets, wave
// partials, window sums) belong to its slot and are guarded by events; results become ordered
// on the caller's stream again at msm_join() (every synchronous entry point and
// lsa_stream_join() do that).  LSA_NO_OVERLAP=1 runs everything on the caller's stream.
// NTAIL tail slots, each with its own stream and buffers, used round-robin: the tails of
// consecutive calls are independent, and for small MSMs (CPpoly's ladder) a tail is longer than
// a front, so several run at once.  Each tail computes its result into the slot and publishes
// it to the caller's buffer with a 96/192-byte copy that waits for the previous call's copy:
// results appear in call order even when a later tail finishes first.
static constexpr int NTAIL = MSM_NTAIL;      // slots that exist; tail_slots() of them are used (LSA_TAIL_SLOTS)
struct TailBuf {
    Workspace ws;
    hipEvent_t done = nullptr;     // recorded after the slot's result has been published
    hipEvent_t front_done = nullptr;   // recorded on the caller's stream after the slot's accumulate stage
    hipStream_t stream = nullptr;
    bool pending = false;          // a tail has been issued on this slot
    bool unjoined = false;         // ... and the caller's stream has not waited for it yet
    void *aux = nullptr;           // 4 KiB of msm_compact_device's (zero between calls)
    const void *out = nullptr;     // where the slot's last tail writes its result
};
static TailBuf g_tail[NTAIL];
static unsigned g_slot = 0;
static unsigned tail_slots() {
    static const unsigned v = [] {
        const char *e = getenv("LSA_TAIL_SLOTS");
        const int want = e ? atoi(e) : NTAIL;
        return (unsigned)(want < 2 ? 2 : (want > NTAIL ? NTAIL : want));
    }();
    return v;
}
static int g_overlap = -1;
static TailBuf &slot_buf(const MsmSlot *slot) { return g_tail[slot->index]; }
static TailBuf &slot_prev(const MsmSlot *slot) { return g_tail[(slot->index + tail_slots() - 1) % tail_slots()]; }

// (Measured and rejected: keeping the tail of call i back until call i+1 has issued its sort, so
// that it runs beside the next accumulate kernel instead of the next sort.  The first sort kernels
// are hit hard by a tail that starts beside them -- k_hist_wide 35 -> 110 us, k_tile_scan_rows
// 6 -> 52 us next to k_reduce1_lane's 1024 long single-wavefront workgroups -- but the tail's ~0.12 ms
// of multiplier work has to run somewhere: beside the accumulate kernel it stretches that one from
// 0.97 to 1.14 ms and itself to 1.8 ms, and the step stays at 1.61 ms either way.  Stream
// priorities and CU masks for the tail streams make every kernel slower: 1.95 - 3.7 ms per step.)
int msm_join(hipStream_t st) {
    for (auto &t : g_tail) {
        if (!t.unjoined) continue;
        if (hipStreamWaitEvent(st, t.done, 0) != hipSuccess) {
            set_error("msm_join: stream wait failed");
            return LSA_ERR_HIP;
        }
        t.unjoined = false;
    }
    return LSA_OK;
}
// `other` waits for every tail issued so far; the caller's own stream is left alone
int msm_join_to(hipStream_t other) {
    for (auto &t : g_tail) {
        if (!t.pending || !t.stream) continue;
        if (hipStreamWaitEvent(other, t.done, 0) != hipSuccess) {
            set_error("msm_join_to: stream wait failed");
            return LSA_ERR_HIP;
        }
    }
    return LSA_OK;
}

int msm_slots_ready() {
    if (g_overlap < 0) g_overlap = getenv("LSA_NO_OVERLAP") ? 0 : 1;
    if (!g_tail[0].done) {
        for (auto &t : g_tail) {
            HIPCHK(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&t.front_done, hipEventDisableTiming));
            if (g_overlap) HIPCHK(hipStreamCreateWithFlags(&t.stream, hipStreamNonBlocking));
            HIPCHK(hipMalloc(&t.aux, 4096));
            HIPCHK(hipMemset(t.aux, 0, 4096));
        }
    }
    return LSA_OK;
}
int msm_slots_warm(size_t bytes) { return g_tail[0].ws.ensure(bytes); }
hipStream_t msm_slot_stream(int index) { return g_tail[index].stream; }

void msm_slots_release() {
    for (auto &t : g_tail) {
        if (t.stream) { (void)hipStreamSynchronize(t.stream); (void)hipStreamDestroy(t.stream); t.stream = nullptr; }
        t.ws.release();
        if (t.aux) (void)hipFree(t.aux);
        t.aux = nullptr; t.out = nullptr;
        if (t.done) (void)hipEventDestroy(t.done);
        if (t.front_done) (void)hipEventDestroy(t.front_done);
        t.done = nullptr; t.front_done = nullptr; t.pending = false; t.unjoined = false;
    }
}

static int grow_tail_slot(TailBuf &t, size_t bytes) {
    if (bytes <= t.ws.cap) return LSA_OK;
    if (t.pending) HIPCHK(hipEventSynchronize(t.done));            // about to reallocate: the old tail must be finished
    if (t.ws.ensure(bytes) != 0) { set_error("msm: tail workspace allocation of %zu bytes failed", bytes); return LSA_ERR_NOMEM; }
    return LSA_OK;
}
// msm_slot_begin grows only the slot it hands out: a prover that only ever blocks keeps re-using one slot and grows one slot
// per problem size (when all eight grew together, the first G2 MSM of a process -- the reference's provers issue a handful,
// each blocking -- paid nine hipFree + hipMalloc pairs, 4 ms on a good box and tens of ms on a slow one).
// A QUEUED large call (the integrator's pipelined form) grows every slot at once before it takes its own: its successors
// take the other slots within microseconds, and a new problem size then pays its allocations in one call instead of in eight.
int msm_slots_grow_all(size_t bytes) {
    int rc = msm_slots_ready();
    for (auto &t : g_tail) if (!rc) rc = grow_tail_slot(t, bytes);
    return rc;
}
int msm_slot_begin(hipStream_t st, size_t ws_bytes, const void *d_out, MsmSlot *slot, bool inline_tail) {
    int rc = msm_slots_ready();
    if (rc) return rc;
    TailBuf &tb = g_tail[g_slot];
    rc = grow_tail_slot(tb, ws_bytes);
    if (rc) return rc;
    if (tb.pending) HIPCHK(hipStreamWaitEvent(st, tb.done, 0));        // the front may not overwrite what the slot's last tail still reads
    slot->tail = (g_overlap && !inline_tail) ? tb.stream : st;
    slot->ws = tb.ws.ptr;
    slot->aux = tb.aux;
    slot->index = (int)g_slot;
    tb.out = d_out;
    return LSA_OK;
}
int msm_slot_continue(MsmSlot *slot, hipStream_t st) {
    TailBuf &tb = slot_buf(slot);
    if (slot->tail == st) return LSA_OK;
    HIPCHK(hipEventRecord(tb.front_done, st));
    HIPCHK(hipStreamWaitEvent(slot->tail, tb.front_done, 0));
    return LSA_OK;
}
// Results appear in call order wherever two calls write the same place.  The two pipelines order their tails differently,
// and on purpose:
//   compact: its tail writes d_out itself, so the whole tail waits -- at hand-over -- for every earlier tail with this
//            destination, and for nothing else; a tail that finished long ago costs no wait command.
//   large:   its tail computes into the slot and only k_publish touches d_out, so the waits sit right before k_publish, behind
//            the reduction kernels already enqueued (at hand-over they would serialise the reduction behind the previous
//            tail).  It waits for the previous slot's tail whatever its destination -- results of queued large calls appear
//            in call order -- and for every other pending tail with this destination (the compact pipeline's among them).
int msm_slot_handover(MsmSlot *slot, hipStream_t st) {
    int rc = msm_slot_continue(slot, st);
    if (rc) return rc;
    TailBuf &tb = slot_buf(slot);
    for (auto &o : g_tail) {
        if (&o == &tb || !o.pending || o.out != tb.out) continue;
        // (a tail that finished long ago needs no wait command: a blocking small call otherwise issues up to seven of them)
        if (!o.unjoined && hipEventQuery(o.done) == hipSuccess) { o.pending = false; continue; }
        HIPCHK(hipStreamWaitEvent(slot->tail, o.done, 0));
    }
    return LSA_OK;
}
int msm_slot_publish_order(MsmSlot *slot) {
    TailBuf &tb = slot_buf(slot), &prev = slot_prev(slot);
    if (prev.pending && &prev != &tb) HIPCHK(hipStreamWaitEvent(slot->tail, prev.done, 0));
    for (auto &o : g_tail)
        if (&o != &tb && &o != &prev && o.pending && o.out == tb.out) HIPCHK(hipStreamWaitEvent(slot->tail, o.done, 0));
    return LSA_OK;
}
bool msm_slot_follows_unjoined(const MsmSlot *slot) {
    const TailBuf &prev = slot_prev(slot);
    return prev.pending && prev.unjoined && &prev != &slot_buf(slot);
}
int msm_slot_finish(MsmSlot *slot, hipStream_t st, bool advance) {
    TailBuf &tb = slot_buf(slot);
    HIPCHK(hipEventRecord(tb.done, slot->tail));
    tb.pending = true;
    tb.unjoined = slot->tail != st;
    if (advance) g_slot = (g_slot + 1) % tail_slots();
    return LSA_OK;
}
int msm_slot_end(MsmSlot *slot, hipStream_t st) {
    // (an inline tail = a blocking call: the slot is free again when it returns)
    return msm_slot_finish(slot, st, slot->tail != st || g_overlap == false);
}

}  // namespace lsa
