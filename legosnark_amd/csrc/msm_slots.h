// legosnark_amd/csrc/msm_slots.h -- the tail slots of the MSM pipelines (msm_slots.hip): a call's front runs on the
// caller's stream, its tail on the slot's internal stream with the slot's workspace; results are ordered again at
// msm_join() (msm.h).  Internal to the two pipelines (msm.hip: msm_pipeline, msm_compact.hip): the slots' state -- which
// tail is pending, which the caller has not joined, where each writes -- is read and written through these functions only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

namespace lsa {

// a grow-only device buffer (the front and staging workspaces of msm.hip, the workspace of every slot)
struct Workspace {
    void *ptr = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        // LSA_TRACE=2: every growth of a workspace (a hipFree + hipMalloc pair inside somebody's call: 0.5 ms on one box, 10+ on another)
        static const bool noisy = getenv("LSA_TRACE") && getenv("LSA_TRACE")[0] == '2';
        if (noisy) fprintf(stderr, "[lsa]   workspace_grow              %zu -> %zu bytes\n", cap, bytes + bytes / 8);
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr; cap = 0;
        size_t want = bytes + bytes / 8;
        if (hipMalloc(&ptr, want) != hipSuccess) {
            if (hipMalloc(&ptr, bytes) != hipSuccess) { ptr = nullptr; return -1; }
            want = bytes;
        }
        cap = want;
        return 0;
    }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; cap = 0; }
};

constexpr int MSM_NTAIL = 8;      // slots that exist; LSA_TAIL_SLOTS of them are used

struct MsmSlot {
    hipStream_t tail;     // the slot's stream (the caller's stream itself under LSA_NO_OVERLAP=1 and for an inline tail)
    void *ws;             // >= the bytes asked for; owned by this call until its tail has run
    void *aux;            // 4 KiB that only msm_compact_device uses: zero at creation, left zero by every call
    int index;
};

// ---- one call, in this order: [grow_all] begin, <front on st>, handover | continue, <tail on slot->tail>, end | finish
// every slot's workspace to `bytes` at once: a QUEUED large call, before it takes its own slot
int msm_slots_grow_all(size_t bytes);
// picks the next slot, grows its workspace, makes `st` wait for the slot's previous tail
int msm_slot_begin(hipStream_t st, size_t ws_bytes, const void *d_out, MsmSlot *slot, bool inline_tail = false);
// the front (on st) is issued: the slot's stream continues from here ...
int msm_slot_continue(MsmSlot *slot, hipStream_t st);
// ... and (the compact pipeline, whose tail writes d_out itself) behind every earlier tail that writes d_out
int msm_slot_handover(MsmSlot *slot, hipStream_t st);
// the large pipeline's order of results, to be called right before its k_publish: the slot's stream waits for the previous
// slot's tail and for every other pending tail that writes d_out
int msm_slot_publish_order(MsmSlot *slot);
// the tail is issued; `advance`: the next call takes the next slot
int msm_slot_finish(MsmSlot *slot, hipStream_t st, bool advance);
// the same with the compact pipeline's rule: advance unless the tail ran on st with overlap on (a blocking call)
int msm_slot_end(MsmSlot *slot, hipStream_t st);
// Whether this call is queued behind the previous one: the previous slot is another slot, its tail has been issued and the
// caller has not joined it since.  A function of the CALL SEQUENCE alone -- not of whether that tail happens to be running
// still -- so whatever is decided from it is decided the same way whenever the same calls are made.
bool msm_slot_follows_unjoined(const MsmSlot *slot);

// ---- warm-up and shutdown
int msm_slots_ready();                        // events, streams and aux buffers of all slots (first use; lsa_init)
int msm_slots_warm(size_t bytes);             // slot 0's workspace, for a process's first (blocking) calls; -1: no memory
hipStream_t msm_slot_stream(int index);       // null: the slots have no streams (LSA_NO_OVERLAP=1, or not ready)
void msm_slots_release();                     // waits for every tail, then streams, workspaces, events

}  // namespace lsa
