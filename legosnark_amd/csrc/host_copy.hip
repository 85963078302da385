// legosnark_amd/csrc/host_copy.hip -- pageable host memory <-> device on lsa_stream(): the pinned-slot copier behind
// upload_host / download_host (capi_internal.h says when a copy goes through the slots and why).  No kernels.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "capi_internal.h"

// ---------------------------------------------------------------- staged host <-> device copies (capi_internal.h)
namespace lsa {
namespace {
class HostCopier {
    size_t SLOT = (size_t)2 << 20;                    // LSA_H2D_SLOT_KB (experiments)
    static constexpr unsigned MAX_WORKERS = 12, SLOTS_PER_WORKER = 2;
    struct Slot { void *p = nullptr; hipEvent_t ev = nullptr; bool pending = false; };
    struct Worker { Slot slot[SLOTS_PER_WORKER]; unsigned turn = 0; };
    Worker w_[MAX_WORKERS];
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, cv_done_;
    uint64_t gen_ = 0;
    unsigned active_ = 0;
    bool stop_ = false, broken_ = false;
    // the job
    char *dev_ = nullptr, *host_ = nullptr;
    bool down_ = false;
    size_t bytes_ = 0, nchunks_ = 0, chunk_ = 0;
    std::atomic<size_t> next_{0};
    std::atomic<int> err_{0};

    void *arena_ = nullptr;                           // every slot, one pinned allocation
    unsigned nworkers_ = 0;
    // Uploads of two slots and more leave lsa_stream(): worker i issues its copies on copy stream i % ncs_, so that
    // several copy engines run at once (one stream = one engine at a time: 23 GB/s measured, against 40-50 for the
    // runtime's own large copy) and a kernel the caller queues on lsa_stream() between two uploads (the normalisation
    // of the previous wave of a CRS vector) does not hold the next copies back.  run() orders the streams: they wait
    // for what lsa_stream() holds at the start (`order_after`), lsa_stream() waits for them at the end.
    static constexpr unsigned MAX_STREAMS = 4;
    hipStream_t cs_[MAX_STREAMS] = {};
    hipEvent_t ev_begin_ = nullptr, ev_done_[MAX_STREAMS] = {};
    unsigned ncs_ = 0;
    bool on_cs_ = false;
    bool slot_ready(Slot &s) {
        if (!s.p || !s.ev) return false;
        if (s.pending) { if (hipEventSynchronize(s.ev) != hipSuccess) return false; s.pending = false; }
        return true;
    }
    // threads, the pinned slots and their events, all at once (lsa_init: not inside somebody's first timed call --
    // sixteen separate pinned allocations took 8 ms of the unchanged hadamard's Lipmaa prover)
    bool prepare_locked() {
        if (arena_) return true;
        const unsigned hw = std::thread::hardware_concurrency();
        const char *e = getenv("LSA_H2D_THREADS");
        // one thread moves ~10 GB/s through a pinned slot; the link takes ~55: ten on a host with cores to spare
        unsigned want = e ? (unsigned)atoi(e) : (hw >= 32 ? 10 : (hw > 8 ? 6 : (hw > 2 ? hw / 2 : 1)));
        if (want < 1) want = 1;
        if (want > MAX_WORKERS) want = MAX_WORKERS;
        if (const char *sk = getenv("LSA_H2D_SLOT_KB")) { const size_t kb = (size_t)atol(sk); if (kb >= 64 && kb <= 16384) SLOT = kb << 10; }
        if (hipHostMalloc(&arena_, (size_t)want * SLOTS_PER_WORKER * SLOT, hipHostMallocDefault) != hipSuccess) { arena_ = nullptr; return false; }
        for (unsigned i = 0; i < want; i++)
            for (unsigned k = 0; k < SLOTS_PER_WORKER; k++) {
                Slot &s = w_[i].slot[k];
                s.p = (char *)arena_ + ((size_t)i * SLOTS_PER_WORKER + k) * SLOT;
                s.pending = false;
                if (hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) != hipSuccess) { s.ev = nullptr; return false; }
            }
        nworkers_ = want;
        const char *se = getenv("LSA_H2D_STREAMS");
        // ONE copy stream by default: enough to run the copies beside the kernels of lsa_stream() (96 MiB of first-sight
        // bases: 3.3 ms, 4.3 on lsa_stream() itself); with two to four, 40 % of the first calls of fresh processes took
        // another 7 ms (more copy engines and queues brought up lazily, in whichever call first overlaps enough copies)
        unsigned ns = se ? (unsigned)atoi(se) : 1u;
        if (ns > MAX_STREAMS) ns = MAX_STREAMS;
        if (ns > want) ns = want;
        ncs_ = 0;
        if (ns && hipEventCreateWithFlags(&ev_begin_, hipEventDisableTiming) == hipSuccess) {
            for (unsigned k = 0; k < ns; k++) {
                if (hipStreamCreateWithFlags(&cs_[k], hipStreamNonBlocking) != hipSuccess) { cs_[k] = nullptr; break; }
                if (hipEventCreateWithFlags(&ev_done_[k], hipEventDisableTiming) != hipSuccess) { (void)hipStreamDestroy(cs_[k]); cs_[k] = nullptr; ev_done_[k] = nullptr; break; }
                ncs_ = k + 1;
            }
        }
        (void)hipGetLastError();
        for (unsigned i = 1; i < want; i++) th_.emplace_back([this, i] { loop(i); });
        return true;
    }
    void work(unsigned id) {
        if (id) (void)hipSetDevice(g.device);
        Worker &w = w_[id];
        for (;;) {
            const size_t c = next_.fetch_add(1);
            if (c >= nchunks_) break;
            const size_t lo = c * chunk_, len = bytes_ - lo < chunk_ ? bytes_ - lo : chunk_;
            Slot &s = w.slot[w.turn++ % SLOTS_PER_WORKER];
            if (!slot_ready(s)) { err_ = 1; continue; }
            if (down_) {
                if (hipMemcpyAsync(s.p, dev_ + lo, len, hipMemcpyDeviceToHost, g.stream) != hipSuccess || hipEventRecord(s.ev, g.stream) != hipSuccess ||
                    hipEventSynchronize(s.ev) != hipSuccess) { err_ = 1; continue; }
                memcpy(host_ + lo, s.p, len);
            } else {
                hipStream_t st = on_cs_ ? cs_[id % ncs_] : g.stream;
                memcpy(s.p, host_ + lo, len);
                if (hipMemcpyAsync(dev_ + lo, s.p, len, hipMemcpyHostToDevice, st) != hipSuccess || hipEventRecord(s.ev, st) != hipSuccess) { err_ = 1; continue; }
                s.pending = true;
            }
        }
    }
    void loop(unsigned id) {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
            }
            work(id);
            {
                std::lock_guard<std::mutex> lk(m_);
                if (--active_ == 0) cv_done_.notify_all();
            }
        }
    }

  public:
    ~HostCopier() { stop_threads(); }
    // 0: done (up: every copy is on the stream; down: the bytes are in host memory), 1: not taken, < 0: LSA error
    int run(void *dev, void *host, size_t bytes, bool down, bool order_after = true) {
        if (broken_) return 1;
        dev_ = (char *)dev; host_ = (char *)host; bytes_ = bytes; down_ = down;
        // whole slots for large copies; a copy of 0.5 .. 4 MiB (the points of a 2^12-pair product: 0.4 + 0.8 MiB) is cut into
        // up to four pieces of >= 256 KiB so that its memcpy is shared too (one thread moves ~10 GB/s: 80 us per 0.8 MiB)
        chunk_ = SLOT;
        if (bytes >= ((size_t)512 << 10) && bytes < 2 * SLOT) {
            const size_t pieces = bytes / ((size_t)256 << 10) < 4 ? bytes / ((size_t)256 << 10) : 4;
            chunk_ = ((bytes + pieces - 1) / pieces + 4095) & ~(size_t)4095;
            if (chunk_ > SLOT) chunk_ = SLOT;
        }
        nchunks_ = (bytes + chunk_ - 1) / chunk_;
        next_.store(0);
        err_.store(0);
        bool alone = nchunks_ < 2;                        // one piece: not worth waking anybody
        {
            std::lock_guard<std::mutex> lk(m_);
            if (!prepare_locked()) { broken_ = true; return 1; }
            if (th_.empty()) alone = true;
            on_cs_ = !down && !alone && ncs_ > 0;
            if (on_cs_ && order_after) {
                bool ok = hipEventRecord(ev_begin_, g.stream) == hipSuccess;
                for (unsigned k = 0; k < ncs_ && ok; k++) ok = hipStreamWaitEvent(cs_[k], ev_begin_, 0) == hipSuccess;
                if (!ok) { (void)hipGetLastError(); on_cs_ = false; }
            }
            if (!alone) {
                active_ = (unsigned)th_.size();
                gen_++;
            }
        }
        if (!alone) cv_.notify_all();
        work(0);
        if (!alone) {
            std::unique_lock<std::mutex> lk(m_);
            cv_done_.wait(lk, [&] { return active_ == 0; });
        }
        if (on_cs_) {
            for (unsigned k = 0; k < ncs_; k++)
                if (hipEventRecord(ev_done_[k], cs_[k]) != hipSuccess || hipStreamWaitEvent(g.stream, ev_done_[k], 0) != hipSuccess) err_ = 1;
            on_cs_ = false;
        }
        if (err_.load()) {
            broken_ = true;
            set_error("a staged host <-> device copy failed (%s)", hipGetErrorString(hipGetLastError()));
            return LSA_ERR_HIP;
        }
        return 0;
    }
    void stop_threads() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) if (t.joinable()) t.join();
        th_.clear();
        std::lock_guard<std::mutex> lk(m_);
        stop_ = false;
        gen_ = 0;
        active_ = 0;
    }
    void prepare() {
        std::lock_guard<std::mutex> lk(m_);
        if (!prepare_locked()) broken_ = true;
    }
    // the first pinned transfer on a stream sets up that stream's copy-engine queue (~7 ms each, measured inside the
    // first CRS upload of a process): paid in lsa_init, per copy stream and per size class a slot can carry
    // (the runtime adds copy engines when copies overlap, and each new engine is another such set-up: the warm-up keeps
    // every copy stream busy at the same time, ordered against lsa_stream() exactly as run() orders them)
    void warm_streams() {
        std::lock_guard<std::mutex> lk(m_);
        if (!arena_ || !ncs_) return;
        void *d = nullptr;
        if (hipMalloc(&d, (size_t)ncs_ * SLOT) != hipSuccess) { (void)hipGetLastError(); return; }
        (void)hipEventRecord(ev_begin_, g.stream);
        for (unsigned k = 0; k < ncs_; k++) (void)hipStreamWaitEvent(cs_[k], ev_begin_, 0);
        for (int rep = 0; rep < 12; rep++)
            for (unsigned k = 0; k < ncs_; k++)
                (void)hipMemcpyAsync((char *)d + (size_t)k * SLOT, (char *)arena_ + (size_t)k * SLOT, rep & 1 ? SLOT / 4 : SLOT, hipMemcpyHostToDevice, cs_[k]);
        for (unsigned k = 0; k < ncs_; k++) { (void)hipEventRecord(ev_done_[k], cs_[k]); (void)hipStreamWaitEvent(g.stream, ev_done_[k], 0); }
        (void)hipStreamSynchronize(g.stream);
        for (unsigned k = 0; k < ncs_; k++) (void)hipStreamSynchronize(cs_[k]);
        (void)hipFree(d);
        (void)hipGetLastError();
    }
    void release() {
        stop_threads();
        for (auto &w : w_)
            for (auto &s : w.slot) {
                if (s.ev) { if (s.pending) (void)hipEventSynchronize(s.ev); (void)hipEventDestroy(s.ev); }
                s = Slot();
            }
        for (unsigned k = 0; k < MAX_STREAMS; k++) {
            if (cs_[k]) { (void)hipStreamSynchronize(cs_[k]); (void)hipStreamDestroy(cs_[k]); }
            if (ev_done_[k]) (void)hipEventDestroy(ev_done_[k]);
            cs_[k] = nullptr; ev_done_[k] = nullptr;
        }
        if (ev_begin_) (void)hipEventDestroy(ev_begin_);
        ev_begin_ = nullptr;
        ncs_ = 0;
        if (arena_) (void)hipHostFree(arena_);
        arena_ = nullptr;
        nworkers_ = 0;
        broken_ = false;
    }
};
HostCopier g_copier;
// 0 auto, 1 direct, 2 staged at every size
int copy_mode() {
    static const int mode = [] {
        const char *e = getenv("LSA_H2D");
        return !e ? 0 : (strcmp(e, "direct") == 0 ? 1 : (strcmp(e, "staged") == 0 ? 2 : 0));
    }();
    return mode;
}
constexpr size_t STAGE_FROM = (size_t)32 << 10;       // below: the runtime copies through its own staging buffer
// from here on the runtime's own path (pin the caller's pages, one DMA) wins: a staged copy is sixteen and more
// commands and six threads of memcpy -- 32 MiB: 0.3-0.4 ms later on the device than the direct copy, and the
// fingerprint threads get less of the host.  (Buffers this large are the ones whose release stalls the GPU when the
// runtime has pinned them: see capi_internal.h; the shim keeps them on the heap, other callers keep them alive.)
constexpr size_t STAGE_BELOW = (size_t)16 << 20;
static bool staged(size_t bytes) { return copy_mode() != 1 && ((bytes >= STAGE_FROM && bytes < STAGE_BELOW) || copy_mode() == 2); }
// A host range the library has NOT been handed before (the reference's provers: one multiExpMA per key vector and
// process, src/gadgets/subspace.cc:78-85; fresh std::vectors of scalars per call) is the other case: the runtime's direct
// path first has to pin its pages, 4 KiB at a time unless the kernel backs the range with huge pages -- 5-20 ms per
// 96 MiB depending on the box, where the slots move it at the link rate whatever the pages are.  The last few large
// ranges are remembered; a range goes through the slots until it has been seen LSA_H2D_DIRECT_AFTER (default 2) times,
// from then on the runtime's registration is worth its price (bench loops, provers that keep their vectors).
struct SeenRange { const void *p = nullptr; size_t bytes = 0; unsigned count = 0; uint64_t tick = 0; };
static SeenRange g_seen[16];
static uint64_t g_seen_tick = 0;
static unsigned direct_after() {
    static const unsigned v = [] { const char *e = getenv("LSA_H2D_DIRECT_AFTER"); return e ? (unsigned)atoi(e) : 2u; }();
    return v;
}
static bool large_copy_staged(const void *h, size_t bytes) {
    if (copy_mode() == 1) return false;
    if (copy_mode() == 2) return true;
    SeenRange *slot = &g_seen[0];
    for (auto &r : g_seen) {
        if (r.p == h && r.bytes == bytes) { r.tick = ++g_seen_tick; return r.count++ < direct_after(); }
        if (r.tick < slot->tick) slot = &r;
    }
    *slot = SeenRange{h, bytes, 1, ++g_seen_tick};
    return direct_after() > 0;
}
}  // namespace

bool upload_takes_slots(const void *h_src, size_t bytes) {
    return staged(bytes) || (bytes >= STAGE_BELOW && large_copy_staged(h_src, bytes));
}
int upload_host_as(void *d_dst, const void *h_src, size_t bytes, bool slots, bool order_after) {
    if (bytes == 0) return LSA_OK;
    if (slots) {
        const int rc = g_copier.run(d_dst, const_cast<void *>(h_src), bytes, false, order_after);
        if (rc <= 0) return rc;
    }
    HIPCHK(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, g.stream));
    return LSA_OK;
}
int upload_host(void *d_dst, const void *h_src, size_t bytes) {
    return upload_host_as(d_dst, h_src, bytes, bytes != 0 && upload_takes_slots(h_src, bytes), true);
}
int download_host(void *h_dst, const void *d_src, size_t bytes) {
    if (bytes == 0) return LSA_OK;
    // (large destinations the library has not seen before go through the slots as well: the runtime would pin the caller's
    // pages and keep them registered, and a caller that frees such a buffer afterwards -- a Python array, a temporary
    // std::vector outside the shim's allocator settings -- stalls its next GPU submission by 12-25 ms when the pages are
    // unmapped: measured as a 15.5 ms bubble in front of the first MSM after a 96-MiB download, 26 ms after 192 MiB)
    if (staged(bytes) || (bytes >= STAGE_BELOW && large_copy_staged(h_dst, bytes))) {
        const int rc = g_copier.run(const_cast<void *>(d_src), h_dst, bytes, true);
        if (rc <= 0) return rc;
    }
    HIPCHK(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return LSA_OK;
}
void upload_release() { g_copier.release(); }
void upload_prepare() {
    if (copy_mode() == 1) return;
    g_copier.prepare();
    // the runtime sets up a copy engine's queue at the first pinned transfer of a direction and size class (measured:
    // 8.4 ms inside the first 128-KiB download of a process that had only done larger ones; none with
    // HSA_ENABLE_SDMA=0): pay that here for every size a slot can carry, not inside a caller's first NTT
    void *d = nullptr;
    if (hipMalloc(&d, (size_t)4 << 20) != hipSuccess) { (void)hipGetLastError(); return; }
    g_copier.warm_streams();
    std::vector<char> h((size_t)4 << 20, 0);
    for (size_t bytes = STAGE_FROM; bytes <= ((size_t)4 << 20); bytes <<= 1) {
        if (upload_host(d, h.data(), bytes) != LSA_OK) break;
        (void)hipStreamSynchronize(g.stream);                       // (a download on an idle stream takes another path)
        if (download_host(h.data(), d, bytes) != LSA_OK) break;
    }
    (void)hipStreamSynchronize(g.stream);
    (void)hipFree(d);
}
}  // namespace lsa
