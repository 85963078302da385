// legosnark_amd/csrc/staging.h -- the host-side frame of the entry points that take either host or device pointers:
// the two kinds of device buffer behind them, the argument checks they share, and the resolution of each operand to the
// pointer the *_device function gets.  Included at the end of capi_internal.h (it needs g, set_error and the copies).
#pragma once
#include <stdint.h>
#include "capi_internal.h"

namespace lsa {

// Grow-only device staging buffer of the host-buffer entry points (the libff shim calls them thousands of times with
// tiny inputs: no hipMalloc / hipFree per call).  Every StageBuf links itself into one list at construction, and
// lsa_shutdown frees them all through stage_release_all(): there is no per-file list to keep complete.
struct StageBuf;
// The head is constant-initialised, so a StageBuf may be constructed in any translation unit at any point of static
// initialisation.  Every StageBuf in the tree is a global or a member of one (g_pending.dev): none is ever destroyed
// before the process ends, so nothing unlinks.
inline StageBuf *g_stage_list = nullptr;
struct StageBuf {
    void *p = nullptr;
    size_t cap = 0;
    StageBuf *const next;
    StageBuf() : next(g_stage_list) { g_stage_list = this; }
    StageBuf(const StageBuf &) = delete;
    StageBuf &operator=(const StageBuf &) = delete;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        static const bool noisy = getenv("LSA_TRACE") && getenv("LSA_TRACE")[0] == '2';
        if (noisy) fprintf(stderr, "[lsa]   stage_grow                  %zu -> %zu bytes\n", cap, bytes < 4096 ? (size_t)4096 : bytes + bytes / 4);
        if (p) { (void)hipStreamSynchronize(g.stream); (void)hipFree(p); }
        p = nullptr; cap = 0;
        size_t want = bytes < 4096 ? 4096 : bytes + bytes / 4;
        if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; return -1; }
        cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
inline void stage_release_all() { for (StageBuf *b = g_stage_list; b; b = b->next) b->release(); }   // lsa_shutdown
extern StageBuf g_stage_gather;    // all-gather landing zone shared by the sharded MSM and pairing paths

// Device memory of one call, freed when the call returns (never null once ensured: an empty operand gets one byte).
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int ensure(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess ? 0 : -1; }
};

// ---- argument checks (the callers format their own messages)
// do the byte ranges [p, p + np) and [q, q + nq) meet?  An empty range meets nothing.
inline bool overlap(const void *p, size_t np, const void *q, size_t nq) {
    if (!np || !nq) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}
inline bool misaligned(const void *p) { return ((uintptr_t)p & 15) != 0; }       // the kernels load 16 bytes at a time
// n * each, and n * m elements of Fr, in bytes: false when the count does not fit size_t
inline bool bytes_of(size_t n, size_t each, size_t *out) { return !__builtin_mul_overflow(n, each, out); }
inline bool fr_bytes_of(size_t n, size_t m, size_t *out) {
    size_t e;
    return !__builtin_mul_overflow(n, m, &e) && !__builtin_mul_overflow(e, sizeof(Fr), out);
}

// The operands of one entry point.  Each call below returns the pointer to hand to the *_device function: the caller's
// own for a device caller, a staged copy for a host caller.  A buffer is a StageBuf or a DevBuf (both: ensure(bytes), p).
// A failure is remembered and turns the later calls into no-ops: the entry point looks at rc() once, before its kernels.
//     OperandFrame f("fr_fold", on_device);
//     const Fr *v = f.in<Fr>(d_v, old, bytes); ...; if (f.rc()) return f.rc();
//     rc = ..._device(v, ...);  if (rc) return rc;
//     return f.download();          // the entry point keeps its own hipStreamSynchronize, where it has one
class OperandFrame {
    struct Pending { void *host; const void *dev; size_t bytes; };
    const char *const name_;
    const bool host_;
    int rc_ = LSA_OK;
    unsigned nout_ = 0;
    Pending out_[3];

    template <class B> bool reserve(B &b, size_t bytes) {
        if (rc_) return false;
        if (b.ensure(bytes)) { set_error("%s: hipMalloc failed", name_); rc_ = LSA_ERR_NOMEM; return false; }
        return true;
    }

  public:
    OperandFrame(const char *name, int on_device) : name_(name), host_(!on_device) {}
    int rc() const { return rc_; }
    // working memory of the kernels: ensured for host and device callers alike
    template <class T = void, class B> T *scratch(B &b, size_t bytes) { return reserve(b, bytes) ? (T *)b.p : nullptr; }
    // read by the kernels.  Host callers: `bytes` are uploaded into b, which holds at least `room` bytes.
    template <class T = void, class B> const T *in(B &b, const void *p, size_t bytes, size_t room = 0) {
        if (!host_) return (const T *)p;
        if (!reserve(b, room > bytes ? room : bytes)) return nullptr;
        rc_ = upload_host(b.p, p, bytes);
        return (const T *)b.p;
    }
    // written by the kernels.  Host callers: download() copies `bytes` from b to p.
    template <class T = void, class B> T *out(B &b, void *p, size_t bytes) {
        if (!host_) return (T *)p;
        return reserve(b, bytes) ? out_in<T>(b.p, p, bytes) : nullptr;
    }
    // a result that lands in an operand staged already (staged = what in() returned).  Device callers: p itself.
    template <class T = void> T *out_in(const void *staged, void *p, size_t bytes) {
        if (!host_) return (T *)p;
        if (!rc_) out_[nout_++] = Pending{p, staged, bytes};
        return (T *)staged;
    }
    // transformed in place
    template <class T = void, class B> T *inout(B &b, void *p, size_t bytes) { return out_in<T>(in<T>(b, p, bytes), p, bytes); }
    // host callers: the results, in the order they were declared, queued behind what is on lsa_stream() (blocking)
    int download() {
        for (unsigned i = 0; i < nout_; i++) LSA_DOWNLOAD(out_[i].host, out_[i].dev, out_[i].bytes);
        return LSA_OK;
    }
};

}  // namespace lsa
