// How a C-ABI handle (plan, scorer, network, trainer, segments) is born and dies: one upload, one builder, one destroy.  Host code only,
// included by the files that create handles and NOT by common.hpp (whose hash ties PMC files to the kernels' source).
// (templates over a runtime stand-in, HIP-free like StageScopeT: tests/native/handle_life.cpp drives them with a malloc-backed one.
//  Rt: static const char* copy(ctx, dst, src, bytes) and wait(ctx) — null, else why it failed —, static void wait_quietly(ctx), quiesce(ctx))
#pragma once
#include <new>
#include <vector>
#ifndef SSP_HANDLE_NO_HIP
#include "common.hpp"
#endif

namespace ssp {

// The ctx stream as one create sees it.  A copy queued from a host image the create built must not outlive that image: every way out waits
// while `queued` is set — wait() with an error message, the destructor without.
template <class Rt, class Ctx>
struct UploadScopeT {
    Ctx* const ctx;
    const char* const who;  // the entry point, for messages
    UploadScopeT(Ctx* c, const char* w) : ctx(c), who(w) {}
    UploadScopeT(const UploadScopeT&) = delete;
    UploadScopeT& operator=(const UploadScopeT&) = delete;
    ~UploadScopeT() { wait_quietly(); }
    int wait() {
        const char* why = queued ? Rt::wait(ctx) : nullptr;
        queued = false;
        if (why) set_error("%s: upload failed: %s", who, why);
        return why ? SSP_ERR_HIP : SSP_OK;
    }
    void wait_quietly() {
        if (queued) Rt::wait_quietly(ctx);
        queued = false;
    }
    void waited() { queued = false; }  // the caller has waited for the stream by means of its own (StageScopeT has the same)

  private:
    bool queued = false;  // an upload's copy, and whatever the create queued behind it, is on the stream and not waited for
    template <class R, class C, class B, class T>
    friend int upload(UploadScopeT<R, C>&, B&, const T*, size_t);
};

// n elements of `host` into a fresh buffer: allocated, the copy queued on the ctx stream, not waited for.  The first failure's message stays
template <class Rt, class Ctx, class Buf, class T>
int upload(UploadScopeT<Rt, Ctx>& q, Buf& b, const T* host, size_t n) {
    const int rc = b.alloc(n * sizeof(T));
    if (rc != SSP_OK || n == 0) return rc;
    if (const char* why = Rt::copy(q.ctx, b.p, host, n * sizeof(T))) {
        set_error("%s: upload failed: %s", q.who, why);
        return SSP_ERR_HIP;
    }
    q.queued = true;
    return SSP_OK;
}
template <class Rt, class Ctx, class Buf, class T>
int upload(UploadScopeT<Rt, Ctx>& q, Buf& b, const std::vector<T>& v) {  // an empty table: no buffer
    return v.empty() ? SSP_OK : upload(q, b, v.data(), v.size());
}

// A handle under construction: the create fills its fields and queues its uploads, then ends in commit.  Leaving any other way (a failed
// commit, an early return, an exception) waits for what was queued and deletes the handle.  A handle that cannot be allocated is
// std::bad_alloc, like every host image of the create: SSP_CREATE_GUARD turns it into SSP_ERR_NOMEM.
template <class H, class Rt, class Ctx>
struct HandleBuildT : UploadScopeT<Rt, Ctx> {
    HandleBuildT(Ctx* c, const char* w) : UploadScopeT<Rt, Ctx>(c, w), h(new H) { h->ctx = c; }
    ~HandleBuildT() { drop(); }
    H* operator->() const { return h; }
    H* get() const { return h; }
    // rc: what the create has come to.  SSP_OK: the create's one host wait, then the handle is the caller's.  A failure: the handle is
    // dropped here, while the create's host images are still alive
    int commit(int rc, H** out) {
        if (rc == SSP_OK) rc = this->wait();
        if (rc != SSP_OK) {
            drop();
            return rc;
        }
        *out = h;
        h = nullptr;
        return SSP_OK;
    }

  private:
    H* h;
    void drop() {
        this->wait_quietly();
        delete h;
        h = nullptr;
    }
};

// Handles may be destroyed after their ctx (quiesce_ctx, common.hpp)
template <class Rt, class H>
int destroy_handle_on(H* h) {
    if (!h) return SSP_OK;
    Rt::quiesce(h->ctx);
    delete h;
    return SSP_OK;
}

// Behind the body of a create, written as a function-try-block: nothing thrown while host images are built leaves the C ABI
#define SSP_CREATE_GUARD(who)                    \
    catch (...) {                                \
        ::ssp::set_error("%s: host alloc", who); \
        return SSP_ERR_NOMEM;                    \
    }

#ifndef SSP_HANDLE_NO_HIP
struct HipRt {
    static const char* copy(const ssp_ctx* c, void* dst, const void* src, size_t bytes) {
        const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
        return e == hipSuccess ? nullptr : hipGetErrorString(e);
    }
    static const char* wait(const ssp_ctx* c) {
        const hipError_t e = hipStreamSynchronize(c->stream);
        return e == hipSuccess ? nullptr : hipGetErrorString(e);
    }
    static void wait_quietly(const ssp_ctx* c) { (void)sync_quietly(c->stream); }
    static void quiesce(const ssp_ctx* c) { quiesce_ctx(c); }
};
using UploadScope = UploadScopeT<HipRt, ssp_ctx>;
template <class H>
using HandleBuild = HandleBuildT<H, HipRt, ssp_ctx>;
template <class H>
int destroy_handle(H* h) {
    return destroy_handle_on<HipRt>(h);
}
#endif  // SSP_HANDLE_NO_HIP

}  // namespace ssp
