// Host-side staging of SSP_HOST calls (included twice by common.hpp: part 1 before ssp_ctx — the pool it holds —, part 2 behind it — the
// per-call scope and its per-operand primitive).  No device code here: the file is deliberately NOT part of bench.py's kernel-source hash.
#if SSP_STAGING_PART == 1
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>
namespace ssp {
// Staging buffers of SSP_HOST calls, kept by the ctx between calls: the reference's callers loop over utterances in Python, and a
// hipMalloc + hipFree pair per staged operand costs up to 0.7 ms each once the allocator has no small block at hand (GMM_UBM.delta
// took 1.4 ms a call in such a state, 0.06 ms with the buffers kept).  A slot is taken for the life of one Staged; all work of a
// ctx is ordered on its one stream, so the next call may overwrite a slot without a host wait.  Buffers above KEEP_MAX are not kept.
// (a template over the buffer type so that tests/native/stagepool_threads.cpp can drive the slot logic from several threads under
//  ThreadSanitizer with a malloc-backed buffer, without a HIP runtime)
template <class Buf>
struct StagePoolT {
    static constexpr int SLOTS = 12;
    static constexpr size_t KEEP_MAX = (size_t)64 << 20;
    Buf slot[SLOTS];
    bool busy[SLOTS] = {};
    std::mutex mu;  // (a ctx is not thread-safe, but before the pool two host-pointer calls on one ctx never shared a staging buffer: keep it so)
    void give_back(int i) {
        std::lock_guard<std::mutex> g(mu);
        busy[i] = false;
    }
    // a free slot of at least n bytes: the smallest that fits, else the smallest free one grown to n; -1 = none free or n too large
    int take(size_t n, int* rc) {
        *rc = SSP_OK;
        if (n > KEEP_MAX) return -1;
        std::lock_guard<std::mutex> g(mu);
        int fit = -1, spare = -1;
        for (int i = 0; i < SLOTS; ++i) {
            if (busy[i]) continue;
            if (slot[i].p && slot[i].bytes >= n && (fit < 0 || slot[i].bytes < slot[fit].bytes)) fit = i;
            if (spare < 0 || slot[i].bytes < slot[spare].bytes) spare = i;
        }
        if (fit < 0) {
            if (spare < 0) return -1;
            size_t want = n < 4096 ? 4096 : n + n / 4;  // headroom: utterance lengths vary from call to call
            if (want > KEEP_MAX) want = KEEP_MAX;
            *rc = slot[spare].alloc(want);
            if (*rc != SSP_OK) return -1;
            fit = spare;
        }
        busy[fit] = true;
        return fit;
    }
};

// Host copies of the list-fed entry points (ssp_mfcc_run_list, ssp_gmm_score_list): the caller's per-utterance arrays are gathered into
// pinned slots, and features leave pinned slots for the caller's array, in pieces of about 1 MiB that a pool of worker threads runs.
// Workers only copy and convert: every stream and event call stays on the calling thread.
enum { COPY_BYTES = 0, COPY_F32_TO_F64 = 1, COPY_F64_TO_F32 = 2 };
struct CopyPiece {
    const void* src;
    void* dst;
    size_t n;   // bytes (COPY_BYTES) or elements
    int kind;
};
// appends the pieces of one span: n bytes (COPY_BYTES) or n elements
static inline void add_pieces(std::vector<CopyPiece>& v, const void* src, void* dst, size_t n, int kind, size_t piece_bytes = (size_t)1 << 20) {
    const size_t ss = kind == COPY_F64_TO_F32 ? 8 : kind == COPY_F32_TO_F64 ? 4 : 1, ds = kind == COPY_F32_TO_F64 ? 8 : kind == COPY_F64_TO_F32 ? 4 : 1;
    const size_t per = std::max<size_t>(1, piece_bytes / std::max(ss, ds));
    for (size_t i = 0; i < n; i += per)
        v.push_back({static_cast<const char*>(src) + i * ss, static_cast<char*>(dst) + i * ds, std::min(per, n - i), kind});
}
static inline void run_piece(const CopyPiece& p) {
    if (p.kind == COPY_BYTES) {
        memcpy(p.dst, p.src, p.n);
    } else if (p.kind == COPY_F32_TO_F64) {   // exact
        const float* s = static_cast<const float*>(p.src);
        double* d = static_cast<double*>(p.dst);
        for (size_t i = 0; i < p.n; ++i) d[i] = (double)s[i];
    } else {                                  // round to nearest even, as numpy's astype(float32)
        const double* s = static_cast<const double*>(p.src);
        float* d = static_cast<float*>(p.dst);
        for (size_t i = 0; i < p.n; ++i) d[i] = (float)s[i];
    }
}
struct CopyJob {
    const CopyPiece* piece;
    void operator()(size_t i) const { run_piece(piece[i]); }
};
// Worker threads that run the jobs of ONE caller at a time: run(n, job) calls job(0 .. n-1) once each, spread over the workers and the
// calling thread, and returns when all have returned.  Started lazily (resize); the destructor joins the workers.
// (a template over the job type, HIP-free, so that tests/native/gather_pool_threads.cpp can run it under ThreadSanitizer)
template <class Job>
struct WorkPoolT {
    WorkPoolT() = default;
    WorkPoolT(const WorkPoolT&) = delete;
    WorkPoolT& operator=(const WorkPoolT&) = delete;
    ~WorkPoolT() { stop(); }
    int threads() const { return (int)th.size() + 1; }   // (the caller included)
    // nthreads copying threads, the caller included; a worker that cannot be started leaves the pool smaller
    void resize(int nthreads) {
        if ((int)th.size() == nthreads - 1) return;
        stop();
        for (int i = 1; i < nthreads; ++i) {
            try {
                th.emplace_back([this] { loop(); });
            } catch (...) {
                break;
            }
        }
    }
    void run(size_t count, const Job& j) {
        if (count == 0) return;
        if (th.empty() || count == 1) {
            for (size_t i = 0; i < count; ++i) j(i);
            return;
        }
        {
            std::lock_guard<std::mutex> g(mu);
            job = &j;
            n = count;
            next.store(0);
            ++gen;
        }
        wake.notify_all();
        for (size_t i; (i = next.fetch_add(1)) < count;) j(i);
        std::unique_lock<std::mutex> lk(mu);
        idle.wait(lk, [&] { return inside == 0; });
        job = nullptr;   // (a worker that wakes only now finds nothing to do)
        n = 0;
    }

  private:
    std::mutex mu;
    std::condition_variable wake, idle;
    std::vector<std::thread> th;
    const Job* job = nullptr;
    size_t n = 0;
    std::atomic<size_t> next{0};
    uint64_t gen = 0;
    int inside = 0;   // workers between taking a job and giving it back
    bool quit = false;
    void stop() {
        {
            std::lock_guard<std::mutex> g(mu);
            quit = true;
        }
        wake.notify_all();
        for (std::thread& t : th) t.join();
        th.clear();
        quit = false;
    }
    void loop() {
        std::unique_lock<std::mutex> lk(mu);
        uint64_t seen = gen;
        for (;;) {
            wake.wait(lk, [&] { return quit || gen != seen; });
            if (quit) return;
            seen = gen;
            const Job* j = job;
            const size_t cnt = n;
            if (!j) continue;
            ++inside;
            lk.unlock();
            for (size_t i; (i = next.fetch_add(1)) < cnt;) (*j)(i);
            lk.lock();
            if (--inside == 0) idle.notify_all();
        }
    }
};
using CopyPool = WorkPoolT<CopyJob>;
static inline void run_pieces(CopyPool& pool, const std::vector<CopyPiece>& v) { pool.run(v.size(), CopyJob{v.data()}); }
// copying threads of the list-fed calls, the caller included: min(8, hardware threads), SSP_HOST_THREADS overrides (1 .. 16)
static inline int host_threads() {
    int n = (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    if (const char* e = getenv("SSP_HOST_THREADS")) n = atoi(e);
    return std::min(16, std::max(1, n));
}

#ifndef SSP_STAGING_NO_HIP
using StagePool = StagePoolT<DevBuf>;
// page-locked host buffer (hipHostMalloc): copies from / to it run asynchronously at the full PCIe rate
struct PinBuf {
    void* p = nullptr;
    size_t bytes = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
    int alloc(size_t n) {
        release();
        if (n == 0) n = 16;
        SSP_HIP(hipHostMalloc(&p, n, hipHostMallocDefault));
        bytes = n;
        return SSP_OK;
    }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};
// Ring of device slots that large SSP_HOST calls stream through, on two copy streams beside the ctx stream: run_sliced (mfcc_plan.hip)
// copies slice i + 1 in while slice i computes and slice i - 1's features go back; feed_rows (below) copies rows in ahead of the scorers.
// The ctx makes it on first use and keeps it (slots grow-only: pipe_reserve); ssp_ctx_destroy drains and frees it.
struct HostPipe {
    static constexpr int RING = 3;
    hipStream_t h2d = nullptr, d2h = nullptr;
    DevBuf in[RING], raw[RING], out[RING];          // fp32 samples | int16 samples as copied in (widened into `in`) | features
    // list-fed calls: pinned copies of the slices' samples and features (the slot's last copy is waited for before the host writes it
    // again: in_ready / out_done), and whole-batch pinned bounces of the one-piece paths; grow-only like the device slots
    PinBuf pin_in[RING], pin_out[RING], bounce_in, bounce_out;
    CopyPool pool;   // their copying threads (started on first use: pipe_pool)
    hipEvent_t in_ready[RING] = {}, computed[RING] = {}, out_done[RING] = {};
    // a call's prologue: the copy streams start behind whatever the ctx stream holds (the slots' last readers of an earlier call included)
    int start(hipStream_t cs) {
        SSP_HIP(hipEventRecord(computed[0], cs));
        SSP_HIP(hipStreamWaitEvent(h2d, computed[0], 0));
        SSP_HIP(hipStreamWaitEvent(d2h, computed[0], 0));
        return SSP_OK;
    }
    ~HostPipe() {
        for (int i = 0; i < RING; ++i) {
            if (in_ready[i]) (void)hipEventDestroy(in_ready[i]);
            if (computed[i]) (void)hipEventDestroy(computed[i]);
            if (out_done[i]) (void)hipEventDestroy(out_done[i]);
        }
        if (h2d) (void)hipStreamDestroy(h2d);
        if (d2h) (void)hipStreamDestroy(d2h);
    }
};
#endif  // SSP_STAGING_NO_HIP
}  // namespace ssp
#elif SSP_STAGING_PART == 2
#include <algorithm>
#include <cstdlib>
#include <memory>
namespace ssp {
// The staged operands of ONE host-or-device call (or of one slab of it).  in / out hand back the pointer the kernels use — the argument
// itself with SSP_DEVICE or for a null pointer, else a staged device copy — and an output's host pointer and byte count are kept, once,
// for the copy back.  The first failure sticks: later in / out calls stage nothing and return null, so ONE SSP_TRY(status()) behind the
// operand block checks them all.  copy_back queues the device-to-host copies in the order of the out calls and does not wait; finish
// adds the call's one wait on SSP_HOST.  A call that leaves with copies queued and not waited for (an error return) waits in the
// destructor, before the slots go back: no copy outlives the call on the caller's arrays.  No heap: CAP operands, as the pool has slots.
// (a template over the operand type, HIP-free like StagePoolT: tests/native/stage_scope.cpp drives it with a malloc-backed stand-in.
//  Op: in / out / back as Staged below, static int wait(ctx) — sets the error message — and static void wait_quietly(ctx))
template <class Op, class Ctx>
struct StageScopeT {
    static constexpr int CAP = 12;  // ssp_vbhmm_resegment's need (three inputs, eight outputs), the largest; = StagePoolT::SLOTS
    StageScopeT(const Ctx* c, int w) : ctx(c), where(w) {}
    ~StageScopeT() {
        if (in_flight) Op::wait_quietly(ctx);
    }
    int status() const { return rc; }
    template <class T>
    const T* in(const T* host, size_t bytes) {
        return static_cast<const T*>(stage(host, bytes, where, true, false));
    }
    template <class T>
    const T* in_host(const T* host, size_t bytes) {  // a host array in the device form too (tables): such a call ends in finish(true)
        return static_cast<const T*>(stage(host, bytes, SSP_HOST, true, false));
    }
    template <class T>
    T* out(T* host, size_t bytes, bool preload = false) {  // preload: the staged copy starts out with the caller's bytes
        return static_cast<T*>(stage(host, bytes, where, preload, true));
    }
    int copy_back() {
        for (int i = 0; i < n && rc == SSP_OK; ++i) {
            if (!back_to[i]) continue;
            in_flight = true;
            rc = op[i].back(ctx, back_to[i], back_bytes[i], SSP_HOST);
            back_to[i] = nullptr;  // (each output goes back once, whichever exit asks)
        }
        return rc;
    }
    int finish(bool device_too = false) {
        if (copy_back() != SSP_OK || (where != SSP_HOST && !device_too)) return rc;
        in_flight = false;
        return rc = Op::wait(ctx);
    }
    void waited() { in_flight = false; }  // the caller has waited for the stream by means of its own since copy_back

  private:
    const Ctx* ctx;
    const int where;
    Op op[CAP];
    void* back_to[CAP];  // the host array of a staged output, else null
    size_t back_bytes[CAP];
    int n = 0, rc = SSP_OK;
    bool in_flight = false;  // device-to-host copies queued and not waited for
    void* stage(const void* host, size_t bytes, int w, bool load, bool is_out) {
        if (rc != SSP_OK) return nullptr;
        if (w == SSP_DEVICE || host == nullptr) return const_cast<void*>(host);
        if (n == CAP) {
            set_error("staging scope: more than %d staged operands in one call", CAP);
            rc = SSP_ERR_UNSUPPORTED;
            return nullptr;
        }
        void* d = load ? const_cast<void*>(op[n].in(ctx, host, bytes, w, &rc)) : op[n].out(ctx, const_cast<void*>(host), bytes, w, &rc);
        back_to[n] = is_out && rc == SSP_OK ? const_cast<void*>(host) : nullptr;
        back_bytes[n++] = bytes;
        return rc == SSP_OK ? d : nullptr;
    }
};

#ifndef SSP_STAGING_NO_HIP
static inline int check_where(int where, const char* fn) {
    if (where != SSP_HOST && where != SSP_DEVICE) SSP_FAIL(SSP_ERR_INVALID, "%s: where", fn);
    return SSP_OK;
}
// hipStreamSynchronize on a stream its owner has already destroyed (a borrowed stream at process exit) does not return an error on
// ROCm 7.2 — it throws std::bad_variant_access out of the C API; nothing may escape a destroy function
static inline bool sync_quietly(hipStream_t s) {
    try {
        return hipStreamSynchronize(s) == hipSuccess;
    } catch (...) {
        return false;
    }
}
// Staging of one operand of an SSP_HOST call: device copy of a host input / device scratch for an output (StageScope's primitive).
struct Staged {
    DevBuf own;  // operands too large for the ctx's pool (or when all its slots are taken)
    const ssp_ctx* pool = nullptr;
    int slot = -1;
    void* p = nullptr;
    Staged() = default;
    Staged(const Staged&) = delete;
    Staged& operator=(const Staged&) = delete;
    ~Staged() {
        if (slot >= 0) pool->stage.give_back(slot);
    }
    int get(const ssp_ctx* ctx, size_t bytes) {
        int rc;
        if (slot >= 0) ctx->stage.give_back(slot);
        slot = ctx->stage.take(bytes, &rc);  // (a slot that could not grow is no error: the operand gets a buffer of its own for the call)
        if (slot >= 0) {
            pool = ctx;
            p = ctx->stage.slot[slot].p;
            return SSP_OK;
        }
        rc = own.alloc(bytes);
        p = own.p;
        return rc;
    }
    const void* in(const ssp_ctx* ctx, const void* host, size_t bytes, int where, int* rc) {
        *rc = SSP_OK;
        if (where == SSP_DEVICE || host == nullptr) return host;
        *rc = get(ctx, bytes);
        if (*rc != SSP_OK) return nullptr;
        hipError_t e = hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            set_error("hipMemcpyAsync H2D failed: %s", hipGetErrorString(e));
            *rc = SSP_ERR_HIP;
            return nullptr;
        }
        return p;
    }
    void* out(const ssp_ctx* ctx, void* host, size_t bytes, int where, int* rc) {
        *rc = SSP_OK;
        if (where == SSP_DEVICE || host == nullptr) return host;
        *rc = get(ctx, bytes);
        return *rc == SSP_OK ? p : nullptr;
    }
    int back(const ssp_ctx* ctx, void* host, size_t bytes, int where) {
        if (where == SSP_DEVICE || host == nullptr) return SSP_OK;
        SSP_HIP(hipMemcpyAsync(host, p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return SSP_OK;
    }
    static int wait(const ssp_ctx* ctx) {
        SSP_HIP(hipStreamSynchronize(ctx->stream));
        return SSP_OK;
    }
    static void wait_quietly(const ssp_ctx* ctx) { (void)sync_quietly(ctx->stream); }
};
using StageScope = StageScopeT<Staged, ssp_ctx>;

// Waits for the ctx stream and the ring's copy streams.  Throws nothing and sets no error message (false = a wait failed).
static inline bool drain_pipe(const ssp_ctx* ctx) {
    bool ok = sync_quietly(ctx->stream);
    if (ctx->pipe) {
        ok = sync_quietly(ctx->pipe->h2d) && ok;
        ok = sync_quietly(ctx->pipe->d2h) && ok;
    }
    return ok;
}
// Scope guard of a ring call: a return before `ok` is set drains the streams, so no copy outlives the call on the CALLER's arrays
struct DrainIfFailed {
    const ssp_ctx* ctx;
    bool ok = false;
    ~DrainIfFailed() {
        if (!ok) (void)drain_pipe(ctx);
    }
};
// The ctx's ring for one call, slots of at least in / raw / out bytes (0: unused).  Made on first use, all or nothing (a half-made pipe
// is freed, the next call starts afresh).  A slot about to grow may still be read by an earlier call's work: all streams drain first.
static inline int pipe_reserve(ssp_ctx* ctx, size_t in, size_t raw, size_t out, size_t pin_in = 0, size_t pin_out = 0) {
    if (!ctx->pipe) {
        std::unique_ptr<HostPipe> p(new (std::nothrow) HostPipe);
        if (!p) SSP_FAIL(SSP_ERR_NOMEM, "host alloc (pipeline)");
        SSP_HIP(hipStreamCreateWithFlags(&p->h2d, hipStreamNonBlocking));
        SSP_HIP(hipStreamCreateWithFlags(&p->d2h, hipStreamNonBlocking));
        for (int i = 0; i < HostPipe::RING; ++i) {
            SSP_HIP(hipEventCreateWithFlags(&p->in_ready[i], hipEventDisableTiming));
            SSP_HIP(hipEventCreateWithFlags(&p->computed[i], hipEventDisableTiming));
            SSP_HIP(hipEventCreateWithFlags(&p->out_done[i], hipEventDisableTiming));
        }
        ctx->pipe = p.release();
    }
    HostPipe& hp = *ctx->pipe;
    bool grow = false;
    for (int k = 0; k < HostPipe::RING; ++k)
        grow = grow || hp.in[k].bytes < in || hp.raw[k].bytes < raw || hp.out[k].bytes < out || hp.pin_in[k].bytes < pin_in ||
               hp.pin_out[k].bytes < pin_out;
    if (!grow) return SSP_OK;
    if (!drain_pipe(ctx)) SSP_FAIL(SSP_ERR_HIP, "host pipeline: draining the streams before its slots grow failed");
    for (int k = 0; k < HostPipe::RING; ++k) {
        if (hp.in[k].bytes < in) SSP_TRY(hp.in[k].alloc(in));
        if (hp.raw[k].bytes < raw) SSP_TRY(hp.raw[k].alloc(raw));
        if (hp.out[k].bytes < out) SSP_TRY(hp.out[k].alloc(out));
        if (hp.pin_in[k].bytes < pin_in) SSP_TRY(hp.pin_in[k].alloc(pin_in));
        if (hp.pin_out[k].bytes < pin_out) SSP_TRY(hp.pin_out[k].alloc(pin_out));
    }
    return SSP_OK;
}
// The ctx's whole-batch pinned bounces (list-fed one-piece paths), at least in / out bytes; grown as the ring's slots are
static inline int pipe_bounce(ssp_ctx* ctx, size_t in, size_t out) {
    SSP_TRY(pipe_reserve(ctx, 0, 0, 0));
    HostPipe& hp = *ctx->pipe;
    if (hp.bounce_in.bytes >= in && hp.bounce_out.bytes >= out) return SSP_OK;
    if (!drain_pipe(ctx)) SSP_FAIL(SSP_ERR_HIP, "host pipeline: draining the streams before its bounce buffers grow failed");
    if (hp.bounce_in.bytes < in) SSP_TRY(hp.bounce_in.alloc(in));
    if (hp.bounce_out.bytes < out) SSP_TRY(hp.bounce_out.alloc(out));
    return SSP_OK;
}
// The ctx's copying threads, sized for this call (SSP_HOST_THREADS is read on every call)
static inline CopyPool& pipe_pool(ssp_ctx* ctx) {
    ctx->pipe->pool.resize(host_threads());
    return ctx->pipe->pool;
}
struct EventSet {  // hipEvents that live as long as the holder (every return path destroys them)
    std::vector<hipEvent_t> ev;
    EventSet() = default;
    EventSet(const EventSet&) = delete;
    EventSet& operator=(const EventSet&) = delete;
    ~EventSet() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int create(size_t n) {
        ev.assign(n, nullptr);
        for (hipEvent_t& e : ev) SSP_HIP(hipEventCreate(&e));
        return SSP_OK;
    }
    hipEvent_t operator[](size_t i) const { return ev[i]; }
};

// feed_rows — a HOST matrix through the ctx's ring of device slots, copied in ahead of its consumer (the scorers' host-fed batches: the
// rows of slice i + 1 and i + 2 cross PCIe on the copy stream while `consume` has slice i's kernels on the ctx stream).  `cuts`: row
// indices 0 = c0 < c1 < ... < cn of the slices; consume(i, dev) launches slice i's work on ctx->stream, dev = device copy of rows
// [cuts[i], cuts[i + 1]).  The host waits for slice i's kernels before it issues the copy that reuses a slot (and consumers may
// therefore reuse host-side tables they upload per slice); on an error everything in flight is drained before it goes up.
template <class F>
static int feed_rows(ssp_ctx* ctx, const void* host, size_t row_bytes, const std::vector<int64_t>& cuts, F&& consume) {
    const int n = (int)cuts.size() - 1;
    if (n <= 0) return SSP_OK;
    size_t max_bytes = 0;
    for (int i = 0; i < n; ++i) max_bytes = std::max(max_bytes, (size_t)(cuts[(size_t)i + 1] - cuts[(size_t)i]) * row_bytes);
    SSP_TRY(pipe_reserve(ctx, max_bytes + 256, 0, 0));
    HostPipe& hp = *ctx->pipe;
    hipStream_t cs = ctx->stream;
    DrainIfFailed guard{ctx};
    auto issue = [&](int i) -> int {
        const int k = i % HostPipe::RING;
        SSP_HIP(hipMemcpyAsync(hp.in[k].p, static_cast<const char*>(host) + (size_t)cuts[(size_t)i] * row_bytes,
                               (size_t)(cuts[(size_t)i + 1] - cuts[(size_t)i]) * row_bytes, hipMemcpyHostToDevice, hp.h2d));
        SSP_HIP(hipEventRecord(hp.in_ready[k], hp.h2d));
        return SSP_OK;
    };
    SSP_TRY(hp.start(cs));
    for (int i = 0; i < n && i < HostPipe::RING - 1; ++i) SSP_TRY(issue(i));
    for (int i = 0; i < n; ++i) {
        if (i + HostPipe::RING - 1 < n) SSP_TRY(issue(i + HostPipe::RING - 1));   // its slot's last reader was slice i - 1: waited for below
        SSP_HIP(hipStreamWaitEvent(cs, hp.in_ready[i % HostPipe::RING], 0));
        SSP_TRY(consume(i, hp.in[i % HostPipe::RING].p));
        SSP_HIP(hipStreamSynchronize(cs));
    }
    guard.ok = true;
    return SSP_OK;
}

static inline size_t host_slice_bytes() {
    size_t mb = 64;  // ~1.2 ms of PCIe per slice: long against a launch's host cost, short against the batch (fill + drain = two slices)
    if (const char* e = getenv("SSP_HOST_SLICE_MB")) mb = (size_t)std::max(1, atoi(e));
    return mb << 20;
}
#endif  // SSP_STAGING_NO_HIP
}  // namespace ssp
#endif
