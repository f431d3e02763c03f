// Host-only driver of how a C-ABI handle is born and dies (speech_signal_processing_amd/csrc/handle.hpp: upload, HandleBuildT,
// destroy_handle_on, SSP_CREATE_GUARD): a three-buffer handle made the way the library's creates make theirs, on a malloc-backed runtime
// stand-in that logs every allocation, queued copy, wait, quiet wait, quiesce and handle destructor call and can be told to fail the k-th
// allocation, the k-th copy or the wait.  No HIP runtime.  Built with -fsanitize=address,undefined and run as a stand-alone process by
// tests/test_host.py::test_handle_life_under_address_sanitizer.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ssp.h"

namespace ssp {
static char g_error[256];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
}  // namespace ssp
#define SSP_HANDLE_NO_HIP 1
#include "../../speech_signal_processing_amd/csrc/handle.hpp"

// 'A' allocation, 'C' queued copy, 'W' wait, 'Q' quiet wait, 'S' quiesce (destroy), 'D' handle destructor
static std::string g_log;
static int g_allocs = 0, g_copies = 0, g_fail_alloc = -1, g_fail_copy = -1;
static bool g_fail_wait = false;

struct FakeCtx {};
struct FakeBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~FakeBuf() { free(p); }
    int alloc(size_t n) {
        if (g_allocs++ == g_fail_alloc) {
            ssp::set_error("injected allocation failure");
            return SSP_ERR_NOMEM;
        }
        g_log += 'A';
        free(p);
        p = malloc(n ? n : 16);
        bytes = n;
        return SSP_OK;
    }
};
struct FakeRt {
    static const char* copy(const FakeCtx*, void* dst, const void* src, size_t bytes) {
        if (g_copies++ == g_fail_copy) return "injected copy failure";
        g_log += 'C';
        memcpy(dst, src, bytes);
        return nullptr;
    }
    static const char* wait(const FakeCtx*) {
        g_log += 'W';
        return g_fail_wait ? "injected wait failure" : nullptr;
    }
    static void wait_quietly(const FakeCtx*) { g_log += 'Q'; }
    static void quiesce(const FakeCtx*) { g_log += 'S'; }
};
struct Handle {
    FakeCtx* ctx = nullptr;
    int tag = 0;
    FakeBuf a, b, c;
    ~Handle() { g_log += 'D'; }
};
using Build = ssp::HandleBuildT<Handle, FakeRt, FakeCtx>;

static int g_failed = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("handle_life: line %d: %s (log %s)\n", __LINE__, #cond, g_log.c_str()); \
            ++g_failed;                                                \
        }                                                              \
    } while (0)

static void reset(int fail_alloc = -1, int fail_copy = -1, bool fail_wait = false) {
    g_log.clear();
    ssp::g_error[0] = 0;
    g_allocs = g_copies = 0;
    g_fail_alloc = fail_alloc;
    g_fail_copy = fail_copy;
    g_fail_wait = fail_wait;
}
static bool starts_with(const char* s, const char* prefix) { return strncmp(s, prefix, strlen(prefix)) == 0; }

// a create as the library writes them: host images, the builder, the uploads, commit; throw_at: 1 = std::bad_alloc before the handle
// exists, 2 = after two uploads; drop: leave without a commit after two uploads
static int make(FakeCtx* ctx, int throw_at, bool drop, Handle** out) try {
    *out = nullptr;
    std::vector<int32_t> ia = {1, 2, 3}, ib = {4, 5};
    const float fc[4] = {6.f, 7.f, 8.f, 9.f};
    if (throw_at == 1) throw std::bad_alloc();
    Build h(ctx, "fake_create");
    h->tag = 42;
    int rc = upload(h, h->a, ia);
    if (rc == SSP_OK) rc = upload(h, h->b, ib);
    if (throw_at == 2) throw std::bad_alloc();
    if (drop) return SSP_ERR_UNSUPPORTED;
    if (rc == SSP_OK) rc = upload(h, h->c, fc, 4);
    return h.commit(rc, out);
}
SSP_CREATE_GUARD("fake_create")

int main() {
    FakeCtx ctx;
    Handle* h = nullptr;

    {   // success: three allocations, three copies, one wait behind the last copy; the handle is the caller's and holds the bytes
        reset();
        CHECK(make(&ctx, 0, false, &h) == SSP_OK);
        CHECK(g_log == "ACACACW" && h != nullptr);
        CHECK(h && h->ctx == &ctx && h->tag == 42 && h->a.bytes == 12 && h->b.bytes == 8 && h->c.bytes == 16);
        CHECK(h && static_cast<int32_t*>(h->a.p)[2] == 3 && static_cast<int32_t*>(h->b.p)[1] == 5 && static_cast<float*>(h->c.p)[3] == 9.f);
        // destroy: one quiesce, then one destructor call; a null handle is nothing at all
        reset();
        CHECK(ssp::destroy_handle_on<FakeRt>(h) == SSP_OK && g_log == "SD");
        reset();
        CHECK(ssp::destroy_handle_on<FakeRt>(static_cast<Handle*>(nullptr)) == SSP_OK && g_log.empty());
    }
    const char* after_alloc_fail[3] = {"D", "ACQD", "ACACQD"};
    for (int k = 0; k < 3; ++k) {   // allocation k fails: nothing later happens; a quiet wait if, and only if, a copy was queued, before the destructor
        reset(k);
        CHECK(make(&ctx, 0, false, &h) == SSP_ERR_NOMEM && h == nullptr);
        CHECK(g_log == after_alloc_fail[k] && g_allocs == k + 1 && g_copies == k);
        CHECK(strcmp(ssp::g_error, "injected allocation failure") == 0);   // (the first failure's message stays)
    }
    const char* after_copy_fail[3] = {"AD", "ACAQD", "ACACAQD"};
    for (int k = 0; k < 3; ++k) {   // copy k fails: the same, with SSP_ERR_HIP and the entry point's name in front
        reset(-1, k);
        CHECK(make(&ctx, 0, false, &h) == SSP_ERR_HIP && h == nullptr);
        CHECK(g_log == after_copy_fail[k] && g_allocs == k + 1 && g_copies == k + 1);
        CHECK(strcmp(ssp::g_error, "fake_create: upload failed: injected copy failure") == 0);
    }
    {   // the final wait fails: no second wait, the destructor once, nothing handed out
        reset(-1, -1, true);
        CHECK(make(&ctx, 0, false, &h) == SSP_ERR_HIP && h == nullptr);
        CHECK(g_log == "ACACACWD");
        CHECK(starts_with(ssp::g_error, "fake_create: upload failed: ") && strstr(ssp::g_error, "injected wait failure"));
    }
    {   // the builder dropped without a commit behind two queued copies: one quiet wait, then the destructor
        reset();
        CHECK(make(&ctx, 0, true, &h) == SSP_ERR_UNSUPPORTED && h == nullptr);
        CHECK(g_log == "ACACQD");
    }
    {   // std::bad_alloc before the handle exists and behind two uploads: SSP_ERR_NOMEM, no leak, the destructor at most once
        reset();
        CHECK(make(&ctx, 1, false, &h) == SSP_ERR_NOMEM && h == nullptr && g_log.empty());
        CHECK(strcmp(ssp::g_error, "fake_create: host alloc") == 0);
        reset();
        CHECK(make(&ctx, 2, false, &h) == SSP_ERR_NOMEM && h == nullptr && g_log == "ACACQD");
        CHECK(strcmp(ssp::g_error, "fake_create: host alloc") == 0);
    }
    {   // an empty table: nothing allocated, nothing copied, nothing to wait for
        reset();
        ssp::UploadScopeT<FakeRt, FakeCtx> q(&ctx, "fake_upload");
        FakeBuf buf;
        const std::vector<float> none;
        CHECK(upload(q, buf, none) == SSP_OK && g_log.empty() && buf.p == nullptr);
        CHECK(q.wait() == SSP_OK && g_log.empty());
    }
    CHECK(g_log.empty());   // (... nor does the scope's destructor wait)
    {   // a scope of its own (a work table outside a create): wait() is the one wait; left early, the destructor waits quietly
        reset();
        FakeBuf buf;
        const std::vector<int32_t> tab = {1, 2};
        {
            ssp::UploadScopeT<FakeRt, FakeCtx> q(&ctx, "fake_upload");
            CHECK(upload(q, buf, tab) == SSP_OK && q.wait() == SSP_OK);
        }
        CHECK(g_log == "ACW");
        {
            ssp::UploadScopeT<FakeRt, FakeCtx> q(&ctx, "fake_upload");
            CHECK(upload(q, buf, tab) == SSP_OK);
        }
        CHECK(g_log == "ACWACQ");
    }
    printf("handle_life: %d failed checks\n", g_failed);
    return g_failed == 0 ? 0 : 1;
}
