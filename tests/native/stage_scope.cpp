// Host-only driver of the staging scope of the host-or-device entry points (speech_signal_processing_amd/csrc/staging.hpp, StageScopeT):
// the scope's own logic — what is staged, what is copied back, when it waits, what it releases — with a malloc-backed operand stand-in
// that logs every copy and wait, on the real slot pool (StagePoolT).  No HIP runtime.  Built with -fsanitize=address,undefined and run as
// a stand-alone process by tests/test_host.py::test_stage_scope_under_address_sanitizer.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
struct FakeBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~FakeBuf() { free(p); }
    int alloc(size_t n) {
        free(p);
        p = malloc(n ? n : 16);
        bytes = p ? n : 0;
        return p ? SSP_OK : SSP_ERR_NOMEM;
    }
};
}  // namespace ssp
#define SSP_STAGING_NO_HIP 1
#define SSP_STAGING_PART 1
#include "../../speech_signal_processing_amd/csrc/staging.hpp"
#undef SSP_STAGING_PART
#define SSP_STAGING_PART 2
#include "../../speech_signal_processing_amd/csrc/staging.hpp"

using Pool = ssp::StagePoolT<ssp::FakeBuf>;
struct FakeCtx {
    mutable Pool stage;
};
struct Event {
    char kind;  // 'I' host-to-device copy, 'O' device-to-host copy, 'W' wait, 'Q' quiet wait, 'R' slot released
    const void* host;
    size_t bytes;
};
static std::vector<Event> g_log;
static int g_gets = 0, g_fail_get = -1;  // staged operands so far; the one whose staging fails (-1: none)

// what Staged is to the library: a pool slot per operand, copies by memcpy
struct FakeOp {
    const FakeCtx* pool = nullptr;
    int slot = -1;
    void* p = nullptr;
    ~FakeOp() {
        if (slot < 0) return;
        g_log.push_back({'R', nullptr, 0});
        pool->stage.give_back(slot);
    }
    int get(const FakeCtx* ctx, size_t bytes) {
        if (g_gets++ == g_fail_get) {
            ssp::set_error("injected staging failure");
            return SSP_ERR_NOMEM;
        }
        int rc;
        slot = ctx->stage.take(bytes, &rc);
        if (slot < 0) return rc != SSP_OK ? rc : SSP_ERR_NOMEM;  // (the tests never exhaust the pool by themselves)
        pool = ctx;
        p = ctx->stage.slot[slot].p;
        return SSP_OK;
    }
    const void* in(const FakeCtx* ctx, const void* host, size_t bytes, int where, int* rc) {
        *rc = SSP_OK;
        if (where == SSP_DEVICE || host == nullptr) return host;
        *rc = get(ctx, bytes);
        if (*rc != SSP_OK) return nullptr;
        memcpy(p, host, bytes);
        g_log.push_back({'I', host, bytes});
        return p;
    }
    void* out(const FakeCtx* ctx, void* host, size_t bytes, int where, int* rc) {
        *rc = SSP_OK;
        if (where == SSP_DEVICE || host == nullptr) return host;
        *rc = get(ctx, bytes);
        return *rc == SSP_OK ? p : nullptr;
    }
    int back(const FakeCtx*, void* host, size_t bytes, int where) {
        if (where == SSP_DEVICE || host == nullptr) return SSP_OK;
        memcpy(host, p, bytes);
        g_log.push_back({'O', host, bytes});
        return SSP_OK;
    }
    static int wait(const FakeCtx*) {
        g_log.push_back({'W', nullptr, 0});
        return SSP_OK;
    }
    static void wait_quietly(const FakeCtx*) { g_log.push_back({'Q', nullptr, 0}); }
};
using Scope = ssp::StageScopeT<FakeOp, FakeCtx>;

static int g_failed = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("stage_scope: line %d: %s\n", __LINE__, #cond);     \
            ++g_failed;                                                \
        }                                                              \
    } while (0)

static int count(char kind) {
    int n = 0;
    for (const Event& e : g_log) n += e.kind == kind;
    return n;
}
static bool is(size_t i, char kind, const void* host, size_t bytes) {
    return i < g_log.size() && g_log[i].kind == kind && g_log[i].host == host && g_log[i].bytes == bytes;
}
static bool all_free(const FakeCtx& c) {
    for (int i = 0; i < Pool::SLOTS; ++i)
        if (c.stage.busy[i]) return false;
    return true;
}
static void reset(int fail_get = -1) {
    g_log.clear();
    g_gets = 0;
    g_fail_get = fail_get;
}

int main() {
    FakeCtx ctx;
    int32_t a[3] = {1, 2, 3}, b[2] = {0, 0}, c[4] = {7, 7, 7, 7}, d[2] = {5, 5};
    int32_t* none = nullptr;

    {   // a host call: inputs go in with their bytes, null operands pass, each output comes back once, in the order of the out calls
        reset();
        {
            Scope st(&ctx, SSP_HOST);
            const int32_t* da = st.in(a, sizeof(a));
            const int32_t* dn = st.in(static_cast<const int32_t*>(none), 64);
            int32_t* db = st.out(b, sizeof(b));
            int32_t* dno = st.out(none, 64);
            int32_t* dc = st.out(c, sizeof(c), true);   // pre-loaded
            CHECK(st.status() == SSP_OK);
            CHECK(da && da != a && da[0] == 1 && da[2] == 3);
            CHECK(dn == nullptr && dno == nullptr);
            CHECK(db && db != b && dc && dc != c);
            CHECK(g_gets == 3 && g_log.size() == 2 && is(0, 'I', a, sizeof(a)) && is(1, 'I', c, sizeof(c)));
            CHECK(dc[0] == 7 && dc[3] == 7);
            db[0] = 10, db[1] = 11, dc[1] = 12;   // (the kernels)
            CHECK(st.copy_back() == SSP_OK);
            CHECK(g_log.size() == 4 && is(2, 'O', b, sizeof(b)) && is(3, 'O', c, sizeof(c)));   // no wait
            CHECK(b[0] == 10 && b[1] == 11 && c[0] == 7 && c[1] == 12);
            CHECK(st.finish() == SSP_OK);
            CHECK(g_log.size() == 5 && is(4, 'W', nullptr, 0));   // nothing copied twice, one wait
            CHECK(!all_free(ctx));
        }
        CHECK(count('Q') == 0 && count('W') == 1 && count('O') == 2 && count('R') == 3 && all_free(ctx));
    }
    {   // finish alone: the copies, then exactly one wait
        reset();
        {
            Scope st(&ctx, SSP_HOST);
            int32_t* db = st.out(b, sizeof(b));
            db[0] = 20, db[1] = 21;
            CHECK(st.finish() == SSP_OK);
            CHECK(g_log.size() == 2 && is(0, 'O', b, sizeof(b)) && is(1, 'W', nullptr, 0) && b[1] == 21);
        }
        CHECK(count('Q') == 0 && count('W') == 1 && all_free(ctx));
    }
    {   // a device call: every pointer passes, nothing is staged, copied or waited for
        reset();
        {
            Scope st(&ctx, SSP_DEVICE);
            CHECK(st.in(a, sizeof(a)) == a && st.out(b, sizeof(b)) == b && st.out(c, sizeof(c), true) == c && st.out(none, 8) == nullptr);
            CHECK(st.status() == SSP_OK && st.copy_back() == SSP_OK && st.finish() == SSP_OK);
            CHECK(all_free(ctx));
        }
        CHECK(g_log.empty() && g_gets == 0);
    }
    {   // a device call with a host table: only the table is staged, and finish(true) is the one wait
        reset();
        {
            Scope st(&ctx, SSP_DEVICE);
            const int32_t* dt = st.in_host(a, sizeof(a));
            CHECK(dt && dt != a && dt[1] == 2 && st.in(d, sizeof(d)) == d && st.out(b, sizeof(b)) == b);
            CHECK(st.finish(true) == SSP_OK);
            CHECK(g_log.size() == 2 && is(0, 'I', a, sizeof(a)) && is(1, 'W', nullptr, 0));
        }
        CHECK(count('Q') == 0 && count('R') == 1 && all_free(ctx));
    }
    {   // a failure on the second staged operand sticks: nothing later is staged, nothing is copied back, nothing waits
        reset(1);
        {
            Scope st(&ctx, SSP_HOST);
            CHECK(st.in(a, sizeof(a)) != nullptr);
            CHECK(st.out(b, sizeof(b)) == nullptr && st.status() == SSP_ERR_NOMEM);
            CHECK(st.out(c, sizeof(c), true) == nullptr && st.in(d, sizeof(d)) == nullptr && st.in(static_cast<const int32_t*>(none), 8) == nullptr);
            CHECK(g_gets == 2 && st.status() == SSP_ERR_NOMEM && strcmp(ssp::g_error, "injected staging failure") == 0);
            CHECK(st.copy_back() == SSP_ERR_NOMEM && st.finish() == SSP_ERR_NOMEM);
            CHECK(g_log.size() == 1 && is(0, 'I', a, sizeof(a)));
        }
        CHECK(count('O') == 0 && count('W') == 0 && count('Q') == 0 && all_free(ctx));
    }
    {   // a failure after outputs were registered: they are not copied back either
        reset(2);
        {
            Scope st(&ctx, SSP_HOST);
            (void)st.out(b, sizeof(b));
            (void)st.out(c, sizeof(c));
            CHECK(st.in(a, sizeof(a)) == nullptr && st.status() == SSP_ERR_NOMEM);
            CHECK(st.finish() == SSP_ERR_NOMEM);
        }
        CHECK(count('O') == 0 && count('W') == 0 && count('Q') == 0 && all_free(ctx));
    }
    {   // a host call that leaves with copies queued and no wait: the destructor waits, quietly, before a slot goes back
        reset();
        {
            Scope st(&ctx, SSP_HOST);
            (void)st.in(a, sizeof(a));
            (void)st.out(b, sizeof(b));
            CHECK(st.copy_back() == SSP_OK);
        }
        CHECK(g_log.size() == 5 && is(0, 'I', a, sizeof(a)) && is(1, 'O', b, sizeof(b)) && is(2, 'Q', nullptr, 0) && g_log[3].kind == 'R' && g_log[4].kind == 'R');
        CHECK(count('W') == 0 && all_free(ctx));
    }
    {   // ... unless the caller has waited by means of its own, or nothing was queued, or the call is a device call
        reset();
        {
            Scope st(&ctx, SSP_HOST);
            (void)st.out(b, sizeof(b));
            CHECK(st.copy_back() == SSP_OK);
            st.waited();
        }
        {
            Scope st(&ctx, SSP_HOST);
            (void)st.in(a, sizeof(a));
            (void)st.out(b, sizeof(b));
        }
        {
            Scope st(&ctx, SSP_DEVICE);
            (void)st.out(b, sizeof(b));
            CHECK(st.copy_back() == SSP_OK);
        }
        CHECK(count('Q') == 0 && count('W') == 0 && count('O') == 1 && all_free(ctx));
    }
    {   // the ninth staged operand is an error, not an overrun; the eight before it are released
        reset();
        int32_t v[Scope::CAP + 1] = {};
        {
            Scope st(&ctx, SSP_HOST);
            for (int i = 0; i < Scope::CAP; ++i) CHECK(st.in(&v[i], sizeof(int32_t)) != nullptr);
            CHECK(st.status() == SSP_OK && !all_free(ctx));
            CHECK(st.out(&v[Scope::CAP], sizeof(int32_t)) == nullptr && st.status() == SSP_ERR_UNSUPPORTED);
            CHECK(g_gets == Scope::CAP && st.finish() == SSP_ERR_UNSUPPORTED);
        }
        CHECK(count('R') == Scope::CAP && count('O') == 0 && count('W') == 0 && count('Q') == 0 && all_free(ctx));
    }
    printf("stage_scope: %d failed checks\n", g_failed);
    return g_failed == 0 ? 0 : 1;
}
