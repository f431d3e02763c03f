// Host-only ThreadSanitizer driver of the list-fed calls' copying threads (speech_signal_processing_amd/csrc/staging.hpp, WorkPoolT and
// the copy pieces): several threads, each with a pool of its own (one ctx each: the supported use), run batch after batch of random
// spans (byte copies, float32 -> float64 widening, float64 -> float32 narrowing) split into pieces of random size, resize their pools
// between batches, and check every destination byte afterwards.  A job run twice or not at all, a worker that outlives its batch or an
// unsynchronised hand-over is a data race TSan reports or a mismatch counted here.  Built and run by
// tests/test_list_feed_host.py::test_gather_pool_under_thread_sanitizer (g++ -fsanitize=thread): no HIP runtime.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "../../include/ssp.h"

namespace ssp {
struct FakeBuf {   // (StagePoolT's buffer type; unused here)
    void* p = nullptr;
    size_t bytes = 0;
    int alloc(size_t) { return SSP_ERR_NOMEM; }
};
}  // namespace ssp
#define SSP_STAGING_NO_HIP 1
#define SSP_STAGING_PART 1
#include "../../speech_signal_processing_amd/csrc/staging.hpp"
#undef SSP_STAGING_PART

static long run_thread(unsigned seed, int batches) {
    std::mt19937_64 rng(seed);
    ssp::CopyPool pool;
    long bad = 0;
    for (int b = 0; b < batches; ++b) {
        pool.resize(1 + (int)(rng() % 6));
        const int spans = 1 + (int)(rng() % 12);
        std::vector<std::vector<char>> src((size_t)spans), dst((size_t)spans);
        std::vector<int> kind((size_t)spans);
        std::vector<size_t> count((size_t)spans);
        std::vector<ssp::CopyPiece> pieces;
        for (int s = 0; s < spans; ++s) {
            kind[(size_t)s] = (int)(rng() % 3);
            count[(size_t)s] = (size_t)(rng() % 5000);
            const size_t ss = kind[(size_t)s] == ssp::COPY_F64_TO_F32 ? 8 : kind[(size_t)s] == ssp::COPY_F32_TO_F64 ? 4 : 1;
            const size_t ds = kind[(size_t)s] == ssp::COPY_F32_TO_F64 ? 8 : kind[(size_t)s] == ssp::COPY_F64_TO_F32 ? 4 : 1;
            src[(size_t)s].resize(count[(size_t)s] * ss + 1);
            dst[(size_t)s].assign(count[(size_t)s] * ds + 1, 0);
            for (size_t i = 0; i < count[(size_t)s]; ++i) {
                if (kind[(size_t)s] == ssp::COPY_BYTES) src[(size_t)s][i] = (char)rng();
                if (kind[(size_t)s] == ssp::COPY_F32_TO_F64) { float v = (float)((double)(int64_t)rng() * 1e-12); memcpy(&src[(size_t)s][i * 4], &v, 4); }
                if (kind[(size_t)s] == ssp::COPY_F64_TO_F32) { double v = (double)(int64_t)rng() * 1e-13; memcpy(&src[(size_t)s][i * 8], &v, 8); }
            }
            ssp::add_pieces(pieces, src[(size_t)s].data(), dst[(size_t)s].data(), count[(size_t)s], kind[(size_t)s], 1 + rng() % 3000);
        }
        ssp::run_pieces(pool, pieces);
        for (int s = 0; s < spans; ++s) {
            const std::vector<char>&a = src[(size_t)s], &d = dst[(size_t)s];
            for (size_t i = 0; i < count[(size_t)s]; ++i) {
                if (kind[(size_t)s] == ssp::COPY_BYTES) bad += a[i] != d[i];
                if (kind[(size_t)s] == ssp::COPY_F32_TO_F64) { float v; double w; memcpy(&v, &a[i * 4], 4); memcpy(&w, &d[i * 8], 8); bad += (double)v != w; }
                if (kind[(size_t)s] == ssp::COPY_F64_TO_F32) { double v; float w; memcpy(&v, &a[i * 8], 8); memcpy(&w, &d[i * 4], 4); bad += (float)v != w; }
            }
            bad += d.back() != 0;   // (nothing written past the span)
        }
    }
    return bad;
}

int main(int argc, char** argv) {
    const int nthreads = argc > 1 ? atoi(argv[1]) : 4, batches = argc > 2 ? atoi(argv[2]) : 200;
    std::vector<long> bad((size_t)nthreads, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t) th.emplace_back([&, t] { bad[(size_t)t] = run_thread(1234u + (unsigned)t, batches); });
    for (std::thread& t : th) t.join();
    long total = 0;
    for (long b : bad) total += b;
    printf("mismatches %ld\n", total);
    return total == 0 ? 0 : 1;
}
