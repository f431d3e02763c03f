// Score normalisation and detection-error counts on gfx950 (ssp_topn_stats, ssp_snorm_apply, ssp_det_counts): what follows a scoring sweep
// in a verification system.  An extension: the reference has neither; Kaldi, sidekit, SpeechBrain and wespeaker ship S-norm / AS-norm and
// a DET sweep.  include/ssp.h has the definitions, tests/snorm_oracle.py restates them.  Everything is fp32, no operation is contracted.
// Kernels:
//   snorm_topn_kernel    one wave per line (a row, or with AXIS = 0 a column read at stride ld).  The line becomes order-preserving 32-bit
//                        keys (sign bit flipped on non-negatives, all bits on negatives); the m-th largest key is found by bisection over
//                        the 32 key bits: per bit one compare per key, whose ballots are counted on the scalar unit — exact, no LDS, no
//                        atomics, ties cost nothing.  Then two fixed-shape passes: sum of (v - kth) over the keys above the threshold
//                        (the copies of the threshold value add zero), and the square sum about the mean.  NK > 0: the line's keys stay in
//                        NK registers per lane (lines up to 64 NK entries); NK = 0: every pass reads the line again (up to 65536 entries).
//   snorm_apply_kernel   one wave per row: z = 0.5 ((x - col_mean) / col_dev + (x - row_mean) / row_dev) (or one term alone) with IEEE
//                        division, written out (in place if asked) under a running (max, first index) over the entries that are not NaN
//   snorm_target_kernel  raises a flag for a target outside [-1, S)
//   snorm_det_kernel     thresholds and the workgroup's two histograms in LDS; per score a fixed-depth binary search and one LDS integer
//                        add; at the end one 64-bit integer add per non-empty bin to the global histograms; the score ranges through
//                        integer maxima of the keys.  Integer sums: exact and the same every call.
#include <algorithm>
#include <cmath>
#include <limits>

#include "common.hpp"

#pragma clang fp contract(off)  // the sums below are restated operation by operation (tests/snorm_oracle.py)

namespace ssp {

constexpr int SN_LINE_MAX = 65536;  // longest line of ssp_topn_stats
constexpr int SN_DET_MAX_M = 4096;  // most thresholds of ssp_det_counts
constexpr int SN_DET_BLOCKS = 2048; // workgroups of the histogram launch (rows are strided over them)

__device__ __forceinline__ uint32_t sn_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sn_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
// the fixed butterfly every lane ends with the same sum
__device__ __forceinline__ float sn_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int sn_count(bool p) { return __builtin_popcountll(__builtin_amdgcn_ballot_w64(p)); }

struct TopnArgs {
    const float* x;
    float* mean;  // each output nullable
    float* sd;
    float* kth;
    int64_t n_lines, ld;
    int32_t len, m;  // entries per line, m = min(n, len)
};

// (64 resident keys and their values do not fit the 128 registers of four waves per SIMD: that instance plans for two)
template <int NK, int AXIS>
__global__ __launch_bounds__(256, NK == 64 ? 2 : 4) void snorm_topn_kernel(TopnArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t line = (int64_t)blockIdx.x * 4 + wave;
    if (line >= a.n_lines) return;
    const float* base = AXIS == 1 ? a.x + line * a.ld : a.x + line;
    const int64_t stride = AXIS == 1 ? 1 : a.ld;
    const int L = a.len, m = a.m;
    // padding has key 0, below the key of every finite value: it is never counted and never above a threshold
    uint32_t k[NK > 0 ? NK : 1];
    bool bad = false;
    if constexpr (NK > 0) {
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            const int idx = lane + 64 * j;
            const float v = idx < L ? base[(int64_t)idx * stride] : 0.f;
            bad = bad || !(fabsf(v) < INFINITY);
            k[j] = idx < L ? sn_key(v) : 0u;
        }
    } else {
        for (int idx = lane; idx < L; idx += 64) bad = bad || !(fabsf(base[(int64_t)idx * stride]) < INFINITY);
    }
    auto each = [&](auto&& f) {  // f(key) for every entry of the line and some padding, the same trip count in every lane
        if constexpr (NK > 0) {
#pragma unroll
            for (int j = 0; j < NK; ++j) f(k[j]);
        } else {
            for (int b0 = 0; b0 < L; b0 += 256) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int idx = b0 + 64 * u + lane;
                    f(idx < L ? sn_key(base[(int64_t)idx * stride]) : 0u);
                }
            }
        }
    };
    // the largest T with #{key >= T} >= m: the m-th largest key
    uint32_t T = 0;
    for (int b = 31; b >= 0; --b) {
        const uint32_t cand = T | (1u << b);
        int cnt = 0;
        each([&](uint32_t kk) { cnt += sn_count(kk >= cand); });
        if (cnt >= m) T = cand;
    }
    const float vT = sn_unkey(T), fm = (float)m;
    int above = 0;
    float s1 = 0.f;
    each([&](uint32_t kk) {
        const bool gt = kk > T;
        above += sn_count(gt);
        s1 += gt ? sn_unkey(kk) - vT : 0.f;
    });
    const float mean = vT + sn_wave_sum(s1) / fm;
    float s2 = 0.f;
    each([&](uint32_t kk) {
        const float d = sn_unkey(kk) - mean;
        s2 += kk > T ? d * d : 0.f;
    });
    const float dT = vT - mean;
    const float sd = sqrtf((sn_wave_sum(s2) + (float)(m - above) * (dT * dT)) / fm);
    const bool any_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if (lane == 0) {
        const float nanv = __builtin_nanf("");
        if (a.mean) a.mean[line] = any_bad ? nanv : mean;
        if (a.sd) a.sd[line] = any_bad ? nanv : sd;
        if (a.kth) a.kth[line] = any_bad ? nanv : vT;
    }
}

template <int AXIS>
static int launch_topn(const TopnArgs& a, hipStream_t s) {
    const int64_t grid = ceil_div<int64_t>(a.n_lines, 4);
    if (grid > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_topn_stats: too many lines for one launch");
    const dim3 g((unsigned)grid), b(256);
    if (a.len <= 256)
        hipLaunchKernelGGL((snorm_topn_kernel<4, AXIS>), g, b, 0, s, a);
    else if (a.len <= 1024)
        hipLaunchKernelGGL((snorm_topn_kernel<16, AXIS>), g, b, 0, s, a);
    else if (a.len <= 2048)
        hipLaunchKernelGGL((snorm_topn_kernel<32, AXIS>), g, b, 0, s, a);
    else if (a.len <= 4096)
        hipLaunchKernelGGL((snorm_topn_kernel<64, AXIS>), g, b, 0, s, a);
    else
        hipLaunchKernelGGL((snorm_topn_kernel<0, AXIS>), g, b, 0, s, a);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

struct ApplyArgs {
    const float* x;  // may alias out
    float* out;      // nullable
    const float *rm, *rs, *cm, *cs;
    int32_t* am;  // nullable
    float* mx;    // nullable
    int64_t N, ld, ldo;
    int32_t S;
    float floor;
};

template <bool ROW, bool COL>
__global__ __launch_bounds__(256, 8) void snorm_apply_kernel(ApplyArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= a.N) return;
    float rmean = 0.f, rden = 1.f;
    if (ROW) {
        rmean = a.rm[row];
        rden = nanmax(a.rs[row], a.floor);
    }
    const float* x = a.x + row * a.ld;
    float* o = a.out ? a.out + row * a.ldo : nullptr;
    float best = -INFINITY;
    int besti = 0x7fffffff;
    for (int c = lane; c < a.S; c += 64) {
        const float v = x[c];
        float z;
        if (ROW && COL)
            z = 0.5f * ((v - a.cm[c]) / nanmax(a.cs[c], a.floor) + (v - rmean) / rden);
        else if (COL)
            z = (v - a.cm[c]) / nanmax(a.cs[c], a.floor);
        else
            z = (v - rmean) / rden;
        if (o) o[c] = z;
        if (z > best || (z == best && c < besti)) {  // (a lane's columns ascend: only the first of equals is kept)
            best = z;
            besti = c;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(besti, off);
        if (ob > best || (ob == best && oi < besti)) {
            best = ob;
            besti = oi;
        }
    }
    if (lane == 0) {
        const bool none = besti == 0x7fffffff;  // every entry NaN
        if (a.am) a.am[row] = none ? -1 : besti;
        if (a.mx) a.mx[row] = none ? __builtin_nanf("") : best;
    }
}

__global__ __launch_bounds__(256) void snorm_target_kernel(const int32_t* __restrict__ target, int64_t N, int S, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N && (target[i] < -1 || target[i] >= S)) *flag = 1;
}

struct DetArgs {
    const float* x;
    const int32_t* target;
    const float* th;           // [M] ascending
    unsigned long long* hist;  // [M + 1] target, [M + 1] non-target, [2] NaN counts
    uint32_t* range;           // maxima of: ~key of target scores, key of target scores, ~key of non-targets, key of non-targets (0 = none)
    int64_t N, ld;
    int32_t S, M, P;           // P: the largest power of two <= M (0 when M = 0)
};

__global__ __launch_bounds__(256, 8) void snorm_det_kernel(DetArgs a) {
    extern __shared__ __attribute__((aligned(16))) char sn_smem[];
    float* th = reinterpret_cast<float*>(sn_smem);           // [M]
    uint32_t* cnt = reinterpret_cast<uint32_t*>(th + a.M);   // [2 (M + 1) + 2], the layout of a.hist
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = a.M, bins = 2 * (M + 1) + 2;
    for (int i = tid; i < M; i += 256) th[i] = a.th[i];
    for (int i = tid; i < bins; i += 256) cnt[i] = 0u;
    __syncthreads();
    uint32_t r[4] = {0u, 0u, 0u, 0u};
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < a.N; row += (int64_t)gridDim.x * 4) {
        const int tg = a.target[row];
        const float* x = a.x + row * a.ld;
        for (int c = lane; c < a.S; c += 64) {
            const float v = x[c];
            const int non = c == tg ? 0 : 1;
            if (v != v) {
                atomicAdd(&cnt[2 * (M + 1) + non], 1u);
                continue;
            }
            int pos = 0;  // #{j : th[j] <= v}
            for (int step = a.P; step > 0; step >>= 1)
                if (pos + step <= M && th[pos + step - 1] <= v) pos += step;
            atomicAdd(&cnt[non * (M + 1) + pos], 1u);
            const uint32_t key = sn_key(v);
            r[2 * non] = max(r[2 * non], ~key);
            r[2 * non + 1] = max(r[2 * non + 1], key);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t v = r[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off));
        if (lane == 0 && v) atomicMax(&a.range[i], v);
    }
    __syncthreads();
    for (int i = tid; i < bins; i += 256)
        if (cnt[i]) atomicAdd(&a.hist[i], (unsigned long long)cnt[i]);
}

}  // namespace ssp

using namespace ssp;

extern "C" {

int ssp_topn_stats(ssp_ctx* ctx, const float* scores, int64_t rows, int32_t cols, int64_t ld, int32_t axis, int32_t n, float* mean_out,
                   float* std_out, float* kth_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_topn_stats");
    if (!ctx) SSP_FAIL(SSP_ERR_INVALID, "null ssp_ctx");
    if (n < 1 || rows < 0 || cols < 1 || ld < cols)
        SSP_FAIL(SSP_ERR_INVALID, "ssp_topn_stats: bad shape (rows=%lld, cols=%d, ld=%lld, n=%d)", (long long)rows, cols, (long long)ld, n);
    if (axis != 0 && axis != 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_topn_stats: axis=%d", axis);
    SSP_TRY(check_where(where, "ssp_topn_stats"));
    if (rows > 0 && !scores) SSP_FAIL(SSP_ERR_INVALID, "ssp_topn_stats: null scores");
    const int64_t len = axis == 1 ? (int64_t)cols : rows, n_lines = axis == 1 ? rows : (int64_t)cols;
    if (len > SN_LINE_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_topn_stats: lines of %lld entries exceed the supported length (%d)", (long long)len, SN_LINE_MAX);
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (rows == 0) return SSP_OK;
    StageScope st(ctx, where);
    const size_t in_bytes = ((size_t)(rows - 1) * (size_t)ld + (size_t)cols) * sizeof(float), out_bytes = (size_t)n_lines * sizeof(float);
    const float* dX = st.in(scores, in_bytes);
    float *dM = st.out(mean_out, out_bytes), *dS = st.out(std_out, out_bytes), *dK = st.out(kth_out, out_bytes);
    SSP_TRY(st.status());
    TopnArgs a{dX, dM, dS, dK, n_lines, ld, (int32_t)len, (int32_t)std::min<int64_t>(n, len)};
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, ctx->stream));
    SSP_TRY(axis == 1 ? launch_topn<1>(a, ctx->stream) : launch_topn<0>(a, ctx->stream));
    SSP_TRY(tm.stop(ctx->stream, kernel_ms));
    return st.finish();
}

int ssp_snorm_apply(ssp_ctx* ctx, const float* scores, int64_t N, int32_t S, int64_t ld, const float* row_mean, const float* row_std,
                    const float* col_mean, const float* col_std, float std_floor, float* out, int64_t ld_out, int32_t* argmax_out, float* max_out,
                    int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_snorm_apply");
    if (!ctx) SSP_FAIL(SSP_ERR_INVALID, "null ssp_ctx");
    if (N < 0 || S < 1 || ld < S) SSP_FAIL(SSP_ERR_INVALID, "ssp_snorm_apply: bad shape (N=%lld, S=%d, ld=%lld)", (long long)N, S, (long long)ld);
    if (out && ld_out < S) SSP_FAIL(SSP_ERR_INVALID, "ssp_snorm_apply: ld_out=%lld < S=%d", (long long)ld_out, S);
    SSP_TRY(check_where(where, "ssp_snorm_apply"));
    if ((row_mean == nullptr) != (row_std == nullptr) || (col_mean == nullptr) != (col_std == nullptr))
        SSP_FAIL(SSP_ERR_INVALID, "ssp_snorm_apply: a mean without its deviation");
    if (!row_mean && !col_mean) SSP_FAIL(SSP_ERR_INVALID, "ssp_snorm_apply: neither row nor column statistics");
    if (!(std_floor > 0.f) || !std::isfinite(std_floor)) SSP_FAIL(SSP_ERR_INVALID, "ssp_snorm_apply: std_floor must be finite and > 0");
    if (N > 0 && !scores) SSP_FAIL(SSP_ERR_INVALID, "ssp_snorm_apply: null scores");
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (N == 0) return SSP_OK;
    if (ceil_div<int64_t>(N, 4) > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_snorm_apply: too many rows for one launch");
    StageScope st(ctx, where);
    const size_t in_bytes = ((size_t)(N - 1) * (size_t)ld + (size_t)S) * sizeof(float);
    const size_t out_bytes = ((size_t)(N - 1) * (size_t)(out ? ld_out : 0) + (size_t)S) * sizeof(float);
    const float* dX = st.in(scores, in_bytes);
    const float *dRm = st.in(row_mean, (size_t)N * sizeof(float)), *dRs = st.in(row_std, (size_t)N * sizeof(float));
    const float *dCm = st.in(col_mean, (size_t)S * sizeof(float)), *dCs = st.in(col_std, (size_t)S * sizeof(float));
    // (a staged output never aliases the staged input: the kernel reads, then writes; pre-loaded when the gaps between the rows of a
    //  host output have to keep their bytes)
    float* dO = st.out(out, out_bytes, ld_out > S);
    int32_t* dA = st.out(argmax_out, (size_t)N * sizeof(int32_t));
    float* dMx = st.out(max_out, (size_t)N * sizeof(float));
    SSP_TRY(st.status());
    ApplyArgs a{dX, dO, dRm, dRs, dCm, dCs, dA, dMx, N, ld, ld_out, S, std_floor};
    const dim3 g((unsigned)ceil_div<int64_t>(N, 4)), b(256);
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, ctx->stream));
    if (dRm && dCm)
        hipLaunchKernelGGL((snorm_apply_kernel<true, true>), g, b, 0, ctx->stream, a);
    else if (dCm)
        hipLaunchKernelGGL((snorm_apply_kernel<false, true>), g, b, 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((snorm_apply_kernel<true, false>), g, b, 0, ctx->stream, a);
    SSP_HIP(hipGetLastError());
    SSP_TRY(tm.stop(ctx->stream, kernel_ms));
    return st.finish();
}

int ssp_det_counts(ssp_ctx* ctx, const float* scores, int64_t N, int32_t S, int64_t ld, const int32_t* target, const float* thresholds, int32_t M,
                   int64_t* tar_hist, int64_t* non_hist, int64_t* nan_count, float* range_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_det_counts");
    if (!ctx) SSP_FAIL(SSP_ERR_INVALID, "null ssp_ctx");
    if (N < 0 || S < 1 || ld < S) SSP_FAIL(SSP_ERR_INVALID, "ssp_det_counts: bad shape (N=%lld, S=%d, ld=%lld)", (long long)N, S, (long long)ld);
    if (M < 0 || M > SN_DET_MAX_M) SSP_FAIL(SSP_ERR_INVALID, "ssp_det_counts: M=%d outside [0, %d]", M, SN_DET_MAX_M);
    SSP_TRY(check_where(where, "ssp_det_counts"));
    if (!tar_hist || !non_hist || !nan_count || !range_out || (M > 0 && !thresholds) || (N > 0 && (!scores || !target)))
        SSP_FAIL(SSP_ERR_INVALID, "ssp_det_counts: null pointer");
    for (int j = 0; j < M; ++j)
        if (!std::isfinite(thresholds[j]) || (j > 0 && thresholds[j] < thresholds[j - 1]))
            SSP_FAIL(SSP_ERR_INVALID, "ssp_det_counts: thresholds[%d] is not finite or descends", j);
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    const float inf = std::numeric_limits<float>::infinity();
    const int bins = 2 * (M + 1) + 2;
    std::vector<unsigned long long> h((size_t)bins + 3, 0ull);  // the histograms and NaN counts, then 4 range words and the flag
    if (N > 0) {
        const unsigned grid = (unsigned)std::min<int64_t>(ceil_div<int64_t>(N, 4), SN_DET_BLOCKS);
        if ((double)(ceil_div<int64_t>(N, (int64_t)grid * 4) * 4) * (double)S >= 4294967296.0)
            SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_det_counts: too many scores per workgroup for 32-bit bins");
        if (ceil_div<int64_t>(N, 256) > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_det_counts: too many rows");
        hipStream_t s = ctx->stream;
        StageScope st(ctx, where);
        const float* dX = st.in(scores, ((size_t)(N - 1) * (size_t)ld + (size_t)S) * sizeof(float));
        const int32_t* dT = st.in(target, (size_t)N * sizeof(int32_t));
        SSP_TRY(st.status());
        DevBuf th, acc;
        SSP_TRY(th.alloc((size_t)std::max(M, 1) * sizeof(float)));
        SSP_TRY(acc.alloc(h.size() * sizeof(unsigned long long)));
        if (M > 0) SSP_HIP(hipMemcpyAsync(th.p, thresholds, (size_t)M * sizeof(float), hipMemcpyHostToDevice, s));
        SSP_HIP(hipMemsetAsync(acc.p, 0, h.size() * sizeof(unsigned long long), s));
        uint32_t* words = reinterpret_cast<uint32_t*>(acc.as<unsigned long long>() + bins);
        int P = M > 0 ? 1 : 0;
        while (M > 0 && 2 * P <= M) P *= 2;
        DetArgs a{dX, dT, th.as<float>(), acc.as<unsigned long long>(), words, N, ld, S, M, P};
        Timer tm;
        SSP_TRY(tm.start(kernel_ms != nullptr, s));
        hipLaunchKernelGGL(snorm_target_kernel, dim3((unsigned)ceil_div<int64_t>(N, 256)), dim3(256), 0, s, dT, N, S, reinterpret_cast<int32_t*>(words + 4));
        hipLaunchKernelGGL(snorm_det_kernel, dim3(grid), dim3(256), (size_t)(M + bins) * sizeof(float), s, a);
        if (hipGetLastError() != hipSuccess) {
            (void)hipStreamSynchronize(s);
            SSP_FAIL(SSP_ERR_HIP, "ssp_det_counts: kernel launch failed");
        }
        SSP_TRY(tm.stop(s, kernel_ms));
        SSP_HIP(hipMemcpyAsync(h.data(), acc.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        SSP_HIP(hipStreamSynchronize(s));  // the one wait of the call
    }
    uint32_t words[6];
    std::memcpy(words, h.data() + bins, sizeof(words));
    if (words[4]) SSP_FAIL(SSP_ERR_INVALID, "ssp_det_counts: a target outside [-1, %d)", S);
    for (int j = 0; j <= M; ++j) {
        tar_hist[j] = (int64_t)h[(size_t)j];
        non_hist[j] = (int64_t)h[(size_t)(M + 1 + j)];
    }
    nan_count[0] = (int64_t)h[(size_t)(2 * (M + 1))];
    nan_count[1] = (int64_t)h[(size_t)(2 * (M + 1) + 1)];
    auto unkey = [](uint32_t k) {
        const uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
        float f;
        std::memcpy(&f, &u, sizeof(f));
        return f;
    };
    for (int i = 0; i < 2; ++i) {
        range_out[2 * i] = words[2 * i] ? unkey(~words[2 * i]) : inf;
        range_out[2 * i + 1] = words[2 * i + 1] ? unkey(words[2 * i + 1]) : -inf;
    }
    return SSP_OK;
}

}  // extern "C"
