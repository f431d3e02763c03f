// k-means++ seeding on the GPU (ssp_kmeanspp_seed): the seeds gmm_train.GaussianMixture._kmeanspp draws for the k-means start of
// sklearn's GaussianMixture(init_params='kmeans') (GMM_UBM.py:158-170; sklearn cluster/_kmeans.py:kmeans_plusplus), with the random numbers
// handed in.  ONE workgroup runs the whole sequential algorithm of one PROBLEM (a model and a start): no grid-wide sync, no host round trip
// between the K - 1 steps; a launch covers P problems.
//
// Arithmetic.  The rows stay float32 in memory and are widened on load; d2, cum, dc and pot are float64 in the direct-difference form
// sum_d (x - c)^2.  No floating-point atomics: every sum has a fixed shape that depends on n and the workgroup size only.
//   distances  one lane per row, d = 0 .. D-1 in order (two interleaved fma chains: even and odd d)
//   pot[l]     per lane over its tiles in order, xor-butterfly over the 64 lanes, the KPP_NW waves in order
//   cum        three sequential levels: a lane's chunk of ceil(n / KPP_T) consecutive rows, the 64 lanes of a wave, the waves;
//              cum[i] = wave offset + (lane offset + running sum).  Every level is a left-to-right sum, so a run of zero d2 (duplicates
//              of a chosen centre) leaves cum bit-equal along the run and total = cum[n-1].
// A candidate is cand[l] = min(n-1, #{i : cum[i] < u*total}) (numpy's searchsorted side='left' and the clip), counted with integers.
//
// Memory.  d2[n] and dc[L][n] of every problem live in the ctx's scratch; a problem given as a row list first gathers its rows into a
// contiguous float32 copy there, so every later pass reads contiguous memory.  The L candidate rows sit in LDS as doubles; a wave stages 64
// rows at a time through LDS (coalesced loads, odd row stride: conflict-free per-lane reads), so D <= KPP_MAX_D = 64.
#include "common.hpp"

#include <cmath>

using namespace ssp;

namespace {

constexpr int KPP_T = 512, KPP_NW = KPP_T / 64, KPP_MAX_D = 64, KPP_LT_MAX = 8, KPP_MAX_L = 24;

struct KppProb {
    int64_t row_off;   // first row (ranges) or first entry of sel (lists)
    int64_t work_off;  // doubles into the work buffer: d2[n], then dc[L][n]
    int32_t n, first;
};

struct KppArgs {
    const float* x;
    const int64_t* sel;  // null: ranges
    const KppProb* prob;
    const double* u;     // [P][K-1][L]
    double* work;
    int32_t* seed_pos;   // [P][K]
    int32_t* flag;       // [P]
    double* centres;     // [P][K][D] or null
    int32_t K, D, L;
};

// the LT candidate rows cand[l0 ..) -> cd[LT][Dp] as doubles (slots past nl and the pad column: zero)
template <int LT>
__device__ __forceinline__ void kpp_load_cands(const float* xs, int D, const int* cand, int l0, int nl, int Dp, double* cd) {
    for (int e = threadIdx.x; e < LT * Dp; e += KPP_T) {
        const int j = e / Dp, d = e - j * Dp;
        double v = 0.0;
        if (j < nl && d < D) v = (double)xs[(int64_t)cand[l0 + j] * D + d];
        cd[e] = v;
    }
}

// A wave's 64-row tile, 64 x D floats contiguous in xs from row r0, into its LDS image [64][S]: lane + 64 t is element t of a lane,
// sixteen loads in flight at a time.  An element past the problem's last row re-reads the last float (staged, never used).
__device__ __forceinline__ void kpp_stage(const float* xs, int D, int n, int64_t r0, int lane, float* tile, int S) {
    const int64_t left = (int64_t)n - r0;
    if (left <= 0) return;  // (wave-uniform)
    const int cnt = (int)(left < 64 ? left : 64) * D, qd = 64 / D, rd = 64 % D;
    const float* src = xs + r0 * D;
    int r = lane / D, d = lane - r * D;
    for (int t0 = 0; t0 < D; t0 += 16) {
        float v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = lane + 64 * (t0 + q);
            v[q] = src[e < cnt ? e : cnt - 1];
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (t0 + q < D) tile[r * S + d] = v[q];
            r += qd;
            d += rd;
            if (d >= D) {
                d -= D;
                ++r;
            }
        }
    }
}

// One pass over the rows (xs: n x D, contiguous) against LT candidates in cd.  init: d2[i] = |x_i - cd[0]|^2.  Otherwise dc[l0 + j][i] = |x_i - cd[j]|^2 and
// pot[j] += min(d2[i], dc) for j < nl.  Every thread of the workgroup must call it (block barriers inside); it ends with a barrier.
template <int LT>
__device__ __forceinline__ void kpp_dist_pass(const float* xs, int D, int n, int l0, int nl, bool init, const double* cd, float* tile, int S,
                                              int Dp, double* d2, double* dc, double (&pot)[LT]) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t ntiles = ((int64_t)n + 63) / 64, iters = (ntiles + KPP_NW - 1) / KPP_NW;
#pragma unroll
    for (int j = 0; j < LT; ++j) pot[j] = 0.0;
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t r0 = (it * KPP_NW + w) * 64, i = r0 + lane;
        const bool live = i < n;
        const double d2i = (live && !init) ? d2[i] : 0.0;
        __syncthreads();  // the tile's last readers are done (first trip: cd is written)
        kpp_stage(xs, D, n, r0, lane, tile, S);
        __syncthreads();
        if (live) {
            double acc0[LT], acc1[LT];
#pragma unroll
            for (int j = 0; j < LT; ++j) acc0[j] = acc1[j] = 0.0;
            const float* xr = tile + lane * S;
#pragma unroll 2
            for (int d = 0; d < Dp; d += 2) {  // (column D of the tile and of cd is zero when D is odd)
                const double x0 = (double)xr[d], x1 = (double)xr[d + 1];
#pragma unroll
                for (int j = 0; j < LT; ++j) {
                    const double2 c = *reinterpret_cast<const double2*>(cd + j * Dp + d);
                    const double e0 = x0 - c.x, e1 = x1 - c.y;
                    acc0[j] = fma(e0, e0, acc0[j]);
                    acc1[j] = fma(e1, e1, acc1[j]);
                }
            }
            if (init) {
                d2[i] = acc0[0] + acc1[0];
            } else {
#pragma unroll
                for (int j = 0; j < LT; ++j)
                    if (j < nl) {
                        const double v = acc0[j] + acc1[j];
                        dc[(int64_t)(l0 + j) * n + i] = v;
                        pot[j] += fmin(d2i, v);
                    }
            }
        }
    }
    __syncthreads();
}

template <int LT>
__global__ __launch_bounds__(KPP_T) void kmeanspp_kernel(KppArgs a) {
    extern __shared__ __attribute__((aligned(16))) double kpp_lds[];
    __shared__ double s_lane[KPP_T];            // lane totals, then the lanes' exclusive offsets inside their wave
    __shared__ double s_wave[KPP_NW + 1];       // wave totals, then the waves' exclusive offsets; [KPP_NW] = total
    __shared__ double s_wpot[KPP_NW][KPP_LT_MAX];
    __shared__ double s_pot[KPP_MAX_L];
    __shared__ int s_cnt[KPP_MAX_L], s_cand[KPP_MAX_L], s_pick[2];

    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const KppProb pb = a.prob[p];
    const int n = pb.n, K = a.K, D = a.D, L = a.L;
    const int Dp = (D + 1) & ~1, S = Dp + 1;
    double* cd = kpp_lds;                                                      // [LT][Dp]
    float* tile = reinterpret_cast<float*>(kpp_lds + LT * Dp) + (size_t)w * 64 * S;  // [64][S] of this wave
    double* d2 = a.work + pb.work_off;
    double* dc = d2 + n;
    int32_t* seeds = a.seed_pos + (int64_t)p * K;
    const double* u = a.u + (int64_t)p * (K - 1) * L;
    double pot[LT];

    for (int e = lane; e < 64 * S; e += 64) tile[e] = 0.f;  // (the pad column stays zero: staging writes d < D only)
    if (tid == 0) {
        s_cand[0] = pb.first;
        seeds[0] = pb.first;
        a.flag[p] = 0;
    }
    const float* xs = a.x + pb.row_off * D;  // the problem's rows, contiguous
    if (a.sel) {  // a list: gather the rows once, eight per wave and trip (one lane per column)
        float* xc = reinterpret_cast<float*>(dc + (int64_t)L * n);
        const int64_t* sel = a.sel + pb.row_off;
        for (int64_t i0 = (int64_t)w * 8; i0 < n; i0 += 8 * KPP_NW) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = (i0 + q < n && lane < D) ? a.x[sel[i0 + q] * D + lane] : 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (i0 + q < n && lane < D) xc[(i0 + q) * D + lane] = v[q];
        }
        xs = xc;
    }
    __syncthreads();
    kpp_load_cands<LT>(xs, D, s_cand, 0, 1, Dp, cd);
    kpp_dist_pass<LT>(xs, D, n, 0, 1, true, cd, tile, S, Dp, d2, dc, pot);

    const int C = (int)(((int64_t)n + KPP_T - 1) / KPP_T);  // rows per lane of the prefix sum
    const int64_t c0 = (int64_t)tid * C;
    const int cn = (int)(c0 >= n ? 0 : (n - c0 < C ? n - c0 : C));
    for (int k = 1; k < K; ++k) {
        // ---- cum, level 1: this lane's chunk
        double run = 0.0;
        for (int j0 = 0; j0 < cn; j0 += 8) {  // (eight loads in flight; the padding adds +0.0, which changes nothing)
            double t[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = j0 + q < cn ? d2[c0 + j0 + q] : 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) run += t[q];
        }
        s_lane[tid] = run;
        if (tid < KPP_MAX_L) s_cnt[tid] = 0;
        __syncthreads();
        if (lane == 0) {  // level 2: the 64 lanes of this wave, left to right
            double o = 0.0;
            for (int j = 0; j < 64; ++j) {
                const double t = s_lane[w * 64 + j];
                s_lane[w * 64 + j] = o;
                o += t;
            }
            s_wave[w] = o;
        }
        __syncthreads();
        if (tid == 0) {  // level 3: the waves
            double o = 0.0;
            for (int j = 0; j < KPP_NW; ++j) {
                const double t = s_wave[j];
                s_wave[j] = o;
                o += t;
            }
            s_wave[KPP_NW] = o;
        }
        __syncthreads();
        const double total = s_wave[KPP_NW];
        if (!(fabs(total) <= 1.7976931348623157e308)) {  // NaN or infinite (uniform: every thread reads the same word)
            if (tid == 0) a.flag[p] = 1;
            return;
        }
        // ---- candidates: #{i : cum[i] < u * total}, eight thresholds at a time
        const double woff = s_wave[w], loff = s_lane[tid];
        for (int l0 = 0; l0 < L; l0 += 8) {
            double v[8];
            int cnt[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                v[j] = l0 + j < L ? u[(int64_t)(k - 1) * L + l0 + j] * total : -1.0;
                cnt[j] = 0;
            }
            run = 0.0;
            for (int j0 = 0; j0 < cn; j0 += 8) {
                double t[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) t[q] = j0 + q < cn ? d2[c0 + j0 + q] : 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    run += t[q];
                    const double cum = woff + (loff + run);
                    const bool in = j0 + q < cn;
#pragma unroll
                    for (int m = 0; m < 8; ++m) cnt[m] += (in && cum < v[m]) ? 1 : 0;
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                int c = cnt[q];
                for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
                if (lane == 0 && l0 + q < L && c) atomicAdd(&s_cnt[l0 + q], c);
            }
        }
        __syncthreads();
        if (tid < L) s_cand[tid] = s_cnt[tid] < n - 1 ? s_cnt[tid] : n - 1;
        __syncthreads();
        // ---- distances to the candidates and the potentials, LT candidates per pass
        for (int l0 = 0; l0 < L; l0 += LT) {
            const int nl = L - l0 < LT ? L - l0 : LT;
            kpp_load_cands<LT>(xs, D, s_cand, l0, nl, Dp, cd);
            kpp_dist_pass<LT>(xs, D, n, l0, nl, false, cd, tile, S, Dp, d2, dc, pot);
#pragma unroll
            for (int j = 0; j < LT; ++j) {
                double s = pot[j];
                for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
                if (lane == 0) s_wpot[w][j] = s;
            }
            __syncthreads();
            if (tid < nl) {
                double s = 0.0;
                for (int j = 0; j < KPP_NW; ++j) s += s_wpot[j][tid];
                s_pot[l0 + tid] = s;
            }
            __syncthreads();
        }
        if (tid == 0) {  // first arg-min
            int b = 0;
            for (int l = 1; l < L; ++l)
                if (s_pot[l] < s_pot[b]) b = l;
            s_pick[0] = b;
            seeds[k] = s_cand[b];
        }
        __syncthreads();
        if (k + 1 < K) {
            const double* dcb = dc + (int64_t)s_pick[0] * n;
            for (int64_t i0 = tid; i0 < n; i0 += 4 * KPP_T) {  // (four rows per trip: d2 and dc share a buffer, so the loads are batched by hand)
                double o[4], c[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t i = i0 + q * KPP_T;
                    o[q] = i < n ? d2[i] : 0.0;
                    c[q] = i < n ? dcb[i] : 0.0;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (i0 + q * KPP_T < n) d2[i0 + q * KPP_T] = fmin(o[q], c[q]);
            }
        }
        __syncthreads();
    }
    if (a.centres) {
        __syncthreads();  // seeds[] of thread 0 (K = 1: no step ran)
        double* out = a.centres + (int64_t)p * K * D;
        for (int64_t e = tid; e < (int64_t)K * D; e += KPP_T) {
            const int k = (int)(e / D), d = (int)(e - (int64_t)k * D);
            out[e] = (double)xs[(int64_t)seeds[k] * D + d];
        }
    }
}

size_t kpp_lds_bytes(int LT, int D) {
    const int Dp = (D + 1) & ~1, S = Dp + 1;
    return (size_t)LT * Dp * sizeof(double) + (size_t)KPP_NW * 64 * S * sizeof(float);
}

template <int LT>
int kpp_launch(const KppArgs& a, int P, hipStream_t s) {
    const size_t lds = kpp_lds_bytes(LT, a.D);
    if (lds > 64 * 1024)
        SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kmeanspp_kernel<LT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kmeanspp_kernel<LT>, dim3((unsigned)P), dim3(KPP_T), lds, s, a);
    return SSP_OK;
}

}  // namespace

extern "C" int ssp_kmeanspp_seed(ssp_ctx* ctx, int32_t P, int32_t K, int32_t D, const float* feats, int64_t n_rows, int where,
                                 const int64_t* row_off, const int64_t* n_sel, const int64_t* sel, const int64_t* first, const double* u,
                                 int64_t* seed_rows_out, double* centres_out, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_kmeanspp_seed");
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (P < 1 || K < 1 || D < 1 || !row_off || !n_sel || !first || !seed_rows_out || (K > 1 && !u))
        SSP_FAIL(SSP_ERR_INVALID, "ssp_kmeanspp_seed: bad shape or null array");
    if (D > KPP_MAX_D) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_kmeanspp_seed: D=%d exceeds the kernel's feature dimension (%d)", D, KPP_MAX_D);
    if (n_rows < 1 || !feats) SSP_FAIL(SSP_ERR_INVALID, "ssp_kmeanspp_seed: no rows");
    SSP_TRY(check_where(where, "ssp_kmeanspp_seed"));
    const int L = 2 + (int)std::log((double)K);  // candidates per step: 2 + int(ln K), as _kmeanspp and sklearn draw them
    if (L > KPP_MAX_L) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_kmeanspp_seed: K=%d gives more than %d candidates per step", K, KPP_MAX_L);
    int64_t sel_total = 0, work_total = 0;
    std::vector<KppProb> pr(P);
    for (int p = 0; p < P; ++p) {
        const int64_t n = n_sel[p], off = row_off[p];
        if (n < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_kmeanspp_seed: problem %d has no rows", p);
        if (n > INT32_MAX - 64 * KPP_NW) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_kmeanspp_seed: problem %d has too many rows", p);
        if (sel) {
            if (off < 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_kmeanspp_seed: problem %d: negative offset into sel", p);
            for (int64_t i = 0; i < n; ++i)
                if (sel[off + i] < 0 || sel[off + i] >= n_rows)
                    SSP_FAIL(SSP_ERR_INVALID, "ssp_kmeanspp_seed: problem %d: row %lld (entry %lld of its list) outside the %lld feature rows", p,
                             (long long)sel[off + i], (long long)i, (long long)n_rows);
            sel_total = std::max(sel_total, off + n);
        } else if (off < 0 || off > n_rows - n) {
            SSP_FAIL(SSP_ERR_INVALID, "ssp_kmeanspp_seed: problem %d: rows [%lld, %lld) outside the %lld feature rows", p, (long long)off,
                     (long long)(off + n), (long long)n_rows);
        }
        if (first[p] < 0 || first[p] >= n)
            SSP_FAIL(SSP_ERR_INVALID, "ssp_kmeanspp_seed: problem %d: first centre %lld outside its %lld rows", p, (long long)first[p], (long long)n);
        const double* up = u + (size_t)p * (K - 1) * L;
        for (int64_t i = 0; i < (int64_t)(K - 1) * L; ++i)
            if (!(up[i] >= 0.0 && up[i] < 1.0))
                SSP_FAIL(SSP_ERR_INVALID, "ssp_kmeanspp_seed: problem %d: draw %lld (%g) outside [0, 1)", p, (long long)i, up[i]);
        pr[p] = KppProb{off, work_total, (int32_t)n, (int32_t)first[p]};
        work_total += n * (1 + (int64_t)L) + (sel ? (n * D + 1) / 2 : 0);  // d2, dc, and a list's gathered float32 rows
    }
    hipStream_t s = ctx->stream;
    DevBuf &d_work = ctx->scratch[0], &d_tab = ctx->scratch[1], &d_out = ctx->scratch[2];
    StageScope st(ctx, where);
    const float* d_x = st.in(feats, (size_t)n_rows * D * sizeof(float));
    SSP_TRY(st.status());
    // one table upload: the draws, the lists, the problems (8-byte entries first)
    const size_t n_u = (size_t)P * (K - 1) * L, b_u = n_u * sizeof(double), b_sel = (size_t)sel_total * sizeof(int64_t), b_pr = (size_t)P * sizeof(KppProb);
    std::vector<char> tab(b_u + b_sel + b_pr);
    if (b_u) memcpy(tab.data(), u, b_u);
    if (b_sel) memcpy(tab.data() + b_u, sel, b_sel);
    memcpy(tab.data() + b_u + b_sel, pr.data(), b_pr);
    // outputs: centres (doubles) first, then positions and flags
    const size_t b_cen = centres_out ? (size_t)P * K * D * sizeof(double) : 0, b_pos = (size_t)P * K * sizeof(int32_t), b_flag = (size_t)P * sizeof(int32_t);
    SSP_TRY(d_work.reserve((size_t)work_total * sizeof(double)));
    SSP_TRY(d_tab.reserve(tab.size()));
    SSP_TRY(d_out.reserve(b_cen + b_pos + b_flag));
    SSP_HIP(hipMemcpyAsync(d_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, s));
    KppArgs a;
    a.x = d_x;
    a.u = (const double*)d_tab.p;
    a.sel = sel ? (const int64_t*)((char*)d_tab.p + b_u) : nullptr;
    a.prob = (const KppProb*)((char*)d_tab.p + b_u + b_sel);
    a.work = d_work.as<double>();
    a.centres = centres_out ? d_out.as<double>() : nullptr;
    a.seed_pos = (int32_t*)((char*)d_out.p + b_cen);
    a.flag = (int32_t*)((char*)d_out.p + b_cen + b_pos);
    a.K = K;
    a.D = D;
    a.L = L;
    Timer tm;
    int rc = tm.start(kernel_ms != nullptr, s);
    if (rc == SSP_OK) {
        switch (std::min(L, KPP_LT_MAX)) {
            case 2: rc = kpp_launch<2>(a, P, s); break;
            case 3: rc = kpp_launch<3>(a, P, s); break;
            case 4: rc = kpp_launch<4>(a, P, s); break;
            case 5: rc = kpp_launch<5>(a, P, s); break;
            case 6: rc = kpp_launch<6>(a, P, s); break;
            case 7: rc = kpp_launch<7>(a, P, s); break;
            default: rc = kpp_launch<8>(a, P, s); break;
        }
        if (rc == SSP_OK && hipGetLastError() != hipSuccess) {
            set_error("ssp_kmeanspp_seed: kernel launch failed");
            rc = SSP_ERR_HIP;
        }
    }
    if (rc == SSP_OK) rc = tm.stop(s, kernel_ms);
    if (rc != SSP_OK) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    std::vector<char> host(b_cen + b_pos + b_flag);
    hipError_t he = hipMemcpyAsync(host.data(), d_out.p, host.size(), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) SSP_FAIL(SSP_ERR_HIP, "ssp_kmeanspp_seed: result copy failed: %s", hipGetErrorString(he));
    const int32_t* pos = (const int32_t*)(host.data() + b_cen);
    const int32_t* flag = (const int32_t*)(host.data() + b_cen + b_pos);
    for (int p = 0; p < P; ++p)
        if (flag[p])
            SSP_FAIL(SSP_ERR_INVALID, "ssp_kmeanspp_seed: problem %d: the sum of squared distances is not finite (NaN or infinite rows)", p);
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < K; ++k) {
            const int64_t i = pos[(size_t)p * K + k];
            seed_rows_out[(size_t)p * K + k] = sel ? sel[row_off[p] + i] : row_off[p] + i;
        }
    if (centres_out) memcpy(centres_out, host.data(), b_cen);
    return SSP_OK;
}
