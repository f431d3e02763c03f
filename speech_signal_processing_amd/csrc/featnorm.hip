// Sliding-window feature normalisation and speech-frame selection on gfx950 (ssp_featnorm_sliding, ssp_select_frames,
// ssp_featnorm_table): what stands between the feature extractors and the models of a verification or diarization chain.  An extension:
// the reference scales once per utterance (GMM_UBM.py:93); Kaldi's apply-cmvn-sliding, sidekit's cep_sliding_norm / stg and Pelecanos and
// Sridharan's feature warping are the counterparts (recalled, parity unpinned).  include/ssp.h has the definitions,
// tests/featnorm_oracle.py restates them in float64.
// Kernels:
//   fn_scan_kernel         one workgroup: exclusive prefix over the utterances of the batch, of their tile counts (the sliding kernel's
//                          tile -> utterance map) or of their kept rows (the selection's output bases); entry n holds the total
//   fn_sliding_kernel      a workgroup takes FN_TILE consecutive frames of ONE utterance and FN_COLS columns.  LDS holds, column by
//                          column, every row a window of the tile reaches (at most FN_TILE + window - 1 rows).  Lanes run along frames:
//                          a wave walks the union of its 64 windows once, every window value is one broadcast LDS read for the wave,
//                          and a lane counts it only while the row lies in its own window.  The rows that lie in ALL 64 windows (the
//                          core: window - 63 of window + 63 rows) run without that test, and tiles without a NaN without the NaN count.
//                          MODE 2 counts {x_s < x_t} and {x_s == x_t} — integers, exact — and looks phi^-1 up (row n = window of the
//                          table from LDS, other rows from global memory).  MODE 0 / 1 sum x_s and x_s^2 in float64 (exact products,
//                          no overflow; the error does not depend on the utterance's length because nothing is carried from frame
//                          to frame).
//   fn_select_count_kernel one workgroup per utterance: its kept rows
//   fn_select_copy_kernel  workgroups (utterance, slice) walk the utterance's 256-row chunks, slice by slice; the kept rows in front of
//                          a chunk are counted from the mask (1 byte a row against 4 dim copied), a chunk's destinations come from wave
//                          ballots, the rows are copied as 32-bit words by the whole workgroup.  No atomics anywhere.
#include <algorithm>
#include <cmath>
#include <memory>
#include <type_traits>

#include "common.hpp"

#pragma clang fp contract(off)

namespace ssp {

constexpr int FN_TILE = SSP_FEATNORM_TILE;  // frames per workgroup of the sliding kernel (= its threads)
constexpr int FN_COLS = 8;           // columns per workgroup
constexpr int FN_MAX_WINDOW = 1024;
constexpr int FN_MAX_DIM = 4096;
constexpr int FN_SEL_SLICES = 64;    // most workgroups that share one utterance in the copy kernel

// the device copies of the warping tables of a ctx (a few windows: callers alternate between two or three) and its work buffers
struct FnTable {
    int window = 0;
    DevBuf dev;
    std::vector<float> host;  // stays alive: the upload is asynchronous
};
struct FeatnormState {
    std::vector<std::unique_ptr<FnTable>> tabs;
    DevBuf tiles;   // int64[n + 1] tile prefix of the sliding kernel
    DevBuf sel;     // int64[n] kept rows, int64[n + 1] their prefix
};
constexpr size_t FN_TABLES_KEPT = 6;

void featnorm_release(ssp_ctx* ctx) {
    delete static_cast<FeatnormState*>(ctx->featnorm);
    ctx->featnorm = nullptr;
}

static int fn_state(ssp_ctx* ctx, FeatnormState** out) {
    if (!ctx->featnorm) {
        ctx->featnorm = new (std::nothrow) FeatnormState;
        if (!ctx->featnorm) SSP_FAIL(SSP_ERR_NOMEM, "featnorm: host alloc");
    }
    *out = static_cast<FeatnormState*>(ctx->featnorm);
    return SSP_OK;
}

// phi^-1(p) for 0 < p < 0.5 in double: Halley steps on Phi(x) - p (std::erfc) inside a bracket that every step narrows
static double fn_inv_phi_lower(double p) {
    const double SQRT1_2 = 0.70710678118654752440, INV_SQRT_2PI = 0.39894228040143267794;
    double lo = -std::sqrt(-2.0 * std::log(2.0 * p));  // Phi(x) <= exp(-x^2 / 2) / 2 for x <= 0: Phi(lo) <= p
    double hi = 0.0;                                     // Phi(0) = 1/2 > p
    double x = lo;
    for (int it = 0; it < 200; ++it) {
        const double f = 0.5 * std::erfc(-x * SQRT1_2) - p;
        if (f == 0.0) break;
        if (f < 0.0) lo = x;
        else hi = x;
        const double d = INV_SQRT_2PI * std::exp(-0.5 * x * x);
        const double r = f / d;
        double xn = x - r / (1.0 + 0.5 * x * r);
        if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
        const bool done = std::fabs(xn - x) <= 2e-16 * std::fabs(xn);
        x = xn;
        if (done) break;
    }
    return x;
}

// row n (1 <= n <= window) at offset (n - 1)^2: float(phi^-1(k / 2n)), k = 1 .. 2n - 1
static void fn_fill_table(int window, float* t) {
    for (int n = 1; n <= window; ++n) {
        float* row = t + (size_t)(n - 1) * (n - 1);
        row[n - 1] = 0.0f;
        for (int k = 1; k < n; ++k) {
            const float v = (float)fn_inv_phi_lower((double)k / (2.0 * n));
            row[k - 1] = v;
            row[2 * n - k - 1] = -v;
        }
    }
}

static int fn_table(ssp_ctx* ctx, FeatnormState* st, int window, const float** dev) {
    for (size_t i = 0; i < st->tabs.size(); ++i)
        if (st->tabs[i]->window == window) {
            std::rotate(st->tabs.begin() + i, st->tabs.begin() + i + 1, st->tabs.end());  // most recently used last
            *dev = st->tabs.back()->dev.as<float>();
            return SSP_OK;
        }
    if (st->tabs.size() >= FN_TABLES_KEPT) {
        SSP_HIP(hipStreamSynchronize(ctx->stream));  // the oldest table may still be read, or still be on its way up
        st->tabs.erase(st->tabs.begin());
    }
    std::unique_ptr<FnTable> t(new (std::nothrow) FnTable);
    if (!t) SSP_FAIL(SSP_ERR_NOMEM, "featnorm: host alloc");
    const size_t n = (size_t)window * window;
    t->window = window;
    t->host.resize(n);
    fn_fill_table(window, t->host.data());
    SSP_TRY(t->dev.alloc(n * sizeof(float)));
    SSP_HIP(hipMemcpyAsync(t->dev.p, t->host.data(), n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    *dev = t->dev.as<float>();
    st->tabs.push_back(std::move(t));
    return SSP_OK;
}

// the window of frame t of an utterance of T frames: centred, slid back inside the utterance (include/ssp.h)
__host__ __device__ __forceinline__ int64_t fn_window_lo(int64_t t, int64_t T, int W) {
    int64_t lo = t - W / 2, hi = lo + W;
    if (lo < 0) {
        hi -= lo;
        lo = 0;
    }
    if (hi > T) {
        lo -= hi - T;
        lo = lo < 0 ? 0 : lo;
    }
    return lo;
}

__device__ __forceinline__ int fn_find(const int64_t* __restrict__ pre, int n, int64_t v) {  // the last u with pre[u] <= v
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// out[u] = sum of value(0 .. u - 1), out[n] = the total; value(u) = counts[u], or without counts the tiles of utterance u
__global__ __launch_bounds__(256) void fn_scan_kernel(const int64_t* __restrict__ off, const int64_t* __restrict__ counts, int64_t n, int tile,
                                                      int64_t* __restrict__ out) {
    __shared__ int64_t part[256];
    const int tid = threadIdx.x;
    const int64_t chunk = (n + 255) / 256, b = min<int64_t>(n, tid * chunk), e = min<int64_t>(n, b + chunk);
    auto value = [&](int64_t u) { return counts ? counts[u] : (off[u + 1] - off[u] + tile - 1) / tile; };
    int64_t s = 0;
    for (int64_t u = b; u < e; ++u) s += value(u);
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int i = 0; i < 256; ++i) {
            const int64_t v = part[i];
            part[i] = run;
            run += v;
        }
        out[n] = run;
    }
    __syncthreads();
    int64_t run = part[tid];
    for (int64_t u = b; u < e; ++u) {
        out[u] = run;
        run += value(u);
    }
}

struct SlidingArgs {
    const float* in;           // row row0 of the caller's matrix
    float* out;
    const int64_t* off;        // [n_utt + 1] frame offsets
    const int64_t* tile_pre;   // [n_utt + 1] tiles in front of each utterance
    const float* tab;          // warping table of `window` (MODE 2)
    int64_t row0;
    int32_t n_utt, dim, window, stride;  // stride: floats between the columns of the LDS image
};

template <int MODE>
__global__ __launch_bounds__(FN_TILE, 4) void fn_sliding_kernel(SlidingArgs a) {
    extern __shared__ __attribute__((aligned(16))) char fn_smem[];
    float* xs = reinterpret_cast<float*>(fn_smem);   // [FN_COLS][stride]
    float* trow = xs + FN_COLS * a.stride;           // [2 window - 1] row n = window of the table (MODE 2)
    const int tid = threadIdx.x, W = a.window, dim = a.dim, NR = a.stride;
    const int u = fn_find(a.tile_pre, a.n_utt, (int64_t)blockIdx.x);
    const int64_t ua = a.off[u], T = a.off[u + 1] - ua;
    const int64_t t0 = ((int64_t)blockIdx.x - a.tile_pre[u]) * FN_TILE;
    const int nt = (int)min<int64_t>(FN_TILE, T - t0);          // frames of this tile, >= 1
    const int cnt = (int)min<int64_t>(W, T);                    // frames of every window of this utterance
    const int64_t rlo = fn_window_lo(t0, T, W);                 // first row any window of the tile reaches
    const int nrows = (int)(fn_window_lo(t0 + nt - 1, T, W) + cnt - rlo);  // <= FN_TILE + W - 1
    const int c0 = blockIdx.y * FN_COLS, nc = min(FN_COLS, dim - c0);
    const float* src = a.in + (ua - a.row0 + rlo) * dim + c0;
    bool nan_here = false;
    for (int i = tid; i < nrows * FN_COLS; i += FN_TILE) {
        const int r = i / FN_COLS, c = i % FN_COLS;
        const float v = c < nc ? src[(int64_t)r * dim + c] : 0.f;
        nan_here = nan_here || v != v;
        xs[c * NR + r] = v;
    }
    if (MODE == 2 && cnt == W)
        for (int i = tid; i < 2 * W - 1; i += FN_TILE) trow[i] = a.tab[(size_t)(W - 1) * (W - 1) + i];
    const bool nans = __syncthreads_or(nan_here) != 0;
    const int wave0 = __builtin_amdgcn_readfirstlane(tid & ~63);
    if (wave0 >= nt) return;  // (no barrier below)
    const bool active = tid < nt;
    const int64_t t = t0 + min(tid, nt - 1);
    const int me = (int)(t - rlo);                               // this lane's frame in the image
    const int lo = (int)(fn_window_lo(t, T, W) - rlo);           // its window: rows [lo, lo + cnt) of the image
    // the union of the wave's windows [wlo, whi) and the rows all of them hold [clo, chi)
    const int64_t tf = t0 + wave0, tl = t0 + min(wave0 + 63, nt - 1);
    const int wlo = (int)(fn_window_lo(tf, T, W) - rlo), clo = (int)(fn_window_lo(tl, T, W) - rlo);
    const int chi = wlo + cnt, whi = clo + cnt;
    const int b1 = clo < chi ? clo : whi, b2 = clo < chi ? chi : whi;  // [wlo, b1) tested, [b1, b2) core, [b2, whi) tested
    float* dst = a.out + (ua - a.row0 + t) * dim + c0;
#pragma unroll 1  // (one copy of the six walks, not eight: the kernel stays inside the instruction cache)
    for (int c = 0; c < nc; ++c) {
        const float* col = xs + c * NR;
        const float x = col[me];
        float y;
        if (MODE == 2) {
            int lt = 0, eq = 0, n = 0;  // a NaN window value is below nothing and equal to nothing
            auto walk = [&](int s0, int s1, auto tested, auto count_nan) {
#pragma unroll 4
                for (int s = s0; s < s1; ++s) {
                    const float v = col[s];
                    const bool in = !tested.value || (unsigned)(s - lo) < (unsigned)cnt;
                    lt += (in && v < x) ? 1 : 0;
                    eq += (in && v == x) ? 1 : 0;
                    if (count_nan.value) n += (in && v == v) ? 1 : 0;
                }
            };
            using std::false_type;
            using std::true_type;
            if (nans) {
                walk(wlo, b1, true_type{}, true_type{});
                walk(b1, b2, false_type{}, true_type{});
                walk(b2, whi, true_type{}, true_type{});
            } else {
                walk(wlo, b1, true_type{}, false_type{});
                walk(b1, b2, false_type{}, false_type{});
                walk(b2, whi, true_type{}, false_type{});
                n = cnt;
            }
            const int k = 2 * lt + eq;  // 1 <= k <= 2 n - 1 unless x is NaN
            float r = __builtin_nanf("");
            if (x == x) r = n == W ? trow[k - 1] : a.tab[(size_t)(n - 1) * (n - 1) + (k - 1)];
            y = r;
        } else {
            double s1 = 0.0, s2 = 0.0;
            int n = 0;
            auto walk = [&](int s0, int s1_, auto tested, auto skip_nan) {
#pragma unroll 4
                for (int s = s0; s < s1_; ++s) {
                    const float v = col[s];
                    bool in = !tested.value || (unsigned)(s - lo) < (unsigned)cnt;
                    if (skip_nan.value) in = in && v == v;
                    const double d = in ? (double)v : 0.0;
                    s1 += d;
                    if (MODE == 1) s2 = fma(d, d, s2);
                    if (skip_nan.value) n += in ? 1 : 0;
                }
            };
            using std::false_type;
            using std::true_type;
            if (nans) {
                walk(wlo, b1, true_type{}, true_type{});
                walk(b1, b2, false_type{}, true_type{});
                walk(b2, whi, true_type{}, true_type{});
            } else {
                walk(wlo, b1, true_type{}, false_type{});
                walk(b1, b2, false_type{}, false_type{});
                walk(b2, whi, true_type{}, false_type{});
                n = cnt;
            }
            // float64 sums of float32 entries: the one-pass variance loses (a / s)^2 2^-53 of itself, far inside the band at any a / s
            // float32 data can hold, and a square cannot overflow
            const double md = s1 / (double)n;  // (no entry: NaN)
            double r = (double)x - md;
            if (MODE == 1) {
                double var = s2 / (double)n - md * md;
                var = var < 0.0 ? 0.0 : var;      // (a NaN stays)
                double sd = sqrt(var);
                if (sd < 10.0 * 1.1920928955078125e-07) sd = 1.0;  // cmvn_kernel's rule
                r = r / sd;
            }
            y = x == x ? (float)r : __builtin_nanf("");
        }
        if (active) dst[c] = y;  // (the eight stores of a lane fill one 32-byte piece of its row)
    }
}

__device__ __forceinline__ int fn_block_sum(int v, int* wsum) {  // the same total in every thread of a 256-thread workgroup
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();  // (wsum's last readers are done)
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    return wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(256) void fn_select_count_kernel(const uint8_t* __restrict__ mask, const int64_t* __restrict__ off, int64_t row0,
                                                              int64_t* __restrict__ counts) {
    __shared__ int wsum[4];
    const int u = blockIdx.x;
    const int64_t a = off[u], T = off[u + 1] - a;
    const uint8_t* m = mask + (a - row0);
    int64_t total = 0;
    for (int64_t b = 0; b < T; b += (int64_t)256 * 4096) {  // (pieces whose count fits an int)
        const int64_t e = min<int64_t>(T, b + (int64_t)256 * 4096);
        int c = 0;
        for (int64_t r = b + threadIdx.x; r < e; r += 256) c += m[r] != 0 ? 1 : 0;
        total += fn_block_sum(c, wsum);
    }
    if (threadIdx.x == 0) counts[u] = total;
}

__global__ __launch_bounds__(256) void fn_select_copy_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                             const uint8_t* __restrict__ mask, const int64_t* __restrict__ off,
                                                             const int64_t* __restrict__ base, int dim, int64_t row0) {
    __shared__ int wsum[4];
    __shared__ int dst[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int u = blockIdx.x;
    const int64_t a = off[u], T = off[u + 1] - a;
    const int64_t n_chunks = (T + 255) / 256;
    const uint8_t* m = mask + (a - row0);
    const uint32_t* src = in + (a - row0) * dim;
    int64_t run = base[u];   // kept rows of the batch in front of row `seen` of this utterance
    int64_t seen = 0;
    for (int64_t ch = blockIdx.y; ch < n_chunks; ch += gridDim.y) {
        int c = 0;
        for (int64_t r = seen + tid; r < ch * 256; r += 256) c += m[r] != 0 ? 1 : 0;  // (at most FN_SEL_SLICES chunks)
        run += fn_block_sum(c, wsum);
        const int64_t r = ch * 256 + tid;
        const bool keep = r < T && m[r] != 0;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(keep);
        const int before = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) wsum[wave] = __builtin_popcountll(bal);
        __syncthreads();
        int wbase = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            wbase += w < wave ? wsum[w] : 0;
            total += wsum[w];
        }
        dst[tid] = keep ? wbase + before : -1;
        __syncthreads();
        const int rows = (int)min<int64_t>(256, T - ch * 256);
        const uint32_t* s = src + ch * 256 * dim;
        for (int i = tid; i < rows * dim; i += 256) {
            const int rr = i / dim, d = i - rr * dim;
            const int to = dst[rr];
            if (to >= 0) out[(run + to) * dim + d] = s[i];
        }
        run += total;
        seen = ch * 256 + rows;
    }
}

}  // namespace ssp

using namespace ssp;

extern "C" {

int ssp_featnorm_table(int32_t window, float* table_out) {
    if (window < 1 || window > FN_MAX_WINDOW) SSP_FAIL(SSP_ERR_INVALID, "ssp_featnorm_table: window=%d outside [1, %d]", window, FN_MAX_WINDOW);
    if (!table_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_featnorm_table: null table_out");
    fn_fill_table(window, table_out);
    return SSP_OK;
}

int ssp_featnorm_sliding(ssp_ctx* ctx, const float* feats, const ssp_segments* frame_seg, int32_t dim, int32_t window, int32_t mode, float* out,
                         int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_featnorm_sliding");
    if (!ctx) SSP_FAIL(SSP_ERR_INVALID, "null ssp_ctx");
    if (!frame_seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_featnorm_sliding: null segments");
    if (dim < 1 || dim > FN_MAX_DIM) SSP_FAIL(SSP_ERR_INVALID, "ssp_featnorm_sliding: dim=%d outside [1, %d]", dim, FN_MAX_DIM);
    if (window < 1 || window > FN_MAX_WINDOW) SSP_FAIL(SSP_ERR_INVALID, "ssp_featnorm_sliding: window=%d outside [1, %d]", window, FN_MAX_WINDOW);
    if (mode < 0 || mode > 2) SSP_FAIL(SSP_ERR_INVALID, "ssp_featnorm_sliding: mode=%d", mode);
    SSP_TRY(check_where(where, "ssp_featnorm_sliding"));
    if (feats && out == feats) SSP_FAIL(SSP_ERR_INVALID, "ssp_featnorm_sliding: out == feats (tiles read their neighbours' rows)");
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    const int64_t n = frame_seg->n, rows = frame_seg->total();
    if (rows == 0 || n == 0) return SSP_OK;
    if (!feats || !out) SSP_FAIL(SSP_ERR_INVALID, "ssp_featnorm_sliding: null data pointer");
    const int64_t row0 = frame_seg->host.front();
    int64_t tiles = 0;
    for (int64_t u = 0; u < n; ++u) tiles += ceil_div<int64_t>(frame_seg->host[u + 1] - frame_seg->host[u], FN_TILE);
    if (tiles > INT32_MAX || n > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_featnorm_sliding: matrix too large for one launch");
    FeatnormState* fs = nullptr;
    SSP_TRY(fn_state(ctx, &fs));
    const float* tab = nullptr;
    if (mode == 2) SSP_TRY(fn_table(ctx, fs, window, &tab));
    SSP_TRY(fs->tiles.reserve((size_t)(n + 1) * sizeof(int64_t)));
    const size_t bytes = (size_t)rows * dim * sizeof(float);
    StageScope st(ctx, where);
    const float* d_in = st.in(feats + row0 * dim, bytes);
    float* d_out = st.out(out + row0 * dim, bytes);
    SSP_TRY(st.status());
    const int stride = ceil_div(FN_TILE + window, 64) * 64 + 8;  // rows of a column, + 8: the eight columns of a row land in eight banks
    const size_t lds = ((size_t)FN_COLS * stride + (mode == 2 ? 2 * (size_t)window - 1 : 0)) * sizeof(float);  // <= 49.4 KB
    SlidingArgs a{d_in, d_out, frame_seg->dev.as<int64_t>(), fs->tiles.as<int64_t>(), tab, row0, (int32_t)n, dim, window, stride};
    const dim3 grid((unsigned)tiles, (unsigned)ceil_div(dim, FN_COLS)), block(FN_TILE);
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, ctx->stream));
    hipLaunchKernelGGL(fn_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, frame_seg->dev.as<int64_t>(), (const int64_t*)nullptr, n, FN_TILE,
                       fs->tiles.as<int64_t>());
    if (mode == 0)
        hipLaunchKernelGGL(fn_sliding_kernel<0>, grid, block, lds, ctx->stream, a);
    else if (mode == 1)
        hipLaunchKernelGGL(fn_sliding_kernel<1>, grid, block, lds, ctx->stream, a);
    else
        hipLaunchKernelGGL(fn_sliding_kernel<2>, grid, block, lds, ctx->stream, a);
    SSP_HIP(hipGetLastError());
    SSP_TRY(tm.stop(ctx->stream, kernel_ms));
    return st.finish();
}

int ssp_select_frames(ssp_ctx* ctx, const float* feats, const ssp_segments* frame_seg, int32_t dim, const uint8_t* mask, float* out,
                      int64_t* counts_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_select_frames");
    if (!ctx) SSP_FAIL(SSP_ERR_INVALID, "null ssp_ctx");
    if (!frame_seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_select_frames: null segments");
    if (dim < 1 || dim > FN_MAX_DIM) SSP_FAIL(SSP_ERR_INVALID, "ssp_select_frames: dim=%d outside [1, %d]", dim, FN_MAX_DIM);
    SSP_TRY(check_where(where, "ssp_select_frames"));
    if (feats && out == feats) SSP_FAIL(SSP_ERR_INVALID, "ssp_select_frames: out == feats");
    const int64_t n = frame_seg->n, rows = frame_seg->total();
    if (n > 0 && !counts_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_select_frames: null counts_out");
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (n == 0) return SSP_OK;
    if (rows == 0) {
        std::fill(counts_out, counts_out + n, (int64_t)0);
        return SSP_OK;
    }
    if (!feats || !out || !mask) SSP_FAIL(SSP_ERR_INVALID, "ssp_select_frames: null data pointer");
    if (n > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_select_frames: too many utterances for one launch");
    const int64_t row0 = frame_seg->host.front();
    FeatnormState* fs = nullptr;
    SSP_TRY(fn_state(ctx, &fs));
    SSP_TRY(fs->sel.reserve((size_t)(2 * n + 1) * sizeof(int64_t)));
    int64_t *counts = fs->sel.as<int64_t>(), *base = counts + n;
    const size_t bytes = (size_t)rows * dim * sizeof(float);
    hipStream_t s = ctx->stream;
    StageScope st(ctx, where);
    const float* d_in = st.in(feats + row0 * dim, bytes);
    const uint8_t* d_mask = st.in(mask + row0, (size_t)rows);
    float* d_out = st.out(out, bytes, true);  // (the rows behind the kept ones keep the caller's bytes)
    SSP_TRY(st.status());
    const int64_t slices = std::min<int64_t>(FN_SEL_SLICES, ceil_div<int64_t>(frame_seg->max_len(), 256));
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    hipLaunchKernelGGL(fn_select_count_kernel, dim3((unsigned)n), dim3(256), 0, s, d_mask, frame_seg->dev.as<int64_t>(), row0, counts);
    hipLaunchKernelGGL(fn_scan_kernel, dim3(1), dim3(256), 0, s, (const int64_t*)nullptr, (const int64_t*)counts, n, 1, base);
    hipLaunchKernelGGL(fn_select_copy_kernel, dim3((unsigned)n, (unsigned)slices), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(d_in),
                       reinterpret_cast<uint32_t*>(d_out), d_mask, frame_seg->dev.as<int64_t>(), (const int64_t*)base, dim, row0);
    SSP_HIP(hipGetLastError());
    SSP_TRY(tm.stop(s, kernel_ms));
    SSP_HIP(hipMemcpyAsync(counts_out, counts, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    return st.finish(true);  // the one wait of the call: the counts
}

}  // extern "C"
