// x-vector extractor forward pass (Snyder et al. 2018: time-delay frame layers -> statistics pooling -> segment layers); the model is
// written out in include/ssp.h ("x-vector extractor").  An EXTENSION and UNPINNED: the reference has no TDNN; tests/xvector_oracle.py is
// the float64 restatement.
//
// * tdnn_kernel     a frame layer as an implicit-im2col GEMM on v_mfma_f32_32x32x2_f32, the staged block of gemm128.hpp that dense_kernel
//                   (dense.hip) runs too: the k index runs over (tap, channel), tap j of output row r reads input row r + j dil through the
//                   buffer resource, nothing unfolded is ever written.  The output keeps the ROW INDEX of its input (left-aligned in
//                   every sequence), so the kernel has no per-sequence logic: the last (taps - 1) dil rows of a sequence are junk that
//                   no valid row of a later layer reads and no window pools.  ONE k-ordered chain per output (taps ascending, channels
//                   ascending in chunks of 32, the tail of a tap's channels cleared in registers): the four waves split the 128 x 128
//                   output tile and never the k range, so a row's bits depend neither on its tile nor on its batch, slab or window.
// * xv_pool_kernel  mean and centred deviation of a window's rows, float64 accumulators, t ascending, one lane per column
// * xv_affine_kernel scale / offset of a segment layer behind ssp_dense_forward (dense.hip stays as it is)
#include <cmath>
#include <cstdlib>

#include "common.hpp"
#include "handle.hpp"
#include "gemm128.hpp"

namespace ssp {

constexpr int TBM = G128_BM;  // units per block step
constexpr int TBN = G128_BN;  // rows per workgroup
constexpr int TBK = G128_BK;  // k-chunk (inside one tap)

constexpr int TDNN_MAX_DIM = 8192;   // d_in and units
constexpr int TDNN_MAX_TAPS = 16;
constexpr int TDNN_MAX_SPAN = 1024;  // (taps - 1) dilation

struct TdnnArgs {
    const float* X;       // [N x d_in]
    const float* W;       // [units x taps x d_in]
    const float* bias;    // [units] (nullable)
    const float* scale;   // [units] (nullable: 1)
    const float* offset;  // [units] (nullable: 0)
    float* Y;             // [N x units], row r = the output whose first tap is input row r
    int64_t N;
    int32_t d_in, units, taps, dil, relu;
};

// where the two operand streams stand in the (tap, chunk) walk; every step is known on entry: taps x n_kc of them, then zeros
struct TdnnStep {
    int j, kc;
    __device__ __forceinline__ void next(int n_kc) {
        const bool wrap = kc + 1 == n_kc;  // (selects, not a branch: the k-loop stays one basic block)
        kc = wrap ? 0 : kc + 1;
        j += wrap ? 1 : 0;
    }
};

// gemm128.hpp's block with the k index running over (tap, channel): slab (j, kc) of the weights is columns [32 kc, 32 kc + 32) of tap j
// of a row of taps x d_in floats, that of the rows the same columns of input row r + j dil (d_in floats on)
__global__ __launch_bounds__(256, 2) void tdnn_kernel(TdnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int64_t col0 = (int64_t)blockIdx.x * TBN;
    const int d = a.d_in, taps = a.taps;
    const int wstride = taps * d, xshift = a.dil * d;
    const int n_kc = (d + TBK - 1) / TBK;
    const int n_rb = (a.units + TBM - 1) / TBM;
    // the rows this workgroup's taps reach: its own 128 and the (taps - 1) dil behind them
    const __amdgpu_buffer_rsrc_t rx = g128_rsrc(a.X, col0, a.N, (int64_t)TBN + (int64_t)(taps - 1) * a.dil, d);
    // (the nullable arrays are resolved here, once: the epilogue's element loop tests nothing that is not a register)
    const float *bias = a.bias, *scale = a.scale, *offset = a.offset;
    const int relu = a.relu;
    const bool affine = scale || offset;
    for (int rb = 0; rb < n_rb; ++rb) {
        const __amdgpu_buffer_rsrc_t rw = g128_rsrc(a.W, (int64_t)rb * TBM, a.units, TBM, wstride);
        TdnnStep sw{0, 0}, sx{0, 0};  // the next slab each stream loads
        f32x16 acc[2][2];
        g128_product(
            reinterpret_cast<float*>(smem), n_kc * taps, tid,
            [&](float4(&v)[4]) {
                g128_load(rw, wstride, sw.j * d, d, sw.kc * TBK, sw.j < taps, tid, v);
                sw.next(n_kc);
            },
            [&](float4(&v)[4]) {
                g128_load(rx, d, sx.j * xshift, d, sx.kc * TBK, sx.j < taps, tid, v);
                sx.next(n_kc);
            },
            acc);
        g128_epilogue(acc, a.Y, a.N, a.units, col0, rb, tid, [=](int unit, float t) {
            t = g128_bias_relu(t, bias, relu, unit);  // (ssp_dense_forward's rule)
            if (affine) t = __builtin_fmaf(scale ? scale[unit] : 1.f, t, offset ? offset[unit] : 0.f);
            return t;
        });
    }
}

// One workgroup per (window, block of 256 columns), one lane per column: two passes over the window's rows, t ascending, float64.
// win[2 w] = first row of window w in X, win[2 w + 1] = its row count (0: a row of NaN)
__global__ __launch_bounds__(256) void xv_pool_kernel(const float* __restrict__ X, int32_t dim, const int64_t* __restrict__ win, double var_floor,
                                                      float* __restrict__ out) {
    const int64_t w = blockIdx.x;
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= dim) return;
    const int64_t r0 = win[2 * w], n = win[2 * w + 1];
    float* o = out + w * 2 * (int64_t)dim;
    if (n <= 0) {
        o[c] = o[dim + c] = __builtin_nanf("");
        return;
    }
    const float* x = X + r0 * dim + c;
    double s = 0.0;
    for (int64_t t = 0; t < n; ++t) s += (double)x[t * dim];
    const double mean = s / (double)n;
    double q = 0.0;
    for (int64_t t = 0; t < n; ++t) {
        const double e = (double)x[t * dim] - mean;
        q += e * e;
    }
    double var = q / (double)n;
    var = var < var_floor ? var_floor : var;  // (a NaN stays a NaN)
    o[c] = (float)mean;
    o[dim + c] = (float)sqrt(var);
}

__global__ __launch_bounds__(256) void xv_affine_kernel(float* __restrict__ Y, int64_t total, int32_t units, const float* __restrict__ scale,
                                                        const float* __restrict__ offset) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int u = (int)(i % units);
    Y[i] = __builtin_fmaf(scale ? scale[u] : 1.f, Y[i], offset ? offset[u] : 0.f);
}

static int tdnn_check_shape(const char* fn, int32_t d_in, int32_t taps, int32_t dil, int32_t units) {
    if (d_in < 1 || taps < 1 || dil < 1 || units < 1) SSP_FAIL(SSP_ERR_INVALID, "%s: d_in, taps, dilation and units must be >= 1", fn);
    if (d_in > TDNN_MAX_DIM || units > TDNN_MAX_DIM || taps > TDNN_MAX_TAPS || (int64_t)(taps - 1) * dil > TDNN_MAX_SPAN)
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: d_in and units up to %d, up to %d taps, (taps - 1) dilation up to %d", fn, TDNN_MAX_DIM, TDNN_MAX_TAPS,
                 TDNN_MAX_SPAN);
    return SSP_OK;
}

// device pointers; N rows
static int tdnn_launch(const TdnnArgs& a, hipStream_t s) {
    if (a.N <= 0) return SSP_OK;
    const int64_t grid = (a.N + TBN - 1) / TBN;
    if (grid > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "tdnn: too many rows for one launch");
    constexpr size_t lds = G128_LDS;
    SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(tdnn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(tdnn_kernel, dim3((unsigned)grid), dim3(256), lds, s, a);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

static int pool_launch(const float* X, int32_t dim, const int64_t* dwin, int64_t n_win, double var_floor, float* out, hipStream_t s) {
    if (n_win <= 0) return SSP_OK;
    hipLaunchKernelGGL(xv_pool_kernel, dim3((unsigned)n_win, (unsigned)((dim + 255) / 256)), dim3(256), 0, s, X, dim, dwin, var_floor, out);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

// (sequence, first, end) rows of a HOST window table checked against the segments; no table: one window per sequence
static int check_windows(const char* fn, const ssp_segments* seg, const int64_t* pool_win, int64_t n_win) {
    if (!pool_win) return SSP_OK;
    int64_t prev = 0;
    for (int64_t w = 0; w < n_win; ++w) {
        const int64_t q = pool_win[3 * w], a = pool_win[3 * w + 1], b = pool_win[3 * w + 2];
        if (q < prev || q >= seg->n) SSP_FAIL(SSP_ERR_INVALID, "%s: window %lld names sequence %lld (sequences must be non-decreasing and below %lld)", fn,
                                              (long long)w, (long long)q, (long long)seg->n);
        if (a < 0 || a > b || b > seg->host[(size_t)q + 1] - seg->host[(size_t)q])
            SSP_FAIL(SSP_ERR_INVALID, "%s: window %lld [%lld, %lld) does not lie inside its sequence of %lld frames", fn, (long long)w, (long long)a,
                     (long long)b, (long long)(seg->host[(size_t)q + 1] - seg->host[(size_t)q]));
        prev = q;
    }
    return SSP_OK;
}

struct XvLayer {
    int32_t d_in = 0, units = 0, taps = 1, dil = 1, relu = 0;
    DevBuf W, bias, scale, offset;  // (bias / scale / offset: empty = none)
};

}  // namespace ssp

struct ssp_xvector {
    ssp_ctx* ctx = nullptr;
    int32_t d_in = 0, receptive = 1, pooled = 0, embed = 0, widest = 0;
    double var_floor = 0.0;
    std::vector<ssp::XvLayer> frame, segment;  // (sized once at creation: DevBuf does not move)
    size_t cap = (size_t)2 << 30;  // workspace cap of one call, bytes
    int64_t last_slab = 0;         // sequences in the largest slab of the last forward call
    ssp::DevBuf act[2];            // ping-pong activations [slab rows x widest]
    ssp::DevBuf pooled_buf, seg_buf[2];  // [windows x pooled], [windows x widest segment layer]
    ssp::DevBuf tab;               // the call's window table (first row, rows) on the device
    std::vector<int64_t> tab_host; // ... and its host image, which the queued copy reads
};

using namespace ssp;

extern "C" {

int ssp_tdnn_forward(ssp_ctx* ctx, const float* X, const ssp_segments* frame_seg, int32_t d_in, const float* W, const float* bias, int32_t taps,
                     int32_t dilation, int32_t units, int32_t relu, const float* scale, const float* offset, float* Y, int64_t* out_len, int where,
                     float* kernel_ms) {
    ssp::TraceRange trace_("ssp_tdnn_forward");
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (!frame_seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_tdnn_forward: null segments");
    SSP_TRY(tdnn_check_shape("ssp_tdnn_forward", d_in, taps, dilation, units));
    SSP_TRY(check_where(where, "ssp_tdnn_forward"));
    if (frame_seg->ctx && frame_seg->ctx->device != ctx->device) SSP_FAIL(SSP_ERR_INVALID, "ssp_tdnn_forward: the segments live on another device");
    const int64_t span = (int64_t)(taps - 1) * dilation;
    if (out_len)
        for (int64_t i = 0; i < frame_seg->n; ++i) {
            const int64_t T = frame_seg->host[(size_t)i + 1] - frame_seg->host[(size_t)i];
            out_len[i] = T > span ? T - span : 0;
        }
    const int64_t row0 = frame_seg->n ? frame_seg->host.front() : 0, N = frame_seg->total();
    if (N == 0) return SSP_OK;
    if (!X || !W || !Y) SSP_FAIL(SSP_ERR_INVALID, "ssp_tdnn_forward: null array");
    hipStream_t s = ctx->stream;
    StageScope st(ctx, where);
    TdnnArgs a{};
    a.X = st.in(X + row0 * d_in, (size_t)N * d_in * sizeof(float));
    a.W = st.in(W, (size_t)units * taps * d_in * sizeof(float));
    a.bias = st.in(bias, (size_t)units * sizeof(float));
    a.scale = st.in(scale, (size_t)units * sizeof(float));
    a.offset = st.in(offset, (size_t)units * sizeof(float));
    a.Y = st.out(Y + row0 * units, (size_t)N * units * sizeof(float));
    SSP_TRY(st.status());
    a.N = N, a.d_in = d_in, a.units = units, a.taps = taps, a.dil = dilation, a.relu = relu ? 1 : 0;
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    SSP_TRY(tdnn_launch(a, s));
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}

int ssp_stats_pool(ssp_ctx* ctx, const float* X, const ssp_segments* frame_seg, int32_t dim, const int64_t* pool_win, int64_t n_win, double var_floor,
                   float* out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_stats_pool");
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (!frame_seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_stats_pool: null segments");
    if (dim < 1 || n_win < 0 || !(var_floor >= 0.0)) SSP_FAIL(SSP_ERR_INVALID, "ssp_stats_pool: dim >= 1, n_win >= 0, var_floor >= 0");
    if (dim > 65535 * 256) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_stats_pool: dim above 65535 x 256");
    SSP_TRY(check_where(where, "ssp_stats_pool"));
    if (frame_seg->ctx && frame_seg->ctx->device != ctx->device) SSP_FAIL(SSP_ERR_INVALID, "ssp_stats_pool: the segments live on another device");
    SSP_TRY(check_windows("ssp_stats_pool", frame_seg, pool_win, n_win));
    if (!pool_win) n_win = frame_seg->n;
    if (n_win > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_stats_pool: too many windows for one launch");
    if (n_win == 0) return SSP_OK;
    if (!out || (!X && frame_seg->total() > 0)) SSP_FAIL(SSP_ERR_INVALID, "ssp_stats_pool: null array");
    // the table shares the diarization block's per-call table and host image (one call at a time on the ctx's stream)
    const int64_t row0 = frame_seg->host.front();
    std::vector<char>& blob = ctx->diar_host;
    try {
        blob.resize((size_t)n_win * 2 * sizeof(int64_t));
    } catch (...) {
        SSP_FAIL(SSP_ERR_NOMEM, "ssp_stats_pool: host alloc");
    }
    int64_t* t = reinterpret_cast<int64_t*>(blob.data());
    for (int64_t w = 0; w < n_win; ++w) {
        const int64_t q = pool_win ? pool_win[3 * w] : w;
        const int64_t T = frame_seg->host[(size_t)q + 1] - frame_seg->host[(size_t)q];
        const int64_t a = pool_win ? pool_win[3 * w + 1] : 0, b = pool_win ? pool_win[3 * w + 2] : T;
        t[2 * w] = frame_seg->host[(size_t)q] - row0 + a;
        t[2 * w + 1] = b - a;
    }
    hipStream_t s = ctx->stream;
    SSP_TRY(ctx->diar_tab.reserve(blob.size()));
    SSP_HIP(hipMemcpyAsync(ctx->diar_tab.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
    StageScope st(ctx, where);
    const size_t in_bytes = (size_t)frame_seg->total() * dim * sizeof(float);
    const float* dX = st.in(in_bytes ? X + row0 * dim : nullptr, in_bytes);
    float* dO = st.out(out, (size_t)n_win * 2 * dim * sizeof(float));
    SSP_TRY(st.status());
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    SSP_TRY(pool_launch(dX, dim, ctx->diar_tab.as<int64_t>(), n_win, var_floor, dO, s));
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}

int ssp_xvector_create(ssp_ctx* ctx, int32_t d_in, int32_t n_frame_layers, const int32_t* units, const int32_t* taps, const int32_t* dilation,
                       const float* const* W, const float* const* bias, const int32_t* relu, const float* const* scale, const float* const* offset,
                       int32_t n_segment_layers, const int32_t* seg_units, const float* const* seg_W, const float* const* seg_bias,
                       const int32_t* seg_relu, const float* const* seg_scale, const float* const* seg_offset, double var_floor, ssp_xvector** out) try {
    if (!out) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_create: null out");
    *out = nullptr;
    if (n_frame_layers < 1 || n_segment_layers < 0 || !units || !taps || !dilation || !W || !relu)
        SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_create: at least one frame layer with units, taps, dilation, W and relu");
    if (n_segment_layers > 0 && (!seg_units || !seg_W || !seg_relu)) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_create: segment layers need units, W and relu");
    if (!(var_floor >= 0.0)) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_create: var_floor must be >= 0");
    if (n_frame_layers > 64 || n_segment_layers > 64) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_xvector_create: up to 64 frame and 64 segment layers");
    int32_t d = d_in;
    int64_t R = 1;
    for (int l = 0; l < n_frame_layers; ++l) {
        SSP_TRY(tdnn_check_shape("ssp_xvector_create", d, taps[l], dilation[l], units[l]));
        if (!W[l]) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_create: null kernel of frame layer %d", l);
        R += (int64_t)(taps[l] - 1) * dilation[l];
        d = units[l];
    }
    if (2 * (int64_t)d > (1 << 21)) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_xvector_create: pooled width above 2^21");
    const int32_t pooled = 2 * d;
    d = pooled;
    for (int l = 0; l < n_segment_layers; ++l) {
        if (seg_units[l] < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_create: segment layer %d without units", l);
        if (seg_units[l] > (1 << 21)) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_xvector_create: segment layer %d wider than 2^21", l);
        if (!seg_W[l]) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_create: null kernel of segment layer %d", l);
        d = seg_units[l];
    }
    SSP_TRY(use_ctx(ctx));
    HandleBuild<ssp_xvector> m(ctx, "ssp_xvector_create");
    m->d_in = d_in;
    m->receptive = (int32_t)R;
    m->pooled = pooled;
    m->embed = d;
    m->var_floor = var_floor;
    int rc = SSP_OK;
    m->frame = std::vector<XvLayer>((size_t)n_frame_layers);
    m->segment = std::vector<XvLayer>((size_t)n_segment_layers);
    auto fill = [&](XvLayer& L, int32_t din, int32_t u, int32_t tp, int32_t dl, int32_t rl, const float* w, const float* b, const float* sc,
                    const float* of) -> int {
        L.d_in = din, L.units = u, L.taps = tp, L.dil = dl, L.relu = rl ? 1 : 0;
        SSP_TRY(upload(m, L.W, w, (size_t)u * tp * din));
        if (b) SSP_TRY(upload(m, L.bias, b, (size_t)u));
        if (sc) SSP_TRY(upload(m, L.scale, sc, (size_t)u));
        if (of) SSP_TRY(upload(m, L.offset, of, (size_t)u));
        return SSP_OK;
    };
    d = d_in;
    for (int l = 0; l < n_frame_layers && rc == SSP_OK; ++l) {
        rc = fill(m->frame[(size_t)l], d, units[l], taps[l], dilation[l], relu[l], W[l], bias ? bias[l] : nullptr, scale ? scale[l] : nullptr,
                  offset ? offset[l] : nullptr);
        d = units[l];
        if (d > m->widest) m->widest = d;
    }
    d = pooled;
    for (int l = 0; l < n_segment_layers && rc == SSP_OK; ++l) {
        rc = fill(m->segment[(size_t)l], d, seg_units[l], 1, 1, seg_relu[l], seg_W[l], seg_bias ? seg_bias[l] : nullptr,
                  seg_scale ? seg_scale[l] : nullptr, seg_offset ? seg_offset[l] : nullptr);
        d = seg_units[l];
    }
    return m.commit(rc, out);
}
SSP_CREATE_GUARD("ssp_xvector_create")

int ssp_xvector_destroy(ssp_xvector* xv) { return destroy_handle(xv); }

int ssp_xvector_info(const ssp_xvector* xv, int32_t* receptive_field, int32_t* pooled_width, int32_t* embed_width) {
    if (!xv) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_info: null handle");
    if (receptive_field) *receptive_field = xv->receptive;
    if (pooled_width) *pooled_width = xv->pooled;
    if (embed_width) *embed_width = xv->embed;
    return SSP_OK;
}

int ssp_xvector_set_workspace(ssp_xvector* xv, size_t bytes) {
    if (!xv) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_set_workspace: null handle");
    if (bytes == 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_set_workspace: zero bytes");
    xv->cap = bytes;
    return SSP_OK;
}

int ssp_xvector_last_slab(const ssp_xvector* xv, int64_t* sequences_out) {
    if (!xv || !sequences_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_last_slab: null argument");
    *sequences_out = xv->last_slab;
    return SSP_OK;
}

int ssp_xvector_forward(ssp_xvector* xv, const float* feats, const ssp_segments* frame_seg, const int64_t* pool_win, int64_t n_win, float* emb_out,
                        int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_xvector_forward");
    if (!xv) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_forward: null handle");
    if (!frame_seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_forward: null segments");
    ssp_ctx* ctx = xv->ctx;
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    SSP_TRY(check_where(where, "ssp_xvector_forward"));
    if (frame_seg->ctx && frame_seg->ctx->device != ctx->device) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_forward: the segments live on another device");
    if (n_win < 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_forward: n_win < 0");
    SSP_TRY(check_windows("ssp_xvector_forward", frame_seg, pool_win, n_win));
    const int64_t n_seq = frame_seg->n;
    if (!pool_win) n_win = n_seq;
    if (n_win > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_xvector_forward: too many windows for one launch");
    if (n_win == 0) return SSP_OK;
    int32_t seg_widest = 0;
    for (const XvLayer& L : xv->segment) seg_widest = L.units > seg_widest ? L.units : seg_widest;
    if (n_win * (int64_t)(seg_widest > 0 ? seg_widest : 1) / 256 >= INT32_MAX)
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_xvector_forward: windows x segment width too large for one launch");
    if (!emb_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_forward: null output");
    if (!feats && frame_seg->total() > 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_xvector_forward: null features");
    const std::vector<int64_t>& off = frame_seg->host;
    const int64_t R = xv->receptive;
    const int32_t E = xv->embed, P = xv->pooled;
    // slabs of WHOLE sequences under the cap (one sequence always runs); the windows of a slab's sequences are a contiguous run of the table
    const size_t per_row = 2 * (size_t)xv->widest * sizeof(float);
    int64_t cap_rows = (int64_t)(xv->cap / per_row);
    if (cap_rows < 1) cap_rows = 1;
    std::vector<int64_t> cut, wcut;  // sequence and window index where each slab starts
    std::vector<int64_t>& tab = xv->tab_host;
    int64_t max_rows = 0, max_win = 0, max_seq = 0;
    try {
        tab.resize((size_t)n_win * 2);
        cut.push_back(0);
        for (int64_t q = 0; q < n_seq;) {
            int64_t e = q + 1;
            while (e < n_seq && off[(size_t)e + 1] - off[(size_t)q] <= cap_rows) ++e;
            cut.push_back(e);
            q = e;
        }
        int64_t w = 0;
        for (size_t c = 0; c + 1 < cut.size(); ++c) {
            wcut.push_back(w);
            const int64_t base = off[(size_t)cut[c]];
            if (pool_win) {
                for (; w < n_win && pool_win[3 * w] < cut[c + 1]; ++w) {
                    const int64_t q = pool_win[3 * w], a = pool_win[3 * w + 1], b = pool_win[3 * w + 2];
                    tab[(size_t)2 * w] = off[(size_t)q] - base + a;
                    tab[(size_t)2 * w + 1] = b - a >= R ? b - a - (R - 1) : 0;
                }
            } else {
                for (; w < cut[c + 1]; ++w) {
                    const int64_t T = off[(size_t)w + 1] - off[(size_t)w];
                    tab[(size_t)2 * w] = off[(size_t)w] - base;
                    tab[(size_t)2 * w + 1] = T >= R ? T - (R - 1) : 0;
                }
            }
            const int64_t rows = off[(size_t)cut[c + 1]] - base;
            max_rows = rows > max_rows ? rows : max_rows;
            max_win = w - wcut.back() > max_win ? w - wcut.back() : max_win;
            max_seq = cut[c + 1] - cut[c] > max_seq ? cut[c + 1] - cut[c] : max_seq;
        }
        wcut.push_back(w);
    } catch (...) {
        SSP_FAIL(SSP_ERR_NOMEM, "ssp_xvector_forward: host alloc");
    }
    xv->last_slab = max_seq;
    hipStream_t s = ctx->stream;
    SSP_TRY(xv->act[0].reserve((size_t)max_rows * xv->widest * sizeof(float)));
    SSP_TRY(xv->act[1].reserve((size_t)max_rows * xv->widest * sizeof(float)));
    SSP_TRY(xv->tab.reserve(tab.size() * sizeof(int64_t)));
    if (!xv->segment.empty()) {
        SSP_TRY(xv->pooled_buf.reserve((size_t)max_win * P * sizeof(float)));
        if (xv->segment.size() > 1) {
            SSP_TRY(xv->seg_buf[0].reserve((size_t)max_win * seg_widest * sizeof(float)));
            SSP_TRY(xv->seg_buf[1].reserve((size_t)max_win * seg_widest * sizeof(float)));
        }
    }
    SSP_HIP(hipMemcpyAsync(xv->tab.p, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const int64_t base = off[(size_t)cut[c]], rows = off[(size_t)cut[c + 1]] - base;
        const int64_t w0 = wcut[c], nw = wcut[c + 1] - w0;
        if (nw == 0) continue;  // (nothing pools this slab's sequences)
        StageScope st(ctx, where);  // (of this slab)
        const float* dX = st.in(rows ? feats + base * xv->d_in : nullptr, (size_t)rows * xv->d_in * sizeof(float));
        float* dE = st.out(emb_out + w0 * E, (size_t)nw * E * sizeof(float));
        SSP_TRY(st.status());
        const float* cur = dX;
        int side = 0;
        for (const XvLayer& L : xv->frame) {
            TdnnArgs a{};
            a.X = cur, a.W = L.W.as<float>(), a.bias = L.bias.as<float>(), a.scale = L.scale.as<float>(), a.offset = L.offset.as<float>();
            a.Y = xv->act[side].as<float>();
            a.N = rows, a.d_in = L.d_in, a.units = L.units, a.taps = L.taps, a.dil = L.dil, a.relu = L.relu;
            SSP_TRY(tdnn_launch(a, s));
            cur = a.Y;
            side ^= 1;
        }
        float* pooled = xv->segment.empty() ? dE : xv->pooled_buf.as<float>();
        SSP_TRY(pool_launch(cur, P / 2, xv->tab.as<int64_t>() + 2 * w0, nw, xv->var_floor, pooled, s));
        const float* in = pooled;
        for (size_t l = 0; l < xv->segment.size(); ++l) {
            const XvLayer& L = xv->segment[l];
            float* y = l + 1 == xv->segment.size() ? dE : xv->seg_buf[l & 1].as<float>();
            SSP_TRY(ssp_dense_forward(ctx, in, nw, L.d_in, L.W.as<float>(), L.bias.as<float>(), L.units, L.relu, y, SSP_DEVICE, nullptr));
            if (L.scale.p || L.offset.p) {
                const int64_t total = nw * L.units;
                hipLaunchKernelGGL(xv_affine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, y, total, L.units, L.scale.as<float>(),
                                   L.offset.as<float>());
                SSP_HIP(hipGetLastError());
            }
            in = y;
        }
        SSP_TRY(st.finish());  // (the slab's wait on SSP_HOST; its staging is given back at the end of the scope)
    }
    SSP_TRY(tm.stop(s, kernel_ms));
    return SSP_OK;
}

}  // extern "C"
