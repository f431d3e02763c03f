// Dense layer forward on gfx950 MFMA: Y = act(X W + b), the building block of the d-vector speaker network's predict()
// (d_vector.py:171-189: Dense(256) x 4 with ReLU between, spkModel.predict at d_vector.py:298-299 / 327 / 348).
// (units x d_in) . (d_in x samples) fp32 MFMA GEMM, output units as the MFMA rows and samples as the columns (the layout
// of the cosine scorer, csrc/cosine.hip, whose operand image this kernel shares), bias + ReLU fused into the epilogue, four
// consecutive units per 16-byte store.  The staged block itself is csrc/gemm128.hpp, shared with tdnn_kernel (xvector.hip).
#include <cstdlib>

#include "common.hpp"
#include "gemm128.hpp"

namespace ssp {

int launch_dense_reg(ssp_ctx* ctx, const float* dX, int64_t N, int d_in, const float* dW, const float* dB, int units, int relu, float* dY,
                     hipStream_t s);  // cosine.hip

constexpr int DBM = G128_BM;  // units per block step
constexpr int DBN = G128_BN;  // samples per workgroup
constexpr int DBK = 32;       // k-chunk
static_assert(DBK == G128_BK, "dense_kernel walks gemm128.hpp's slabs");

struct DenseArgs {
    const float* X;     // [N x d_in]
    const float* Wt;    // [units x d_in]  (the Keras kernel transposed)
    const float* bias;  // [units] (nullable)
    float* Y;           // [N x units]
    int64_t N;
    int32_t d_in, units, relu;
};

// gemm128.hpp's block with both streams plain advancing columns of d_in-float rows: weights as the units, samples as the rows
__global__ __launch_bounds__(256, 2) void dense_kernel(DenseArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int64_t col0 = (int64_t)blockIdx.x * DBN;
    const int d = a.d_in;
    const int n_kc = (d + DBK - 1) / DBK;
    const int n_rb = (a.units + DBM - 1) / DBM;
    const __amdgpu_buffer_rsrc_t rx = g128_rsrc(a.X, col0, a.N, DBN, d);
    const float* bias = a.bias;
    const int relu = a.relu;
    for (int rb = 0; rb < n_rb; ++rb) {
        const __amdgpu_buffer_rsrc_t rw = g128_rsrc(a.Wt, (int64_t)rb * DBM, a.units, DBM, d);
        int kw = 0, kx = 0;  // the column each stream loads next (beyond d_in: zeros)
        f32x16 acc[2][2];
        g128_product(
            reinterpret_cast<float*>(smem), n_kc, tid,
            [&](float4(&v)[4]) {
                g128_load(rw, d, 0, d, kw, true, tid, v);
                kw += DBK;
            },
            [&](float4(&v)[4]) {
                g128_load(rx, d, 0, d, kx, true, tid, v);
                kx += DBK;
            },
            acc);
        g128_epilogue(acc, a.Y, a.N, a.units, col0, rb, tid, [=](int unit, float t) { return g128_bias_relu(t, bias, relu, unit); });
    }
}

}  // namespace ssp

using namespace ssp;

extern "C" int ssp_dense_forward(ssp_ctx* ctx, const float* X, int64_t N, int32_t d_in, const float* Wt, const float* bias,
                                 int32_t units, int32_t relu, float* Y, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_dense_forward");
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (N < 0 || d_in < 1 || units < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_dense_forward: bad shape");
    if (d_in > (1 << 21)) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_dense_forward: d_in above 2^21 (32-bit offsets inside a 128-row block)");
    SSP_TRY(check_where(where, "ssp_dense_forward"));
    if (N == 0) return SSP_OK;
    if (!X || !Wt || !Y) SSP_FAIL(SSP_ERR_INVALID, "ssp_dense_forward: null array");
    const int64_t grid = (N + DBN - 1) / DBN;
    if (grid > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_dense_forward: too many samples");
    hipStream_t s = ctx->stream;
    StageScope st(ctx, where);
    const float *dX = st.in(X, (size_t)N * d_in * sizeof(float)), *dW = st.in(Wt, (size_t)units * d_in * sizeof(float));
    const float* dB = st.in(bias, (size_t)units * sizeof(float));
    float* dY = st.out(Y, (size_t)N * units * sizeof(float));
    SSP_TRY(st.status());
    if (d_in <= 256 && !getenv("SSP_DENSE_NO_REG")) {  // samples held in registers, weight tiles streamed (cosine.hip): the network's hidden layers
        Timer tr;
        SSP_TRY(tr.start(kernel_ms != nullptr, s));
        SSP_TRY(launch_dense_reg(ctx, dX, N, d_in, dW, dB, units, relu ? 1 : 0, dY, s));
        SSP_TRY(tr.stop(s, kernel_ms));
        return st.finish();
    }
    DenseArgs a{dX, dW, dB, dY, N, d_in, units, relu ? 1 : 0};
    constexpr size_t lds = G128_LDS;
    SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(dense_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    hipLaunchKernelGGL(dense_kernel, dim3((unsigned)grid), dim3(256), lds, s, a);
    SSP_HIP(hipGetLastError());
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}
