// Forward pass of the reference's conv + GRU d-vector network (d_vector.py:213-269 inference_gru: Conv2D(64, 5x5, stride 2, same) ->
// TimeDistributed(Flatten) -> 3 x GRU(1024, return_sequences) -> mean over time -> Dense(512) -> L2 normalisation; the network the
// reference's __main__ evaluates at d_vector.py:389 under model_name 'lstm_conv').  Keras' arithmetic at inference:
//     conv   Y[t, f, c] = b[c] + sum_ij X[t sh + i - top, f sw + j - left] K[i, j, 0, c]     (cross-correlation, TensorFlow's `same`)
//     GRU    gate blocks z | r | h, s = hard_sigmoid or sigmoid, zero initial state
//            reset_after = 0:  z = s(x W_z + b_z + h U_z)   r = s(x W_r + b_r + h U_r)   hh = tanh(x W_h + b_h + (r . h) U_h)
//            reset_after = 1:  z = s(x W_z + b_iz + h U_z + b_rz)   r likewise   hh = tanh(x W_h + b_ih + r . (h U_h + b_rh))
//            h_t = z . h_{t-1} + (1 - z) . hh
//   * the input projection x W + b_input of all N T rows of a layer is ONE GEMM (ssp_dense_forward's kernels) into a projection buffer
//   * the recurrence is one launch per time step (two for reset_after = 0, whose candidate needs r . h first): an exact-fp32
//     v_mfma_f32_16x16x4_f32 GEMM of h_{t-1} (N x H) against U, units as the MFMA rows and sequences as the columns (the layout of
//     lstm.hip).  U is packed at create time by unit tile: for tile j (units 16 j .. 16 j + 15) and k group g the three gates are three
//     operand fragments, so lane (kq, n) register r of the three accumulators is unit 16 j + 4 kq + r of sequence n — z, r and h
//     pre-activations of one unit meet in one lane and the gate arithmetic is element-wise in the epilogue, which reads the step's slice
//     of the projection and writes h_t straight into row t of the layer's output sequence; h_{t-1} is row t - 1 of the same buffer
//   * a wave = 32 units x 64 sequences, a workgroup = 4 waves = 128 units of the same 64 sequences (their h fragments are the same
//     addresses: the second to fourth wave hit the vector cache); operands are 16-byte loads straight from global memory, the packed
//     image of U coalesced (1 KiB per wave and fragment), loaded one k group ahead of the MFMAs that consume them
//   * every output element sums k in ascending groups in one accumulator: its bits do not depend on the batch, and MFMA columns are
//     independent, so a sequence never sees its neighbours.  No grid-wide barrier, no spin: steps are ordered by the stream
#include <cstdlib>
#include <vector>

#include "common.hpp"
#include "handle.hpp"
#include "nn_device.hpp"

namespace ssp {

constexpr int GRU_MAXH = 1024;   // widest state
constexpr int GRU_MAXD = 4096;   // widest input
constexpr int CONV_MAXK = 7, CONV_MAXF = 256;

struct GruStepArgs {
    const float* img;    // packed U: [unit tile j][k group g][3 gates][64 lanes][4 r]
    const float* hsrc;   // B operand rows: h_{t-1}, or r . h_{t-1} for the candidate launch; null = zero (t = 0: no product)
    const float* hprev;  // h_{t-1} rows for the epilogue; null = zero
    const float* proj;   // this step's slice of the projection: row n at proj + n ld_p, gate q at + q H
    const float* rbias;  // [3H] recurrent bias (reset_after = 1) or null
    float* hout;         // h_t rows: row n at hout + n ld_seq
    float* zbuf;         // [N x H] z of this step      (reset_after = 0)
    float* rhbuf;        // [N x H] r . h_{t-1}          (reset_after = 0)
    int64_t N, ld_src, ld_seq, ld_p;
    int32_t H;
};

// MODE 0: reset_after = 1, all three gates, one launch per step
// MODE 1: reset_after = 0, first launch: z and r; leaves z and r . h_{t-1} in the workspace
// MODE 2: reset_after = 0, second launch: candidate from (r . h_{t-1}) U_h, then the state update
// ACT = 0 hard_sigmoid | 1 sigmoid (MODE 2 applies none)
template <int MODE, int ACT>
__global__ __launch_bounds__(256, 2) void gru_step_kernel(GruStepArgs a) {
    constexpr int NG = MODE == 0 ? 3 : MODE == 1 ? 2 : 1;
    constexpr int Q0 = MODE == 2 ? 2 : 0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, kq = lane >> 4;
    const int KG = a.H >> 4;                               // k groups of 16 = unit tiles of 16
    // unit blocks vary fastest in the linear workgroup id: workgroups are dealt round-robin over the 8 XCDs, so with the 8 unit blocks of
    // H = 1024 every XCD multiplies by ONE 1.5 MiB slice of U, which fits its 4 MiB L2 (sequence blocks fastest: all 12 MiB per XCD).
    // (Measured at the reference's shape: the same time either way — the step is not bound by where U comes from; profiles/gru.md.)
    const int UB = (a.H + 127) >> 7;
    const int ub = (int)(blockIdx.x % (unsigned)UB);
    const int j0 = (ub * 4 + wave) * 2;                    // the first of this wave's two unit tiles
    if (j0 >= KG) return;                                  // (no barrier in this kernel)
    const int64_t seq0 = (int64_t)(blockIdx.x / (unsigned)UB) * 64;

    f32x4 acc[NG][2][4];
#pragma unroll
    for (int q = 0; q < NG; ++q)
#pragma unroll
        for (int ut = 0; ut < 2; ++ut)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[q][ut][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (a.hsrc) {
        const float* __restrict__ bp[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            int64_t row = seq0 + 16 * c + n;
            row = row < a.N ? row : a.N - 1;               // (columns beyond the batch repeat its last row and are never stored)
            bp[c] = a.hsrc + row * a.ld_src + 4 * kq;
        }
        const size_t tile = (size_t)KG * 768;              // floats per unit tile (the image holds an even number of tiles)
        const float* __restrict__ ap = a.img + (size_t)j0 * tile + (size_t)Q0 * 256 + lane * 4;
        f32x4 wa[2][NG], ha[4], wb[2][NG], hb[4];
        auto load = [&](int g, f32x4 (&ww)[2][NG], f32x4 (&hh)[4]) {
#pragma unroll
            for (int ut = 0; ut < 2; ++ut)
#pragma unroll
                for (int q = 0; q < NG; ++q) ww[ut][q] = *reinterpret_cast<const f32x4*>(ap + ut * tile + (size_t)g * 768 + q * 256);
#pragma unroll
            for (int c = 0; c < 4; ++c) hh[c] = *reinterpret_cast<const f32x4*>(bp[c] + 16 * g);
        };
        auto mul = [&](const f32x4 (&ww)[2][NG], const f32x4 (&hh)[4]) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < NG; ++q)
#pragma unroll
                    for (int ut = 0; ut < 2; ++ut)
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            acc[q][ut][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(ww[ut][q][r], hh[c][r], acc[q][ut][c], 0, 0, 0);
        };
        // two register sets: the loads of group g + 1 are issued before the products of group g and land under them (the scheduling
        // barriers keep the compiler from sinking the loads to their first use, which it otherwise does)
        load(0, wa, ha);
        for (int g = 0; g < KG; g += 2) {
            load(g + 1 < KG ? g + 1 : g, wb, hb);
            __builtin_amdgcn_sched_barrier(0);
            mul(wa, ha);
            __builtin_amdgcn_sched_barrier(0);
            if (g + 1 < KG) {
                load(g + 2 < KG ? g + 2 : g + 1, wa, ha);
                __builtin_amdgcn_sched_barrier(0);
                mul(wb, hb);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    // epilogue: accumulator register r of lane (kq, n) = unit 16 j + 4 kq + r of sequence seq0 + 16 c + n
#pragma unroll
    for (int ut = 0; ut < 2; ++ut) {
        const int u = 16 * (j0 + ut) + 4 * kq;
        if (u >= a.H) continue;                            // (the padding tile of an odd tile count)
        f32x4 rb[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        if (MODE == 0 && a.rbias) {
#pragma unroll
            for (int q = 0; q < 3; ++q) rb[q] = *reinterpret_cast<const f32x4*>(a.rbias + q * a.H + u);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t seq = seq0 + 16 * c + n;
            if (seq >= a.N) continue;
            const float* __restrict__ pr = a.proj + seq * a.ld_p + u;
            f32x4 hp = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.hprev) hp = *reinterpret_cast<const f32x4*>(a.hprev + seq * a.ld_seq + u);
            f32x4 out;
            if (MODE == 0) {
                const f32x4 xz = *reinterpret_cast<const f32x4*>(pr), xr = *reinterpret_cast<const f32x4*>(pr + a.H),
                            xh = *reinterpret_cast<const f32x4*>(pr + 2 * a.H);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float z = gate<ACT>(xz[r] + (acc[0][ut][c][r] + rb[0][r]));
                    const float rg = gate<ACT>(xr[r] + (acc[1][ut][c][r] + rb[1][r]));
                    const float hh = tanh_hw(xh[r] + rg * (acc[2][ut][c][r] + rb[2][r]));
                    out[r] = z * hp[r] + (1.f - z) * hh;
                }
                *reinterpret_cast<f32x4*>(a.hout + seq * a.ld_seq + u) = out;
            } else if (MODE == 1) {
                const f32x4 xz = *reinterpret_cast<const f32x4*>(pr), xr = *reinterpret_cast<const f32x4*>(pr + a.H);
                f32x4 rh;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    out[r] = gate<ACT>(xz[r] + acc[0][ut][c][r]);
                    rh[r] = gate<ACT>(xr[r] + acc[1][ut][c][r]) * hp[r];
                }
                *reinterpret_cast<f32x4*>(a.zbuf + seq * a.H + u) = out;
                *reinterpret_cast<f32x4*>(a.rhbuf + seq * a.H + u) = rh;
            } else {
                const f32x4 xh = *reinterpret_cast<const f32x4*>(pr + 2 * a.H);
                const f32x4 z = *reinterpret_cast<const f32x4*>(a.zbuf + seq * a.H + u);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float hh = tanh_hw(xh[r] + acc[0][ut][c][r]);
                    out[r] = z[r] * hp[r] + (1.f - z[r]) * hh;
                }
                *reinterpret_cast<f32x4*>(a.hout + seq * a.ld_seq + u) = out;
            }
        }
    }
}

// mean over time of a layer's output sequence (d_vector.py:234-237, the temporalAverage Lambda): t ascending, one thread
// per (sequence, unit)
__global__ __launch_bounds__(256) void gru_time_mean_kernel(const float* __restrict__ seq, int64_t N, int32_t T, int32_t H, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N * H) return;
    const int64_t nn = i / H;
    const int u = (int)(i - nn * H);
    const float* p = seq + nn * T * H + u;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += p[(int64_t)t * H];
    out[i] = s / (float)T;
}

// Conv2D with one input channel, channels last, TensorFlow's `same` padding (d_vector.py:216-221): one thread per output element,
// taps in (i, j) order.  0.07 % of the network's arithmetic.
struct ConvArgs {
    const float* X;     // [N x T x D]
    const float* K;     // [kh x kw x F]
    const float* bias;  // [F] or null
    float* Y;           // [N x To x Do x F]
    int64_t total;      // N To Do F
    int32_t T, D, To, Do, F, kh, kw, sh, sw, pt, pl;
};

__global__ __launch_bounds__(256) void conv2d_same_kernel(ConvArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % a.F);
        int64_t rest = i / a.F;
        const int fo = (int)(rest % a.Do);
        rest /= a.Do;
        const int to = (int)(rest % a.To);
        const int64_t nn = rest / a.To;
        const float* __restrict__ x = a.X + nn * a.T * a.D;
        float s = a.bias ? a.bias[c] : 0.f;
        for (int ki = 0; ki < a.kh; ++ki) {
            const int t = to * a.sh + ki - a.pt;
            if (t < 0 || t >= a.T) continue;
            for (int kj = 0; kj < a.kw; ++kj) {
                const int f = fo * a.sw + kj - a.pl;
                if (f < 0 || f >= a.D) continue;
                s = fmaf(x[t * a.D + f], a.K[(ki * a.kw + kj) * a.F + c], s);
            }
        }
        a.Y[i] = s;
    }
}

// K.l2_normalize (d_vector.py:243-246): y = x / sqrt(max(sum x^2, eps)); one wave per row, lane-strided partial sums joined by a butterfly
// (the same order for every row of a given width); a NaN stays a NaN through the maximum, as numpy's does
__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* __restrict__ X, int64_t N, int32_t d, float eps, float* __restrict__ Y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float* x = X + row * d;
    float s = 0.f;
    for (int k = lane; k < d; k += 64) s = fmaf(x[k], x[k], s);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    const float inv = 1.f / sqrtf(nanmax(s, eps));
    for (int k = lane; k < d; k += 64) Y[row * d + k] = x[k] * inv;
}

static int gru_check_shape(const char* who, int32_t d_in, int32_t units) {
    if (d_in < 1 || units < 1) SSP_FAIL(SSP_ERR_INVALID, "%s: d_in and units must be >= 1", who);
    if (units % 16 != 0 || units > GRU_MAXH) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: units must be a multiple of 16 up to %d (got %d)", who, GRU_MAXH, units);
    if (d_in > GRU_MAXD) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: d_in up to %d (got %d)", who, GRU_MAXD, d_in);
    return SSP_OK;
}

template <int MODE, int ACT>
static int gru_launch(const GruStepArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)(((a.N + 63) / 64) * ((a.H + 127) / 128)));  // (N <= 2^30 / T rows per slab: far below 2^31 workgroups)
    hipLaunchKernelGGL((gru_step_kernel<MODE, ACT>), grid, dim3(256), 0, s, a);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

}  // namespace ssp

struct ssp_gru {
    ssp_ctx* ctx = nullptr;
    int32_t d_in = 0, units = 0, act = 0, reset_after = 0;
    bool has_rbias = false;
    size_t cap = (size_t)2 << 30;  // workspace cap of one call, bytes
    int64_t last_slab = 0;         // chunks per slab of the last forward call
    ssp::DevBuf img;               // packed U
    ssp::DevBuf Wt;                // [3H x d_in]: the kernel transposed, ssp_dense_forward's operand
    ssp::DevBuf bin;               // [3H] input bias (zero without one)
    ssp::DevBuf brec;              // [3H] recurrent bias (reset_after = 1 with a bias)
    ssp::DevBuf seq, zrh;          // workspace: output sequence when the caller's cannot be written in place, z | r.h [2 n H]; the projection
                                   // [n T 3H] is ctx->gru_proj
};

using namespace ssp;

extern "C" {

int ssp_gru_create(ssp_ctx* ctx, int32_t d_in, int32_t units, const float* W, const float* U, const float* bias,
                   int32_t recurrent_activation, int32_t reset_after, ssp_gru** out) try {
    if (!out) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_create: null out");
    *out = nullptr;
    if (!W || !U) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_create: null kernel");
    if (recurrent_activation != 0 && recurrent_activation != 1)
        SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_create: recurrent_activation must be 0 (hard_sigmoid) or 1 (sigmoid)");
    if (reset_after != 0 && reset_after != 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_create: reset_after must be 0 or 1");
    SSP_TRY(gru_check_shape("ssp_gru_create", d_in, units));
    SSP_TRY(use_ctx(ctx));
    const int H = units, H3 = 3 * units, KG = H / 16, JT = (KG + 1) / 2 * 2;
    std::vector<float> image((size_t)JT * KG * 768, 0.f), wt((size_t)H3 * d_in), bi(H3, 0.f), br;
    // image[(((j KG + g) 3 + q) 64 + lane) 4 + r] = U[16 g + 4 (lane >> 4) + r][q H + 16 j + (lane & 15)]; the tile that pads an odd
    // count to an even one stays zero
    for (int j = 0; j < KG; ++j)
        for (int g = 0; g < KG; ++g)
            for (int q = 0; q < 3; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    for (int r = 0; r < 4; ++r)
                        image[((((size_t)j * KG + g) * 3 + q) * 64 + lane) * 4 + r] =
                            U[(size_t)(16 * g + 4 * (lane >> 4) + r) * H3 + q * H + 16 * j + (lane & 15)];
    for (int k = 0; k < d_in; ++k)
        for (int c = 0; c < H3; ++c) wt[(size_t)c * d_in + k] = W[(size_t)k * H3 + c];
    if (bias) {
        for (int c = 0; c < H3; ++c) bi[c] = bias[c];
        if (reset_after) br.assign(bias + H3, bias + 2 * H3);
    }
    HandleBuild<ssp_gru> m(ctx, "ssp_gru_create");
    m->d_in = d_in;
    m->units = units;
    m->act = recurrent_activation;
    m->reset_after = reset_after;
    m->has_rbias = !br.empty();
    int rc = upload(m, m->img, image);
    if (rc == SSP_OK) rc = upload(m, m->Wt, wt);
    if (rc == SSP_OK) rc = upload(m, m->bin, bi);
    if (rc == SSP_OK) rc = upload(m, m->brec, br);  // (empty without a recurrent bias)
    return m.commit(rc, out);
}
SSP_CREATE_GUARD("ssp_gru_create")

int ssp_gru_destroy(ssp_gru* gru) { return destroy_handle(gru); }

int ssp_gru_set_workspace(ssp_gru* gru, size_t bytes) {
    if (!gru) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_set_workspace: null handle");
    if (bytes == 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_set_workspace: zero bytes");
    gru->cap = bytes;
    return SSP_OK;
}

int ssp_gru_last_slab(const ssp_gru* gru, int64_t* chunks_out) {
    if (!gru || !chunks_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_last_slab: null argument");
    *chunks_out = gru->last_slab;
    return SSP_OK;
}

int ssp_gru_forward(ssp_gru* gru, const float* X, int64_t N, int32_t T, float* seq_out, float* mean_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_gru_forward");
    if (!gru) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_forward: null handle");
    if (kernel_ms) *kernel_ms = 0.f;
    SSP_TRY(check_where(where, "ssp_gru_forward"));
    if (N < 0 || T < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_forward: N >= 0 and T >= 1");
    if (N == 0) return SSP_OK;
    if (!X) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_forward: null input");
    if (!seq_out && !mean_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_forward: no output asked for");
    ssp_ctx* ctx = gru->ctx;
    SSP_TRY(use_ctx(ctx));
    hipStream_t s = ctx->stream;
    const int H = gru->units, D = gru->d_in;
    const int64_t H3 = 3 * (int64_t)H;
    // the sequence is written in place when the caller's buffer is a 16-byte aligned device array
    const bool in_place = where == SSP_DEVICE && seq_out && (reinterpret_cast<uintptr_t>(seq_out) & 15) == 0;
    const size_t per_chunk = ((size_t)T * H3 + (in_place ? 0 : (size_t)T * H) + (gru->reset_after ? 0 : 2 * (size_t)H)) * sizeof(float);
    int64_t slab = (int64_t)(gru->cap / per_chunk);
    const int64_t max_rows = (int64_t)1 << 30;  // rows of one projection GEMM
    if (slab > max_rows / T) slab = max_rows / T;
    if (slab < 1) slab = 1;  // (one chunk is the least a call can run: the cap then yields)
    if (slab > N) slab = N;
    gru->last_slab = slab;
    SSP_TRY(ctx->gru_proj.reserve((size_t)slab * T * H3 * sizeof(float)));
    if (!in_place) SSP_TRY(gru->seq.reserve((size_t)slab * T * H * sizeof(float)));
    if (!gru->reset_after) SSP_TRY(gru->zrh.reserve((size_t)slab * 2 * H * sizeof(float)));
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    for (int64_t c0 = 0; c0 < N; c0 += slab) {
        const int64_t n = N - c0 < slab ? N - c0 : slab;
        StageScope st(ctx, where);  // (of this slab)
        const float* dX = st.in(X + c0 * T * D, (size_t)n * T * D * sizeof(float));
        float* dM = st.out(mean_out ? mean_out + c0 * H : nullptr, (size_t)n * H * sizeof(float));
        SSP_TRY(st.status());
        float* P = ctx->gru_proj.as<float>();
        float* S = in_place ? seq_out + c0 * T * H : gru->seq.as<float>();
        SSP_TRY(ssp_dense_forward(ctx, dX, n * T, D, gru->Wt.as<float>(), gru->bin.as<float>(), (int32_t)H3, 0, P, SSP_DEVICE, nullptr));
        GruStepArgs a{};
        a.img = gru->img.as<float>();
        a.rbias = gru->has_rbias ? gru->brec.as<float>() : nullptr;
        a.zbuf = gru->zrh.as<float>();
        a.rhbuf = gru->reset_after ? nullptr : gru->zrh.as<float>() + (size_t)n * H;
        a.N = n;
        a.ld_seq = (int64_t)T * H;
        a.ld_p = (int64_t)T * H3;
        a.H = H;
        for (int t = 0; t < T; ++t) {
            a.proj = P + (int64_t)t * H3;
            a.hout = S + (int64_t)t * H;
            a.hprev = t ? S + (int64_t)(t - 1) * H : nullptr;
            if (gru->reset_after) {
                a.hsrc = a.hprev;
                a.ld_src = a.ld_seq;
                if (gru->act) SSP_TRY((gru_launch<0, 1>(a, s)));
                else SSP_TRY((gru_launch<0, 0>(a, s)));
            } else {
                a.hsrc = a.hprev;
                a.ld_src = a.ld_seq;
                if (gru->act) SSP_TRY((gru_launch<1, 1>(a, s)));
                else SSP_TRY((gru_launch<1, 0>(a, s)));
                a.hsrc = t ? a.rhbuf : nullptr;  // (t = 0: r . 0)
                a.ld_src = H;
                SSP_TRY((gru_launch<2, 0>(a, s)));
            }
        }
        if (dM) {
            hipLaunchKernelGGL(gru_time_mean_kernel, dim3((unsigned)((n * H + 255) / 256)), dim3(256), 0, s, S, n, T, H, dM);
            SSP_HIP(hipGetLastError());
            SSP_TRY(st.copy_back());
        }
        if (seq_out && !in_place)
            SSP_HIP(hipMemcpyAsync(seq_out + c0 * T * H, S, (size_t)n * T * H * sizeof(float),
                                   where == SSP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
        SSP_TRY(st.finish());  // (the slab's wait; its staging is given back at the end of the scope)
    }
    SSP_TRY(tm.stop(s, kernel_ms));
    return SSP_OK;
}

int ssp_conv2d_same_forward(ssp_ctx* ctx, const float* X, int64_t N, int32_t T, int32_t D, const float* K, const float* bias, int32_t kh,
                            int32_t kw, int32_t F, int32_t sh, int32_t sw, float* Y, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_conv2d_same_forward");
    if (kernel_ms) *kernel_ms = 0.f;
    if (N < 0 || T < 1 || D < 1 || kh < 1 || kw < 1 || F < 1 || sh < 1 || sw < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_conv2d_same_forward: bad shape");
    SSP_TRY(check_where(where, "ssp_conv2d_same_forward"));
    if (kh > CONV_MAXK || kw > CONV_MAXK || F > CONV_MAXF || sh > 2 || sw > 2)
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_conv2d_same_forward: kernels up to %d x %d, up to %d filters, strides 1 or 2", CONV_MAXK, CONV_MAXK, CONV_MAXF);
    if ((int64_t)T * D > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_conv2d_same_forward: T x D above 2^31");
    if (!K || (N > 0 && (!X || !Y))) SSP_FAIL(SSP_ERR_INVALID, "ssp_conv2d_same_forward: null array");
    SSP_TRY(use_ctx(ctx));
    if (N == 0) return SSP_OK;
    ConvArgs a{};
    a.T = T, a.D = D, a.F = F, a.kh = kh, a.kw = kw, a.sh = sh, a.sw = sw;
    a.To = (T + sh - 1) / sh;
    a.Do = (D + sw - 1) / sw;
    const int ph = (a.To - 1) * sh + kh - T, pw = (a.Do - 1) * sw + kw - D;  // TensorFlow's `same`: the smaller half goes in front
    a.pt = (ph > 0 ? ph : 0) / 2;
    a.pl = (pw > 0 ? pw : 0) / 2;
    a.total = N * a.To * a.Do * F;
    hipStream_t s = ctx->stream;
    StageScope st(ctx, where);
    a.X = st.in(X, (size_t)N * T * D * sizeof(float));
    a.K = st.in(K, (size_t)kh * kw * F * sizeof(float));
    a.bias = st.in(bias, (size_t)F * sizeof(float));
    a.Y = st.out(Y, (size_t)a.total * sizeof(float));
    SSP_TRY(st.status());
    const int64_t blocks = (a.total + 255) / 256;
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    hipLaunchKernelGGL(conv2d_same_kernel, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(256), 0, s, a);
    SSP_HIP(hipGetLastError());
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}

int ssp_l2_normalize(ssp_ctx* ctx, const float* X, int64_t N, int32_t d, float eps, float* Y, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_l2_normalize");
    if (kernel_ms) *kernel_ms = 0.f;
    if (N < 0 || d < 1 || !(eps >= 0.f)) SSP_FAIL(SSP_ERR_INVALID, "ssp_l2_normalize: bad shape or eps");
    SSP_TRY(check_where(where, "ssp_l2_normalize"));
    if (N > 0 && (!X || !Y)) SSP_FAIL(SSP_ERR_INVALID, "ssp_l2_normalize: null array");
    if ((N + 3) / 4 > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_l2_normalize: too many rows for one launch");
    SSP_TRY(use_ctx(ctx));
    if (N == 0) return SSP_OK;
    hipStream_t s = ctx->stream;
    StageScope st(ctx, where);
    const float* dX = st.in(X, (size_t)N * d * sizeof(float));
    float* dY = st.out(Y, (size_t)N * d * sizeof(float));
    SSP_TRY(st.status());
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    hipLaunchKernelGGL(l2_normalize_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, dX, N, d, eps, dY);
    SSP_HIP(hipGetLastError());
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}

}  // extern "C"
