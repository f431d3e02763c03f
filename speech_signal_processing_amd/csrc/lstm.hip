// Forward pass of the reference's recurrent d-vector network (d_vector.py:271-294 inference_lstm: ONE LSTM(128) over the (98, 13) MFCC
// matrix of a 1-second chunk, last hidden state = the embedding; spkModel.predict at d_vector.py:297-299, 330-331, 347-348) as one
// kernel for a ragged batch of sequences.  Keras' cell, gate blocks i | f | c | o:
//     z = x_t W + h_{t-1} U + b;  i = s(z_i), f = s(z_f), g = tanh(z_c), o = s(z_o);  c_t = f c_{t-1} + i g;  h_t = o tanh(c_t)
// with s = hard_sigmoid (clip(0.2 z + 0.5, 0, 1)) or the logistic sigmoid.
//   * wave = 16 sequences, v_mfma_f32_16x16x4_f32 (exact fp32): gate units are the MFMA rows, sequences the columns, K = [x_t | h_{t-1}]
//   * the B operand lives in registers: lane (kq = l >> 4, n = l & 15) holds x[n][16 g + 4 kq + r] in register 4 g + r of the x block and
//     h[n][16 t + 4 kq + r] in register 4 t + r of the h block
//   * the packed weight image orders the 4H gate rows by hidden tile: for tile j (hidden units 16 j .. 16 j + 15) the four gates are four
//     accumulators of 4 registers, and lane (kq, n) register r of each is unit 16 j + 4 kq + r of sequence n — the i, f, c, o
//     pre-activations of one unit meet in one lane and register index, the cell update is element-wise, and the new h is already
//     register 4 j + r of the next step's B operand.  c and h never leave the registers over the T steps
//   * the weights (288 KiB at D = 13, H = 128: more than the LDS) stream per time step, one hidden tile (36 KiB) at a time, through a
//     two-slot LDS ring by LDS-DMA shared by the workgroup's 4 waves; tile g + 1 is in flight while tile g is multiplied
//   * a lane whose sequence has ended keeps its h and c (a select, no branch) while its workgroup finishes its longest sequence;
//     MFMA columns are independent, so a sequence's bits do not depend on its neighbours
#include <cstdlib>
#include <vector>

#include "common.hpp"
#include "handle.hpp"
#include "nn_device.hpp"

namespace ssp {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

constexpr int LS_MAXH = 128;  // widest state the registers hold
constexpr int LS_MAXD = 64;   // widest input

struct LstmArgs {
    const float* feats;    // [frames x D] row-major
    const int64_t* off;    // [n_seq + 1] frame offsets
    const float* img;      // [HT tiles][dT + HT groups][4 gates][64 lanes][4 r] packed weights, then [4][16 HT] bias
    float* h_out;          // [n_seq x H]
    int64_t n_seq;
    int32_t D, dT, H;
};

// HT = hidden tiles of 16 units (1, 2, 4, 8); ACT = 0 hard_sigmoid | 1 sigmoid
template <int HT, int ACT>
__global__ __launch_bounds__(256, 2) void lstm_kernel(LstmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int dT = a.dT;
    const int TF = (dT + HT) * 1024;                   // floats per weight tile
    float* ring = reinterpret_cast<float*>(smem);      // [2][TF]
    float* s_bias = ring + 2 * TF;                     // [4][16 HT]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, kq = lane >> 4;
    const int64_t seq0 = (int64_t)blockIdx.x * 64;
    const int64_t seq = seq0 + wave * 16 + n;          // this lane's sequence

    // the workgroup runs for its longest sequence (every wave computes the same maximum over the workgroup's 64)
    int T_blk;
    {
        const int64_t s = seq0 + lane;
        int64_t l64 = s < a.n_seq ? a.off[s + 1] - a.off[s] : 0;
        int l = (int)l64;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) l = max(l, __shfl_xor(l, m));
        T_blk = __builtin_amdgcn_readfirstlane(l);
    }
    int64_t row0 = 0;
    int len = 0;
    if (seq < a.n_seq) {
        row0 = a.off[seq];
        len = (int)(a.off[seq + 1] - row0);
    }

    auto stage = [&](int j, int slot) {  // hidden tile j -> ring slot: (dT + HT) x 4 pieces of 1 KiB, one per wave and instruction
        const float* src = a.img + (size_t)j * TF;
        float* dst = ring + slot * TF;
        for (int p = wave; p < (dT + HT) * 4; p += 4)
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src + p * 256 + lane * 4), (lds_ptr_t)(dst + p * 256), 16, 0, 0);
    };
    auto load_x = [&](int t, float (&xr)[16]) {  // x[seq][t][16 g + 4 kq + r] -> register 4 g + r (zero beyond D and beyond the sequence)
        const bool on = t < len;
        const float* __restrict__ p = a.feats + (row0 + t) * a.D;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f4u v = {0.f, 0.f, 0.f, 0.f};
            const int k = 16 * g + 4 * kq;
            if (g < dT && on) {
                if (k + 3 < a.D) {
                    v = *reinterpret_cast<const f4u*>(p + k);
                } else {
                    if (k < a.D) v.x = p[k];
                    if (k + 1 < a.D) v.y = p[k + 1];
                    if (k + 2 < a.D) v.z = p[k + 2];
                }
            }
            xr[4 * g + 0] = v.x;
            xr[4 * g + 1] = v.y;
            xr[4 * g + 2] = v.z;
            xr[4 * g + 3] = v.w;
        }
    };

    float hb[4 * HT], cs[4 * HT], xb[16];
#pragma unroll
    for (int i = 0; i < 4 * HT; ++i) hb[i] = cs[i] = 0.f;

    if (T_blk > 0) {
        stage(0, 0);
        for (int i = tid; i < 64 * HT; i += 256) s_bias[i] = a.img[(size_t)HT * TF + i];
        load_x(0, xb);
        __syncthreads();  // bias table + tile 0 (the barrier drains the LDS-DMA)
    }

    int slot = 0;
    for (int t = 0; t < T_blk; ++t) {
        float xn[16], nb[4 * HT];
        load_x(t + 1, xn);  // next step's inputs, in flight behind this step's products
        const bool on = t < len;
#pragma unroll
        for (int j = 0; j < HT; ++j) {
            // tile g + 1 of the (step, tile) stream into the slot tile g - 1 left at the last barrier
            if (j + 1 < HT)
                stage(j + 1, slot ^ 1);
            else if (t + 1 < T_blk)
                stage(0, slot ^ 1);
            const float* wcur = ring + slot * TF;
            f32x4 acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = *reinterpret_cast<const f32x4*>(s_bias + q * 16 * HT + 16 * j + 4 * kq);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (g < dT) {
                    f32x4 w[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) w[q] = *reinterpret_cast<const f32x4*>(wcur + ((g * 4 + q) * 64 + lane) * 4);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[q][r], xb[4 * g + r], acc[q], 0, 0, 0);
                }
            }
            const float* wh = wcur + dT * 1024;
#pragma unroll
            for (int g = 0; g < HT; ++g) {
                f32x4 w[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = *reinterpret_cast<const f32x4*>(wh + ((g * 4 + q) * 64 + lane) * 4);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[q][r], hb[4 * g + r], acc[q], 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float gi, gf, go;
                if (ACT == 0) {
                    gi = hard_sigm(acc[0][r]);
                    gf = hard_sigm(acc[1][r]);
                    go = hard_sigm(acc[3][r]);
                } else {
                    gi = sigm(acc[0][r]);
                    gf = sigm(acc[1][r]);
                    go = sigm(acc[3][r]);
                }
                const float gg = tanh_hw(acc[2][r]);
                const float cn = gf * cs[4 * j + r] + gi * gg;
                const float hn = go * tanh_hw(cn);
                cs[4 * j + r] = on ? cn : cs[4 * j + r];
                nb[4 * j + r] = on ? hn : hb[4 * j + r];
            }
            __syncthreads();  // tile g is consumed by every wave; tile g + 1 has landed
            slot ^= 1;
        }
#pragma unroll
        for (int i = 0; i < 4 * HT; ++i) hb[i] = nb[i];
#pragma unroll
        for (int i = 0; i < 16; ++i) xb[i] = xn[i];
    }

    if (seq < a.n_seq) {
        float* y = a.h_out + seq * a.H;
        const bool vec = (reinterpret_cast<uintptr_t>(a.h_out) & 15) == 0;  // (H is a multiple of 16: rows keep the base's alignment)
#pragma unroll
        for (int j = 0; j < HT; ++j) {
            const int u = 16 * j + 4 * kq;
            if (u < a.H) {  // (tiles beyond H are padding: zero weights, zero state)
                if (vec) {
                    *reinterpret_cast<f32x4*>(y + u) = f32x4{hb[4 * j], hb[4 * j + 1], hb[4 * j + 2], hb[4 * j + 3]};
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[u + r] = hb[4 * j + r];
                }
            }
        }
    }
}

static inline int lstm_tiles(int units) { return units <= 16 ? 1 : units <= 32 ? 2 : units <= 64 ? 4 : 8; }

static int lstm_check_shape(const char* who, int32_t d_in, int32_t units) {
    if (d_in < 1 || units < 1) SSP_FAIL(SSP_ERR_INVALID, "%s: d_in and units must be >= 1", who);
    if (units % 16 != 0 || units > LS_MAXH) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: units must be a multiple of 16 up to %d (got %d)", who, LS_MAXH, units);
    if (d_in > LS_MAXD) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: d_in up to %d (got %d)", who, LS_MAXD, d_in);
    return SSP_OK;
}

template <int HT, int ACT>
static int lstm_launch(const LstmArgs& a, size_t lds, unsigned blocks, hipStream_t s) {
    if (lds > 64 * 1024)
        SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_kernel<HT, ACT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((lstm_kernel<HT, ACT>), dim3(blocks), dim3(256), lds, s, a);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

}  // namespace ssp

struct ssp_lstm {
    ssp_ctx* ctx = nullptr;
    int32_t d_in = 0, units = 0, act = 0, HT = 0, dT = 0;
    ssp::DevBuf img;
};

using namespace ssp;

extern "C" {

int ssp_lstm_pack_weights(int32_t d_in, int32_t units, const float* W, const float* U, const float* bias, float* image_out,
                          int64_t* n_floats_out) {
    SSP_TRY(lstm_check_shape("ssp_lstm_pack_weights", d_in, units));
    const int HT = lstm_tiles(units), dT = (d_in + 15) / 16, G = dT + HT;
    const int64_t n_img = (int64_t)HT * G * 1024, n_all = n_img + 64 * HT;
    if (n_floats_out) *n_floats_out = n_all;
    if (!image_out) {
        if (!n_floats_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_pack_weights: nothing to write");
        return SSP_OK;  // (size query)
    }
    if (!W || !U) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_pack_weights: null kernel");
    const int H4 = 4 * units;
    for (int j = 0; j < HT; ++j)
        for (int g = 0; g < G; ++g)
            for (int q = 0; q < 4; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    for (int r = 0; r < 4; ++r) {
                        const int u = 16 * j + (lane & 15);
                        const int k = 16 * (g < dT ? g : g - dT) + 4 * (lane >> 4) + r;
                        float v = 0.f;
                        if (u < units) {
                            if (g < dT) {
                                if (k < d_in) v = W[(size_t)k * H4 + q * units + u];
                            } else if (k < units) {
                                v = U[(size_t)k * H4 + q * units + u];
                            }
                        }
                        image_out[((((size_t)j * G + g) * 4 + q) * 64 + lane) * 4 + r] = v;
                    }
    for (int q = 0; q < 4; ++q)
        for (int u = 0; u < 16 * HT; ++u) image_out[n_img + q * 16 * HT + u] = (bias && u < units) ? bias[q * units + u] : 0.f;
    return SSP_OK;
}

int ssp_lstm_create(ssp_ctx* ctx, int32_t d_in, int32_t units, const float* W, const float* U, const float* bias,
                    int32_t recurrent_activation, ssp_lstm** out) try {
    if (!out) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_create: null out");
    *out = nullptr;
    if (!W || !U) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_create: null kernel");
    if (recurrent_activation != 0 && recurrent_activation != 1)
        SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_create: recurrent_activation must be 0 (hard_sigmoid) or 1 (sigmoid)");
    SSP_TRY(lstm_check_shape("ssp_lstm_create", d_in, units));
    SSP_TRY(use_ctx(ctx));
    int64_t nf = 0;
    SSP_TRY(ssp_lstm_pack_weights(d_in, units, nullptr, nullptr, nullptr, nullptr, &nf));
    std::vector<float> image((size_t)nf);
    SSP_TRY(ssp_lstm_pack_weights(d_in, units, W, U, bias, image.data(), nullptr));
    HandleBuild<ssp_lstm> m(ctx, "ssp_lstm_create");
    m->d_in = d_in;
    m->units = units;
    m->act = recurrent_activation;
    m->HT = lstm_tiles(units);
    m->dT = (d_in + 15) / 16;
    return m.commit(upload(m, m->img, image), out);
}
SSP_CREATE_GUARD("ssp_lstm_create")

int ssp_lstm_destroy(ssp_lstm* lstm) { return destroy_handle(lstm); }

int ssp_lstm_forward(ssp_lstm* lstm, const float* feats, const ssp_segments* frame_seg, float* h_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_lstm_forward");
    if (!lstm) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_forward: null handle");
    if (!frame_seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_forward: null segments");
    ssp_ctx* ctx = lstm->ctx;
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    SSP_TRY(check_where(where, "ssp_lstm_forward"));
    if (frame_seg->ctx && frame_seg->ctx->device != ctx->device) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_forward: the segments live on another device");
    const int64_t n_seq = frame_seg->n;
    if (n_seq == 0) return SSP_OK;
    if (!h_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_forward: null output");
    if (!feats && frame_seg->total() > 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_forward: null features");
    if (frame_seg->max_len() > INT32_MAX || (n_seq + 63) / 64 > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_lstm_forward: batch too large for one launch");
    hipStream_t s = ctx->stream;
    const size_t in_bytes = (size_t)frame_seg->host.back() * lstm->d_in * sizeof(float);
    const size_t out_bytes = (size_t)n_seq * lstm->units * sizeof(float);
    StageScope st(ctx, where);
    const float* dX = st.in(in_bytes ? feats : nullptr, in_bytes);
    float* dY = st.out(h_out, out_bytes);
    SSP_TRY(st.status());
    LstmArgs a{};
    a.feats = dX;
    a.off = frame_seg->dev.as<int64_t>();
    a.img = lstm->img.as<float>();
    a.h_out = dY;
    a.n_seq = n_seq;
    a.D = lstm->d_in;
    a.dT = lstm->dT;
    a.H = lstm->units;
    const size_t lds = (size_t)(2 * (lstm->dT + lstm->HT) * 1024 + 64 * lstm->HT) * sizeof(float);
    const unsigned blocks = (unsigned)((n_seq + 63) / 64);
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    switch (lstm->HT * 2 + lstm->act) {
        case 2: SSP_TRY((lstm_launch<1, 0>(a, lds, blocks, s))); break;
        case 3: SSP_TRY((lstm_launch<1, 1>(a, lds, blocks, s))); break;
        case 4: SSP_TRY((lstm_launch<2, 0>(a, lds, blocks, s))); break;
        case 5: SSP_TRY((lstm_launch<2, 1>(a, lds, blocks, s))); break;
        case 8: SSP_TRY((lstm_launch<4, 0>(a, lds, blocks, s))); break;
        case 9: SSP_TRY((lstm_launch<4, 1>(a, lds, blocks, s))); break;
        case 16: SSP_TRY((lstm_launch<8, 0>(a, lds, blocks, s))); break;
        case 17: SSP_TRY((lstm_launch<8, 1>(a, lds, blocks, s))); break;
        default: SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_lstm_forward: no kernel instance");
    }
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}

}  // extern "C"
