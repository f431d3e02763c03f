// Training of the reference's recurrent d-vector network (d_vector.py:271-294 nn_model.inference_lstm: ONE LSTM(128) :274 over the (98, 13)
// chunk, Dense(n_class) softmax :278 on the last hidden state, categorical cross-entropy and Adam(lr=1e-4) :281-284, spk.fit(batch_size
// 128, epochs 50) :289-290) as a chain of launches on the ctx stream: recurrent forward with a stash, Dense head, softmax cross-entropy,
// backward through time, the weight gradients as GEMMs over the stash, Adam.  All fp32, every product on v_mfma_f32_16x16x4_f32.
//   * the inference kernel (lstm.hip) gives one wave 16 sequences and ALL hidden tiles and streams the weights per step; a batch of 128
//     is then two workgroups.  Here a workgroup owns 16 sequences (the MFMA's columns) and each of its waves ONE hidden tile of 16 units
//     x 4 gates: units / 16 waves, 8 workgroups x 8 waves at the reference shape
//   * a wave's slice of [W; U] — (16 ceil(d_in / 16) + units) x 64 floats, 16 registers per lane and 16-k group, 144 at the reference
//     shape — is loaded ONCE from the master weights (Keras layout) and stays in registers for all T steps (two waves per SIMD: 256
//     registers each)
//   * the B operand [x_t | h_{t-1}] of the 16 sequences lives in LDS, double buffered: per step every wave multiplies its slice against
//     it, updates the cells of its own units in registers (the four gates of a unit meet in one lane, as in lstm.hip), writes its 16
//     units of h_t into the other buffer, and ONE barrier ends the step.  x_{t+1} is loaded (gathered through the epoch's order, X is
//     never permuted) while the products of step t run
//   * the stash is time-major, row t Bn + b: the gathered x_t, h_t, c_t and the four gate activations; the backward kernel overwrites the
//     gate activations with dz in place, so that dW = Xs^T dZ, dU = H[0 .. T-2]^T dZ[1 .. T-1] and db are plain GEMMs with K = T Bn
//     (dnn_train.hip's mode 2: K in fixed quarters over four waves, added in wave order)
//   * backward through time is the same decomposition in reverse: a wave keeps dh and dc of its 16 units in registers and its 16 rows of U
//     (the A operand of dh_{t-1} = dz U^T, 16 units / 16 x 16 registers) resident; per step it forms dz of its units from the stash, writes
//     it to LDS and to the stash, barrier, multiplies the workgroup's dz against its rows of U, barrier
//   * no floating-point atomic: a sequence is one MFMA column, every sum over rows has a fixed partition and order
#include <cmath>
#include <vector>

#include "common.hpp"
#include "nn_device.hpp"
#include "trainer_core.hpp"

namespace ssp {

constexpr int LT_MAXH = 128, LT_MAXD = 64, LT_MAXT = 1024, LT_MAXB = 1024, LT_MAXC = 4096;

struct LtFwdArgs {
    const float* X;      // [rows x T x D]
    const int64_t* idx;  // rows of this batch (nullable = 0 .. Bn - 1)
    const float* W;      // [D x 4H]
    const float* U;      // [H x 4H]
    const float* bias;   // [4H] (zeros when the layer has none)
    float* Xs;           // stash [T Bn x D]
    float* Hs;           // stash [T Bn x H]
    float* Cs;           // stash [T Bn x H]
    float* Gs;           // stash [T Bn x 4H]: i | f | g | o
    float* hlast;        // [Bn x H] (the variant without stash)
    int32_t Bn, T, D, dT, H, act;
};

// x elements a thread moves per step: the x block is addressed as 16 sequences x 64, the workgroup has at least max(1, KG - 4) waves
constexpr int lt_emax(int KG) { return (16 + (KG > 5 ? KG - 4 : 1) - 1) / (KG > 5 ? KG - 4 : 1); }

// KG = ceil(D / 16) + H / 16 groups of 16 k; blockDim.x = 64 (H / 16)
// (KG - 1 waves at the most, eight from KG = 9 on: the register budget of the small instances is not cut to the large ones')
template <int KG, bool STASH>
__global__ __launch_bounds__(64 * (KG - 1 < 8 ? KG - 1 : 8)) void lt_fwd_kernel(LtFwdArgs a) {
    constexpr int OPW = 16 * KG + 4;  // (row stride off a multiple of the banks)
    constexpr int EMAX = lt_emax(KG);
    __shared__ __attribute__((aligned(16))) float op[2][16][OPW];  // [x_t padded to 16 dT | h_{t-1}] of the 16 sequences
    __shared__ __attribute__((aligned(16))) float s_bias[4 * LT_MAXH];
    __shared__ int64_t s_row[16];
    // the widest instance (d_in > 48 with 128 units: 192 weight registers) keeps its first x group in LDS instead, in operand order
    constexpr int LG = KG >= 12 ? 1 : 0;
    __shared__ __attribute__((aligned(16))) float wl[LG ? 8 * 4 * 64 * 4 : 4];
    const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, kq = lane >> 4;
    const int D = a.D, dT = a.dT, H = a.H, T = a.T, Bn = a.Bn;
    const int H4 = 4 * H;
    const int b0 = blockIdx.x * 16;
    const int u0 = 16 * wave + 4 * kq;  // this lane's four units
    const bool valid = b0 + n < Bn;

    // this wave's slice of [W; U]: lane (kq, m) register (g, q, r) = row 16 g + 4 kq + r, column q H + 16 wave + m
    float w[KG][4][4];
#pragma unroll
    for (int g = 0; g < KG; ++g) {
        const bool isx = g < dT;
        const float* src = isx ? a.W : a.U;
        const int kb = 16 * (isx ? g : g - dT) + 4 * kq;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {  // (unconditional loads off a uniform base: a row beyond D reads row 0 and is zeroed)
                const bool ok = !isx || kb + r < D;
                const float v = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(src) +
                                                                (uint32_t)(((ok ? kb + r : 0) * H4 + q * H + 16 * wave + n) * 4));
                if (g < LG)
                    wl[((wave * 4 + q) * 64 + lane) * 4 + r] = ok ? v : 0.f;
                else
                    w[g][q][r] = ok ? v : 0.f;
            }
    }
    for (int i = tid; i < 2 * 16 * OPW; i += nthr) (&op[0][0][0])[i] = 0.f;
    for (int i = tid; i < H4; i += nthr) s_bias[i] = a.bias[i];
    if (tid < 16) s_row[tid] = b0 + tid < Bn ? (a.idx ? a.idx[b0 + tid] : (int64_t)(b0 + tid)) * T * D : -1;
    __syncthreads();

    auto load_x = [&](int t, float (&xr)[EMAX]) {
#pragma unroll
        for (int i = 0; i < EMAX; ++i) {
            const int e = tid + i * nthr;
            const int xn = (e >> 6) & 15, k = e & 63;
            const int64_t row = s_row[xn];
            xr[i] = (e < 1024 && k < D && row >= 0 && t < T) ? a.X[row + (int64_t)t * D + k] : 0.f;
        }
    };
    auto store_x = [&](int t, int buf, const float (&xr)[EMAX]) {
#pragma unroll
        for (int i = 0; i < EMAX; ++i) {
            const int e = tid + i * nthr;
            const int xn = (e >> 6) & 15, k = e & 63;
            if (e < 1024 && k < 16 * dT) op[buf][xn][k] = xr[i];
            if (STASH && e < 1024 && k < D && b0 + xn < Bn && t < T) {  // (a uniform 64-bit base per step, a 32-bit offset per lane)
                char* xs = reinterpret_cast<char*>(a.Xs + (int64_t)t * Bn * D);
                *reinterpret_cast<float*>(xs + (uint32_t)(((b0 + xn) * D + k) * 4)) = xr[i];
            }
        }
    };
    {
        float x0[EMAX];
        load_x(0, x0);
        store_x(0, 0, x0);
    }
    __syncthreads();

    f32x4 c = {0.f, 0.f, 0.f, 0.f}, h = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1;
        float xn[EMAX];
        load_x(t + 1, xn);  // in flight behind this step's products
        f32x4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = *reinterpret_cast<const f32x4*>(&s_bias[q * H + u0]);
#pragma unroll
        for (int g = 0; g < KG; ++g) {
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(&op[cur][n][16 * g + 4 * kq]);
            if (g < LG) {
                f32x4 wq[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) wq[q] = *reinterpret_cast<const f32x4*>(&wl[((wave * 4 + q) * 64 + lane) * 4]);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wq[q][r], b4[r], acc[q], 0, 0, 0);
                continue;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[g][q][r], b4[r], acc[q], 0, 0, 0);
        }
        f32x4 gi, gf, gg, go;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (a.act == 0) {
                gi[r] = hard_sigm(acc[0][r]);
                gf[r] = hard_sigm(acc[1][r]);
                go[r] = hard_sigm(acc[3][r]);
            } else {
                gi[r] = sigm(acc[0][r]);
                gf[r] = sigm(acc[1][r]);
                go[r] = sigm(acc[3][r]);
            }
            gg[r] = tanh_hw(acc[2][r]);
            c[r] = gf[r] * c[r] + gi[r] * gg[r];
            h[r] = go[r] * tanh_hw(c[r]);
        }
        *reinterpret_cast<f32x4*>(&op[cur ^ 1][n][16 * dT + u0]) = h;
        store_x(t + 1, cur ^ 1, xn);
        if (STASH && valid) {  // (a uniform 64-bit base per step, a 32-bit offset per lane: max_batch 4 H floats stay below 2^32 bytes)
            const int64_t trow = (int64_t)t * Bn;
            char* gp = reinterpret_cast<char*>(a.Gs + trow * H4) + (uint32_t)(((b0 + n) * H4 + u0) * 4);
            const uint32_t oh = (uint32_t)(((b0 + n) * H + u0) * 4);
            *reinterpret_cast<f32x4*>(gp) = gi;
            *reinterpret_cast<f32x4*>(gp + 4 * H) = gf;
            *reinterpret_cast<f32x4*>(gp + 8 * H) = gg;
            *reinterpret_cast<f32x4*>(gp + 12 * H) = go;
            *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(a.Cs + trow * H) + oh) = c;
            *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(a.Hs + trow * H) + oh) = h;
        }
        __syncthreads();  // h_t and x_{t+1} are complete; every wave has read buffer `cur`
    }
    if (!STASH && valid) *reinterpret_cast<f32x4*>(a.hlast + (int64_t)(b0 + n) * H + u0) = h;
}

struct LtBwdArgs {
    const float* U;   // [H x 4H]
    const float* dH;  // [Bn x H] the gradient at the last hidden state
    float* Gs;        // [T Bn x 4H] gate activations in, dz out
    const float* Cs;  // [T Bn x H]
    int32_t Bn, T, H, act;
};

// HT = H / 16 waves; wave j keeps dh, dc of units 16 j .. 16 j + 15 and rows 16 j .. 16 j + 15 of U
template <int HT>
__global__ __launch_bounds__(64 * HT) void lt_bwd_kernel(LtBwdArgs a) {
    constexpr int H = 16 * HT, H4 = 64 * HT, ZW = H4 + 4;
    __shared__ __attribute__((aligned(16))) float dzs[16][ZW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, kq = lane >> 4;
    const int T = a.T, Bn = a.Bn;
    const int b0 = blockIdx.x * 16;
    const int u0 = 16 * wave + 4 * kq;
    const bool valid = b0 + n < Bn;

    // lane (kq, m) register (g, r) = U[16 wave + m][16 g + 4 kq + r]
    f32x4 uw[4 * HT];
#pragma unroll
    for (int g = 0; g < 4 * HT; ++g) uw[g] = *reinterpret_cast<const f32x4*>(a.U + (int64_t)(16 * wave + n) * H4 + 16 * g + 4 * kq);

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 dh = valid ? *reinterpret_cast<const f32x4*>(a.dH + (int64_t)(b0 + n) * H + u0) : zero;
    f32x4 dc = zero;
    f32x4 gi = zero, gf = zero, gg = zero, go = zero, ct = zero, cp = zero;
    auto load = [&](int t, f32x4& i_, f32x4& f_, f32x4& g_, f32x4& o_, f32x4& cp_) {
        i_ = f_ = g_ = o_ = cp_ = zero;
        if (valid) {
            const int64_t row = (int64_t)t * Bn + b0 + n;
            const float* gp = a.Gs + row * H4 + u0;
            i_ = *reinterpret_cast<const f32x4*>(gp);
            f_ = *reinterpret_cast<const f32x4*>(gp + H);
            g_ = *reinterpret_cast<const f32x4*>(gp + 2 * H);
            o_ = *reinterpret_cast<const f32x4*>(gp + 3 * H);
            if (t > 0) cp_ = *reinterpret_cast<const f32x4*>(a.Cs + (row - Bn) * H + u0);
        }
    };
    load(T - 1, gi, gf, gg, go, cp);
    if (valid) ct = *reinterpret_cast<const f32x4*>(a.Cs + ((int64_t)(T - 1) * Bn + b0 + n) * H + u0);

    for (int t = T - 1; t >= 0; --t) {
        f32x4 zi, zf, zg, zo;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float tc = tanh_hw(ct[r]);
            const float d_o = dh[r] * tc;
            const float d_c = dc[r] + dh[r] * go[r] * (1.f - tc * tc);
            float si, sf, so;
            if (a.act == 0) {
                si = dgate<0>(gi[r]);
                sf = dgate<0>(gf[r]);
                so = dgate<0>(go[r]);
            } else {
                si = dgate<1>(gi[r]);
                sf = dgate<1>(gf[r]);
                so = dgate<1>(go[r]);
            }
            zi[r] = d_c * gg[r] * si;
            zf[r] = d_c * cp[r] * sf;
            zg[r] = d_c * gi[r] * (1.f - gg[r] * gg[r]);
            zo[r] = d_o * so;
            dc[r] = d_c * gf[r];
        }
        *reinterpret_cast<f32x4*>(&dzs[n][u0]) = zi;
        *reinterpret_cast<f32x4*>(&dzs[n][H + u0]) = zf;
        *reinterpret_cast<f32x4*>(&dzs[n][2 * H + u0]) = zg;
        *reinterpret_cast<f32x4*>(&dzs[n][3 * H + u0]) = zo;
        if (valid) {
            float* gp = a.Gs + ((int64_t)t * Bn + b0 + n) * H4 + u0;
            *reinterpret_cast<f32x4*>(gp) = zi;
            *reinterpret_cast<f32x4*>(gp + H) = zf;
            *reinterpret_cast<f32x4*>(gp + 2 * H) = zg;
            *reinterpret_cast<f32x4*>(gp + 3 * H) = zo;
        }
        __syncthreads();  // the workgroup's dz_t is complete
        if (t > 0) {
            ct = cp;  // c_{t-1}
            load(t - 1, gi, gf, gg, go, cp);  // in flight behind the products
            f32x4 acc = zero;
#pragma unroll
            for (int g = 0; g < 4 * HT; ++g) {
                const f32x4 b4 = *reinterpret_cast<const f32x4*>(&dzs[n][16 * g + 4 * kq]);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(uw[g][r], b4[r], acc, 0, 0, 0);
            }
            dh = acc;
        }
        __syncthreads();  // every wave has read dz_t
    }
}

template <int KG, bool STASH>
static int lt_fwd_launch(const LtFwdArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((lt_fwd_kernel<KG, STASH>), dim3((unsigned)((a.Bn + 15) / 16)), dim3((unsigned)(4 * a.H)), 0, s, a);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

template <bool STASH>
static int lt_fwd(const LtFwdArgs& a, hipStream_t s) {
    switch (a.dT + a.H / 16) {
        case 2: return lt_fwd_launch<2, STASH>(a, s);
        case 3: return lt_fwd_launch<3, STASH>(a, s);
        case 4: return lt_fwd_launch<4, STASH>(a, s);
        case 5: return lt_fwd_launch<5, STASH>(a, s);
        case 6: return lt_fwd_launch<6, STASH>(a, s);
        case 7: return lt_fwd_launch<7, STASH>(a, s);
        case 8: return lt_fwd_launch<8, STASH>(a, s);
        case 9: return lt_fwd_launch<9, STASH>(a, s);
        case 10: return lt_fwd_launch<10, STASH>(a, s);
        case 11: return lt_fwd_launch<11, STASH>(a, s);
        case 12: return lt_fwd_launch<12, STASH>(a, s);
    }
    SSP_FAIL(SSP_ERR_UNSUPPORTED, "lstm trainer: no forward kernel instance");
}

template <int HT>
static int lt_bwd_launch(const LtBwdArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((lt_bwd_kernel<HT>), dim3((unsigned)((a.Bn + 15) / 16)), dim3(64 * HT), 0, s, a);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

static int lt_bwd(const LtBwdArgs& a, hipStream_t s) {
    switch (a.H / 16) {
        case 1: return lt_bwd_launch<1>(a, s);
        case 2: return lt_bwd_launch<2>(a, s);
        case 3: return lt_bwd_launch<3>(a, s);
        case 4: return lt_bwd_launch<4>(a, s);
        case 5: return lt_bwd_launch<5>(a, s);
        case 6: return lt_bwd_launch<6>(a, s);
        case 7: return lt_bwd_launch<7>(a, s);
        case 8: return lt_bwd_launch<8>(a, s);
    }
    SSP_FAIL(SSP_ERR_UNSUPPORTED, "lstm trainer: no backward kernel instance");
}

}  // namespace ssp

struct ssp_lstm_trainer : ssp::TrainerCore {
    int32_t D = 0, H = 0, T = 0, act = 0;
    bool has_b = false, has_bd = false;
    int64_t off[5] = {0, 0, 0, 0, 0}, len[5] = {0, 0, 0, 0, 0};  // W U B WD BD in the flat buffers
    ssp::DevBuf Xs, Hs, Cs, Gs;        // the stash of one step, time-major
    ssp::DevBuf hlast, dH, logits;     // evaluate's last hidden state; the gradient at it; the logits and the gradient at them (in place)
};

using namespace ssp;

namespace {

float* lt_p(ssp_lstm_trainer* tr, const DevBuf& b, int tensor) { return b.as<float>() + tr->off[tensor]; }

constexpr int LT_LAUNCHES = 9;  // of one step: the slots of ssp_lstm_trainer_step_times, in launch order

// recurrent forward of rows [row0, row0 + Bn) (of idx when given), then the Dense head's logits
int lt_forward(ssp_lstm_trainer* tr, const float* X, const int64_t* idx, int64_t row0, int Bn, bool stash, hipStream_t s, StepMarks* mk = nullptr) {
    LtFwdArgs a{};
    a.X = idx ? X : X + row0 * tr->T * tr->D;
    a.idx = idx ? idx + row0 : nullptr;
    a.W = lt_p(tr, tr->P, 0), a.U = lt_p(tr, tr->P, 1), a.bias = lt_p(tr, tr->P, 2);
    a.Xs = tr->Xs.as<float>(), a.Hs = tr->Hs.as<float>(), a.Cs = tr->Cs.as<float>(), a.Gs = tr->Gs.as<float>();
    a.hlast = tr->hlast.as<float>();
    a.Bn = Bn, a.T = tr->T, a.D = tr->D, a.dT = (tr->D + 15) / 16, a.H = tr->H, a.act = tr->act;
    SSP_TRY(stash ? lt_fwd<true>(a, s) : lt_fwd<false>(a, s));
    SSP_TRY(mark(mk, s, 0));
    const float* hl = stash ? tr->Hs.as<float>() + (int64_t)(tr->T - 1) * Bn * tr->H : tr->hlast.as<float>();
    return dt_launch_gemm(0, hl, lt_p(tr, tr->P, 3), tr->logits.as<float>(), nullptr, Bn, tr->n_class, tr->H, tr->H,
                          tr->has_bd ? lt_p(tr, tr->P, 4) : nullptr, nullptr, s);
}

int lt_backward(ssp_lstm_trainer* tr, int Bn, hipStream_t s, StepMarks* mk = nullptr) {
    const int H = tr->H, H4 = 4 * tr->H, T = tr->T;
    const float* hl = tr->Hs.as<float>() + (int64_t)(T - 1) * Bn * H;
    float* dlog = tr->logits.as<float>();
    // the Dense head: dWd = h_T^T dlogits, dbd; dh_T = dlogits Wd^T
    SSP_TRY(dt_launch_gemm(2, hl, dlog, lt_p(tr, tr->G, 3), nullptr, H, tr->n_class, Bn, H, nullptr, tr->has_bd ? lt_p(tr, tr->G, 4) : nullptr, s));
    SSP_TRY(mark(mk, s, 3));
    SSP_TRY(dt_launch_gemm(1, dlog, lt_p(tr, tr->P, 3), tr->dH.as<float>(), nullptr, Bn, H, tr->n_class, tr->n_class, nullptr, nullptr, s));
    SSP_TRY(mark(mk, s, 4));
    LtBwdArgs b{};
    b.U = lt_p(tr, tr->P, 1), b.dH = tr->dH.as<float>(), b.Gs = tr->Gs.as<float>(), b.Cs = tr->Cs.as<float>();
    b.Bn = Bn, b.T = T, b.H = H, b.act = tr->act;
    SSP_TRY(lt_bwd(b, s));
    SSP_TRY(mark(mk, s, 5));
    // dW = Xs^T dZ and db over the T Bn rows; dU = H_prev^T dZ over the rows of t >= 1 (h_{-1} = 0)
    const float* dZ = tr->Gs.as<float>();
    SSP_TRY(dt_launch_gemm(2, tr->Xs.as<float>(), dZ, lt_p(tr, tr->G, 0), nullptr, tr->D, H4, T * Bn, tr->D, nullptr,
                           tr->has_b ? lt_p(tr, tr->G, 2) : nullptr, s));
    SSP_TRY(mark(mk, s, 6));
    SSP_TRY(dt_launch_gemm(2, tr->Hs.as<float>(), dZ + (int64_t)Bn * H4, lt_p(tr, tr->G, 1), nullptr, H, H4, (T - 1) * Bn, H, nullptr, nullptr, s));
    return mark(mk, s, 7);
}

// one training step on rows [row0, row0 + Bn) (of idx when given): nine launches
int lt_step(ssp_lstm_trainer* tr, const float* X, const int32_t* labels, const int64_t* idx, int64_t row0, int Bn, int64_t slot, float lr,
            hipStream_t s, StepMarks* mk = nullptr) {
    SSP_TRY(mark(mk, s, -1));
    SSP_TRY(lt_forward(tr, X, idx, row0, Bn, true, s, mk));
    SSP_TRY(mark(mk, s, 1));
    SSP_TRY(tr->loss(labels, idx, row0, Bn, true, slot, tr->logits.as<float>(), s));
    SSP_TRY(mark(mk, s, 2));
    SSP_TRY(lt_backward(tr, Bn, s, mk));
    SSP_TRY(tr->adam(lr, s));
    return mark(mk, s, 8);
}

}  // namespace

extern "C" {

int ssp_lstm_trainer_create(ssp_ctx* ctx, int32_t d_in, int32_t units, int32_t n_class, int32_t T, int32_t recurrent_activation, const float* W,
                            const float* U, const float* bias, const float* Wd, const float* bd, int32_t max_batch, ssp_lstm_trainer** out) try {
    if (!out) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_trainer_create: null out");
    *out = nullptr;
    if (!W || !U || !Wd) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_trainer_create: null kernel");
    if (recurrent_activation != 0 && recurrent_activation != 1)
        SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_trainer_create: recurrent_activation must be 0 (hard_sigmoid) or 1 (sigmoid)");
    if (d_in < 1 || units < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_trainer_create: d_in and units must be >= 1");
    if (units % 16 != 0 || units > LT_MAXH)
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_lstm_trainer_create: units must be a multiple of 16 up to %d (got %d)", LT_MAXH, units);
    if (d_in > LT_MAXD) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_lstm_trainer_create: d_in up to %d (got %d)", LT_MAXD, d_in);
    if (T < 1 || T > LT_MAXT) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_lstm_trainer_create: T in [1, %d] (got %d)", LT_MAXT, T);
    if (n_class < 2 || n_class > LT_MAXC) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_lstm_trainer_create: n_class in [2, %d] (got %d)", LT_MAXC, n_class);
    if (max_batch < 1 || max_batch > LT_MAXB) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_lstm_trainer_create: max_batch in [1, %d] (got %d)", LT_MAXB, max_batch);
    SSP_TRY(use_ctx(ctx));
    HandleBuild<ssp_lstm_trainer> tr(ctx, "ssp_lstm_trainer_create");
    tr->D = d_in, tr->H = units, tr->n_class = n_class, tr->T = T, tr->act = recurrent_activation, tr->max_batch = max_batch;
    tr->has_b = bias != nullptr, tr->has_bd = bd != nullptr;
    const int64_t H4 = 4 * (int64_t)units;
    tr->len[0] = d_in * H4, tr->len[1] = units * H4, tr->len[2] = H4, tr->len[3] = (int64_t)units * n_class, tr->len[4] = n_class;
    int64_t np = 0;
    for (int i = 0; i < 5; ++i) tr->off[i] = np, np += tr->len[i];
    std::vector<float> flat((size_t)np, 0.f);
    const float* src[5] = {W, U, bias, Wd, bd};
    for (int i = 0; i < 5; ++i)
        if (src[i]) memcpy(flat.data() + tr->off[i], src[i], (size_t)tr->len[i] * sizeof(float));
    const size_t rows = (size_t)T * max_batch;
    int rc = tr->Xs.alloc(rows * d_in * sizeof(float));
    if (rc == SSP_OK) rc = tr->Hs.alloc(rows * units * sizeof(float));
    if (rc == SSP_OK) rc = tr->Cs.alloc(rows * units * sizeof(float));
    if (rc == SSP_OK) rc = tr->Gs.alloc(rows * H4 * sizeof(float));
    if (rc == SSP_OK) rc = tr->hlast.alloc((size_t)max_batch * units * sizeof(float));
    if (rc == SSP_OK) rc = tr->dH.alloc((size_t)max_batch * units * sizeof(float));
    if (rc == SSP_OK) rc = tr->logits.alloc((size_t)max_batch * n_class * sizeof(float));
    if (rc == SSP_OK) rc = tr->alloc_state(tr, flat);
    return tr.commit(rc, out);
}
SSP_CREATE_GUARD("ssp_lstm_trainer_create")

int ssp_lstm_trainer_destroy(ssp_lstm_trainer* trainer) { return destroy_handle(trainer); }

int ssp_lstm_trainer_epoch(ssp_lstm_trainer* trainer, const float* X, const int32_t* labels, int64_t N, const int64_t* order, int32_t batch_size,
                           float lr, double* loss_sum, int64_t* n_correct, int where, float* kernel_ms) {
    ssp_lstm_trainer* tr = trainer;
    return trainer_epoch("ssp_lstm_trainer_epoch", tr, X, tr ? (int64_t)tr->T * tr->D : 0, labels, N, order, batch_size, lr, loss_sum, n_correct, where,
                         kernel_ms, [&](const float* dX, const int32_t* dL, const int64_t* dO, int64_t row0, int Bn, int64_t slot, hipStream_t s) {
                             return lt_step(tr, dX, dL, dO, row0, Bn, slot, lr, s);
                         });
}

int ssp_lstm_trainer_evaluate(ssp_lstm_trainer* trainer, const float* X, const int32_t* labels, int64_t N, double* loss_sum, int64_t* n_correct,
                              int where, float* kernel_ms) {
    ssp_lstm_trainer* tr = trainer;
    return trainer_evaluate("ssp_lstm_trainer_evaluate", tr, X, tr ? (int64_t)tr->T * tr->D : 0, labels, N, loss_sum, n_correct, where, kernel_ms,
                            [&](const float* dX, const int32_t* dL, int64_t row0, int Bn, int64_t slot, hipStream_t s) {
                                SSP_TRY(lt_forward(tr, dX, nullptr, row0, Bn, false, s));
                                return tr->loss(dL, nullptr, row0, Bn, false, slot, tr->logits.as<float>(), s);
                            });
}

int ssp_lstm_trainer_step_times(ssp_lstm_trainer* trainer, const float* X, const int32_t* labels, int32_t batch_size, float lr, float* ms_out) {
    const char* who = "ssp_lstm_trainer_step_times";
    ssp_lstm_trainer* tr = trainer;
    StepMarks mk;
    SSP_TRY(trainer_timed_step(who, tr, X, labels, batch_size, lr, ms_out, mk,
                               [&](hipStream_t s, StepMarks* m) { return lt_step(tr, X, labels, nullptr, 0, batch_size, 0, lr, s, m); }));
    if (mk.slot.size() != LT_LAUNCHES + 1) SSP_FAIL(SSP_ERR_HIP, "%s: %d marks", who, (int)mk.slot.size());
    return mk.times(ms_out, LT_LAUNCHES);
}

int ssp_lstm_trainer_read(ssp_lstm_trainer* trainer, int32_t what, int32_t tensor, float* out) {
    if (!trainer || !out) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_trainer_read: null argument");
    ssp_lstm_trainer* tr = trainer;
    if (what < 0 || what > 3) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_trainer_read: what must be SSP_LSTM_PARAM .. SSP_LSTM_V");
    if (tensor < 0 || tensor > 4) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_trainer_read: tensor must be SSP_LSTM_W .. SSP_LSTM_BD");
    if ((tensor == 2 && !tr->has_b) || (tensor == 4 && !tr->has_bd)) SSP_FAIL(SSP_ERR_INVALID, "ssp_lstm_trainer_read: the network has no such bias");
    return tr->read_flat("ssp_lstm_trainer_read", what, tr->off[tensor], tr->len[tensor], out);
}

int ssp_lstm_trainer_steps(const ssp_lstm_trainer* trainer, int64_t* t) { return trainer_steps("ssp_lstm_trainer_steps", trainer, t); }

}  // extern "C"
