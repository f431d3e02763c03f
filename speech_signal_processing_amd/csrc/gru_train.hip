// Training of the reference's conv + GRU d-vector network (d_vector.py:213-269 nn_model.inference_gru: Conv2D(64, 5x5, strides 2, same,
// l2-regularised kernel) :216-221 -> TimeDistributed(Flatten) :226 -> 3 x GRU(1024, return_sequences) :229-231 -> mean over time :234-237
// -> Dense(512) :240 -> K.l2_normalize :243-246 -> Dense(n_class) softmax :252, categorical cross-entropy, Adam(lr=1e-4), spk.fit(batch
// 128, epochs 50) :264-265) as a chain of launches on the ctx stream.  All fp32, every product on v_mfma_f32_16x16x4_f32, no floating-point
// atomic.  The GRU cell is gru.hip's with reset_after = 0 (stand-alone Keras).
//   * everything of one step is TIME-MAJOR, row t Bn + b: the conv output, the input projection P = x W + b of a layer (ONE GEMM over
//     the To Bn rows, dnn_train.hip's mode 0), the stash h | z | r | hh | r . h_{t-1} per layer, the gate gradients dA = [da_z | da_r |
//     da_h] and the gradient at a layer's input.  A step's slice of any of them is then contiguous, and h_{t-1} is the h stash Bn rows back
//   * time steps are ordered by the stream, two launches per step and direction, as in gru.hip; no grid-wide barrier, no spin
//       forward   gt_fwd_kernel<1>: [z | r] = s(P_zr + h_{t-1} [U_z | U_r]), stashes z, r and r . h_{t-1}
//                 gt_fwd_kernel<2>: hh = tanh(P_h + (r . h_{t-1}) U_h), h_t = z h_{t-1} + (1 - z) hh, stashes hh and h_t
//       backward  gt_bwd_r_kernel:  G = da_h U_h^T; its epilogue forms da_r = G h_{t-1} s'(r) and G . r
//                 gt_bwd_h_kernel:  dh_{t-1} = dh_t z + G . r + [da_z | da_r] [U_z | U_r]^T + the gradient from above; its epilogue forms
//                                   da_h and da_z of step t - 1, which need only the finished dh_{t-1} of the same (sequence, unit)
//   * the tile is made for a batch of 128, not for gru.hip's slabs of thousands of chunks: a wave owns 16 units x 16 sequences (one MFMA
//     tile per gate), a workgroup four waves = 64 units of the same 16 sequences.  128 sequences x 1024 units are 128 workgroups, 512
//     waves, per launch.  An output element sums its K = 1024 (2048 in gt_bwd_h_kernel) in ascending k groups in ONE accumulator, and a
//     sequence is one MFMA column: its bits do not depend on its place in the batch
//   * the forward reads U as gru.hip's packed image (by unit tile and k group: 16-byte loads, 1 KiB per wave and fragment); the image is
//     made from the master weights by gt_pack_kernel at create and again after every Adam launch (3 H^2 floats read and written per
//     layer and step: 24 MiB at H = 1024, against the 12 MiB per step LAUNCH the recurrence reads).  The backward needs U transposed: with
//     the units of h_{t-1} as MFMA rows and the gate columns as k, lane (kq, i) reads U[16 j + i][16 g + 4 kq ..+3] — 16 bytes straight
//     from the master layout, 64 contiguous bytes per row and k group.  No second image
//   * the other gradients once per layer and step as GEMMs over the stash: dW = x^T dA with db (mode 2, K = To Bn), dx = dA W^T (mode 1);
//     dU_zr = h_{t-1}^T [da_z | da_r] and dU_h = (r . h_{t-1})^T da_h write column blocks of the (H, 3H) gradient from column blocks of
//     dA: gt_gemm_tn_kernel, mode 2's loader with row strides for B and C on the same split-K tile (nn_device.hpp)
//   * conv backward (dK, db only): the To Bn Do output positions are cut into 64 fixed chunks, one wave per (tap, chunk, 64 filters), the
//     chunks added in order by a second launch, which also adds the regulariser's 2 lambda K
#include <cmath>
#include <vector>

#include "common.hpp"
#include "nn_device.hpp"
#include "trainer_core.hpp"

namespace ssp {

constexpr int GT_MAXH = 1024, GT_MAXD = 4096, GT_MAXK = 7, GT_MAXF = 256, GT_MAXT = 1024, GT_MAXB = 1024, GT_MAXC = 4096, GT_MAXE = 4096;
constexpr int GT_MAXL = 4;
constexpr int GT_MAXROWS = 1 << 19;           // To max_batch: the rows of one projection GEMM (a 16-row tile per workgroup, 65535 in grid.y)
constexpr int GT_TENSORS = 6 + 3 * GT_MAXL;   // conv_K conv_b | W U b per layer | dense_W dense_b head_W head_b
constexpr int GT_TIMES = 6 + 6 * GT_MAXL;     // ssp_gru_trainer_step_times
constexpr int GT_CCH = 64;                    // chunks of output positions in the conv backward
constexpr size_t GT_WS_CAP = (size_t)4 << 30; // workspace cap, bytes
constexpr float GT_LAMBDA = 0.01f;            // regularizers.l2()'s default factor
constexpr float GT_EPS = 1e-12f;              // K.l2_normalize's epsilon

// acc[q] += sum over g < KG of A_q(g) B(g): lane (kq, i) holds A_q[i][16 g + 4 kq + r] at ap[q] + g astride and B[16 g + 4 kq + r][n] at
// bp + 16 g, r = 0..3 one 16-byte load each.  k ascends in one accumulator per gate.  Two register sets: the loads of group g + 1 are
// issued before the products of group g (the scheduling barriers keep the compiler from sinking them to their first use)
template <int NG>
__device__ __forceinline__ void gt_dot(const float* const (&ap)[NG], int astride, const float* bp, int KG, f32x4 (&acc)[NG]) {
    f32x4 wa[NG], wb[NG], ha, hb;
    auto load = [&](int g, f32x4 (&w)[NG], f32x4& h) {
#pragma unroll
        for (int q = 0; q < NG; ++q) w[q] = *reinterpret_cast<const f32x4*>(ap[q] + (size_t)g * astride);
        h = *reinterpret_cast<const f32x4*>(bp + 16 * g);
    };
    auto mul = [&](const f32x4 (&w)[NG], const f32x4& h) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < NG; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[q][r], h[r], acc[q], 0, 0, 0);
    };
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

struct GtFwdArgs {
    const float* img;    // packed U: [unit tile j][k group g][3 gates][64 lanes][4 r]
    const float* hprev;  // [Bn x H] h_{t-1}; null = zero (t = 0: no product)
    const float* proj;   // [Bn x 3H] this step's slice of the projection
    float *Z, *R, *RH, *HH, *Hout;  // [Bn x H] this step's slices of the stash
    int32_t Bn, H;
};

// MODE 1: z and r, stashing z, r and r . h_{t-1};  MODE 2: the candidate from (r . h_{t-1}) U_h and the state update (ACT unused)
// grid (H / 64 rounded up, Bn / 16 rounded up), 256 threads: wave = unit tile 4 blockIdx.x + wave of sequences 16 blockIdx.y ..+15
template <int MODE, int ACT>
__global__ __launch_bounds__(256) void gt_fwd_kernel(GtFwdArgs a) {
    constexpr int NG = MODE == 1 ? 2 : 1;
    constexpr int Q0 = MODE == 1 ? 0 : 2;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 15, kq = lane >> 4;
    const int H = a.H, KG = H >> 4;
    const int j = blockIdx.x * 4 + wave;
    if (j >= KG) return;  // (no barrier in this kernel)
    const int seq = blockIdx.y * 16 + n;
    const int row = seq < a.Bn ? seq : a.Bn - 1;  // (columns beyond the batch repeat its last row and are never stored)
    f32x4 acc[NG];
#pragma unroll
    for (int q = 0; q < NG; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.hprev) {
        const float* src = MODE == 1 ? a.hprev : a.RH;
        const float* ap[NG];
#pragma unroll
        for (int q = 0; q < NG; ++q) ap[q] = a.img + ((size_t)j * KG * 3 + Q0 + q) * 256 + lane * 4;
        gt_dot<NG>(ap, 768, src + (size_t)row * H + 4 * kq, KG, acc);
    }
    if (seq >= a.Bn) return;
    // accumulator register r of lane (kq, n) = unit 16 j + 4 kq + r of sequence n
    const int u = 16 * j + 4 * kq;
    const size_t o = (size_t)seq * H + u;
    const float* pr = a.proj + (size_t)seq * 3 * H + u;
    f32x4 hp = f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.hprev) hp = *reinterpret_cast<const f32x4*>(a.hprev + o);
    if (MODE == 1) {
        const f32x4 xz = *reinterpret_cast<const f32x4*>(pr), xr = *reinterpret_cast<const f32x4*>(pr + H);
        f32x4 z, rg, rh;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            z[r] = gate<ACT>(xz[r] + acc[0][r]);
            rg[r] = gate<ACT>(xr[r] + acc[NG - 1][r]);
            rh[r] = rg[r] * hp[r];
        }
        *reinterpret_cast<f32x4*>(a.Z + o) = z;
        *reinterpret_cast<f32x4*>(a.R + o) = rg;
        *reinterpret_cast<f32x4*>(a.RH + o) = rh;
    } else {
        const f32x4 xh = *reinterpret_cast<const f32x4*>(pr + 2 * H);
        const f32x4 z = *reinterpret_cast<const f32x4*>(a.Z + o);
        f32x4 hh, out;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            hh[r] = tanh_hw(xh[r] + acc[0][r]);
            out[r] = z[r] * hp[r] + (1.f - z[r]) * hh[r];
        }
        *reinterpret_cast<f32x4*>(a.HH + o) = hh;
        *reinterpret_cast<f32x4*>(a.Hout + o) = out;
    }
}

struct GtBwdArgs {
    const float* U;       // [H x 3H] master weights, Keras' layout
    float* dA;            // gt_bwd_r: [Bn x 3H] of step t (da_h in, da_r out);  gt_bwd_h: of the step being finished (da_z, da_h out)
    const float* dAn;     // gt_bwd_h: [Bn x 3H] of step t + 1 (da_z | da_r in); null = the last step: dh is the gradient from above alone
    const float* Zn;      // gt_bwd_h: z of step t + 1
    const float* R;       // gt_bwd_r: r of step t
    const float* Hprev;   // [Bn x H] h of the step before the one whose gates are formed; null = zero
    const float* Z;       // gt_bwd_h: z of the step being finished
    const float* HH;      // gt_bwd_h: hh of the step being finished
    const float* above;   // gt_bwd_h: [Bn x H] the gradient from above at the step being finished
    float* GR;            // [Bn x H] G . r of step t (gt_bwd_r out, gt_bwd_h in)
    float* DH;            // [Bn x H] dh (gt_bwd_h: dh_{t+1} in, dh_t out, element-wise in place)
    int32_t Bn, H;
};

// G = da_h U_h^T of step t; da_r = G h_{t-1} s'(r); G . r.  At t = 0 (Hprev null) h_{-1} = 0: da_r = 0 and nothing is multiplied
template <int ACT>
__global__ __launch_bounds__(256) void gt_bwd_r_kernel(GtBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 15, kq = lane >> 4;
    const int H = a.H, KG = H >> 4;
    const int j = blockIdx.x * 4 + wave;
    if (j >= KG) return;
    const int seq = blockIdx.y * 16 + n;
    const int row = seq < a.Bn ? seq : a.Bn - 1;
    f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
    if (a.Hprev) {
        const float* ap[1] = {a.U + (size_t)(16 * j + n) * 3 * H + 2 * H + 4 * kq};
        gt_dot<1>(ap, 16, a.dA + (size_t)row * 3 * H + 2 * H + 4 * kq, KG, acc);
    }
    if (seq >= a.Bn) return;
    const int u = 16 * j + 4 * kq;
    const size_t o = (size_t)seq * H + u;
    f32x4 dr = f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.Hprev) {
        const f32x4 rg = *reinterpret_cast<const f32x4*>(a.R + o), hp = *reinterpret_cast<const f32x4*>(a.Hprev + o);
        f32x4 gr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            dr[r] = acc[0][r] * hp[r] * dgate<ACT>(rg[r]);
            gr[r] = acc[0][r] * rg[r];
        }
        *reinterpret_cast<f32x4*>(a.GR + o) = gr;
    }
    *reinterpret_cast<f32x4*>(a.dA + (size_t)seq * 3 * H + H + u) = dr;
}

// dh = dh_{t+1} z_{t+1} + G . r + [da_z | da_r]_{t+1} [U_z | U_r]^T + above (the last step: above alone), then da_h and da_z of this step
template <int ACT>
__global__ __launch_bounds__(256) void gt_bwd_h_kernel(GtBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 15, kq = lane >> 4;
    const int H = a.H, KG = H >> 4;
    const int j = blockIdx.x * 4 + wave;
    if (j >= KG) return;
    const int seq = blockIdx.y * 16 + n;
    const int row = seq < a.Bn ? seq : a.Bn - 1;
    f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
    if (a.dAn) {
        const float* ap[1] = {a.U + (size_t)(16 * j + n) * 3 * H + 4 * kq};
        gt_dot<1>(ap, 16, a.dAn + (size_t)row * 3 * H + 4 * kq, 2 * KG, acc);
    }
    if (seq >= a.Bn) return;
    const int u = 16 * j + 4 * kq;
    const size_t o = (size_t)seq * H + u;
    f32x4 dh = *reinterpret_cast<const f32x4*>(a.above + o);
    if (a.dAn) {
        const f32x4 dn = *reinterpret_cast<const f32x4*>(a.DH + o), zn = *reinterpret_cast<const f32x4*>(a.Zn + o),
                    gr = *reinterpret_cast<const f32x4*>(a.GR + o);
#pragma unroll
        for (int r = 0; r < 4; ++r) dh[r] = ((dn[r] * zn[r] + gr[r]) + acc[0][r]) + dh[r];
    }
    const f32x4 z = *reinterpret_cast<const f32x4*>(a.Z + o), hh = *reinterpret_cast<const f32x4*>(a.HH + o);
    f32x4 hp = f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.Hprev) hp = *reinterpret_cast<const f32x4*>(a.Hprev + o);
    f32x4 dz, dc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        dc[r] = dh[r] * (1.f - z[r]) * (1.f - hh[r] * hh[r]);
        dz[r] = dh[r] * (hp[r] - hh[r]) * dgate<ACT>(z[r]);
    }
    float* da = a.dA + (size_t)seq * 3 * H + u;
    *reinterpret_cast<f32x4*>(da) = dz;
    *reinterpret_cast<f32x4*>(da + 2 * H) = dc;
    *reinterpret_cast<f32x4*>(a.DH + o) = dh;
}

// image[(((j KG + g) 3 + q) 64 + lane) 4 + r] = U[16 g + 4 (lane >> 4) + r][q H + 16 j + (lane & 15)]   (gru.hip's layout)
__global__ __launch_bounds__(256) void gt_pack_kernel(const float* __restrict__ U, float* __restrict__ img, int32_t H) {
    const int KG = H >> 4;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)KG * KG * 768) return;
    const int r = (int)(e & 3), lane = (int)((e >> 2) & 63);
    int64_t rest = e >> 8;
    const int q = (int)(rest % 3);
    rest /= 3;
    const int g = (int)(rest % KG), j = (int)(rest / KG);
    img[e] = U[(int64_t)(16 * g + 4 * (lane >> 4) + r) * 3 * H + q * H + 16 * j + (lane & 15)];
}

// C[M x N] (row stride ldc) = A^T B, A [K x M] (row stride lda), B [K x N] (row stride ldb): dnn_train.hip's mode 2 with strides — the
// split-K tile of nn_device.hpp (splitk_range, splitk_walk, splitk_sum) behind a strided loader
struct GtGemmArgs {
    const float *A, *B;
    float* C;
    int32_t M, N, K;
    int64_t lda, ldb, ldc;
};

__global__ __launch_bounds__(256) void gt_gemm_tn_kernel(GtGemmArgs a) {
    __shared__ __attribute__((aligned(16))) float red[4][256];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, kq = lane >> 4;
    const int m0 = blockIdx.y * 16, n0 = blockIdx.x * 16;
    const int M = a.M, N = a.N, K = a.K;
    const SplitK ks = splitk_range(K, wave);
    const int kend = ks.kend;
    const bool m_ok = m0 + i < M, n_ok = n0 + i < N;
    auto load = [&](int kb, float (&av)[4], float (&bv)[4]) {
        const int k = kb + 4 * kq;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            av[r] = (m_ok && k + r < kend) ? a.A[(int64_t)(k + r) * a.lda + m0 + i] : 0.f;
            bv[r] = (n_ok && k + r < kend) ? a.B[(int64_t)(k + r) * a.ldb + n0 + i] : 0.f;
        }
    };
    const SplitKElem el = splitk_sum(red, splitk_walk(ks, load), tid, wave);
    if (m0 + el.row < M && n0 + el.col < N) a.C[(int64_t)(m0 + el.row) * a.ldc + n0 + el.col] = el.v;
}

// Conv2D, one input channel, channels last, TensorFlow's `same` (gru.hip's conv2d_same_kernel) on the rows of this batch, gathered through
// the epoch's order, TIME-MAJOR out: Y[((t Bn + b) Do + fo) F + c]
struct GtConvArgs {
    const float* X;      // [rows x T x D]
    const int64_t* idx;  // rows of this batch (nullable = 0 .. Bn - 1)
    const float* K;      // [kh x kw x F]
    const float* bias;   // [F] or null
    float* Y;            // forward out
    const float* dY;     // backward in, Y's layout
    float* part;         // backward: [(kh kw + 1) x GT_CCH x F] partial sums
    int64_t total;       // To Bn Do F
    int32_t Bn, T, D, To, Do, F, kh, kw, sh, sw, pt, pl;
};

__global__ __launch_bounds__(256) void gt_conv_fwd_kernel(GtConvArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.total) return;
    const int c = (int)(i % a.F);
    int64_t rest = i / a.F;
    const int fo = (int)(rest % a.Do);
    rest /= a.Do;
    const int b = (int)(rest % a.Bn);
    const int to = (int)(rest / a.Bn);
    const float* __restrict__ x = a.X + (a.idx ? a.idx[b] : (int64_t)b) * a.T * a.D;
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

// grid (kh kw + 1, GT_CCH, F / 64 rounded up), 64 threads: tap blockIdx.x (the last one is the bias: x = 1) over the positions of chunk
// blockIdx.y in ascending order, one filter per lane
__global__ __launch_bounds__(64) void gt_conv_bwd_kernel(GtConvArgs a) {
    const int tap = blockIdx.x, chunk = blockIdx.y;
    const int c = blockIdx.z * 64 + threadIdx.x;
    const int taps = a.kh * a.kw;
    const int ki = tap / a.kw, kj = tap - ki * a.kw;
    const int64_t P = (int64_t)a.To * a.Bn * a.Do;
    const int64_t per = (P + GT_CCH - 1) / GT_CCH;
    const int64_t p0 = chunk * per, p1 = p0 + per < P ? p0 + per : P;
    float s = 0.f;
    for (int64_t p = p0; p < p1; ++p) {
        float x = 1.f;
        if (tap < taps) {
            const int fo = (int)(p % a.Do);
            const int64_t rest = p / a.Do;
            const int b = (int)(rest % a.Bn), to = (int)(rest / a.Bn);
            const int t = to * a.sh + ki - a.pt, f = fo * a.sw + kj - a.pl;
            if (t < 0 || t >= a.T || f < 0 || f >= a.D) continue;
            x = a.X[(a.idx ? a.idx[b] : (int64_t)b) * a.T * a.D + t * a.D + f];
        }
        if (c < a.F) s = fmaf(x, a.dY[p * a.F + c], s);
    }
    if (c < a.F) a.part[((int64_t)tap * GT_CCH + chunk) * a.F + c] = s;
}

// the chunks in order; dK gains 2 lambda K
__global__ __launch_bounds__(256) void gt_conv_sum_kernel(const float* __restrict__ part, const float* __restrict__ K, float* __restrict__ dK,
                                                          float* __restrict__ db, int32_t taps, int32_t F, float lambda2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (taps + 1) * F) return;
    const int tap = i / F, c = i - tap * F;
    float s = 0.f;
    for (int ch = 0; ch < GT_CCH; ++ch) s += part[((int64_t)tap * GT_CCH + ch) * F + c];
    if (tap < taps)
        dK[i] = s + lambda2 * K[i];
    else if (db)
        db[c] = s;
}

// *slot += coef sum K^2: 256 strided partial sums, added in order (one workgroup)
__global__ __launch_bounds__(256) void gt_reg_kernel(const float* __restrict__ K, int32_t n, float coef, float* __restrict__ slot) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s = fmaf(K[i], K[i], s);
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = red[0];
        for (int i = 1; i < 256; ++i) t += red[i];
        *slot += coef * t;
    }
}

// mean over time of a time-major sequence, t ascending (gru.hip's gru_time_mean_kernel), and its backward dseq_t = dmean / T for every t
__global__ __launch_bounds__(256) void gt_mean_kernel(const float* __restrict__ seq, int32_t Bn, int32_t T, int32_t H, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Bn * H) return;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += seq[(int64_t)t * Bn * H + i];
    out[i] = s / (float)T;
}
__global__ __launch_bounds__(256) void gt_mean_bwd_kernel(const float* __restrict__ dmean, int32_t n, int32_t T, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = dmean[i] / (float)T;
}

// K.l2_normalize, one wave per row (gru.hip's l2_normalize_kernel), keeping sum x^2 per row; and its backward: with n = sqrt(max(sum x^2,
// eps)), dx = (dy - y (y . dy)) / n where sum x^2 >= eps, dy / n below it
__global__ __launch_bounds__(256) void gt_l2_kernel(const float* __restrict__ X, int32_t N, int32_t d, float* __restrict__ Y, float* __restrict__ ss) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float* x = X + (int64_t)row * d;
    float s = 0.f;
    for (int k = lane; k < d; k += 64) s = fmaf(x[k], x[k], s);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    const float inv = 1.f / sqrtf(fmaxf(s, GT_EPS));
    for (int k = lane; k < d; k += 64) Y[(int64_t)row * d + k] = x[k] * inv;
    if (lane == 0) ss[row] = s;
}
__global__ __launch_bounds__(256) void gt_l2_bwd_kernel(const float* __restrict__ dY, const float* __restrict__ Y, const float* __restrict__ ss,
                                                        int32_t N, int32_t d, float* __restrict__ dX) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float *dy = dY + (int64_t)row * d, *y = Y + (int64_t)row * d;
    float dot = 0.f;
    for (int k = lane; k < d; k += 64) dot = fmaf(y[k], dy[k], dot);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) dot += __shfl_xor(dot, m);
    const float s = ss[row];
    const float inv = 1.f / sqrtf(fmaxf(s, GT_EPS));
    if (!(s >= GT_EPS)) dot = 0.f;
    for (int k = lane; k < d; k += 64) dX[(int64_t)row * d + k] = (dy[k] - y[k] * dot) * inv;
}

}  // namespace ssp

struct ssp_gru_trainer : ssp::TrainerCore {
    int32_t T = 0, D = 0, kh = 0, kw = 0, F = 0, sh = 0, sw = 0, To = 0, Do = 0, pt = 0, pl = 0, d0 = 0;
    int32_t L = 0, H[ssp::GT_MAXL] = {}, E = 0, act = 0, Hmax = 0;
    bool has[ssp::GT_TENSORS] = {};
    int64_t off[ssp::GT_TENSORS] = {}, len[ssp::GT_TENSORS] = {};
    ssp::DevBuf img[ssp::GT_MAXL];              // packed U per layer (forward)
    ssp::DevBuf X0, proj;                       // conv output [To Bn x d0]; the running layer's projection [To Bn x 3H]
    ssp::DevBuf Hs[ssp::GT_MAXL], Zs[ssp::GT_MAXL], Rs[ssp::GT_MAXL], HHs[ssp::GT_MAXL], RHs[ssp::GT_MAXL];  // the stash, [To Bn x H] each
    ssp::DevBuf dA, Dx, GR, DH;                 // [To Bn x 3H]; the gradient at a layer's input [To Bn x max(H, d0)]; [Bn x H] each
    ssp::DevBuf mean, e1, l2s, y, dy, de, dmean, dMT, logits, cpart;
};

using namespace ssp;

namespace {

enum { GT_CONV_K = 0, GT_CONV_B = 1, GT_DENSE_W = 2 + 3 * GT_MAXL, GT_DENSE_B = 3 + 3 * GT_MAXL, GT_HEAD_W = 4 + 3 * GT_MAXL, GT_HEAD_B = 5 + 3 * GT_MAXL };
constexpr int gt_w(int l) { return 2 + 3 * l; }
constexpr int gt_u(int l) { return 3 + 3 * l; }
constexpr int gt_b(int l) { return 4 + 3 * l; }

float* gt_p(ssp_gru_trainer* tr, int tensor) { return tr->P.as<float>() + tr->off[tensor]; }
float* gt_g(ssp_gru_trainer* tr, int tensor) { return tr->G.as<float>() + tr->off[tensor]; }
const float* gt_pb(ssp_gru_trainer* tr, int tensor) { return tr->has[tensor] ? gt_p(tr, tensor) : nullptr; }
float* gt_gb(ssp_gru_trainer* tr, int tensor) { return tr->has[tensor] ? gt_g(tr, tensor) : nullptr; }
int gt_din(const ssp_gru_trainer* tr, int l) { return l ? tr->H[l - 1] : tr->d0; }

GtConvArgs gt_conv_args(ssp_gru_trainer* tr, const float* X, const int64_t* idx, int64_t row0, int Bn) {
    GtConvArgs a{};
    a.X = idx ? X : X + row0 * tr->T * tr->D;
    a.idx = idx ? idx + row0 : nullptr;
    a.K = gt_p(tr, GT_CONV_K);
    a.bias = gt_pb(tr, GT_CONV_B);
    a.Bn = Bn, a.T = tr->T, a.D = tr->D, a.To = tr->To, a.Do = tr->Do, a.F = tr->F;
    a.kh = tr->kh, a.kw = tr->kw, a.sh = tr->sh, a.sw = tr->sw, a.pt = tr->pt, a.pl = tr->pl;
    a.total = (int64_t)tr->To * Bn * tr->d0;
    return a;
}

template <class K, class A>
int gt_launch(K kernel, dim3 grid, dim3 block, hipStream_t s, const A& a) {
    hipLaunchKernelGGL(kernel, grid, block, 0, s, a);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

dim3 gt_grid(int H, int Bn) { return dim3((unsigned)((H + 63) / 64), (unsigned)((Bn + 15) / 16)); }

// forward of rows [row0, row0 + Bn) (of idx when given) up to the logits, stashing what the backward needs
int gt_forward(ssp_gru_trainer* tr, const float* X, const int64_t* idx, int64_t row0, int Bn, hipStream_t s, StepMarks* mk = nullptr) {
    const int To = tr->To;
    const int64_t rows = (int64_t)To * Bn;
    GtConvArgs c = gt_conv_args(tr, X, idx, row0, Bn);
    c.Y = tr->X0.as<float>();
    SSP_TRY(gt_launch(gt_conv_fwd_kernel, dim3((unsigned)((c.total + 255) / 256)), dim3(256), s, c));
    SSP_TRY(mark(mk, s, 0));
    for (int l = 0; l < tr->L; ++l) {
        const int H = tr->H[l], d_in = gt_din(tr, l);
        const float* in = l ? tr->Hs[l - 1].as<float>() : tr->X0.as<float>();
        float* P = tr->proj.as<float>();
        SSP_TRY(dt_launch_gemm(0, in, gt_p(tr, gt_w(l)), P, nullptr, (int32_t)rows, 3 * H, d_in, d_in, gt_pb(tr, gt_b(l)), nullptr, s));
        SSP_TRY(mark(mk, s, 6 + 6 * l));
        GtFwdArgs a{};
        a.img = tr->img[l].as<float>();
        a.Bn = Bn, a.H = H;
        for (int t = 0; t < To; ++t) {
            const size_t o = (size_t)t * Bn * H;
            a.hprev = t ? tr->Hs[l].as<float>() + o - (size_t)Bn * H : nullptr;
            a.proj = P + 3 * o;
            a.Z = tr->Zs[l].as<float>() + o, a.R = tr->Rs[l].as<float>() + o, a.RH = tr->RHs[l].as<float>() + o;
            a.HH = tr->HHs[l].as<float>() + o, a.Hout = tr->Hs[l].as<float>() + o;
            if (tr->act) SSP_TRY(gt_launch(gt_fwd_kernel<1, 1>, gt_grid(H, Bn), dim3(256), s, a));
            else SSP_TRY(gt_launch(gt_fwd_kernel<1, 0>, gt_grid(H, Bn), dim3(256), s, a));
            SSP_TRY(gt_launch(gt_fwd_kernel<2, 0>, gt_grid(H, Bn), dim3(256), s, a));
        }
        SSP_TRY(mark(mk, s, 6 + 6 * l + 1));
    }
    const int Hl = tr->H[tr->L - 1];
    hipLaunchKernelGGL(gt_mean_kernel, dim3((unsigned)((Bn * Hl + 255) / 256)), dim3(256), 0, s, tr->Hs[tr->L - 1].as<float>(), Bn, To, Hl,
                       tr->mean.as<float>());
    SSP_HIP(hipGetLastError());
    SSP_TRY(dt_launch_gemm(0, tr->mean.as<float>(), gt_p(tr, GT_DENSE_W), tr->e1.as<float>(), nullptr, Bn, tr->E, Hl, Hl, gt_pb(tr, GT_DENSE_B), nullptr, s));
    hipLaunchKernelGGL(gt_l2_kernel, dim3((unsigned)((Bn + 3) / 4)), dim3(256), 0, s, tr->e1.as<float>(), Bn, tr->E, tr->y.as<float>(), tr->l2s.as<float>());
    SSP_HIP(hipGetLastError());
    SSP_TRY(dt_launch_gemm(0, tr->y.as<float>(), gt_p(tr, GT_HEAD_W), tr->logits.as<float>(), nullptr, Bn, tr->n_class, tr->E, tr->E, gt_pb(tr, GT_HEAD_B), nullptr, s));
    return mark(mk, s, 1);
}

// cross-entropy of the batch into its slot, then the regulariser's Bn lambda sum K^2 on top
int gt_loss(ssp_gru_trainer* tr, const int32_t* labels, const int64_t* idx, int64_t row0, int Bn, bool grad, int64_t slot, hipStream_t s) {
    SSP_TRY(tr->loss(labels, idx, row0, Bn, grad, slot, tr->logits.as<float>(), s));
    hipLaunchKernelGGL(gt_reg_kernel, dim3(1), dim3(256), 0, s, gt_p(tr, GT_CONV_K), (int32_t)tr->len[GT_CONV_K], (float)Bn * GT_LAMBDA,
                       tr->slot_loss.as<float>() + slot);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

int gt_gemm_tn(const float* A, const float* B, float* C, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, hipStream_t s) {
    GtGemmArgs g{};
    g.A = A, g.B = B, g.C = C, g.M = M, g.N = N, g.K = K, g.lda = lda, g.ldb = ldb, g.ldc = ldc;
    return gt_launch(gt_gemm_tn_kernel, dim3((unsigned)((N + 15) / 16), (unsigned)((M + 15) / 16)), dim3(256), s, g);
}

int gt_backward(ssp_gru_trainer* tr, const float* X, const int64_t* idx, int64_t row0, int Bn, hipStream_t s, StepMarks* mk = nullptr) {
    const int To = tr->To, E = tr->E, C = tr->n_class, Hl = tr->H[tr->L - 1];
    const int64_t rows = (int64_t)To * Bn;
    float* dlog = tr->logits.as<float>();
    // the head, the normalisation, Dense(E), the mean
    SSP_TRY(dt_launch_gemm(2, tr->y.as<float>(), dlog, gt_g(tr, GT_HEAD_W), nullptr, E, C, Bn, E, nullptr, gt_gb(tr, GT_HEAD_B), s));
    SSP_TRY(dt_launch_gemm(1, dlog, gt_p(tr, GT_HEAD_W), tr->dy.as<float>(), nullptr, Bn, E, C, C, nullptr, nullptr, s));
    hipLaunchKernelGGL(gt_l2_bwd_kernel, dim3((unsigned)((Bn + 3) / 4)), dim3(256), 0, s, tr->dy.as<float>(), tr->y.as<float>(), tr->l2s.as<float>(), Bn,
                       E, tr->de.as<float>());
    SSP_HIP(hipGetLastError());
    SSP_TRY(dt_launch_gemm(2, tr->mean.as<float>(), tr->de.as<float>(), gt_g(tr, GT_DENSE_W), nullptr, Hl, E, Bn, Hl, nullptr, gt_gb(tr, GT_DENSE_B), s));
    SSP_TRY(dt_launch_gemm(1, tr->de.as<float>(), gt_p(tr, GT_DENSE_W), tr->dmean.as<float>(), nullptr, Bn, Hl, E, E, nullptr, nullptr, s));
    hipLaunchKernelGGL(gt_mean_bwd_kernel, dim3((unsigned)((Bn * Hl + 255) / 256)), dim3(256), 0, s, tr->dmean.as<float>(), Bn * Hl, To, tr->dMT.as<float>());
    SSP_HIP(hipGetLastError());
    SSP_TRY(mark(mk, s, 3));
    float* dA = tr->dA.as<float>();
    float* Dx = tr->Dx.as<float>();
    for (int l = tr->L - 1; l >= 0; --l) {
        const int H = tr->H[l], d_in = gt_din(tr, l);
        const bool top = l == tr->L - 1;
        const size_t bh = (size_t)Bn * H;
        GtBwdArgs a{};
        a.U = gt_p(tr, gt_u(l));
        a.GR = tr->GR.as<float>(), a.DH = tr->DH.as<float>();
        a.Bn = Bn, a.H = H;
        // finish step tp: dh_tp from step tp + 1 (none at the last step), then da_h and da_z of step tp
        auto finish = [&](int tp) {
            GtBwdArgs b = a;
            b.dA = dA + 3 * tp * bh;
            b.dAn = tp + 1 < To ? dA + 3 * (tp + 1) * bh : nullptr;
            b.Zn = tp + 1 < To ? tr->Zs[l].as<float>() + (tp + 1) * bh : nullptr;
            b.Z = tr->Zs[l].as<float>() + tp * bh, b.HH = tr->HHs[l].as<float>() + tp * bh;
            b.Hprev = tp ? tr->Hs[l].as<float>() + (tp - 1) * bh : nullptr;
            b.above = top ? tr->dMT.as<float>() : Dx + tp * bh;
            return tr->act ? gt_launch(gt_bwd_h_kernel<1>, gt_grid(H, Bn), dim3(256), s, b) : gt_launch(gt_bwd_h_kernel<0>, gt_grid(H, Bn), dim3(256), s, b);
        };
        SSP_TRY(finish(To - 1));
        for (int t = To - 1; t >= 0; --t) {
            GtBwdArgs b = a;
            b.dA = dA + 3 * t * bh;
            b.R = tr->Rs[l].as<float>() + t * bh;
            b.Hprev = t ? tr->Hs[l].as<float>() + (t - 1) * bh : nullptr;
            if (tr->act) SSP_TRY(gt_launch(gt_bwd_r_kernel<1>, gt_grid(H, Bn), dim3(256), s, b));
            else SSP_TRY(gt_launch(gt_bwd_r_kernel<0>, gt_grid(H, Bn), dim3(256), s, b));
            if (t) SSP_TRY(finish(t - 1));
        }
        SSP_TRY(mark(mk, s, 6 + 6 * l + 2));
        const float* in = l ? tr->Hs[l - 1].as<float>() : tr->X0.as<float>();
        SSP_TRY(dt_launch_gemm(2, in, dA, gt_g(tr, gt_w(l)), nullptr, d_in, 3 * H, (int32_t)rows, d_in, nullptr, gt_gb(tr, gt_b(l)), s));
        SSP_TRY(mark(mk, s, 6 + 6 * l + 3));
        // dU_zr = h_{t-1}^T [da_z | da_r] over the rows of t >= 1 (h_{-1} = 0); dU_h = (r . h_{t-1})^T da_h (its rows of t = 0 are zero)
        SSP_TRY(gt_gemm_tn(tr->Hs[l].as<float>(), dA + 3 * bh, gt_g(tr, gt_u(l)), H, 2 * H, (To - 1) * Bn, H, 3 * H, 3 * H, s));
        SSP_TRY(gt_gemm_tn(tr->RHs[l].as<float>(), dA + 2 * H, gt_g(tr, gt_u(l)) + 2 * H, H, H, (int)rows, H, 3 * H, 3 * H, s));
        SSP_TRY(mark(mk, s, 6 + 6 * l + 4));
        SSP_TRY(dt_launch_gemm(1, dA, gt_p(tr, gt_w(l)), Dx, nullptr, (int32_t)rows, d_in, 3 * H, 3 * H, nullptr, nullptr, s));
        SSP_TRY(mark(mk, s, 6 + 6 * l + 5));
    }
    GtConvArgs c = gt_conv_args(tr, X, idx, row0, Bn);
    c.dY = Dx, c.part = tr->cpart.as<float>();
    const int taps = tr->kh * tr->kw;
    SSP_TRY(gt_launch(gt_conv_bwd_kernel, dim3((unsigned)(taps + 1), GT_CCH, (unsigned)((tr->F + 63) / 64)), dim3(64), s, c));
    hipLaunchKernelGGL(gt_conv_sum_kernel, dim3((unsigned)(((taps + 1) * tr->F + 255) / 256)), dim3(256), 0, s, tr->cpart.as<float>(), gt_p(tr, GT_CONV_K),
                       gt_g(tr, GT_CONV_K), gt_gb(tr, GT_CONV_B), taps, tr->F, 2.f * GT_LAMBDA);
    SSP_HIP(hipGetLastError());
    return mark(mk, s, 4);
}

int gt_pack(ssp_gru_trainer* tr, hipStream_t s) {
    for (int l = 0; l < tr->L; ++l) {
        const int64_t n = 3 * (int64_t)tr->H[l] * tr->H[l];
        hipLaunchKernelGGL(gt_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, gt_p(tr, gt_u(l)), tr->img[l].as<float>(), tr->H[l]);
        SSP_HIP(hipGetLastError());
    }
    return SSP_OK;
}

// one training step on rows [row0, row0 + Bn) (of idx when given)
int gt_step(ssp_gru_trainer* tr, const float* X, const int32_t* labels, const int64_t* idx, int64_t row0, int Bn, int64_t slot, float lr,
            hipStream_t s, StepMarks* mk = nullptr) {
    SSP_TRY(mark(mk, s, -1));
    SSP_TRY(gt_forward(tr, X, idx, row0, Bn, s, mk));
    SSP_TRY(gt_loss(tr, labels, idx, row0, Bn, true, slot, s));
    SSP_TRY(mark(mk, s, 2));
    SSP_TRY(gt_backward(tr, X, idx, row0, Bn, s, mk));
    SSP_TRY(tr->adam(lr, s));
    SSP_TRY(gt_pack(tr, s));
    return mark(mk, s, 5);
}

}  // namespace

extern "C" {

int ssp_gru_trainer_create(ssp_ctx* ctx, int32_t T, int32_t D, int32_t kh, int32_t kw, int32_t F, int32_t sh, int32_t sw, const float* conv_K,
                           const float* conv_b, int32_t n_gru, const int32_t* units, const float* const* W, const float* const* U,
                           const float* const* bias, int32_t E, const float* dense_W, const float* dense_b, int32_t n_class, const float* head_W,
                           const float* head_b, int32_t recurrent_activation, int32_t reset_after, int32_t max_batch, ssp_gru_trainer** out) try {
    const char* who = "ssp_gru_trainer_create";
    if (!out) SSP_FAIL(SSP_ERR_INVALID, "%s: null out", who);
    *out = nullptr;
    if (!conv_K || !units || !W || !U || !dense_W || !head_W) SSP_FAIL(SSP_ERR_INVALID, "%s: null kernel", who);
    if (recurrent_activation != 0 && recurrent_activation != 1)
        SSP_FAIL(SSP_ERR_INVALID, "%s: recurrent_activation must be 0 (hard_sigmoid) or 1 (sigmoid)", who);
    if (reset_after != 0 && reset_after != 1) SSP_FAIL(SSP_ERR_INVALID, "%s: reset_after must be 0 or 1", who);
    if (reset_after) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: reset_after = 1 is not trained (the forward pass ssp_gru_forward has it)", who);
    if (kh < 1 || kw < 1 || F < 1 || sh < 1 || sw < 1 || D < 1 || E < 1) SSP_FAIL(SSP_ERR_INVALID, "%s: bad shape", who);
    if (kh > GT_MAXK || kw > GT_MAXK || F > GT_MAXF || sh > 2 || sw > 2)
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: kernels up to %d x %d, up to %d filters, strides 1 or 2", who, GT_MAXK, GT_MAXK, GT_MAXF);
    if (n_gru < 1 || n_gru > GT_MAXL) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: 1 to %d GRU layers (got %d)", who, GT_MAXL, n_gru);
    if (T < 1 || T > GT_MAXT) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: T in [1, %d] (got %d)", who, GT_MAXT, T);
    if (D > GT_MAXD) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: D up to %d (got %d)", who, GT_MAXD, D);
    const int To = (T + sh - 1) / sh, Do = (D + sw - 1) / sw;
    const int64_t d0 = (int64_t)Do * F;
    if (d0 > GT_MAXD) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: the first GRU's d_in up to %d (got %lld)", who, GT_MAXD, (long long)d0);
    int Hmax = 0;
    for (int l = 0; l < n_gru; ++l) {
        if (!W[l] || !U[l]) SSP_FAIL(SSP_ERR_INVALID, "%s: null kernel (GRU layer %d)", who, l);
        if (units[l] < 1) SSP_FAIL(SSP_ERR_INVALID, "%s: units must be >= 1", who);
        if (units[l] % 16 != 0 || units[l] > GT_MAXH)
            SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: units must be a multiple of 16 up to %d (got %d)", who, GT_MAXH, units[l]);
        Hmax = units[l] > Hmax ? units[l] : Hmax;
    }
    if (E > GT_MAXE) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: embedding up to %d (got %d)", who, GT_MAXE, E);
    if (n_class < 2 || n_class > GT_MAXC) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: n_class in [2, %d] (got %d)", who, GT_MAXC, n_class);
    if (max_batch < 1 || max_batch > GT_MAXB) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: max_batch in [1, %d] (got %d)", who, GT_MAXB, max_batch);
    if ((int64_t)To * max_batch > GT_MAXROWS)
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: To x max_batch up to %d rows (got %lld)", who, GT_MAXROWS, (long long)To * max_batch);
    // the workspace: conv output, projection, five stashed tensors per layer, dA and the gradient at a layer's input
    const size_t rows = (size_t)To * max_batch;
    const size_t wide = (size_t)(Hmax > d0 ? Hmax : d0);
    size_t ws = rows * ((size_t)d0 + 6 * (size_t)Hmax + wide);
    for (int l = 0; l < n_gru; ++l) ws += rows * 5 * (size_t)units[l];
    ws *= sizeof(float);
    if (ws > GT_WS_CAP)
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: the workspace of one step would be %.2f GiB, above the cap of %.0f GiB: lower max_batch", who,
                 (double)ws / (double)((size_t)1 << 30), (double)GT_WS_CAP / (double)((size_t)1 << 30));
    SSP_TRY(use_ctx(ctx));
    HandleBuild<ssp_gru_trainer> tr(ctx, who);
    tr->T = T, tr->D = D, tr->kh = kh, tr->kw = kw, tr->F = F, tr->sh = sh, tr->sw = sw, tr->To = To, tr->Do = Do, tr->d0 = (int32_t)d0;
    const int ph = (To - 1) * sh + kh - T, pw = (Do - 1) * sw + kw - D;  // TensorFlow's `same`: the smaller half goes in front
    tr->pt = (ph > 0 ? ph : 0) / 2, tr->pl = (pw > 0 ? pw : 0) / 2;
    tr->L = n_gru, tr->E = E, tr->n_class = n_class, tr->act = recurrent_activation, tr->max_batch = max_batch, tr->Hmax = Hmax;
    const float* src[GT_TENSORS] = {};
    src[GT_CONV_K] = conv_K, tr->len[GT_CONV_K] = (int64_t)kh * kw * F;
    src[GT_CONV_B] = conv_b, tr->len[GT_CONV_B] = F;
    for (int l = 0; l < n_gru; ++l) {
        tr->H[l] = units[l];
        const int64_t H3 = 3 * (int64_t)units[l];
        src[gt_w(l)] = W[l], tr->len[gt_w(l)] = (l ? units[l - 1] : d0) * H3;
        src[gt_u(l)] = U[l], tr->len[gt_u(l)] = units[l] * H3;
        src[gt_b(l)] = bias ? bias[l] : nullptr, tr->len[gt_b(l)] = H3;
    }
    src[GT_DENSE_W] = dense_W, tr->len[GT_DENSE_W] = (int64_t)units[n_gru - 1] * E;
    src[GT_DENSE_B] = dense_b, tr->len[GT_DENSE_B] = E;
    src[GT_HEAD_W] = head_W, tr->len[GT_HEAD_W] = (int64_t)E * n_class;
    src[GT_HEAD_B] = head_b, tr->len[GT_HEAD_B] = n_class;
    int64_t np = 0;
    for (int i = 0; i < GT_TENSORS; ++i) {
        tr->has[i] = src[i] != nullptr;
        tr->off[i] = np;
        np += (tr->len[i] + 3) / 4 * 4;  // (every tensor starts on 16 bytes: the step kernels read U with 16-byte loads; the padding stays zero)
    }
    std::vector<float> flat((size_t)np, 0.f);
    for (int i = 0; i < GT_TENSORS; ++i)
        if (src[i]) memcpy(flat.data() + tr->off[i], src[i], (size_t)tr->len[i] * sizeof(float));
    const size_t f4 = sizeof(float), mb = (size_t)max_batch;
    int rc = tr->X0.alloc(rows * d0 * f4);
    if (rc == SSP_OK) rc = tr->proj.alloc(rows * 3 * Hmax * f4);
    if (rc == SSP_OK) rc = tr->dA.alloc(rows * 3 * Hmax * f4);
    if (rc == SSP_OK) rc = tr->Dx.alloc(rows * wide * f4);
    for (int l = 0; l < n_gru && rc == SSP_OK; ++l) {
        const size_t b = rows * units[l] * f4;
        rc = tr->Hs[l].alloc(b);
        if (rc == SSP_OK) rc = tr->Zs[l].alloc(b);
        if (rc == SSP_OK) rc = tr->Rs[l].alloc(b);
        if (rc == SSP_OK) rc = tr->HHs[l].alloc(b);
        if (rc == SSP_OK) rc = tr->RHs[l].alloc(b);
        if (rc == SSP_OK) rc = tr->img[l].alloc(3 * (size_t)units[l] * units[l] * f4);
    }
    if (rc == SSP_OK) rc = tr->GR.alloc(mb * Hmax * f4);
    if (rc == SSP_OK) rc = tr->DH.alloc(mb * Hmax * f4);
    if (rc == SSP_OK) rc = tr->mean.alloc(mb * Hmax * f4);
    if (rc == SSP_OK) rc = tr->dmean.alloc(mb * Hmax * f4);
    if (rc == SSP_OK) rc = tr->dMT.alloc(mb * Hmax * f4);
    if (rc == SSP_OK) rc = tr->e1.alloc(mb * E * f4);
    if (rc == SSP_OK) rc = tr->y.alloc(mb * E * f4);
    if (rc == SSP_OK) rc = tr->dy.alloc(mb * E * f4);
    if (rc == SSP_OK) rc = tr->de.alloc(mb * E * f4);
    if (rc == SSP_OK) rc = tr->l2s.alloc(mb * f4);
    if (rc == SSP_OK) rc = tr->logits.alloc(mb * n_class * f4);
    if (rc == SSP_OK) rc = tr->cpart.alloc((size_t)(kh * kw + 1) * GT_CCH * F * f4);
    if (rc == SSP_OK) rc = tr->alloc_state(tr, flat);
    if (rc == SSP_OK) rc = gt_pack(tr.get(), ctx->stream);  // (queued behind the upload: one host wait for both)
    return tr.commit(rc, out);
}
SSP_CREATE_GUARD("ssp_gru_trainer_create")

int ssp_gru_trainer_destroy(ssp_gru_trainer* trainer) { return destroy_handle(trainer); }

int ssp_gru_trainer_epoch(ssp_gru_trainer* trainer, const float* X, const int32_t* labels, int64_t N, const int64_t* order, int32_t batch_size,
                          float lr, double* loss_sum, int64_t* n_correct, int where, float* kernel_ms) {
    ssp_gru_trainer* tr = trainer;
    return trainer_epoch("ssp_gru_trainer_epoch", tr, X, tr ? (int64_t)tr->T * tr->D : 0, labels, N, order, batch_size, lr, loss_sum, n_correct, where,
                         kernel_ms, [&](const float* dX, const int32_t* dL, const int64_t* dO, int64_t row0, int Bn, int64_t slot, hipStream_t s) {
                             return gt_step(tr, dX, dL, dO, row0, Bn, slot, lr, s);
                         });
}

int ssp_gru_trainer_evaluate(ssp_gru_trainer* trainer, const float* X, const int32_t* labels, int64_t N, double* loss_sum, int64_t* n_correct,
                             int where, float* kernel_ms) {
    ssp_gru_trainer* tr = trainer;
    return trainer_evaluate("ssp_gru_trainer_evaluate", tr, X, tr ? (int64_t)tr->T * tr->D : 0, labels, N, loss_sum, n_correct, where, kernel_ms,
                            [&](const float* dX, const int32_t* dL, int64_t row0, int Bn, int64_t slot, hipStream_t s) {
                                SSP_TRY(gt_forward(tr, dX, nullptr, row0, Bn, s));
                                return gt_loss(tr, dL, nullptr, row0, Bn, false, slot, s);
                            });
}

int ssp_gru_trainer_step_times(ssp_gru_trainer* trainer, const float* X, const int32_t* labels, int32_t batch_size, float lr, float* ms_out) {
    const char* who = "ssp_gru_trainer_step_times";
    ssp_gru_trainer* tr = trainer;
    StepMarks mk;
    SSP_TRY(trainer_timed_step(who, tr, X, labels, batch_size, lr, ms_out, mk,
                               [&](hipStream_t s, StepMarks* m) { return gt_step(tr, X, labels, nullptr, 0, batch_size, 0, lr, s, m); }));
    return mk.times(ms_out, GT_TIMES);
}

int ssp_gru_trainer_read(ssp_gru_trainer* trainer, int32_t what, int32_t tensor, float* out) {
    if (!trainer || !out) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_trainer_read: null argument");
    ssp_gru_trainer* tr = trainer;
    if (what < 0 || what > 3) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_trainer_read: what must be SSP_GRUT_PARAM .. SSP_GRUT_V");
    if (tensor < 0 || tensor >= GT_TENSORS || tr->len[tensor] == 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_trainer_read: the network has no tensor %d", tensor);
    if (!tr->has[tensor]) SSP_FAIL(SSP_ERR_INVALID, "ssp_gru_trainer_read: the network has no such bias");
    return tr->read_flat("ssp_gru_trainer_read", what, tr->off[tensor], tr->len[tensor], out);
}

int ssp_gru_trainer_steps(const ssp_gru_trainer* trainer, int64_t* t) { return trainer_steps("ssp_gru_trainer_steps", trainer, t); }

}  // extern "C"
