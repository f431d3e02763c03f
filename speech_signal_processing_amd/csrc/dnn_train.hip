// Training of the reference's fully connected d-vector network (d_vector.py:168-206 nn_model.inference: Dense(256) ReLU Dropout x 3,
// Dense(256), ReLU Dropout(0.5), Dense(n_class) softmax; categorical cross-entropy, Adam(lr=1e-4), batch 128, spk.fit at :205-206) as
// a chain of small launches on the ctx stream: forward with dropout, softmax cross-entropy, backward, Adam.  All arithmetic is fp32 and
// every product runs on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32).
//   * one step is tiny (128 rows, ~0.5 M parameters): the epoch is bound by launch count and by how much of the chip a 128-row problem
//     fills, so the GEMM tile is 16 x 16 per workgroup and a 128 x 256 layer is 128 workgroups, the 1274 x 256 weight gradient 1280
//   * ONE kernel body serves the three GEMM forms over the master weights in Keras' (d_in, units) layout, by how it addresses its operands:
//       mode 0  Y = act(X W + b), then inverted dropout           (rows of X optionally gathered through the epoch's order)
//       mode 1  dX = (dY W^T) . relu'(below) . dropout'(below)    (the derivative of the layer below, in the epilogue)
//       mode 2  dW = X^T dY, db = sum over rows of dY
//     operands go from global memory (L2 resident) straight into the MFMA's registers: lane (kq, i) holds A[i][16 g + 4 kq + r] and
//     B[16 g + 4 kq + r][i], r = 0..3, so that a contiguous k-run is one 16-byte load (rows of 1274 floats are only 8-byte aligned and
//     the caller's arrays need no more than 4: the loads are packed 4-byte-aligned ones, the same code for every address)
//   * K is split over the workgroup's four waves into a FIXED partition (quarters of K rounded up to 16) and the four partial tiles are
//     added through LDS in wave order; db is sixteen strided partial sums added in order; the loss of a batch is added by the last
//     workgroup to finish (an integer ticket) in a fixed order (64 strided partial sums, then a butterfly).  No floating-point atomic anywhere: the same seed, data and order give the
//     same bits
//   * the dropout decision is never stored: it is a pure function of (seed, step, layer, row in the batch, column), recomputed in the
//     backward epilogue.  What the backward pass keeps of the forward pass is each layer's output
//   * Adam is ONE launch over the flat parameter, gradient, m and v buffers (rather than a fold into the dW epilogue: dX of the same
//     layer reads the weights of this step, and ssp_dnn_trainer_read hands out the step's gradients)
#include <cmath>
#include <vector>

#include "common.hpp"
#include "nn_device.hpp"
#include "trainer_core.hpp"

namespace ssp {

constexpr int DT_MAXW = 4096;  // widest layer
constexpr int DT_MAXB = 1024;  // largest batch

// ---- the dropout generator (host and device): lowbias32 mixing, a key per (seed, step, layer), one mix per element
__host__ __device__ static inline uint32_t dt_mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}
static inline uint32_t dt_key(uint64_t seed, int64_t step, int32_t layer) {
    uint32_t k = dt_mix32(0x9e3779b9U ^ (uint32_t)seed);
    k = dt_mix32(k ^ (uint32_t)(seed >> 32));
    k = dt_mix32(k ^ (uint32_t)(uint64_t)step);
    k = dt_mix32(k ^ (uint32_t)((uint64_t)step >> 32));
    return dt_mix32(k ^ (uint32_t)layer);
}
// kept iff the top 24 bits of the element's word reach thr = floor(rate 2^24)
__host__ __device__ static inline bool dt_keep(uint32_t key, uint32_t thr, int row, int col) {
    return (dt_mix32(key ^ (uint32_t)(row * DT_MAXW + col)) >> 8) >= thr;
}
static inline uint32_t dt_thr(float rate) { return (uint32_t)((double)rate * 16777216.0); }

struct GemmArgs {
    const float* A;      // mode 0: X [rows x K]; 1: dY [M x K]; 2: X [rows x M] (read transposed)
    const float* B;      // mode 0: W [K x N]; 1: W [N x K] (read transposed); 2: dY [K x N]
    float* C;            // [M x N]
    const int64_t* idx;  // rows of A's batch dimension (mode 0: m, mode 2: k), nullable = the identity
    int32_t M, N, K;
    int64_t lda;
    const float* bias;   // mode 0 (nullable)
    const float* Yref;   // mode 1: the output of the layer below (read when relu)
    float* db;           // mode 2 (nullable)
    int32_t relu;
    uint32_t thr, key;   // dropout of this layer (mode 0) / of the layer below (mode 1); thr 0 = none
    float scale;         // 1 / (1 - rate)
};

template <int MODE>
__global__ __launch_bounds__(256) void dt_gemm_kernel(GemmArgs a) {
    __shared__ __attribute__((aligned(16))) float red[4][256];  // the waves' partial tiles (splitk_sum), then mode 2's db sums
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, kq = lane >> 4;
    const int m0 = blockIdx.y * 16, n0 = blockIdx.x * 16;
    const int M = a.M, N = a.N, K = a.K;
    const SplitK ks = splitk_range(K, wave);  // the fixed partition of K over the four waves (nn_device.hpp)
    const int kend = ks.kend;
    const bool m_ok = m0 + i < M, n_ok = n0 + i < N;
    const float* arow = a.A;  // modes 0, 1: this lane's row of A
    if (MODE != 2 && m_ok) arow = a.A + (a.idx ? a.idx[m0 + i] : (int64_t)(m0 + i)) * a.lda;
    const float* brow = a.B + (int64_t)(n0 + i) * K;  // mode 1: this lane's row of W

    // operands of the 16-k block at kb into registers (zero beyond this wave's k range and beyond the matrices)
    auto load = [&](int kb, float (&av)[4], float (&bv)[4]) {
        const int k = kb + 4 * kq;
#pragma unroll
        for (int r = 0; r < 4; ++r) av[r] = bv[r] = 0.f;
        if (MODE != 2) {
            if (m_ok) {
                if (k + 3 < kend) {
                    const f4u t = *reinterpret_cast<const f4u*>(arow + k);
                    av[0] = t.x, av[1] = t.y, av[2] = t.z, av[3] = t.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (k + r < kend) av[r] = arow[k + r];
                }
            }
        } else if (m_ok) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (k + r < kend) av[r] = a.A[(a.idx ? a.idx[k + r] : (int64_t)(k + r)) * a.lda + m0 + i];
        }
        if (MODE == 1) {
            if (n_ok) {
                if (k + 3 < kend) {
                    const f4u t = *reinterpret_cast<const f4u*>(brow + k);
                    bv[0] = t.x, bv[1] = t.y, bv[2] = t.z, bv[3] = t.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (k + r < kend) bv[r] = brow[k + r];
                }
            }
        } else if (n_ok) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (k + r < kend) bv[r] = a.B[(int64_t)(k + r) * N + n0 + i];
        }
    };
    const SplitKElem el = splitk_sum(red, splitk_walk(ks, load), tid, wave);
    const int row = el.row, m = m0 + row, n = n0 + el.col;
    float v = el.v;
    if (m < M && n < N) {
        if (MODE == 0) {
            if (a.bias) v += a.bias[n];
            if (a.relu) v = fmaxf(v, 0.f);
            if (a.thr) v = dt_keep(a.key, a.thr, m, n) ? v * a.scale : 0.f;
        } else if (MODE == 1) {
            if (a.thr) v = dt_keep(a.key, a.thr, m, n) ? v * a.scale : 0.f;
            if (a.relu) v = a.Yref[(int64_t)m * N + n] > 0.f ? v : 0.f;
        }
        a.C[(int64_t)m * N + n] = v;
    }
    if (MODE == 2 && a.db && blockIdx.y == 0) {  // db of this workgroup's 16 columns: 16 strided partial sums, added in order
        __syncthreads();
        float s = 0.f;
        if (n < N)
            for (int k = row; k < K; k += 16) s += a.B[(int64_t)k * N + n];
        red[0][tid] = s;
        __syncthreads();
        if (tid < 16 && n0 + tid < N) {
            float t = red[0][tid];
#pragma unroll
            for (int j = 1; j < 16; ++j) t += red[0][j * 16 + tid];
            a.db[n0 + tid] = t;
        }
    }
}

struct LossArgs {
    float* Z;               // [B x C] logits in, (softmax - onehot) inv_B out (write_grad)
    const int32_t* labels;  // label of row r: labels[idx ? idx[r] : r]
    const int64_t* idx;
    int32_t B, C, write_grad;
    float inv_B;
    float* rowloss;         // [B]
    int32_t* rowcorr;       // [B]
    uint32_t* ticket;
    float* loss_slot;       // the batch's loss sum
    int32_t* corr_slot;     // the batch's count of rows whose arg-max (first index on ties) is the label
};

// one wave per row: maximum and arg-max, log-sum-exp, gradient in place; the last workgroup to finish adds the rows up in a fixed order
__global__ __launch_bounds__(256) void dt_loss_kernel(LossArgs a) {
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x * 4 + wave;
    const int C = a.C;
    if (row < a.B) {
        float* z = a.Z + (int64_t)row * C;
        const int lab = a.labels[a.idx ? a.idx[row] : (int64_t)row];
        float mx = -INFINITY;
        int am = 0x7fffffff;
        for (int c = lane; c < C; c += 64) {
            const float v = z[c];
            if (v > mx) mx = v, am = c;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float omx = __shfl_xor(mx, o);
            const int oam = __shfl_xor(am, o);
            if (omx > mx || (omx == mx && oam < am)) mx = omx, am = oam;
        }
        float s = 0.f, zl = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float v = z[c] - mx;
            s += expf(v);
            if (c == lab) zl = v;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            s += __shfl_xor(s, o);
            zl += __shfl_xor(zl, o);  // (one lane holds the value, the others zero)
        }
        if (a.write_grad) {
            const float inv_s = 1.f / s;
            for (int c = lane; c < C; c += 64) {
                const float p = expf(z[c] - mx) * inv_s;
                z[c] = (p - (c == lab ? 1.f : 0.f)) * a.inv_B;
            }
        }
        if (lane == 0) {
            // (a label outside [0, C) on the device: no one-hot entry, the loss is the log-sum-exp of the logits)
            a.rowloss[row] = (lab >= 0 && lab < C) ? logf(s) - zl : logf(s) + mx;
            a.rowcorr[row] = am == lab ? 1 : 0;
            __threadfence();
        }
    }
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(a.ticket, 1u) == gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (s_last && wave == 0) {
        __threadfence();
        const volatile float* rl = a.rowloss;
        const volatile int32_t* rc = a.rowcorr;
        float s = 0.f;
        int n = 0;
        for (int r = lane; r < a.B; r += 64) {
            s += rl[r];
            n += rc[r];
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            s += __shfl_xor(s, o);
            n += __shfl_xor(n, o);
        }
        if (lane == 0) {
            *a.loss_slot = s;
            *a.corr_slot = n;
            *a.ticket = 0u;
        }
    }
}

// Keras 2's Adam: eps outside the root, the bias correction folded into lr_t.  c1 = 1 - b1 and c2 = 1 - b2 arrive rounded once from
// float64 (1.f - 0.999f is off by 1.3e-5 of itself, which would sit in every v)
__global__ __launch_bounds__(256) void dt_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, int64_t n, float lr_t, float b1, float c1, float b2, float c2,
                                                      float eps) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float mi = b1 * m[i] + c1 * gi;
    const float vi = b2 * v[i] + c2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= lr_t * mi / (sqrtf(vi) + eps);
}

template <int MODE>
static int dt_gemm(const GemmArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((dt_gemm_kernel<MODE>), dim3((unsigned)((a.N + 15) / 16), (unsigned)((a.M + 15) / 16)), dim3(256), 0, s, a);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

}  // namespace ssp

struct ssp_dnn_trainer : ssp::TrainerCore {
    int32_t L = 0;
    std::vector<int32_t> dims, relu, has_bias;
    std::vector<float> rate, scale;
    std::vector<uint32_t> thr;
    std::vector<int64_t> woff, boff, aoff;  // layer l's kernel / bias in the flat buffers; its output in `act` / `dz`
    ssp::DevBuf act, dz;                    // every layer's output and the gradient at it (the last layer's lives in act: in place)
};

using namespace ssp;

namespace {

float* dt_act(ssp_dnn_trainer* tr, int l) { return tr->act.as<float>() + tr->aoff[l]; }
float* dt_dz(ssp_dnn_trainer* tr, int l) { return l == tr->L - 1 ? dt_act(tr, l) : tr->dz.as<float>() + tr->aoff[l]; }

// forward pass of rows [row0, row0 + Bn) (of idx when given) into tr->act; train: dropout on, keyed by (seed, step)
int dt_forward(ssp_dnn_trainer* tr, const float* X, const int64_t* idx, int64_t row0, int Bn, bool train, uint64_t seed, int64_t step,
               hipStream_t s) {
    for (int l = 0; l < tr->L; ++l) {
        GemmArgs a{};
        if (l == 0) {
            a.A = idx ? X : X + row0 * tr->dims[0];
            a.idx = idx ? idx + row0 : nullptr;
        } else {
            a.A = dt_act(tr, l - 1);
        }
        a.B = tr->P.as<float>() + tr->woff[l];
        a.C = dt_act(tr, l);
        a.M = Bn, a.N = tr->dims[l + 1], a.K = tr->dims[l];
        a.lda = tr->dims[l];
        a.bias = tr->has_bias[l] ? tr->P.as<float>() + tr->boff[l] : nullptr;
        a.relu = tr->relu[l];
        a.thr = train ? tr->thr[l] : 0u;
        a.key = dt_key(seed, step, l);
        a.scale = tr->scale[l];
        SSP_TRY(dt_gemm<0>(a, s));
    }
    return SSP_OK;
}

int dt_backward(ssp_dnn_trainer* tr, const float* X, const int64_t* idx, int64_t row0, int Bn, uint64_t seed, int64_t step, hipStream_t s) {
    for (int l = tr->L - 1; l >= 0; --l) {
        GemmArgs w{};
        if (l == 0) {
            w.A = idx ? X : X + row0 * tr->dims[0];
            w.idx = idx ? idx + row0 : nullptr;
        } else {
            w.A = dt_act(tr, l - 1);
        }
        w.lda = tr->dims[l];
        w.B = dt_dz(tr, l);
        w.C = tr->G.as<float>() + tr->woff[l];
        w.db = tr->has_bias[l] ? tr->G.as<float>() + tr->boff[l] : nullptr;
        w.M = tr->dims[l], w.N = tr->dims[l + 1], w.K = Bn;
        SSP_TRY(dt_gemm<2>(w, s));
        if (l == 0) break;
        GemmArgs x{};
        x.A = dt_dz(tr, l);
        x.lda = tr->dims[l + 1];
        x.B = tr->P.as<float>() + tr->woff[l];
        x.C = dt_dz(tr, l - 1);
        x.M = Bn, x.N = tr->dims[l], x.K = tr->dims[l + 1];
        x.Yref = dt_act(tr, l - 1);
        x.relu = tr->relu[l - 1];
        x.thr = tr->thr[l - 1];
        x.key = dt_key(seed, step, l - 1);
        x.scale = tr->scale[l - 1];
        SSP_TRY(dt_gemm<1>(x, s));
    }
    return SSP_OK;
}

}  // namespace

extern "C" {

int ssp_dropout_keep(uint64_t seed, int64_t step, int32_t layer, int32_t rows, int32_t width, float rate, uint8_t* keep_out) {
    if (rows < 0 || width < 0 || layer < 0 || step < 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_dropout_keep: negative argument");
    if (!(rate >= 0.f && rate < 1.f)) SSP_FAIL(SSP_ERR_INVALID, "ssp_dropout_keep: rate must lie in [0, 1)");
    if (rows > DT_MAXB || width > DT_MAXW) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_dropout_keep: up to %d rows of up to %d columns", DT_MAXB, DT_MAXW);
    if (!keep_out && (int64_t)rows * width > 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_dropout_keep: null output");
    const uint32_t key = dt_key(seed, step, layer), thr = dt_thr(rate);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < width; ++c) keep_out[(size_t)r * width + c] = dt_keep(key, thr, r, c) ? 1 : 0;
    return SSP_OK;
}

int ssp_dnn_trainer_create(ssp_ctx* ctx, int32_t n_layers, const int32_t* dims, const int32_t* relu, const float* dropout_rate,
                           const float* const* W, const float* const* bias, int32_t max_batch, ssp_dnn_trainer** out) try {
    if (!out) SSP_FAIL(SSP_ERR_INVALID, "ssp_dnn_trainer_create: null out");
    *out = nullptr;
    if (n_layers < 1 || !dims || !relu || !dropout_rate || !W) SSP_FAIL(SSP_ERR_INVALID, "ssp_dnn_trainer_create: null argument or no layer");
    if (max_batch < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_dnn_trainer_create: max_batch < 1");
    for (int l = 0; l <= n_layers; ++l)
        if (dims[l] < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_dnn_trainer_create: width %d of layer boundary %d", dims[l], l);
    for (int l = 0; l < n_layers; ++l) {
        if (!W[l]) SSP_FAIL(SSP_ERR_INVALID, "ssp_dnn_trainer_create: null kernel (layer %d)", l);
        if (!(dropout_rate[l] >= 0.f && dropout_rate[l] < 1.f))
            SSP_FAIL(SSP_ERR_INVALID, "ssp_dnn_trainer_create: dropout rate of layer %d must lie in [0, 1)", l);
    }
    if (dims[n_layers] < 2) SSP_FAIL(SSP_ERR_INVALID, "ssp_dnn_trainer_create: at least two classes");
    for (int l = 0; l <= n_layers; ++l)
        if (dims[l] > DT_MAXW) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_dnn_trainer_create: widths up to %d (got %d)", DT_MAXW, dims[l]);
    if (max_batch > DT_MAXB) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_dnn_trainer_create: max_batch up to %d (got %d)", DT_MAXB, max_batch);
    if (n_layers > 64) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_dnn_trainer_create: up to 64 layers");
    SSP_TRY(use_ctx(ctx));
    HandleBuild<ssp_dnn_trainer> tr(ctx, "ssp_dnn_trainer_create");
    tr->L = n_layers;
    tr->max_batch = max_batch;
    tr->n_class = dims[n_layers];
    int64_t np = 0, na = 0;
    for (int l = 0; l < n_layers; ++l) {
        tr->relu.push_back(relu[l] ? 1 : 0);
        tr->has_bias.push_back(bias && bias[l] ? 1 : 0);
        tr->rate.push_back(dropout_rate[l]);
        tr->scale.push_back(1.0f / (1.0f - dropout_rate[l]));
        tr->thr.push_back(dt_thr(dropout_rate[l]));
        tr->woff.push_back(np);
        np += (int64_t)dims[l] * dims[l + 1];
        tr->boff.push_back(np);
        np += dims[l + 1];
        tr->aoff.push_back(na);
        na += (int64_t)max_batch * dims[l + 1];
    }
    tr->dims.assign(dims, dims + n_layers + 1);
    std::vector<float> flat((size_t)np, 0.f);
    for (int l = 0; l < n_layers; ++l) {
        memcpy(flat.data() + tr->woff[l], W[l], (size_t)dims[l] * dims[l + 1] * sizeof(float));
        if (tr->has_bias[l]) memcpy(flat.data() + tr->boff[l], bias[l], (size_t)dims[l + 1] * sizeof(float));
    }
    int rc = tr->act.alloc((size_t)na * sizeof(float));
    if (rc == SSP_OK) rc = tr->dz.alloc((size_t)na * sizeof(float));
    if (rc == SSP_OK) rc = tr->alloc_state(tr, flat);
    return tr.commit(rc, out);
}
SSP_CREATE_GUARD("ssp_dnn_trainer_create")

int ssp_dnn_trainer_destroy(ssp_dnn_trainer* trainer) { return destroy_handle(trainer); }

int ssp_dnn_trainer_epoch(ssp_dnn_trainer* trainer, const float* X, const int32_t* labels, int64_t N, const int64_t* order, int32_t batch_size,
                          float lr, uint64_t seed, double* loss_sum, int64_t* n_correct, int where, float* kernel_ms) {
    ssp_dnn_trainer* tr = trainer;
    return trainer_epoch("ssp_dnn_trainer_epoch", tr, X, tr ? tr->dims[0] : 0, labels, N, order, batch_size, lr, loss_sum, n_correct, where, kernel_ms,
                         [&](const float* dX, const int32_t* dL, const int64_t* dO, int64_t row0, int Bn, int64_t slot, hipStream_t s) {
                             const int64_t step = tr->t;  // the dropout counter: steps taken before this one, over the whole fit
                             SSP_TRY(dt_forward(tr, dX, dO, row0, Bn, true, seed, step, s));
                             SSP_TRY(tr->loss(dL, dO, row0, Bn, true, slot, dt_act(tr, tr->L - 1), s));
                             SSP_TRY(dt_backward(tr, dX, dO, row0, Bn, seed, step, s));
                             return tr->adam(lr, s);
                         });
}

int ssp_dnn_trainer_evaluate(ssp_dnn_trainer* trainer, const float* X, const int32_t* labels, int64_t N, double* loss_sum, int64_t* n_correct,
                             int where, float* kernel_ms) {
    ssp_dnn_trainer* tr = trainer;
    return trainer_evaluate("ssp_dnn_trainer_evaluate", tr, X, tr ? tr->dims[0] : 0, labels, N, loss_sum, n_correct, where, kernel_ms,
                            [&](const float* dX, const int32_t* dL, int64_t row0, int Bn, int64_t slot, hipStream_t s) {
                                SSP_TRY(dt_forward(tr, dX, nullptr, row0, Bn, false, 0, 0, s));
                                return tr->loss(dL, nullptr, row0, Bn, false, slot, dt_act(tr, tr->L - 1), s);
                            });
}

int ssp_dnn_trainer_read(ssp_dnn_trainer* trainer, int32_t what, int32_t layer, float* out) {
    if (!trainer || !out) SSP_FAIL(SSP_ERR_INVALID, "ssp_dnn_trainer_read: null argument");
    ssp_dnn_trainer* tr = trainer;
    if (layer < 0 || layer >= tr->L) SSP_FAIL(SSP_ERR_INVALID, "ssp_dnn_trainer_read: layer %d of %d", layer, tr->L);
    if (what < 0 || what > 7) SSP_FAIL(SSP_ERR_INVALID, "ssp_dnn_trainer_read: what must be SSP_DNN_W .. SSP_DNN_V_B");
    const bool is_bias = (what & 1) != 0;
    if (is_bias && !tr->has_bias[layer]) SSP_FAIL(SSP_ERR_INVALID, "ssp_dnn_trainer_read: layer %d has no bias", layer);
    const int64_t n = is_bias ? (int64_t)tr->dims[layer + 1] : (int64_t)tr->dims[layer] * tr->dims[layer + 1];
    return tr->read_flat("ssp_dnn_trainer_read", what >> 1, is_bias ? tr->boff[layer] : tr->woff[layer], n, out);
}

int ssp_dnn_trainer_steps(const ssp_dnn_trainer* trainer, int64_t* t) { return trainer_steps("ssp_dnn_trainer_steps", trainer, t); }

}  // extern "C"

// ---- the step kernels as plain launches (dnn_train.hpp): what every trainer, this one included, queues them through

namespace ssp {

int dt_launch_gemm(int mode, const float* A, const float* B, float* C, const int64_t* idx, int32_t M, int32_t N, int32_t K, int64_t lda,
                   const float* bias, float* db, hipStream_t s) {
    GemmArgs a{};
    a.A = A, a.B = B, a.C = C, a.idx = idx;
    a.M = M, a.N = N, a.K = K, a.lda = lda;
    a.bias = bias, a.db = db;
    a.scale = 1.f;
    if (mode == 0) return dt_gemm<0>(a, s);
    if (mode == 1) return dt_gemm<1>(a, s);
    if (mode == 2) return dt_gemm<2>(a, s);
    SSP_FAIL(SSP_ERR_INVALID, "dt_launch_gemm: mode");
}

int dt_launch_loss(float* Z, const int32_t* labels, const int64_t* idx, int32_t B, int32_t C, int write_grad, float* rowloss, int32_t* rowcorr,
                   uint32_t* ticket, float* loss_slot, int32_t* corr_slot, hipStream_t s) {
    LossArgs a{};
    a.Z = Z, a.labels = labels, a.idx = idx;
    a.B = B, a.C = C, a.write_grad = write_grad ? 1 : 0;
    a.inv_B = 1.f / (float)B;
    a.rowloss = rowloss, a.rowcorr = rowcorr, a.ticket = ticket, a.loss_slot = loss_slot, a.corr_slot = corr_slot;
    hipLaunchKernelGGL(dt_loss_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, a);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

int dt_launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, int64_t t1, hipStream_t s) {
    const double b1 = 0.9, b2 = 0.999;
    const float lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow(b2, (double)t1)) / (1.0 - std::pow(b1, (double)t1)));
    hipLaunchKernelGGL(dt_adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, g, m, v, n, lr_t, (float)b1, (float)(1.0 - b1),
                       (float)b2, (float)(1.0 - b2), 1e-7f);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

}  // namespace ssp
