// VB-HMM resegmentation of diarization labels on gfx950 (ssp_vbhmm_resegment): the Bayesian HMM over a recording's projected window
// embeddings (VBx, Landini et al. 2022), started from the AHC labels, batched over recordings.  An extension and UNPINNED; include/ssp.h
// has the model, tests/vbhmm_oracle.py restates it in float64.  The tables and the workspace are the diarization block's (ctx->diar_*):
// all of a ctx's work is ordered on its one stream.
// Kernels:
//   vb_rowstat_kernel  one wave per row: G_t = -1/2 (sum_d x_td^2 + q ln 2 pi), summed in float64 and rounded once (lane l adds entries
//                      l, l + 64, ... then a butterfly); NaN for a row with a non-finite entry, which is how the main kernel learns of it
//   vb_hmm_kernel      <NS, RES>: one 256-thread workgroup per recording, longest first, runs the WHOLE iteration loop.  S is padded to
//                      SP = 16 NS columns (NS = 1, 2, 4).  Two T x SP buffers — ll, and a-hat which gamma overwrites — sit in LDS (RES)
//                      or in the ctx's workspace; alpha (SP x (q | 1)) sits in LDS up to VB_ALPHA_LDS bytes, else in the workspace.
//                      Per iteration:  N_s (fixed-order partial sums);  gamma^T rho on v_mfma_f32_16x16x4_f32, a wave per 64 columns
//                      of q and ONE chain over t per output, ascending, its epilogue forms alpha;  per state the constant of ll and the
//                      ELBO's model term in float64 (a wave per state);  rho alpha^T on the same MFMA, a wave per 16 rows and one chain
//                      over d per output, ascending, epilogue ll;  then wave 0, states on lanes, runs the scaled forward recursion and
//                      after it the backward one, which forms gamma in place and the pi update from the same scaled quantities:
//                      (1 - P) pi_s / (P a-hat_{t-1,s} + (1 - P) pi_s) is the share of gamma_ts that arrived by the non-loop branch.
//                      rho = x sqrt(phi) is formed as X is loaded and never stored.  ln p(X), the ELBO and the stop decision are
//                      float64.  Every loop has a trip count known on entry (max_iters, T, q); no workgroup talks to another.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace ssp {

constexpr int VB_MAX_Q = 1024, VB_MAX_N = 4096, VB_MAX_S = 64, VB_MAX_ITERS = 100;
constexpr int VB_LDS_BYTES = SSP_VBHMM_LDS_BYTES;              // dynamic LDS of a workgroup: alpha and the two T x SP buffers
constexpr int VB_ALPHA_LDS = SSP_VBHMM_ALPHA_LDS_BYTES;        // alpha sits in LDS up to this many bytes

using f32x4 = __attribute__((ext_vector_type(4))) float;

__global__ __launch_bounds__(256) void vb_rowstat_kernel(const float* __restrict__ X, int64_t row0, int64_t rows, int q, float* __restrict__ G) {
    const int lane = threadIdx.x & 63;
    const int64_t row = row0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= row0 + rows) return;
    const float* x = X + row * q;
    double s = 0.0;
    bool bad = false;
    for (int d = lane; d < q; d += 64) {
        const float v = x[d];
        bad = bad || !(fabsf(v) < INFINITY);
        s += (double)v * (double)v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const bool any_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if (lane == 0) G[row] = any_bad ? __builtin_nanf("") : (float)(-0.5 * (s + (double)q * 1.8378770664093453));
}

struct VbRec {  // one recording of a launch (host-made, uploaded per call)
    int64_t row0;    // first row of X / the per-row arrays
    int64_t ws_off;  // float offset of what it keeps in the workspace
    int32_t n, rec;  // rows; index in the batch
};

struct VbArgs {
    const float* X;
    const float* G;     // per row, NaN: the row has a non-finite entry
    const float* sphi;  // sqrt(phi)
    const float* phi;
    const VbRec* recs;  // this launch's recordings, longest first
    const int32_t* init_labels;
    const int32_t* n_init;  // nullable
    float* ws;
    int32_t* labels;
    int32_t* states;  // nullable
    int32_t* n_speakers;
    int32_t* n_iters;
    double* elbo;   // nullable
    float* gamma;   // nullable
    float* pi;      // nullable
    float* loglik;  // nullable
    int32_t q, S, max_iters;
    float P, Fa, Fb, smooth;
    double eps;
};

template <int CTRL>
__device__ __forceinline__ float vb_dpp(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
// sum / max over the first SP lanes (every one of them gets the same bits): rotations by 8, 4, 2, 1 inside the rows of 16 lanes, each
// level adding two values that the lanes of the level share, then the rows
template <int SP>
__device__ __forceinline__ float vb_sum(float x) {
    x += vb_dpp<0x128>(x);
    x += vb_dpp<0x124>(x);
    x += vb_dpp<0x122>(x);
    x += vb_dpp<0x121>(x);
    if (SP > 16) x += __shfl_xor(x, 16);
    if (SP > 32) x += __shfl_xor(x, 32);
    return x;
}
template <int SP>
__device__ __forceinline__ float vb_max(float x) {
    x = fmaxf(x, vb_dpp<0x128>(x));
    x = fmaxf(x, vb_dpp<0x124>(x));
    x = fmaxf(x, vb_dpp<0x122>(x));
    x = fmaxf(x, vb_dpp<0x121>(x));
    if (SP > 16) x = fmaxf(x, __shfl_xor(x, 16));
    if (SP > 32) x = fmaxf(x, __shfl_xor(x, 32));
    return x;
}
__device__ __forceinline__ double vb_sum64(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

template <int NS, bool RES>
__global__ __launch_bounds__(256, NS == 4 ? 2 : 4) void vb_hmm_kernel(VbArgs a, int alpha_in_lds) {
    constexpr int SP = 16 * NS;
    extern __shared__ __attribute__((aligned(16))) char vb_smem[];
    __shared__ float s_N[64], s_cs[64], s_pi[64], s_part[256];
    __shared__ double s_e[64];
    __shared__ int s_first[64], s_rank[64], s_stop, s_count;
    const VbRec rc = a.recs[blockIdx.x];
    const int T = rc.n, q = a.q, S = a.S, ldq = q | 1, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g4 = lane >> 4;
    float* smem = reinterpret_cast<float*>(vb_smem);
    float* wsr = a.ws + rc.ws_off;
    float* alpha;
    if (alpha_in_lds) {
        alpha = smem;
        smem += SP * ldq;
    } else {
        alpha = wsr;
        wsr += SP * ldq;
    }
    float* buf0 = RES ? smem : wsr;  // ll of the iteration; at the end the winning states
    float* buf1 = buf0 + T * SP;     // gamma; inside the recursion a-hat
    const float* X = a.X + rc.row0 * q;
    const float* G = a.G + rc.row0;
    const int Sr = a.n_init ? min(max(a.n_init[rc.rec], 1), S) : S;
    const float P = a.P, Q = 1.f - a.P, FaFb = a.Fa / a.Fb;
    const float qnan = __builtin_nanf("");

    int bad = 0;
    for (int t = tid; t < T; t += 256) bad |= G[t] != G[t];
    bad = __syncthreads_or(bad);
    if (bad) {  // a non-finite entry in X: the recording is poisoned, nothing else is
        for (int t = tid; t < T; t += 256) {
            a.labels[rc.row0 + t] = -1;
            if (a.states) a.states[rc.row0 + t] = -1;
        }
        for (int e = tid; e < T * S; e += 256) {
            if (a.gamma) a.gamma[rc.row0 * S + e] = qnan;
            if (a.loglik) a.loglik[rc.row0 * S + e] = qnan;
        }
        for (int s = tid; s < S; s += 256)
            if (a.pi) a.pi[(int64_t)rc.rec * S + s] = qnan;
        for (int i = tid; i < a.max_iters; i += 256)
            if (a.elbo) a.elbo[(int64_t)rc.rec * a.max_iters + i] = (double)qnan;
        if (tid == 0) {
            a.n_speakers[rc.rec] = -1;
            a.n_iters[rc.rec] = 0;
        }
        return;
    }

    {  // the start: pi uniform over the live states, gamma the softmax of smooth * onehot(label)
        const float w = expf(-a.smooth), den = 1.f + (float)(Sr - 1) * w, hit = 1.f / den, miss = w / den, uni = 1.f / (float)Sr;
        for (int e = tid; e < T * SP; e += 256) {
            const int t = e / SP, s = e % SP, lab = a.init_labels[rc.row0 + t];
            float v = 0.f;
            if (s < Sr) v = (lab >= 0 && lab < Sr) ? (s == lab ? hit : miss) : uni;
            buf1[e] = v;
        }
        if (tid < 64) s_pi[tid] = tid < Sr ? uni : 0.f;
    }

    int n_it = 0;
    double prev = 0.0;
    for (int it = 0; it < a.max_iters; ++it) {
        __syncthreads();
        {  // N_s: 256 / SP partial sums per state, each over every (256 / SP)-th row, added in their order
            const int c = tid & (SP - 1), part = tid / SP;
            float acc = 0.f;
            for (int t = part; t < T; t += 256 / SP) acc += buf1[t * SP + c];
            s_part[tid] = acc;
        }
        __syncthreads();
        if (tid < SP) {
            float n = 0.f;
            for (int p = 0; p < 256 / SP; ++p) n += s_part[p * SP + tid];
            s_N[tid] = n;
        }
        __syncthreads();
        // gamma^T rho: a wave per 64 columns of q, the chain over t
        for (int d0 = wave * 64; d0 < q; d0 += 256) {
            f32x4 acc[NS][4];
#pragma unroll
            for (int i = 0; i < NS; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            float sp[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) sp[j] = d0 + 16 * j + c16 < q ? a.sphi[d0 + 16 * j + c16] : 0.f;
            for (int t0 = 0; t0 < T; t0 += 4) {
                const int t = t0 + g4;
                const bool tin = t < T;
                float bv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int d = d0 + 16 * j + c16;
                    bv[j] = (tin && d < q) ? X[(int64_t)t * q + d] * sp[j] : 0.f;
                }
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    const float av = tin ? buf1[t * SP + 16 * i + c16] : 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j], acc[i][j], 0, 0, 0);
                }
            }
            // accumulator r: state 16 i + 4 g4 + r, column d0 + 16 j + c16
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = d0 + 16 * j + c16;
                if (d < q) {
                    const float ph = a.phi[d];
#pragma unroll
                    for (int i = 0; i < NS; ++i)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int s = 16 * i + 4 * g4 + r;
                            const float invL = 1.f / (1.f + FaFb * s_N[s] * ph);
                            alpha[s * ldq + d] = FaFb * invL * acc[i][j][r];
                        }
                }
            }
        }
        __syncthreads();
        // per live state: the constant of ll, -1/2 sum_d (invL + alpha^2) phi, and the ELBO's sum_d (ln invL - invL - alpha^2 + 1)
        for (int s = wave; s < SP; s += 4) {
            double cs = 0.0, e = 0.0;
            if (s < Sr) {
                const float n = s_N[s];
                for (int d = lane; d < q; d += 64) {
                    const float ph = a.phi[d], al = alpha[s * ldq + d];
                    const double x = (double)(FaFb * n * ph), invL = 1.0 / (1.0 + x), a2 = (double)al * (double)al;
                    cs += (invL + a2) * (double)ph;
                    e += -log1p(x) - invL - a2 + 1.0;
                }
                cs = vb_sum64(cs);
                e = vb_sum64(e);
            }
            if (lane == 0) {
                s_cs[s] = (float)(-0.5 * cs);
                s_e[s] = e;
            }
        }
        __syncthreads();
        // rho alpha^T: a wave per 16 rows, the chain over d; ll = Fa (rho . alpha_s + c_s + G_t)
        for (int t0 = wave * 16; t0 < T; t0 += 64) {
            f32x4 acc[NS];
#pragma unroll
            for (int i = 0; i < NS; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int trow = t0 + c16;
            const bool tin = trow < T;
            const float* xr = X + (int64_t)(tin ? trow : 0) * q;
            for (int k0 = 0; k0 < q; k0 += 4) {
                const int d = k0 + g4;
                const bool din = d < q;
                const float av = (tin && din) ? xr[d] * a.sphi[d] : 0.f;
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    const float bv = din ? alpha[(16 * i + c16) * ldq + d] : 0.f;
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[i], 0, 0, 0);
                }
            }
            // accumulator r: row t0 + 4 g4 + r, state 16 i + c16
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = t0 + 4 * g4 + r;
                if (t < T) {
                    const float gt = G[t];
#pragma unroll
                    for (int i = 0; i < NS; ++i) {
                        const int s = 16 * i + c16;
                        const float v = a.Fa * (acc[i][r] + s_cs[s] + gt);
                        buf0[t * SP + s] = v;
                        if (a.loglik && s < S) a.loglik[(rc.row0 + t) * S + s] = v;
                    }
                }
            }
        }
        __syncthreads();
        if (wave == 0) {  // the recursions: state s on lane s
            const int s = lane;
            const bool act = s < Sr, inb = s < SP;
            const float pis = s_pi[s];
            double lnp = 0.0;
            float ah = 0.f;
            for (int t = 0; t < T; ++t) {
                const float l = inb ? buf0[t * SP + s] : 0.f;
                const float w = t == 0 ? pis : P * ah + Q * pis;
                const bool on = act && w > 0.f;  // (the scale is the largest ll among the states that can be reached)
                const float m = vb_max<SP>(on ? l : -INFINITY);
                const float av = on ? expf(l - m) * w : 0.f;
                const float c = vb_sum<SP>(av);
                ah = act ? av / c : 0.f;
                if (inb) buf1[t * SP + s] = ah;
                lnp += (double)logf(c) + (double)m;
            }
            float bh = act ? 1.f : 0.f, pacc = 0.f;
            for (int t = T - 1; t >= 0; --t) {
                const float at = inb ? buf1[t * SP + s] : 0.f;
                const float gp = at * bh;
                const float D = vb_sum<SP>(gp);
                const float gam = act ? gp / D : 0.f;
                if (t > 0) {
                    const float ap = inb ? buf1[(t - 1) * SP + s] : 0.f;
                    const float den = P * ap + Q * pis;
                    pacc += den > 0.f ? gam * (Q * pis) / den : 0.f;
                    const float l = inb ? buf0[t * SP + s] : 0.f;
                    const bool on = act && bh > 0.f;
                    const float m = vb_max<SP>(on ? l : -INFINITY);
                    const float y = on ? expf(l - m) * bh : 0.f;
                    const float sy = vb_sum<SP>(pis * y);
                    const float bt = act ? P * y + Q * sy : 0.f;
                    bh = bt / vb_max<SP>(bt);
                } else {
                    pacc += gam;
                }
                if (inb) buf1[t * SP + s] = gam;
            }
            const float tot = vb_sum<SP>(pacc);
            s_pi[s] = act ? pacc / tot : 0.f;
            const double elbo = lnp + 0.5 * (double)a.Fb * vb_sum64(inb ? s_e[s] : 0.0);
            if (lane == 0) {
                if (a.elbo) a.elbo[(int64_t)rc.rec * a.max_iters + it] = elbo;
                s_stop = (it > 0 && elbo - prev < a.eps) || it == a.max_iters - 1;
            }
            prev = elbo;
        }
        __syncthreads();
        n_it = it + 1;
        if (s_stop) break;
    }

    // states: the arg-max of a row, ties to the lowest state; labels: the rank of the state among the winners by their first row
    if (tid < 64) s_first[tid] = INT32_MAX;
    __syncthreads();
    int32_t* win = reinterpret_cast<int32_t*>(buf0);
    for (int t = tid; t < T; t += 256) {
        int best = 0;
        float bv = buf1[t * SP];
        for (int s = 1; s < Sr; ++s) {
            const float v = buf1[t * SP + s];
            if (v > bv) {
                bv = v;
                best = s;
            }
        }
        win[t] = best;
        atomicMin(&s_first[best], t);
    }
    __syncthreads();
    if (tid < 64) {
        const int f = s_first[tid];
        int r = 0;
        for (int s = 0; s < 64; ++s) r += s_first[s] < f ? 1 : 0;
        s_rank[tid] = r;
        const unsigned long long won = __builtin_amdgcn_ballot_w64(f != INT32_MAX);
        if (tid == 0) s_count = __popcll(won);
    }
    __syncthreads();
    for (int t = tid; t < T; t += 256) {
        a.labels[rc.row0 + t] = s_rank[win[t]];
        if (a.states) a.states[rc.row0 + t] = win[t];
    }
    if (a.gamma)
        for (int e = tid; e < T * S; e += 256) a.gamma[rc.row0 * S + e] = buf1[(e / S) * SP + e % S];
    if (a.pi)
        for (int s = tid; s < S; s += 256) a.pi[(int64_t)rc.rec * S + s] = s_pi[s];
    if (a.elbo)
        for (int i = n_it + tid; i < a.max_iters; i += 256) a.elbo[(int64_t)rc.rec * a.max_iters + i] = (double)qnan;
    if (tid == 0) {
        a.n_speakers[rc.rec] = s_count;
        a.n_iters[rc.rec] = n_it;
    }
}

static size_t vb_blob_add(std::vector<char>& blob, const void* src, size_t bytes) {
    const size_t at = (blob.size() + 15) / 16 * 16;
    blob.resize(at + bytes);
    if (bytes) std::memcpy(blob.data() + at, src, bytes);
    return at;
}

template <int NS>
static int vb_launch(bool res, unsigned blocks, size_t lds, hipStream_t s, const VbArgs& a, int alpha_in_lds) {
    if (res) {
        SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(vb_hmm_kernel<NS, true>), hipFuncAttributeMaxDynamicSharedMemorySize, VB_LDS_BYTES));
        hipLaunchKernelGGL((vb_hmm_kernel<NS, true>), dim3(blocks), dim3(256), lds, s, a, alpha_in_lds);
    } else {
        SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(vb_hmm_kernel<NS, false>), hipFuncAttributeMaxDynamicSharedMemorySize, VB_LDS_BYTES));
        hipLaunchKernelGGL((vb_hmm_kernel<NS, false>), dim3(blocks), dim3(256), lds, s, a, alpha_in_lds);
    }
    return SSP_OK;
}

}  // namespace ssp

using namespace ssp;

extern "C" int ssp_vbhmm_resegment(ssp_ctx* ctx, const float* X, const ssp_segments* seg, int32_t q, const float* phi, const int32_t* init_labels,
                                   const int32_t* n_init, int32_t S, float loop_prob, float Fa, float Fb, float init_smoothing,
                                   int32_t max_iters, double epsilon, int32_t* labels_out, int32_t* states_out, int32_t* n_speakers_out,
                                   int32_t* n_iters_out, double* elbo_out, float* gamma_out, float* pi_out, float* loglik_out, int where,
                                   float* kernel_ms) {
    ssp::TraceRange trace_("ssp_vbhmm_resegment");
    const char* who = "ssp_vbhmm_resegment";
    if (!ctx) SSP_FAIL(SSP_ERR_INVALID, "null ssp_ctx");
    if (!seg) SSP_FAIL(SSP_ERR_INVALID, "%s: null segments", who);
    if (q < 1 || S < 1 || max_iters < 1) SSP_FAIL(SSP_ERR_INVALID, "%s: q=%d, S=%d, max_iters=%d", who, q, S, max_iters);
    if (!(loop_prob >= 0.f && loop_prob < 1.f)) SSP_FAIL(SSP_ERR_INVALID, "%s: loop_prob=%g is outside [0, 1)", who, (double)loop_prob);
    if (!(std::isfinite(Fa) && Fa > 0.f && std::isfinite(Fb) && Fb > 0.f)) SSP_FAIL(SSP_ERR_INVALID, "%s: Fa=%g, Fb=%g", who, (double)Fa, (double)Fb);
    if (!(std::isfinite(init_smoothing) && init_smoothing >= 0.f)) SSP_FAIL(SSP_ERR_INVALID, "%s: init_smoothing=%g", who, (double)init_smoothing);
    if (epsilon != epsilon) SSP_FAIL(SSP_ERR_INVALID, "%s: epsilon is NaN", who);
    if (!phi) SSP_FAIL(SSP_ERR_INVALID, "%s: null phi", who);
    for (int d = 0; d < q && d < VB_MAX_Q; ++d)
        if (!(std::isfinite(phi[d]) && phi[d] >= 0.f)) SSP_FAIL(SSP_ERR_INVALID, "%s: phi[%d]=%g", who, d, (double)phi[d]);
    SSP_TRY(check_where(where, who));
    if (S > VB_MAX_S || q > VB_MAX_Q || max_iters > VB_MAX_ITERS)
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: S=%d, q=%d, max_iters=%d exceed the supported %d, %d, %d", who, S, q, max_iters, VB_MAX_S, VB_MAX_Q, VB_MAX_ITERS);
    for (int64_t r = 0; r < seg->n; ++r)
        if (seg->host[(size_t)r + 1] - seg->host[(size_t)r] > VB_MAX_N)
            SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: recording %lld has %lld rows, more than the supported %d", who, (long long)r,
                     (long long)(seg->host[(size_t)r + 1] - seg->host[(size_t)r]), VB_MAX_N);
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (seg->n == 0) return SSP_OK;
    const int SP = S <= 16 ? 16 : (S <= 32 ? 32 : 64), ldq = q | 1;
    const size_t alpha_floats = (size_t)SP * (size_t)ldq;
    const int alpha_in_lds = alpha_floats * sizeof(float) <= (size_t)VB_ALPHA_LDS;
    const size_t lds_alpha = alpha_in_lds ? alpha_floats * sizeof(float) : 0;
    const int n_lds = (int)((VB_LDS_BYTES - lds_alpha) / (2 * (size_t)SP * sizeof(float)));  // rows whose two buffers fit beside alpha
    std::vector<VbRec> recs;
    int64_t ws_floats = 0;
    for (int64_t r = 0; r < seg->n; ++r) {
        const int64_t n = seg->host[(size_t)r + 1] - seg->host[(size_t)r];
        if (n <= 0) continue;
        VbRec d{seg->host[(size_t)r], ws_floats, (int32_t)n, (int32_t)r};
        ws_floats += (alpha_in_lds ? 0 : (int64_t)alpha_floats) + (n > n_lds ? 2 * n * SP : 0);
        recs.push_back(d);
    }
    if (recs.empty()) return SSP_OK;  // (recordings without rows are not written)
    if (!X || !init_labels || !labels_out || !n_speakers_out || !n_iters_out)
        SSP_FAIL(SSP_ERR_INVALID, "%s: null X, init_labels, labels_out, n_speakers_out or n_iters_out", who);
    const int64_t rows = seg->host.back(), row0 = seg->host.front(), R = seg->n;
    std::stable_sort(recs.begin(), recs.end(), [](const VbRec& x, const VbRec& y) { return x.n > y.n; });
    size_t first_res = 0;
    while (first_res < recs.size() && recs[first_res].n > n_lds) ++first_res;
    std::vector<float> tab(2 * (size_t)q);
    for (int d = 0; d < q; ++d) {
        tab[(size_t)d] = (float)std::sqrt((double)phi[d]);
        tab[(size_t)q + d] = phi[d];
    }
    std::vector<char>& blob = ctx->diar_host;
    blob.clear();
    const size_t at_recs = vb_blob_add(blob, recs.data(), recs.size() * sizeof(VbRec));
    const size_t at_tab = vb_blob_add(blob, tab.data(), tab.size() * sizeof(float));
    hipStream_t s = ctx->stream;
    SSP_TRY(ctx->diar_tab.reserve(blob.size()));
    SSP_TRY(ctx->diar_r.reserve((size_t)rows * sizeof(float)));
    if (ws_floats) SSP_TRY(ctx->diar_ws.reserve((size_t)ws_floats * sizeof(float)));
    SSP_HIP(hipMemcpyAsync(ctx->diar_tab.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
    // what no workgroup writes (rows before offsets[0], the entries of recordings without rows) keeps the caller's bytes: the per-recording
    // outputs are pre-loaded whole, of the per-row outputs the `lead` rows
    StageScope st(ctx, where);
    const float* dX = st.in(X, (size_t)rows * (size_t)q * sizeof(float));
    const int32_t* dI = st.in(init_labels, (size_t)rows * sizeof(int32_t));
    const int32_t* dNi = st.in(n_init, (size_t)R * sizeof(int32_t));
    int32_t* dL = st.out(labels_out, (size_t)rows * sizeof(int32_t));
    int32_t* dSt = st.out(states_out, (size_t)rows * sizeof(int32_t));
    int32_t* dNs = st.out(n_speakers_out, (size_t)R * sizeof(int32_t), true);
    int32_t* dIt = st.out(n_iters_out, (size_t)R * sizeof(int32_t), true);
    double* dE = st.out(elbo_out, (size_t)R * (size_t)max_iters * sizeof(double), true);
    float* dG = st.out(gamma_out, (size_t)rows * (size_t)S * sizeof(float));
    float* dP = st.out(pi_out, (size_t)R * (size_t)S * sizeof(float), true);
    float* dLl = st.out(loglik_out, (size_t)rows * (size_t)S * sizeof(float));
    SSP_TRY(st.status());
    if (where == SSP_HOST && row0 > 0) {
        const size_t lead = (size_t)row0;
        SSP_HIP(hipMemcpyAsync(dL, labels_out, lead * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (dSt) SSP_HIP(hipMemcpyAsync(dSt, states_out, lead * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (dG) SSP_HIP(hipMemcpyAsync(dG, gamma_out, lead * (size_t)S * sizeof(float), hipMemcpyHostToDevice, s));
        if (dLl) SSP_HIP(hipMemcpyAsync(dLl, loglik_out, lead * (size_t)S * sizeof(float), hipMemcpyHostToDevice, s));
    }
    const char* dtab = ctx->diar_tab.as<char>();
    const VbRec* dRecs = reinterpret_cast<const VbRec*>(dtab + at_recs);
    const float* dTab = reinterpret_cast<const float*>(dtab + at_tab);
    VbArgs a{dX, ctx->diar_r.as<float>(), dTab, dTab + q, dRecs, dI, dNi, ctx->diar_ws.as<float>(), dL, dSt, dNs, dIt, dE, dG, dP, dLl,
             q, S, max_iters, loop_prob, Fa, Fb, init_smoothing, epsilon};
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    hipLaunchKernelGGL(vb_rowstat_kernel, dim3((unsigned)ceil_div<int64_t>(rows - row0, 4)), dim3(256), 0, s, dX, row0, rows - row0, q,
                       ctx->diar_r.as<float>());
    for (int b = 0; b < 2; ++b) {  // the workspace-resident recordings, then the LDS-resident ones (the LDS a workgroup takes follows the launch's longest)
        const size_t lo = b == 0 ? 0 : first_res, hi = b == 0 ? first_res : recs.size();
        if (lo == hi) continue;
        a.recs = dRecs + lo;
        const size_t lds = lds_alpha + (b == 0 ? 0 : 2 * (size_t)recs[lo].n * (size_t)SP * sizeof(float));
        if (SP == 16)
            SSP_TRY(vb_launch<1>(b == 1, (unsigned)(hi - lo), lds, s, a, alpha_in_lds));
        else if (SP == 32)
            SSP_TRY(vb_launch<2>(b == 1, (unsigned)(hi - lo), lds, s, a, alpha_in_lds));
        else
            SSP_TRY(vb_launch<4>(b == 1, (unsigned)(hi - lo), lds, s, a, alpha_in_lds));
    }
    SSP_HIP(hipGetLastError());
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}
