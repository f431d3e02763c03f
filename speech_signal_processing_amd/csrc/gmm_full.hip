// Full-covariance GMMs on gfx950: EM sufficient statistics (ssp_gmm_full_em_stats) and scoring (ssp_gmm_full_*), the O(frames x K x D^2)
// part of sklearn's GaussianMixture(covariance_type='full') — mixture/_gaussian_mixture.py:_estimate_log_gaussian_prob ('full' branch),
// _estimate_log_prob_resp, _estimate_gaussian_parameters / _estimate_gaussian_covariances_full — restated in include/ssp.h.
//
// Model on the device.  Mixture k is one fp32 image [KR][Dp] (k-major) of the AUGMENTED factor and one constant:
//   row 0        -(mu_k - c) U_k          the constant row: aug column 0 of a frame is 1
//   row 1 + d    U_k[d][.]                upper triangle, zeros below it (never read from the caller's array)
//   cst_k        log w_k - D/2 log 2 pi + sum_j log U_k[j][j]          (-1e30 for a mixture of weight 0: it does not exist)
// Dp = D rounded up to 32 (zero columns), KR = D + 1 rounded up to 2 (a zero row), c the caller's shift; mu - c is formed in float64.
//
// E pass (gmm_full_e_kernel<NRT>, NRT = Dp / 32).  Workgroup = 256 frames, wave = 64 of them (two 32-frame column tiles); the frame tile
// aug = [1, x - c, 0] sits in LDS for the whole walk over the mixtures, a mixture's image is staged in LDS while the one before is used.
//   y^T[Dp x 64] = image^T . aug^T  on v_mfma_f32_32x32x2_f32: the columns j of y are MFMA rows, frames are MFMA columns, so the 16
//   accumulators of a lane belong to ONE frame.  Row tile r (columns 32 r .. 32 r + 31 of U) needs the k-steps up to image row 32 r + 32
//   only (U is triangular): the steps beyond are skipped.
//   lp = cst - 1/2 sum_j y_j^2 (in-lane squares, one exchange between the two half-waves), then an online (max, sum) per frame over the
//   mixtures of a model.  EM: lp goes to the workspace lp[k][frame]; the scorer keeps nothing but the model's log-sum-exp.
// Moment pass (gmm_full_mom_kernel<NT>, NT = ceil((D + 1) / 32)).  Grid (walkers, K / 4): wave w of a workgroup owns mixture 4 y + w and
// accumulates S_k = sum_t resp_tk aug_t aug_t^T (nk = S[0][0], sx = S[0][1..], sxx = S[1..][1..]) over the walker's 64-frame tiles
// (tiles g, g + G, ...), frames as the MFMA reduction dimension, the UPPER block triangle of 32 x 32 tiles only; resp = exp(lp - lse).
// A walker adds at most FG_CAP_TILES tiles = 8192 frames into one fp32 accumulator; the partials [G][K][tiles][32][32] are added in
// float64 in walker order by gmm_full_reduce_kernel, which reads entry (i, j) and (j, i) from the same cell: sxx is exactly symmetric.
// Frames go through both passes in slabs so that lp[K][slab] respects SSP_GMM_FULL_SCRATCH_MB (default 256); the float64 sums carry on
// from slab to slab in slab order.  No atomics anywhere: the same call gives the same bits.
#include <cmath>

#include "common.hpp"
#include "handle.hpp"

namespace ssp {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int FG_TF = 256;         // frames per workgroup of the E pass (4 waves x 64)
constexpr int FG_MT = 64;          // frames per tile of the moment pass
constexpr int FG_MW = 4;           // mixtures per workgroup of the moment pass (one per wave)
constexpr int FG_CAP_TILES = 128;  // moment tiles per walker: 8192 frames per fp32 accumulator
constexpr int FG_MAX_D = 64;
constexpr float FG_PAD_CONST = -1.0e30f;

extern __shared__ __attribute__((aligned(16))) float fg_sm[];

struct FgEArgs {
    const float* x;      // frame t of the launch at x + t D
    const float* shift;  // [D] (always set: zeros without a shift)
    const float* img;    // [M K][KR][Dp]
    const float* cst;    // [M K]
    float* lp;           // EM: [K][ld]; scorer: null
    float* ll;           // [M][ldll]: per-frame log-sum-exp of every model (NaN for a bad frame)
    float* lse_part;     // EM: one sum of ll per workgroup; scorer: null
    int64_t n, ld, ldll;
    int32_t D, K, M, KS;
};

template <int NRT>
__global__ __launch_bounds__(256) void gmm_full_e_kernel(FgEArgs a) {
    constexpr int Dp = 32 * NRT;
    constexpr int NV = NRT == 1 ? 2 : 5;  // float4 per thread that cover one image: 34 x 32 <= 2048, 66 x 64 <= 5120 floats
    const int D = a.D, KS = a.KS, KR = 2 * KS, XS = KR | 1, IMG = KR * Dp;
    float* xs = fg_sm;              // [256 frames][XS]  aug = [1, x - c, 0]
    float* ub = xs + FG_TF * XS;    // [KR][Dp]          the image of the mixture in hand
    float* red = ub + IMG;          // [4]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fl = lane & 31, h = lane >> 5;
    const int64_t base = (int64_t)blockIdx.x * FG_TF;
    const int nt = (int)min<int64_t>(FG_TF, a.n - base);
    for (int i = tid; i < FG_TF * KR; i += 256) {
        const int r = i / KR, c = i - r * KR;
        float v = c == 0 ? 1.f : 0.f;
        if (c >= 1 && c <= D) v = r < nt ? a.x[(base + r) * D + (c - 1)] - a.shift[c - 1] : 0.f;
        xs[r * XS + c] = v;
    }
    const int total = a.M * a.K;
    float4 pre[NV];
    auto fetch = [&](int mix) {
        const float4* p = reinterpret_cast<const float4*>(a.img + (size_t)mix * IMG);
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int i = tid + u * 256;
            pre[u] = (mix < total && 4 * i < IMG) ? p[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    fetch(0);
    const float* ua = ub + h * Dp + fl;                  // A[row = column j of U][k = image row 2 s + h]
    const float* xb0 = xs + (wave * 64 + fl) * XS + h;   // B[k = aug column 2 s + h][col = frame]
    const float* xb1 = xb0 + 32 * XS;
    const int KS0 = KS < 17 ? KS : 17;  // row tile 0 holds columns 0 .. 31 of U: nothing below image row 32
    float mx[2] = {-INFINITY, -INFINITY}, sum[2] = {0.f, 0.f}, lsum = 0.f;
    int k = 0, m = 0;
    for (int mix = 0; mix < total; ++mix) {
        __syncthreads();  // the mixture before is done with ub (first turn: nothing)
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int i = tid + u * 256;
            if (4 * i < IMG) reinterpret_cast<float4*>(ub)[i] = pre[u];
        }
        fetch(mix + 1);
        __syncthreads();
        f32x16 acc[NRT][2];
#pragma unroll
        for (int r = 0; r < NRT; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[r][c][i] = 0.f;
        int s = 0;
#pragma unroll 2
        for (; s < KS0; ++s) {
            const float b0 = xb0[2 * s], b1 = xb1[2 * s];
            const float a0 = ua[2 * s * Dp];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            if constexpr (NRT == 2) {
                const float a1 = ua[2 * s * Dp + 32];
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        if constexpr (NRT == 2) {
#pragma unroll 2
            for (; s < KS; ++s) {
                const float b0 = xb0[2 * s], b1 = xb1[2 * s];
                const float a1 = ua[2 * s * Dp + 32];
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        const float cst = a.cst[mix];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float ss = 0.f;
#pragma unroll
            for (int r = 0; r < NRT; ++r)
#pragma unroll
                for (int i = 0; i < 16; ++i) ss = fmaf(acc[r][c][i], acc[r][c][i], ss);
            ss += __shfl_xor(ss, 32);
            const float lp = cst - 0.5f * ss;
            const int t = wave * 64 + c * 32 + fl;
            if (a.lp && h == 0 && t < nt) a.lp[(size_t)k * a.ld + base + t] = lp;
            const float mn = fmaxf(mx[c], lp);
            sum[c] = sum[c] * __expf(mx[c] - mn) + __expf(lp - mn);
            mx[c] = mn;
        }
        if (++k == a.K) {  // the model is complete: its log-sum-exp per frame
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                float l = mx[c] + __logf(sum[c]);
                if (!(fabsf(l) < INFINITY)) l = __builtin_nanf("");  // a bad frame is NaN under every model, never -inf
                const int t = wave * 64 + c * 32 + fl;
                if (h == 0 && t < nt) {
                    a.ll[(size_t)m * a.ldll + base + t] = l;
                    lsum += l;
                }
                mx[c] = -INFINITY;
                sum[c] = 0.f;
            }
            k = 0;
            ++m;
        }
    }
    if (a.lse_part) {  // the sum of this workgroup's 256 values, in a fixed shape
        for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o);
        __syncthreads();
        if (lane == 0) red[wave] = lsum;
        __syncthreads();
        if (tid == 0) a.lse_part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

struct FgMArgs {
    const float* x;      // frame t of the slab at x + t D
    const float* shift;  // [D]
    const float* lp;     // [K][ld]
    const float* lse;    // [n]
    float* part;         // [G][K][NT (NT + 1) / 2][32][32]
    int64_t n, ld;
    int32_t D, K, G, n_tiles;
};

template <int NT>
__global__ __launch_bounds__(256) void gmm_full_mom_kernel(FgMArgs a) {
    constexpr int WA = 32 * NT, XS = NT == 2 ? 96 : WA;  // the two rows of a k-step lie 32 banks apart
    constexpr int NTRI = NT * (NT + 1) / 2;
    constexpr int XP = 16;                               // floats per thread that cover a frame tile: 64 x D <= 4096
    float* xs = fg_sm;                                   // [64 frames][XS]  aug = [1, x - c, 0]
    const int D = a.D;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fl = lane & 31, h = lane >> 5;
    const int k = blockIdx.y * FG_MW + wave;
    const bool live = k < a.K;  // (wave-uniform)
    for (int i = tid; i < FG_MT * XS; i += 256) {
        const int c = i % XS;
        xs[i] = c == 0 ? 1.f : 0.f;  // the constant and the pad columns, written once
    }
    f32x16 acc[NTRI];
#pragma unroll
    for (int q = 0; q < NTRI; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
    float xpre[XP], rpre = 0.f;
    auto fetch = [&](int tile) {
        const int64_t base = (int64_t)tile * FG_MT;
        const int nt = tile < a.n_tiles ? (int)min<int64_t>(FG_MT, a.n - base) : 0;
#pragma unroll
        for (int u = 0; u < XP; ++u) {
            const int i = tid + u * 256;
            const int r = i / D, c = i - r * D;
            xpre[u] = (i < FG_MT * D && r < nt) ? a.x[base * D + i] - a.shift[c] : 0.f;
        }
        // frames past the end carry no mass; a bad frame's lse is NaN and so is its responsibility under every mixture
        rpre = (live && lane < nt) ? __expf(a.lp[(size_t)k * a.ld + base + lane] - a.lse[base + lane]) : 0.f;
    };
    fetch(blockIdx.x);
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += a.G) {
        __syncthreads();  // the tile before is done with xs
#pragma unroll
        for (int u = 0; u < XP; ++u) {
            const int i = tid + u * 256;
            if (i < FG_MT * D) {
                const int r = i / D, c = i - r * D;
                xs[r * XS + 1 + c] = xpre[u];
            }
        }
        const float rv = rpre;
        fetch(tile + a.G);
        __syncthreads();
        if (live) {
#pragma unroll 4
            for (int s = 0; s < FG_MT / 2; ++s) {
                const int f = 2 * s + h;  // A[row = aug index][k = frame f] = resp aug, B[k = frame f][col = aug index] = aug
                const float r = __shfl(rv, f);
                float bv[NT], av[NT];
#pragma unroll
                for (int c = 0; c < NT; ++c) {
                    bv[c] = xs[f * XS + 32 * c + fl];
                    av[c] = r * bv[c];
                }
                int q = 0;
#pragma unroll
                for (int rr = 0; rr < NT; ++rr)
#pragma unroll
                    for (int c = rr; c < NT; ++c, ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[rr], bv[c], acc[q], 0, 0, 0);
            }
        }
    }
    if (live) {
        float* out = a.part + ((size_t)blockIdx.x * a.K + k) * (NTRI * 1024);
#pragma unroll
        for (int q = 0; q < NTRI; ++q)
#pragma unroll
            for (int i = 0; i < 16; ++i) out[q * 1024 + ((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + fl] = acc[q][i];
    }
}

// out[k][i][j] (+)= sum_g part[g][k][tile of (min, max)][min & 31][max & 31] in float64, walker order; i, j index aug = [1, x - c]
__global__ __launch_bounds__(256) void gmm_full_reduce_kernel(const float* __restrict__ part, int G, int K, int D, int NT, double* out, int first) {
    const int W = D + 1;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)K * W * W) return;
    const int k = (int)(idx / (W * W)), rem = (int)(idx - (int64_t)k * W * W);
    const int i = rem / W, j = rem - i * W;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int r = lo >> 5, c = hi >> 5;
    const int ntri = NT * (NT + 1) / 2;
    const size_t off = (size_t)(r * NT - r * (r - 1) / 2 + (c - r)) * 1024 + (lo & 31) * 32 + (hi & 31);
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += (double)part[((size_t)g * K + k) * ((size_t)ntri * 1024) + off];
    out[idx] = first ? s : out[idx] + s;
}

// out[0] (+)= sum of the E pass's workgroup sums: fixed strided order, then a tree
__global__ __launch_bounds__(256) void gmm_full_lse_reduce_kernel(const float* __restrict__ lse_part, int64_t n, double* out, int first) {
    __shared__ double sh[256];
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) v += (double)lse_part[i];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = first ? sh[0] : out[0] + sh[0];
}

// per-utterance means of ll[M][ld] (columns frame_off[u] - frame_base ..) and the arg-max of score - UBM score: ssp_gmm_score's rules
// (an empty utterance and one with a bad frame: a NaN row and arg-max 0; ties to the first index)
__global__ __launch_bounds__(256) void gmm_full_utt_kernel(const float* __restrict__ ll, int64_t ld, const int64_t* __restrict__ frame_off,
                                                           int64_t frame_base, int n_models, int has_ubm, float* __restrict__ scores,
                                                           int32_t* __restrict__ argmax_out) {
    float* sc = fg_sm;
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t a0 = frame_off[u] - frame_base;
    const int64_t T = frame_off[u + 1] - frame_off[u];
    for (int m = wave; m < n_models; m += 4) {
        const float* __restrict__ p = ll + (size_t)m * ld + a0;
        float s = 0.f;
        for (int64_t t = lane; t < T; t += 64) s += p[t];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float v = s / (float)T;  // T == 0: NaN, numpy's mean of nothing
        if (lane == 0) {
            sc[m] = v;
            if (scores) scores[(size_t)u * n_models + m] = v;
        }
    }
    __syncthreads();
    if (wave == 0 && argmax_out) {
        const float ref = has_ubm ? sc[0] : 0.f;
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int m = has_ubm + lane; m < n_models; m += 64) {
            const float v = sc[m] - ref;
            if (v > best || bi == 0x7fffffff) {
                best = v;
                bi = m - has_ubm;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) {
                best = ob;
                bi = oi;
            }
        }
        if (lane == 0) argmax_out[u] = bi == 0x7fffffff ? 0 : bi;
    }
}

// ---- host side
struct FgGeom {
    int D, NRT, Dp, KS, KR, IMG, NT;
    explicit FgGeom(int d) : D(d), NRT(d <= 32 ? 1 : 2), Dp(32 * NRT), KS((d + 2) / 2), KR(2 * KS), IMG(KR * Dp), NT((d + 1 + 31) / 32) {}
    size_t e_lds() const { return ((size_t)FG_TF * (KR | 1) + IMG + 8) * sizeof(float); }
    size_t m_lds() const { return (size_t)FG_MT * (NT == 2 ? 96 : 32 * NT) * sizeof(float); }
};

static int64_t fg_budget_bytes() {
    int64_t mb = 256;
    if (const char* e = getenv("SSP_GMM_FULL_SCRATCH_MB")) mb = std::max<int64_t>(1, atoll(e));
    return mb << 20;
}

// float64 parameters of n_models models -> images, constants and the shift: par = [n_models K IMG | n_models K | D] floats, zeroed by
// the caller.  Validation first: nothing is written for a model set that is refused.
static int fg_pack(const char* fn, int n_models, int K, int D, const double* weights, const double* means, const double* U, const double* shift,
                   const FgGeom& g, float* par) {
    for (int m = 0; m < n_models; ++m) {
        bool any = false;
        for (int k = 0; k < K; ++k) {
            const double wk = weights[(size_t)m * K + k];
            if (!(wk >= 0.0) || std::isinf(wk)) SSP_FAIL(SSP_ERR_INVALID, "%s: negative or non-finite weight (model %d, mix %d)", fn, m, k);
            any = any || wk > 0.0;
            const double* mu = means + ((size_t)m * K + k) * D;
            const double* u = U + ((size_t)m * K + k) * D * D;
            for (int d = 0; d < D; ++d) {
                if (!std::isfinite(mu[d])) SSP_FAIL(SSP_ERR_INVALID, "%s: non-finite mean (model %d, mix %d)", fn, m, k);
                if (!(u[(size_t)d * D + d] > 0.0) || !std::isfinite(u[(size_t)d * D + d]))
                    SSP_FAIL(SSP_ERR_INVALID, "%s: a diagonal entry of precisions_cholesky is not finite and > 0 (model %d, mix %d)", fn, m, k);
                for (int j = d + 1; j < D; ++j)
                    if (!std::isfinite(u[(size_t)d * D + j]))
                        SSP_FAIL(SSP_ERR_INVALID, "%s: non-finite entry in the upper triangle of precisions_cholesky (model %d, mix %d)", fn, m, k);
            }
        }
        if (!any) SSP_FAIL(SSP_ERR_INVALID, "%s: every weight of model %d is zero", fn, m);
    }
    if (shift)
        for (int d = 0; d < D; ++d)
            if (!std::isfinite(shift[d])) SSP_FAIL(SSP_ERR_INVALID, "%s: non-finite shift", fn);
    const size_t total = (size_t)n_models * K;
    float* cst = par + total * g.IMG;
    float* sh = cst + total;
    const double ln2pi = std::log(2.0 * M_PI);
    for (int d = 0; d < D; ++d) sh[d] = shift ? (float)shift[d] : 0.f;
    for (size_t mk = 0; mk < total; ++mk) {
        const double wk = weights[mk];
        const double* mu = means + mk * D;
        const double* u = U + mk * D * D;
        float* img = par + mk * g.IMG;
        double c = std::log(wk > 0.0 ? wk : 1.0) - 0.5 * D * ln2pi;
        for (int j = 0; j < D; ++j) {
            double b = 0.0;
            for (int d = 0; d <= j; ++d) {
                b -= (mu[d] - (shift ? shift[d] : 0.0)) * u[(size_t)d * D + j];
                img[(size_t)(1 + d) * g.Dp + j] = (float)u[(size_t)d * D + j];
            }
            img[j] = (float)b;
            c += std::log(u[(size_t)j * D + j]);
        }
        cst[mk] = wk > 0.0 ? (float)c : FG_PAD_CONST;
    }
    return SSP_OK;
}

static int fg_launch_e(const FgGeom& g, const FgEArgs& a, hipStream_t s) {
    if (a.n <= 0) return SSP_OK;
    const size_t lds = g.e_lds();
    const void* kf = g.NRT == 1 ? reinterpret_cast<const void*>(gmm_full_e_kernel<1>) : reinterpret_cast<const void*>(gmm_full_e_kernel<2>);
    if (lds > 64 * 1024) SSP_HIP(hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t tiles = (a.n + FG_TF - 1) / FG_TF;
    if (tiles > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "gmm_full: too many frames");
    if (g.NRT == 1) hipLaunchKernelGGL(gmm_full_e_kernel<1>, dim3((unsigned)tiles), dim3(256), lds, s, a);
    else hipLaunchKernelGGL(gmm_full_e_kernel<2>, dim3((unsigned)tiles), dim3(256), lds, s, a);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

}  // namespace ssp

using namespace ssp;

struct ssp_gmm_full {
    ssp_ctx* ctx = nullptr;
    int n_models = 0, K = 0, D = 0, has_ubm = 0;
    ssp::DevBuf par;  // images, constants, a zero shift
    ssp::DevBuf ws;   // ll[M][slab] of the calls that ask for no loglik_out
};

extern "C" int ssp_gmm_full_em_stats(ssp_ctx* ctx, int32_t K, int32_t D, const double* weights, const double* means, const double* prec_chol,
                                     const double* shift, const float* feats, int64_t n_frames, double* nk_out, double* sx_out,
                                     double* sxx_out, double* loglik_sum_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_gmm_full_em_stats");
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (K < 1 || D < 1 || !weights || !means || !prec_chol || !nk_out || !sx_out || !sxx_out || !loglik_sum_out)
        SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_full_em_stats: bad shape or null array");
    if (D > FG_MAX_D) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_gmm_full_em_stats: D=%d exceeds the supported feature dimension (%d)", D, FG_MAX_D);
    if (n_frames < 1 || !feats) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_full_em_stats: no frames");
    SSP_TRY(check_where(where, "ssp_gmm_full_em_stats"));
    const FgGeom g(D);
    const size_t par_n = (size_t)K * g.IMG + K + D;
    std::vector<float> par(par_n, 0.f);
    SSP_TRY(fg_pack("ssp_gmm_full_em_stats", 1, K, D, weights, means, prec_chol, shift, g, par.data()));
    hipStream_t s = ctx->stream;
    // slabs: lp[K][slab] within the budget, whole E-pass tiles
    int64_t slab = fg_budget_bytes() / ((int64_t)K * (int64_t)sizeof(float)) / FG_TF * FG_TF;
    slab = std::max<int64_t>(FG_TF, std::min<int64_t>(slab, (n_frames + FG_TF - 1) / FG_TF * FG_TF));
    const int64_t slab_tiles = slab / FG_MT, e_tiles = slab / FG_TF;
    if (slab_tiles > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_gmm_full_em_stats: too many frames");
    const int groups = (K + FG_MW - 1) / FG_MW;
    const int ntri = g.NT * (g.NT + 1) / 2;
    auto walkers = [&](int64_t n_tiles) {
        const int64_t want = std::max<int64_t>(1, 2 * (int64_t)ctx->num_cu / groups);
        return (int)std::max<int64_t>((n_tiles + FG_CAP_TILES - 1) / FG_CAP_TILES, std::min<int64_t>(n_tiles, want));
    };
    const int G_max = walkers(slab_tiles);
    const int W = D + 1;
    const int64_t cells = (int64_t)K * W * W;
    DevBuf &d_par = ctx->scratch[0], &d_lp = ctx->scratch[1], &d_lse = ctx->scratch[2], &d_part = ctx->scratch[3], &d_out = ctx->scratch[4];
    StageScope st(ctx, where);
    const float* d_x = st.in(feats, (size_t)n_frames * D * sizeof(float));
    SSP_TRY(st.status());
    SSP_TRY(d_par.reserve(par_n * sizeof(float)));
    SSP_TRY(d_lp.reserve((size_t)K * slab * sizeof(float)));
    SSP_TRY(d_lse.reserve((size_t)(slab + e_tiles) * sizeof(float)));
    SSP_TRY(d_part.reserve((size_t)G_max * K * ntri * 1024 * sizeof(float)));
    SSP_TRY(d_out.reserve((size_t)(cells + 1) * sizeof(double)));
    SSP_HIP(hipMemcpyAsync(d_par.p, par.data(), par_n * sizeof(float), hipMemcpyHostToDevice, s));
    const float* d_img = d_par.as<float>();
    const float* d_cst = d_img + (size_t)K * g.IMG;
    const float* d_shift = d_cst + K;
    float* d_lsep = d_lse.as<float>() + slab;
    const size_t mlds = g.m_lds();
    Timer tm;
    int rc = tm.start(kernel_ms != nullptr, s);
    for (int64_t f0 = 0; rc == SSP_OK && f0 < n_frames; f0 += slab) {
        const int64_t n = std::min<int64_t>(slab, n_frames - f0);
        const int first = f0 == 0 ? 1 : 0;
        FgEArgs ea{d_x + (size_t)f0 * D, d_shift, d_img, d_cst, d_lp.as<float>(), d_lse.as<float>(), d_lsep, n, slab, slab, D, K, 1, g.KS};
        rc = fg_launch_e(g, ea, s);
        if (rc != SSP_OK) break;
        const int64_t n_tiles = (n + FG_MT - 1) / FG_MT;
        const int G = walkers(n_tiles);
        FgMArgs ma{d_x + (size_t)f0 * D, d_shift, d_lp.as<float>(), d_lse.as<float>(), d_part.as<float>(), n, slab, D, K, G, (int32_t)n_tiles};
        const dim3 grid((unsigned)G, (unsigned)groups);
        switch (g.NT) {
            case 1: hipLaunchKernelGGL(gmm_full_mom_kernel<1>, grid, dim3(256), mlds, s, ma); break;
            case 2: hipLaunchKernelGGL(gmm_full_mom_kernel<2>, grid, dim3(256), mlds, s, ma); break;
            default: hipLaunchKernelGGL(gmm_full_mom_kernel<3>, grid, dim3(256), mlds, s, ma); break;
        }
        hipLaunchKernelGGL(gmm_full_reduce_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, d_part.as<float>(), G, K, D, g.NT,
                           d_out.as<double>(), first);
        hipLaunchKernelGGL(gmm_full_lse_reduce_kernel, dim3(1), dim3(256), 0, s, d_lsep, (n + FG_TF - 1) / FG_TF, d_out.as<double>() + cells, first);
        if (hipGetLastError() != hipSuccess) {
            set_error("ssp_gmm_full_em_stats: kernel launch failed");
            rc = SSP_ERR_HIP;
        }
    }
    if (rc == SSP_OK) rc = tm.stop(s, kernel_ms);
    if (rc != SSP_OK) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    std::vector<double> host((size_t)cells + 1);
    hipError_t he = hipMemcpyAsync(host.data(), d_out.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) SSP_FAIL(SSP_ERR_HIP, "ssp_gmm_full_em_stats: result copy failed: %s", hipGetErrorString(he));
    for (int k = 0; k < K; ++k) {
        const double* o = host.data() + (size_t)k * W * W;
        nk_out[k] = o[0];
        for (int d = 0; d < D; ++d) {
            sx_out[(size_t)k * D + d] = o[1 + d];
            for (int e = 0; e < D; ++e) sxx_out[((size_t)k * D + d) * D + e] = o[(size_t)(1 + d) * W + 1 + e];
        }
    }
    *loglik_sum_out = host[(size_t)cells];
    return SSP_OK;
}

extern "C" int ssp_gmm_full_pack(ssp_ctx* ctx, int32_t n_models, int32_t K, int32_t D, const double* weights, const double* means,
                                 const double* prec_chol, int32_t has_ubm, ssp_gmm_full** out) try {
    ssp::TraceRange trace_("ssp_gmm_full_pack");
    if (!out) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_full_pack: null out");
    *out = nullptr;
    SSP_TRY(use_ctx(ctx));
    if (n_models < 1 || K < 1 || D < 1 || !weights || !means || !prec_chol)
        SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_full_pack: bad shape or null parameter array");
    if (has_ubm && n_models < 2) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_full_pack: has_ubm needs at least one speaker model");
    if (D > FG_MAX_D) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_gmm_full_pack: D=%d exceeds the supported feature dimension (%d)", D, FG_MAX_D);
    if ((int64_t)n_models * K > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_gmm_full_pack: too many mixtures");
    const FgGeom g(D);
    const size_t par_n = (size_t)n_models * K * g.IMG + (size_t)n_models * K + D;
    std::vector<float> par(par_n, 0.f);
    SSP_TRY(fg_pack("ssp_gmm_full_pack", n_models, K, D, weights, means, prec_chol, nullptr, g, par.data()));
    HandleBuild<ssp_gmm_full> h(ctx, "ssp_gmm_full_pack");
    h->n_models = n_models;
    h->K = K;
    h->D = D;
    h->has_ubm = has_ubm ? 1 : 0;
    return h.commit(upload(h, h->par, par), out);
}
SSP_CREATE_GUARD("ssp_gmm_full_pack")

extern "C" int ssp_gmm_full_destroy(ssp_gmm_full* h) { return destroy_handle(h); }

extern "C" int ssp_gmm_full_score(ssp_gmm_full* h, const float* feats, const ssp_segments* frame_seg, float* loglik_out, float* scores_out,
                                  int32_t* argmax_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_gmm_full_score");
    if (!h || !frame_seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_full_score: null handle");
    ssp_ctx* ctx = h->ctx;
    SSP_TRY(use_ctx(ctx));
    SSP_TRY(check_where(where, "ssp_gmm_full_score"));
    if (kernel_ms) *kernel_ms = 0.f;
    const int64_t F = frame_seg->host.back();
    const int64_t n_utt = frame_seg->n;
    if (n_utt == 0) return SSP_OK;
    if (F > 0 && !feats) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_full_score: null feats");
    if (n_utt > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_gmm_full_score: too many utterances");
    hipStream_t s = ctx->stream;
    const int M = h->n_models, K = h->K, D = h->D;
    const FgGeom g(D);
    const float* d_img = h->par.as<float>();
    const float* d_cst = d_img + (size_t)M * K * g.IMG;
    const float* d_shift = d_cst + (size_t)M * K;
    StageScope st(ctx, where);
    const float* d_feats = st.in(feats, (size_t)F * D * sizeof(float));
    float* d_ll = st.out(loglik_out, (size_t)M * (size_t)std::max<int64_t>(F, 1) * sizeof(float));
    float* d_sc = st.out(scores_out, (size_t)n_utt * M * sizeof(float));
    int32_t* d_am = st.out(argmax_out, (size_t)n_utt * sizeof(int32_t));
    SSP_TRY(st.status());
    const int64_t* d_off = frame_seg->dev.as<int64_t>();
    const std::vector<int64_t>& ho = frame_seg->host;
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    if (loglik_out) {
        // score_samples: the whole [M x F] matrix in one pass, the per-utterance means from it
        FgEArgs ea{d_feats, d_shift, d_img, d_cst, nullptr, d_ll, nullptr, F, 0, F, D, K, M, g.KS};
        SSP_TRY(fg_launch_e(g, ea, s));
        if (scores_out || argmax_out) {
            hipLaunchKernelGGL(gmm_full_utt_kernel, dim3((unsigned)n_utt), dim3(256), (size_t)M * sizeof(float), s, d_ll, F, d_off, (int64_t)0, M,
                               h->has_ubm, d_sc, d_am);
            SSP_HIP(hipGetLastError());
        }
    } else if (scores_out || argmax_out) {
        // runs of whole utterances whose ll[M][frames] fits the budget: the [M x F] matrix never exists
        const int64_t per = std::max<int64_t>(1, fg_budget_bytes() / ((int64_t)M * (int64_t)sizeof(float)));
        int64_t need = 1;
        for (int64_t u = 0; u < n_utt;) {
            int64_t e = u + 1;
            while (e < n_utt && ho[(size_t)e + 1] - ho[(size_t)u] <= per) ++e;
            need = std::max(need, ho[(size_t)e] - ho[(size_t)u]);
            u = e;
        }
        SSP_TRY(h->ws.reserve((size_t)M * need * sizeof(float)));
        for (int64_t u = 0; u < n_utt;) {
            int64_t e = u + 1;
            while (e < n_utt && ho[(size_t)e + 1] - ho[(size_t)u] <= per) ++e;
            const int64_t f0 = ho[(size_t)u], n = ho[(size_t)e] - f0;
            FgEArgs ea{d_feats + (size_t)f0 * D, d_shift, d_img, d_cst, nullptr, h->ws.as<float>(), nullptr, n, 0, need, D, K, M, g.KS};
            SSP_TRY(fg_launch_e(g, ea, s));
            hipLaunchKernelGGL(gmm_full_utt_kernel, dim3((unsigned)(e - u)), dim3(256), (size_t)M * sizeof(float), s, h->ws.as<float>(), need,
                               d_off + u, f0, M, h->has_ubm, d_sc ? d_sc + (size_t)u * M : nullptr, d_am ? d_am + u : nullptr);
            SSP_HIP(hipGetLastError());
            u = e;
        }
    }
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}
