// EM sufficient statistics of a diagonal-covariance GMM on gfx950 — the O(frames x K x D) part of one iteration of
// sklearn's GaussianMixture.fit as the reference runs it (GMM_UBM.py:158-170: GaussianMixture(n_components, 'diag').fit):
//   E step   log_resp[t,k] = log w_k + log N(x_t; mu_k, diag cov_k) - logsumexp_k(...)      sk:mixture/_base.py:_e_step
//   M sums   nk[k] = sum_t resp[t,k],  sx[k,d] = sum_t resp[t,k] x[t,d],  sxx[k,d] = sum_t resp[t,k] x[t,d]^2
//            (the resp.T @ X and resp.T @ X*X products of _estimate_gaussian_parameters / _estimate_gaussian_covariances_diag)
// The O(K x D) closing arithmetic of the M step (means, covariances + reg_covar, weights, convergence test) stays on the
// host in float64 exactly as sklearn writes it (speech_signal_processing_amd/gmm_train.py).
//
// Kernels per call (D > 47; the MFMA path for D <= 47 is described at gmm_em_acc_mfma_kernel):
//   gmm_em_lse_kernel    workgroup = 64 frames: lp[t,k] for every mixture in 64-mixture chunks staged in LDS, online
//                        log-sum-exp -> lse[t] and one partial of sum_t lse[t] per workgroup
//   gmm_em_acc_kernel    grid (G, K/64): the workgroup keeps ONE 64-mixture chunk of parameters in LDS and walks its frame
//                        tiles; per tile  resp = exp(lp - lse)  (64 x 64, LDS)  then  thread (k, dim group) accumulates
//                        nk / sx / sxx in registers over all its tiles; one fp32 partial per (workgroup, mixture, column)
//   gmm_em_reduce_kernel partials -> float64 sums in a fixed order (bit-reproducible)
// Parameters enter as A = mu P, B = -P/2, c = ln w + 1/2 sum ln P - 1/2 sum mu^2 P - D/2 ln 2pi (float64 on the host, fp32
// on the device): lp = c + sum_d x_d (A_d + x_d B_d).
// Batched form (ssp_gmm_em_stats_batch, D <= 47): M models over row ranges of one feature buffer, one launch group per scratch budget:
//   gmm_em_acc_mfma_seg_kernel  the body of gmm_em_acc_mfma_kernel over a work table of (model, walker) — K <= 64 bit-identical per model
//   gmm_em_lse_mfma_seg_kernel  K > 64: per-frame log-sum-exp over every 64-mixture chunk of a model (MFMA, online max / sum); the single
//                               call's unfused path runs the same body as gmm_em_lse_mfma_kernel
//   gmm_em_reduce_seg_kernel    the body of gmm_em_reduce_kernel per model
#include <cmath>

#include "common.hpp"
#include "gmm_lp_tile.hpp"

namespace ssp {

constexpr int EM_TF = 64;   // frames per tile
constexpr int EM_KC = 64;   // mixtures per chunk
constexpr int EM_DG = 16;   // max dims per accumulation group (4 groups: D <= 64)
constexpr int EM_WS = 65;   // LDS row stride of the lse kernels' k-major parameter chunk (em_lse_mfma_body)

struct EmArgs {
    const float* x;       // [n x D]
    const float* par;     // [Kp][2D+1]  (A[0..D), B[0..D), c), Kp = K rounded up to a multiple of 64, padded c = -1e30
    float* lse;           // [n]
    float* lse_part;      // [ceil(n / 64)]
    float* part;          // [G][Kp][2D+1]
    int64_t n;
    int32_t D, K, Kp, G, n_tiles;
};

// lp of frame `xs` (LDS row, D floats) under mixture row `w` (LDS, 2D+1 floats; wave-uniform address: broadcast reads)
__device__ __forceinline__ float em_lp(const float* __restrict__ xs, const float* __restrict__ w, int D) {
    float acc = w[2 * D];
    for (int d = 0; d < D; ++d) {
        const float xv = xs[d];
        acc = fmaf(xv, fmaf(xv, w[D + d], w[d]), acc);
    }
    return acc;
}

__global__ __launch_bounds__(256) void gmm_em_lse_kernel(EmArgs a) {
    extern __shared__ float sm[];
    const int D = a.D, W = 2 * D + 1, XS = D | 1;  // odd row stride: the 64 frames of a wave read distinct banks
    float* xs = sm;                   // [64][XS]
    float* ws = xs + EM_TF * XS;      // [64][W]
    float* red = ws + EM_KC * W;      // [4][64] x 2
    const int tid = threadIdx.x, t = tid & 63, kg = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t base = (int64_t)blockIdx.x * EM_TF;
    const int nt = (int)min<int64_t>(EM_TF, a.n - base);
    for (int i = tid; i < EM_TF * D; i += 256) {
        const int r = i / D, c = i - r * D;
        xs[r * XS + c] = r < nt ? a.x[(base + r) * D + c] : 0.f;
    }
    float m = -INFINITY, s = 0.f;
    for (int kc = 0; kc < a.Kp; kc += EM_KC) {
        __syncthreads();
        for (int i = tid; i < EM_KC * W; i += 256) ws[i] = a.par[(size_t)kc * W + i];
        __syncthreads();
        for (int kk = 0; kk < 16; ++kk) {
            const float lp = em_lp(xs + t * XS, ws + (kg * 16 + kk) * W, D);
            const float mn = fmaxf(m, lp);
            s = s * __expf(m - mn) + __expf(lp - mn);
            m = mn;
        }
    }
    red[kg * 64 + t] = m;
    red[256 + kg * 64 + t] = s;
    __syncthreads();
    if (tid < 64) {
        float mm = red[t], ss = red[256 + t];
        for (int g = 1; g < 4; ++g) {
            const float m2 = red[g * 64 + t], s2 = red[256 + g * 64 + t];
            const float mn = fmaxf(mm, m2);
            ss = ss * __expf(mm - mn) + s2 * __expf(m2 - mn);
            mm = mn;
        }
        float l = t < nt ? mm + __logf(ss) : 0.f;
        if (t < nt) a.lse[base + t] = l;
        for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o);
        if (t == 0) a.lse_part[blockIdx.x] = l;
    }
}

__global__ __launch_bounds__(256) void gmm_em_acc_kernel(EmArgs a) {
    extern __shared__ float sm[];
    const int D = a.D, W = 2 * D + 1, XS = D | 1;
    float* xs = sm;                   // [64][XS]
    float* ws = xs + EM_TF * XS;      // [64][W]    this workgroup's chunk of mixtures, loaded once
    float* rs = ws + EM_KC * W;       // [64 frames][65]  responsibilities of the tile
    const int tid = threadIdx.x, t = tid & 63, kg = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kc = blockIdx.y * EM_KC;
    for (int i = tid; i < EM_KC * W; i += 256) ws[i] = a.par[(size_t)kc * W + i];
    // accumulation role: mixture k = tid & 63 of the chunk, dims [dg * dper, dg * dper + dper)
    const int dper = (D + 3) / 4, d0 = kg * dper;
    float ax[EM_DG], axx[EM_DG], an = 0.f;
#pragma unroll
    for (int i = 0; i < EM_DG; ++i) ax[i] = axx[i] = 0.f;
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += a.G) {
        const int64_t base = (int64_t)tile * EM_TF;
        const int nt = (int)min<int64_t>(EM_TF, a.n - base);
        __syncthreads();
        for (int i = tid; i < EM_TF * D; i += 256) {
            const int r = i / D, c = i - r * D;
            xs[r * XS + c] = r < nt ? a.x[(base + r) * D + c] : 0.f;
        }
        __syncthreads();
        const float l = t < nt ? a.lse[base + t] : INFINITY;  // frames beyond the end get resp = exp(-inf) = 0
        for (int kk = 0; kk < 16; ++kk) {
            const int k = kg * 16 + kk;
            rs[t * 65 + k] = __expf(em_lp(xs + t * XS, ws + k * W, D) - l);
        }
        __syncthreads();
        for (int r = 0; r < EM_TF; ++r) {
            const float rv = rs[r * 65 + t];  // mixture t of the chunk, frame r
            if (kg == 0) an += rv;
            const float* xr = xs + r * XS + d0;  // wave-uniform: broadcast
#pragma unroll
            for (int i = 0; i < EM_DG; ++i)
                if (i < dper && d0 + i < D) {
                    const float xv = xr[i], rx = rv * xv;
                    ax[i] += rx;
                    axx[i] = fmaf(rx, xv, axx[i]);
                }
        }
    }
    float* out = a.part + ((size_t)blockIdx.x * a.Kp + kc + t) * W;
#pragma unroll
    for (int i = 0; i < EM_DG; ++i)
        if (i < dper && d0 + i < D) {
            out[d0 + i] = ax[i];
            out[D + d0 + i] = axx[i];
        }
    if (kg == 0) out[2 * D] = an;
}


// MFMA form of gmm_em_acc_kernel (D <= 47: at most 3 column tiles of [x, x^2, 1]).  Grid (G, K/64), 4 waves; per 64-frame tile
//   GEMM1  lp[64 mix x 64 frames] = W[64 x (2D+1)] . aug^T        wave (r, c) owns one 32 x 32 tile; mixtures = MFMA rows, frames =
//                                                                  columns, so a lane's 16 accumulators belong to ONE frame
//   resp   = exp(lp - lse[frame])  -> LDS tile rs[frame][mix]
//   GEMM2  S[64 mix x (2D+1)] += resp[64 mix x 64 frames] . aug    split over the waves by frames (wave w: frames 16w..16w+15 of
//                                                                  the tile); accumulators stay in registers over all tiles
// Each wave leaves its own partial [64 mix][2D+1]; gmm_em_reduce_kernel adds the 4 G partials in float64.
// FUSE (K <= 64: the workgroup sees every mixture of a frame): the per-frame log-sum-exp is taken right here from the GEMM1
// accumulators (in-lane over 16 mixtures, across the two half-waves, across the two waves that share a frame through LDS) instead of a
// separate scoring pass; sum_t lse[t] leaves as one partial per workgroup.
// The body of gmm_em_acc_mfma_kernel, shared with its batched form gmm_em_acc_mfma_seg_kernel so that a model's frames meet the same
// instructions in both (the batched path is bit-identical to the single-model call): `a` describes ONE model's frames, parameters and
// partials, `wg` is this workgroup's walker index among a.G (tiles wg, wg + a.G, ...).  SEG: the staging loops run with wave-uniform
// trip counts (the batched kernels keep no loop over lane masks; the single-model kernel keeps its instructions as they were).
template <int NCT, bool FUSE, bool SEG>
__device__ __forceinline__ void em_mfma_body(const EmArgs& a, unsigned wg) {
    extern __shared__ float sm[];
    const int D = a.D, W = 2 * D + 1, KS = (W + 1) / 2;  // KS k-steps of 2 over [x, x^2, 1] (+ a zero pad column)
    const int XS = (2 * KS) | 1;       // odd row stride of the augmented frame tile
    float* xs = sm;                    // [64 frames][XS]  aug = [x, x^2, 1, 0]: the B operand of both GEMMs, read as it stands (forming
                                       // x^2 / the constants per MFMA put branches and a dependent LDS read into the inner loops)
    float* wsT = xs + EM_TF * XS;      // [2 KS][64 mix]   parameter chunk, k-major: the A operand of GEMM1
    float* rs = wsT + 2 * KS * EM_KC;  // [64 frames][65]  responsibilities: the A operand of GEMM2
    float* ex = rs + EM_TF * 65;       // [2 mixture halves][64 frames][2]  (max, sum) exchange of the fused log-sum-exp
    float lsum = 0.f;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fl = lane & 31, h = lane >> 5;
    const int kc = blockIdx.y * EM_KC;
    if constexpr (SEG) {
        for (int i0 = 0; i0 < 2 * KS * EM_KC; i0 += 256) {
            const int i = i0 + tid;
            if (i < 2 * KS * EM_KC) {
                const int k = i / EM_KC, m = i - k * EM_KC;
                wsT[i] = k < W ? a.par[(size_t)(kc + m) * W + k] : 0.f;
            }
        }
        for (int i0 = 0; i0 < EM_TF * (2 * KS - 2 * D); i0 += 256) {
            const int i = i0 + tid;
            if (i < EM_TF * (2 * KS - 2 * D)) {
                const int r = i / (2 * KS - 2 * D), c = i - r * (2 * KS - 2 * D);
                xs[r * XS + 2 * D + c] = c == 0 ? 1.f : 0.f;
            }
        }
    } else {
        for (int i = tid; i < 2 * KS * EM_KC; i += 256) {
            const int k = i / EM_KC, m = i - k * EM_KC;
            wsT[i] = k < W ? a.par[(size_t)(kc + m) * W + k] : 0.f;
        }
        for (int i = tid; i < EM_TF * (2 * KS - 2 * D); i += 256) {  // the constant columns [1, 0...] of every row, written once
            const int r = i / (2 * KS - 2 * D), c = i - r * (2 * KS - 2 * D);
            xs[r * XS + 2 * D + c] = c == 0 ? 1.f : 0.f;
        }
    }
    const int r1 = wave >> 1, c1 = wave & 1;  // GEMM1 tile of this wave
    f32x16 acc2[2][NCT];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < NCT; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc2[r][c][i] = 0.f;
    // the frame tile of the NEXT iteration is fetched into registers while this one's MFMAs run (a synchronous load would expose a
    // full memory latency per 64-frame tile): EM_XP floats per thread cover 64 x D <= 64 x 47
    constexpr int EM_XP = 12;
    float xpre[EM_XP];
    float lpre = INFINITY;
    auto fetch = [&](int tile) {
        const int64_t base = (int64_t)tile * EM_TF;
        const int nt = tile < a.n_tiles ? (int)min<int64_t>(EM_TF, a.n - base) : 0;
#pragma unroll
        for (int u = 0; u < EM_XP; ++u) {
            const int i = tid + u * 256;
            const int r = i / D;
            xpre[u] = (i < EM_TF * D && r < nt) ? a.x[base * D + i] : 0.f;
        }
        const int fr = 32 * c1 + fl;
        if (FUSE) lpre = fr < nt ? 0.f : INFINITY;
        else lpre = fr < nt ? a.lse[base + fr] : INFINITY;  // frames beyond the end: resp = exp(-inf) = 0
    };
    fetch(wg);
    for (int tile = wg; tile < a.n_tiles; tile += a.G) {
        __syncthreads();  // the previous tile's GEMM2 is done with xs / rs
#pragma unroll
        for (int u = 0; u < EM_XP; ++u) {
            const int i = tid + u * 256;
            if (i < EM_TF * D) {
                const int r = i / D, c = i - r * D;
                const float v = xpre[u];
                xs[r * XS + c] = v;
                xs[r * XS + D + c] = v * v;
            }
        }
        const float l = lpre;
        fetch(tile + a.G);
        __syncthreads();
        // ---- GEMM1: A[row = mix 32 r1 + fl][k = 2 s + h], B[k = 2 s + h][col = frame 32 c1 + fl] = aug[frame][k]
        const f32x16 acc1 = em_lp_tile<EM_KC>(xs + (32 * c1 + fl) * XS, wsT + h * EM_KC + 32 * r1 + fl, KS, h);
        // ---- responsibilities of this lane's frame; accumulator i = mixture 32 r1 + em_lp_mix(i, h)
        const int fr = 32 * c1 + fl;
        if (FUSE) {
            float m = acc1[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) m = fmaxf(m, acc1[i]);
            m = fmaxf(m, __shfl_xor(m, 32));
            float e[16], ssum = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                e[i] = __expf(acc1[i] - m);
                ssum += e[i];
            }
            ssum += __shfl_xor(ssum, 32);
            if (h == 0) *reinterpret_cast<float2*>(ex + (r1 * 64 + fr) * 2) = make_float2(m, ssum);
            __syncthreads();
            const float2 o = *reinterpret_cast<const float2*>(ex + ((1 - r1) * 64 + fr) * 2);
            const float mm = fmaxf(m, o.x);
            const float tot = ssum * __expf(m - mm) + o.y * __expf(o.x - mm);
            const bool valid = l == 0.f;
            const float scale = valid ? __expf(m - mm) / tot : 0.f;
            if (valid && r1 == 0 && h == 0) lsum += mm + __logf(tot);
#pragma unroll
            for (int i = 0; i < 16; ++i) rs[fr * 65 + 32 * r1 + em_lp_mix(i, h)] = e[i] * scale;
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) rs[fr * 65 + 32 * r1 + em_lp_mix(i, h)] = __expf(acc1[i] - l);
        }
        __syncthreads();
        // ---- GEMM2 over this wave's 16 frames: A[row = mix 32 r + fl][k = frame], B[k = frame][col = 32 c + fl] = aug[frame][col]
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
            const int f2 = 16 * wave + 2 * s2 + h;
            float av[2], bv[NCT];
#pragma unroll
            for (int r = 0; r < 2; ++r) av[r] = rs[f2 * 65 + 32 * r + fl];
            const float* xr = xs + f2 * XS;
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                const int col = 32 * c + fl;
                bv[c] = col < 2 * KS ? xr[col] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < NCT; ++c) acc2[r][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[r], bv[c], acc2[r][c], 0, 0, 0);
        }
    }
    if (FUSE) {  // sum of this workgroup's lse values: lanes (r1 == 0, h == 0) of waves 0 and 1 hold them
        for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o);
        __syncthreads();
        if (lane == 0 && r1 == 0) ex[c1] = lsum;
        __syncthreads();
        if (tid == 0) a.lse_part[wg] = ex[0] + ex[1];
    }
    float* out = a.part + ((size_t)(wg * 4 + wave) * a.Kp + kc) * W;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
            const int col = 32 * c + fl;
            if (col < W)
#pragma unroll
                for (int i = 0; i < 16; ++i) out[(size_t)(32 * r + (i & 3) + 8 * (i >> 2) + 4 * h) * W + col] = acc2[r][c][i];
        }
}

template <int NCT, bool FUSE>
__global__ __launch_bounds__(256) void gmm_em_acc_mfma_kernel(EmArgs a) {
    em_mfma_body<NCT, FUSE, false>(a, blockIdx.x);
}

// out[j] = sum_g part[g][j] (float64, fixed order): block = 32 columns x 8 slices of the partial index (coalesced 128-byte
// reads), the 8 slice sums are added in slice order;  block 0 also reduces the lse partials
__device__ __forceinline__ void em_reduce_body(const float* part, int G, int64_t cols, const float* lse_part, int64_t n_lse, double* out,
                                               unsigned bx) {
    __shared__ double sh[256];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t j = (int64_t)bx * 32 + tx;
    double s = 0.0;
    if (j < cols)
        for (int g = ty; g < G; g += 8) s += (double)part[(size_t)g * cols + j];
    sh[ty * 32 + tx] = s;
    __syncthreads();
    if (ty == 0 && j < cols) {
        double t = 0.0;
        for (int k = 0; k < 8; ++k) t += sh[k * 32 + tx];
        out[j] = t;
    }
    if (bx == 0) {  // sum_t lse[t]: fixed strided order + tree
        __syncthreads();
        double v = 0.0;
        for (int64_t i = threadIdx.x; i < n_lse; i += 256) v += (double)lse_part[i];
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[cols] = sh[0];
    }
}

__global__ __launch_bounds__(256) void gmm_em_reduce_kernel(const float* part, int G, int64_t cols, const float* lse_part, int64_t n_lse,
                                                            double* out) {
    em_reduce_body(part, G, cols, lse_part, n_lse, out, blockIdx.x);
}

// ---- batched form (ssp_gmm_em_stats_batch): M models, each scored over its own row range of one feature buffer
// one model of a batched call: where its frames, parameters and partials live
struct EmModel {
    int64_t x_off;     // first feature row of its range
    int64_t n;         // frames
    int64_t lse_off;   // its per-frame lse values in the call's lse buffer (K > 64)
    int64_t part_off;  // its [4 G][Kp][2D+1] wave partials in the launch group's partial buffer (floats)
    int64_t lsep_off;  // its lse partials: G of them (K <= 64, fused), n_tiles otherwise
    int32_t n_tiles, G;
};

struct EmBatchArgs {
    const float* x;         // [n_rows x D]
    const float* par;       // [M][Kp][2D+1]  (shared form: ONE block [Kp][2D+1], par_stride 0)
    float* lse;             // [sum of n]  (K > 64)
    float* lse_part;        // [sum of the models' lse partials]
    float* part;            // the launch group's wave partials
    const EmModel* models;  // [M]
    const int2* work;       // per workgroup: (model, walker g) for the accumulation kernel, (model, tile) for the lse kernel
    int32_t D, K, Kp;
    int64_t par_stride;     // floats between two models' parameter blocks: Kp (2D+1), or 0 when every model reads the same block
};

// model m of a batched call as the EmArgs of a single-model call; every value wave-uniform (read through readfirstlane: a persistent
// walk whose bounds the compiler cannot prove uniform may be rebuilt as a loop over lane masks — tests/test_isa_guards.py)
__device__ __forceinline__ EmArgs em_seg_args(const EmBatchArgs& b, int m) {
    const EmModel& md = b.models[m];
    EmArgs a;
    const int D = b.D;
    a.x = b.x + em_uniform64(md.x_off) * D;
    a.par = b.par + (size_t)m * b.par_stride;
    a.lse = b.lse + em_uniform64(md.lse_off);
    a.lse_part = b.lse_part + em_uniform64(md.lsep_off);
    a.part = b.part + em_uniform64(md.part_off);
    a.n = em_uniform64(md.n);
    a.D = D;
    a.K = b.K;
    a.Kp = b.Kp;
    a.G = em_uniform(md.G);
    a.n_tiles = em_uniform(md.n_tiles);
    return a;
}

// gmm_em_acc_mfma_kernel over a work table: workgroup (x, y) = walker g of model m (work[x]), mixture chunk y.  What it reads and
// writes for its model is exactly what the single-model kernel does for walker g of a call on that model's rows.
template <int NCT, bool FUSE>
__global__ __launch_bounds__(256) void gmm_em_acc_mfma_seg_kernel(EmBatchArgs b) {
    const int2 w = b.work[blockIdx.x];
    const int m = em_uniform(w.x), g = em_uniform(w.y);
    em_mfma_body<NCT, FUSE, true>(em_seg_args(b, m), (unsigned)g);
}

// per-frame log-sum-exp of the unfused MFMA path (several 64-mixture chunks, or SSP_EM_NO_FUSE): workgroup = one 64-frame tile of one
// model.  Per chunk: em_mfma_body's GEMM1 (wave (r1, c1): mixtures 32 r1.., frames 32 c1..), the same em_lp_tile (gmm_lp_tile.hpp) over
// the same parameter values, so that lp - lse in the accumulation kernel is the difference of two evaluations of one formula; then an online
// (max, sum) per frame over the chunks; the two mixture halves meet in LDS.  Writes lse[t] of the tile's frames and one lse partial per
// tile.  The body is shared by the single-model kernel (tile = blockIdx.x) and the batched one (work[x] = (model, tile)).
__device__ __forceinline__ void em_lse_mfma_body(const EmArgs& a, int tile) {
    extern __shared__ float sm[];
    const int D = a.D, W = 2 * D + 1, KS = (W + 1) / 2;
    const int XS = (2 * KS) | 1;
    float* xs = sm;                    // [64 frames][XS]  aug = [x, x^2, 1, 0]
    float* wsT = xs + EM_TF * XS;      // [2 KS][EM_WS]    parameter chunk, k-major, row stride 65: the chunk is read from global memory as
                                       // it lies (mixture-major, consecutive lanes consecutive addresses) and transposed on the way in
                                       // — lane to lane the LDS address moves by 65 floats (or by 1), never onto the same bank.  Read
                                       // k-major from global memory, every lane touched a cache line of its own: 64 lines per load.
    float* ex = wsT + 2 * KS * EM_WS;  // [2 mixture halves][64 frames][2]  (max, sum) exchange, then 4 wave sums
    const int tid = threadIdx.x, lane = tid & 63, wave = em_uniform(tid >> 6);
    const int fl = lane & 31, h = lane >> 5, r1 = wave >> 1, c1 = wave & 1;
    const int64_t base = (int64_t)tile * EM_TF;
    const int nt = (int)min<int64_t>(EM_TF, a.n - base);
    em_stage_aug(xs, a.x, base, nt, D, KS, XS);
    const float* xrow = xs + (32 * c1 + fl) * XS;
    const float* wcol = wsT + h * EM_WS + 32 * r1 + fl;
    if (tid < EM_KC) wsT[W * EM_WS + tid] = 0.f;  // the zero pad row k = 2 D + 1 of the last k-step: written once, no chunk touches it
    // element i = tid + 256 j of a chunk [64 mix][W] is (mixture i / W, column i % W): stepped, not divided
    const int i_q = 256 / W, i_r = 256 - i_q * W, m_first = tid / W, k_first = tid - m_first * W;
    // the parameter chunk of the NEXT iteration is fetched into registers while this one's MFMAs run, as em_mfma_body fetches its frame
    // tiles: EM_WP floats per thread cover 64 x (2 D + 1) <= 64 x 95
    constexpr int EM_WP = 24;
    float wpre[EM_WP];
    auto fetchw = [&](int kc) {
        const float* pc = a.par + (size_t)kc * W;
#pragma unroll
        for (int u = 0; u < EM_WP; ++u) {
            const int i = tid + u * 256;
            wpre[u] = (kc < a.Kp && i < EM_KC * W) ? pc[i] : 0.f;
        }
    };
    fetchw(0);
    float m = -INFINITY, s = 0.f;  // this lane's frame over the mixtures of half r1 seen so far
    for (int kc = 0; kc < a.Kp; kc += EM_KC) {
        __syncthreads();  // the previous chunk's GEMM1 is done with wsT
        int pm = m_first, pk = k_first;
#pragma unroll
        for (int u = 0; u < EM_WP; ++u) {
            if (tid + u * 256 < EM_KC * W) wsT[pk * EM_WS + pm] = wpre[u];
            pm += i_q;
            pk += i_r;
            if (pk >= W) {
                pk -= W;
                ++pm;
            }
        }
        fetchw(kc + EM_KC);  // the next chunk travels while this one's MFMAs run
        __syncthreads();
        const f32x16 acc1 = em_lp_tile<EM_WS>(xrow, wcol, KS, h);
        float cm = acc1[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) cm = fmaxf(cm, acc1[i]);
        cm = fmaxf(cm, __shfl_xor(cm, 32));
        float cs = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) cs += __expf(acc1[i] - cm);
        cs += __shfl_xor(cs, 32);
        const float mn = fmaxf(m, cm);  // (padded mixtures: c = -1e30, finite; the first chunk makes m finite)
        s = s * __expf(m - mn) + cs * __expf(cm - mn);
        m = mn;
    }
    const int fr = 32 * c1 + fl;
    if (h == 0) *reinterpret_cast<float2*>(ex + (r1 * 64 + fr) * 2) = make_float2(m, s);
    __syncthreads();
    const float2 o = *reinterpret_cast<const float2*>(ex + ((1 - r1) * 64 + fr) * 2);
    const float mm = fmaxf(m, o.x);
    const float l = mm + __logf(s * __expf(m - mm) + o.y * __expf(o.x - mm));
    const bool mine = r1 == 0 && h == 0 && fr < nt;  // waves 0 and 1 own frames 0..31 and 32..63
    if (mine) a.lse[base + fr] = l;
    float v = mine ? l : 0.f;
    for (int o2 = 32; o2 > 0; o2 >>= 1) v += __shfl_xor(v, o2);
    __syncthreads();  // every wave has read the exchange
    if (lane == 0) ex[wave] = v;
    __syncthreads();
    if (tid == 0) a.lse_part[tile] = ex[0] + ex[1];
}

__global__ __launch_bounds__(256) void gmm_em_lse_mfma_kernel(EmArgs a) { em_lse_mfma_body(a, (int)blockIdx.x); }

__global__ __launch_bounds__(256) void gmm_em_lse_mfma_seg_kernel(EmBatchArgs b) {
    const int2 w = b.work[blockIdx.x];
    const int mi = em_uniform(w.x), tile = em_uniform(w.y);
    em_lse_mfma_body(em_seg_args(b, mi), tile);
}

// gmm_em_reduce_kernel per model: grid (column blocks, models of the launch group from m0); out[m][cols + 1]
__global__ __launch_bounds__(256) void gmm_em_reduce_seg_kernel(EmBatchArgs b, int m0, int64_t cols, int fused, double* out) {
    const int m = m0 + blockIdx.y;
    const EmModel& md = b.models[m];
    em_reduce_body(b.part + md.part_off, 4 * md.G, cols, b.lse_part + md.lsep_off, fused ? (int64_t)md.G : (int64_t)md.n_tiles,
                   out + (size_t)m * (cols + 1), blockIdx.x);
}

}  // namespace ssp

using namespace ssp;

// float64 parameters of one model -> the fp32 rows [Kp][2D+1] the EM kernels read (A = mu P, B = -P/2, c; padded rows c = -1e30).
// par must be zeroed.  model >= 0: a batched call's model index, named in the messages.
static int em_pack(int K, int D, int Kp, const double* weights, const double* means, const double* covars, float* par, int model,
                   const char* fn = "ssp_gmm_em_stats_batch") {
    const int W = 2 * D + 1;
    const double ln2pi = std::log(2.0 * M_PI);
    for (int k = 0; k < Kp; ++k) {
        float* w = par + (size_t)k * W;
        if (k >= K) {
            w[2 * D] = -1.0e30f;  // padded mixture: resp = exp(-1e30 - lse) = 0
            continue;
        }
        if (!(weights[k] > 0.0)) {
            if (model < 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_em_stats: non-positive weight (mix %d)", k);
            SSP_FAIL(SSP_ERR_INVALID, "%s: non-positive weight (model %d, mix %d)", fn, model, k);
        }
        double c = std::log(weights[k]) - 0.5 * D * ln2pi;
        for (int d = 0; d < D; ++d) {
            const double cv = covars[(size_t)k * D + d], mu = means[(size_t)k * D + d];
            if (!(cv > 0.0)) {
                if (model < 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_em_stats: non-positive covariance (mix %d)", k);
                SSP_FAIL(SSP_ERR_INVALID, "%s: non-positive covariance (model %d, mix %d)", fn, model, k);
            }
            const double P = 1.0 / cv;
            w[d] = (float)(mu * P);
            w[D + d] = (float)(-0.5 * P);
            c += 0.5 * std::log(P) - 0.5 * mu * mu * P;
        }
        w[2 * D] = (float)c;
    }
    return SSP_OK;
}

extern "C" int ssp_gmm_em_stats(ssp_ctx* ctx, int32_t K, int32_t D, const double* weights, const double* means,
                                const double* covars, const float* feats, int64_t n_frames, double* nk_out, double* sx_out,
                                double* sxx_out, double* loglik_sum_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_gmm_em_stats");
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (K < 1 || D < 1 || !weights || !means || !covars || !nk_out || !sx_out || !sxx_out || !loglik_sum_out)
        SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_em_stats: bad shape or null array");
    if (D > 4 * EM_DG) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_gmm_em_stats: D=%d exceeds the supported feature dimension (%d)", D, 4 * EM_DG);
    if (n_frames < 1 || !feats) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_em_stats: no frames");
    SSP_TRY(check_where(where, "ssp_gmm_em_stats"));
    const int W = 2 * D + 1, Kp = (K + EM_KC - 1) / EM_KC * EM_KC;
    std::vector<float> par((size_t)Kp * W, 0.f);
    SSP_TRY(em_pack(K, D, Kp, weights, means, covars, par.data(), -1));
    hipStream_t s = ctx->stream;
    const int64_t n_tiles = (n_frames + EM_TF - 1) / EM_TF;
    if (n_tiles > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_gmm_em_stats: too many frames");
    const int G = (int)std::min<int64_t>(n_tiles, 2 * (int64_t)ctx->num_cu);
    const int64_t cols = (int64_t)Kp * W;
    const int nct = (W + 31) / 32;
    const bool mfma = nct <= 3 && !getenv("SSP_EM_NO_MFMA");  // D <= 47: both GEMM-shaped products on the matrix cores
    const int GP = mfma ? 4 * G : G;                           // partials: one per wave on the MFMA path
    // device scratch lives in the ctx (grow-only): an EM loop calls this once per iteration
    DevBuf &d_par = ctx->scratch[0], &d_lse = ctx->scratch[1], &d_lsep = ctx->scratch[2], &d_part = ctx->scratch[3],
           &d_out = ctx->scratch[4];
    StageScope st(ctx, where);
    const float* d_x = st.in(feats, (size_t)n_frames * D * sizeof(float));
    SSP_TRY(st.status());
    SSP_TRY(d_par.reserve(par.size() * sizeof(float)));
    SSP_TRY(d_lse.reserve((size_t)n_frames * sizeof(float)));
    SSP_TRY(d_lsep.reserve((size_t)std::max<int64_t>(n_tiles, G) * sizeof(float)));
    SSP_TRY(d_part.reserve((size_t)GP * cols * sizeof(float)));
    SSP_TRY(d_out.reserve((size_t)(cols + 1) * sizeof(double)));
    SSP_HIP(hipMemcpyAsync(d_par.p, par.data(), par.size() * sizeof(float), hipMemcpyHostToDevice, s));
    SSP_HIP(hipMemsetAsync(d_part.p, 0, (size_t)GP * cols * sizeof(float), s));
    EmArgs a{d_x, d_par.as<float>(), d_lse.as<float>(), d_lsep.as<float>(), d_part.as<float>(), n_frames, D, K, Kp, G, (int32_t)n_tiles};
    const int XS = D | 1;
    const size_t lds1 = ((size_t)EM_TF * XS + (size_t)EM_KC * W + 512) * sizeof(float);
    const size_t lds2 = ((size_t)EM_TF * XS + (size_t)EM_KC * W + (size_t)EM_TF * 65) * sizeof(float);
    const size_t lds3 = ((size_t)EM_TF * ((W + 1) | 1) + (size_t)(W + 1) * EM_KC + (size_t)EM_TF * 65 + 256) * sizeof(float);
    const size_t lds4 = ((size_t)EM_TF * ((W + 1) | 1) + (size_t)(W + 1) * EM_WS + 256) * sizeof(float);
    const bool fuse = mfma && Kp == EM_KC && !getenv("SSP_EM_NO_FUSE");  // K <= 64: log-sum-exp inside the accumulation kernel
    if (lds1 > 64 * 1024)
        SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gmm_em_lse_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1));
    if (lds2 > 64 * 1024)
        SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gmm_em_acc_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
    if (mfma && lds3 > 64 * 1024) {
        const void* ks[6] = {reinterpret_cast<const void*>(gmm_em_acc_mfma_kernel<1, true>), reinterpret_cast<const void*>(gmm_em_acc_mfma_kernel<2, true>),
                             reinterpret_cast<const void*>(gmm_em_acc_mfma_kernel<3, true>), reinterpret_cast<const void*>(gmm_em_acc_mfma_kernel<1, false>),
                             reinterpret_cast<const void*>(gmm_em_acc_mfma_kernel<2, false>), reinterpret_cast<const void*>(gmm_em_acc_mfma_kernel<3, false>)};
        for (const void* k : ks) SSP_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3));
    }
    // the per-frame log-sum-exp of the unfused MFMA path comes from gmm_em_lse_mfma_kernel: the image, formula and k order of the
    // accumulation kernel's own GEMM1 (it once came from the scorer of csrc/gmm.hip, whose log2 image rounds differently: resp =
    // exp(lp - lse) then carried the DIFFERENCE of two roundings of an exponent of size |lp| — 1 % of a frame's mass at |lp| = 5e4)
    if (mfma && !fuse && lds4 > 64 * 1024)
        SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gmm_em_lse_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds4));
    Timer tm;
    int rc = tm.start(kernel_ms != nullptr, s);
    if (rc == SSP_OK && fuse) {
        switch (nct) {
            case 1: hipLaunchKernelGGL((gmm_em_acc_mfma_kernel<1, true>), dim3(G, 1), dim3(256), lds3, s, a); break;
            case 2: hipLaunchKernelGGL((gmm_em_acc_mfma_kernel<2, true>), dim3(G, 1), dim3(256), lds3, s, a); break;
            default: hipLaunchKernelGGL((gmm_em_acc_mfma_kernel<3, true>), dim3(G, 1), dim3(256), lds3, s, a); break;
        }
    } else if (rc == SSP_OK && mfma) {
        hipLaunchKernelGGL(gmm_em_lse_mfma_kernel, dim3((unsigned)n_tiles), dim3(256), lds4, s, a);
        switch (nct) {
            case 1: hipLaunchKernelGGL((gmm_em_acc_mfma_kernel<1, false>), dim3(G, Kp / EM_KC), dim3(256), lds3, s, a); break;
            case 2: hipLaunchKernelGGL((gmm_em_acc_mfma_kernel<2, false>), dim3(G, Kp / EM_KC), dim3(256), lds3, s, a); break;
            default: hipLaunchKernelGGL((gmm_em_acc_mfma_kernel<3, false>), dim3(G, Kp / EM_KC), dim3(256), lds3, s, a); break;
        }
    } else if (rc == SSP_OK) {
        hipLaunchKernelGGL(gmm_em_lse_kernel, dim3((unsigned)n_tiles), dim3(256), lds1, s, a);
        hipLaunchKernelGGL(gmm_em_acc_kernel, dim3(G, Kp / EM_KC), dim3(256), lds2, s, a);
    }
    if (rc == SSP_OK) {
        hipLaunchKernelGGL(gmm_em_reduce_kernel, dim3((unsigned)((cols + 31) / 32)), dim3(256), 0, s, d_part.as<float>(), GP, cols,
                           d_lsep.as<float>(), fuse ? (int64_t)G : n_tiles, d_out.as<double>());
        if (hipGetLastError() != hipSuccess) {
            set_error("ssp_gmm_em_stats: kernel launch failed");
            rc = SSP_ERR_HIP;
        }
    }
    if (rc == SSP_OK) rc = tm.stop(s, kernel_ms);
    if (rc != SSP_OK) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    std::vector<double> host((size_t)cols + 1);
    hipError_t he = hipMemcpyAsync(host.data(), d_out.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) SSP_FAIL(SSP_ERR_HIP, "ssp_gmm_em_stats: result copy failed: %s", hipGetErrorString(he));
    for (int k = 0; k < K; ++k) {
        const double* r = host.data() + (size_t)k * W;
        for (int d = 0; d < D; ++d) {
            sx_out[(size_t)k * D + d] = r[d];
            sxx_out[(size_t)k * D + d] = r[D + d];
        }
        nk_out[k] = r[2 * D];
    }
    *loglik_sum_out = host[(size_t)cols];
    return SSP_OK;
}

// ssp_gmm_em_stats_batch and (shared) ssp_gmm_em_stats_shared: the second packs and uploads ONE parameter block that every model reads
// (parameter stride 0); partition, kernels, launch groups and reduction are the same code, so its outputs are the bits of the first
// called with the block repeated M times.  fn: the entry point's name for the messages.
static int em_stats_batch_impl(ssp_ctx* ctx, int32_t M, int32_t K, int32_t D, const double* weights, const double* means,
                               const double* covars, const float* feats, int64_t n_rows, const int64_t* row_off, const int64_t* n_frames,
                               double* nk_out, double* sx_out, double* sxx_out, double* loglik_sum_out, int where, float* kernel_ms,
                               bool shared, const char* fn) {
    ssp::TraceRange trace_(fn);
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (M < 1 || K < 1 || D < 1 || !weights || !means || !covars || !row_off || !n_frames || !nk_out || !sx_out || !sxx_out ||
        !loglik_sum_out)
        SSP_FAIL(SSP_ERR_INVALID, "%s: bad shape or null array", fn);
    const int W = 2 * D + 1, nct = (W + 31) / 32;
    if (nct > 3) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: D=%d exceeds the batched path's feature dimension (47)", fn, D);
    if (n_rows < 1 || !feats) SSP_FAIL(SSP_ERR_INVALID, "%s: no frames", fn);
    SSP_TRY(check_where(where, fn));
    for (int m = 0; m < M; ++m) {
        if (n_frames[m] < 1) SSP_FAIL(SSP_ERR_INVALID, "%s: model %d has no frames", fn, m);
        if (row_off[m] < 0 || row_off[m] > n_rows - n_frames[m])
            SSP_FAIL(SSP_ERR_INVALID, "%s: model %d: rows [%lld, %lld) outside the %lld feature rows", fn, m,
                     (long long)row_off[m], (long long)(row_off[m] + n_frames[m]), (long long)n_rows);
    }
    const int Kp = (K + EM_KC - 1) / EM_KC * EM_KC, chunks = Kp / EM_KC;
    const bool fuse = chunks == 1;  // K <= 64: the fused kernel, bit-identical to ssp_gmm_em_stats per model
    const int64_t cols = (int64_t)Kp * W;
    const int n_par = shared ? 1 : M;  // parameter blocks packed and uploaded
    std::vector<float> par((size_t)n_par * Kp * W, 0.f);
    for (int m = 0; m < n_par; ++m)
        SSP_TRY(em_pack(K, D, Kp, weights + (size_t)m * K, means + (size_t)m * K * D, covars + (size_t)m * K * D, par.data() + (size_t)m * Kp * W, m, fn));
    // partition: K <= 64 as the single call (G = min(tiles, 2 CUs' worth)); K > 64: G capped so that G x chunks <= 2 x num_cu
    // workgroups per model (bounded partials: 4 G Kp (2D+1) floats)
    const int64_t gcap = fuse ? 2 * (int64_t)ctx->num_cu : std::max<int64_t>(1, 2 * (int64_t)ctx->num_cu / chunks);
    // launch groups: consecutive models whose partials fit the scratch budget (SSP_EM_BATCH_SCRATCH_MB, default 1024); the partial
    // buffer is reused group after group on the ctx stream
    int64_t budget = (int64_t)1 << 30;
    if (const char* e = getenv("SSP_EM_BATCH_SCRATCH_MB")) budget = std::max<int64_t>(1, atoll(e)) << 20;
    const int64_t budget_f = budget / (int64_t)sizeof(float);
    std::vector<EmModel> md(M);
    std::vector<int> gstart;                         // first model of every launch group (+ M)
    std::vector<int64_t> wstart;                     // first work item of every group (+ total)
    std::vector<int2> work, tiles;
    int64_t lse_tot = 0, lsep_tot = 0, cur = 0, part_max = 0;
    for (int m = 0; m < M; ++m) {
        const int64_t nt = (n_frames[m] + EM_TF - 1) / EM_TF;
        if (nt > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: too many frames (model %d)", fn, m);
        const int G = (int)std::min<int64_t>(nt, gcap);
        const int64_t pf = 4 * (int64_t)G * cols;
        if (m == 0 || (cur > 0 && cur + pf > budget_f) || m - gstart.back() >= 65535) {
            gstart.push_back(m);
            wstart.push_back((int64_t)work.size());
            cur = 0;
        }
        md[m] = EmModel{row_off[m], n_frames[m], lse_tot, cur, lsep_tot, (int32_t)nt, G};
        cur += pf;
        part_max = std::max(part_max, cur);
        if (!fuse) lse_tot += n_frames[m];
        lsep_tot += fuse ? G : nt;
        for (int g = 0; g < G; ++g) work.push_back(make_int2(m, g));
        if (!fuse)
            for (int64_t t = 0; t < nt; ++t) tiles.push_back(make_int2(m, (int)t));
    }
    gstart.push_back(M);
    wstart.push_back((int64_t)work.size());
    if ((int64_t)tiles.size() > INT32_MAX || (int64_t)work.size() > INT32_MAX)
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: too many frames", fn);
    hipStream_t s = ctx->stream;
    DevBuf &d_par = ctx->scratch[0], &d_lse = ctx->scratch[1], &d_lsep = ctx->scratch[2], &d_part = ctx->scratch[3],
           &d_out = ctx->scratch[4], &d_tab = ctx->scratch[5];
    StageScope st(ctx, where);
    const float* d_x = st.in(feats, (size_t)n_rows * D * sizeof(float));
    SSP_TRY(st.status());
    const size_t tab_models = (size_t)M * sizeof(EmModel), tab_work = work.size() * sizeof(int2), tab_tiles = tiles.size() * sizeof(int2);
    SSP_TRY(d_par.reserve(par.size() * sizeof(float)));
    SSP_TRY(d_lse.reserve((size_t)std::max<int64_t>(lse_tot, 1) * sizeof(float)));
    SSP_TRY(d_lsep.reserve((size_t)lsep_tot * sizeof(float)));
    SSP_TRY(d_part.reserve((size_t)part_max * sizeof(float)));
    SSP_TRY(d_out.reserve((size_t)M * (cols + 1) * sizeof(double)));
    SSP_TRY(d_tab.reserve(tab_models + tab_work + tab_tiles));
    std::vector<char> tab(tab_models + tab_work + tab_tiles);
    memcpy(tab.data(), md.data(), tab_models);
    memcpy(tab.data() + tab_models, work.data(), tab_work);
    if (tab_tiles) memcpy(tab.data() + tab_models + tab_work, tiles.data(), tab_tiles);
    SSP_HIP(hipMemcpyAsync(d_par.p, par.data(), par.size() * sizeof(float), hipMemcpyHostToDevice, s));
    SSP_HIP(hipMemcpyAsync(d_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, s));
    const EmModel* d_models = (const EmModel*)d_tab.p;
    const int2* d_work = (const int2*)((char*)d_tab.p + tab_models);
    const int2* d_tiles = (const int2*)((char*)d_tab.p + tab_models + tab_work);
    EmBatchArgs b{d_x, d_par.as<float>(), d_lse.as<float>(), d_lsep.as<float>(), d_part.as<float>(), d_models, d_work, D, K, Kp, shared ? (int64_t)0 : (int64_t)Kp * W};
    const size_t lds_acc = ((size_t)EM_TF * ((W + 1) | 1) + (size_t)(W + 1) * EM_KC + (size_t)EM_TF * 65 + 256) * sizeof(float);
    const size_t lds_lse = ((size_t)EM_TF * ((W + 1) | 1) + (size_t)(W + 1) * EM_WS + 256) * sizeof(float);
    const void* acc_k = nullptr;
    switch (nct * 2 + (fuse ? 1 : 0)) {
        case 2: acc_k = reinterpret_cast<const void*>(gmm_em_acc_mfma_seg_kernel<1, false>); break;
        case 3: acc_k = reinterpret_cast<const void*>(gmm_em_acc_mfma_seg_kernel<1, true>); break;
        case 4: acc_k = reinterpret_cast<const void*>(gmm_em_acc_mfma_seg_kernel<2, false>); break;
        case 5: acc_k = reinterpret_cast<const void*>(gmm_em_acc_mfma_seg_kernel<2, true>); break;
        case 6: acc_k = reinterpret_cast<const void*>(gmm_em_acc_mfma_seg_kernel<3, false>); break;
        default: acc_k = reinterpret_cast<const void*>(gmm_em_acc_mfma_seg_kernel<3, true>); break;
    }
    if (lds_acc > 64 * 1024) SSP_HIP(hipFuncSetAttribute(acc_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_acc));
    if (!fuse && lds_lse > 64 * 1024)
        SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gmm_em_lse_mfma_seg_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_lse));
    Timer tm;
    int rc = tm.start(kernel_ms != nullptr, s);
    if (rc == SSP_OK) {
        if (!fuse) {
            EmBatchArgs bt = b;
            bt.work = d_tiles;
            hipLaunchKernelGGL(gmm_em_lse_mfma_seg_kernel, dim3((unsigned)tiles.size()), dim3(256), lds_lse, s, bt);
        }
        for (size_t gi = 0; gi + 1 < gstart.size(); ++gi) {
            EmBatchArgs bg = b;
            bg.work = d_work + wstart[gi];
            const dim3 grid((unsigned)(wstart[gi + 1] - wstart[gi]), (unsigned)chunks);
            switch (nct * 2 + (fuse ? 1 : 0)) {
                case 2: hipLaunchKernelGGL((gmm_em_acc_mfma_seg_kernel<1, false>), grid, dim3(256), lds_acc, s, bg); break;
                case 3: hipLaunchKernelGGL((gmm_em_acc_mfma_seg_kernel<1, true>), grid, dim3(256), lds_acc, s, bg); break;
                case 4: hipLaunchKernelGGL((gmm_em_acc_mfma_seg_kernel<2, false>), grid, dim3(256), lds_acc, s, bg); break;
                case 5: hipLaunchKernelGGL((gmm_em_acc_mfma_seg_kernel<2, true>), grid, dim3(256), lds_acc, s, bg); break;
                case 6: hipLaunchKernelGGL((gmm_em_acc_mfma_seg_kernel<3, false>), grid, dim3(256), lds_acc, s, bg); break;
                default: hipLaunchKernelGGL((gmm_em_acc_mfma_seg_kernel<3, true>), grid, dim3(256), lds_acc, s, bg); break;
            }
            hipLaunchKernelGGL(gmm_em_reduce_seg_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)(gstart[gi + 1] - gstart[gi])), dim3(256), 0,
                               s, b, gstart[gi], cols, fuse ? 1 : 0, d_out.as<double>());
        }
        if (hipGetLastError() != hipSuccess) {
            set_error("%s: kernel launch failed", fn);
            rc = SSP_ERR_HIP;
        }
    }
    if (rc == SSP_OK) rc = tm.stop(s, kernel_ms);
    if (rc != SSP_OK) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    std::vector<double> host((size_t)M * (cols + 1));
    hipError_t he = hipMemcpyAsync(host.data(), d_out.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) SSP_FAIL(SSP_ERR_HIP, "%s: result copy failed: %s", fn, hipGetErrorString(he));
    for (int m = 0; m < M; ++m) {
        const double* o = host.data() + (size_t)m * (cols + 1);
        for (int k = 0; k < K; ++k) {
            const double* r = o + (size_t)k * W;
            for (int d = 0; d < D; ++d) {
                sx_out[((size_t)m * K + k) * D + d] = r[d];
                sxx_out[((size_t)m * K + k) * D + d] = r[D + d];
            }
            nk_out[(size_t)m * K + k] = r[2 * D];
        }
        loglik_sum_out[m] = o[cols];
    }
    return SSP_OK;
}

extern "C" int ssp_gmm_em_stats_batch(ssp_ctx* ctx, int32_t M, int32_t K, int32_t D, const double* weights, const double* means,
                                      const double* covars, const float* feats, int64_t n_rows, const int64_t* row_off,
                                      const int64_t* n_frames, double* nk_out, double* sx_out, double* sxx_out, double* loglik_sum_out,
                                      int where, float* kernel_ms) {
    return em_stats_batch_impl(ctx, M, K, D, weights, means, covars, feats, n_rows, row_off, n_frames, nk_out, sx_out, sxx_out, loglik_sum_out,
                               where, kernel_ms, false, "ssp_gmm_em_stats_batch");
}

extern "C" int ssp_gmm_em_stats_shared(ssp_ctx* ctx, int32_t M, int32_t K, int32_t D, const double* weights, const double* means,
                                       const double* covars, const float* feats, int64_t n_rows, const int64_t* row_off,
                                       const int64_t* n_frames, double* nk_out, double* sx_out, double* sxx_out, double* loglik_sum_out,
                                       int where, float* kernel_ms) {
    return em_stats_batch_impl(ctx, M, K, D, weights, means, covars, feats, n_rows, row_off, n_frames, nk_out, sx_out, sxx_out, loglik_sum_out,
                               where, kernel_ms, true, "ssp_gmm_em_stats_shared");
}
