// Top-C fast scoring of mean-adapted GMM-UBM speaker models on gfx950 (ssp_gmm_map_*).  An extension: the reference scores every mixture
// of every independently trained speaker model (GMM_UBM.py:158-170,181-197).  For S speaker models that share the UBM's weights and
// covariances and differ in their means, GMM[i].score(x) - UBM.score(x) (GMM_UBM.py:185) is evaluated over the UBM's best C mixtures of
// every frame (include/ssp.h has the definition):
//   L_s(x) - L_ubm(x) = log sum_{k in T(x)} post_k(x) exp(delta_{s,k}(x)),   post_k = exp(lp_k - L_ubm),   delta_{s,k} = x . a_{s,k} - b_{s,k}
// Kernels per call:
//   gmm_map_select_kernel  workgroup = 64 frames: the UBM's lp tiles per 64-mixture chunk on v_mfma_f32_32x32x2_f32, the tile function the
//                          EM kernels call (gmm_lp_tile.hpp: em_stage_aug, em_lp_tile); every lane keeps a sorted top-8 (value, index) of the 16 mixtures per chunk
//                          it sees of ITS frame; the four lists of a frame (two mixture halves x two lane halves) meet in LDS and one thread
//                          per frame merges them -> idx[frame][C] in rank order, q[frame][C] = lp - L_ubm (log posterior within T), L_ubm
//   gmm_map_score_kernel   workgroup = one utterance x 256 speakers, one wave per 64 of them (lane = speaker: a table row [k][d][speakers] is
//                          read coalesced).  Per block of 64 frames: the (frame, rank) pairs are bucketed by mixture in LDS once for the
//                          four waves (counting sort over K, integer LDS atomics); every wave then loads each distinct mixture's D + 1
//                          table columns ONCE into registers (those of the next two mixtures are in flight meanwhile) and walks the frames
//                          of its bucket; a (max, sum) pair per (frame, speaker) lives in LDS (4 x 32 KiB) and is updated online (delta is
//                          unbounded for a caller's means: no exp-domain sum without a running maximum); then log, and the block's frames
//                          are added in frame order in float64.  The workgroup walks all blocks of its utterance, so diff[u][s] leaves
//                          directly: no partials.
//   gmm_map_reduce_kernel  per utterance: mean of L_ubm (float64, fixed tree) and the first-index arg-max of the diff row
// A frame's folding order is ascending mixture index whatever else sits in its block, blocks never mix utterances, and no
// floating-point atomic exists here: same bits every call, and an utterance's results do not depend on its neighbours.
// Every loop bound and table index that is uniform per wave is read through readfirstlane (em_uniform, gmm_lp_tile.hpp).
#include <chrono>
#include <cmath>

#include "common.hpp"
#include "handle.hpp"
#include "gmm_lp_tile.hpp"

namespace ssp {

constexpr int MAP_TF = 64;    // frames per selection tile and per scoring block
constexpr int MAP_KC = 64;    // mixtures per chunk
constexpr int MAP_CMAX = 8;   // largest C
constexpr int MAP_SL = 64;    // speakers per wave
constexpr int MAP_WV = 4;     // waves (speaker tiles) per scoring workgroup

// (value, index) a ranks before b: larger value, of equal values the lower index
__device__ __forceinline__ bool map_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

struct MapSelArgs {
    const float* x;    // [frames x D], absolute rows
    const float* par;  // [Kp][2D+1]  (A = mu P, B = -P/2, c), padded and zero-weight mixtures c = -1e30
    int32_t* idx;      // [frames x C]
    float* q;          // [frames x C]
    float* lam;        // [frames]
    int64_t f0, f1;    // frame range of the call
    int32_t D, K, Kp, C;
};

__global__ __launch_bounds__(256) void gmm_map_select_kernel(MapSelArgs a) {
    extern __shared__ float sm[];
    const int D = a.D, W = 2 * D + 1, KS = (W + 1) / 2;
    const int XS = (2 * KS) | 1;
    float* xs = sm;                      // [64 frames][XS]  aug = [x, x^2, 1, 0]
    float* wsT = xs + MAP_TF * XS;       // [2 KS][64 mix]   parameter chunk, k-major
    float* lv = wsT + 2 * KS * MAP_KC;   // [64 frames][4 lists][8] values
    int* li = reinterpret_cast<int*>(lv + MAP_TF * 4 * MAP_CMAX);  // ... and indices
    const int tid = threadIdx.x, lane = tid & 63, wave = em_uniform(tid >> 6);
    const int fl = lane & 31, h = lane >> 5, r1 = wave >> 1, c1 = wave & 1;
    const int64_t base = a.f0 + (int64_t)blockIdx.x * MAP_TF;
    const int nt = (int)min<int64_t>(MAP_TF, a.f1 - base);
    em_stage_aug(xs, a.x, base, nt, D, KS, XS);
    const float* xrow = xs + (32 * c1 + fl) * XS;
    const float* wcol = wsT + h * MAP_KC + 32 * r1 + fl;
    float tv[MAP_CMAX];
    int ti[MAP_CMAX];
#pragma unroll
    for (int j = 0; j < MAP_CMAX; ++j) {
        tv[j] = -INFINITY;
        ti[j] = INT32_MAX;
    }
    for (int kc = 0; kc < a.Kp; kc += MAP_KC) {
        __syncthreads();  // the previous chunk's GEMM is done with wsT
        for (int i0 = 0; i0 < 2 * KS * MAP_KC; i0 += 256) {
            const int i = i0 + tid;
            if (i < 2 * KS * MAP_KC) {
                const int k = i / MAP_KC, mm = i - k * MAP_KC;
                wsT[i] = k < W ? a.par[(size_t)(kc + mm) * W + k] : 0.f;
            }
        }
        __syncthreads();
        const f32x16 acc = em_lp_tile<MAP_KC>(xrow, wcol, KS, h);
        // accumulator i = mixture kc + 32 r1 + em_lp_mix(i, h) of this lane's frame: ascending in i
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float v = acc[i];
            const int k = kc + 32 * r1 + em_lp_mix(i, h);
            if (map_before(v, k, tv[MAP_CMAX - 1], ti[MAP_CMAX - 1])) {  // (a NaN never enters: its frame is answered as bad below)
                tv[MAP_CMAX - 1] = v;
                ti[MAP_CMAX - 1] = k;
#pragma unroll
                for (int j = MAP_CMAX - 1; j > 0; --j) {
                    const bool up = map_before(tv[j], ti[j], tv[j - 1], ti[j - 1]);
                    const float v0 = tv[j - 1], v1 = tv[j];
                    const int i0 = ti[j - 1], i1 = ti[j];
                    tv[j - 1] = up ? v1 : v0;
                    tv[j] = up ? v0 : v1;
                    ti[j - 1] = up ? i1 : i0;
                    ti[j] = up ? i0 : i1;
                }
            }
        }
    }
    {
        const int fr = 32 * c1 + fl, part = 2 * r1 + h;
#pragma unroll
        for (int j = 0; j < MAP_CMAX; ++j) {
            lv[(fr * 4 + part) * MAP_CMAX + j] = tv[j];
            li[(fr * 4 + part) * MAP_CMAX + j] = ti[j];
        }
    }
    __syncthreads();
    if (tid < nt) {  // one thread per frame: merge of its four sorted lists, then the log posteriors within T
        const int fr = tid, C = a.C;
        bool bad = false;
        for (int d = 0; d < D; ++d) bad |= !(fabsf(xs[fr * XS + d]) <= 3.402823466e38f);
        int pos[4] = {0, 0, 0, 0};
        float ov[MAP_CMAX];
        int oi[MAP_CMAX];
#pragma unroll
        for (int j = 0; j < MAP_CMAX; ++j) {
            ov[j] = -INFINITY;
            oi[j] = -1;
            if (j < C) {
                float bvv = -INFINITY;
                int bi = INT32_MAX, bp = 0;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int at = (fr * 4 + p) * MAP_CMAX + min(pos[p], MAP_CMAX - 1);
                    const float v = pos[p] < MAP_CMAX ? lv[at] : -INFINITY;
                    const int k = pos[p] < MAP_CMAX ? li[at] : INT32_MAX;
                    if (map_before(v, k, bvv, bi)) {
                        bvv = v;
                        bi = k;
                        bp = p;
                    }
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) pos[p] += p == bp ? 1 : 0;
                ov[j] = bvv;
                oi[j] = bi;
            }
        }
        // finite entries whose squares overflow fp32 leave no C real mixtures with a finite lp: such a frame is bad too ("a value too large
        // for float32"), and no index outside [0, K) ever leaves this kernel
#pragma unroll
        for (int j = 0; j < MAP_CMAX; ++j)
            if (j < C) bad |= !(oi[j] >= 0 && oi[j] < a.K && ov[j] > -1.0e29f);
        float ssum = 0.f;
#pragma unroll
        for (int j = 0; j < MAP_CMAX; ++j)
            if (j < C) ssum += expf(ov[j] - ov[0]);
        const float lam = ov[0] + logf(ssum);
        const float nanv = __builtin_nanf("");
        a.lam[base + fr] = bad ? nanv : lam;
#pragma unroll
        for (int j = 0; j < MAP_CMAX; ++j)
            if (j < C) {
                a.idx[(base + fr) * C + j] = bad ? -1 : oi[j];
                a.q[(base + fr) * C + j] = bad ? nanv : ov[j] - lam;
            }
    }
}

struct MapScoreArgs {
    const float* x;        // [frames x D]
    const float* tab;      // [K][DP + 1][Sp]: a (DP columns, zero beyond D), then b
    const int32_t* idx;    // [frames x C]
    const float* q;        // [frames x C]
    const int64_t* off;    // [n_utt + 1] frame offsets
    float* diff;           // [n_utt x S]
    int32_t D, K, C, S, Sp;
};

template <int DP>
__global__ __launch_bounds__(256) void gmm_map_score_kernel(MapScoreArgs a) {
    extern __shared__ float sm[];
    const int D = a.D, C = a.C, K = a.K;
    float* xs = sm;                                   // [64 frames][DP]
    float* st = xs + MAP_TF * DP;                     // [4 waves][max | sum][64 frames][64 speakers]
    float* eq = st + MAP_WV * 2 * MAP_TF * MAP_SL;    // [64 x 8] log posterior of every sorted pair
    int* ent = reinterpret_cast<int*>(eq + MAP_TF * MAP_CMAX);  // [64 x 8] sorted pairs: mixture << 6 | frame
    int* badf = ent + MAP_TF * MAP_CMAX;              // [64]
    int* ntot = badf + MAP_TF;                        // [1] pairs of the block (+ 3 pad)
    int* cnt = ntot + 4;                              // [K]  histogram -> bucket starts -> bucket ends
    const int tid = threadIdx.x, lane = tid & 63, wave = em_uniform(tid >> 6);
    const int u = blockIdx.x, s0 = em_uniform((blockIdx.y * MAP_WV + wave) * MAP_SL);
    const bool live = s0 < a.Sp;                      // (a wave past the last speaker tile stages and sorts with the others, then idles)
    float* st_m = st + wave * 2 * MAP_TF * MAP_SL;
    float* st_s = st_m + MAP_TF * MAP_SL;
    const int64_t f0 = em_uniform64(a.off[u]), f1 = em_uniform64(a.off[u + 1]);
    const float* tcol = a.tab + (live ? s0 : 0) + lane;
    const size_t kstride = (size_t)(DP + 1) * a.Sp;
    const int per = (K + 63) / 64;  // histogram bins per lane in the scan
    double acc = 0.0;
    for (int64_t fb = f0; fb < f1; fb += MAP_TF) {
        const int nf = em_uniform((int)min<int64_t>(MAP_TF, f1 - fb));
        __syncthreads();  // the previous block is done with everything below
        for (int i0 = 0; i0 < nf * DP; i0 += 256) {
            const int i = i0 + tid;
            if (i < nf * DP) {
                const int r = i / DP, d = i - r * DP;
                xs[i] = d < D ? a.x[(fb + r) * D + d] : 0.f;
            }
        }
        for (int r = 0; r < nf; ++r) {
            st_m[r * MAP_SL + lane] = -INFINITY;
            st_s[r * MAP_SL + lane] = 0.f;
        }
        for (int k0 = 0; k0 < K; k0 += 256)
            if (k0 + tid < K) cnt[k0 + tid] = 0;
        if (tid < nf) badf[tid] = a.idx[(fb + tid) * C] < 0 ? 1 : 0;
        __syncthreads();
        const int np = em_uniform(nf * C);
        for (int p0 = 0; p0 < np; p0 += 256) {
            const int p = p0 + tid;
            if (p < np) {
                const int k = a.idx[fb * C + p];
                if (k >= 0 && k < K) atomicAdd(&cnt[k], 1);
            }
        }
        __syncthreads();
        if (wave == 0) {  // exclusive scan of the histogram: `per` consecutive bins per lane, then across the lanes
            int loc = 0;
            for (int j = 0; j < per; ++j) {
                const int k = lane * per + j;
                loc += k < K ? cnt[k] : 0;
            }
            int inc = loc;
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(inc, o);
                if (lane >= o) inc += t;
            }
            if (lane == 63) ntot[0] = inc;
            int run = inc - loc;
            for (int j = 0; j < per; ++j) {
                const int k = lane * per + j;
                if (k < K) {
                    const int c = cnt[k];
                    cnt[k] = run;
                    run += c;
                }
            }
        }
        __syncthreads();
        for (int p0 = 0; p0 < np; p0 += 256) {
            const int p = p0 + tid;
            if (p < np) {
                const int k = a.idx[fb * C + p];
                if (k >= 0 && k < K) {
                    const int at = atomicAdd(&cnt[k], 1);  // (the order inside a bucket is free: its pairs belong to different frames)
                    ent[at] = (k << 6) | (p / C);
                    eq[at] = a.q[fb * C + p];
                }
            }
        }
        __syncthreads();  // cnt[k] is now the END of bucket k
        const int n = live ? em_uniform(ntot[0]) : 0;
        // the table columns of the next TWO distinct mixtures fly while a bucket is walked: a wave keeps 2 (DP + 1) x 256 bytes in flight
        float n1[DP + 1], n2[DP + 1];
#pragma unroll
        for (int d = 0; d <= DP; ++d) n1[d] = n2[d] = 0.f;
        int e1 = 0, e2 = n;  // bucket starts of the mixtures in n1 (the one to walk next) and n2
        if (n > 0) {
            const int k1 = em_uniform(ent[0]) >> 6;
            const float* t = tcol + (size_t)k1 * kstride;
#pragma unroll
            for (int d = 0; d <= DP; ++d) n1[d] = t[(size_t)d * a.Sp];
            e2 = em_uniform(cnt[k1]);
            if (e2 < n) {
                const float* t2 = tcol + (size_t)(em_uniform(ent[e2]) >> 6) * kstride;
#pragma unroll
                for (int d = 0; d <= DP; ++d) n2[d] = t2[(size_t)d * a.Sp];
            }
        }
        while (e1 < n) {
            float cu[DP + 1];
#pragma unroll
            for (int d = 0; d <= DP; ++d) {
                cu[d] = n1[d];
                n1[d] = n2[d];
            }
            const int b0 = e1, b1 = e2;  // this bucket
            e1 = e2;
            if (e2 < n) {
                e2 = em_uniform(cnt[em_uniform(ent[e2]) >> 6]);
                if (e2 < n) {
                    const float* t2 = tcol + (size_t)(em_uniform(ent[e2]) >> 6) * kstride;
#pragma unroll
                    for (int d = 0; d <= DP; ++d) n2[d] = t2[(size_t)d * a.Sp];
                }
            }
            for (int i = b0; i < b1; ++i) {
                const int r = em_uniform(ent[i]) & 63;
                const float* xr = xs + r * DP;
                float dl[4] = {0.f, 0.f, 0.f, 0.f};  // four interleaved chains (fixed shape): a single one waits on itself
#pragma unroll
                for (int d = 0; d < DP; ++d) dl[d & 3] = fmaf(xr[d], cu[d], dl[d & 3]);
                const float v = eq[i] + (((dl[0] + dl[1]) + (dl[2] + dl[3])) - cu[DP]);
                const float m = st_m[r * MAP_SL + lane], s = st_s[r * MAP_SL + lane];
                const float ex = __expf(-fabsf(v - m));  // (first pair of a frame: m = -inf, ex = 0, s -> 1)
                const bool up = v > m;
                st_m[r * MAP_SL + lane] = up ? v : m;
                st_s[r * MAP_SL + lane] = up ? fmaf(s, ex, 1.f) : s + ex;
            }
        }
        if (live)
            for (int r = 0; r < nf; ++r) {  // (this wave's own state: no barrier needed)
                const float v = st_m[r * MAP_SL + lane] + __logf(st_s[r * MAP_SL + lane]);
                acc += badf[r] ? (double)__builtin_nanf("") : (double)v;
            }
    }
    if (live && s0 + lane < a.S) a.diff[(size_t)u * a.S + s0 + lane] = (float)(acc / (double)(f1 - f0));  // (T = 0: 0 / 0 = NaN)
}

// per utterance: ubm[u] = mean_t L_ubm (float64: strided partial sums in a fixed order, then a fixed tree) and the FIRST index of the
// diff row's maximum as numpy.argmax finds it (a NaN is the maximum)
__global__ __launch_bounds__(256) void gmm_map_reduce_kernel(const float* __restrict__ lam, const int64_t* __restrict__ off,
                                                             const float* __restrict__ diff, int S, float* __restrict__ ubm,
                                                             int32_t* __restrict__ argmax) {
    __shared__ double sh[256];
    __shared__ float bv[256];
    __shared__ int bi[256];
    const int u = blockIdx.x, tid = threadIdx.x;
    const int64_t f0 = off[u], f1 = off[u + 1];
    if (ubm) {
        double v = 0.0;
        for (int64_t f = f0 + tid; f < f1; f += 256) v += (double)lam[f];
        sh[tid] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) sh[tid] += sh[tid + o];
            __syncthreads();
        }
        if (tid == 0) ubm[u] = (float)(sh[0] / (double)(f1 - f0));
    }
    if (argmax) {
        auto before = [](float va, int ia, float vb, int ib) {  // (va, ia) wins over (vb, ib)
            const bool na = va != va, nb = vb != vb;
            if (na || nb) return na && (!nb || ia < ib);
            return va > vb || (va == vb && ia < ib);
        };
        float best = -INFINITY;
        int at = INT32_MAX;
        for (int s = tid; s < S; s += 256) {
            const float v = diff[(size_t)u * S + s];
            if (before(v, s, best, at)) {
                best = v;
                at = s;
            }
        }
        bv[tid] = best;
        bi[tid] = at;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o && before(bv[tid + o], bi[tid + o], bv[tid], bi[tid])) {
                bv[tid] = bv[tid + o];
                bi[tid] = bi[tid + o];
            }
            __syncthreads();
        }
        if (tid == 0) argmax[u] = bi[0] == INT32_MAX ? 0 : bi[0];
    }
}

}  // namespace ssp

struct ssp_gmm_map {
    ssp_ctx* ctx = nullptr;
    int32_t K = 0, D = 0, S = 0, Kp = 0, DP = 0, Sp = 0, nnz = 0;
    ssp::DevBuf par, tab;              // the UBM's rows for the selection kernel; the speakers' a | b table
    ssp::DevBuf idx, q, lam, diff;     // grow-only scratch of the calls
};

using namespace ssp;

static size_t map_select_lds(int D) {
    const int W = 2 * D + 1, KS = (W + 1) / 2;
    return ((size_t)MAP_TF * ((2 * KS) | 1) + (size_t)2 * KS * MAP_KC + (size_t)2 * MAP_TF * 4 * MAP_CMAX) * sizeof(float);
}
static size_t map_score_lds(int DP, int K) {
    return ((size_t)MAP_TF * DP + (size_t)MAP_WV * 2 * MAP_TF * MAP_SL + (size_t)2 * MAP_TF * MAP_CMAX + MAP_TF + 4 + (size_t)K) * sizeof(float);
}
constexpr size_t MAP_LDS_MAX = 160 * 1024;

extern "C" {

int ssp_gmm_map_pack(ssp_ctx* ctx, int32_t K, int32_t D, const double* ubm_weights, const double* ubm_means, const double* ubm_covars,
                     int32_t S, const double* spk_means, ssp_gmm_map** out) try {
    ssp::TraceRange trace_("ssp_gmm_map_pack");
    if (!out) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_map_pack: null out");
    *out = nullptr;
    SSP_TRY(use_ctx(ctx));
    if (K < 1 || D < 1 || !ubm_weights || !ubm_means || !ubm_covars) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_map_pack: bad shape or null parameter array");
    if (S < 1 || !spk_means) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_map_pack: S < 1 (no speaker model)");
    if (2 * D + 1 > 96) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_gmm_map_pack: D=%d exceeds the supported feature dimension (47)", D);
    const int DP = (D + 7) / 8 * 8;
    if (map_score_lds(DP, K) > MAP_LDS_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_gmm_map_pack: K=%d: the bucket table does not fit the LDS", K);
    int nnz = 0;
    for (int k = 0; k < K; ++k) {
        const double wk = ubm_weights[k];
        if (!(wk >= 0.0) || std::isinf(wk)) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_map_pack: negative or non-finite weight (mix %d)", k);
        nnz += wk > 0.0 ? 1 : 0;
        for (int d = 0; d < D; ++d)
            if (!(ubm_covars[(size_t)k * D + d] > 0.0)) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_map_pack: non-positive covariance (mix %d)", k);
    }
    if (nnz == 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_map_pack: every weight is zero");
    const int W = 2 * D + 1, Kp = (K + MAP_KC - 1) / MAP_KC * MAP_KC, Sp = (S + MAP_SL - 1) / MAP_SL * MAP_SL;
    // the UBM's rows as the EM kernels read them (A = mu P, B = -P / 2, c); padded and zero-weight mixtures: the finite constant -1e30
    std::vector<float> par((size_t)Kp * W, 0.f);
    const double ln2pi = std::log(2.0 * M_PI);
    for (int k = 0; k < Kp; ++k) {
        float* w = par.data() + (size_t)k * W;
        if (k >= K || !(ubm_weights[k] > 0.0)) {
            w[2 * D] = -1.0e30f;
            continue;
        }
        double c = std::log(ubm_weights[k]) - 0.5 * D * ln2pi;
        for (int d = 0; d < D; ++d) {
            const double P = 1.0 / ubm_covars[(size_t)k * D + d], mu = ubm_means[(size_t)k * D + d];
            w[d] = (float)(mu * P);
            w[D + d] = (float)(-0.5 * P);
            c += 0.5 * std::log(P) - 0.5 * mu * mu * P;
        }
        w[2 * D] = (float)c;
    }
    // a | b of every (mixture, speaker), float64 then fp32: [K][DP + 1][Sp], speakers innermost
    std::vector<float> tab((size_t)K * (DP + 1) * Sp, 0.f);
    for (int s = 0; s < S; ++s)
        for (int k = 0; k < K; ++k) {
            const double* ms = spk_means + ((size_t)s * K + k) * D;
            const double* mu = ubm_means + (size_t)k * D;
            const double* cv = ubm_covars + (size_t)k * D;
            float* t = tab.data() + (size_t)k * (DP + 1) * Sp + s;
            double b = 0.0;
            for (int d = 0; d < D; ++d) {
                const double P = 1.0 / cv[d];
                t[(size_t)d * Sp] = (float)((ms[d] - mu[d]) * P);
                b += (ms[d] * ms[d] - mu[d] * mu[d]) * P;
            }
            t[(size_t)DP * Sp] = (float)(0.5 * b);
        }
    HandleBuild<ssp_gmm_map> g(ctx, "ssp_gmm_map_pack");
    g->K = K;
    g->D = D;
    g->S = S;
    g->Kp = Kp;
    g->DP = DP;
    g->Sp = Sp;
    g->nnz = nnz;
    int rc = upload(g, g->par, par);
    if (rc == SSP_OK) rc = upload(g, g->tab, tab);
    return g.commit(rc, out);
}
SSP_CREATE_GUARD("ssp_gmm_map_pack")

int ssp_gmm_map_destroy(ssp_gmm_map* map) { return destroy_handle(map); }

// every argument check of ssp_gmm_map_score that needs no GPU work
static int map_check(const ssp_gmm_map* map, const ssp_segments* frame_seg, int32_t C, const char* fn) {
    if (!map || !frame_seg) SSP_FAIL(SSP_ERR_INVALID, "%s: null handle", fn);
    if (C < 1) SSP_FAIL(SSP_ERR_INVALID, "%s: C=%d: at least one mixture per frame", fn, C);
    if (C > MAP_CMAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: C=%d exceeds the supported %d mixtures per frame", fn, C, MAP_CMAX);
    if (C > map->nnz) SSP_FAIL(SSP_ERR_INVALID, "%s: C=%d exceeds the UBM's %d mixtures of non-zero weight", fn, C, map->nnz);
    return SSP_OK;
}

int ssp_gmm_map_score(ssp_gmm_map* map, const float* feats, const ssp_segments* frame_seg, int32_t C, float* diff_out, float* ubm_out,
                      int32_t* argmax_out, int32_t* idx_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_gmm_map_score");
    SSP_TRY(map_check(map, frame_seg, C, "ssp_gmm_map_score"));
    ssp_ctx* ctx = map->ctx;
    SSP_TRY(use_ctx(ctx));
    SSP_TRY(check_where(where, "ssp_gmm_map_score"));
    if (kernel_ms) *kernel_ms = 0.f;
    const int64_t f0 = frame_seg->host.front(), F = frame_seg->host.back(), n_utt = frame_seg->n;
    if (n_utt == 0) return SSP_OK;
    if (F > f0 && !feats) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_map_score: null feats");
    if (n_utt > INT32_MAX || (F - f0 + MAP_TF - 1) / MAP_TF > INT32_MAX || F > INT64_MAX / (MAP_CMAX * 8))
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_gmm_map_score: too many utterances or frames");
    hipStream_t s = ctx->stream;
    const int D = map->D, S = map->S;
    const size_t rows = (size_t)std::max<int64_t>(F, 1);
    StageScope st(ctx, where);
    const float* d_x = st.in(feats, (size_t)F * D * sizeof(float));
    float* d_diff = st.out(diff_out, (size_t)n_utt * S * sizeof(float));
    float* d_ubm = st.out(ubm_out, (size_t)n_utt * sizeof(float));
    int32_t* d_am = st.out(argmax_out, (size_t)n_utt * sizeof(int32_t));
    // (a batch without frames has no idx_out entries to give back: `rows` is 1 then, the caller's array empty)
    int32_t* d_idx = st.out(F > 0 || where == SSP_DEVICE ? idx_out : nullptr, rows * C * sizeof(int32_t));
    SSP_TRY(st.status());
    if (!d_idx) {
        SSP_TRY(map->idx.reserve(rows * C * sizeof(int32_t)));
        d_idx = map->idx.as<int32_t>();
    }
    SSP_TRY(map->q.reserve(rows * C * sizeof(float)));
    SSP_TRY(map->lam.reserve(rows * sizeof(float)));
    const bool want_diff = diff_out || argmax_out;
    if (want_diff && !d_diff) {
        SSP_TRY(map->diff.reserve((size_t)n_utt * S * sizeof(float)));
        d_diff = map->diff.as<float>();
    }
    const size_t lds_sel = map_select_lds(D), lds_sc = map_score_lds(map->DP, map->K);
    const void* score_k = nullptr;
    switch (map->DP) {
        case 8: score_k = reinterpret_cast<const void*>(gmm_map_score_kernel<8>); break;
        case 16: score_k = reinterpret_cast<const void*>(gmm_map_score_kernel<16>); break;
        case 24: score_k = reinterpret_cast<const void*>(gmm_map_score_kernel<24>); break;
        case 32: score_k = reinterpret_cast<const void*>(gmm_map_score_kernel<32>); break;
        case 40: score_k = reinterpret_cast<const void*>(gmm_map_score_kernel<40>); break;
        default: score_k = reinterpret_cast<const void*>(gmm_map_score_kernel<48>); break;
    }
    if (lds_sel > 64 * 1024)
        SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gmm_map_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sel));
    if (lds_sc > 64 * 1024) SSP_HIP(hipFuncSetAttribute(score_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sc));
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    if (F > f0) {
        MapSelArgs a{d_x, map->par.as<float>(), d_idx, map->q.as<float>(), map->lam.as<float>(), f0, F, D, map->K, map->Kp, C};
        hipLaunchKernelGGL(gmm_map_select_kernel, dim3((unsigned)((F - f0 + MAP_TF - 1) / MAP_TF)), dim3(256), lds_sel, s, a);
    }
    if (want_diff) {
        MapScoreArgs b{d_x, map->tab.as<float>(), d_idx, map->q.as<float>(), frame_seg->dev.as<int64_t>(), d_diff, D, map->K, C, S, map->Sp};
        const dim3 grid((unsigned)n_utt, (unsigned)((map->Sp / MAP_SL + MAP_WV - 1) / MAP_WV));
        switch (map->DP) {
            case 8: hipLaunchKernelGGL(gmm_map_score_kernel<8>, grid, dim3(256), lds_sc, s, b); break;
            case 16: hipLaunchKernelGGL(gmm_map_score_kernel<16>, grid, dim3(256), lds_sc, s, b); break;
            case 24: hipLaunchKernelGGL(gmm_map_score_kernel<24>, grid, dim3(256), lds_sc, s, b); break;
            case 32: hipLaunchKernelGGL(gmm_map_score_kernel<32>, grid, dim3(256), lds_sc, s, b); break;
            case 40: hipLaunchKernelGGL(gmm_map_score_kernel<40>, grid, dim3(256), lds_sc, s, b); break;
            default: hipLaunchKernelGGL(gmm_map_score_kernel<48>, grid, dim3(256), lds_sc, s, b); break;
        }
    }
    if (d_ubm || d_am)
        hipLaunchKernelGGL(gmm_map_reduce_kernel, dim3((unsigned)n_utt), dim3(256), 0, s, map->lam.as<float>(), frame_seg->dev.as<int64_t>(), d_diff, S,
                           d_ubm, d_am);
    if (hipGetLastError() != hipSuccess) {
        (void)hipStreamSynchronize(s);
        SSP_FAIL(SSP_ERR_HIP, "ssp_gmm_map_score: kernel launch failed");
    }
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}

int ssp_gmm_map_score_list(ssp_gmm_map* map, const void* const* rows, int row_type, int32_t dim, const ssp_segments* frame_seg, int32_t C,
                           float* diff_out, float* ubm_out, int32_t* argmax_out, int32_t* idx_out, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_gmm_map_score_list");
    // (every argument is checked before the ctx is touched; the gather is ssp_gmm_score_list's)
    SSP_TRY(map_check(map, frame_seg, C, "ssp_gmm_map_score_list"));
    if (row_type != 0 && row_type != 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_map_score_list: row_type must be 0 (float32) or 1 (float64)");
    if (dim != map->D) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_map_score_list: dim=%d, the models have D=%d", dim, map->D);
    const std::vector<int64_t>& fo = frame_seg->host;
    if (fo.front() != 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_map_score_list: frame segments must start at frame 0");
    const int64_t n = frame_seg->n, F = fo.back();
    if (n > 0 && !rows) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_map_score_list: null row table");
    for (int64_t u = 0; u < n; ++u)
        if (!rows[u] && fo[(size_t)u + 1] > fo[(size_t)u])
            SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_map_score_list: null pointer for utterance %lld of %lld rows", (long long)u,
                     (long long)(fo[(size_t)u + 1] - fo[(size_t)u]));
    ssp_ctx* ctx = map->ctx;
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (n == 0 || F == 0) return ssp_gmm_map_score(map, nullptr, frame_seg, C, diff_out, ubm_out, argmax_out, idx_out, SSP_HOST, kernel_ms);
    const size_t row_elems = (size_t)dim;
    SSP_TRY(pipe_bounce(ctx, (size_t)F * row_elems * sizeof(float) + 16, 0));
    float* bounce = ctx->pipe->bounce_in.as<float>();
    std::vector<CopyPiece> pieces;
    for (int64_t u = 0; u < n; ++u) {
        const size_t T = (size_t)(fo[(size_t)u + 1] - fo[(size_t)u]);
        if (!T) continue;
        float* dst = bounce + (size_t)fo[(size_t)u] * row_elems;
        if (row_type == 1)
            add_pieces(pieces, rows[u], dst, T * row_elems, COPY_F64_TO_F32);
        else
            add_pieces(pieces, rows[u], dst, T * row_elems * sizeof(float), COPY_BYTES);
    }
    run_pieces(pipe_pool(ctx), pieces);
    return ssp_gmm_map_score(map, bounce, frame_seg, C, diff_out, ubm_out, argmax_out, idx_out, SSP_HOST, kernel_ms);
}

}  // extern "C"
