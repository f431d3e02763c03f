// i-vector extraction and the E-step of total-variability training on gfx950 (ssp_ivector_*).  An extension: the reference has no factor
// analysis; sidekit, the package it imports its features from, ships this model as FactorAnalyser.total_variability / extract_ivectors
// (Dehak et al. 2011, after Kenny 2005).  include/ssp.h has the definitions.  Everything on the device is fp32 with exact-fp32 MFMA.
// Kernels:
//   iv_pack_kernel    P[k] = T_k' diag(1/cv_k) T_k as a packed lower triangle (row i, column j <= i at i (i + 1) / 2 + j) and
//                     G = diag(1/cv) T, both summed in float64 from the float64 T on the device and rounded once
//   iv_gemm_kernel    C[M x N] = A[M x Kd] . B[Kd x N] on v_mfma_f32_32x32x2_f32, staged through LDS in k-major panels of 16 (the next
//                     panel's global loads fly in registers under the MFMAs); a workgroup of four waves owns 64 TM x 64 TN outputs
//                     (2 x 2 waves of TM x TN MFMA tiles).  A is read row-major or, transA, as [Kd x M]: Lp = N . P and b = f . G take
//                     it row-major, the E-step accumulators N' . S and f' . W transposed.  The sum over k is cut into chunks of 1024
//                     (grid z), each ONE k-ordered fma chain; iv_fold_kernel adds the chunks in ascending order in fp32: an
//                     output's bits do not depend on the tile shape, on M or on where its row sits.
//   iv_chol_kernel    one workgroup per utterance, the packed triangle of L_u = I + Lp_u in LDS: left-looking Cholesky in place (thread
//                     = row: its own row is contiguous, and triangular numbers mod 32 are a permutation, so a wave's row reads hit every
//                     bank once; the pivot row is a broadcast), forward and back substitution, log|L| and b'w as fixed float64 trees.
//                     E-step: on in place to the inverse of the factor (columns from the last), its Gram product L^-1 (rows from the
//                     first), and S = L^-1 + w w' back over Lp.
//   iv_accum_kernel   float64 accumulators += the chunks of one slab's accumulator GEMM, chunks and slabs in order
// No floating-point atomic exists here and every sum has a fixed shape: same bits every call.
#include <algorithm>
#include <cmath>
#include <thread>

#include "common.hpp"
#include "handle.hpp"

namespace ssp {

constexpr int IV_RMAX = 256;   // largest rank: the packed triangle and the kernel's other LDS stay inside a workgroup's 160 KiB
constexpr int IV_BK = 16;      // k per staged panel
constexpr int IV_KC = 1024;     // k per fma chain: a GEMM's sum over k is cut into chunks of this many, each one chain (grid z)
constexpr int IV_STAGES = 5;   // precision GEMM, right-hand-side GEMM, Cholesky, A accumulator GEMM, C accumulator GEMM

using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ int iv_tri(int i) { return i * (i + 1) / 2; }

struct IvPackArgs {
    const double* T;    // [K][D][R]
    const double* icv;  // [K][D] 1 / covariance
    float* P;           // [K][tri]
    float* G;           // [K D][R]
    int32_t K, D, R, tri;
};

__global__ __launch_bounds__(256) void iv_pack_kernel(IvPackArgs a) {
    const int k = blockIdx.y, D = a.D, R = a.R;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const double* T = a.T + (size_t)k * D * R;
    const double* icv = a.icv + (size_t)k * D;
    if (p < a.tri) {
        int i = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
        while (iv_tri(i) > p) --i;
        while (iv_tri(i + 1) <= p) ++i;
        const int j = p - iv_tri(i);
        double s = 0.0;
        for (int d = 0; d < D; ++d) s = fma(T[(size_t)d * R + i] * icv[d], T[(size_t)d * R + j], s);
        a.P[(size_t)k * a.tri + p] = (float)s;
    }
    if (p < D * R) a.G[(size_t)k * D * R + p] = (float)(T[p] * icv[p / R]);
}

struct IvGemmArgs {
    const float* A;  // [M x Kd] (lda), or with transA [Kd x M]
    const float* B;  // [Kd x N] (ldb)
    float* C;        // [chunks][M x N]: chunk z holds the sum over k in [z IV_KC, (z + 1) IV_KC)
    int64_t M, N, Kd, lda, ldb;
    int32_t transA;
};

template <int TM, int TN>
__global__ __launch_bounds__(256) void iv_gemm_kernel(IvGemmArgs a) {
    constexpr int BM = 64 * TM, BN = 64 * TN, LA = BM + 4, LB = BN + 4, SA = BM * IV_BK / 256, SB = BN * IV_BK / 256;
    __shared__ float As[IV_BK * LA];
    __shared__ float Bs[IV_BK * LB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5, wr = wave >> 1, wc = wave & 1;
    const int64_t m0 = (int64_t)blockIdx.y * BM, n0 = (int64_t)blockIdx.x * BN;
    const int64_t kbeg = (int64_t)blockIdx.z * IV_KC, kend = min(a.Kd, kbeg + IV_KC);
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // this thread's cells of a panel: where they come from (relative to the panel's first k) and where they go in LDS
    int64_t oa[SA], ob[SB];
    int ka[SA], kb[SB], la[SA], lb[SB];
#pragma unroll
    for (int s = 0; s < SA; ++s) {
        const int e = s * 256 + tid, k = a.transA ? e / BM : e % IV_BK, m = a.transA ? e % BM : e / IV_BK;
        const int64_t gm = m0 + m;
        ka[s] = gm < a.M ? k : IV_KC;  // (a row past M never passes the k test below)
        la[s] = k * LA + m;
        oa[s] = a.transA ? (int64_t)k * a.lda + gm : gm * a.lda + k;
    }
#pragma unroll
    for (int s = 0; s < SB; ++s) {
        const int e = s * 256 + tid, n = e % BN, k = e / BN;
        const int64_t gn = n0 + n;
        kb[s] = gn < a.N ? k : IV_KC;
        lb[s] = k * LB + n;
        ob[s] = (int64_t)k * a.ldb + gn;
    }
    float ra[SA], rb[SB];
    auto fetch = [&](int64_t k0) {
        const float* pa = a.A + (a.transA ? k0 * a.lda : k0);
        const float* pb = a.B + k0 * a.ldb;
#pragma unroll
        for (int s = 0; s < SA; ++s) ra[s] = k0 + ka[s] < kend ? pa[oa[s]] : 0.f;
#pragma unroll
        for (int s = 0; s < SB; ++s) rb[s] = k0 + kb[s] < kend ? pb[ob[s]] : 0.f;
    };
    fetch(kbeg);
    for (int64_t k0 = kbeg; k0 < kend; k0 += IV_BK) {
        __syncthreads();  // the previous panel's MFMAs are done with As and Bs
#pragma unroll
        for (int s = 0; s < SA; ++s) As[la[s]] = ra[s];
#pragma unroll
        for (int s = 0; s < SB; ++s) Bs[lb[s]] = rb[s];
        __syncthreads();
        if (k0 + IV_BK < kend) fetch(k0 + IV_BK);  // the next panel's loads fly under this panel's MFMAs
#pragma unroll
        for (int kk = 0; kk < IV_BK; kk += 2) {
            float av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = As[(kk + lh) * LA + (wr * TM + i) * 32 + li];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = Bs[(kk + lh) * LB + (wc * TN + j) * 32 + li];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }
    // accumulator r of a tile: row (r & 3) + 8 (r >> 2) + 4 lh, column li
    float* C = a.C + (size_t)blockIdx.z * (size_t)a.M * (size_t)a.N;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int64_t gn = n0 + (wc * TN + j) * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t gm = m0 + (wr * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (gm < a.M && gn < a.N) C[gm * a.N + gn] = acc[i][j][r];
            }
        }
}

// out = the chunks of a GEMM added in ascending order (fp32)
__global__ __launch_bounds__(256) void iv_fold_kernel(float* __restrict__ out, const float* __restrict__ part, size_t n, int chunks) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = part[i];
    for (int z = 1; z < chunks; ++z) v += part[(size_t)z * n + i];
    out[i] = v;
}

struct IvCholArgs {
    float* Lp;       // [U x tri]: sum_k nk P_k in; with mode 1, S = L^-1 + w w' out
    const float* b;  // [U x R]
    float* w;        // [U x R]
    float* logdet;   // [U]
    float* quad;     // [U]
    double* obj;     // [U]  -logdet / 2 + quad / 2 before either is rounded to fp32
    int32_t R, tri, mode;
};

// fixed tree over the workgroup's 256 values
__device__ __forceinline__ double iv_reduce(double* red, int tid, double v) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void iv_chol_kernel(IvCholArgs a) {
    extern __shared__ double iv_smem[];
    double* red = iv_smem;                             // [256]
    float* ys = reinterpret_cast<float*>(red + 256);   // [256]
    float* L = ys + 256;                               // [tri]
    const int R = a.R, tri = a.tri, tid = threadIdx.x;
    const size_t u = blockIdx.x;
    float* g = a.Lp + u * (size_t)tri;
    for (int p = tid; p < tri; p += 256) L[p] = g[p];
    const bool mine = tid < R;
    const int row = iv_tri(tid);  // this thread's row starts here (rows beyond R are never touched)
    __syncthreads();
    if (mine) L[row + tid] += 1.f;
    __syncthreads();
    // left-looking Cholesky, in place
    for (int j = 0; j < R; ++j) {
        const int rj = iv_tri(j);
        float s = 0.f;
        if (mine && tid >= j) {
            s = L[row + j];
#pragma unroll 8
            for (int k = 0; k < j; ++k) s = fmaf(-L[row + k], L[rj + k], s);
            if (tid == j) L[rj + j] = sqrtf(s);
        }
        __syncthreads();
        if (mine && tid > j) L[row + j] = s / L[rj + j];
        __syncthreads();
    }
    const double ld = 2.0 * iv_reduce(red, tid, mine ? log((double)L[row + tid]) : 0.0);
    // forward substitution L y = b (thread = row; y_j through LDS)
    float bi = mine ? a.b[u * R + tid] : 0.f;
    for (int j = 0; j < R; ++j) {
        if (tid == j) ys[j] = bi / L[row + j];
        __syncthreads();
        if (mine && tid > j) bi = fmaf(-L[row + j], ys[j], bi);
    }
    float yi = mine ? ys[tid] : 0.f;
    const double qd = iv_reduce(red, tid, (double)yi * (double)yi);  // b' L^-1 b = y' y
    // back substitution L' w = y, over ys
    for (int j = R - 1; j >= 0; --j) {
        if (tid == j) ys[j] = yi / L[row + j];
        __syncthreads();
        if (tid < j) yi = fmaf(-L[iv_tri(j) + tid], ys[j], yi);
    }
    if (mine) a.w[u * R + tid] = ys[tid];
    if (tid == 0) {
        a.logdet[u] = (float)ld;
        a.quad[u] = (float)qd;
        a.obj[u] = 0.5 * (qd - ld);
    }
    if (!a.mode) return;
    // M = (the factor)^-1 in place, columns from the last: M[i][j] = -(sum_{j < k <= i} M[i][k] L[k][j]) / L[j][j]
    for (int j = R - 1; j >= 0; --j) {
        const int rj = iv_tri(j);
        const float dj = 1.f / L[rj + j];
        float x = 0.f;
        if (mine && tid > j) {
            int tk = iv_tri(j + 1);
#pragma unroll 8
            for (int k = j + 1; k <= tid; ++k) {
                x = fmaf(L[row + k], L[tk + j], x);
                tk += k + 1;
            }
        }
        __syncthreads();  // column j has been read
        if (tid == j)
            L[rj + j] = dj;
        else if (mine && tid > j)
            L[row + j] = -x * dj;
        __syncthreads();
    }
    // L^-1 = M' M in place, rows from the first (thread = column): row i reads rows >= i, which are still M
    for (int i = 0; i < R; ++i) {
        float s = 0.f;
        if (tid <= i) {
            int tk = iv_tri(i);
#pragma unroll 8
            for (int k = i; k < R; ++k) {
                s = fmaf(L[tk + i], L[tk + tid], s);
                tk += k + 1;
            }
        }
        __syncthreads();
        if (tid <= i) L[iv_tri(i) + tid] = s;
    }
    __syncthreads();
    const float wt = mine ? ys[tid] : 0.f;
    for (int i = 0; i < R; ++i)
        if (tid <= i) g[iv_tri(i) + tid] = fmaf(ys[i], wt, L[iv_tri(i) + tid]);
}

// float64 accumulator (+)= the chunks of one slab's accumulator GEMM, in ascending order
__global__ __launch_bounds__(256) void iv_accum_kernel(double* __restrict__ acc, const float* __restrict__ part, size_t n, int chunks, int first) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v = first ? 0.0 : acc[i];
    for (int z = 0; z < chunks; ++z) v += (double)part[(size_t)z * n + i];
    acc[i] = v;
}

}  // namespace ssp

struct ssp_ivector {
    ssp_ctx* ctx = nullptr;
    int32_t K = 0, D = 0, R = 0, tri = 0;
    std::vector<double> mu;                 // [K x D]
    ssp::DevBuf T64, icv, P, G;             // the model on the device
    ssp::DevBuf nk, f, Lp, b, w, ld, qd, obj;   // one slab
    ssp::DevBuf part;                       // the chunks of the GEMM that is running, when it has more than one (or accumulates)
    ssp::DevBuf Aacc, Cacc;                 // E-step: the float64 sums over the chunks and slabs
    size_t cap = (size_t)1 << 30;
    int64_t last_slab = 0;
    float stage_ms[ssp::IV_STAGES] = {0.f, 0.f, 0.f, 0.f, 0.f};
    hipEvent_t ev[ssp::IV_STAGES + 1] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~ssp_ivector() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

using namespace ssp;

static size_t iv_chol_lds(int tri) { return 256 * sizeof(double) + 256 * sizeof(float) + (size_t)tri * sizeof(float); }

static int64_t iv_chunks(int64_t Kd) { return ceil_div<int64_t>(Kd, IV_KC); }

// the chunks of C[M x N] = A . B into `part` ([chunks][M x N]; one chunk may be the destination itself)
static void iv_gemm(hipStream_t s, const float* A, const float* B, float* part, int64_t M, int64_t N, int64_t Kd, int64_t lda, int64_t ldb, bool transA) {
    IvGemmArgs g{A, B, part, M, N, Kd, lda, ldb, transA ? 1 : 0};
    const unsigned nz = (unsigned)iv_chunks(Kd);
    // 128 x 128 tiles once they fill the device, else 64 x 64 (the bits are the same)
    if (ceil_div<int64_t>(M, 128) * ceil_div<int64_t>(N, 128) * nz >= 256)
        hipLaunchKernelGGL((iv_gemm_kernel<2, 2>), dim3((unsigned)ceil_div<int64_t>(N, 128), (unsigned)ceil_div<int64_t>(M, 128), nz), dim3(256), 0, s, g);
    else
        hipLaunchKernelGGL((iv_gemm_kernel<1, 1>), dim3((unsigned)ceil_div<int64_t>(N, 64), (unsigned)ceil_div<int64_t>(M, 64), nz), dim3(256), 0, s, g);
}

// C = A . B in fp32: straight into C when the sum over k is one chain, else through `part` and the fold kernel
static void iv_gemm_f32(hipStream_t s, const float* A, const float* B, float* C, float* part, int64_t M, int64_t N, int64_t Kd) {
    const int nz = (int)iv_chunks(Kd);
    iv_gemm(s, A, B, nz == 1 ? C : part, M, N, Kd, Kd, N, false);
    if (nz > 1) hipLaunchKernelGGL(iv_fold_kernel, dim3((unsigned)ceil_div<size_t>((size_t)M * N, 256)), dim3(256), 0, s, C, part, (size_t)M * N, nz);
}

// acc (+)= A' . B, A [Kd x M], in float64 over the chunks
static void iv_gemm_acc(hipStream_t s, const float* A, const float* B, double* acc, float* part, int64_t M, int64_t N, int64_t Kd, bool first) {
    iv_gemm(s, A, B, part, M, N, Kd, M, N, true);
    hipLaunchKernelGGL(iv_accum_kernel, dim3((unsigned)ceil_div<size_t>((size_t)M * N, 256)), dim3(256), 0, s, acc, part, (size_t)M * N, (int)iv_chunks(Kd),
                       first ? 1 : 0);
}

static int iv_upload_T(ssp_ivector* iv, const double* T) {
    const size_t n = (size_t)iv->K * iv->D * iv->R;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(T[i])) SSP_FAIL(SSP_ERR_INVALID, "ssp_ivector: non-finite entry in T (mixture %lld)", (long long)(i / ((size_t)iv->D * iv->R)));
    hipStream_t s = iv->ctx->stream;
    SSP_HIP(hipMemcpyAsync(iv->T64.p, T, n * sizeof(double), hipMemcpyHostToDevice, s));
    IvPackArgs a{iv->T64.as<double>(), iv->icv.as<double>(), iv->P.as<float>(), iv->G.as<float>(), iv->K, iv->D, iv->R, iv->tri};
    const int cells = std::max(iv->tri, iv->D * iv->R);
    hipLaunchKernelGGL(iv_pack_kernel, dim3((unsigned)ceil_div(cells, 256), (unsigned)iv->K), dim3(256), 0, s, a);
    SSP_HIP(hipGetLastError());
    SSP_HIP(hipStreamSynchronize(s));
    return SSP_OK;
}

// one call of either kind.  estep: A_out / C_out / objective_out; else w_out / logdet_out / quad_out
static int iv_run(ssp_ivector* iv, const char* fn, const double* nk, const double* sx, int64_t U, bool estep, float* w_out, float* logdet_out,
                  float* quad_out, double* A_out, double* C_out, double* objective_out, float* kernel_ms) {
    if (!iv) SSP_FAIL(SSP_ERR_INVALID, "%s: null handle", fn);
    if (U < 1) SSP_FAIL(SSP_ERR_INVALID, "%s: U=%lld: at least one utterance", fn, (long long)U);
    if (!nk || !sx) SSP_FAIL(SSP_ERR_INVALID, "%s: null statistics", fn);
    if (estep ? (!A_out || !C_out) : !w_out) SSP_FAIL(SSP_ERR_INVALID, "%s: null output", fn);
    ssp_ctx* ctx = iv->ctx;
    SSP_TRY(use_ctx(ctx));
    hipStream_t s = ctx->stream;
    if (kernel_ms) *kernel_ms = 0.f;
    for (float& v : iv->stage_ms) v = 0.f;
    const int K = iv->K, D = iv->D, R = iv->R, tri = iv->tri;
    const size_t KD = (size_t)K * D;
    // a GEMM whose sum over k is more than one chain writes its chunks first: K > IV_KC for Lp, K D > IV_KC for b
    const size_t zl = (size_t)iv_chunks(K), zb = (size_t)iv_chunks((int64_t)KD);
    const size_t part_utt = std::max(zl > 1 ? zl * tri : 0, zb > 1 ? zb * R : 0);
    const size_t per_utt = sizeof(float) * ((size_t)tri + K + KD + 2 * (size_t)R + 2 + part_utt) + sizeof(double);
    const int64_t slab = std::min<int64_t>(U, std::max<int64_t>(1, (int64_t)(iv->cap / per_utt)));
    if (ceil_div<int64_t>(slab, 64) > 65535) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: a slab of %lld utterances (lower the workspace cap)", fn, (long long)slab);
    iv->last_slab = slab;
    SSP_TRY(iv->nk.reserve((size_t)slab * K * sizeof(float)));
    SSP_TRY(iv->f.reserve((size_t)slab * KD * sizeof(float)));
    SSP_TRY(iv->Lp.reserve((size_t)slab * tri * sizeof(float)));
    SSP_TRY(iv->b.reserve((size_t)slab * R * sizeof(float)));
    SSP_TRY(iv->w.reserve((size_t)slab * R * sizeof(float)));
    SSP_TRY(iv->ld.reserve((size_t)slab * sizeof(float)));
    SSP_TRY(iv->qd.reserve((size_t)slab * sizeof(float)));
    SSP_TRY(iv->obj.reserve((size_t)slab * sizeof(double)));
    const size_t nA = (size_t)K * tri, nC = KD * R;
    size_t part_elems = (size_t)slab * part_utt;
    if (estep) {
        part_elems = std::max(part_elems, (size_t)iv_chunks(slab) * std::max(nA, nC));
        SSP_TRY(iv->Aacc.reserve(nA * sizeof(double)));
        SSP_TRY(iv->Cacc.reserve(nC * sizeof(double)));
    }
    SSP_TRY(iv->part.reserve(part_elems * sizeof(float)));
    const size_t lds = iv_chol_lds(tri);
    if (lds > 64 * 1024)
        SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(iv_chol_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (kernel_ms)
        for (hipEvent_t& e : iv->ev)
            if (!e) SSP_HIP(hipEventCreate(&e));
    std::vector<float> hnk((size_t)slab * K), hf((size_t)slab * KD), hw, hld((size_t)slab), hqd((size_t)slab);
    std::vector<double> hobj((size_t)slab);
    if (!estep) hw.resize((size_t)slab * R);
    std::vector<char> bad((size_t)U, 0);
    bool any_bad = false;
    double objective = 0.0;
    const float nanf_ = std::nanf("");
    for (int64_t u0 = 0; u0 < U; u0 += slab) {
        const int64_t n = std::min<int64_t>(slab, U - u0);
        // centred statistics in float64, rounded once; an utterance with a non-finite entry runs as zeros and is answered as NaN below
        auto centre = [&](int64_t i) {
            const double* nu = nk + (size_t)(u0 + i) * K;
            const double* su = sx + (size_t)(u0 + i) * KD;
            float* fo = hf.data() + (size_t)i * KD;
            float* no = hnk.data() + (size_t)i * K;
            bool ok = true;
            for (int k = 0; k < K; ++k) {
                const double c = nu[k];
                no[k] = (float)c;
                ok = ok && std::isfinite(no[k]);  // (the rounded value: finite in float64 but too large for fp32 is bad too)
                const double* m = iv->mu.data() + (size_t)k * D;
                for (int d = 0; d < D; ++d) {
                    const float v = (float)(su[(size_t)k * D + d] - c * m[d]);
                    ok = ok && std::isfinite(v);
                    fo[(size_t)k * D + d] = v;
                }
            }
            if (!ok) {
                bad[(size_t)(u0 + i)] = 1;
                std::memset(fo, 0, KD * sizeof(float));
                std::memset(no, 0, (size_t)K * sizeof(float));
            }
        };
        // (a pass over U K D doubles: a large slab is split over a few host threads, utterance by utterance)
        const int nth = (size_t)n * KD < ((size_t)1 << 22) ? 1 : (int)std::min<int64_t>(n, std::min(16u, std::max(1u, std::thread::hardware_concurrency())));
        if (nth == 1) {
            for (int64_t i = 0; i < n; ++i) centre(i);
        } else {
            std::vector<std::thread> pool;
            for (int t = 0; t < nth; ++t)
                pool.emplace_back([&, t] {
                    for (int64_t i = t; i < n; i += nth) centre(i);
                });
            for (std::thread& t : pool) t.join();
        }
        for (int64_t i = 0; i < n; ++i) any_bad = any_bad || bad[(size_t)(u0 + i)] != 0;
        SSP_HIP(hipMemcpyAsync(iv->nk.p, hnk.data(), (size_t)n * K * sizeof(float), hipMemcpyHostToDevice, s));
        SSP_HIP(hipMemcpyAsync(iv->f.p, hf.data(), (size_t)n * KD * sizeof(float), hipMemcpyHostToDevice, s));
        int e = 0;
        if (kernel_ms) SSP_HIP(hipEventRecord(iv->ev[e++], s));
        iv_gemm_f32(s, iv->nk.as<float>(), iv->P.as<float>(), iv->Lp.as<float>(), iv->part.as<float>(), n, tri, K);
        if (kernel_ms) SSP_HIP(hipEventRecord(iv->ev[e++], s));
        iv_gemm_f32(s, iv->f.as<float>(), iv->G.as<float>(), iv->b.as<float>(), iv->part.as<float>(), n, R, (int64_t)KD);
        if (kernel_ms) SSP_HIP(hipEventRecord(iv->ev[e++], s));
        IvCholArgs c{iv->Lp.as<float>(), iv->b.as<float>(), iv->w.as<float>(), iv->ld.as<float>(), iv->qd.as<float>(), iv->obj.as<double>(), R, tri,
                     estep ? 1 : 0};
        hipLaunchKernelGGL(iv_chol_kernel, dim3((unsigned)n), dim3(256), lds, s, c);
        if (kernel_ms) SSP_HIP(hipEventRecord(iv->ev[e++], s));
        if (estep) {
            iv_gemm_acc(s, iv->nk.as<float>(), iv->Lp.as<float>(), iv->Aacc.as<double>(), iv->part.as<float>(), K, tri, n, u0 == 0);
            if (kernel_ms) SSP_HIP(hipEventRecord(iv->ev[e++], s));
            iv_gemm_acc(s, iv->f.as<float>(), iv->w.as<float>(), iv->Cacc.as<double>(), iv->part.as<float>(), (int64_t)KD, R, n, u0 == 0);
            if (kernel_ms) SSP_HIP(hipEventRecord(iv->ev[e++], s));
        }
        if (hipGetLastError() != hipSuccess) {
            (void)hipStreamSynchronize(s);
            SSP_FAIL(SSP_ERR_HIP, "%s: kernel launch failed", fn);
        }
        if (estep) {
            SSP_HIP(hipMemcpyAsync(hobj.data(), iv->obj.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
        } else {
            SSP_HIP(hipMemcpyAsync(hw.data(), iv->w.p, (size_t)n * R * sizeof(float), hipMemcpyDeviceToHost, s));
            SSP_HIP(hipMemcpyAsync(hld.data(), iv->ld.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
            SSP_HIP(hipMemcpyAsync(hqd.data(), iv->qd.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
        }
        SSP_HIP(hipStreamSynchronize(s));  // (the host buffers are filled again for the next slab)
        if (kernel_ms)
            for (int i = 0; i + 1 < e; ++i) {
                float ms = 0.f;
                SSP_HIP(hipEventElapsedTime(&ms, iv->ev[i], iv->ev[i + 1]));
                iv->stage_ms[i] += ms;
                *kernel_ms += ms;
            }
        if (estep) {
            for (int64_t i = 0; i < n; ++i) objective += hobj[(size_t)i];
        } else {
            for (int64_t i = 0; i < n; ++i) {
                const bool nb = bad[(size_t)(u0 + i)] != 0;
                float* wo = w_out + (size_t)(u0 + i) * R;
                if (nb)
                    for (int r = 0; r < R; ++r) wo[r] = nanf_;
                else
                    std::memcpy(wo, hw.data() + (size_t)i * R, (size_t)R * sizeof(float));
                if (logdet_out) logdet_out[u0 + i] = nb ? nanf_ : hld[(size_t)i];
                if (quad_out) quad_out[u0 + i] = nb ? nanf_ : hqd[(size_t)i];
            }
        }
    }
    if (!estep) return SSP_OK;
    const double nand = std::nan("");
    if (any_bad) {
        for (size_t i = 0; i < (size_t)K * R * R; ++i) A_out[i] = nand;
        for (size_t i = 0; i < nC; ++i) C_out[i] = nand;
        if (objective_out) *objective_out = nand;
        return SSP_OK;
    }
    std::vector<double> hA(nA);
    SSP_HIP(hipMemcpyAsync(hA.data(), iv->Aacc.p, nA * sizeof(double), hipMemcpyDeviceToHost, s));
    SSP_HIP(hipMemcpyAsync(C_out, iv->Cacc.p, nC * sizeof(double), hipMemcpyDeviceToHost, s));
    SSP_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < K; ++k) {
        const double* t = hA.data() + (size_t)k * tri;
        double* o = A_out + (size_t)k * R * R;
        for (int i = 0; i < R; ++i)
            for (int j = 0; j <= i; ++j) o[(size_t)i * R + j] = o[(size_t)j * R + i] = t[(size_t)i * (i + 1) / 2 + j];
    }
    if (objective_out) *objective_out = objective;
    return SSP_OK;
}

extern "C" {

int ssp_ivector_create(ssp_ctx* ctx, int32_t K, int32_t D, int32_t R, const double* ubm_means, const double* ubm_covars, const double* T,
                       ssp_ivector** out) try {
    ssp::TraceRange trace_("ssp_ivector_create");
    if (!out) SSP_FAIL(SSP_ERR_INVALID, "ssp_ivector_create: null out");
    *out = nullptr;
    if (!ctx) SSP_FAIL(SSP_ERR_INVALID, "null ssp_ctx");
    if (K < 1 || D < 1 || R < 1 || !ubm_means || !ubm_covars || !T) SSP_FAIL(SSP_ERR_INVALID, "ssp_ivector_create: bad shape or null parameter array");
    if (R > IV_RMAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_ivector_create: R=%d exceeds the supported rank (%d)", R, IV_RMAX);
    if (K > 65535) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_ivector_create: K=%d exceeds the supported 65535 mixtures", K);
    if ((int64_t)D * R > INT32_MAX / 2 || (int64_t)K * D > INT32_MAX / 2) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_ivector_create: K x D or D x R too large");
    const size_t KD = (size_t)K * D;
    std::vector<double> icv(KD);
    for (size_t i = 0; i < KD; ++i) {
        if (!(ubm_covars[i] > 0.0) || !std::isfinite(ubm_covars[i]))
            SSP_FAIL(SSP_ERR_INVALID, "ssp_ivector_create: non-positive or non-finite covariance (mix %lld)", (long long)(i / D));
        if (!std::isfinite(ubm_means[i])) SSP_FAIL(SSP_ERR_INVALID, "ssp_ivector_create: non-finite mean (mix %lld)", (long long)(i / D));
        icv[i] = 1.0 / ubm_covars[i];
    }
    for (size_t i = 0; i < KD * R; ++i)
        if (!std::isfinite(T[i])) SSP_FAIL(SSP_ERR_INVALID, "ssp_ivector_create: non-finite entry in T (mixture %lld)", (long long)(i / ((size_t)D * R)));
    SSP_TRY(use_ctx(ctx));
    HandleBuild<ssp_ivector> iv(ctx, "ssp_ivector_create");
    iv->K = K;
    iv->D = D;
    iv->R = R;
    iv->tri = R * (R + 1) / 2;
    iv->mu.assign(ubm_means, ubm_means + KD);
    int rc = iv->T64.alloc(KD * R * sizeof(double));
    if (rc == SSP_OK) rc = upload(iv, iv->icv, icv);
    if (rc == SSP_OK) rc = iv->P.alloc((size_t)K * iv->tri * sizeof(float));
    if (rc == SSP_OK) rc = iv->G.alloc(KD * R * sizeof(float));
    if (rc == SSP_OK) rc = iv_upload_T(iv.get(), T);
    if (rc == SSP_OK) iv.waited();  // (iv_upload_T ends in the create's one host wait)
    return iv.commit(rc, out);
}
SSP_CREATE_GUARD("ssp_ivector_create")

int ssp_ivector_destroy(ssp_ivector* iv) { return destroy_handle(iv); }

int ssp_ivector_set_t(ssp_ivector* iv, const double* T) {
    ssp::TraceRange trace_("ssp_ivector_set_t");
    if (!iv || !T) SSP_FAIL(SSP_ERR_INVALID, "ssp_ivector_set_t: null argument");
    SSP_TRY(use_ctx(iv->ctx));
    return iv_upload_T(iv, T);
}

int ssp_ivector_set_workspace(ssp_ivector* iv, size_t bytes) {
    if (!iv) SSP_FAIL(SSP_ERR_INVALID, "ssp_ivector_set_workspace: null handle");
    iv->cap = bytes;
    return SSP_OK;
}

int ssp_ivector_last_slab(const ssp_ivector* iv, int64_t* utterances) {
    if (!iv || !utterances) SSP_FAIL(SSP_ERR_INVALID, "ssp_ivector_last_slab: null argument");
    *utterances = iv->last_slab;
    return SSP_OK;
}

int ssp_ivector_last_stages(const ssp_ivector* iv, float* ms) {
    if (!iv || !ms) SSP_FAIL(SSP_ERR_INVALID, "ssp_ivector_last_stages: null argument");
    for (int i = 0; i < IV_STAGES; ++i) ms[i] = iv->stage_ms[i];
    return SSP_OK;
}

int ssp_ivector_extract(ssp_ivector* iv, const double* nk, const double* sx, int64_t U, float* w_out, float* logdet_out, float* quad_out,
                        float* kernel_ms) {
    ssp::TraceRange trace_("ssp_ivector_extract");
    return iv_run(iv, "ssp_ivector_extract", nk, sx, U, false, w_out, logdet_out, quad_out, nullptr, nullptr, nullptr, kernel_ms);
}

int ssp_ivector_estep(ssp_ivector* iv, const double* nk, const double* sx, int64_t U, double* A_out, double* C_out, double* objective_out,
                      float* kernel_ms) {
    ssp::TraceRange trace_("ssp_ivector_estep");
    return iv_run(iv, "ssp_ivector_estep", nk, sx, U, true, nullptr, nullptr, nullptr, A_out, C_out, objective_out, kernel_ms);
}

}  // extern "C"
