// PLDA back end on gfx950 (ssp_plda_*): class statistics for the EM, and the log-likelihood-ratio sweep of a diagonalised two-covariance
// model against enrolled speakers.  An extension: the reference has no back end; sidekit and Kaldi ship this chain (Ioffe 2006, Prince &
// Elder 2007, Sizov et al. 2014; Kaldi's PldaEstimator).  include/ssp.h has the definitions.  Everything on the device is fp32 with
// exact-fp32 MFMA, sums that feed the EM are float64.
// Kernels:
//   plda_label_kernel   raises a flag for a label outside [0, S) (an int store of the same value from every finder)
//   plda_sum_kernel     one workgroup per class: its rows, IN ROW ORDER, into float64 sums (centroid_kernel's scan of the label array),
//                       the count, and the class mean sum / count in float64
//   plda_centre_kernel  Xc = fp32(x - m_class) for one slab of rows, formed in float64 and rounded once
//   plda_gram_kernel    the chunks of Xc' Xc on v_mfma_f32_32x32x2_f32: a chunk is 1024 rows and ONE k-ordered fma chain per output
//                       (grid z); a workgroup of four waves owns 64 x 64 outputs, only blocks on or below the diagonal are computed;
//                       k-major panels of 16 rows go through LDS, the next panel's global loads fly in registers under the MFMAs
//   plda_accum_kernel   float64 S_w (+)= the chunks of one slab, in ascending order
//   plda_score_kernel   the sweep, cosine_reg_kernel's shape: a wave keeps its 32 test vectors in registers as the MFMA B operand,
//                       packed 32-speaker tiles of beta stream through a ring of three half-tile LDS slots by LDS-DMA, one k-ordered
//                       chain per output; the epilogue adds c_s and keeps a running (max, first index).  The t^2 term: SHARED — one
//                       tile of the G <= 32 class rows of -alpha / 2 against the squared operand (squared on the fly) first, parked in
//                       a per-wave 32 x 32 LDS table that every speaker row's epilogue reads at its class; general — every beta tile
//                       is followed by its -alpha / 2 tile against the squared operand into the same accumulator.
// No floating-point atomic exists here and every sum has a fixed shape: same bits every call.
#include <algorithm>
#include <cmath>
#include <map>

#include "common.hpp"
#include "handle.hpp"
#include "reg_sweep.hpp"  // the operand staging and the LDS-DMA that this sweep shares with cosine_reg_kernel

namespace ssp {

constexpr int PL_QMAX = 256;        // largest dimension: the test vectors of a wave stay in 128 registers per lane
constexpr int PL_BK = 16;           // k per staged panel of the scatter GEMM
constexpr int PL_KC = 1024;         // rows per fma chain of the scatter GEMM
constexpr int PL_SLAB_CHUNKS = 64;  // chunks per launch of the scatter GEMM: the centred rows and the chunk images of one slab are resident
constexpr int PL_SCAN = 8;          // 256-row slices per scan batch of the class sums

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
__global__ __launch_bounds__(256) void plda_label_kernel(const int32_t* __restrict__ labels, int64_t N, int S, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N && (labels[i] < 0 || labels[i] >= S)) *flag = 1;
}

// sums [S x q] float64, counts [S], means [S x q] float64 (zero for a class without rows); q <= 256: thread = column
__global__ __launch_bounds__(256) void plda_sum_kernel(const float* __restrict__ X, const int32_t* __restrict__ labels, int64_t N, int q,
                                                       double* __restrict__ sums, long long* __restrict__ counts, double* __restrict__ means) {
    __shared__ int32_t list[256 * PL_SCAN];  // row offsets (relative to the batch base) of this class, in row order
    __shared__ int32_t wcnt[PL_SCAN][4];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc = 0.0;
    long long cnt = 0;
    for (int64_t base = 0; base < N; base += 256 * PL_SCAN) {
        int32_t lab[PL_SCAN];
#pragma unroll
        for (int k = 0; k < PL_SCAN; ++k) {
            const int64_t r = base + 256 * k + tid;
            lab[k] = r < N ? labels[r] : -1;
        }
        unsigned long long bal[PL_SCAN];
#pragma unroll
        for (int k = 0; k < PL_SCAN; ++k) {
            bal[k] = __ballot(lab[k] == s);
            if (lane == 0) wcnt[k][wave] = __popcll(bal[k]);
        }
        __syncthreads();
        int total = 0;
#pragma unroll
        for (int k = 0; k < PL_SCAN; ++k) {
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int c = wcnt[k][w];
                before += w < wave ? c : 0;
                all += c;
            }
            if (lab[k] == s) list[total + before + __popcll(bal[k] & ((1ull << lane) - 1ull))] = 256 * k + tid;
            total += all;
        }
        __syncthreads();
        cnt += total;
        if (tid < q) {
            const float* __restrict__ xb = X + base * q + tid;
            int j = 0;
            for (; j + 3 < total; j += 4) {
                const float v0 = xb[(size_t)list[j] * q], v1 = xb[(size_t)list[j + 1] * q], v2 = xb[(size_t)list[j + 2] * q],
                            v3 = xb[(size_t)list[j + 3] * q];
                acc += (double)v0;
                acc += (double)v1;
                acc += (double)v2;
                acc += (double)v3;
            }
            for (; j < total; ++j) acc += (double)xb[(size_t)list[j] * q];
        }
        __syncthreads();  // the list is rewritten by the next batch
    }
    if (tid < q) {
        sums[(size_t)s * q + tid] = acc;
        means[(size_t)s * q + tid] = cnt > 0 ? acc / (double)cnt : 0.0;
    }
    if (tid == 0) counts[s] = cnt;
}

// Xc[i - r0] = fp32(x_i - m_{label i}) for rows [r0, r0 + n); a row whose label is out of range (the call then fails) is written as zeros
__global__ __launch_bounds__(256) void plda_centre_kernel(const float* __restrict__ X, const int32_t* __restrict__ labels, const double* __restrict__ means,
                                                          int64_t r0, int64_t n, int q, int S, float* __restrict__ Xc) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * q) return;
    const int64_t i = e / q;
    const int c = (int)(e - i * q);
    const int l = labels[r0 + i];
    Xc[e] = (l >= 0 && l < S) ? (float)((double)X[(r0 + i) * q + c] - means[(size_t)l * q + c]) : 0.f;
}

// part[z][q x q] (blocks on or below the diagonal only) = sum over the rows k of chunk z of Xc[k][i] Xc[k][j]
__global__ __launch_bounds__(256) void plda_gram_kernel(const float* __restrict__ Xc, int64_t n, int q, float* __restrict__ part) {
    constexpr int BM = 64, LA = BM + 4;
    __shared__ float As[PL_BK * LA];
    __shared__ float Bs[PL_BK * LA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5, wr = wave >> 1, wc = wave & 1;
    int bi = 0, rest = blockIdx.x;  // block pair (bi, bj <= bi): blockIdx.x = bi (bi + 1) / 2 + bj
    while (rest > bi) {
        rest -= bi + 1;
        ++bi;
    }
    const int m0 = bi * BM, n0 = rest * BM;
    const int64_t kbeg = (int64_t)blockIdx.z * PL_KC, kend = min(n, kbeg + (int64_t)PL_KC);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // this thread's four cells of a panel: row e / 64 of the panel, column e % 64 of the block
    float ra[4], rb[4];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int e = s * 256 + tid, k = e >> 6, m = e & 63;
            const bool in = k0 + k < kend;
            ra[s] = (in && m0 + m < q) ? Xc[(k0 + k) * q + m0 + m] : 0.f;
            rb[s] = (in && n0 + m < q) ? Xc[(k0 + k) * q + n0 + m] : 0.f;
        }
    };
    fetch(kbeg);
    for (int64_t k0 = kbeg; k0 < kend; k0 += PL_BK) {
        __syncthreads();  // the previous panel's MFMAs are done with As and Bs
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int e = s * 256 + tid;
            As[(e >> 6) * LA + (e & 63)] = ra[s];
            Bs[(e >> 6) * LA + (e & 63)] = rb[s];
        }
        __syncthreads();
        if (k0 + PL_BK < kend) fetch(k0 + PL_BK);  // the next panel's loads fly under this panel's MFMAs
#pragma unroll
        for (int kk = 0; kk < PL_BK; kk += 2) {
            const float av = As[(kk + lh) * LA + wr * 32 + li];
            const float bv = Bs[(kk + lh) * LA + wc * 32 + li];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
    }
    // accumulator r: row (r & 3) + 8 (r >> 2) + 4 lh, column li
    float* C = part + (size_t)blockIdx.z * (size_t)q * (size_t)q;
    const int gn = n0 + wc * 32 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gm = m0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (gm < q && gn < q) C[(size_t)gm * q + gn] = acc[r];
    }
}

// acc[i][j] (+)= the chunks of one slab in ascending order, for the cells the scatter GEMM computes (64 x 64 blocks on or below the
// diagonal); the others are zero and the host mirrors the lower triangle
__global__ __launch_bounds__(256) void plda_accum_kernel(double* __restrict__ acc, const float* __restrict__ part, int q, int chunks, int first) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= q * q) return;
    const int i = e / q, j = e - i * q;
    if ((j >> 6) > (i >> 6)) {
        acc[e] = 0.0;
        return;
    }
    double v = first ? 0.0 : acc[e];
    for (int z = 0; z < chunks; ++z) v += (double)part[(size_t)z * q * q + e];
    acc[e] = v;
}

// x * x where it is used: the squares of the resident operand are loop invariants, and hoisted they would double its 128 registers.
// The MFMA that follows reads y as an operand: a VALU write needs two wait states before that read, and the compiler pads nothing it
// cannot see inside the string.
__device__ __forceinline__ float pl_square(float x) {
    float y;
    asm volatile("v_mul_f32 %0, %1, %1\n\ts_nop 1" : "=v"(y) : "v"(x));
    return y;
}

struct PldaScoreArgs {
    const float* T;      // [N x q]
    const float* img;    // the stream of 32-row tile images, [NQ x 256] floats each ([q8][h][row 32][e 4] = v[row][8 q8 + 2 e + h], zero padded)
    const float* c;      // [n_tiles x 32]
    const int32_t* cls;  // [n_tiles x 32] class of every speaker (SHARED)
    float* llr;          // [N x S], nullable
    int32_t* argmax;     // nullable
    float* maxv;         // nullable
    int64_t N;
    int32_t q, S, n_tiles;
};

// SHARED: the stream is [class tile][beta tile 0][beta tile 1] ...; else [beta tile 0][-alpha/2 tile 0][beta tile 1][-alpha/2 tile 1] ...
template <int NQ, bool SHARED>
__global__ __launch_bounds__(256, 2) void plda_score_kernel(PldaScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) char pl_smem[];
    constexpr int TILE_FLOATS = NQ * 256, HALF = TILE_FLOATS / 2;
    constexpr int RING_FLOATS = 3 * HALF > 4 * SWEEP_XS_FLOATS ? 3 * HALF : 4 * SWEEP_XS_FLOATS;
    float* wbuf = reinterpret_cast<float*>(pl_smem);  // [3][HALF]; the first bytes double as the staging area of the test vectors
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* tab = wbuf + RING_FLOATS + wave * 1024;     // SHARED: this wave's [class 32][column 32] table of the t^2 term
    const int fl = lane & 31, h = lane >> 5;
    const int d = a.q;
    const int64_t col0 = (int64_t)blockIdx.x * 128 + wave * 32;  // this wave's 32 test vectors
    const int64_t Nn = a.N;

    // ---- B operand: b[q8][e] = t[col][8 q8 + 2 e + h] (reg_sweep.hpp); a non-finite entry flags the column on the way
    float b[NQ][4];
    bool bad = false;
    sweep_load_operand<NQ>(
        b, wbuf + wave * SWEEP_XS_FLOATS, lane, d,
        [&](int r) -> const float* {
            const int64_t row = col0 + r;
            return row < Nn ? a.T + row * d : nullptr;
        },
        [&](float v) { bad = bad || !(fabsf(v) < INFINITY); });
    const int other_bad = __shfl_xor((int)bad, 32);  // the other k half of this column (every lane takes part: no short circuit)
    bad = bad || other_bad != 0;
    __syncthreads();  // the staging area is about to be overwritten by the first tile

    const int n_stream = __builtin_amdgcn_readfirstlane(SHARED ? a.n_tiles + 1 : 2 * a.n_tiles);  // tiles of the stream, two half-steps each
    const int n_steps = 2 * n_stream;
    auto stage = [&](int step, int slot) { sweep_stage_half<NQ>(a.img + (size_t)step * HALF, wbuf + slot * HALF, wave, lane); };
    stage(0, 0);
    stage(1, 1);
    __syncthreads();

    float best = -INFINITY;
    int besti = 0x7fffffff;
    const int64_t gc = col0 + fl;
    const float nanv = __builtin_nanf("");
    int slot = 0;  // slot of half-step 2 t
    f32x16 acc;
    for (int t = 0; t < n_stream; ++t) {
        const int s1 = slot == 2 ? 0 : slot + 1, s2 = s1 == 2 ? 0 : s1 + 1;
        const bool sq = SHARED ? t == 0 : (t & 1) != 0;  // this tile multiplies the squared operand
        if (SHARED || !sq) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        }
        // ---- first k half
        if (2 * t + 2 < n_steps) stage(2 * t + 2, s2);
        {
            const float* wcur = wbuf + slot * HALF;
            if (sq) {
#pragma unroll
                for (int q8 = 0; q8 < NQ / 2; ++q8) {
                    const f32x4 a4 = *reinterpret_cast<const f32x4*>(wcur + ((q8 * 2 + h) * 32 + fl) * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], pl_square(b[q8][e]), acc, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int q8 = 0; q8 < NQ / 2; ++q8) {
                    const f32x4 a4 = *reinterpret_cast<const f32x4*>(wcur + ((q8 * 2 + h) * 32 + fl) * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], b[q8][e], acc, 0, 0, 0);
                }
            }
        }
        __syncthreads();
        // ---- second k half
        if (2 * t + 3 < n_steps) stage(2 * t + 3, slot);
        {
            const float* wcur = wbuf + s1 * HALF;
            if (sq) {
#pragma unroll
                for (int q8 = 0; q8 < NQ / 2; ++q8) {
                    const f32x4 a4 = *reinterpret_cast<const f32x4*>(wcur + ((q8 * 2 + h) * 32 + fl) * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], pl_square(b[NQ / 2 + q8][e]), acc, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int q8 = 0; q8 < NQ / 2; ++q8) {
                    const f32x4 a4 = *reinterpret_cast<const f32x4*>(wcur + ((q8 * 2 + h) * 32 + fl) * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], b[NQ / 2 + q8][e], acc, 0, 0, 0);
                }
            }
        }
        // accumulator i: row (i & 3) + 8 (i >> 2) + 4 h of the tile, column fl
        if (SHARED && t == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) tab[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + fl] = acc[i];
        } else if (SHARED || sq) {
            const int st = SHARED ? t - 1 : t >> 1;  // the speaker tile this accumulator now holds
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) {
                const int row0 = st * 32 + 8 * i4 + 4 * h;
                const float4 c4 = *reinterpret_cast<const float4*>(a.c + row0);
                int4 g4 = make_int4(0, 0, 0, 0);
                if (SHARED) g4 = *reinterpret_cast<const int4*>(a.cls + row0);
                const float cc[4] = {c4.x, c4.y, c4.z, c4.w};
                const int gg[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = row0 + e;
                    if (row < a.S) {
                        float v = acc[i4 * 4 + e];
                        if (SHARED) v += tab[gg[e] * 32 + fl];
                        v += cc[e];
                        if (bad) v = nanv;
                        if (a.llr && gc < Nn) a.llr[gc * a.S + row] = v;
                        if (v > best || (v == best && row < besti)) {
                            best = v;
                            besti = row;
                        }
                    }
                }
            }
        }
        __syncthreads();
        slot = s2;
    }
    const float ob = __shfl_xor(best, 32);
    const int oi = __shfl_xor(besti, 32);
    if (ob > best || (ob == best && oi < besti)) {
        best = ob;
        besti = oi;
    }
    if (h == 0 && gc < Nn) {
        const bool none = besti == 0x7fffffff;  // a non-finite test vector, or every ratio NaN
        if (a.argmax) a.argmax[gc] = none ? -1 : besti;
        if (a.maxv) a.maxv[gc] = none ? nanv : best;
    }
}

template <int NQ, bool SHARED>
static size_t plda_score_lds() {
    const size_t ring = (size_t)3 * NQ * 128 * sizeof(float), xst = (size_t)4 * SWEEP_XS_FLOATS * sizeof(float);
    return std::max(ring, xst) + (SHARED ? (size_t)4 * 1024 * sizeof(float) : 0);
}

template <int NQ, bool SHARED>
static int launch_plda_score(const PldaScoreArgs& a, hipStream_t s) {
    const size_t lds = plda_score_lds<NQ, SHARED>();
    const int64_t grid = ceil_div<int64_t>(a.N, 128);
    if (grid > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_plda_score: too many test vectors for one launch");
    hipLaunchKernelGGL((plda_score_kernel<NQ, SHARED>), dim3((unsigned)grid), dim3(256), lds, s, a);
    SSP_HIP(hipGetLastError());
    return SSP_OK;
}

template <bool SHARED>
static int launch_plda_score_nq(int nq, const PldaScoreArgs& a, hipStream_t s) {
    switch (nq) {
        case 8: return launch_plda_score<8, SHARED>(a, s);
        case 16: return launch_plda_score<16, SHARED>(a, s);
        case 24: return launch_plda_score<24, SHARED>(a, s);
        default: return launch_plda_score<32, SHARED>(a, s);
    }
}

}  // namespace ssp

struct ssp_plda {
    ssp_ctx* ctx = nullptr;
    int32_t q = 0, S = 0, nq = 0, n_tiles = 0, G = 0;
    bool shared = false;
    ssp::DevBuf img, c, cls;
};

using namespace ssp;

extern "C" {

int ssp_plda_stats(ssp_ctx* ctx, const float* X, const int32_t* labels, int64_t N, int32_t q, int32_t S, double* sum_out, int64_t* count_out,
                   double* mean_out, double* sw_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_plda_stats");
    SSP_TRY(use_ctx(ctx));
    if (N < 1 || q < 1 || S < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_plda_stats: bad shape (N=%lld, q=%d, S=%d)", (long long)N, q, S);
    if (q > PL_QMAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_plda_stats: q=%d exceeds the supported dimension (%d)", q, PL_QMAX);
    SSP_TRY(check_where(where, "ssp_plda_stats"));
    if (!X || !labels || !sum_out || !count_out || !mean_out || !sw_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_plda_stats: null pointer");
    if (ceil_div<int64_t>(N, 256) > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_plda_stats: too many rows");
    if (kernel_ms) *kernel_ms = 0.f;
    hipStream_t s = ctx->stream;
    StageScope st(ctx, where);
    const float* dX = st.in(X, (size_t)N * q * sizeof(float));
    const int32_t* dL = st.in(labels, (size_t)N * sizeof(int32_t));
    SSP_TRY(st.status());
    const size_t Sq = (size_t)S * q, qq = (size_t)q * q;
    const int64_t slab = std::min<int64_t>(N, (int64_t)PL_SLAB_CHUNKS * PL_KC);
    const int slab_chunks = (int)ceil_div<int64_t>(slab, PL_KC);
    DevBuf sums, means, counts, flag, xc, part, acc;
    SSP_TRY(sums.alloc(Sq * sizeof(double)));
    SSP_TRY(means.alloc(Sq * sizeof(double)));
    SSP_TRY(counts.alloc((size_t)S * sizeof(long long)));
    SSP_TRY(flag.alloc(sizeof(int32_t)));
    SSP_TRY(xc.alloc((size_t)slab * q * sizeof(float)));
    SSP_TRY(part.alloc((size_t)slab_chunks * qq * sizeof(float)));
    SSP_TRY(acc.alloc(qq * sizeof(double)));
    SSP_HIP(hipMemsetAsync(flag.p, 0, sizeof(int32_t), s));
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    hipLaunchKernelGGL(plda_label_kernel, dim3((unsigned)ceil_div<int64_t>(N, 256)), dim3(256), 0, s, dL, N, S, flag.as<int32_t>());
    hipLaunchKernelGGL(plda_sum_kernel, dim3((unsigned)S), dim3(256), 0, s, dX, dL, N, q, sums.as<double>(), counts.as<long long>(),
                       means.as<double>());
    const int nb = ceil_div(q, 64);
    for (int64_t r0 = 0; r0 < N; r0 += slab) {
        const int64_t n = std::min<int64_t>(slab, N - r0);
        const int chunks = (int)ceil_div<int64_t>(n, PL_KC);
        hipLaunchKernelGGL(plda_centre_kernel, dim3((unsigned)ceil_div<int64_t>(n * q, 256)), dim3(256), 0, s, dX, dL, means.as<double>(), r0, n, q, S,
                           xc.as<float>());
        hipLaunchKernelGGL(plda_gram_kernel, dim3((unsigned)(nb * (nb + 1) / 2), 1, (unsigned)chunks), dim3(256), 0, s, xc.as<float>(), n, q,
                           part.as<float>());
        hipLaunchKernelGGL(plda_accum_kernel, dim3((unsigned)ceil_div<size_t>(qq, 256)), dim3(256), 0, s, acc.as<double>(), part.as<float>(), q, chunks,
                           r0 == 0 ? 1 : 0);
    }
    if (hipGetLastError() != hipSuccess) {
        (void)hipStreamSynchronize(s);
        SSP_FAIL(SSP_ERR_HIP, "ssp_plda_stats: kernel launch failed");
    }
    SSP_TRY(tm.stop(s, kernel_ms));
    int32_t hflag = 0;
    std::vector<double> hsum(Sq), hacc(qq);
    std::vector<long long> hcnt((size_t)S);
    SSP_HIP(hipMemcpyAsync(&hflag, flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SSP_HIP(hipMemcpyAsync(hsum.data(), sums.p, Sq * sizeof(double), hipMemcpyDeviceToHost, s));
    SSP_HIP(hipMemcpyAsync(hcnt.data(), counts.p, (size_t)S * sizeof(long long), hipMemcpyDeviceToHost, s));
    SSP_HIP(hipMemcpyAsync(hacc.data(), acc.p, qq * sizeof(double), hipMemcpyDeviceToHost, s));
    SSP_HIP(hipStreamSynchronize(s));  // the one wait of the call
    if (hflag) SSP_FAIL(SSP_ERR_INVALID, "ssp_plda_stats: a label outside [0, %d)", S);
    std::memcpy(sum_out, hsum.data(), Sq * sizeof(double));
    for (int i = 0; i < S; ++i) count_out[i] = (int64_t)hcnt[(size_t)i];
    for (int c = 0; c < q; ++c) {
        double t = 0.0;
        for (int i = 0; i < S; ++i) t += hsum[(size_t)i * q + c];
        mean_out[c] = t / (double)N;
    }
    for (int i = 0; i < q; ++i)
        for (int j = 0; j <= i; ++j) sw_out[(size_t)i * q + j] = sw_out[(size_t)j * q + i] = hacc[(size_t)i * q + j];
    return SSP_OK;
}

int ssp_plda_pack(ssp_ctx* ctx, int32_t q, const double* psi, int32_t S, const double* enrol_mean, const int32_t* enrol_count, int32_t flags,
                  ssp_plda** out) try {
    ssp::TraceRange trace_("ssp_plda_pack");
    if (!out) SSP_FAIL(SSP_ERR_INVALID, "ssp_plda_pack: null out");
    *out = nullptr;
    // (the parameters first: a refusal needs no device)
    if (q < 1 || S < 1 || !psi || !enrol_mean || !enrol_count) SSP_FAIL(SSP_ERR_INVALID, "ssp_plda_pack: bad shape or null parameter array");
    if (q > PL_QMAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_plda_pack: q=%d exceeds the supported dimension (%d)", q, PL_QMAX);
    for (int d = 0; d < q; ++d)
        if (!std::isfinite(psi[d]) || psi[d] < 0.0) SSP_FAIL(SSP_ERR_INVALID, "ssp_plda_pack: psi[%d] is negative or not finite", d);
    for (int s = 0; s < S; ++s) {
        if (enrol_count[s] < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_plda_pack: speaker %d has an enrolment count below 1", s);
        for (int d = 0; d < q; ++d)
            if (!std::isfinite(enrol_mean[(size_t)s * q + d])) SSP_FAIL(SSP_ERR_INVALID, "ssp_plda_pack: non-finite enrolment mean (speaker %d)", s);
    }
    SSP_TRY(use_ctx(ctx));
    const int nq = q <= 64 ? 8 : (q <= 128 ? 16 : (q <= 192 ? 24 : 32));
    const int n_tiles = (S + 31) / 32;
    const size_t tile = (size_t)nq * 256;
    // classes of equal enrolment count, in order of first appearance
    std::map<int32_t, int32_t> cls_of;
    std::vector<int32_t> cls_count, cls((size_t)n_tiles * 32, 0);
    for (int s = 0; s < S; ++s) {
        auto it = cls_of.find(enrol_count[s]);
        if (it == cls_of.end()) {
            it = cls_of.emplace(enrol_count[s], (int32_t)cls_count.size()).first;
            cls_count.push_back(enrol_count[s]);
        }
        cls[(size_t)s] = it->second;
    }
    const int G = (int)cls_count.size();
    const bool shared = G <= 32 && !(flags & SSP_PLDA_NO_CLASS_PATH);
    auto at = [&](int row, int k) { return ((size_t)((k >> 3) * 2 + (k & 1)) * 32 + (size_t)(row & 31)) * 4 + (size_t)((k & 7) >> 1); };
    // -alpha / 2 of an enrolment count (float64, rounded once; the halving is exact)
    auto half_alpha = [&](int32_t n, int d) {
        const double var = 1.0 + psi[d] / ((double)n * psi[d] + 1.0);
        return (float)(-0.5 * (1.0 / var - 1.0 / (1.0 + psi[d])));
    };
    std::vector<float> img((size_t)(shared ? n_tiles + 1 : 2 * n_tiles) * tile, 0.f), cs((size_t)n_tiles * 32, 0.f);
    if (shared)
        for (int g = 0; g < G; ++g)
            for (int d = 0; d < q; ++d) img[at(g, d)] = half_alpha(cls_count[(size_t)g], d);
    for (int s = 0; s < S; ++s) {
        const double n = (double)enrol_count[s];
        float* bt = img.data() + (shared ? (size_t)(s / 32 + 1) : (size_t)(s / 32) * 2) * tile;
        double c = 0.0;
        for (int d = 0; d < q; ++d) {
            const double den = n * psi[d] + 1.0;
            const double mean = n * psi[d] * enrol_mean[(size_t)s * q + d] / den, var = 1.0 + psi[d] / den;
            bt[at(s, d)] = (float)(mean / var);
            if (!shared) bt[tile + at(s, d)] = half_alpha(enrol_count[s], d);
            c += std::log(var) - std::log1p(psi[d]) + mean * mean / var;
        }
        cs[(size_t)s] = (float)(-0.5 * c);
    }
    HandleBuild<ssp_plda> p(ctx, "ssp_plda_pack");
    p->q = q;
    p->S = S;
    p->nq = nq;
    p->n_tiles = n_tiles;
    p->G = G;
    p->shared = shared;
    int rc = upload(p, p->img, img);
    if (rc == SSP_OK) rc = upload(p, p->c, cs);
    if (rc == SSP_OK) rc = upload(p, p->cls, cls);
    return p.commit(rc, out);
}
SSP_CREATE_GUARD("ssp_plda_pack")

int ssp_plda_destroy(ssp_plda* p) { return destroy_handle(p); }

int ssp_plda_info(const ssp_plda* p, int32_t* n_classes, int32_t* class_shared) {
    if (!p || !n_classes || !class_shared) SSP_FAIL(SSP_ERR_INVALID, "ssp_plda_info: null argument");
    *n_classes = p->G;
    *class_shared = p->shared ? 1 : 0;
    return SSP_OK;
}

int ssp_plda_score(ssp_plda* p, const float* T, int64_t N, float* llr_out, int32_t* argmax_out, float* max_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_plda_score");
    if (!p) SSP_FAIL(SSP_ERR_INVALID, "ssp_plda_score: null handle");
    ssp_ctx* ctx = p->ctx;
    SSP_TRY(use_ctx(ctx));
    if (N < 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_plda_score: N=%lld", (long long)N);
    SSP_TRY(check_where(where, "ssp_plda_score"));
    if (N > 0 && !T) SSP_FAIL(SSP_ERR_INVALID, "ssp_plda_score: null test vectors");
    if (kernel_ms) *kernel_ms = 0.f;
    if (N == 0) return SSP_OK;
    StageScope st(ctx, where);
    const float* dT = st.in(T, (size_t)N * p->q * sizeof(float));
    float* dL = st.out(llr_out, (size_t)N * p->S * sizeof(float));
    int32_t* dA = st.out(argmax_out, (size_t)N * sizeof(int32_t));
    float* dM = st.out(max_out, (size_t)N * sizeof(float));
    SSP_TRY(st.status());
    PldaScoreArgs a{dT, p->img.as<float>(), p->c.as<float>(), p->cls.as<int32_t>(), dL, dA, dM, N, p->q, p->S, p->n_tiles};
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, ctx->stream));
    SSP_TRY(p->shared ? launch_plda_score_nq<true>(p->nq, a, ctx->stream) : launch_plda_score_nq<false>(p->nq, a, ctx->stream));
    SSP_TRY(tm.stop(ctx->stream, kernel_ms));
    return st.finish();
}

}  // extern "C"
