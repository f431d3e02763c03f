// Speaker diarization on gfx950 (ssp_pairwise_size, ssp_pairwise_scores, ssp_ahc_cluster): the scores of all window pairs of a recording
// and agglomerative hierarchical clustering of them, batched over recordings.  An extension: the reference has no diarization; Kaldi's
// diarization/ recipe, sidekit, SpeechBrain and wespeaker ship this chain.  include/ssp.h has the definitions, tests/diarize_oracle.py
// restates them.  Everything is fp32 and no operation is contracted, except the row terms r_i, which are summed in float64 and rounded once.
// Kernels:
//   diar_rowstat_kernel  one wave per row: r_i = sum_d h_d x_id^2 (float64, lane l adds entries l, l + 64, ... then a butterfly), NaN for a
//                        row with a non-finite entry (which carries the NaN-row rule through the epilogue's r_i + r_j)
//   diar_pair_kernel     one workgroup per 64 x 64 block of pairs on or above the diagonal of a recording, four waves, one 32 x 32 tile
//                        each on v_mfma_f32_32x32x2_f32 (the tile below the diagonal of a diagonal block is not computed); q is walked in
//                        panels of 32 through LDS ([row][33]: the MFMA operand reads of 32 rows are conflict-free), the next panel's
//                        loads fly under this panel's MFMAs; one k-ordered chain per output, ascending d; g scales the A operand.  The
//                        epilogue writes out[i][j] and out[j][i] from the one value computed for i <= j: exact symmetry, no atomics.
//   diar_ahc_kernel      one 256-thread workgroup per recording, longest first.  The working copy (symmetric, odd row stride) sits in
//                        LDS (n <= DZ_N_LDS) or in the ctx's workspace.  Per row a best (key, column) over the live columns j > i is kept
//                        in LDS; the arg-max of a merge is ONE 64-bit integer max over (key << 32 | ~row).  After a merge: row a and the
//                        rows whose best pointed at a or b are rescanned (a list in LDS, one wave per row), every other row i < a compares
//                        its one changed entry (an equal entry wins if its column is lower).  Column b is retired by writing -inf.
//                        Every loop has a trip count known on entry; there is no communication between workgroups.
#include <algorithm>
#include <cmath>

#include "common.hpp"

#pragma clang fp contract(off)  // the linkage updates are restated operation by operation (tests/diarize_oracle.py)

namespace ssp {

constexpr int DZ_MAX_Q = 1024;  // largest embedding dimension of ssp_pairwise_scores
constexpr int DZ_MAX_N = 4096;  // most segments of one recording
constexpr int DZ_N_LDS = 192;   // recordings up to this many segments cluster in LDS (192 x 193 floats = 144.75 KiB)
constexpr int DZ_BM = 64, DZ_BK = 32, DZ_LS = DZ_BK + 1;

using f32x16 = __attribute__((ext_vector_type(16))) float;

// order-preserving key of a float (snorm.hip's), after -0.0 has become +0.0: equal floats have equal keys
__device__ __forceinline__ uint32_t dz_key(float v) {
    const uint32_t u = __float_as_uint(v + 0.f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long dz_wave_max(unsigned long long k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(k, o);
        k = other > k ? other : k;
    }
    return k;
}

__global__ __launch_bounds__(256) void diar_rowstat_kernel(const float* __restrict__ X, const float* __restrict__ h, int64_t row0, int64_t rows, int q,
                                                           float* __restrict__ r) {
    const int lane = threadIdx.x & 63;
    const int64_t row = row0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= row0 + rows) return;
    const float* x = X + row * q;
    double s = 0.0;
    bool bad = false;
    for (int d = lane; d < q; d += 64) {
        const float v = x[d];
        bad = bad || !(fabsf(v) < INFINITY);
        if (h) s += (double)h[d] * ((double)v * (double)v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const bool any_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if (lane == 0) r[row] = any_bad ? __builtin_nanf("") : (float)s;
}

struct DiarRec {  // one recording of a launch (host-made, uploaded per call)
    int64_t row0;    // first row of X / labels / merge outputs
    int64_t sq_off;  // float offset of its n x n block
    int64_t ws_off;  // float offset of its working copy in the workspace (workspace-resident form)
    int32_t n, lo;   // segments; clusters at which merging stops
    int32_t rec, forced;  // index in the batch; n_speakers[r] > 0
};

struct PairArgs {
    const float* X;
    const float* g;  // nullable
    const float* r;
    float* out;
    const DiarRec* recs;
    const int32_t* tiles;  // per workgroup: entry of recs, (block row << 16 | block column)
    int32_t q;
    float c0;
};

__global__ __launch_bounds__(256) void diar_pair_kernel(PairArgs a) {
    __shared__ float As[DZ_BM * DZ_LS];
    __shared__ float Bs[DZ_BM * DZ_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5, wr = wave >> 1, wc = wave & 1;
    const DiarRec rc = a.recs[a.tiles[2 * blockIdx.x]];
    const int bij = a.tiles[2 * blockIdx.x + 1];
    const int m0 = (bij >> 16) * DZ_BM, n0 = (bij & 0xffff) * DZ_BM, n = rc.n, q = a.q;
    const float* X = a.X + rc.row0 * q;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // this thread's eight cells of a panel: row e / 32 of the block, column e % 32 of the panel (a row's 32 floats are one 128-byte run)
    float ra[8], rb[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int e = s * 256 + tid, m = e >> 5, k = k0 + (e & 31);
            const bool in = k < q;
            float av = (in && m0 + m < n) ? X[(int64_t)(m0 + m) * q + k] : 0.f;
            if (a.g && in) av *= a.g[k];
            ra[s] = av;
            rb[s] = (in && n0 + m < n) ? X[(int64_t)(n0 + m) * q + k] : 0.f;
        }
    };
    const bool skip = m0 == n0 && wr > wc;  // the tile below the diagonal of a diagonal block
    fetch(0);
    for (int k0 = 0; k0 < q; k0 += DZ_BK) {
        __syncthreads();  // the previous panel's MFMAs are done with As and Bs
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int e = s * 256 + tid;
            As[(e >> 5) * DZ_LS + (e & 31)] = ra[s];
            Bs[(e >> 5) * DZ_LS + (e & 31)] = rb[s];
        }
        __syncthreads();
        if (k0 + DZ_BK < q) fetch(k0 + DZ_BK);
        if (!skip) {
#pragma unroll
            for (int kk = 0; kk < DZ_BK; kk += 2) {
                const float av = As[(wr * 32 + li) * DZ_LS + kk + lh];
                const float bv = Bs[(wc * 32 + li) * DZ_LS + kk + lh];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
            }
        }
    }
    if (skip) return;
    // accumulator r: row (r & 3) + 8 (r >> 2) + 4 lh, column li
    float* out = a.out + rc.sq_off;
    const int gj = n0 + wc * 32 + li;
    const float rj = gj < n ? a.r[rc.row0 + gj] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gi = m0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (gi < n && gj < n && gi <= gj) {
            const float v = acc[r] - (a.r[rc.row0 + gi] + rj) + a.c0;
            out[(int64_t)gi * n + gj] = v;
            if (gi != gj) out[(int64_t)gj * n + gi] = v;
        }
    }
}

struct AhcArgs {
    const float* scores;
    const DiarRec* recs;  // this launch's recordings, longest first
    float* ws;            // workspace-resident form
    int32_t* labels;
    int32_t* n_clusters;
    int32_t* merge_pair;  // nullable
    float* merge_score;   // nullable
    int32_t linkage;
    float threshold;
};

// dynamic LDS of a launch whose longest recording has nmax segments: the working copy (LDS-resident form), then five words per segment
static size_t ahc_lds_bytes(int nmax, bool resident) {
    return ((resident ? (size_t)nmax * (size_t)(nmax | 1) : 0) + 5 * (size_t)nmax + 16) * sizeof(float);
}

template <bool RES>
__global__ __launch_bounds__(256) void diar_ahc_kernel(AhcArgs a, int nmax) {
    extern __shared__ __attribute__((aligned(16))) char dz_smem[];
    __shared__ unsigned long long red[4];
    __shared__ int n_list;
    const DiarRec rc = a.recs[blockIdx.x];
    const int n = rc.n, ld = n | 1, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* smem = reinterpret_cast<float*>(dz_smem);
    float* W;
    uint32_t* bestk;
    if constexpr (RES) {
        W = smem;
        bestk = reinterpret_cast<uint32_t*>(smem + (size_t)nmax * (size_t)(nmax | 1));
    } else {
        W = a.ws + rc.ws_off;
        bestk = reinterpret_cast<uint32_t*>(smem);
    }
    int32_t* bestc = reinterpret_cast<int32_t*>(bestk + nmax);
    int32_t* size = bestc + nmax;  // 0: the cluster has been merged away
    int32_t* clus = size + nmax;   // the cluster a segment is in
    int32_t* list = clus + nmax;   // rows to rescan; at the end the ranks of the clusters
    const float* S = a.scores + rc.sq_off;
    int32_t* labels = a.labels + rc.row0;
    const float ninf = -INFINITY;

    // the working copy, mirrored from the upper triangle; the merge rows start unused
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        for (int j = i + 1 + tid; j < n; j += 256) {
            const float v = S[(int64_t)i * n + j];
            bad |= !(fabsf(v) < INFINITY);
            W[(int64_t)i * ld + j] = v;
            W[(int64_t)j * ld + i] = v;
        }
    }
    for (int i = tid; i < n; i += 256) {
        size[i] = 1;
        clus[i] = i;
        if (a.merge_pair) a.merge_pair[2 * (rc.row0 + i)] = a.merge_pair[2 * (rc.row0 + i) + 1] = -1;
        if (a.merge_score) a.merge_score[rc.row0 + i] = __builtin_nanf("");
    }
    if (tid == 0) n_list = 0;
    bad = __syncthreads_or(bad);
    if (bad) {
        for (int i = tid; i < n; i += 256) labels[i] = -1;
        if (tid == 0) a.n_clusters[rc.rec] = -1;
        return;
    }
    // best (key, lowest column) of row i over the columns j > i that are live (a retired column holds -inf: key 0 = none)
    auto rescan = [&](int i) {
        unsigned long long best = 0ull;
        for (int j = i + 1 + lane; j < n; j += 64) {
            const float v = W[(int64_t)i * ld + j];
            const unsigned long long k = v == ninf ? 0ull : ((unsigned long long)dz_key(v) << 32) | (uint32_t)~j;
            best = k > best ? k : best;
        }
        best = dz_wave_max(best);
        if (lane == 0) {
            bestk[i] = (uint32_t)(best >> 32);
            bestc[i] = (int32_t) ~(uint32_t)best;
        }
    };
    for (int i = wave; i < n; i += 4) rescan(i);
    __syncthreads();

    const float thr = rc.forced ? ninf : a.threshold;
    int count = n;
    for (int m = 0; m + 1 < n; ++m) {
        if (count <= rc.lo) break;
        // the pair with the largest score; ties to the lowest a, then the lowest b (the row's best holds its lowest column)
        unsigned long long top = 0ull;
        for (int i = tid; i < n; i += 256) {
            const unsigned long long k = ((unsigned long long)bestk[i] << 32) | (uint32_t)~i;
            top = (size[i] != 0 && bestk[i] != 0u && k > top) ? k : top;
        }
        top = dz_wave_max(top);
        if (lane == 0) red[wave] = top;
        __syncthreads();
        top = red[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) top = red[w] > top ? red[w] : top;
        if (top == 0ull) break;  // (no live pair: cannot happen while count > 1)
        const int ra = (int32_t) ~(uint32_t)top, rb = bestc[ra];
        const float s = W[(int64_t)ra * ld + rb];
        if (!(s >= thr)) break;
        const float fa = (float)size[ra], fb = (float)size[rb];
        // the new scores of cluster a; column b retires
        for (int k = tid; k < n; k += 256) {
            if (clus[k] == rb) clus[k] = ra;
            if (k == ra || k == rb) continue;
            if (size[k] != 0) {
                const float sa = W[(int64_t)ra * ld + k], sb = W[(int64_t)rb * ld + k];
                float v;
                if (a.linkage == 0)
                    v = (fa * sa + fb * sb) / (fa + fb);
                else if (a.linkage == 1)
                    v = fminf(sa, sb);
                else
                    v = fmaxf(sa, sb);
                W[(int64_t)ra * ld + k] = v;
                W[(int64_t)k * ld + ra] = v;
            }
            W[(int64_t)k * ld + rb] = ninf;
        }
        if (tid == 0) {
            if (a.merge_pair) {
                a.merge_pair[2 * (rc.row0 + m)] = ra;
                a.merge_pair[2 * (rc.row0 + m) + 1] = rb;
            }
            if (a.merge_score) a.merge_score[rc.row0 + m] = s;
        }
        __syncthreads();
        // rows whose best is gone are listed for a rescan; the others compare their one changed entry
        for (int i = tid; i < n; i += 256) {
            if (i == rb) {
                size[i] = 0;
                bestk[i] = 0u;
            } else if (i == ra) {
                size[i] = (int32_t)(fa + fb);
                W[(int64_t)ra * ld + rb] = ninf;  // (every thread has read s: a barrier back)
                list[atomicAdd(&n_list, 1)] = i;
            } else if (size[i] != 0) {
                if (bestk[i] != 0u && (bestc[i] == ra || bestc[i] == rb)) {
                    list[atomicAdd(&n_list, 1)] = i;
                } else if (i < ra) {
                    const uint32_t k = dz_key(W[(int64_t)i * ld + ra]);
                    if (k > bestk[i] || (k == bestk[i] && ra < bestc[i])) {
                        bestk[i] = k;
                        bestc[i] = ra;
                    }
                }
            }
        }
        __syncthreads();
        const int nl = n_list;
        for (int t = wave; t < nl; t += 4) rescan(list[t]);
        __syncthreads();
        if (tid == 0) n_list = 0;
        --count;
    }
    __syncthreads();
    // label = rank of the segment's cluster among the live clusters, which are numbered by their lowest member: a cluster's index
    const int chunk = (n + 255) / 256;
    int mine = 0;
    for (int t = 0; t < chunk; ++t) {
        const int i = tid * chunk + t;
        mine += (i < n && size[i] != 0) ? 1 : 0;
    }
    int32_t* part = reinterpret_cast<int32_t*>(bestk);  // (the row bests are done with)
    int before = 0;
    if (n >= 256) {
        part[tid] = mine;
        __syncthreads();
        for (int t = 0; t < tid; ++t) before += part[t];
    } else {  // chunk == 1: thread i owns segment i
        for (int t = 0; t < tid && t < n; ++t) before += size[t] != 0 ? 1 : 0;
    }
    for (int t = 0; t < chunk; ++t) {
        const int i = tid * chunk + t;
        if (i < n) {
            list[i] = before;
            before += size[i] != 0 ? 1 : 0;
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) labels[i] = list[clus[i]];
    if (tid == 0) a.n_clusters[rc.rec] = count;
}

static int check_recordings(const ssp_segments* seg, const char* who) {
    for (int64_t r = 0; r < seg->n; ++r)
        if (seg->host[(size_t)r + 1] - seg->host[(size_t)r] > DZ_MAX_N)
            SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: recording %lld has %lld segments, more than the supported %d", who, (long long)r,
                     (long long)(seg->host[(size_t)r + 1] - seg->host[(size_t)r]), DZ_MAX_N);
    return SSP_OK;
}

// the recordings with segments, their blocks packed in batch order
static void make_recs(const ssp_segments* seg, std::vector<DiarRec>& recs) {
    recs.clear();
    int64_t sq = 0;
    for (int64_t r = 0; r < seg->n; ++r) {
        const int64_t n = seg->host[(size_t)r + 1] - seg->host[(size_t)r];
        if (n > 0) recs.push_back(DiarRec{seg->host[(size_t)r], sq, 0, (int32_t)n, 1, (int32_t)r, 0});
        sq += n * n;
    }
}

// appends `bytes` of `src` to the host image at a 16-byte boundary; returns the offset
static size_t blob_add(std::vector<char>& blob, const void* src, size_t bytes) {
    const size_t at = (blob.size() + 15) / 16 * 16;
    blob.resize(at + bytes);
    if (bytes) std::memcpy(blob.data() + at, src, bytes);
    return at;
}

}  // namespace ssp

using namespace ssp;

extern "C" {

int ssp_pairwise_size(const ssp_segments* seg, int64_t* total_out) {
    if (!seg || !total_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_pairwise_size: null pointer");
    int64_t t = 0;
    for (int64_t r = 0; r < seg->n; ++r) {
        const int64_t n = seg->host[(size_t)r + 1] - seg->host[(size_t)r];
        t += n * n;
    }
    *total_out = t;
    return SSP_OK;
}

int ssp_pairwise_scores(ssp_ctx* ctx, const float* X, const ssp_segments* seg, int32_t q, const float* g, const float* h, float c0, float* out,
                        int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_pairwise_scores");
    if (!ctx) SSP_FAIL(SSP_ERR_INVALID, "null ssp_ctx");
    if (!seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_pairwise_scores: null segments");
    if (q < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_pairwise_scores: q=%d", q);
    SSP_TRY(check_where(where, "ssp_pairwise_scores"));
    if (!std::isfinite(c0)) SSP_FAIL(SSP_ERR_INVALID, "ssp_pairwise_scores: c0 is not finite");
    for (int d = 0; d < q && d < DZ_MAX_Q; ++d)
        if ((g && !std::isfinite(g[d])) || (h && !std::isfinite(h[d]))) SSP_FAIL(SSP_ERR_INVALID, "ssp_pairwise_scores: g or h is not finite at %d", d);
    if (q > DZ_MAX_Q) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_pairwise_scores: q=%d exceeds the supported dimension (%d)", q, DZ_MAX_Q);
    SSP_TRY(check_recordings(seg, "ssp_pairwise_scores"));
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    std::vector<DiarRec> recs;
    make_recs(seg, recs);
    if (recs.empty()) return SSP_OK;
    if (!X || !out) SSP_FAIL(SSP_ERR_INVALID, "ssp_pairwise_scores: null X or out");
    const int64_t rows = seg->host.back();
    int64_t total_sq = 0;
    SSP_TRY(ssp_pairwise_size(seg, &total_sq));
    std::vector<int32_t> tiles;
    for (size_t e = 0; e < recs.size(); ++e) {
        const int nb = ceil_div(recs[e].n, DZ_BM);
        for (int bi = 0; bi < nb; ++bi)
            for (int bj = bi; bj < nb; ++bj) {
                tiles.push_back((int32_t)e);
                tiles.push_back((bi << 16) | bj);
            }
    }
    if (tiles.size() / 2 > (size_t)INT32_MAX || ceil_div<int64_t>(rows, 4) > INT32_MAX)
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_pairwise_scores: too many blocks for one launch");
    std::vector<char>& blob = ctx->diar_host;
    blob.clear();
    const size_t at_recs = blob_add(blob, recs.data(), recs.size() * sizeof(DiarRec));
    const size_t at_tiles = blob_add(blob, tiles.data(), tiles.size() * sizeof(int32_t));
    const size_t at_g = blob_add(blob, g, g ? (size_t)q * sizeof(float) : 0);
    const size_t at_h = blob_add(blob, h, h ? (size_t)q * sizeof(float) : 0);
    hipStream_t s = ctx->stream;
    SSP_TRY(ctx->diar_tab.reserve(blob.size()));
    SSP_TRY(ctx->diar_r.reserve((size_t)rows * sizeof(float)));
    SSP_HIP(hipMemcpyAsync(ctx->diar_tab.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
    StageScope st(ctx, where);
    const float* dX = st.in(X, (size_t)rows * (size_t)q * sizeof(float));
    float* dO = st.out(out, (size_t)total_sq * sizeof(float));
    SSP_TRY(st.status());
    const char* tab = ctx->diar_tab.as<char>();
    const int64_t row0 = seg->host.front();
    PairArgs a{dX, g ? reinterpret_cast<const float*>(tab + at_g) : nullptr, ctx->diar_r.as<float>(), dO,
               reinterpret_cast<const DiarRec*>(tab + at_recs), reinterpret_cast<const int32_t*>(tab + at_tiles), q, c0};
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    hipLaunchKernelGGL(diar_rowstat_kernel, dim3((unsigned)ceil_div<int64_t>(rows - row0, 4)), dim3(256), 0, s, dX,
                       h ? reinterpret_cast<const float*>(tab + at_h) : nullptr, row0, rows - row0, q, ctx->diar_r.as<float>());
    hipLaunchKernelGGL(diar_pair_kernel, dim3((unsigned)(tiles.size() / 2)), dim3(256), 0, s, a);
    SSP_HIP(hipGetLastError());
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}

int ssp_ahc_cluster(ssp_ctx* ctx, const float* scores, const ssp_segments* seg, int32_t linkage, float threshold, int32_t min_clusters,
                    const int32_t* n_speakers, int32_t* labels_out, int32_t* n_clusters_out, int32_t* merge_pair_out, float* merge_score_out,
                    int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_ahc_cluster");
    if (!ctx) SSP_FAIL(SSP_ERR_INVALID, "null ssp_ctx");
    if (!seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_ahc_cluster: null segments");
    if (linkage < 0 || linkage > 2) SSP_FAIL(SSP_ERR_INVALID, "ssp_ahc_cluster: linkage=%d (0 average, 1 complete, 2 single)", linkage);
    if (threshold != threshold) SSP_FAIL(SSP_ERR_INVALID, "ssp_ahc_cluster: the threshold is NaN");
    if (min_clusters < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_ahc_cluster: min_clusters=%d", min_clusters);
    SSP_TRY(check_where(where, "ssp_ahc_cluster"));
    for (int64_t r = 0; n_speakers && r < seg->n; ++r)
        if (n_speakers[r] < 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_ahc_cluster: n_speakers[%lld]=%d", (long long)r, n_speakers[r]);
    SSP_TRY(check_recordings(seg, "ssp_ahc_cluster"));
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (seg->n == 0) return SSP_OK;
    if (!n_clusters_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_ahc_cluster: null n_clusters_out");
    std::vector<DiarRec> recs;
    make_recs(seg, recs);
    if (recs.empty()) return SSP_OK;  // (recordings without segments are not written)
    const int64_t rows = seg->host.back(), R = seg->n;
    if (!scores || !labels_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_ahc_cluster: null scores or labels_out");
    int64_t total_sq = 0, ws_floats = 0;
    SSP_TRY(ssp_pairwise_size(seg, &total_sq));
    for (DiarRec& d : recs) {
        const int32_t ns = n_speakers ? n_speakers[d.rec] : 0;
        d.forced = ns > 0;
        d.lo = ns > 0 ? ns : min_clusters;
        if (d.n > DZ_N_LDS) {
            d.ws_off = ws_floats;
            ws_floats += (int64_t)d.n * (d.n | 1);
        }
    }
    // longest first; four launches: LDS-resident recordings of up to 64, 128 and DZ_N_LDS segments (the LDS a workgroup takes follows the
    // launch's longest), and the workspace-resident ones
    std::stable_sort(recs.begin(), recs.end(), [](const DiarRec& x, const DiarRec& y) { return x.n > y.n; });
    const int caps[4] = {DZ_MAX_N, DZ_N_LDS, 128, 64};
    size_t first[5] = {0, 0, 0, 0, recs.size()};
    for (int b = 1; b < 4; ++b) {
        first[b] = first[b - 1];
        while (first[b] < recs.size() && recs[first[b]].n > caps[b]) ++first[b];
    }
    std::vector<char>& blob = ctx->diar_host;
    blob.clear();
    const size_t at_recs = blob_add(blob, recs.data(), recs.size() * sizeof(DiarRec));
    hipStream_t s = ctx->stream;
    SSP_TRY(ctx->diar_tab.reserve(blob.size()));
    if (ws_floats) SSP_TRY(ctx->diar_ws.reserve((size_t)ws_floats * sizeof(float)));
    SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(diar_ahc_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)ahc_lds_bytes(DZ_N_LDS, true)));
    SSP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(diar_ahc_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)ahc_lds_bytes(DZ_MAX_N, false)));
    SSP_HIP(hipMemcpyAsync(ctx->diar_tab.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
    // what no workgroup writes (counts of empty recordings, rows before offsets[0]) keeps the caller's bytes: the counts are pre-loaded
    // whole, of the per-row outputs the `lead` rows
    StageScope st(ctx, where);
    const float* dS = st.in(scores, (size_t)total_sq * sizeof(float));
    int32_t* dL = st.out(labels_out, (size_t)rows * sizeof(int32_t));
    int32_t* dN = st.out(n_clusters_out, (size_t)R * sizeof(int32_t), true);
    int32_t* dP = st.out(merge_pair_out, (size_t)rows * 2 * sizeof(int32_t));
    float* dM = st.out(merge_score_out, (size_t)rows * sizeof(float));
    SSP_TRY(st.status());
    if (where == SSP_HOST && seg->host.front() > 0) {
        const size_t lead = (size_t)seg->host.front();
        SSP_HIP(hipMemcpyAsync(dL, labels_out, lead * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (dP) SSP_HIP(hipMemcpyAsync(dP, merge_pair_out, lead * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (dM) SSP_HIP(hipMemcpyAsync(dM, merge_score_out, lead * sizeof(float), hipMemcpyHostToDevice, s));
    }
    const DiarRec* dRecs = reinterpret_cast<const DiarRec*>(ctx->diar_tab.as<char>() + at_recs);
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    for (int b = 0; b < 4; ++b) {
        const size_t cnt = first[b + 1] - first[b];
        if (cnt == 0) continue;
        AhcArgs a{dS, dRecs + first[b], ctx->diar_ws.as<float>(), dL, dN, dP, dM, linkage, threshold};
        const int nmax = recs[first[b]].n;
        if (b == 0)
            hipLaunchKernelGGL(diar_ahc_kernel<false>, dim3((unsigned)cnt), dim3(256), ahc_lds_bytes(nmax, false), s, a, nmax);
        else
            hipLaunchKernelGGL(diar_ahc_kernel<true>, dim3((unsigned)cnt), dim3(256), ahc_lds_bytes(nmax, true), s, a, nmax);
    }
    SSP_HIP(hipGetLastError());
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}

}  // extern "C"
