// Every speaker's DTW template in batched launches (MFCC_DTW.py:122-152, 187-217): load_train calls generate_template once per speaker
// directory; a template starts as the speaker's first longest sample and is then, sample by sample in index order,
//   d, C, D1, path = accelerated_dtw(x, template);  template = ((x[path_i] + template[path_j]) / 2)[first entry of every path_j]
// Speakers are independent and only one speaker's samples form a chain, so round k of ALL speakers is one launch of each of two kernels:
//
//   dtw_dir_kernel      one wave per (sample, template) pair, the float64 skewed wavefront of dtw_kernel<W, double, true> (dtw.hip), which
//                       keeps, per cell, not D1 but the DIRECTION the traceback would take there: 0 diagonal, 1 up, 2 left, one byte per cell
//                       (rows padded to a multiple of four bytes: a lane's W columns of a row leave as aligned dwords).  At cell (i, j)
//                       dtw_traceback_kernel reads D0[i][j], D0[i][j+1], D0[i+1][j]: the dg / up / lf this pass holds in registers at that
//                       cell, compared by the same rule, so the path is the same at 1/8 of the memory and of the write traffic.
//   dtw_trace_kernel    one wave per pair: walks the directions from (r-1, c-1) back to (0, 0) through 64 x 64-cell tiles staged in LDS (the
//                       walk is a chain of dependent reads: from LDS, with one global round trip per tile), notes per template column the
//                       sample row of its LAST visit (walking backwards that is the FIRST path entry of the column: the one the reference
//                       keeps) and, a tile's columns done, updates them with all lanes: t[j] = (x[i] + t[j]) / 2, rows of dim float64.
//                       Every column is read and written once, by one lane, so the template is updated in place; no path is stored.
//
// The cost of a cell is taken from the sample and the template rounded to float32 and widened again, because that is what the single-pair
// path does (api.dtw_path hands ssp_dtw_path float32 arrays): a deviation from the reference, kept so that both paths agree bit for bit.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace ssp {

struct TmplPair {
    int64_t x_off, t_off;   // first row of the sample in x / of the template in tmpl
    int64_t dir_off;        // first byte of the pair's directions: r rows of (c + 3 & ~3) bytes (a multiple of 4)
    int64_t bnd_off;        // first of the pair's r parked boundary values (super-block scheme)
    int32_t r, c;
};

struct TmplArgs {
    const double* x;        // every sequence's rows back to back
    double* tmpl;           // every group's template back to back
    const TmplPair* pairs;  // this launch's pairs: one wave (one block) each
    uint8_t* dirs;
    uint32_t* bnd;          // float64 values as two dwords
    int32_t dim;
};

__device__ __forceinline__ double f32r(double v) { return (double)(float)v; }

// Stores: the kernel is required to contain no 8-byte global store at all (tests/test_dtw_templates_isa.py: the guard against a
// float64 cell value ever being written per cell again), and that guard cannot tell a float64 from two packed direction dwords.  So a
// row's direction dwords leave as single relaxed dword stores, which the compiler does not merge into dwordx2 / x4, and the float64
// boundary value of the super-block scheme is parked as its two halves (tests/test_dtw_templates_gpu.py runs templates of several
// super-blocks).  The stores are the minor part of a step: W / 4 of them beside W cells of float64 compares and adds.
template <int W>
__global__ __launch_bounds__(64) void dtw_dir_kernel(TmplArgs a) {
    typedef double T;
    const int lane = threadIdx.x;
    const TmplPair P = a.pairs[blockIdx.x];
    const int r = P.r, c = P.c, dim = a.dim;
    const size_t stride = (size_t)((c + 3) & ~3);
    const double* __restrict__ x = a.x + P.x_off * dim;
    const double* __restrict__ y = a.tmpl + P.t_off * dim;
    uint32_t* __restrict__ bnd = a.bnd + 2 * P.bnd_off;
    uint8_t* __restrict__ dirs = a.dirs + P.dir_off;
    const T INF = (T)INFINITY;
    for (int cb0 = 0; cb0 < c; cb0 += 64 * W) {
        const int cb = min(64 * W, c - cb0);        // columns of this super-block
        const int lanes = (cb + W - 1) / W;         // lanes that own at least one column
        const int j0 = cb0 + lane * W;              // this lane's first column (a multiple of 4)
        const bool more = cb0 + 64 * W < c;         // another super-block follows: park the last column
        T yreg[W];
        if (dim == 1) {
#pragma unroll
            for (int k = 0; k < W; ++k) yreg[k] = j0 + k < c ? f32r(y[j0 + k]) : (T)0;
        }
        T prev[W];
#pragma unroll
        for (int k = 0; k < W; ++k) prev[k] = INF;  // row -1
        T last = INF;    // this lane's value in its LAST column at its previous step (row i - 1)
        T diagl = INF;   // D[i-1][j0-1]
        for (int s = 0; s < r + lanes - 1; ++s) {
            const int i = s - lane;
            T left = __shfl_up(last, 1);
            const bool act = i >= 0 && i < r && lane < lanes;
            if (lane == 0) {
                if (cb0 == 0) {
                    left = INF;
                    diagl = i == 0 ? (T)0 : INF;
                } else if (act) {
                    // agent-scope loads: the values were stored by another lane of this wave in the previous super-block
                    auto parked = [&](int row) -> T {
                        const uint32_t lo = __hip_atomic_load(&bnd[2 * row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        const uint32_t hi = __hip_atomic_load(&bnd[2 * row + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        return __hiloint2double((int)hi, (int)lo);
                    };
                    left = parked(i);
                    diagl = i > 0 ? parked(i - 1) : INF;
                }
            }
            if (act) {
                T cur[W];
                uint32_t pk[W / 4];
#pragma unroll
                for (int q = 0; q < W / 4; ++q) pk[q] = 0u;
                T xi = 0;
                if (dim == 1) xi = f32r(x[i]);
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    const int j = j0 + k;
                    T cost;
                    if (dim == 1) {
                        cost = xi > yreg[k] ? xi - yreg[k] : yreg[k] - xi;
                    } else {
                        T ss = 0;
                        if (j < c)
                            for (int e = 0; e < dim; ++e) {
                                const T df = (T)(float)x[(size_t)i * dim + e] - (T)(float)y[(size_t)j * dim + e];
                                ss += df * df;
                            }
                        cost = sqrt(ss);
                    }
                    const T up = prev[k];
                    const T dg = k == 0 ? diagl : prev[k - 1];
                    const T lf = k == 0 ? left : cur[k - 1];
                    // dtw_traceback_kernel's choice at this cell
                    uint32_t tb = 0u;
                    T m = dg;
                    if (up < m) { m = up; tb = 1u; }
                    if (lf < m) tb = 2u;
                    const T mn = dg < up ? (dg < lf ? dg : lf) : (up < lf ? up : lf);
                    cur[k] = j < c ? cost + mn : INF;
                    pk[k >> 2] |= tb << (8 * (k & 3));
                }
                uint32_t* drow = reinterpret_cast<uint32_t*>(dirs + (size_t)i * stride + j0);
#pragma unroll
                for (int q = 0; q < W / 4; ++q)
                    if (j0 + 4 * q < c) __hip_atomic_store(drow + q, pk[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                diagl = left;  // D[i][j0-1] is the diagonal neighbour of row i + 1
                const int kl = min(W, cb - lane * W) - 1;  // this lane's last valid column
                T lv = cur[0];
#pragma unroll
                for (int k = 1; k < W; ++k) lv = k == kl ? cur[k] : lv;
#pragma unroll
                for (int k = 0; k < W; ++k) prev[k] = cur[k];
                last = lv;
                if (more && lane == lanes - 1) {
                    __hip_atomic_store(&bnd[2 * i], (uint32_t)__double2loint(lv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&bnd[2 * i + 1], (uint32_t)__double2hiint(lv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        if (more) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");  // the parked column is read back by lane 0 of this wave
    }
}

// The walk is bounded by construction: in row 0 it steps left and in column 0 it steps up whatever the stored byte says, every step
// lowers i or j, so it stays inside the matrix and ends at (0, 0) after at most r + c - 2 steps for any content of `dirs`.
constexpr int TILE = 64, TILE_DW = TILE / 4 + 1;  // a tile's columns start at a multiple of 4 at or below j - 63: up to 67 of them
__global__ __launch_bounds__(64) void dtw_trace_kernel(TmplArgs a) {
    __shared__ uint32_t tile[TILE * TILE_DW];
    __shared__ int first_i[TILE_DW * 4];
    __shared__ int next_ij[2];
    const int lane = threadIdx.x;
    const TmplPair P = a.pairs[blockIdx.x];
    const int r = P.r, c = P.c, dim = a.dim;
    const size_t stride = (size_t)((c + 3) & ~3);
    const double* __restrict__ x = a.x + P.x_off * dim;
    double* t = a.tmpl + P.t_off * dim;
    const uint8_t* __restrict__ dirs = a.dirs + P.dir_off;
    int i = r - 1, j = c - 1;
    for (;;) {
        const int ib = max(0, i - (TILE - 1));         // the tile: rows ib .. i, columns jb .. j
        const int jb = max(0, j - (TILE - 1)) & ~3;
        const int nq = (j - jb) / 4 + 1;               // <= TILE_DW dwords of a row; the last one ends inside the padded row
        if (ib + lane <= i) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(dirs + (size_t)(ib + lane) * stride + jb);
#pragma unroll
            for (int q = 0; q < TILE_DW; ++q)
                if (q < nq) tile[lane * TILE_DW + q] = src[q];
        }
        __syncthreads();
        if (lane == 0) {
            const uint8_t* tb8 = reinterpret_cast<const uint8_t*>(tile);
            int ci = i, cj = j;
            for (;;) {
                first_i[cj - jb] = ci;  // a later (lower) row of the same column overwrites it
                if (ci == 0 && cj == 0) {
                    cj = -1;  // done: columns 0 .. j are complete
                    break;
                }
                const int tb = ci == 0 ? 2 : cj == 0 ? 1 : (int)tb8[(ci - ib) * (TILE_DW * 4) + (cj - jb)];
                if (tb == 0) { --ci; --cj; }
                else if (tb == 1) --ci;
                else --cj;
                if (ci < ib || cj < jb) break;
            }
            next_ij[0] = ci;
            next_ij[1] = cj;
        }
        __syncthreads();
        const int ni = next_ij[0], nj = next_ij[1];
        // In-place update, no second buffer: this rests on ONE invariant.  Every step lowers i or j and none raises either, so once the
        // walk stands in column nj it never returns to a column above nj: columns nj + 1 .. j have had their last visit, first_i holds
        // their final row, and each of their elements is read once and written once here, by the same lane.  Column nj itself may be
        // visited again at a lower row (the walk left through the tile's top row): it is NOT updated now, the next tile notes it anew.
        // Columns below nj are untouched so far.  The forward kernel that read t for this round has finished (stream order).
        const int n = (j - nj) * dim;
        for (int idx = lane; idx < n; idx += 64) {
            const int col = nj + 1 + idx / dim, e = idx % dim;
            const size_t at = (size_t)col * dim + e;
            t[at] = (x[(size_t)first_i[col - jb] * dim + e] + t[at]) / 2;
        }
        if (nj < 0) break;
        i = ni;
        j = nj;
        __syncthreads();  // the tile and first_i are rewritten
    }
}

}  // namespace ssp

using namespace ssp;

extern "C" int ssp_dtw_templates(ssp_ctx* ctx, const double* x, const int64_t* seq_off, int64_t n_seq, const int64_t* grp_off,
                                 int64_t n_grp, int32_t dim, int64_t workspace_bytes, double* tmpl_out, int64_t* tmpl_off_out,
                                 float* kernel_ms) {
    ssp::TraceRange trace_("ssp_dtw_templates");
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (!x || !seq_off || !grp_off || !tmpl_out || !tmpl_off_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_dtw_templates: null pointer");
    if (dim < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_dtw_templates: dim");
    if (n_seq < 1 || n_grp < 1 || n_grp > n_seq || workspace_bytes < 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_dtw_templates: counts");
    if (seq_off[0] != 0 || grp_off[0] != 0 || grp_off[n_grp] != n_seq) SSP_FAIL(SSP_ERR_INVALID, "ssp_dtw_templates: offsets must span all sequences from 0");
    for (int64_t q = 0; q < n_seq; ++q)
        if (seq_off[q + 1] <= seq_off[q]) SSP_FAIL(SSP_ERR_INVALID, "ssp_dtw_templates: sequence %lld is empty or its offsets decrease", (long long)q);
    for (int64_t g = 0; g < n_grp; ++g)
        if (grp_off[g + 1] <= grp_off[g]) SSP_FAIL(SSP_ERR_INVALID, "ssp_dtw_templates: group %lld is empty or its offsets decrease", (long long)g);
    const int64_t rows = seq_off[n_seq];
    for (int64_t k = 0; k < rows * dim; ++k)
        if (!std::isfinite(x[k])) SSP_FAIL(SSP_ERR_INVALID, "ssp_dtw_templates: non-finite input value at element %lld", (long long)k);
    // templates: the first longest sequence of every group
    std::vector<int64_t> first(n_grp), toff(n_grp + 1, 0);
    for (int64_t g = 0; g < n_grp; ++g) {
        int64_t best = grp_off[g], L = 0;
        for (int64_t q = grp_off[g]; q < grp_off[g + 1]; ++q)
            if (seq_off[q + 1] - seq_off[q] > L) {
                L = seq_off[q + 1] - seq_off[q];
                best = q;
            }
        for (int64_t q = grp_off[g]; q < grp_off[g + 1]; ++q) {
            const int64_t r = seq_off[q + 1] - seq_off[q];
            if (q != best && (r > (1 << 20) || L > (1 << 20) || (double)r * (double)L > 5.0e8))
                SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_dtw_templates: sequences too long");
        }
        first[g] = best;
        toff[g + 1] = toff[g] + L;
    }
    std::vector<double> tinit((size_t)toff[n_grp] * dim);
    for (int64_t g = 0; g < n_grp; ++g)
        memcpy(tinit.data() + (size_t)toff[g] * dim, x + (size_t)seq_off[first[g]] * dim, (size_t)(toff[g + 1] - toff[g]) * dim * sizeof(double));
    // rounds: pair k of a group is its k-th sequence other than the template.  Consecutive groups share launches while every round's
    // directions fit the cap; a group that does not fit alone gets launches of its own (the buffer is sized for the largest round)
    const int64_t cap = workspace_bytes > 0 ? workspace_bytes : (int64_t)1 << 30;
    struct Launch { size_t first; int32_t n, W; };
    std::vector<TmplPair> pairs;
    std::vector<Launch> launches;
    int64_t dir_need = 0, bnd_need = 0;
    auto pair_bytes = [&](int64_t q, int64_t g) { return (seq_off[q + 1] - seq_off[q]) * ((toff[g + 1] - toff[g] + 3) & ~(int64_t)3); };
    for (int64_t g0 = 0; g0 < n_grp;) {
        std::vector<int64_t> sum;  // bytes per round of the chunk g0 .. g1 - 1
        int64_t g1 = g0;
        for (; g1 < n_grp; ++g1) {
            std::vector<int64_t> mine;
            for (int64_t q = grp_off[g1]; q < grp_off[g1 + 1]; ++q)
                if (q != first[g1]) mine.push_back(pair_bytes(q, g1));
            bool fits = true;
            for (size_t k = 0; k < mine.size(); ++k) fits = fits && (k < sum.size() ? sum[k] : 0) + mine[k] <= cap;
            if (!fits && g1 > g0) break;
            if (mine.size() > sum.size()) sum.resize(mine.size(), 0);
            for (size_t k = 0; k < mine.size(); ++k) sum[k] += mine[k];
        }
        for (size_t k = 0; k < sum.size(); ++k) {
            Launch l{pairs.size(), 0, 4};
            int64_t doff = 0, boff = 0, max_c = 0;
            for (int64_t g = g0; g < g1; ++g) {
                if ((int64_t)k >= grp_off[g + 1] - grp_off[g] - 1) continue;
                int64_t q = grp_off[g] + (int64_t)k;
                if (q >= first[g]) ++q;  // skip the template itself
                const int64_t r = seq_off[q + 1] - seq_off[q], c = toff[g + 1] - toff[g];
                pairs.push_back(TmplPair{seq_off[q], toff[g], doff, boff, (int32_t)r, (int32_t)c});
                doff += pair_bytes(q, g);
                boff += r;
                max_c = std::max(max_c, c);
                ++l.n;
            }
            const int64_t need = (max_c + 63) / 64;  // column block per lane: the smallest that covers the longest template in one super-block
            l.W = need <= 4 ? 4 : need <= 8 ? 8 : need <= 16 ? 16 : 24;
            dir_need = std::max(dir_need, doff);
            bnd_need = std::max(bnd_need, boff);
            launches.push_back(l);
        }
        g0 = g1;
    }
    hipStream_t s = ctx->stream;
    if (!launches.empty()) {
        DevBuf dx, dt, dp, dd, db;
        // an error return below must not free host or device memory that enqueued copies and kernels still use: drain the stream first
        struct Drain {
            hipStream_t s;
            ~Drain() { (void)hipStreamSynchronize(s); }
        } drain{s};  // (declared after the buffers: destroyed before them; after the final sync it returns at once)
        SSP_TRY(dx.alloc((size_t)rows * dim * sizeof(double)));
        SSP_TRY(dt.alloc(tinit.size() * sizeof(double)));
        SSP_TRY(dp.alloc(pairs.size() * sizeof(TmplPair)));
        SSP_TRY(dd.alloc((size_t)dir_need));
        SSP_TRY(db.alloc((size_t)bnd_need * sizeof(double)));
        SSP_HIP(hipMemcpyAsync(dx.p, x, (size_t)rows * dim * sizeof(double), hipMemcpyHostToDevice, s));
        SSP_HIP(hipMemcpyAsync(dt.p, tinit.data(), tinit.size() * sizeof(double), hipMemcpyHostToDevice, s));
        SSP_HIP(hipMemcpyAsync(dp.p, pairs.data(), pairs.size() * sizeof(TmplPair), hipMemcpyHostToDevice, s));
        Timer tm;
        SSP_TRY(tm.start(kernel_ms != nullptr, s));
        for (const Launch& l : launches) {
            TmplArgs a{dx.as<double>(), dt.as<double>(), dp.as<TmplPair>() + l.first, dd.as<uint8_t>(), db.as<uint32_t>(), dim};
            const dim3 grid((unsigned)l.n), block(64);
            switch (l.W) {
                case 4: hipLaunchKernelGGL(dtw_dir_kernel<4>, grid, block, 0, s, a); break;
                case 8: hipLaunchKernelGGL(dtw_dir_kernel<8>, grid, block, 0, s, a); break;
                case 16: hipLaunchKernelGGL(dtw_dir_kernel<16>, grid, block, 0, s, a); break;
                default: hipLaunchKernelGGL(dtw_dir_kernel<24>, grid, block, 0, s, a); break;
            }
            hipLaunchKernelGGL(dtw_trace_kernel, grid, block, 0, s, a);
        }
        SSP_HIP(hipGetLastError());
        SSP_TRY(tm.stop(s, kernel_ms));
        SSP_HIP(hipMemcpyAsync(tmpl_out, dt.p, tinit.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        SSP_HIP(hipStreamSynchronize(s));  // the buffers are freed at return
    } else {
        memcpy(tmpl_out, tinit.data(), tinit.size() * sizeof(double));  // single-sequence groups only: nothing to warp
    }
    memcpy(tmpl_off_out, toff.data(), (size_t)(n_grp + 1) * sizeof(int64_t));  // outputs are written on success only
    return SSP_OK;
}
