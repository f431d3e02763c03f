// PLP back end for gfx950: RASTA filtering of the log critical-band energies, equal-loudness weighting + cube-root compression,
// autocorrelation, Levinson-Durbin, LPC -> cepstrum, lifter.  The front end (framing, pre-emphasis, window, FFT, power spectrum,
// Bark filterbank, ln) is the fused MFCC pass with a Bark table and an identity DCT (frontend.preset_sidekit_plp).
//
// Replaces sidekit.frontend.features.plp at the reference's call sites GMM_UBM.py:95, d_vector.py:93, UI/GMM_UBM_GUI.py:93,
// UI/tmp.py:315-318 (sidekit's source is absent: the algorithm is the published rastamat one that sidekit ports, see
// oracle/ref_cpu.py "PLP" — parity unpinned).
//
//   plp_rasta_kernel   thread = (utterance, band): the recursion y[t] = sum_i b_i x[t-i] + 0.94 y[t-1] along time, transposed
//                      direct form II as scipy / Matlab run it; first four outputs zero, the FIR part alone primes the state
//   plp_cep_kernel     thread = frame: everything after the filter stays in registers (NB bands, P + 1 autocorrelation lags,
//                      P LPC coefficients, P + 1 cepstra); the cosine table of the real IDFT and the equal-loudness curve come
//                      from LDS
#include <cmath>
#include <cstring>
#include <type_traits>

#include "common.hpp"

namespace ssp {

constexpr int PLP_NB_MAX = 40;  // bands: ceil(hz2bark(fs / 2)) + 1 = 21 at 16 kHz, 27 at 44.1 kHz
constexpr int PLP_P_MAX = 24;   // LPC order (sidekit: plp_order - 1 = 12)

__global__ __launch_bounds__(256) void plp_rasta_kernel(const float* __restrict__ x, float* __restrict__ y, const int64_t* __restrict__ off,
                                                        int64_t n_utt, int nb) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_utt * nb) return;
    const int64_t u = idx / nb;
    const int b = (int)(idx - u * nb);
    const int64_t f0 = off[u], T = off[u + 1] - f0;
    const float* __restrict__ xp = x + f0 * nb + b;
    float* __restrict__ yp = y + f0 * nb + b;
    float z0 = 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
    // RB inputs per trip, the next trip's already in flight: the recursion is serial along time, and with one load ahead every step
    // waited out most of a memory latency (1.64 ms for 100k x 298 frames x 21 bands; the traffic alone is 0.6 ms)
    constexpr int RB = 8;
    float cur[RB], nxt[RB];
    if (T <= 0) return;
    // (loads past the utterance's end re-read its last frame, unconditionally: a load under a per-lane condition sits in its own
    //  branch with a wait behind it; the values are never stored)
#pragma unroll
    for (int i = 0; i < RB; ++i) cur[i] = xp[min((int64_t)i, T - 1) * nb];
    for (int64_t t = 0; t < T; t += RB) {
#pragma unroll
        for (int i = 0; i < RB; ++i) nxt[i] = xp[min(t + RB + i, T - 1) * nb];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const float xv = cur[i];
            const float a1 = t + i < 4 ? 0.f : -0.94f;
            const float out = fmaf(0.2f, xv, z0);
            z0 = fmaf(0.1f, xv, z1) - a1 * out;
            z1 = z2;  // b2 = 0
            z2 = fmaf(-0.1f, xv, z3);
            z3 = -0.2f * xv;
            if (t + i < T) yp[(t + i) * nb] = t + i < 4 ? 0.f : out;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) cur[i] = nxt[i];
    }
}

struct PlpArgs {
    const float* y;    // [F x nb]  ln critical-band energies (RASTA filtered or not)
    float* out;        // [F x (P + 1)]
    const float* tab;  // [nb] equal-loudness, [(P + 1) x nb] autocorrelation weights, [P + 1] lifter
    int64_t n_frames;
    int32_t nb, P;
};

// Tables of the fixed-size instances, passed BY VALUE in the kernel argument segment: every weight is then a scalar load into an SGPR
// and rides as the scalar operand of its FMA (from LDS the 273 weights of the 21-band / 12th-order autocorrelation were 273 LDS
// reads per frame, every thread fetching the same address).
template <int NB, int PP>
struct PlpTab {
    float lq[NB];              // 0.33 log2(equal loudness) (-inf where the curve is 0)
    float cw[(PP + 1) * NB];   // cw[k * NB + n]: weight of band n in lag k
    float lw[PP + 1];          // lifter
};

// a / b with a hardware reciprocal and one Newton step (the correctly rounded expansion is ~10 instructions and a branchy scale fix-up)
__device__ __forceinline__ float div_nr(float a, float b) {
    float r = __builtin_amdgcn_rcpf(b);
    r = fmaf(fmaf(-b, r, 1.0f), r, r);
    return a * r;
}

// everything after the RASTA filter for one frame, in registers.  z = (exp(y) eql)^0.33 = exp2(0.33 log2(e) y + 0.33 log2(eql)): one
// FMA and one v_exp_f32 per band (powf(expf()) is ~60 instructions)
template <int NBM, int PM, class EQ, class CW, class LW>
__device__ __forceinline__ void plp_frame(const float* __restrict__ yp, float* __restrict__ o, int nb, int P, EQ lq, CW cw, LW lw) {
    float z[NBM];
#pragma unroll
    for (int n = 0; n < NBM; ++n)
        if (n < nb) z[n] = __builtin_amdgcn_exp2f(fmaf(yp[n], 0.33f * 1.4426950408889634f, lq(n)));
    // first and last band are replaced by their neighbours
    float zz[NBM];
#pragma unroll
    for (int n = 0; n < NBM; ++n)
        if (n < nb) zz[n] = n == 0 ? z[1] : (n == nb - 1 ? z[n - 1] : z[n]);
    // autocorrelation lags 0..P = real IDFT of the symmetric extension
    float r[PM + 1];
#pragma unroll
    for (int k = 0; k <= PM; ++k)
        if (k <= P) {
            float acc = 0.f;
#pragma unroll
            for (int n = 0; n < NBM; ++n)
                if (n < nb) acc = fmaf(zz[n], cw(k, n), acc);
            r[k] = acc;
        }
    // Levinson-Durbin
    float lp[PM];
    float e = r[0];
#pragma unroll
    for (int k = 0; k < PM; ++k)
        if (k < P) {
            float acc = r[k + 1];
#pragma unroll
            for (int j = 0; j < PM; ++j)
                if (j < k) acc = fmaf(lp[j], r[k - j], acc);
            const float refl = -div_nr(acc, e);
            e *= 1.0f - refl * refl;
#pragma unroll
            for (int j = 0; j < PM / 2 + 1; ++j)
                if (j < (k + 1) / 2) {
                    const int kj = k - 1 - j;
                    const float s = lp[j], t = lp[kj];
                    lp[j] = fmaf(refl, t, s);
                    if (j != kj) lp[kj] = fmaf(refl, s, t);
                }
            lp[k] = refl;
        }
    // cepstra of the gain-normalised polynomial [1, lp] / (e + 1e-8): c0 = ln(e + 1e-8), then the LPC recursion
    float c[PM + 1];
    c[0] = __builtin_amdgcn_logf(e + 1e-8f) * 0.6931471805599453f;
#pragma unroll
    for (int n = 1; n <= PM; ++n)
        if (n <= P) {
            float acc = 0.f;
#pragma unroll
            for (int m = 1; m < PM + 1; ++m)
                if (m < n) acc = fmaf((float)(n - m) * lp[m - 1], c[n - m], acc);
            c[n] = -fmaf(acc, 1.0f / (float)n, lp[n - 1]);
        }
#pragma unroll
    for (int n = 0; n <= PM; ++n)
        if (n <= P) o[n] = c[n] * lw(n);
}

// fixed sizes: thread = frame, tables in the kernel arguments
template <int NB, int PP>
__global__ __launch_bounds__(128) void plp_cep_fixed_kernel(PlpArgs a, PlpTab<NB, PP> t) {
    const int64_t f = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (f >= a.n_frames) return;
    plp_frame<NB, PP>(a.y + f * NB, a.out + f * (PP + 1), NB, PP, [&](int n) { return t.lq[n]; }, [&](int k, int n) { return t.cw[k * NB + n]; },
                      [&](int n) { return t.lw[n]; });
}

// runtime sizes up to the maxima: tables from LDS
__global__ __launch_bounds__(128) void plp_cep_kernel(PlpArgs a) {
    extern __shared__ float sh[];
    const int nb = a.nb, P = a.P;
    const int n_tab = nb + (P + 1) * nb + (P + 1);
    for (int i = threadIdx.x; i < n_tab; i += 128) sh[i] = a.tab[i];
    __syncthreads();
    const float* lq = sh;
    const float* cw = sh + nb;
    const float* lw = sh + nb + (P + 1) * nb;
    const int64_t f = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (f >= a.n_frames) return;
    plp_frame<PLP_NB_MAX, PLP_P_MAX>(a.y + f * nb, a.out + f * (P + 1), nb, P, [&](int n) { return lq[n]; }, [&](int k, int n) { return cw[k * nb + n]; },
                                     [&](int n) { return lw[n]; });
}

// ---------------------------------------------------------------------------------------------------------------- fused tail
// ssp_plp_features: RASTA -> cepstra -> delta (-> delta delta) -> per-utterance scale -> interleave with a finished "left" block, one
// workgroup per utterance, everything between the log band energies and the output rows in LDS and registers.
//
//   LDS (floats)   red[512] | mean[3 (PP + 1)] | istd[3 (PP + 1)] | ya[T x NB] | ce[T x (PP + 1)] | dd[T x (PP + 1)] (delta_order 2 only)
//                  ya holds the log energies (RASTA in place); once every frame's cepstrum is in ce it is dead and takes the deltas
//                  (rows of PP + 1 <= NB floats).  Row strides 21 / 17 / 13 are odd: lane = frame reads are free of bank conflicts.
//   workgroup      64 ceil(longest utterance / 64) lanes, 64..512 (plp_feat_threads; a longer utterance takes the composed path): lane =
//                  frame in the cepstrum step, lane = element in the others; band b's RASTA recursion runs on lane b
struct PlpFeatArgs {
    const float* x;      // [F x NB] ln critical-band energies
    const float* left;   // [F x left_dim] finished columns, or null
    void* out;           // [F x (left_dim + (1 + delta_order)(PP + 1))] float or double
    const int64_t* off;  // [n_utt + 1] frame offsets
    int32_t left_dim, delta_order, rasta, scale;
};

constexpr int PLP_FEAT_MAX_THREADS = 512;
constexpr size_t PLP_FEAT_LDS_BUDGET = 64 * 1024;  // two workgroups per CU (160 KiB of LDS) with room to spare; no opt-in attribute needed

// regression delta over +-2 frames with edge padding inside the utterance: delta_kernel<2>'s arithmetic (the 0 . c[t] term included)
__device__ __forceinline__ float plp_delta2(const float* __restrict__ c, int t, int d, int T, int dim) {
    const int p1 = min(t + 1, T - 1), p2 = min(t + 2, T - 1), m1 = max(t - 1, 0), m2 = max(t - 2, 0);
    float acc = 0.f * c[t * dim + d];
    const float vp0 = c[p1 * dim + d], vm0 = c[m1 * dim + d], vp1 = c[p2 * dim + d], vm1 = c[m2 * dim + d];
    acc += 1.0f * (vp0 - vm0);
    acc += 2.0f * (vp1 - vm1);
    return acc * (1.0f / 10.0f);
}

// mean and 1 / standard deviation of every column of src[T x dim] (LDS), cmvn_kernel's rules: statistics over the entries that are not
// NaN, mean first, then the variance about it; a deviation below 10 FLT_EPSILON counts as 1.  Lane = (row phase, column); the partial
// sums meet in `red` in a fixed order (no atomics).  Every lane of the workgroup calls it.
__device__ __forceinline__ void plp_col_stats(const float* __restrict__ src, int T, int dim, float* red, float* mean, float* istd, int tid, int nt) {
    const int R = nt / dim, c = tid % dim, ph = tid / dim;
    const bool act = ph < R;
    float s = 0.f, cn = 0.f;
    if (act)
        for (int t = ph; t < T; t += R) {
            const float x = src[t * dim + c];
            const bool ok = x == x;
            s += ok ? x : 0.f;
            cn += ok ? 1.f : 0.f;
        }
    if (act) red[tid] = cn;
    __syncthreads();
    float n_ok = 0.f;
    if (act)
        for (int k = 0; k < R; ++k) n_ok += red[k * dim + c];
    __syncthreads();
    if (act) red[tid] = s;
    __syncthreads();
    if (act && ph == 0) {
        float tot = 0.f;
        for (int k = 0; k < R; ++k) tot += red[k * dim + c];
        mean[c] = tot / n_ok;  // (no entry at all: NaN, as nanmean has it)
    }
    __syncthreads();
    if (act) {
        const float m = mean[c];
        float v = 0.f;
        for (int t = ph; t < T; t += R) {
            const float x = src[t * dim + c];
            const float e = x == x ? x - m : 0.f;
            v = fmaf(e, e, v);
        }
        red[tid] = v;
    }
    __syncthreads();
    if (act && ph == 0) {
        float tot = 0.f;
        for (int k = 0; k < R; ++k) tot += red[k * dim + c];
        float sd = sqrtf(tot / n_ok);
        if (sd < 10.0f * 1.1920929e-07f) sd = 1.0f;
        istd[c] = 1.0f / sd;
    }
    __syncthreads();
}

template <int NB, int PP, class OUT>
__global__ __launch_bounds__(PLP_FEAT_MAX_THREADS) void plp_feat_fixed_kernel(PlpFeatArgs a, PlpTab<NB, PP> tb) {
    constexpr int P1 = PP + 1;
    static_assert(P1 <= NB, "the deltas take the place of the log energies");
    extern __shared__ float sh[];
    const int64_t f0 = a.off[blockIdx.x];
    const int T = (int)(a.off[blockIdx.x + 1] - f0);
    if (T <= 0) return;  // (the whole workgroup)
    const int tid = threadIdx.x, nt = blockDim.x;
    float* red = sh;
    float* mean = red + PLP_FEAT_MAX_THREADS;
    float* istd = mean + 3 * P1;
    float* ya = istd + 3 * P1;
    float* ce = ya + T * NB;
    float* dd = ce + T * P1;  // (delta_order == 2 only: the launch sizes the LDS)
    float* dl = ya;
    // 1. the utterance's log energies
    const float* __restrict__ x = a.x + f0 * NB;
    for (int i = tid; i < T * NB; i += nt) ya[i] = x[i];
    __syncthreads();
    // 2. RASTA along time, in place: plp_rasta_kernel's recursion, band = lane
    if (a.rasta) {
        if (tid < NB) {
            float* p = ya + tid;
            float z0 = 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
#pragma unroll 8
            for (int t = 0; t < T; ++t) {
                const float xv = p[t * NB];
                const float a1 = t < 4 ? 0.f : -0.94f;
                const float out = fmaf(0.2f, xv, z0);
                z0 = fmaf(0.1f, xv, z1) - a1 * out;
                z1 = z2;  // b2 = 0
                z2 = fmaf(-0.1f, xv, z3);
                z3 = -0.2f * xv;
                p[t * NB] = t < 4 ? 0.f : out;
            }
        }
        __syncthreads();
    }
    // 3. lane = frame (the launch has T <= nt): equal loudness ... lifter in registers.  No loop over frames here: inside one the 307
    //    table words are loop invariants, all loaded ahead of it, and most of them then wait in VGPR lanes (300 v_writelane / v_readlane)
    if (tid < T)
        plp_frame<NB, PP>(ya + tid * NB, ce + tid * P1, NB, PP, [&](int n) { return tb.lq[n]; }, [&](int k, int n) { return tb.cw[k * NB + n]; },
                          [&](int n) { return tb.lw[n]; });
    __syncthreads();
    // 4. delta, delta of delta
    if (a.delta_order >= 1) {
        for (int i = tid; i < T * P1; i += nt) dl[i] = plp_delta2(ce, i / P1, i % P1, T, P1);
        __syncthreads();
    }
    if (a.delta_order == 2) {
        for (int i = tid; i < T * P1; i += nt) dd[i] = plp_delta2(dl, i / P1, i % P1, T, P1);
        __syncthreads();
    }
    // 5. per-column statistics of every block
    if (a.scale)
        for (int b = 0; b <= a.delta_order; ++b)
            plp_col_stats(b == 0 ? ce : (b == 1 ? dl : dd), T, P1, red, mean + b * P1, istd + b * P1, tid, nt);
    // 6. the output rows, each written once: for b = 0 .. delta_order: [left block b | PLP block b]
    const int lw = a.left_dim / (1 + a.delta_order), bw = lw + P1, D = (1 + a.delta_order) * bw;
    OUT* __restrict__ o = static_cast<OUT*>(a.out) + f0 * D;
    const float* __restrict__ lf = a.left + f0 * a.left_dim;  // (read only where lw > 0)
    for (int i = tid; i < T * D; i += nt) {
        const int t = i / D, c = i - t * D, b = c / bw, w = c - b * bw;
        float v;
        if (w < lw) {
            v = lf[(int64_t)t * a.left_dim + b * lw + w];
        } else {
            const int d = w - lw;
            v = (b == 0 ? ce : (b == 1 ? dl : dd))[t * P1 + d];
            if (a.scale) v = (v - mean[b * P1 + d]) * istd[b * P1 + d];
        }
        o[i] = (OUT)v;
    }
}

// composed fallback, last step: blk holds 1 + delta_order matrices [F x P1] one after the other (cepstra, delta, delta delta, each
// already scaled when asked for); rows of [left block b | PLP block b] go out, widened exactly for a float64 output
template <class OUT>
__global__ __launch_bounds__(256) void plp_interleave_kernel(const float* __restrict__ blk, const float* __restrict__ left, OUT* __restrict__ out,
                                                             int64_t F, int P1, int left_dim, int delta_order) {
    const int lw = left_dim / (1 + delta_order), bw = lw + P1, D = (1 + delta_order) * bw;
    const int64_t n = F * D;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t f = i / D;
        const int c = (int)(i - f * D), b = c / bw, w = c - b * bw;
        const float v = w < lw ? left[f * left_dim + b * lw + w] : blk[((int64_t)b * F + f) * P1 + (w - lw)];
        out[i] = (OUT)v;
    }
}

// the runtime-sized cepstrum kernel reads its tables from device memory; a device-pointer call may not wait on the host for a copy
// of them, so they travel in kernel arguments, PLP_TAB_CHUNK floats a launch
constexpr int PLP_TAB_CHUNK = 512;
struct PlpTabChunk {
    float v[PLP_TAB_CHUNK];
};
__global__ __launch_bounds__(256) void plp_tab_store_kernel(PlpTabChunk c, float* __restrict__ dst, int n) {
    for (int i = threadIdx.x; i < n; i += 256) dst[i] = c.v[i];
}

int launch_cmvn(const float* in, float* out, const int64_t* frame_off_dev, int64_t n_utt, int dim, int64_t max_T, hipStream_t stream);  // feat_ops.hip
int launch_delta2(const float* in, float* out, const int64_t* frame_off_dev, int64_t n_utt, int dim, int64_t n_rows, hipStream_t stream);

// the limits of the back end, shared by its two entry points
static int plp_check_sizes(const char* fn, int nb, int plp_order) {
    const int P = plp_order - 1;  // plp_order counts c0, as sidekit's argument does
    if (nb < 3 || nb > PLP_NB_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: %d bands (3..%d supported)", fn, nb, PLP_NB_MAX);
    if (P < 1 || P > PLP_P_MAX || P > nb - 1)
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: plp_order=%d needs 1 <= order - 1 <= min(%d, bands - 1)", fn, plp_order, PLP_P_MAX);
    return SSP_OK;
}

// tables (float64 on the host): equal loudness at the band centres, the IDFT weights of the symmetric extension, lifter
static std::vector<float> plp_tables(int nb, int P, float fmax_hz, float lift) {
    std::vector<float> tab((size_t)nb + (size_t)(P + 1) * nb + (P + 1));
    const double zmax = 6.0 * std::asinh((double)fmax_hz / 600.0);
    for (int n = 0; n < nb; ++n) {
        const double hz = 600.0 * std::sinh(zmax * n / (nb - 1) / 6.0), fsq = hz * hz, ft = fsq + 1.6e5;
        const double eql = (fsq / ft) * (fsq / ft) * ((fsq + 1.44e6) / (fsq + 9.61e6));
        tab[n] = eql > 0.0 ? (float)(0.33 * std::log2(eql)) : -INFINITY;  // (the kernel forms (exp(y) eql)^0.33 as exp2(0.33 log2(e) y + this))
    }
    const int N = 2 * (nb - 1);
    for (int k = 0; k <= P; ++k)
        for (int n = 0; n < nb; ++n) {
            double w = std::cos(M_PI * k * n / (nb - 1)) / N;
            if (n > 0 && n < nb - 1) w *= 2.0;
            tab[(size_t)nb + (size_t)k * nb + n] = (float)w;
        }
    for (int n = 0; n <= P; ++n) tab[(size_t)nb + (size_t)(P + 1) * nb + n] = n == 0 || lift == 0.f ? 1.f : (float)std::pow((double)n, (double)lift);
    return tab;
}

template <int NB, int PP>
static PlpTab<NB, PP> plp_fixed_tab(const std::vector<float>& tab) {
    PlpTab<NB, PP> t;
    memcpy(t.lq, tab.data(), sizeof(t.lq));
    memcpy(t.cw, tab.data() + NB, sizeof(t.cw));
    memcpy(t.lw, tab.data() + NB + (PP + 1) * NB, sizeof(t.lw));
    return t;
}

// LDS of one fused workgroup for an utterance of T frames
static size_t plp_feat_lds(int nb, int P1, int delta_order, int64_t T) {
    return ((size_t)PLP_FEAT_MAX_THREADS + 6 * (size_t)P1 + (size_t)T * (size_t)(nb + P1 + (delta_order == 2 ? P1 : 0))) * sizeof(float);
}

// lanes of a fused workgroup: a lane per frame of the call's longest utterance, in whole waves (a batch of 98-frame chunks runs 128-lane
// workgroups, not 256-lane ones with 158 lanes idle through the cepstrum step)
static int plp_feat_threads(int64_t max_T) {
    const int need = (int)(ceil_div<int64_t>(max_T < 1 ? 1 : max_T, 64) * 64);  // (the caller has max_T <= PLP_FEAT_MAX_THREADS)
    if (const char* e = getenv("SSP_PLP_FEATURES_THREADS")) {  // (measurement, tools/bench_plp_features.py: larger workgroups only)
        const int n = atoi(e);
        if (n >= need && n <= PLP_FEAT_MAX_THREADS && n % 64 == 0) return n;
    }
    return need;
}

template <int NB, int PP>
static void launch_plp_feat(const PlpFeatArgs& a, const std::vector<float>& tab, int64_t n_utt, int threads, size_t lds, int out_type, hipStream_t s) {
    const PlpTab<NB, PP> t = plp_fixed_tab<NB, PP>(tab);
    if (out_type == 1) hipLaunchKernelGGL((plp_feat_fixed_kernel<NB, PP, double>), dim3((unsigned)n_utt), dim3(threads), lds, s, a, t);
    else hipLaunchKernelGGL((plp_feat_fixed_kernel<NB, PP, float>), dim3((unsigned)n_utt), dim3(threads), lds, s, a, t);
}

}  // namespace ssp

using namespace ssp;

extern "C" int ssp_plp_features(ssp_ctx* ctx, const float* logspec, const ssp_segments* frame_seg, int32_t n_bands, float fmax_hz,
                                int32_t plp_order, int32_t rasta, float lift, const float* left, int32_t left_dim, int32_t delta_order,
                                int32_t scale, void* feats_out, int out_type, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_plp_features");
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (!frame_seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_plp_features: null segments");
    const int nb = n_bands, P = plp_order - 1, P1 = plp_order;
    SSP_TRY(plp_check_sizes("ssp_plp_features", nb, plp_order));
    if (!(fmax_hz > 0.f)) SSP_FAIL(SSP_ERR_INVALID, "ssp_plp_features: fmax");
    SSP_TRY(check_where(where, "ssp_plp_features"));
    if (out_type != 0 && out_type != 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_plp_features: out_type must be 0 (float32) or 1 (float64)");
    if (delta_order < 0 || delta_order > 2) SSP_FAIL(SSP_ERR_INVALID, "ssp_plp_features: delta_order must be 0, 1 or 2");
    if (left_dim < 0 || left_dim > 4096 || left_dim % (1 + delta_order) != 0)
        SSP_FAIL(SSP_ERR_INVALID, "ssp_plp_features: left_dim=%d must be a multiple of 1 + delta_order = %d (0..4096)", left_dim, 1 + delta_order);
    if (frame_seg->host.front() != 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_plp_features: segments must start at frame 0");
    const int64_t F = frame_seg->total(), n_utt = frame_seg->n, max_T = frame_seg->max_len();
    if (F == 0) return SSP_OK;
    if (!logspec || !feats_out || (left_dim > 0 && !left)) SSP_FAIL(SSP_ERR_INVALID, "ssp_plp_features: null data pointer");
    if (n_utt > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_plp_features: too many utterances");
    const int nblk = 1 + delta_order, D = left_dim + nblk * P1;
    const std::vector<float> tab = plp_tables(nb, P, fmax_hz, lift);
    hipStream_t s = ctx->stream;
    const size_t in_bytes = (size_t)F * nb * sizeof(float), left_bytes = (size_t)F * left_dim * sizeof(float),
                 out_bytes = (size_t)F * D * (out_type == 1 ? sizeof(double) : sizeof(float));
    StageScope st(ctx, where);
    const float* d_x = st.in(logspec, in_bytes);
    const float* d_left = st.in(left_dim > 0 ? left : nullptr, left_bytes);
    void* d_out = st.out(feats_out, out_bytes);
    SSP_TRY(st.status());
    // one path per call, decided on the longest utterance: the fused kernel for the two fixed sizes when that utterance fits the LDS
    // budget, else the existing kernels chained on the stream
    const bool fixed21 = nb == 21 && P == 12, fixed17 = nb == 17 && P == 12;
    const size_t lds = plp_feat_lds(nb, P1, delta_order, max_T);
    const char* force = getenv("SSP_PLP_FEATURES");  // "composed": the fallback for every call (measurement and tests)
    const bool fused = (fixed21 || fixed17) && lds <= PLP_FEAT_LDS_BUDGET && max_T <= PLP_FEAT_MAX_THREADS && !(force && strcmp(force, "composed") == 0);
    const int64_t* d_off = frame_seg->dev.as<int64_t>();
    DevBuf &d_tab = ctx->scratch[0], &d_blk = ctx->scratch[1], &d_y = ctx->scratch[5];
    if (!fused) {  // (before the timer: a scratch buffer that grows frees the old one, which waits for the device)
        SSP_TRY(d_blk.reserve((size_t)nblk * F * P1 * sizeof(float)));
        if (rasta) SSP_TRY(d_y.reserve(in_bytes));
        if (!fixed21 && !fixed17) SSP_TRY(d_tab.reserve(tab.size() * sizeof(float)));
    }
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    if (fused) {
        PlpFeatArgs a{d_x, d_left, d_out, d_off, left_dim, delta_order, rasta ? 1 : 0, scale ? 1 : 0};
        const int threads = plp_feat_threads(max_T);
        if (fixed21) launch_plp_feat<21, 12>(a, tab, n_utt, threads, lds, out_type, s);
        else launch_plp_feat<17, 12>(a, tab, n_utt, threads, lds, out_type, s);
        SSP_HIP(hipGetLastError());
    } else {
        const float* d_in = d_x;
        if (rasta) {
            hipLaunchKernelGGL(plp_rasta_kernel, dim3((unsigned)ceil_div<int64_t>(n_utt * nb, 256)), dim3(256), 0, s, d_x, d_y.as<float>(), d_off, n_utt, nb);
            d_in = d_y.as<float>();
        }
        float* blk = d_blk.as<float>();
        PlpArgs a{d_in, blk, d_tab.as<float>(), F, nb, P};
        const unsigned grid = (unsigned)ceil_div<int64_t>(F, 128);
        if (fixed21) {
            hipLaunchKernelGGL((plp_cep_fixed_kernel<21, 12>), dim3(grid), dim3(128), 0, s, a, plp_fixed_tab<21, 12>(tab));
        } else if (fixed17) {
            hipLaunchKernelGGL((plp_cep_fixed_kernel<17, 12>), dim3(grid), dim3(128), 0, s, a, plp_fixed_tab<17, 12>(tab));
        } else {
            for (size_t i = 0; i < tab.size(); i += PLP_TAB_CHUNK) {
                PlpTabChunk c;
                const int n = (int)std::min<size_t>(PLP_TAB_CHUNK, tab.size() - i);
                memcpy(c.v, tab.data() + i, (size_t)n * sizeof(float));
                hipLaunchKernelGGL(plp_tab_store_kernel, dim3(1), dim3(256), 0, s, c, d_tab.as<float>() + i, n);
            }
            hipLaunchKernelGGL(plp_cep_kernel, dim3(grid), dim3(128), tab.size() * sizeof(float), s, a);
        }
        SSP_HIP(hipGetLastError());
        for (int b = 1; b < nblk; ++b) SSP_TRY(launch_delta2(blk + (size_t)(b - 1) * F * P1, blk + (size_t)b * F * P1, d_off, n_utt, P1, F, s));
        if (scale)
            for (int b = 0; b < nblk; ++b) SSP_TRY(launch_cmvn(blk + (size_t)b * F * P1, blk + (size_t)b * F * P1, d_off, n_utt, P1, max_T, s));
        const unsigned g2 = (unsigned)std::min<int64_t>(ceil_div<int64_t>(F * D, 256), (int64_t)ctx->num_cu * 16);
        if (out_type == 1) hipLaunchKernelGGL(plp_interleave_kernel<double>, dim3(g2), dim3(256), 0, s, blk, d_left, (double*)d_out, F, P1, left_dim, delta_order);
        else hipLaunchKernelGGL(plp_interleave_kernel<float>, dim3(g2), dim3(256), 0, s, blk, d_left, (float*)d_out, F, P1, left_dim, delta_order);
        SSP_HIP(hipGetLastError());
    }
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}

extern "C" int ssp_plp_post(ssp_ctx* ctx, const float* logspec, const ssp_segments* frame_seg, int32_t n_bands, float fmax_hz,
                            int32_t plp_order, int32_t rasta, float lift, float* ceps_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_plp_post");
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (!frame_seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_plp_post: null segments");
    const int nb = n_bands, P = plp_order - 1;  // plp_order counts c0, as sidekit's argument does
    SSP_TRY(plp_check_sizes("ssp_plp_post", nb, plp_order));
    if (!(fmax_hz > 0.f)) SSP_FAIL(SSP_ERR_INVALID, "ssp_plp_post: fmax");
    SSP_TRY(check_where(where, "ssp_plp_post"));
    if (frame_seg->host.front() != 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_plp_post: segments must start at frame 0");
    const int64_t F = frame_seg->total();
    if (F == 0) return SSP_OK;
    if (!logspec || !ceps_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_plp_post: null data pointer");
    const std::vector<float> tab = plp_tables(nb, P, fmax_hz, lift);
    hipStream_t s = ctx->stream;
    DevBuf &d_tab = ctx->scratch[0], &d_y = ctx->scratch[5];
    SSP_TRY(d_tab.reserve(tab.size() * sizeof(float)));
    SSP_HIP(hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, s));
    SSP_HIP(hipStreamSynchronize(s));  // `tab` (host) dies at return
    const size_t in_bytes = (size_t)F * nb * sizeof(float), out_bytes = (size_t)F * (P + 1) * sizeof(float);
    StageScope st(ctx, where);
    const float* d_x = st.in(logspec, in_bytes);
    float* d_out = st.out(ceps_out, out_bytes);
    SSP_TRY(st.status());
    const float* d_in = d_x;
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    if (rasta) {
        SSP_TRY(d_y.reserve(in_bytes));
        const int64_t n_thr = frame_seg->n * nb;
        hipLaunchKernelGGL(plp_rasta_kernel, dim3((unsigned)ceil_div<int64_t>(n_thr, 256)), dim3(256), 0, s, d_x, d_y.as<float>(),
                           frame_seg->dev.as<int64_t>(), frame_seg->n, nb);
        d_in = d_y.as<float>();
    }
    PlpArgs a{d_in, d_out, d_tab.as<float>(), F, nb, P};
    const size_t lds = tab.size() * sizeof(float);
    const unsigned grid = (unsigned)ceil_div<int64_t>(F, 128);
    if (nb == 21 && P == 12) hipLaunchKernelGGL((plp_cep_fixed_kernel<21, 12>), dim3(grid), dim3(128), 0, s, a, plp_fixed_tab<21, 12>(tab));
    else if (nb == 17 && P == 12) hipLaunchKernelGGL((plp_cep_fixed_kernel<17, 12>), dim3(grid), dim3(128), 0, s, a, plp_fixed_tab<17, 12>(tab));
    else hipLaunchKernelGGL(plp_cep_kernel, dim3(grid), dim3(128), lds, s, a);
    SSP_HIP(hipGetLastError());
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}
