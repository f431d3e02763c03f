// VAD threshold search (the objective of VAD.py's optimize, :189-220): for every (utterance, threshold triple) the counts that the F1
// score of VAD_detection against frame labels is made of — tp = |mark & label|, fp = |mark & ~label|, fn = |~mark & label| — in ONE
// launch for thousands of triples.  `mark` is what vad_detect_kernel (vad.hip) writes for that triple: both kernels run the state
// machine of vad_machine.hpp.  No mask leaves the device.
//
// vad_sweep_kernel — one WAVE per (utterance, triple), W waves of a workgroup on W neighbouring triples of one utterance:
//   * the label plane (label != 0 as 64-frame ballot words) is built once per workgroup, each wave a share of it, and read by all W;
//   * every wave builds its own loud (power > amph) and active (power > ampl or zcr > zcr_gate) planes from coalesced reads of the
//     utterance's zcr / power planes (which every triple re-reads: they stay in L2), 64 ballots at a time — lane k keeps the k-th word,
//     then one 512-byte LDS store per plane — zeroes its mark plane and runs vad_mark_runs on them;
//   * tp / fp / fn are popcounts over the words, lane-parallel, summed across the wave with integer adds;
//   * lanes 0..2 store the three int32 of (triple, utterance).
// Word planes live in dynamic LDS, (1 + 3 W) planes of ceil(longest utterance / 64) words: W = 4 up to 40 320 frames (16 384 frames
// — the detector's 64 VAD_LDS_WORDS — take 26 KiB), 2 up to 74 880, 1 up to SWEEP_MAX_FRAMES = 131 072 (64 KiB).  Planes are whole
// 16-byte multiples apart; the wave-uniform reads of the state machine broadcast and the lane-parallel ones are unit stride.
// Mode 1 (VAD_frequency with a list of thresholds): mark = !(entropy > thr) needs no plane of its own, the ballot meets the label word.
// Comparisons only, no atomics: the counts do not depend on the launch shape.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "vad_machine.hpp"

namespace ssp {
namespace {

constexpr int SWEEP_WAVES = 4;
constexpr int64_t SWEEP_MAX_FRAMES = 131072;  // 4 planes of 2048 words = 64 KiB
constexpr size_t SWEEP_LDS_BYTES = 65536;

struct SweepArgs {
    const float* zcr;
    const float* pw;
    const uint8_t* lab;
    const int64_t* foff;
    const float* thr;  // [3][n_par]: zcr_gate, ampl, amph (mode 1: ampl only, at [n_par, 2 n_par))
    int32_t* counts;   // [n_par][n_utt][3]
    int n_utt, n_par, mode, min_len;
    int nwp;           // words per plane
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(64 * SWEEP_WAVES) void vad_sweep_kernel(SweepArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t sweep_words[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W = blockDim.x >> 6;
    uint64_t* const Y = sweep_words;
    uint64_t* const L = sweep_words + (size_t)a.nwp * (1 + 3 * wave);  // (mode 1 has the label plane only and never forms these)
    uint64_t* const A = L + a.nwp;
    uint64_t* const M = A + a.nwp;
    const int n_groups = (a.n_par + W - 1) / W;
    const int64_t n_items = (int64_t)a.n_utt * n_groups;
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int u = (int)(item / n_groups);
        const int q = (int)(item - (int64_t)u * n_groups) * W + wave;  // this wave's triple
        const bool live = q < a.n_par;
        const int64_t f0 = a.foff[u];
        const int T = (int)(a.foff[u + 1] - f0);
        const int nw = (T + 63) >> 6;
        // ---- the label plane, 64 words to a wave
        for (int c = wave; c * 64 < nw; c += W) {
            const int wlim = nw - c * 64 < 64 ? nw - c * 64 : 64;
            uint64_t mine = 0;
#pragma unroll 4
            for (int k = 0; k < wlim; ++k) {
                const int i = (c * 64 + k) * 64 + lane;
                const uint64_t b = __builtin_amdgcn_ballot_w64(i < T && a.lab[f0 + i] != 0);
                if (lane == k) mine = b;
            }
            if (lane < wlim) Y[c * 64 + lane] = mine;
        }
        float gate = 0.f, lo = 0.f, hi = 0.f;
        if (live) {
            lo = a.thr[a.n_par + q];
            if (a.mode == 0) {
                gate = a.thr[q];
                hi = a.thr[2 * a.n_par + q];
                for (int c = 0; c * 64 < nw; ++c) {
                    const int wlim = nw - c * 64 < 64 ? nw - c * 64 : 64;
                    uint64_t loud = 0, act = 0;
#pragma unroll 4
                    for (int k = 0; k < wlim; ++k) {
                        const int i = (c * 64 + k) * 64 + lane;
                        const float p = i < T ? a.pw[f0 + i] : 0.f, z = i < T ? a.zcr[f0 + i] : 0.f;
                        const uint64_t bl = __builtin_amdgcn_ballot_w64(i < T && p > hi);
                        const uint64_t ba = __builtin_amdgcn_ballot_w64(i < T && (p > lo || z > gate));
                        if (lane == k) loud = bl, act = ba;
                    }
                    if (lane < wlim) {
                        L[c * 64 + lane] = loud;
                        A[c * 64 + lane] = act;
                        M[c * 64 + lane] = 0;
                    }
                }
            }
        }
        __syncthreads();  // the label plane is whole (and this wave's own planes are visible to all its lanes)
        if (live) {
            int tp = 0, fp = 0, fn = 0;
            if (a.mode == 0) {
                vad_mark_runs(L, A, M, T, a.min_len, lane);
                for (int w = lane; w < nw; w += 64) {
                    const uint64_t m = M[w], y = Y[w];
                    tp += __builtin_popcountll(m & y);
                    fp += __builtin_popcountll(m & ~y);
                    fn += __builtin_popcountll(~m & y);
                }
                tp = wave_sum(tp), fp = wave_sum(fp), fn = wave_sum(fn);
            } else {  // 0 where entropy > thr, else 1 (a NaN entropy compares false: 1, as numpy.where gives)
                for (int w = 0; w < nw; ++w) {
                    const int i = w * 64 + lane;
                    const uint64_t m = __builtin_amdgcn_ballot_w64(i < T && !(a.pw[f0 + i] > lo));
                    const uint64_t y = ldw(Y + w);
                    tp += __builtin_popcountll(m & y);
                    fp += __builtin_popcountll(m & ~y);
                    fn += __builtin_popcountll(~m & y);
                }
            }
            if (lane < 3) a.counts[((int64_t)q * a.n_utt + u) * 3 + lane] = lane == 0 ? tp : (lane == 1 ? fp : fn);
        }
        __syncthreads();  // (the next item rewrites the planes)
    }
}

}  // namespace
}  // namespace ssp

using namespace ssp;

extern "C" {

int ssp_vad_sweep(ssp_ctx* ctx, const float* zcr, const float* power_or_entropy, const uint8_t* labels, const ssp_segments* frame_seg,
                  int32_t mode, int32_t n_par, const float* zcr_gate, const float* ampl, const float* amph, int32_t min_len,
                  int32_t* counts_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_vad_sweep");
    if (mode != 0 && mode != 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_sweep: mode must be 0 (VAD_detection) or 1 (VAD_frequency)");
    SSP_TRY(check_where(where, "ssp_vad_sweep"));
    if (n_par < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_sweep: n_par must be >= 1");
    if (min_len < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_sweep: min_len must be >= 1");
    if (!ampl || (mode == 0 && (!zcr_gate || !amph))) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_sweep: null threshold array");
    if (!ctx || !frame_seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_sweep: null ctx or segments");
    if (kernel_ms) *kernel_ms = 0.f;
    const int64_t n_utt = frame_seg->n;
    if (n_utt == 0) return SSP_OK;
    if (!counts_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_sweep: null counts_out");
    if (frame_seg->total() > 0 && (!power_or_entropy || !labels || (mode == 0 && !zcr))) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_sweep: null data pointer");
    if (frame_seg->max_len() > SWEEP_MAX_FRAMES)
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_vad_sweep: an utterance of %lld frames; the limit is %lld frames per utterance", (long long)frame_seg->max_len(),
                 (long long)SWEEP_MAX_FRAMES);
    if (n_utt > INT32_MAX || (int64_t)n_par * n_utt * 3 > ((int64_t)1 << 31))
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_vad_sweep: counts_out would hold more than 2^31 entries (%lld triples x %lld utterances x 3)", (long long)n_par,
                 (long long)n_utt);
    SSP_TRY(use_ctx(ctx));
    hipStream_t s = ctx->stream;

    // waves per workgroup: as many triples of one utterance side by side as the word planes leave room for
    const int nwp = std::max<int>(2, (int)(((frame_seg->max_len() + 63) / 64 + 1) & ~(int64_t)1));
    int W = 1;
    size_t lds = (size_t)nwp * sizeof(uint64_t);
    if (mode == 0) {
        for (W = SWEEP_WAVES; W > 1 && (size_t)(1 + 3 * W) * nwp * sizeof(uint64_t) > SWEEP_LDS_BYTES; W >>= 1) {
        }
        W = std::min<int>(W, n_par);
        lds = (size_t)(1 + 3 * W) * nwp * sizeof(uint64_t);
    } else {
        W = std::min<int>(SWEEP_WAVES, n_par);
    }

    // the thresholds: host arrays, uploaded as [3][n_par] (they are the caller's: the one host wait of the call lets them go)
    DevBuf& d_thr = ctx->scratch[4];
    SSP_TRY(d_thr.reserve((size_t)n_par * 3 * sizeof(float)));
    const size_t tb = (size_t)n_par * sizeof(float);
    if (mode == 0) {
        SSP_HIP(hipMemcpyAsync(d_thr.as<float>(), zcr_gate, tb, hipMemcpyHostToDevice, s));
        SSP_HIP(hipMemcpyAsync(d_thr.as<float>() + 2 * (size_t)n_par, amph, tb, hipMemcpyHostToDevice, s));
    }
    SSP_HIP(hipMemcpyAsync(d_thr.as<float>() + n_par, ampl, tb, hipMemcpyHostToDevice, s));
    SSP_HIP(hipStreamSynchronize(s));

    const size_t n_all = (size_t)frame_seg->host.back(), n_out = (size_t)n_par * (size_t)n_utt * 3 * sizeof(int32_t);
    StageScope st(ctx, where);
    const float *d_z = st.in(mode == 0 ? zcr : nullptr, n_all * sizeof(float)), *d_p = st.in(power_or_entropy, n_all * sizeof(float));
    const uint8_t* d_l = st.in(labels, n_all);
    int32_t* d_c = st.out(counts_out, n_out);
    SSP_TRY(st.status());

    SweepArgs a;
    a.zcr = d_z;
    a.pw = d_p;
    a.lab = d_l;
    a.foff = frame_seg->dev.as<int64_t>();
    a.thr = d_thr.as<float>();
    a.counts = d_c;
    a.n_utt = (int)n_utt;
    a.n_par = (int)n_par;
    a.mode = (int)mode;
    a.min_len = (int)min_len;
    a.nwp = nwp;
    const int64_t n_items = n_utt * ceil_div<int64_t>(n_par, W);
    const int grid = (int)std::min<int64_t>(n_items, (int64_t)ctx->num_cu * 8);
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    hipLaunchKernelGGL(vad_sweep_kernel, dim3(grid), dim3(64 * W), lds, s, a);
    SSP_HIP(hipGetLastError());
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}

}  // extern "C"
