// Voice activity detection: the per-frame features of the reference's VAD.py (enframe :28-50 without window or pre-emphasis, energy
// :67-76, ZCR :53-64, spectrum_entropy :79-105, feature :108-119, wavdata's peak normalisation :131) for a ragged batch of utterances as
// ONE pass, and its two detectors (VAD_detection :136-182, VAD_frequency :185-186) as one wave per utterance.
//
// vad_feature_kernel — every WAVE walks its own chunk (a run of frames of one utterance, a multiple of 8 frames from the utterance's
// start), eight frames at a time, 16 lanes per PAIR of frames, no workgroup barrier (the layout of mfcc_stream_kernel.hpp):
//   * the 8 frames' samples (8 step + 256 - step of them: frames overlap by half, every sample is fetched once) arrive by LDS-DMA, float32
//     or int16 as they are; the next eight frames' DMA flies under the arithmetic of these;
//   * two real frames per complex transform: z[n] = a[n] + i b[n], 256 points = radix 16 x radix 16 through a swizzled LDS transpose
//     (cplx.hpp); |A[k]|^2 = |Z[k] + conj Z[256 - k]|^2 / 4 and |B[k]|^2 = |Z[k] - conj Z[256 - k]|^2 / 4 need no twiddle, and only
//     squared magnitudes are ever used (no square root);
//   * energy = sum of squares in the time domain; zero crossings from the SIGNS of neighbouring samples (two ballots per 16-sample row:
//     no product that could underflow, a zero sample makes no crossing);
//   * the peak of wavdata (:131) is folded in AFTERWARDS: the transform runs on the samples as they are and the frame's energy, block
//     energies and total are multiplied by 1 / peak^2 before the > 0.1 gate and the two 1e-8 terms are applied, i.e. in the scaled
//     domain.  The peak itself comes from vad_peak_kernel, a pre-pass that writes one float per utterance.  peak = 0 (digital silence):
//     1 / peak^2 = inf and 0 . inf = NaN for energy and entropy, zcr 0 — the reference's 0 / 0; the zero padding behind an utterance's
//     end never meets the scale, it stays 0.
// vad_detect_kernel — one wave per utterance: coalesced reads of 64 frames, the loud (power > amph) and active (power > ampl or
// zcr > zcr_gate) predicates as ballot words, the reference's sequential state machine on those words (find next set / clear bit
// instead of a frame loop), the mark words written out as a coalesced uint8 mask.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "cplx.hpp"
#include "vad_machine.hpp"

namespace ssp {
namespace {

constexpr int VAD_FRAME = 256;
constexpr int VAD_WAVES = 4;
constexpr int VAD_IMG = 2048;       // per 16-lane group: transpose image (16 rows of 128 B), afterwards the two frames' 128 power bins
constexpr int VAD_CHUNK_MAX = 1024;  // frames per chunk at most
constexpr int VAD_LDS_WORDS = 256;  // detect kernel: utterances up to 64 x this many frames keep their predicate words in LDS

struct VadChunk {
    int32_t utt, t0, n, pad;
};

struct VadArgs {
    const void* samples;
    const int64_t* sample_off;
    const int64_t* frame_off;
    const VadChunk* chunks;
    int n_chunks;
    const float* peak;   // per utterance max |x| (null: samples are taken as they are)
    const v2f* tw;       // W_256^(k1 j) at [k1 * 16 + j]
    float* zcr;
    float* power;
    float* entropy;
    int step;            // 128 | 256
    int need;            // bytes of one eight-frame stage (a multiple of 16)
    int wave_bytes;      // LDS per wave: 4 images + the stage
    float gate;          // zcr is kept where power > gate (0.1, VAD.py:112; -inf: the bare count of ZCR, VAD.py:53-64)
};

// sum over the 16 lanes of a row, the same bits on every lane (each step adds two values that both lanes of the pair hold)
__device__ __forceinline__ float row_sum16(float x) {
    x += __builtin_amdgcn_update_dpp(0.f, x, 0xB1 /*quad_perm 1,0,3,2*/, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0.f, x, 0x4E /*quad_perm 2,3,0,1*/, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0.f, x, 0x141 /*row_half_mirror*/, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0.f, x, 0x140 /*row_mirror*/, 0xF, 0xF, true);
    return x;
}

template <int P, int NP>
__device__ __forceinline__ void vad_dma_pieces(const __amdgpu_buffer_rsrc_t& rs, uint32_t stage_lds, uint32_t vo, int lane, int need) {
    if constexpr (P < NP) {
        // 1-KiB pieces: the instruction offset advances the global and the LDS address together (12 bits: a second base above 4 KiB)
        if (P * 1024 + lane * 16 < need)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(uintptr_t)(stage_lds + (P >= 4 ? 4096 : 0)), 16, (int)(vo + (P >= 4 ? 4096u : 0u)), 0,
                                                     (P & 3) * 1024, 0);
        vad_dma_pieces<P + 1, NP>(rs, stage_lds, vo, lane, need);
    }
}

// I16: samples are int16 PCM (utils.tools.read), taken at their integer value
template <int I16>
__global__ __launch_bounds__(64 * VAD_WAVES, 3) void vad_feature_kernel(VadArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, j = lane & 15;
    constexpr int ES = I16 ? 2 : 4;

    char* img = smem + wave * a.wave_bytes;
    char* stage = img + 4 * VAD_IMG;
    const uint32_t stage_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_ptr_t)stage);
    v2f twr[15];
#pragma unroll
    for (int k1 = 1; k1 < 16; ++k1) twr[k1 - 1] = a.tw[k1 * 16 + j];
    const int step = a.step, need = a.need;

    for (int cidx = blockIdx.x * VAD_WAVES + wave; cidx < a.n_chunks; cidx += gridDim.x * VAD_WAVES) {
        const VadChunk ch = a.chunks[cidx];
        const int utt = __builtin_amdgcn_readfirstlane(ch.utt);
        const int64_t s0 = a.sample_off[utt];
        const int64_t N = a.sample_off[utt + 1] - s0;
        const int64_t f0 = a.frame_off[utt];
        const int t0 = __builtin_amdgcn_readfirstlane(ch.t0), tend = __builtin_amdgcn_readfirstlane(ch.t0 + ch.n);
        const int nq = (tend - t0 + 7) >> 3;
        float c2 = 1.f;  // 1 / peak^2 (wavdata, VAD.py:131)
        if (a.peak) {
            const float r = __builtin_amdgcn_rcpf(a.peak[utt]);
            c2 = r * r;
        }
        // the utterance as a buffer: reads behind its end come back as zero (enframe's zero padding, VAD.py:38-47).  int16 data may
        // start on an odd sample: the buffer starts at the dword below (sh = 1: every stage index moves up by one) and ends at the dword
        // that holds the last sample — the one foreign sample that dword may carry behind the end is zeroed in the stage
        const uint64_t xaddr = reinterpret_cast<uint64_t>(static_cast<const char*>(a.samples) + s0 * ES);
        const int sh = I16 ? (int)((xaddr >> 1) & 1) : 0;
        const uint64_t xbase = I16 ? (xaddr & ~(uint64_t)3) : xaddr;
        const uint32_t xlo = __builtin_amdgcn_readfirstlane((uint32_t)xbase), xhi = __builtin_amdgcn_readfirstlane((uint32_t)(xbase >> 32));
        const int xbytes = __builtin_amdgcn_readfirstlane(I16 ? (int)((((N + sh) * 2) + 3) & ~(int64_t)3) : (int)(N * 4));
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(((uint64_t)xhi << 32) | xlo), 0, xbytes, 0x00020000);
        auto prefetch = [&](int q) {
            // (unsigned: an utterance of nearly 2^29 float32 samples puts the last pieces' offsets above 2^31)
            const uint32_t vo = (uint32_t)(t0 + 8 * q) * (uint32_t)(step * ES) + (uint32_t)lane * 16u;
            vad_dma_pieces<0, 8>(rs, stage_lds, vo, lane, need);
        };
        prefetch(0);
        for (int q = 0; q < nq; ++q) {
            const int tb0 = t0 + 8 * q;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stage has landed (and the last iteration's stores have left)
            v2f z[16];
            if (I16) {
                const int64_t e = N - (int64_t)tb0 * step + sh;  // stage index of the first sample behind the utterance
                if (((N + sh) & 1) && e * 2 < need && lane == 0) reinterpret_cast<int16_t*>(stage)[e] = 0;
                const int16_t* sp = reinterpret_cast<const int16_t*>(stage) + sh + 2 * g * step + j;
#pragma unroll
                for (int n1 = 0; n1 < 16; ++n1) z[n1] = v2f{(float)sp[16 * n1], (float)sp[step + 16 * n1]};
            } else {
                const float* sp = reinterpret_cast<const float*>(stage) + 2 * g * step + j;
#pragma unroll
                for (int n1 = 0; n1 < 16; ++n1) z[n1] = v2f{sp[16 * n1], sp[step + 16 * n1]};
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the stage is in registers: the next eight frames may overwrite it
            if (q + 1 < nq) prefetch(q + 1);                     // flies under this whole iteration

            // ---- energy (VAD.py:67-76) of both frames
            v2f acc = v2f{0.f, 0.f};
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) acc = __builtin_elementwise_fma(z[n1], z[n1], acc);
            const float pw_a = row_sum16(acc.x) * c2, pw_b = row_sum16(acc.y) * c2;

            // ---- zero crossings (VAD.py:53-64): pairs (n, n + 1), n = j + 16 n1, whose signs are opposite.  Bit l of a ballot = lane l:
            // lane j and lane j + 1 of a row hold neighbours; lane 15's neighbour is lane 0 of the next row (bit 15 of the group stands for it)
            unsigned cnt_a = 0, cnt_b = 0;
            {
                constexpr uint64_t IN_ROW = 0x7FFF7FFF7FFF7FFFull, TO_NEXT = 0x8000800080008000ull;
                uint64_t nNa = 0, nPa = 0, nNb = 0, nPb = 0;
#pragma unroll
                for (int n1 = 15; n1 >= 0; --n1) {
                    const uint64_t Na = __builtin_amdgcn_ballot_w64(z[n1].x < 0.f), Pa = __builtin_amdgcn_ballot_w64(z[n1].x > 0.f);
                    const uint64_t Nb = __builtin_amdgcn_ballot_w64(z[n1].y < 0.f), Pb = __builtin_amdgcn_ballot_w64(z[n1].y > 0.f);
                    const uint64_t ca = (((Na & (Pa >> 1)) | (Pa & (Na >> 1))) & IN_ROW) | (((Na & (nPa << 15)) | (Pa & (nNa << 15))) & TO_NEXT);
                    const uint64_t cb = (((Nb & (Pb >> 1)) | (Pb & (Nb >> 1))) & IN_ROW) | (((Nb & (nPb << 15)) | (Pb & (nNb << 15))) & TO_NEXT);
                    cnt_a += (unsigned)((ca >> lane) & 1);
                    cnt_b += (unsigned)((cb >> lane) & 1);
                    nNa = Na, nPa = Pa, nNb = Nb, nPb = Pb;
                }
            }
            const float zc_a = row_sum16((float)cnt_a), zc_b = row_sum16((float)cnt_b);

            // ---- 256-point transform of z = a + i b: FFT16 over n1, twiddle W_256^(j k1), transpose through LDS, FFT16 over n2
            fft16(z);
#pragma unroll
            for (int k1 = 1; k1 < 16; ++k1) z[k1] = cmul(z[k1], twr[k1 - 1]);
            char* zf = img + g * VAD_IMG;
            {   // rows of 128 B, 16-byte chunks XOR-swizzled by (row >> 1) & 7 (mfcc_fast.hip)
                int wb0 = ((j >> 1) << 4) | ((j & 1) << 3);
                asm volatile("" : "+v"(wb0));
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    char* wp = zf + (wb0 ^ (m << 4));
                    *reinterpret_cast<v2f*>(wp + (2 * m) * 128) = z[2 * m];
                    *reinterpret_cast<v2f*>(wp + (2 * m + 1) * 128) = z[2 * m + 1];
                }
                int rb0 = j * 128 + (((j >> 1) & 7) << 4);
                asm volatile("" : "+v"(rb0));
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const v4f r = *reinterpret_cast<const v4f*>(zf + (rb0 ^ (c << 4)));
                    z[2 * c] = v2f{r.x, r.y};
                    z[2 * c + 1] = v2f{r.z, r.w};
                }
            }
            fft16(z);  // lane j, register k2: Z[j + 16 k2]
            // ---- the two frames' power bins 0..127 (k = j + 16 k2, k2 < 8); partner Z[256 - k] sits on lane 16 - j, register 15 - k2
            // (lane 0: its own register 16 - k2): row_mirror, then row_shr:1 with `old`.  Odd groups' rows start 64 B later: the two groups
            // of a half-wave then write different banks
            float* Pa = reinterpret_cast<float*>(zf + (g & 1) * 64);
            float* Pb = Pa + 256;
#pragma unroll
            for (int k2 = 0; k2 < 8; ++k2) {
                const float sx = z[15 - k2].x, sy = z[15 - k2].y;
                const v2f own = z[(16 - k2) & 15];
                float mx = __builtin_amdgcn_update_dpp(sx, sx, 0x140 /*row_mirror*/, 0xF, 0xF, true);
                float my = __builtin_amdgcn_update_dpp(sy, sy, 0x140 /*row_mirror*/, 0xF, 0xF, true);
                mx = __builtin_amdgcn_update_dpp(own.x, mx, 0x111 /*row_shr:1*/, 0xF, 0xF, false);
                my = __builtin_amdgcn_update_dpp(own.y, my, 0x111 /*row_shr:1*/, 0xF, 0xF, false);
                const v2f m = v2f{mx, my};
                const v2f ea = __builtin_elementwise_fma(m, v2f{1.f, -1.f}, z[k2]);   // 2 A[k]
                const v2f eb = __builtin_elementwise_fma(m, v2f{-1.f, 1.f}, z[k2]);   // 2 i B[k]
                Pa[j + 16 * k2] = 0.25f * __builtin_fmaf(ea.x, ea.x, ea.y * ea.y);
                Pb[j + 16 * k2] = 0.25f * __builtin_fmaf(eb.x, eb.x, eb.y * eb.y);
            }
            // ---- spectral entropy (VAD.py:79-92): lane b < 10 sums block b = bins 12 b .. 12 b + 11, lane 10 the bins 120..127 that only
            // the total holds
            float ent_a, ent_b;
            {
                const int jb = j < 10 ? j : 10;
                const v4f* ra = reinterpret_cast<const v4f*>(Pa) + 3 * jb;
                const v4f* rb = reinterpret_cast<const v4f*>(Pb) + 3 * jb;
                const v4f a0 = ra[0], a1 = ra[1], a2 = ra[2], b0 = rb[0], b1 = rb[1], b2 = rb[2];  // (lane 10's third quad lies behind the row, inside the image; unused)
                const float ha = ((a0.x + a0.y) + (a0.z + a0.w)) + ((a1.x + a1.y) + (a1.z + a1.w)), ta = (a2.x + a2.y) + (a2.z + a2.w);
                const float hb = ((b0.x + b0.y) + (b0.z + b0.w)) + ((b1.x + b1.y) + (b1.z + b1.w)), tb = (b2.x + b2.y) + (b2.z + b2.w);
                const float sa = j < 10 ? ha + ta : 0.f, sb = j < 10 ? hb + tb : 0.f;
                const float Ea = row_sum16(j < 10 ? ha + ta : (j == 10 ? ha : 0.f)) * c2;
                const float Eb = row_sum16(j < 10 ? hb + tb : (j == 10 ? hb : 0.f)) * c2;
                const float qa = (sa * c2) * __builtin_amdgcn_rcpf(Ea + 1e-8f), qb = (sb * c2) * __builtin_amdgcn_rcpf(Eb + 1e-8f);
                const float la = qa * __builtin_amdgcn_logf(qa + 1e-8f), lb = qb * __builtin_amdgcn_logf(qb + 1e-8f);  // v_log_f32 = log2
                ent_a = -row_sum16(j < 10 ? la : 0.f);
                ent_b = -row_sum16(j < 10 ? lb : 0.f);
            }
            // ---- lanes 0 / 1 of each group store the pair's frames: three stores of eight consecutive floats per wave
            const int t = tb0 + 2 * g + j;
            if (j < 2 && t < tend) {
                const float pw = j ? pw_b : pw_a, zc = j ? zc_b : zc_a;
                a.power[f0 + t] = pw;
                a.zcr[f0 + t] = pw > a.gate ? zc : 0.f;  // zcr * (power > 0.1), VAD.py:112
                a.entropy[f0 + t] = j ? ent_b : ent_a;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the next chunk's DMA overwrites the stage)
    }
}

// max |x| per utterance (wavdata, VAD.py:131), int16 widened first (|-32768| = 32768).  Grid (utterance, piece); non-negative floats order
// like their bit patterns, so the pieces meet in an unsigned atomic max.  V: elements per 16-byte load (1: the array is not 16-byte aligned).
template <typename T, int V>
__global__ __launch_bounds__(256) void vad_peak_kernel(const T* __restrict__ x, const int64_t* __restrict__ off, int64_t piece, unsigned* __restrict__ peak_bits) {
    __shared__ float red[4];
    const int u = blockIdx.x;
    const int64_t s0 = off[u], s1 = off[u + 1];
    const int64_t a = s0 + (int64_t)blockIdx.y * piece, b = a + piece < s1 ? a + piece : s1;
    if (a >= b) return;
    float m = 0.f;
    if constexpr (V == 1) {
        for (int64_t i = a + threadIdx.x; i < b; i += 256) m = fmaxf(m, fabsf((float)x[i]));
    } else {
        struct alignas(16) Vec {
            T v[V];
        };
        // whole 16-byte groups of the array; elements outside [a, b) are masked (a group that straddles b lies inside the page that holds b - 1)
        for (int64_t gi = a / V + threadIdx.x; gi * V < b; gi += 256) {
            const Vec w = reinterpret_cast<const Vec*>(x)[gi];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int64_t i = gi * V + k;
                m = fmaxf(m, (i >= a && i < b) ? fabsf((float)w.v[k]) : 0.f);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(peak_bits + u, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

// ---- detectors -------------------------------------------------------------------------------------------------------------------
// (ldw / vad_next / vad_prev_clear and the state machine itself, vad_mark_runs: vad_machine.hpp, shared with vad_sweep.hip)
// mode 0: VAD_detection (VAD.py:136-182) on (zcr, power); mode 1: VAD_frequency (VAD.py:185-186) on the entropy with threshold `ampl`.
// gwords: three planes of `plane` words for utterances longer than 64 VAD_LDS_WORDS frames (null when there is none).
__global__ __launch_bounds__(64 * VAD_WAVES) void vad_detect_kernel(const float* __restrict__ zcr, const float* __restrict__ pw,
                                                                    const int64_t* __restrict__ foff, int n_utt, int mode, float zcr_gate,
                                                                    float ampl, float amph, int min_len, uint8_t* __restrict__ mask,
                                                                    int32_t* __restrict__ n_speech, uint64_t* gwords, int64_t plane) {
    __shared__ uint64_t words[VAD_WAVES][3][VAD_LDS_WORDS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int u = blockIdx.x * VAD_WAVES + wave; u < n_utt; u += gridDim.x * VAD_WAVES) {
        const int64_t f0 = foff[u];
        const int T = (int)(foff[u + 1] - f0);
        int count = 0;
        if (mode == 1) {  // 0 where entropy > 0.4, else 1 (a NaN entropy compares false: 1, as numpy.where gives)
            for (int base = 0; base < T; base += 64) {
                const int i = base + lane;
                const bool sp = i < T && !(pw[f0 + i] > ampl);
                if (i < T) mask[f0 + i] = sp ? 1 : 0;
                count += __builtin_popcountll(__builtin_amdgcn_ballot_w64(sp));
            }
            if (lane == 0 && n_speech) n_speech[u] = count;
            continue;
        }
        const int nw = (T + 63) >> 6;
        uint64_t *L, *A, *M;
        if (nw <= VAD_LDS_WORDS) {
            L = words[wave][0], A = words[wave][1], M = words[wave][2];
        } else {  // (utterance u's words start at floor(first frame / 64) + u: room for ceil(T / 64) before the next one's)
            const int64_t o = ((f0 - foff[0]) >> 6) + u;
            L = gwords + o, A = gwords + plane + o, M = gwords + 2 * plane + o;
        }
        for (int base = 0; base < T; base += 64) {
            const int i = base + lane;
            const float p = i < T ? pw[f0 + i] : 0.f, z = i < T ? zcr[f0 + i] : 0.f;
            const uint64_t loud = __builtin_amdgcn_ballot_w64(i < T && p > amph);
            const uint64_t act = __builtin_amdgcn_ballot_w64(i < T && (p > ampl || z > zcr_gate));
            if (lane == 0) {
                L[base >> 6] = loud;
                A[base >> 6] = act;
                M[base >> 6] = 0;
            }
        }
        __threadfence_block();
        vad_mark_runs(L, A, M, T, min_len, lane);  // the reference's sequential loop as bit searches on the words
        for (int base = 0; base < T; base += 64) {
            const int i = base + lane;
            const uint64_t m = ldw(M + (base >> 6));
            if (i < T) mask[f0 + i] = (uint8_t)((m >> lane) & 1);
            count += __builtin_popcountll(m);
        }
        if (lane == 0 && n_speech) n_speech[u] = count;
        __threadfence_block();  // (the next utterance rewrites the words)
    }
}

int vad_check_step(const char* who, int32_t frame_size, int32_t step) {
    if (frame_size < 1 || step < 1) SSP_FAIL(SSP_ERR_INVALID, "%s: frame_size and step must be positive", who);
    if (frame_size != VAD_FRAME || (step != 128 && step != 256))
        SSP_FAIL(SSP_ERR_UNSUPPORTED, "%s: frame_size 256 with step 128 or 256 only (got %d / %d)", who, (int)frame_size, (int)step);
    return SSP_OK;
}

}  // namespace
}  // namespace ssp

using namespace ssp;

extern "C" {

int ssp_vad_num_frames(int64_t n_samples, int32_t step, int64_t* n_frames) {
    if (n_samples < 0 || step < 1 || !n_frames) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_num_frames: bad argument");
    *n_frames = (n_samples + step - 1) / step;  // math.ceil(wlen / step), VAD.py:37
    return SSP_OK;
}

int ssp_vad_frame_segments(ssp_ctx* ctx, const ssp_segments* sample_seg, int32_t step, ssp_segments** frame_seg_out) {
    if (!ctx || !sample_seg || !frame_seg_out || step < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_frame_segments: bad argument");
    std::vector<int64_t> off((size_t)sample_seg->n + 1, 0);
    for (int64_t u = 0; u < sample_seg->n; ++u)
        off[(size_t)u + 1] = off[(size_t)u] + (sample_seg->host[(size_t)u + 1] - sample_seg->host[(size_t)u] + step - 1) / step;
    return segments_make(ctx, off.data(), sample_seg->n, frame_seg_out);
}

int ssp_vad_features(ssp_ctx* ctx, const void* samples, int sample_type, const ssp_segments* sample_seg, const ssp_segments* frame_seg,
                     int32_t frame_size, int32_t step, int32_t normalize, uint32_t flags, float* zcr_out, float* power_out, float* entropy_out, int where,
                     float* kernel_ms) {
    ssp::TraceRange trace_("ssp_vad_features");
    if (!ctx || !sample_seg || !frame_seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_features: null ctx or segments");
    if (sample_type != 0 && sample_type != 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_features: sample_type must be 0 (float32) or 1 (int16)");
    SSP_TRY(check_where(where, "ssp_vad_features"));
    SSP_TRY(vad_check_step("ssp_vad_features", frame_size, step));
    if (flags & ~(uint32_t)SSP_VAD_ZCR_UNGATED) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_features: unknown flag bits %#x", (unsigned)flags);
    if (sample_seg->n != frame_seg->n) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_features: sample and frame segments differ in count");
    const int64_t n_utt = sample_seg->n;
    for (int64_t u = 0; u < n_utt; ++u) {
        const int64_t N = sample_seg->host[(size_t)u + 1] - sample_seg->host[(size_t)u], T = frame_seg->host[(size_t)u + 1] - frame_seg->host[(size_t)u];
        if (T != (N + step - 1) / step)
            SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_features: utterance %lld has %lld frames in frame_seg, ceil(%lld / %d) expected", (long long)u,
                     (long long)T, (long long)N, (int)step);
        if (N >= ((int64_t)1 << 29)) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_vad_features: utterance %lld is longer than 2^29 samples", (long long)u);
    }
    if (kernel_ms) *kernel_ms = 0.f;
    const int64_t total_frames = frame_seg->total();
    if (total_frames == 0) return SSP_OK;
    if (!samples || !zcr_out || !power_out || !entropy_out) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_features: null data pointer");
    if (n_utt > INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_vad_features: too many utterances");
    SSP_TRY(use_ctx(ctx));
    hipStream_t s = ctx->stream;
    const size_t es = sample_type ? 2 : 4;

    // chunks: runs of whole eight-frame groups from each utterance's start (a frame's place in its pair and group, and with it every bit
    // of its features, does not depend on how the batch is cut), sized so that a machine-filling number of waves has work
    int64_t per = ceil_div<int64_t>(total_frames, (int64_t)ctx->num_cu * 12);
    per = std::min<int64_t>(VAD_CHUNK_MAX, std::max<int64_t>(8, ceil_div<int64_t>(per, 8) * 8));
    std::vector<VadChunk> chunks;
    for (int64_t u = 0; u < n_utt; ++u) {
        const int64_t T = frame_seg->host[(size_t)u + 1] - frame_seg->host[(size_t)u];
        for (int64_t t0 = 0; t0 < T; t0 += per) chunks.push_back({(int32_t)u, (int32_t)t0, (int32_t)std::min<int64_t>(per, T - t0), 0});
    }
    if (chunks.size() > (size_t)INT32_MAX) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_vad_features: batch too large for one launch");
    static const std::vector<float> tw = [] {   // W_256^(k1 j); lives as long as the library: its upload needs no host wait
        std::vector<float> t(512);
        for (int k1 = 0; k1 < 16; ++k1)
            for (int j = 0; j < 16; ++j) {
                const double ang = -2.0 * M_PI * (double)(k1 * j) / 256.0;
                t[(size_t)(k1 * 16 + j) * 2] = (float)std::cos(ang);
                t[(size_t)(k1 * 16 + j) * 2 + 1] = (float)std::sin(ang);
            }
        return t;
    }();
    DevBuf &d_chunks = ctx->scratch[0], &d_tw = ctx->scratch[1], &d_peak = ctx->scratch[2];
    SSP_TRY(d_chunks.reserve(chunks.size() * sizeof(VadChunk)));
    SSP_TRY(d_tw.reserve(tw.size() * sizeof(float)));
    const bool norm = normalize != 0;
    if (norm) SSP_TRY(d_peak.reserve((size_t)n_utt * sizeof(float)));
    SSP_HIP(hipMemcpyAsync(d_chunks.p, chunks.data(), chunks.size() * sizeof(VadChunk), hipMemcpyHostToDevice, s));
    SSP_HIP(hipMemcpyAsync(d_tw.p, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice, s));
    SSP_HIP(hipStreamSynchronize(s));  // `chunks` (host) dies at return

    const size_t in_bytes = (size_t)sample_seg->host.back() * es, out_bytes = (size_t)frame_seg->host.back() * sizeof(float);
    StageScope st(ctx, where);
    const void* d_in = st.in(samples, in_bytes);
    float *d_z = st.out(zcr_out, out_bytes), *d_p = st.out(power_out, out_bytes), *d_e = st.out(entropy_out, out_bytes);
    SSP_TRY(st.status());

    VadArgs a;
    a.samples = d_in;
    a.sample_off = sample_seg->dev.as<int64_t>();
    a.frame_off = frame_seg->dev.as<int64_t>();
    a.chunks = d_chunks.as<VadChunk>();
    a.n_chunks = (int)chunks.size();
    a.peak = norm ? d_peak.as<float>() : nullptr;
    a.gate = (flags & SSP_VAD_ZCR_UNGATED) ? -INFINITY : 0.1f;
    a.tw = d_tw.as<v2f>();
    a.zcr = d_z;
    a.power = d_p;
    a.entropy = d_e;
    a.step = step;
    a.need = (int)((((size_t)(8 * step + VAD_FRAME - step) * es + (sample_type ? 4 : 0)) + 15) & ~(size_t)15);
    a.wave_bytes = 4 * VAD_IMG + a.need;
    const size_t lds = (size_t)VAD_WAVES * a.wave_bytes;
    const int grid = (int)std::min<int64_t>(ceil_div<int64_t>((int64_t)chunks.size(), VAD_WAVES), (int64_t)ctx->num_cu * 3);

    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    if (norm) {
        SSP_HIP(hipMemsetAsync(d_peak.p, 0, (size_t)n_utt * sizeof(float), s));
        const int64_t max_len = sample_seg->max_len();
        const int64_t piece = std::max<int64_t>(16384, ceil_div<int64_t>(max_len, 64));
        const dim3 pg((unsigned)n_utt, (unsigned)std::max<int64_t>(1, ceil_div<int64_t>(max_len, piece)));
        const bool al = (reinterpret_cast<uintptr_t>(d_in) & 15) == 0;
        unsigned* pk = d_peak.as<unsigned>();
        const int64_t* so = sample_seg->dev.as<int64_t>();
        if (sample_type) {
            if (al) hipLaunchKernelGGL((vad_peak_kernel<int16_t, 8>), pg, dim3(256), 0, s, (const int16_t*)d_in, so, piece, pk);
            else hipLaunchKernelGGL((vad_peak_kernel<int16_t, 1>), pg, dim3(256), 0, s, (const int16_t*)d_in, so, piece, pk);
        } else {
            if (al) hipLaunchKernelGGL((vad_peak_kernel<float, 4>), pg, dim3(256), 0, s, (const float*)d_in, so, piece, pk);
            else hipLaunchKernelGGL((vad_peak_kernel<float, 1>), pg, dim3(256), 0, s, (const float*)d_in, so, piece, pk);
        }
        SSP_HIP(hipGetLastError());
    }
    if (sample_type) hipLaunchKernelGGL(vad_feature_kernel<1>, dim3(grid), dim3(64 * VAD_WAVES), lds, s, a);
    else hipLaunchKernelGGL(vad_feature_kernel<0>, dim3(grid), dim3(64 * VAD_WAVES), lds, s, a);
    SSP_HIP(hipGetLastError());
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}

int ssp_vad_detect(ssp_ctx* ctx, const float* zcr, const float* power_or_entropy, const ssp_segments* frame_seg, int32_t mode, float zcr_gate,
                   float ampl, float amph, int32_t min_len, uint8_t* mask_out, int32_t* n_speech_out, int where, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_vad_detect");
    if (!ctx || !frame_seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_detect: null ctx or segments");
    if (mode != 0 && mode != 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_detect: mode must be 0 (VAD_detection) or 1 (VAD_frequency)");
    SSP_TRY(check_where(where, "ssp_vad_detect"));
    if (mode == 0 && min_len < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_detect: min_len must be >= 1");
    if (kernel_ms) *kernel_ms = 0.f;
    const int64_t n_utt = frame_seg->n;
    if (n_utt == 0) return SSP_OK;
    if (frame_seg->total() > 0 && (!power_or_entropy || (mode == 0 && !zcr) || !mask_out)) SSP_FAIL(SSP_ERR_INVALID, "ssp_vad_detect: null data pointer");
    if (n_utt > INT32_MAX || frame_seg->max_len() > INT32_MAX - 64) SSP_FAIL(SSP_ERR_UNSUPPORTED, "ssp_vad_detect: batch too large");
    SSP_TRY(use_ctx(ctx));
    hipStream_t s = ctx->stream;
    const size_t n_all = (size_t)frame_seg->host.back();
    StageScope st(ctx, where);
    const float *d_z = st.in(mode == 0 ? zcr : nullptr, n_all * sizeof(float)), *d_p = st.in(power_or_entropy, n_all * sizeof(float));
    uint8_t* d_m = st.out(mask_out, n_all);
    int32_t* d_n = st.out(n_speech_out, (size_t)n_utt * sizeof(int32_t));
    SSP_TRY(st.status());
    uint64_t* gw = nullptr;
    int64_t plane = 0;
    if (mode == 0 && frame_seg->max_len() > (int64_t)64 * VAD_LDS_WORDS) {
        plane = frame_seg->total() / 64 + n_utt + 1;
        SSP_TRY(ctx->scratch[3].reserve((size_t)plane * 3 * sizeof(uint64_t)));
        gw = ctx->scratch[3].as<uint64_t>();
    }
    const int grid = (int)std::min<int64_t>(ceil_div<int64_t>(n_utt, VAD_WAVES), (int64_t)ctx->num_cu * 8);
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    hipLaunchKernelGGL(vad_detect_kernel, dim3(grid), dim3(64 * VAD_WAVES), 0, s, d_z, d_p, frame_seg->dev.as<int64_t>(), (int)n_utt, (int)mode,
                       zcr_gate, ampl, amph, (int)min_len, d_m, d_n, gw, plane);
    SSP_HIP(hipGetLastError());
    SSP_TRY(tm.stop(s, kernel_ms));
    return st.finish();
}

}  // extern "C"
