// The 32 x 32 log-probability tile of the diagonal-GMM MFMA kernels: lp[mixture][frame] = W[mixture][0 .. 2D] . aug[frame], aug = [x, x^2,
// 1, 0], on v_mfma_f32_32x32x2_f32.  ONE definition for the E pass (gmm_em.hip em_mfma_body), the log-sum-exp pass (em_lse_mfma_body) and
// the UBM selection of top-C scoring (gmm_map.hip gmm_map_select_kernel): lp - lse in the unfused EM route is the difference of two
// evaluations of this one formula in this one k order, and the selection ranks the values the dense scorer would.
#pragma once
#include <hip/hip_runtime.h>

namespace ssp {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// values that are uniform per wave, read through readfirstlane: a persistent walk whose bounds the compiler cannot prove uniform may
// be rebuilt as a loop over lane masks (tests/test_isa_guards.py)
__device__ __forceinline__ int em_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t em_uniform64(int64_t v) {
    const uint64_t u = (uint64_t)v;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(u >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// the augmented tile of 64 frames, xs[r * XS + c] = [x, x^2, 1, 0][c] of frame base + r for c < 2 KS (rows at and past nt: x = 0), with
// wave-uniform trip counts; 256 threads
__device__ __forceinline__ void em_stage_aug(float* xs, const float* __restrict__ x, int64_t base, int nt, int D, int KS, int XS) {
    const int tid = threadIdx.x;
    for (int i0 = 0; i0 < 64 * 2 * KS; i0 += 256) {
        const int i = i0 + tid;
        if (i < 64 * 2 * KS) {
            const int r = i / (2 * KS), c = i - r * (2 * KS);
            float v = c == 2 * D ? 1.f : 0.f;
            if (c < 2 * D) {
                const int cd = c < D ? c : c - D;
                const float xv = r < nt ? x[(base + r) * D + cd] : 0.f;
                v = c < D ? xv : xv * xv;
            }
            xs[r * XS + c] = v;
        }
    }
}

// one wave's tile: A[row = this lane's mixture][k = 2 s + h] = wcol[2 s WS] (wcol = the k-major parameter image of row stride WS at row
// h, this lane's mixture), B[k = 2 s + h][col = this lane's frame] = xrow[2 s + h] (xrow = the frame's row of the augmented tile), KS
// k-steps in ascending order in one accumulator, four steps' operands in flight
template <int WS>
__device__ __forceinline__ f32x16 em_lp_tile(const float* xrow, const float* wcol, int KS, int h) {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    int s2 = 0;
    for (; s2 + 3 < KS; s2 += 4) {
        float av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            av[u] = wcol[(2 * (s2 + u)) * WS];
            bv[u] = xrow[2 * (s2 + u) + h];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
    }
    for (; s2 < KS; ++s2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wcol[(2 * s2) * WS], xrow[2 * s2 + h], acc, 0, 0, 0);
    return acc;
}

// accumulator register i of a lane of half h = this mixture of the 32-mixture tile (ascending in i), of the lane's frame
__device__ __forceinline__ int em_lp_mix(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

}  // namespace ssp
