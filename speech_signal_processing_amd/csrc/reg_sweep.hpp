// What the register-resident streaming sweeps share (cosine_reg_kernel in cosine.hip, plda_score_kernel in plda.hip): a wave keeps 32
// vectors in registers as the MFMA B operand, and 32-row tile images of the other side stream through a ring of half-tile LDS slots by
// LDS-DMA.  Image layout of a tile: [q8][h][row 32][e 4] = v[row][8 q8 + 2 e + h], NQ * 256 floats, zero padded.
#pragma once
#include <hip/hip_runtime.h>

namespace ssp {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

struct __attribute__((packed, aligned(4))) f4u {  // 16-byte load at dword alignment (rows of any length)
    float x, y, z, w;
};

constexpr int SWEEP_XS_FLOATS = 32 * 65;  // a wave's staging area: [32 rows][64 + 1 pad]

// B operand of this wave: b[q8][e] = x[row fl][8 q8 + 2 e + h] for its 32 rows, staged through `xs` (this wave's SWEEP_XS_FLOATS of LDS)
// in 64-wide k chunks so the HBM reads stay coalesced: 32 rows x 64 floats of a chunk = 512 float4, 8 per lane, all in flight together.
// row_ptr(r) -> the first element of row r of the wave (any 4-byte alignment), or nullptr past the end (the row is then zeros);
// each(v) sees every value this lane keeps.
template <int NQ, class RowPtr, class Each>
__device__ __forceinline__ void sweep_load_operand(float (&b)[NQ][4], float* xs, int lane, int d, RowPtr row_ptr, Each each) {
    const int fl = lane & 31, h = lane >> 5;
#pragma unroll
    for (int kc = 0; kc < NQ / 8; ++kc) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = lane + 64 * u, r = idx >> 4, k = kc * 64 + 4 * (idx & 15);
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            const float* __restrict__ row = row_ptr(r);
            if (row) {
                const float* __restrict__ p = row + k;
                if (k + 3 < d) {
                    const f4u t4 = *reinterpret_cast<const f4u*>(p);
                    v[u] = make_float4(t4.x, t4.y, t4.z, t4.w);
                } else {
                    if (k < d) v[u].x = p[0];
                    if (k + 1 < d) v[u].y = p[1];
                    if (k + 2 < d) v[u].z = p[2];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = lane + 64 * u, r = idx >> 4, c = 4 * (idx & 15);
            float* dst = xs + r * 65 + c;
            dst[0] = v[u].x;
            dst[1] = v[u].y;
            dst[2] = v[u].z;
            dst[3] = v[u].w;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q8 = 0; q8 < 8; ++q8)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x = xs[fl * 65 + 8 * q8 + 2 * e + h];
                b[kc * 8 + q8][e] = x;
                each(x);
            }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// one half tile (NQ * 128 floats) from the image into an LDS slot by LDS-DMA: NQ / 2 pieces of 256 floats, dealt over the four waves
template <int NQ>
__device__ __forceinline__ void sweep_stage_half(const float* src, float* dst, int wave, int lane) {
#pragma unroll
    for (int p = 0; p < (NQ / 2 + 3) / 4; ++p) {
        const int piece = wave + 4 * p;
        if (piece < NQ / 2) __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src + piece * 256 + lane * 4), (lds_ptr_t)(dst + piece * 256), 16, 0, 0);
    }
}

}  // namespace ssp
