// The 128 x 128 x 32 staged fp32 GEMM block on v_mfma_f32_32x32x2_f32 that dense_kernel (dense.hip) and tdnn_kernel (xvector.hip) share:
// C[unit][row] = sum_k A[unit][k] B[row][k], both operands row-major in global memory, 256 threads = 2 x 2 waves of 64 units x 64 rows.
// One definition each of the tile constants, the clipped buffer resource, the slab load, the operand-image store, the product of one
// 128-unit block and the epilogue's walk; a kernel hands in how its two operand streams advance (a callable that loads the stream's
// NEXT slab) and how an output element is finished.
//
// A [128 x 32] slab of a row-major matrix goes global -> registers -> MFMA operand image [q = 4][h = 2] planes of [row = 128][e = 4]
// (element (row, k = 8 q + 2 e + h)) in two steps: the loads of a later slab are issued before the MFMAs of the current one and land
// under them.  The loads are branch-free 16-byte buffer loads through a resource that covers exactly the rows the workgroup may read
// (what lies outside reads as zero; rows of 98 x 13 = 1274 floats are only 8-byte aligned, which buffer loads allow); the columns past
// the row's end inside the last slab are cleared in registers.  (Per-load bounds branches cut the k-loop into ~20 basic blocks and kept
// the compiler from placing any load among the MFMAs.)
#pragma once
#include <hip/hip_runtime.h>

#include "nn_device.hpp"

namespace ssp {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int G128_BM = 128;  // units per block step
constexpr int G128_BN = 128;  // rows (samples, frames) per workgroup
constexpr int G128_BK = 32;   // k-slab
constexpr int G128_PL = 128 * 4 + 4;  // floats per (q, h) plane of the operand image: 128 rows x 4 + 4 pad, so that the 8 planes the
                                      // 16 lanes of a ds_write_b64 group touch start on different banks (unpadded: 4-way conflicts)
constexpr int G128_SLAB = (G128_BK / 8) * 2 * G128_PL;                // floats of one slab's operand image
constexpr size_t G128_LDS = (size_t)4 * G128_SLAB * sizeof(float);    // two slabs of two operand images: 66 KB of dynamic LDS

// rows [row0, row0 + n_rows) of a row-major matrix of d floats a row, clipped to the matrix: what lies outside reads as zero
__device__ __forceinline__ __amdgpu_buffer_rsrc_t g128_rsrc(const float* A, int64_t row0, int64_t total_rows, int64_t n_rows, int d) {
    const int64_t rows = total_rows - row0 < n_rows ? total_rows - row0 : n_rows;
    const uint64_t addr = reinterpret_cast<uint64_t>(A + row0 * d);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)addr), hi = __builtin_amdgcn_readfirstlane((uint32_t)(addr >> 32));
    const int bytes = __builtin_amdgcn_readfirstlane((int)(rows > 0 ? rows * d * 4 : 0));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(((uint64_t)hi << 32) | lo), 0, bytes, 0x00020000);
}

// a [128 x 32] slab, columns [k0, k0 + 32) of rows of d floats: row r of the slab is `stride` floats after row r - 1 and column 0 is
// `base` floats into row 0.  Columns at and past d (the next row's, or a neighbouring block of a wider row) are cleared in registers;
// a slab that is not `live` is all zeros, as is one whose every offset is out of range (slabs past the last one)
__device__ __forceinline__ void g128_load(__amdgpu_buffer_rsrc_t rs, int stride, int base, int d, int k0, bool live, int tid, float4 (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + i * 256;
        const int r = idx >> 3, c4 = idx & 7;
        const int k = k0 + c4 * 4;
        // (the whole vector is bit-cast before any element is taken: element reads straight off the builtin's result are narrowed
        //  to a one-dword load by this compiler)
        const f32x4 t = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (live && k < d) ? (r * stride + base + k) * 4 : 0x7ffffff0, 0, 0));
        v[i].x = t.x;
        v[i].y = k + 1 < d ? t.y : 0.f;
        v[i].z = k + 2 < d ? t.z : 0.f;
        v[i].w = k + 3 < d ? t.w : 0.f;
    }
}

__device__ __forceinline__ void g128_store(float* __restrict__ img, int tid, const float4 (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + i * 256;
        const int r = idx >> 3, c4 = idx & 7;
        const int q = c4 >> 1, e0 = (c4 & 1) * 2;
        *reinterpret_cast<float2*>(img + (size_t)(q * 2 + 0) * G128_PL + r * 4 + e0) = make_float2(v[i].x, v[i].z);
        *reinterpret_cast<float2*>(img + (size_t)(q * 2 + 1) * G128_PL + r * 4 + e0) = make_float2(v[i].y, v[i].w);
    }
}

// acc = the product of one 128-unit block over n_slab slabs, ONE k-ordered chain per output: the four waves split the 128 x 128 tile
// and never the k range.  load_a(v) / load_b(v) load the NEXT slab of the unit stream / the row stream into v and advance the stream;
// they are called n_slab + 1 and n_slab + 2 times, and a stream past its last slab must deliver zeros.
// `img` holds two slabs of each operand image: slab s + 1 is written (from registers loaded one or two steps earlier) in the middle of
// the MFMAs of slab s, so a k-step costs ONE workgroup barrier and no wave waits on a store it has just issued (3.25 -> 2.95 ms on the
// 1274-wide d-vector input layer at 5e5 samples against store, barrier, MFMAs, barrier on a single buffer).  Register staging: the unit
// stream (weights: L2 resident) runs one slab ahead of the LDS image, the row stream (HBM, a TLB miss away) two.
template <class LoadA, class LoadB>
__device__ __forceinline__ void g128_product(float* img, int n_slab, int tid, LoadA&& load_a, LoadB&& load_b, f32x16 (&acc)[2][2]) {
    float* imgA = img;                  // units [2][G128_SLAB]
    float* imgB = img + 2 * G128_SLAB;  // rows  [2][G128_SLAB]
    const int lane = tid & 63, wave = tid >> 6;
    const int fl = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;  // 2 x 2 waves, each 64 units x 64 rows
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rt][ct][i] = 0.f;
    float4 va[4], vp[4], vq[4];
    load_a(va);
    load_b(vq);
    load_b(vp);
    __syncthreads();  // the previous unit block's last slab is consumed
    g128_store(imgA, tid, va);
    g128_store(imgB, tid, vq);
    load_a(va);
    load_b(vq);
    __syncthreads();
    // step s: MFMAs on image s & 1; `vn` holds row slab s + 1 and is refilled with slab s + 3 once stored
    auto slab = [&](int s, float4 (&vn)[4]) {
        const float* cA = imgA + (s & 1) * G128_SLAB;
        const float* cB = imgB + (s & 1) * G128_SLAB;
#pragma unroll
        for (int q = 0; q < G128_BK / 8; ++q) {
            if (q == G128_BK / 16 && s + 1 < n_slab) {
                g128_store(imgA + ((s + 1) & 1) * G128_SLAB, tid, va);
                g128_store(imgB + ((s + 1) & 1) * G128_SLAB, tid, vn);
                load_a(va);
                load_b(vn);
            }
            f32x4 av[2], bv[2];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
                av[rt] = *reinterpret_cast<const f32x4*>(cA + (size_t)(q * 2 + h) * G128_PL + (wr * 64 + rt * 32 + fl) * 4);
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
                bv[ct] = *reinterpret_cast<const f32x4*>(cB + (size_t)(q * 2 + h) * G128_PL + (wc * 64 + ct * 32 + fl) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[rt][e], bv[ct][e], acc[rt][ct], 0, 0, 0);
        }
        __syncthreads();  // image s is consumed, image s + 1 is complete
    };
    for (int s = 0; s < n_slab; s += 2) {
        slab(s, vp);
        if (s + 1 < n_slab) slab(s + 1, vq);
    }
}

// bias and ReLU of one output element.  (Not fmaxf: a NaN stays a NaN, as under np.maximum; -0 -> +0)
__device__ __forceinline__ float g128_bias_relu(float t, const float* bias, int relu, int unit) {
    if (bias) t += bias[unit];
    if (relu) t = t <= 0.f ? 0.f : t;
    return t;
}

// the block's outputs to Y [N x units]: accumulator register i of a lane = unit (i & 3) + 8 (i >> 2) + 4 h of the 32-unit tile, row fl,
// so four consecutive units leave in one 16-byte store where the row pitch and Y allow it.  finish(unit, t) -> the stored value of
// every unit below `units`
template <class Finish>
__device__ __forceinline__ void g128_epilogue(const f32x16 (&acc)[2][2], float* Y, int64_t N, int units, int64_t col0, int rb, int tid,
                                              Finish&& finish) {
    const int lane = tid & 63, wave = tid >> 6;
    const int fl = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
    const bool vst = (units & 3) == 0 && (reinterpret_cast<uintptr_t>(Y) & 15) == 0;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int64_t gc = col0 + wc * 64 + ct * 32 + fl;
        if (gc >= N) continue;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) {
                const int row = rb * G128_BM + wr * 64 + rt * 32 + 8 * i4 + 4 * h;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = acc[rt][ct][i4 * 4 + e];
                    if (row + e < units) t = finish(row + e, t);
                    v[e] = t;
                }
                float* y = Y + gc * units + row;
                if (vst && row + 3 < units) {
                    *reinterpret_cast<float4*>(y) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (row + e < units) y[e] = v[e];
                }
            }
    }
}

}  // namespace ssp
