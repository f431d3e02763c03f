// Device helpers shared by the neural kernels (dense.hip, dnn_chain.hip, dnn_train.hip, lstm.hip, lstm_train.hip, gru.hip, gru_train.hip):
// the MFMA accumulator type, the dword-aligned 16-byte load, Keras' gate activations with their derivatives and the trainers' split-K
// output tile.  One definition each, so that the forward kernels and the trainers cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

namespace ssp {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// 16-byte load at dword alignment (rows of any length)
struct __attribute__((packed, aligned(4))) f4u {
    float x, y, z, w;
};

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float sigm(float z) { return __builtin_amdgcn_rcpf(1.f + ex2(-1.44269504088896341f * z)); }
__device__ __forceinline__ float tanh_hw(float z) { return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + ex2(2.88539008177792681f * z)); }
__device__ __forceinline__ float hard_sigm(float z) { return fminf(fmaxf(0.2f * z + 0.5f, 0.f), 1.f); }
// the recurrent activation: ACT = 0 hard_sigmoid | 1 sigmoid
template <int ACT>
__device__ __forceinline__ float gate(float z) {
    return ACT == 0 ? hard_sigm(z) : sigm(z);
}
// its derivative from the fp32 activation s: Keras' clip passes no gradient at or beyond the bounds
template <int ACT>
__device__ __forceinline__ float dgate(float s) {
    return ACT == 0 ? ((s > 0.f && s < 1.f) ? 0.2f : 0.f) : s * (1.f - s);
}

// ---- the 16 x 16 split-K output tile of the trainers' GEMMs (dnn_train.hip dt_gemm_kernel, gru_train.hip gt_gemm_tn_kernel): 256 threads,
// K in FIXED quarters over the four waves, every wave one ascending chain on v_mfma_f32_16x16x4_f32, the four partial tiles added in
// wave order.  The partition and the order of the sum depend on K alone: that is what makes the trainers' bits reproducible.
struct SplitK {
    int kbeg, kend;  // this wave's quarter of K (rounded up to 16; empty past the end)
};
__device__ __forceinline__ SplitK splitk_range(int K, int wave) {
    const int kchunk = (((K + 3) / 4 + 15) / 16) * 16;
    const int kbeg = wave * kchunk;
    return {kbeg, kbeg + kchunk < K ? kbeg + kchunk : K};
}

// this wave's partial tile.  load(kb, av, bv): the operands of the 16-k block at kb for lane (kq, i) = (lane >> 4, lane & 15), av[r] =
// A[m0 + i][kb + 4 kq + r], bv[r] = B[kb + 4 kq + r][n0 + i], zero at and past kend and beyond the matrices.  Two register sets: the
// loads of the blocks at kb + 32 and kb + 48 are issued before the MFMAs of the blocks at kb and kb + 16, so two blocks' round trips to
// L2 are in flight under the products (k still accumulates in ascending order: the same bits)
template <class Load>
__device__ __forceinline__ f32x4 splitk_walk(SplitK k, Load&& load) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float a0[4], b0[4], a1[4], b1[4];
    load(k.kbeg, a0, b0);
    load(k.kbeg + 16, a1, b1);
    for (int kb = k.kbeg; kb < k.kend; kb += 32) {
        float a2[4], b2[4], a3[4], b3[4];
        load(kb + 32, a2, b2);
        load(kb + 48, a3, b3);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[r], b0[r], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[r], b1[r], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) a0[r] = a2[r], b0[r] = b2[r], a1[r] = a3[r], b1[r] = b3[r];
    }
    return acc;
}

// the four waves' partial tiles meet in `red` (each wave stores its tile 16 bytes per lane: lane (kq, i) register r = element (4 kq + r,
// i)) and thread tid leaves with element (row, col) = (tid >> 4, tid & 15) of their sum, added in wave order
struct SplitKElem {
    int row, col;
    float v;
};
__device__ __forceinline__ SplitKElem splitk_sum(float (&red)[4][256], f32x4 acc, int tid, int wave) {
    *reinterpret_cast<f32x4*>(&red[wave][(tid & 63) * 4]) = acc;
    __syncthreads();
    const int row = tid >> 4, col = tid & 15;
    const int e = ((row >> 2) * 16 + col) * 4 + (row & 3);
    return {row, col, ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e]};
}

}  // namespace ssp
