// Device helpers shared by the neural kernels (dense.hip, dnn_chain.hip, dnn_train.hip, lstm.hip, lstm_train.hip, gru.hip, gru_train.hip):
// the MFMA accumulator type, the dword-aligned 16-byte load and Keras' gate activations with their derivatives.  One definition each, so
// that the forward kernels and the trainers cannot drift apart.
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

}  // namespace ssp
