// The dense trainer's step kernels (dnn_train.hip: dt_gemm_kernel modes 0 / 1 / 2, dt_loss_kernel, dt_adam_kernel) as plain launches.  Every
// trainer queues its loss and its Adam update through them (trainer_core.hpp), the dense trainer included; the recurrent trainers also
// run their Dense heads and their weight gradients over the stash on the GEMM.  The kernels and their arithmetic live in dnn_train.hip;
// these only fill the argument blocks.  Every pointer is a device pointer, every launch goes on `s` without a host wait.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ssp {

// mode 0: C[M x N] = A[M x K] B[K x N] + bias (rows of A through idx when given; lda = A's row stride)
// mode 1: C[M x N] = A[M x K] B^T, B stored [N x K]
// mode 2: C[M x N] = A^T B with A stored [K x M] (row stride lda), B [K x N]; db (nullable) = the column sums of B.  K is split over four
//         waves into fixed quarters added in wave order
int dt_launch_gemm(int mode, const float* A, const float* B, float* C, const int64_t* idx, int32_t M, int32_t N, int32_t K, int64_t lda,
                   const float* bias, float* db, hipStream_t s);
// softmax cross-entropy of Z[B x C] (gradient (softmax - onehot) / B written in place when write_grad), the label of row r is
// labels[idx ? idx[r] : r]; the batch's loss sum and count of correct rows land in *loss_slot / *corr_slot
int dt_launch_loss(float* Z, const int32_t* labels, const int64_t* idx, int32_t B, int32_t C, int write_grad, float* rowloss, int32_t* rowcorr,
                   uint32_t* ticket, float* loss_slot, int32_t* corr_slot, hipStream_t s);
// Keras 2's Adam at step t1 (counted from 1) over flat buffers of n floats
int dt_launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, int64_t t1, hipStream_t s);

}  // namespace ssp
