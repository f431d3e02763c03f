// What the network trainers (dnn_train.hip, lstm_train.hip, gru_train.hip) share on the host: the flat parameter / gradient / Adam
// buffers, the per-step loss slots, the validation and staging of one epoch or evaluation, and the events of a timed step.  Host code
// only: every kernel stays in its trainer's file, and the loss and Adam launches are the dense trainer's (dnn_train.hpp).
#pragma once
#include <vector>

#include "common.hpp"
#include "dnn_train.hpp"
#include "handle.hpp"

namespace ssp {

// Base of every trainer handle.  A step's loss sum and correct-row count land in slot `step index within the call`.
struct TrainerCore {
    ssp_ctx* ctx = nullptr;
    int32_t max_batch = 0, n_class = 0;
    int64_t n_params = 0, t = 0;  // t: steps taken over the whole fit (Adam's and the dropout's counter)
    DevBuf P, G, Mo, Vo;          // parameters, last step's gradients, Adam's moments: one flat buffer each
    DevBuf rowloss, rowcorr, ticket, slot_loss, slot_corr, order;

    int slots(int64_t n) {
        SSP_TRY(slot_loss.reserve((size_t)n * sizeof(float)));
        SSP_TRY(slot_corr.reserve((size_t)n * sizeof(int32_t)));
        return SSP_OK;
    }

    // the upload of `flat`, the other flat buffers, the loss buffers and 4096 slots (an epoch of up to 4096 steps allocates nothing), and
    // the memsets, queued on the ctx stream.  No host wait: the create's commit waits once, after whatever else it queues (`flat` lives
    // until then)
    int alloc_state(UploadScope& q, const std::vector<float>& flat) {
        n_params = (int64_t)flat.size();
        const size_t pb = flat.size() * sizeof(float);
        SSP_TRY(upload(q, P, flat.data(), flat.size()));
        SSP_TRY(G.alloc(pb));
        SSP_TRY(Mo.alloc(pb));
        SSP_TRY(Vo.alloc(pb));
        SSP_TRY(rowloss.alloc((size_t)max_batch * sizeof(float)));
        SSP_TRY(rowcorr.alloc((size_t)max_batch * sizeof(int32_t)));
        SSP_TRY(ticket.alloc(sizeof(uint32_t)));
        SSP_TRY(slots(4096));
        hipError_t e = hipMemsetAsync(ticket.p, 0, sizeof(uint32_t), ctx->stream);
        for (const DevBuf* z : {&G, &Mo, &Vo})
            if (e == hipSuccess) e = hipMemsetAsync(z->p, 0, pb, ctx->stream);
        if (e != hipSuccess) SSP_FAIL(SSP_ERR_HIP, "%s: upload failed: %s", q.who, hipGetErrorString(e));
        return SSP_OK;
    }

    // the per-step sums back to the host, once, and added in float64 in step order
    int collect(int64_t n, double* loss_sum, int64_t* n_correct, hipStream_t s) {
        std::vector<float> hl((size_t)n);
        std::vector<int32_t> hc((size_t)n);
        SSP_HIP(hipMemcpyAsync(hl.data(), slot_loss.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
        SSP_HIP(hipMemcpyAsync(hc.data(), slot_corr.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        SSP_HIP(hipStreamSynchronize(s));
        double ls = 0.0;
        int64_t nc = 0;
        for (int64_t i = 0; i < n; ++i) ls += (double)hl[(size_t)i], nc += hc[(size_t)i];
        if (loss_sum) *loss_sum = ls;
        if (n_correct) *n_correct = nc;
        return SSP_OK;
    }

    int check_data(const char* who, const float* X, const int32_t* labels, int64_t N, int where) const {
        SSP_TRY(check_where(where, who));
        if (N < 0) SSP_FAIL(SSP_ERR_INVALID, "%s: N < 0", who);
        if (N > 0 && (!X || !labels)) SSP_FAIL(SSP_ERR_INVALID, "%s: null array", who);
        if (where == SSP_HOST)
            for (int64_t r = 0; r < N; ++r)
                if (labels[r] < 0 || labels[r] >= n_class)
                    SSP_FAIL(SSP_ERR_INVALID, "%s: label %d of row %lld lies outside [0, %d)", who, labels[r], (long long)r, n_class);
        return SSP_OK;
    }

    int check_step(const char* who, int32_t batch_size, float lr) const {
        if (batch_size < 1 || batch_size > max_batch) SSP_FAIL(SSP_ERR_INVALID, "%s: batch_size %d outside [1, %d]", who, batch_size, max_batch);
        if (!(lr >= 0.f)) SSP_FAIL(SSP_ERR_INVALID, "%s: lr", who);
        return SSP_OK;
    }

    // softmax cross-entropy of the logits Z [Bn x n_class] of rows [row0, row0 + Bn) (of idx when given) into `slot`; grad: the gradient
    // at the logits in place
    int loss(const int32_t* labels, const int64_t* idx, int64_t row0, int Bn, bool grad, int64_t slot, float* Z, hipStream_t s) {
        return dt_launch_loss(Z, idx ? labels : labels + row0, idx ? idx + row0 : nullptr, Bn, n_class, grad ? 1 : 0, rowloss.as<float>(),
                              rowcorr.as<int32_t>(), ticket.as<uint32_t>(), slot_loss.as<float>() + slot, slot_corr.as<int32_t>() + slot, s);
    }

    // Adam over the flat buffers; t counts per queued step: a call that fails half way leaves t in step with the weights it has already moved
    int adam(float lr, hipStream_t s) {
        SSP_TRY(dt_launch_adam(P.as<float>(), G.as<float>(), Mo.as<float>(), Vo.as<float>(), n_params, lr, t + 1, s));
        ++t;
        return SSP_OK;
    }

    // len floats at off of the parameters (what 0), gradients (1) or Adam's moments (2, 3) to the host, waited for
    int read_flat(const char* who, int what, int64_t off, int64_t len, float* out) {
        if (what < 0 || what > 3 || off < 0 || len < 0 || off + len > n_params) SSP_FAIL(SSP_ERR_INVALID, "%s: outside the flat buffers", who);
        const DevBuf& buf = what == 0 ? P : what == 1 ? G : what == 2 ? Mo : Vo;
        SSP_TRY(use_ctx(ctx));
        SSP_HIP(hipMemcpyAsync(out, buf.as<float>() + off, (size_t)len * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        SSP_HIP(hipStreamSynchronize(ctx->stream));
        return SSP_OK;
    }
};

inline int trainer_steps(const char* who, const TrainerCore* c, int64_t* t) {
    if (!c || !t) SSP_FAIL(SSP_ERR_INVALID, "%s: null argument", who);
    *t = c->t;
    return SSP_OK;
}

// The body of ssp_*_trainer_epoch and ssp_*_trainer_evaluate: zero the outputs, validate (all of it before the context is touched), stage
// X (row_floats per row) and the labels, upload the order, then queue `run(dX, dL, dO, row0, Bn, slot, s)` per batch and collect the slots.
// train: batch_size, lr and order are the caller's and are checked (an evaluation has none of them)
template <class Run>
int trainer_run(const char* who, TrainerCore* c, const float* X, int64_t row_floats, const int32_t* labels, int64_t N, const int64_t* order,
                int32_t batch_size, float lr, bool train, double* loss_sum, int64_t* n_correct, int where, float* kernel_ms, Run&& run) {
    TraceRange trace_(who);
    if (kernel_ms) *kernel_ms = 0.f;
    if (loss_sum) *loss_sum = 0.0;
    if (n_correct) *n_correct = 0;
    if (!c) SSP_FAIL(SSP_ERR_INVALID, "%s: null handle", who);
    SSP_TRY(c->check_data(who, X, labels, N, where));
    if (train) {
        SSP_TRY(c->check_step(who, batch_size, lr));
        if (order)
            for (int64_t r = 0; r < N; ++r)
                if (order[r] < 0 || order[r] >= N) SSP_FAIL(SSP_ERR_INVALID, "%s: order[%lld] lies outside [0, N)", who, (long long)r);
    }
    if (N == 0) return SSP_OK;
    ssp_ctx* ctx = c->ctx;
    SSP_TRY(use_ctx(ctx));
    hipStream_t s = ctx->stream;
    const int64_t steps = (N + batch_size - 1) / batch_size;
    SSP_TRY(c->slots(steps));
    StageScope st(ctx, where);
    const float* dX = st.in(X, (size_t)N * row_floats * sizeof(float));
    const int32_t* dL = st.in(labels, (size_t)N * sizeof(int32_t));
    SSP_TRY(st.status());
    const int64_t* dO = nullptr;
    if (order) {
        SSP_TRY(c->order.reserve((size_t)N * sizeof(int64_t)));
        SSP_HIP(hipMemcpyAsync(c->order.p, order, (size_t)N * sizeof(int64_t), hipMemcpyHostToDevice, s));
        dO = c->order.as<int64_t>();
    }
    Timer tm;
    SSP_TRY(tm.start(kernel_ms != nullptr, s));
    for (int64_t st = 0; st < steps; ++st) {
        const int64_t row0 = st * batch_size;
        const int Bn = (int)(N - row0 < batch_size ? N - row0 : batch_size);
        SSP_TRY(run(dX, dL, dO, row0, Bn, st, s));
    }
    SSP_TRY(tm.stop(s, kernel_ms));
    return c->collect(steps, loss_sum, n_correct, s);
}

// step(dX, dL, dO, row0, Bn, slot, s) queues one training step (it ends in c->adam)
template <class Step>
int trainer_epoch(const char* who, TrainerCore* c, const float* X, int64_t row_floats, const int32_t* labels, int64_t N, const int64_t* order,
                  int32_t batch_size, float lr, double* loss_sum, int64_t* n_correct, int where, float* kernel_ms, Step&& step) {
    return trainer_run(who, c, X, row_floats, labels, N, order, batch_size, lr, true, loss_sum, n_correct, where, kernel_ms, step);
}

// eval(dX, dL, row0, Bn, slot, s) queues the forward pass and the loss of one batch; nothing is updated
template <class Eval>
int trainer_evaluate(const char* who, TrainerCore* c, const float* X, int64_t row_floats, const int32_t* labels, int64_t N, double* loss_sum,
                     int64_t* n_correct, int where, float* kernel_ms, Eval&& eval) {
    return trainer_run(who, c, X, row_floats, labels, N, nullptr, c ? c->max_batch : 1, 0.f, false, loss_sum, n_correct, where, kernel_ms,
                       [&](const float* dX, const int32_t* dL, const int64_t*, int64_t row0, int Bn, int64_t slot, hipStream_t s) {
                           return eval(dX, dL, row0, Bn, slot, s);
                       });
}

// hipEvents between the launches of one step (ssp_*_trainer_step_times): the time since the mark before goes to `slot` (-1: nowhere)
struct StepMarks {
    EventSet ev;
    std::vector<int> slot;
    int mark(hipStream_t s, int to) {
        hipEvent_t e = nullptr;
        SSP_HIP(hipEventCreate(&e));
        ev.ev.push_back(e);
        slot.push_back(to);
        SSP_HIP(hipEventRecord(e, s));
        return SSP_OK;
    }
    // ms_out[0 .. n) = the milliseconds of each slot, after the stream has been waited for
    int times(float* ms_out, int n) const {
        for (int i = 0; i < n; ++i) ms_out[i] = 0.f;
        for (size_t i = 1; i < ev.ev.size(); ++i) {
            float ms = 0.f;
            SSP_HIP(hipEventElapsedTime(&ms, ev[i - 1], ev[i]));
            if (slot[i] >= 0 && slot[i] < n) ms_out[slot[i]] += ms;
        }
        return SSP_OK;
    }
};
// a null pointer marks nothing (the steps of an epoch)
inline int mark(StepMarks* m, hipStream_t s, int to) { return m ? m->mark(s, to) : SSP_OK; }

// The front of ssp_*_trainer_step_times: ONE step on the first batch_size rows of device arrays, queued by step(s, &mk), and waited for
template <class Step>
int trainer_timed_step(const char* who, TrainerCore* c, const float* X, const int32_t* labels, int32_t batch_size, float lr, const float* ms_out,
                       StepMarks& mk, Step&& step) {
    if (!ms_out) SSP_FAIL(SSP_ERR_INVALID, "%s: null output", who);
    if (!c) SSP_FAIL(SSP_ERR_INVALID, "%s: null handle", who);
    SSP_TRY(c->check_data(who, X, labels, batch_size, SSP_DEVICE));
    SSP_TRY(c->check_step(who, batch_size, lr));
    SSP_TRY(use_ctx(c->ctx));
    hipStream_t s = c->ctx->stream;
    SSP_TRY(step(s, &mk));
    SSP_HIP(hipStreamSynchronize(s));
    return SSP_OK;
}

}  // namespace ssp
