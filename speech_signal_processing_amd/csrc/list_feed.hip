// List-fed GMM scoring (ssp_gmm_score_list): the reference's scoring loops (GMM_UBM.py:181-197) hold one feature matrix per utterance.
// The rows are gathered and narrowed to float32 into a pinned buffer kept on the ctx by the pipe's copying threads, then the public
// ssp_gmm_score(SSP_HOST) scores that buffer: its own paths (one piece, the feed_rows ring, re-scoring, auto) run unchanged at the pinned
// rate, so scores and arg-max are its bits by construction.  No device code here.
#include <chrono>

#include "common.hpp"

using namespace ssp;

extern "C" {

int ssp_gmm_score_list(ssp_gmm* gmm, const void* const* rows, int row_type, int32_t dim, const ssp_segments* frame_seg,
                       float* scores_out, int32_t* argmax_out, int precision, float* kernel_ms) {
    ssp::TraceRange trace_("ssp_gmm_score_list");
    // (every argument is checked before the ctx is touched)
    if (!gmm || !frame_seg) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_score_list: null handle");
    if (row_type != 0 && row_type != 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_score_list: row_type must be 0 (float32) or 1 (float64)");
    if (dim < 1) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_score_list: dim < 1");
    if (precision < 0 || precision > 4) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_score_list: precision must be in [0, 4] (ssp_gmm_score)");
    const std::vector<int64_t>& fo = frame_seg->host;
    if (fo.front() != 0) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_score_list: frame segments must start at frame 0");
    const int64_t n = frame_seg->n, F = fo.back();
    if (n > 0 && !rows) SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_score_list: null row table");
    for (int64_t u = 0; u < n; ++u)
        if (!rows[u] && fo[(size_t)u + 1] > fo[(size_t)u])
            SSP_FAIL(SSP_ERR_INVALID, "ssp_gmm_score_list: null pointer for utterance %lld of %lld rows", (long long)u,
                     (long long)(fo[(size_t)u + 1] - fo[(size_t)u]));
    ssp_ctx* ctx = frame_seg->ctx;
    SSP_TRY(use_ctx(ctx));
    if (kernel_ms) *kernel_ms = 0.f;
    if (n == 0 || F == 0)   // (nothing to gather: ssp_gmm_score answers as it does for an empty batch)
        return ssp_gmm_score(gmm, nullptr, frame_seg, nullptr, scores_out, argmax_out, SSP_HOST, precision, kernel_ms);
    const size_t row_elems = (size_t)dim;
    SSP_TRY(pipe_bounce(ctx, (size_t)F * row_elems * sizeof(float) + 16, 0));
    float* bounce = ctx->pipe->bounce_in.as<float>();
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<CopyPiece> pieces;
    for (int64_t u = 0; u < n; ++u) {
        const size_t T = (size_t)(fo[(size_t)u + 1] - fo[(size_t)u]);
        if (!T) continue;
        float* dst = bounce + (size_t)fo[(size_t)u] * row_elems;
        if (row_type == 1)
            add_pieces(pieces, rows[u], dst, T * row_elems, COPY_F64_TO_F32);
        else
            add_pieces(pieces, rows[u], dst, T * row_elems * sizeof(float), COPY_BYTES);
    }
    run_pieces(pipe_pool(ctx), pieces);
    if (getenv("SSP_HOST_TRACE"))
        fprintf(stderr, "[ssp host pipeline] gmm list: %d copying threads; host ms: gather %.3f\n", ctx->pipe->pool.threads(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return ssp_gmm_score(gmm, bounce, frame_seg, nullptr, scores_out, argmax_out, SSP_HOST, precision, kernel_ms);
}

}  // extern "C"
