"""Full-covariance GMM statistics and scoring beside the diagonal entry points and beside torch, in one process on one GPU
(profiles/gmm_full.md).

    python tools/bench_gmm_full.py [--frames 3000000] [--mixtures 64] [--dim 39] [--models 51] [--score-frames 300000] [--reps 3]

Shapes: ssp_gmm_full_em_stats at --frames x --mixtures x --dim (the README's training shape), the scorer at --models x --mixtures x --dim
on --score-frames frames in utterances of 300 — a batch whose [models x frames] block fits the scratch budget.  Each beside
  diag    the diagonal entry point (api.gmm_em_stats / api.GmmScorer precision 0) on the same frames, and
  torch   the same computation composed from torch.matmul / einsum in float32 with TF32 off, frames in chunks: y = (x - mu_k) U_k for all k
          as one matmul against [U_1 | ... | U_K], lp, logsumexp, and for the statistics resp^T [1, x'] and einsum('tk,ti,tj->kij').
Kernel ms from hipEvents (best of --reps after one untimed call); torch timed with events the same way.  The fraction of the 157.3 TFLOP/s
fp32 MFMA peak is taken on the DENSE count 2 N K D^2 per pass (statistics: two passes; scorer: one pass per model).  One JSON line per
measurement; nothing is asserted."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_TFLOPS = 157.3


def ev_ms(fn, reps):
    import torch
    fn()
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3000000)
    ap.add_argument("--mixtures", type=int, default=64)
    ap.add_argument("--dim", type=int, default=39)
    ap.add_argument("--models", type=int, default=51)
    ap.add_argument("--score-frames", type=int, default=300000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=65536)
    a = ap.parse_args()
    import torch
    import gmm_full_cases as FC
    from speech_signal_processing_amd import api
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    ctx = api.default_context()
    N, K, D, M = a.frames, a.mixtures, a.dim, a.models
    rng = np.random.default_rng(0)
    w, mu, cov, U = FC.draw_model(rng, K, D)
    dcov = np.diagonal(cov, axis1=1, axis2=2).copy()
    X = torch.randn((N, D), device="cuda", dtype=torch.float32) * 1.3
    shift = X.mean(dim=0, dtype=torch.float64).cpu().numpy()

    def frac(flops, ms):
        return round(flops / (ms * 1e-3) / (PEAK_TFLOPS * 1e12), 4)

    # ---- statistics
    ms_full = min(api.gmm_full_em_stats(ctx, w, mu, U, X, shift=shift, timing=True)["kernel_ms"] for _ in range(a.reps + 1))
    ms_diag = min(api.gmm_em_stats(ctx, w, mu, dcov, X, timing=True)["kernel_ms"] for _ in range(a.reps + 1))
    Ucat = torch.from_numpy(np.concatenate(list(np.triu(U)), axis=1).astype(np.float32)).cuda()            # (D, K D)
    bias = torch.from_numpy(-np.einsum("kd,kdj->kj", mu - shift[None], np.triu(U)).reshape(-1).astype(np.float32)).cuda()
    cst = torch.from_numpy((np.log(w) - 0.5 * D * np.log(2 * np.pi) + np.log(np.diagonal(U, axis1=1, axis2=2)).sum(1)).astype(np.float32)).cuda()
    sh32 = torch.from_numpy(shift.astype(np.float32)).cuda()

    def torch_stats():
        nk = torch.zeros(K, device="cuda", dtype=torch.float64)
        sx = torch.zeros((K, D), device="cuda", dtype=torch.float64)
        sxx = torch.zeros((K, D, D), device="cuda", dtype=torch.float64)
        ll = torch.zeros((), device="cuda", dtype=torch.float64)
        for o in range(0, N, a.chunk):
            xc = X[o:o + a.chunk] - sh32
            y = torch.addmm(bias, xc, Ucat).view(-1, K, D)
            lp = cst - 0.5 * (y * y).sum(dim=2)
            lse = torch.logsumexp(lp, dim=1)
            r = torch.exp(lp - lse[:, None])
            nk += r.sum(dim=0)
            sx += r.t() @ xc
            sxx += torch.einsum("tk,ti,tj->kij", r, xc, xc)
            ll += lse.sum()
        return nk, sx, sxx, ll
    ms_torch = ev_ms(torch_stats, a.reps)
    flops = 2.0 * 2.0 * N * K * D * D
    print(json.dumps({"what": "full_em_stats", "frames": N, "K": K, "D": D, "kernel_ms": round(ms_full, 3), "diag_kernel_ms": round(ms_diag, 3),
                      "torch_ms": round(ms_torch, 3), "dense_tflop": round(flops / 1e12, 3), "fraction_of_fp32_mfma_peak": frac(flops, ms_full),
                      "torch_fraction_of_peak": frac(flops, ms_torch)}), flush=True)
    del X
    # ---- scorer
    F = a.score_frames // 300 * 300
    models = [FC.draw_model(rng, K, D) for _ in range(M)]
    ws, mus, Us = (np.stack([m[i] for m in models]) for i in (0, 1, 3))
    dcv = np.stack([np.diagonal(m[2], axis1=1, axis2=2) for m in models])
    Y = torch.randn((F, D), device="cuda", dtype=torch.float32) * 1.3
    seg = api.Segments.from_lengths(ctx, [300] * (F // 300))
    full = api.GmmFullScorer(ctx, ws, mus, Us, has_ubm=True)
    diag = api.GmmScorer(ctx, ws, mus, dcv, has_ubm=True)
    ms_full = min(full.score(Y, seg, timing=True)["kernel_ms"] for _ in range(a.reps + 1))
    ms_diag = min(diag.score(Y, seg, precision=0, timing=True)["kernel_ms"] for _ in range(a.reps + 1))
    Uc = [torch.from_numpy(np.concatenate(list(np.triu(Us[m])), axis=1).astype(np.float32)).cuda() for m in range(M)]
    bs = [torch.from_numpy(-np.einsum("kd,kdj->kj", mus[m], np.triu(Us[m])).reshape(-1).astype(np.float32)).cuda() for m in range(M)]
    cs = [torch.from_numpy((np.log(ws[m]) - 0.5 * D * np.log(2 * np.pi) + np.log(np.diagonal(Us[m], axis1=1, axis2=2)).sum(1)).astype(np.float32)).cuda()
          for m in range(M)]

    def torch_score():
        out = torch.empty((F // 300, M), device="cuda", dtype=torch.float32)
        for m in range(M):
            for o in range(0, F, a.chunk // 300 * 300):
                yc = Y[o:o + a.chunk // 300 * 300]
                y = torch.addmm(bs[m], yc, Uc[m]).view(-1, K, D)
                lse = torch.logsumexp(cs[m] - 0.5 * (y * y).sum(dim=2), dim=1)
                out[o // 300:o // 300 + len(yc) // 300, m] = lse.view(-1, 300).mean(dim=1)
        return out
    ms_torch = ev_ms(torch_score, a.reps)
    flops = 2.0 * F * M * K * D * D
    print(json.dumps({"what": "full_score", "frames": F, "models": M, "K": K, "D": D, "kernel_ms": round(ms_full, 3),
                      "diag_kernel_ms": round(ms_diag, 3), "torch_ms": round(ms_torch, 3), "dense_tflop": round(flops / 1e12, 3),
                      "fraction_of_fp32_mfma_peak": frac(flops, ms_full), "torch_fraction_of_peak": frac(flops, ms_torch)}), flush=True)


if __name__ == "__main__":
    main()
