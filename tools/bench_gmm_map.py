"""MAP-adapted speaker models and top-C fast scoring against the dense scorer, in one process on one GPU (profiles/gmm_map.md).

    python tools/bench_gmm_map.py [--speakers 1251] [--utts 12000] [--frames 298] [--train-frames 2000] [--reps 3] [--no-dense]

Model shape of bench.py's configs[3]: K = 512, D = 39, S mean-adapted speakers + the UBM.  The UBM has means N(0, 1), variances in
[0.5, 1.5] and Dirichlet(5) weights; speaker s truly speaks from the UBM with its means moved by 0.3 N(0, 1); its model is what
gmm_train.map_adapt makes of --train-frames frames of it; utterance u is spoken by speaker u mod S.  The utterances sit in HBM.
Timed: map_adapt for all speakers (wall, and the statistics call's kernel ms); api.MapScorer at C = 5 and 8 (wall of a device-pointer
call ended by a device sync, best of --reps after one untimed call; kernel ms from hipEvents; per kernel by asking for less: idx alone
runs the selection kernel, ubm adds the reduce kernel, diff + argmax the scoring kernel); the dense api.GmmScorer at precision 0 and 1
on the same models (one untimed call on 64 utterances, then one timed call).  Reported, not asserted: the share of utterances whose
top-C arg-max is the dense fp32 arg-max, and the largest |diff_topC - diff_dense| — the approximation's price.  One JSON line per
measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


class _Model:
    covariance_type = "diag"
    reg_covar = 1e-6

    def __init__(self, w, mu, cv):
        self.weights_, self.means_, self.covariances_ = w, mu, cv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speakers", type=int, default=1251)
    ap.add_argument("--utts", type=int, default=12000)
    ap.add_argument("--frames", type=int, default=298)
    ap.add_argument("--train-frames", type=int, default=2000)
    ap.add_argument("--mixtures", type=int, default=512)
    ap.add_argument("--dim", type=int, default=39)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-dense", action="store_true")
    a = ap.parse_args()
    import torch
    from speech_signal_processing_amd import api
    from speech_signal_processing_amd.gmm_train import map_adapt
    S, K, D, U, T = a.speakers, a.mixtures, a.dim, a.utts, a.frames
    ctx = api.default_context()
    rng = np.random.default_rng(0)
    w = rng.dirichlet(5 * np.ones(K))
    mu = rng.standard_normal((K, D))
    cv = rng.uniform(0.5, 1.5, (K, D))
    true = (mu[None] + 0.3 * rng.standard_normal((S, K, D))).astype(np.float32)
    sd = np.sqrt(cv).astype(np.float32)

    def speak(s, n):
        k = rng.choice(K, size=n, p=w)
        return true[s, k] + sd[k] * rng.standard_normal((n, D), dtype=np.float32)

    shape = {"K": K, "D": D, "S": S, "utts": U, "frames": T}
    # ---- adaptation
    Xs = [speak(s, a.train_frames) for s in range(S)]
    ubm = _Model(w, mu, cv)
    map_adapt(ubm, Xs[:2])   # (untimed first call)
    dt, gms = timed(lambda: map_adapt(ubm, Xs))
    feats = torch.from_numpy(np.concatenate(Xs)).cuda()
    ns = np.full(S, a.train_frames, np.int64)
    st = api.gmm_em_stats_shared(ctx, w, mu, cv, feats, np.arange(S) * a.train_frames, ns, timing=True)
    print(json.dumps({"what": "map_adapt", **shape, "train_frames": a.train_frames, "wall_s": round(dt, 4),
                      "stats_kernel_ms": round(st["kernel_ms"], 3)}), flush=True)
    del feats, Xs, st
    sm = np.stack([g.means_ for g in gms])
    del gms
    # ---- utterances, resident
    X = torch.empty((U * T, D), dtype=torch.float32, device="cuda")
    step = 500
    for u0 in range(0, U, step):
        blk = np.concatenate([speak(u % S, T) for u in range(u0, min(U, u0 + step))])
        X[u0 * T:u0 * T + len(blk)] = torch.from_numpy(blk).cuda()
    seg = api.Segments.from_lengths(ctx, [T] * U)
    spoke = np.arange(U) % S
    # ---- top-C
    sc = api.MapScorer(ctx, w, mu, cv, sm)
    res = {}
    for Ck in (5, 8):
        sc.score(X, seg, top_c=Ck)
        wall = min(timed(lambda: sc.score(X, seg, top_c=Ck))[0] for _ in range(a.reps))
        full = sc.score(X, seg, top_c=Ck, ubm=True, timing=True)
        sel = sc.score(X, seg, top_c=Ck, diff=False, argmax=False, idx=True, timing=True)["kernel_ms"]
        selred = sc.score(X, seg, top_c=Ck, diff=False, argmax=False, ubm=True, timing=True)["kernel_ms"]
        res[Ck] = {"diff": full["diff"].cpu().numpy(), "argmax": full["argmax"].cpu().numpy()}
        print(json.dumps({"what": "map_score", **shape, "C": Ck, "wall_s": round(wall, 4), "kernel_ms": round(full["kernel_ms"], 3),
                          "select_kernel_ms": round(sel, 3), "reduce_kernel_ms": round(max(selred - sel, 0.0), 3),
                          "score_kernel_ms": round(full["kernel_ms"] - selred, 3),
                          "speaker_identified": round(float((res[Ck]["argmax"] == spoke).mean()), 5)}), flush=True)
        del full
    sc.close()
    if a.no_dense:
        return
    # ---- dense, same models
    dense = api.GmmScorer(ctx, np.stack([w] * (S + 1)), np.concatenate([mu[None], sm]), np.stack([cv] * (S + 1)))
    small = api.Segments.from_lengths(ctx, [T] * 64)
    ref = None
    for prec in (1, 0):
        dense.score(X[:64 * T], small, precision=prec)
        dt, r = timed(lambda: dense.score(X, seg, precision=prec, timing=True))
        scm = r["scores"].cpu().numpy().astype(np.float64)
        out = {"what": "dense_score", **shape, "precision": prec, "wall_s": round(dt, 4), "kernel_ms": round(r["kernel_ms"], 3),
               "speaker_identified": round(float((r["argmax"].cpu().numpy() == spoke).mean()), 5)}
        if prec == 1:
            out["rescored"] = dense.last_rescored
        print(json.dumps(out), flush=True)
        if prec == 0:
            ref = {"diff": scm[:, 1:] - scm[:, :1], "argmax": r["argmax"].cpu().numpy()}
        del r, scm
    for Ck in (5, 8):
        print(json.dumps({"what": "topc_against_dense_fp32", **shape, "C": Ck,
                          "argmax_equal": round(float((res[Ck]["argmax"] == ref["argmax"]).mean()), 5),
                          "max_abs_diff_minus_dense": float(np.abs(res[Ck]["diff"] - ref["diff"]).max()),
                          "mean_abs_diff_minus_dense": float(np.abs(res[Ck]["diff"] - ref["diff"]).mean())}), flush=True)


if __name__ == "__main__":
    main()
