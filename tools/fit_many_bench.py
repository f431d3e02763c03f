"""Wall time of training many speaker GMMs: a loop of gmm_train.GaussianMixture.fit (one EM launch + host sync per model and
iteration) against gmm_train.fit_many (one ssp_gmm_em_stats_batch launch per iteration for all models).  Every timed region ends in a
device sync; every shape is run once untimed first.  Prints one JSON line per case.

    python tools/fit_many_bench.py [--cases 1,2,3]

case 1: 50 speakers x 9000 frames, K = 64, D = 39, from given inits, max_iter = 20, tol = 0 (+ the per-iteration split of fit_many:
        kernel time from hipEvents, host M step, the rest)
case 2: the same from the default k-means start (random_state = 0); k-means++ host time on its own
case 3: 200 speakers x 9000 frames, K = 512, D = 39, max_iter = 5, from given inits
case 4: case 2 with seeding='host' and seeding='device' (k-means++ through ssp_kmeanspp_seed: one launch for all 50 seedings) in the same
        process: fit_many wall time of both, the seeding's share of each, the seeding kernel's time, and whether the models agree
case 5: the UBM-shaped single fit, 450000 frames x 39, K = 64, max_iter = 5: GaussianMixture.fit with both seedings, and the seeding alone
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def data(S, n, K, D, seed=0):
    rng = np.random.default_rng(seed)
    Xs, inits = [], []
    for _ in range(S):
        centres = 2.0 * rng.standard_normal((K, D))
        X = (centres[rng.integers(0, K, n)] + rng.standard_normal((n, D))).astype(np.float32)
        Xs.append(X)
        inits.append((rng.dirichlet(5 * np.ones(K)), centres + 0.5 * rng.standard_normal((K, D)), rng.uniform(0.8, 2.0, (K, D))))
    return Xs, inits


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def run(case, S, n, K, D, max_iter, given, reps=1):
    from speech_signal_processing_amd.gmm_train import GaussianMixture, fit_many
    Xs, inits = data(S, n, K, D)
    kw = dict(n_components=K, max_iter=max_iter, tol=0.0)
    if given:
        per = dict(weights_init=[i[0] for i in inits], means_init=[i[1] for i in inits], precisions_init=[1.0 / i[2] for i in inits])
        loop_fn = lambda: [GaussianMixture(weights_init=i[0], means_init=i[1], precisions_init=1.0 / i[2], **kw).fit(X)  # noqa: E731
                           for X, i in zip(Xs, inits)]
    else:
        kw["random_state"] = 0
        per = {}
        loop_fn = lambda: [GaussianMixture(**kw).fit(X) for X in Xs]  # noqa: E731
    many_fn = lambda: fit_many(Xs, **kw, **per)  # noqa: E731
    # warm-up of every shape at full size (the ctx's device scratch grows to the batch on the first call)
    wk = dict(kw, max_iter=2)
    fit_many(Xs, **wk, **per)
    GaussianMixture(**wk, **({k: v[0] for k, v in per.items()})).fit(Xs[0])
    t_loop = min(timed(loop_fn)[0] for _ in range(reps))
    t_many, gms = min((timed(many_fn) for _ in range(reps)), key=lambda r: r[0])
    prof = {}
    t_prof, _ = timed(lambda: fit_many(Xs, profile=prof, **kw, **per))
    iters = max(1, int(prof["em_iters"]))
    res = {"case": case, "speakers": S, "frames": n, "K": K, "D": D, "max_iter": max_iter, "start": "given" if given else "kmeans",
           "loop_s": round(t_loop, 4), "fit_many_s": round(t_many, 4), "reps": reps, "speedup": round(t_loop / t_many, 2),
           "batched_calls": int(prof["calls"]), "em_iters": iters,
           "profiled_run_s": round(t_prof, 4), "kernel_ms_total": round(prof["kernel_ms"], 3), "mstep_ms_total": round(1e3 * prof["mstep_s"], 3),
           "kernel_ms_per_call": round(prof["kernel_ms"] / max(1, prof["calls"]), 4),
           "mstep_ms_per_iter": round(1e3 * prof["mstep_s"] / iters, 4)}
    if not given:
        res["kmeanspp_host_s"] = round(prof["kmeanspp_s"], 4)
    res["rest_ms_total"] = round(1e3 * t_prof - prof["kernel_ms"] - 1e3 * prof["mstep_s"] - 1e3 * prof["kmeanspp_s"], 3)
    print(json.dumps(res), flush=True)


def _same(a, b):
    return bool(all(np.array_equal(getattr(x, k), getattr(y, k)) for x, y in zip(a, b) for k in ("weights_", "means_", "covariances_")))


def run_seeding_many(case, S, n, K, D, max_iter, reps=1):
    """case 2's fit_many with the k-means++ seeds from the host and from the device, side by side"""
    from speech_signal_processing_amd.gmm_train import fit_many
    Xs, _ = data(S, n, K, D)
    kw = dict(n_components=K, max_iter=max_iter, tol=0.0, random_state=0)
    res = {"case": case, "speakers": S, "frames": n, "K": K, "D": D, "max_iter": max_iter, "start": "kmeans", "reps": reps}
    models = {}
    for side in ("host", "device"):
        fit_many(Xs, seeding=side, **dict(kw, max_iter=2))
        t, models[side] = min((timed(lambda: fit_many(Xs, seeding=side, **kw)) for _ in range(reps)), key=lambda r: r[0])
        prof = {}
        timed(lambda: fit_many(Xs, seeding=side, profile=prof, **kw))
        res["fit_many_%s_s" % side] = round(t, 4)
        res["kmeanspp_%s_s" % side] = round(prof["kmeanspp_s"], 4)
        if side == "device":
            res["kmeanspp_kernel_ms"] = round(prof["kmeanspp_kernel_ms"], 3)
    res["kmeanspp_ratio"] = round(res["kmeanspp_host_s"] / max(res["kmeanspp_device_s"], 1e-9), 2)
    res["fit_many_ratio"] = round(res["fit_many_host_s"] / res["fit_many_device_s"], 2)
    res["same_models"] = _same(models["host"], models["device"])
    print(json.dumps(res), flush=True)


def run_seeding_one(case, n, K, D, max_iter, reps=1):
    """the UBM-shaped fit: one model on every frame, seeded on a 20000-row subsample"""
    import torch
    from speech_signal_processing_amd import api
    from speech_signal_processing_amd.gmm_train import GaussianMixture
    X = data(1, n, K, D)[0][0]
    ctx = api.default_context()
    Xd = torch.from_numpy(X).to("cuda:%d" % ctx.device)
    kw = dict(n_components=K, max_iter=max_iter, tol=0.0)
    res = {"case": case, "speakers": 1, "frames": n, "K": K, "D": D, "max_iter": max_iter, "start": "kmeans", "reps": reps}
    models = {}
    for side in ("host", "device"):
        GaussianMixture(seeding=side, random_state=0, **dict(kw, max_iter=2)).fit(Xd)
        t, models[side] = min((timed(lambda: GaussianMixture(seeding=side, random_state=0, **kw).fit(Xd)) for _ in range(reps)), key=lambda r: r[0])
        gm = GaussianMixture(seeding=side, **kw)
        ts = min(timed(lambda: gm._seeds(ctx, Xd, n, D, np.random.RandomState(0)))[0] for _ in range(reps))
        res["fit_%s_s" % side] = round(t, 4)
        res["kmeanspp_%s_s" % side] = round(ts, 4)
    from speech_signal_processing_amd.gmm_train import _kmeanspp_draws
    idx, first, u = _kmeanspp_draws(np.random.RandomState(0), n, K)
    res["kmeanspp_kernel_ms"] = round(api.kmeanspp_seeds(ctx, Xd, K, [first], u[None], sel=idx, timing=True)["kernel_ms"], 3)
    res["kmeanspp_ratio"] = round(res["kmeanspp_host_s"] / max(res["kmeanspp_device_s"], 1e-9), 2)
    res["fit_ratio"] = round(res["fit_host_s"] / res["fit_device_s"], 2)
    res["same_models"] = _same([models["host"]], [models["device"]])
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,2,3")
    ap.add_argument("--reps", type=int, default=3, help="timed runs of each side (the minimum is reported)")
    a = ap.parse_args()
    cases = {1: (50, 9000, 64, 39, 20, True), 2: (50, 9000, 64, 39, 20, False), 3: (200, 9000, 512, 39, 5, True)}
    for c in [int(x) for x in a.cases.split(",")]:
        if c == 4:
            run_seeding_many(4, 50, 9000, 64, 39, 20, reps=a.reps)
        elif c == 5:
            run_seeding_one(5, 450000, 64, 39, 5, reps=a.reps)
        else:
            run(c, *cases[c], reps=a.reps)


if __name__ == "__main__":
    main()
