"""i-vector extraction and one E-step of total-variability training against the same computation composed from torch, in one process on
one GPU, on the same statistics (profiles/ivector.md).

    python tools/bench_ivector.py [--utts 12000] [--frames 298] [--mixtures 512] [--dim 39] [--rank 256] [--reps 20] [--out profiles/ivector.md]

Model shape of bench.py's configs[3]: K = 512, D = 39, with a rank-256 T.  Synthetic: a UBM with means N(0, 1), variances in [0.5, 2],
Dirichlet(5) weights; T = 0.9 * 0.85^r * N(0, 1) per column r (the tests' recipe); utterance u is drawn from the mixture with means
mu + T w_u, w_u ~ N(0, I).  Its statistics come from ONE ssp_gmm_em_stats_shared call per block of utterances.
Library: api.IvectorExtractor.extract and .estep on the host statistics; per stage the device time between hipEvents on the ctx stream
(ssp_ivector_last_stages), median of --reps calls after one untimed call; the wall time of a call (host centring pass, copies and
kernels) beside it.  torch: the same stages on resident fp32 tensors, TF32 off — matmul for L and b, torch.linalg.cholesky,
cholesky_solve, cholesky_inverse, matmul for the accumulators — each between torch events, median of --reps after one untimed pass.
FLOP counts are the algorithm's: 2 U K R(R+1)/2 for L from packed triangles (torch multiplies the full R^2), 2 U K D R for b, U R^3 / 3 for
the factor (+ 2 U R^3 / 3 for the inverse), and the same two GEMM counts for the accumulators.  One JSON line per measurement; the
markdown file holds the table."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=12000)
    ap.add_argument("--frames", type=int, default=298)
    ap.add_argument("--mixtures", type=int, default=512)
    ap.add_argument("--dim", type=int, default=39)
    ap.add_argument("--rank", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivector.md"))
    a = ap.parse_args()
    import torch
    from speech_signal_processing_amd import api
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    U, F, K, D, R = a.utts, a.frames, a.mixtures, a.dim, a.rank
    tri = R * (R + 1) // 2
    ctx = api.default_context()
    rng = np.random.default_rng(0)
    w = rng.dirichlet(5 * np.ones(K))
    mu = rng.standard_normal((K, D))
    cv = rng.uniform(0.5, 2.0, (K, D))
    T = 0.9 * 0.85 ** np.arange(R) * rng.standard_normal((K, D, R))
    shape = {"K": K, "D": D, "R": R, "utts": U, "frames": F}
    # ---- statistics: frames drawn on the device, block by block
    g = torch.Generator(device="cuda").manual_seed(0)
    d_mu = torch.from_numpy(mu).float().cuda()
    d_sd = torch.from_numpy(np.sqrt(cv)).float().cuda()
    d_T = torch.from_numpy(T).float().cuda()
    d_w = torch.from_numpy(w).float().cuda()
    nk = np.empty((U, K))
    sx = np.empty((U, K, D))
    t0 = time.perf_counter()
    step = 1000
    for u0 in range(0, U, step):
        n = min(step, U - u0)
        wu = torch.randn((n, R), generator=g, device="cuda")
        k = torch.multinomial(d_w, n * F, replacement=True, generator=g).view(n, F)
        shift = torch.einsum("kdr,ur->ukd", d_T, wu)                      # (n, K, D)
        means = d_mu[None] + shift
        X = torch.gather(means, 1, k[:, :, None].expand(n, F, D)) + d_sd[k] * torch.randn((n, F, D), generator=g, device="cuda")
        st = api.gmm_em_stats_shared(ctx, w, mu, cv, X.reshape(n * F, D), np.arange(n) * F, np.full(n, F, np.int64))
        nk[u0:u0 + n], sx[u0:u0 + n] = st["nk"], st["sx"]
        del X, means, shift, st
    print(json.dumps({"what": "statistics", **shape, "wall_s": round(time.perf_counter() - t0, 2)}), flush=True)

    def med(xs):
        return float(statistics.median(xs))

    flops = {"gemm_L": 2.0 * U * K * tri, "gemm_b": 2.0 * U * K * D * R, "cholesky": U * R ** 3 / 3.0, "cholesky_estep": U * R ** 3,
             "gemm_A": 2.0 * U * K * tri, "gemm_C": 2.0 * U * K * D * R}
    # ---- the library
    ext = api.IvectorExtractor(ctx, mu, cv, T)
    ext.extract(nk, sx)
    lib = {}
    rows, walls = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = ext.extract(nk, sx, logdet=True, quad=True, timing=True)
        walls.append(time.perf_counter() - t0)
        rows.append(dict(ext.last_stages, kernel_ms=r["kernel_ms"]))
    lib["extract"] = {k: med([x[k] for x in rows]) for k in ("gemm_L", "gemm_b", "cholesky", "kernel_ms")}
    lib["extract"]["wall_ms"] = 1e3 * med(walls)
    lib_w, slab = r["w"], ext.last_slab
    print(json.dumps({"what": "lib_extract", **shape, "slab": slab, **{k: round(v, 3) for k, v in lib["extract"].items()}}), flush=True)
    ext.estep(nk, sx)
    rows, walls = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = ext.estep(nk, sx, timing=True)
        walls.append(time.perf_counter() - t0)
        rows.append(dict(ext.last_stages, kernel_ms=r["kernel_ms"]))
    lib["estep"] = {k: med([x[k] for x in rows]) for k in api.IVECTOR_STAGES + ("kernel_ms",)}
    lib["estep"]["wall_ms"] = 1e3 * med(walls)
    lib_A = r["A"]
    print(json.dumps({"what": "lib_estep", **shape, "slab": slab, **{k: round(v, 3) for k, v in lib["estep"].items()}}), flush=True)
    ext.close()
    # ---- torch, on the same statistics (centred in float64, rounded once, as the library forms them)
    tor, err, note, err_note, tw, ta = {}, {}, None, None, None, None
    try:
        f32 = torch.from_numpy((sx - nk[:, :, None] * mu[None]).astype(np.float32).reshape(U, K * D)).cuda()
        n32 = torch.from_numpy(nk.astype(np.float32)).cuda()
        G64 = torch.from_numpy(T / cv[:, :, None]).cuda()
        P = torch.einsum("kdi,kdj->kij", G64, torch.from_numpy(T).cuda()).float().reshape(K, R * R)
        G = G64.float().reshape(K * D, R)
        eye = torch.eye(R, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]

        def once(estep):
            ev[0].record()
            L = (n32 @ P).view(U, R, R) + eye
            ev[1].record()
            b = f32 @ G
            ev[2].record()
            ch = torch.linalg.cholesky(L)
            wv = torch.cholesky_solve(b[:, :, None], ch)[:, :, 0]
            logdet = 2.0 * torch.log(torch.diagonal(ch, dim1=1, dim2=2)).sum(dim=1)
            quad = (b * wv).sum(dim=1)
            out = {"w": wv, "logdet": logdet, "quad": quad}
            if estep:
                S = torch.cholesky_inverse(ch)
                S += wv[:, :, None] * wv[:, None, :]
            ev[3].record()
            if estep:
                out["A"] = (n32.T @ S.reshape(U, R * R)).view(K, R, R)
                ev[4].record()
                out["C"] = f32.T @ wv
                ev[5].record()
            torch.cuda.synchronize()
            names = api.IVECTOR_STAGES[:5 if estep else 3]
            return {nm: ev[i].elapsed_time(ev[i + 1]) for i, nm in enumerate(names)}, out

        for estep in (False, True):
            once(estep)
            rows = []
            for _ in range(a.reps):
                ms, out = once(estep)
                rows.append(dict(ms, kernel_ms=sum(ms.values())))
            key = "estep" if estep else "extract"
            tor[key] = {k: med([x[k] for x in rows]) for k in rows[0]}
            print(json.dumps({"what": "torch_" + key, **shape, **{k: round(v, 3) for k, v in tor[key].items()}}), flush=True)
            if not estep:
                tw = out["w"].cpu().numpy()
            else:
                ta = out["A"].double().cpu().numpy()
            del out
    except Exception as e:  # the torch side is a comparison, not a dependency: say what was not measured
        note = "%s: %s" % (type(e).__name__, str(e).splitlines()[0] if str(e) else "")
        print(json.dumps({"what": "torch_failed", "error": note}), flush=True)
    # ---- the arbiter: the same quantities in float64 on the device (Cholesky factor and solves), block by block
    try:
        G64 = torch.from_numpy(T / cv[:, :, None]).cuda()
        P64 = torch.einsum("kdi,kdj->kij", G64, torch.from_numpy(T).cuda()).reshape(K, R * R)
        eye64 = torch.eye(R, dtype=torch.float64, device="cuda")
        A64 = torch.zeros((K, R * R), dtype=torch.float64, device="cuda")
        ew_lib = ew_tor = 0.0
        blk = 500
        for u0 in range(0, U, blk):
            n = min(blk, U - u0)
            nb = torch.from_numpy(nk[u0:u0 + n]).cuda()
            fb = torch.from_numpy((sx[u0:u0 + n] - nk[u0:u0 + n, :, None] * mu[None]).reshape(n, K * D)).cuda()
            ch = torch.linalg.cholesky((nb @ P64).view(n, R, R) + eye64)
            rhs = torch.cat([(fb @ G64.reshape(K * D, R))[:, :, None], eye64.expand(n, R, R)], dim=2)
            sol = torch.cholesky_solve(rhs, ch)
            wb, Si = sol[:, :, 0], sol[:, :, 1:]
            A64 += nb.T @ (Si + wb[:, :, None] * wb[:, None, :]).reshape(n, R * R)
            wb = wb.cpu().numpy()
            den = np.maximum(1.0, np.abs(wb).max(axis=1))
            ew_lib = max(ew_lib, float((np.abs(lib_w[u0:u0 + n] - wb).max(axis=1) / den).max()))
            if tw is not None:
                ew_tor = max(ew_tor, float((np.abs(tw[u0:u0 + n] - wb).max(axis=1) / den).max()))
        A64 = A64.view(K, R, R).cpu().numpy()
        err = {"w_lib": ew_lib, "A_lib": float(np.abs(lib_A - A64).max() / np.abs(A64).max())}
        if tw is not None and ta is not None:
            err.update({"w_torch": ew_tor, "A_torch": float(np.abs(ta - A64).max() / np.abs(A64).max())})
        print(json.dumps({"what": "against_float64", **shape, **err}), flush=True)
    except Exception as e:
        err_note = "%s: %s" % (type(e).__name__, str(e).splitlines()[0] if str(e) else "")
        print(json.dumps({"what": "float64_failed", "error": err_note}), flush=True)
    # ---- the table
    names = {"gemm_L": "precision GEMM (L = N P)", "gemm_b": "right-hand-side GEMM (b = f G)", "cholesky": "Cholesky, solves%s",
             "gemm_A": "accumulator GEMM A = N' S", "gemm_C": "accumulator GEMM C = f' W", "kernel_ms": "all stages"}
    lines = ["# i-vector extraction and the total-variability E-step (`tools/bench_ivector.py`)", "",
             "K = %d, D = %d, R = %d, %d utterances of %d frames, synthetic; slabs of %d utterances (1 GiB workspace cap); median of %d calls "
             "after one untimed call.  Device milliseconds between events; FLOP counts are the algorithm's (the docstring of the tool has "
             "them)." % (K, D, R, U, F, slab, a.reps), ""]
    for key, title in (("extract", "extract"), ("estep", "one E-step")):
        lines += ["## %s" % title, "", "| stage | library ms | TFLOP/s | torch ms | torch / library |", "|---|---|---|---|---|"]
        for st in (api.IVECTOR_STAGES[:3] if key == "extract" else api.IVECTOR_STAGES) + ("kernel_ms",):
            lm = lib[key][st]
            fl = flops.get("cholesky_estep" if (st == "cholesky" and key == "estep") else st)
            tm = tor.get(key, {}).get(st)
            label = names[st] % (", inverse and S" if key == "estep" else "") if st == "cholesky" else names[st]
            lines.append("| %s | %.2f | %s | %s | %s |" % (label, lm, "%.1f" % (fl / lm / 1e9) if fl else "—",
                                                           "%.2f" % tm if tm is not None else "not measured",
                                                           "%.2f" % (tm / lm) if tm is not None else "—"))
        lines += ["", "Wall time of a library call (host centring pass in float64, copies, kernels): %.0f ms." % lib[key]["wall_ms"], ""]
    if note:
        lines += ["The torch side was NOT measured in full: %s." % note, ""]
    if err:
        lines += ["Against the same quantities in float64 (Cholesky factor and solves in float64 on the device, same process): largest "
                  "per-utterance |w - w64| / max(1, max|w64|) library %.2g, torch fp32 %s; largest |A - A64| / max|A64| library %.2g, torch fp32 %s."
                  % (err["w_lib"], "%.2g" % err["w_torch"] if "w_torch" in err else "not measured", err["A_lib"],
                     "%.2g" % err["A_torch"] if "A_torch" in err else "not measured"), ""]
        if err.get("A_torch", 0.0) > 1e-2:
            lines += ["torch's composed E-step is WRONG at this shape (its batched cholesky_inverse; at the tests' sizes it agrees): the torch "
                      "time of the Cholesky stage of the E-step is the time of a wrong answer.", ""]
    else:
        lines += ["The float64 comparison was NOT measured: %s." % err_note, ""]
    lost = [(key, st) for key in tor for st in tor[key] if st != "kernel_ms" and tor[key][st] < lib[key][st]]
    if tor:
        lines += ["Stages the library loses to torch: %s." % (", ".join("%s of %s" % (names[st].split(" (")[0].replace("%s", ""), key) for key, st in lost) or "none"), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
