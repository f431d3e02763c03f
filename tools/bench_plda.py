"""The PLDA back end against its yardsticks, in one process on one GPU (profiles/plda.md).

    python tools/bench_plda.py [--tests 1000000] [--speakers 1251] [--dim 256] [--reps 20] [--out profiles/plda.md]

Scoring at the cosine row's shape (1e6 test vectors x 1251 speakers x q = 256, resident in HBM, arg-max and maximum only): the
class-shared path with enrolment counts drawn from 1..30, and the general path through PLDA_NO_CLASS_PATH, against
  ssp_cosine_identify precision 0 on the same shape — the same matrix work as the class-shared path: the yardstick for the kernel;
  the same ratio composed from torch: two matmuls (T beta', T^2 (-alpha/2)') plus the broadcast of c and an arg-max, TF32 off, in blocks
  of rows so that the (rows x speakers) matrix fits.
ssp_plda_stats at N = 1e6, q = 256, S = 1251 against torch's index_add_ (float64 sums) plus a float32 matmul of the centred rows.
plda.Plda.fit wall time on 100000 of those rows (10 iterations), with the host EM's share.
Every time is the median of --reps calls after one untimed call, between device events on the stream the work runs on (the library's
kernel_ms; torch events).  Counted flops: 2 N S q for a sweep (4 N S q on the general path), 2 N q^2 / 2 for the scatter product (the
blocks on or below the diagonal).  The fraction of the fp32-input MFMA peak is that over 157.3 TFLOP/s.  One JSON line per measurement;
the markdown file holds the table.  Registers per lane are read from the compiled code (hipcc -S); the kernels take their LDS
dynamically, so LDS per workgroup is computed here by the launchers' formula (ring of three half tiles, or the staging area where that
is larger, plus four 4 KiB class tables on the class-shared path)."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP32_MFMA_PEAK_TFLOPS = 157.3


def compiled_resources():
    """-> {kernel: registers per lane} of csrc/plda.hip, or {} where hipcc is missing"""
    from speech_signal_processing_amd.build import CSRC, FLAGS, HIPCC, SOURCE_FLAGS
    if not os.path.exists(HIPCC):
        return {}
    r = subprocess.run([HIPCC, *FLAGS, *SOURCE_FLAGS.get("plda.hip", []), "-S", "--cuda-device-only", "-o", "-", os.path.join(CSRC, "plda.hip")],
                       capture_output=True, text=True)
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", r.stdout, flags=re.S):
        out[m.group(1)] = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tests", type=int, default=1000000)
    ap.add_argument("--speakers", type=int, default=1251)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fit-rows", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plda.md"))
    a = ap.parse_args()
    import torch
    from speech_signal_processing_amd import api, plda
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    N, S, q = a.tests, a.speakers, a.dim
    ctx = api.default_context()
    rng = np.random.default_rng(0)
    psi = 4.0 * np.linspace(1.0, 0.05, q)
    counts = rng.integers(1, 31, S).astype(np.int32)
    y = rng.standard_normal((S, q)) * np.sqrt(psi)
    enrol = y + rng.standard_normal((S, q)) / np.sqrt(counts)[:, None]
    g = torch.Generator(device="cuda").manual_seed(0)
    spk = torch.randint(0, S, (N,), generator=g, device="cuda")
    T = torch.from_numpy(y).float().cuda()[spk] + torch.randn((N, q), generator=g, device="cuda")
    shape = {"N": N, "S": S, "q": q}

    def med(xs):
        return float(statistics.median(xs))

    def lib_ms(fn):
        fn()
        return med([fn()["kernel_ms"] for _ in range(a.reps)])

    res = {}
    sweep = 2.0 * N * S * q
    shared = api.PldaScorer(ctx, psi, enrol, counts)
    general = api.PldaScorer(ctx, psi, enrol, counts, flags=api.PLDA_NO_CLASS_PATH)
    assert shared.class_shared and not general.class_shared
    res["plda_shared"] = lib_ms(lambda: shared.score(T, timing=True))
    res["plda_general"] = lib_ms(lambda: general.score(T, timing=True))
    same = bool((shared.score(T)["argmax"] == general.score(T)["argmax"]).float().mean() > 0.999)
    Cn = torch.from_numpy(enrol).float().cuda()
    res["cosine"] = lib_ms(lambda: api.cosine_identify(ctx, T, Cn, precision=0, timing=True))
    for k in ("plda_shared", "plda_general", "cosine"):
        print(json.dumps({"what": k, **shape, "ms": round(res[k], 3)}), flush=True)
    # ---- torch: the packed form, in blocks of rows
    torch_note = None
    try:
        n = counts.astype(np.float64)[:, None]
        den = n * psi + 1.0
        mean, var = n * psi * enrol / den, 1.0 + psi / den
        beta = torch.from_numpy(mean / var).float().cuda()
        ha = torch.from_numpy(-0.5 * (1.0 / var - 1.0 / (1.0 + psi))).float().cuda()
        c = torch.from_numpy(-0.5 * (np.log(var) - np.log1p(psi) + mean * mean / var).sum(axis=1)).float().cuda()
        blk = 65536
        am, mx = torch.empty(N, dtype=torch.int64, device="cuda"), torch.empty(N, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def once():
            e0.record()
            for r0 in range(0, N, blk):
                t = T[r0:r0 + blk]
                llr = t @ beta.T
                llr.addmm_(t * t, ha.T)
                llr += c
                torch.max(llr, dim=1, out=(mx[r0:r0 + blk], am[r0:r0 + blk]))
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        once()
        res["torch_llr"] = med([once() for _ in range(a.reps)])
        agree = float((am.int() == shared.score(T)["argmax"]).float().mean())
        print(json.dumps({"what": "torch_llr", **shape, "ms": round(res["torch_llr"], 3), "argmax_agreement": agree}), flush=True)
        del beta, ha, c, am, mx
    except Exception as e:  # the torch side is a comparison, not a dependency: say what was not measured
        torch_note = "%s: %s" % (type(e).__name__, str(e).splitlines()[0] if str(e) else "")
        print(json.dumps({"what": "torch_llr_failed", "error": torch_note}), flush=True)
    # ---- statistics
    lab = spk.int()
    res["stats"] = lib_ms(lambda: api.plda_stats(ctx, T, lab, S, timing=True))
    print(json.dumps({"what": "plda_stats", **shape, "ms": round(res["stats"], 3)}), flush=True)
    stats_note = None
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        idx = spk.long()

        def once_stats():
            e0.record()
            sums = torch.zeros((S, q), dtype=torch.float64, device="cuda").index_add_(0, idx, T.double())
            cnt = torch.bincount(idx, minlength=S).clamp(min=1)
            sw = torch.zeros((q, q), device="cuda")
            m = (sums / cnt[:, None]).float()
            for r0 in range(0, N, 131072):
                xc = T[r0:r0 + 131072] - m[idx[r0:r0 + 131072]]
                sw.addmm_(xc.T, xc)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        once_stats()
        res["torch_stats"] = med([once_stats() for _ in range(a.reps)])
        print(json.dumps({"what": "torch_stats", **shape, "ms": round(res["torch_stats"], 3)}), flush=True)
    except Exception as e:
        stats_note = "%s: %s" % (type(e).__name__, str(e).splitlines()[0] if str(e) else "")
        print(json.dumps({"what": "torch_stats_failed", "error": stats_note}), flush=True)
    # ---- fit
    nf = min(a.fit_rows, N)
    Xf, lf = T[:nf].cpu().numpy(), spk[:nf].cpu().numpy().astype(np.int32)
    _, lf = np.unique(lf, return_inverse=True)
    model = plda.Plda(n_iter=10, ctx=ctx)
    model.fit(Xf, lf)
    t0 = time.perf_counter()
    model.fit(Xf, lf)
    fit_s = time.perf_counter() - t0
    st = plda.class_stats(model._front(Xf), lf, ctx=ctx)
    t0 = time.perf_counter()
    model._fit_stats(st)
    em_s = time.perf_counter() - t0
    print(json.dumps({"what": "fit", "rows": nf, "q": q, "classes": int(lf.max()) + 1, "wall_s": round(fit_s, 3), "host_em_s": round(em_s, 3)}), flush=True)
    # ---- the table
    reg = compiled_resources()
    nq = 8 if q <= 64 else 16 if q <= 128 else 24 if q <= 192 else 32
    ring = max(3 * nq * 128 * 4, 4 * 32 * 65 * 4)

    def regs(tag):
        k = [v for n_, v in reg.items() if "plda_score_kernelILi%dE%s" % (nq, tag) in n_]
        return "%d" % k[0] if k else "not measured"

    def row(name, ms, flops, vg, lds):
        return "| %s | %.2f | %.1f | %.1f %% | %s | %s |" % (name, ms, flops / ms / 1e9, 100.0 * flops / ms / 1e9 / FP32_MFMA_PEAK_TFLOPS, vg, lds)
    lines = ["# PLDA back end: scoring, statistics and fit (`tools/bench_plda.py`)", "",
             "%d test vectors x %d speakers x q = %d, resident in HBM, arg-max and maximum only; enrolment counts drawn from 1..30 (%d classes); "
             "median of %d calls after one untimed call, device milliseconds between events.  Counted flops: 2 N S q per sweep (4 N S q on the "
             "general path); peak = %.1f TFLOP/s (fp32-input MFMA)." % (N, S, q, shared.n_classes, a.reps, FP32_MFMA_PEAK_TFLOPS), "",
             "| sweep | ms | TFLOP/s | of fp32 MFMA peak | registers per lane (compiled) | LDS per workgroup (computed) |", "|---|---|---|---|---|---|",
             row("`ssp_plda_score`, class-shared path", res["plda_shared"], sweep, regs("Lb1E"), "%d B" % (ring + 16384)),
             row("`ssp_plda_score`, general path (flag)", res["plda_general"], 2 * sweep, regs("Lb0E"), "%d B" % ring),
             row("`ssp_cosine_identify` precision 0", res["cosine"], sweep, "—", "%d B" % ring)]
    if "torch_llr" in res:
        lines.append(row("torch: two matmuls + broadcast + max, TF32 off", res["torch_llr"], 2 * sweep, "—", "—"))
    else:
        lines += ["", "The torch composition was NOT measured: %s." % torch_note]
    ratio = res["plda_shared"] / res["cosine"]
    lines += ["", "Class-shared path / cosine sweep measured beside it: %.2f.  General path / class-shared path: %.2f.  The two paths agree on the "
              "arg-max of more than 99.9 %% of the rows: %s." % (ratio, res["plda_general"] / res["plda_shared"], "yes" if same else "NO"), ""]
    if ratio > 1.3:
        lines += ["The class-shared path takes more than 1.3 x the cosine sweep.  The stage that loses is occupancy, and two figures hold it down: "
                  "%s registers per lane under __launch_bounds__(256, 2) (two waves per SIMD whatever the LDS is; the cosine sweep is built for "
                  "three, at most 168), and ring (%d B) + 4 class tables (16384 B) = %d B of LDS per workgroup (two workgroups per CU whatever the "
                  "registers are; the cosine sweep takes %d B).  The MFMA chain of a wave is covered by one partner wave per SIMD instead of two.  "
                  "The epilogue (a float4 of c, an int4 of classes and 16 table reads per tile of 128 MFMAs) and the one extra tile are small "
                  "beside that.  (Read from the compiled code and the launcher's formula; no counter run has isolated it.)"
                  % (regs("Lb1E"), ring, ring + 16384, ring), ""]
    lines += ["## Class statistics", "", "`ssp_plda_stats` at N = %d, q = %d, S = %d (device arrays; one host wait): %.2f ms of kernels%s.  Counted on "
              "the scatter product alone (N q^2 flops on or below the diagonal): %.1f TFLOP/s." % (
                  N, q, S, res["stats"], "; torch index_add_ (float64) + centred float32 matmul in blocks: %.2f ms" % res["torch_stats"]
                  if "torch_stats" in res else "; the torch side was NOT measured: %s" % stats_note, N * q * q / res["stats"] / 1e9), "",
              "## Fit", "", "`plda.Plda(n_iter=10).fit` on %d rows of q = %d in %d classes (host arrays, length normalisation on): %.2f s wall, of "
              "which the host EM and diagonalisation %.2f s." % (nf, q, int(lf.max()) + 1, fit_s, em_s), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
