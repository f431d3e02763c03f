"""Score normalisation and detection-error counts against their yardsticks on one GPU (profiles/snorm.md).

    python tools/bench_snorm.py [--tests 1000000] [--speakers 1251] [--cohort 2048] [--top 300] [--dim 256] [--reps 10] [--out profiles/snorm.md]

The PLDA shape of profiles/plda.md (1e6 test vectors x 1251 enrolled speakers x q = 256) against a cohort of 2048 speakers, top 300, every
matrix resident in HBM.  Three steps, each in a child process of its own under its own time limit (--step-timeout); the parent never opens
the GPU, and after a child that ends on a signal or at its limit no further step is started:
  topn    ssp_topn_stats (axis 1) on the (tests x cohort) ratios, beside the cohort sweep (ssp_plda_score writing its matrix) that
          produces them, and torch.topk + mean / std in blocks of rows on the same tensor
  apply   ssp_snorm_apply in place on the (tests x speakers) ratios with both pairs of statistics and the decision, beside the enrolled
          sweep that produces them, and the same formula composed from torch broadcasting + max
  det     ssp_det_counts with 1024 thresholds on the (tests x speakers) ratios, beside the same sweep, and torch.bucketize + bincount in
          blocks of rows
Every time is the median of --reps calls after one untimed call, between device events (the library's kernel_ms; torch events).  One
JSON line per measurement; the markdown file holds the table.  Registers per lane and the absence of a private segment are read from the
compiled code (hipcc -S).  With --no-gpu only that is written and the times read "not measured yet"."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("topn", "apply", "det")


def compiled_resources():
    """-> {kernel: (registers per lane, private segment bytes)} of csrc/snorm.hip, or {} where hipcc is missing"""
    from speech_signal_processing_amd.build import CSRC, FLAGS, HIPCC, SOURCE_FLAGS
    if not os.path.exists(HIPCC):
        return {}
    r = subprocess.run([HIPCC, *FLAGS, *SOURCE_FLAGS.get("snorm.hip", []), "-S", "--cuda-device-only", "-o", "-", os.path.join(CSRC, "snorm.hip")],
                       capture_output=True, text=True)
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", r.stdout, flags=re.S):
        out[m.group(1)] = (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1)),
                           int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1)))
    return out


def med(xs):
    return float(statistics.median(xs))


def run_step(a):
    """one step in this process; prints one JSON line per measurement"""
    import torch
    from speech_signal_processing_amd import api
    N, S, Cc, q, top = a.tests, a.speakers, a.cohort, a.dim, a.top
    ctx = api.default_context()
    rng = np.random.default_rng(0)
    psi = 4.0 * np.linspace(1.0, 0.05, q)

    def scorer(n_spk):
        counts = rng.integers(1, 31, n_spk).astype(np.int32)
        y = rng.standard_normal((n_spk, q)) * np.sqrt(psi)
        return y, api.PldaScorer(ctx, psi, y + rng.standard_normal((n_spk, q)) / np.sqrt(counts)[:, None], counts)
    y, enrolled = scorer(S)
    _, cohort = scorer(Cc)
    g = torch.Generator(device="cuda").manual_seed(0)
    spk = torch.randint(0, S, (N,), generator=g, device="cuda")
    T = torch.from_numpy(y).float().cuda()[spk] + torch.randn((N, q), generator=g, device="cuda")
    shape = {"N": N, "S": S, "C": Cc, "top": top, "q": q}

    def lib_ms(fn):
        fn()
        return med([fn()["kernel_ms"] for _ in range(a.reps)])

    def torch_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def once():
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        once()
        return med([once() for _ in range(a.reps)])

    def say(what, ms, **kw):
        print(json.dumps({"what": what, **shape, "ms": round(ms, 3), **kw}), flush=True)
    blk = 65536
    if a.step == "topn":
        say("cohort_sweep", lib_ms(lambda: cohort.score(T, llr=True, timing=True)))
        tc = cohort.score(T, llr=True)["llr"]
        say("topn_stats", lib_ms(lambda: api.topn_stats(ctx, tc, top, timing=True)))
        mine = api.topn_stats(ctx, tc, top)
        mean, std = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")

        def torch_topn():
            for r0 in range(0, N, blk):
                v = torch.topk(tc[r0:r0 + blk], top, dim=1).values
                mean[r0:r0 + blk] = v.mean(dim=1)
                std[r0:r0 + blk] = v.std(dim=1, unbiased=False)
        say("torch_topk_mean_std", torch_ms(torch_topn), max_abs_diff_mean=float((mean - mine["mean"]).abs().max()),
            max_abs_diff_std=float((std - mine["std"]).abs().max()))
    elif a.step == "apply":
        say("enrolled_sweep", lib_ms(lambda: enrolled.score(T, llr=True, timing=True)))
        x = enrolled.score(T, llr=True)["llr"]
        st = api.topn_stats(ctx, cohort.score(T, llr=True)["llr"], top)
        cm = x[:4096].mean(dim=0).contiguous()
        cs = x[:4096].std(dim=0).contiguous()
        want = api.snorm_apply(ctx, x, st["mean"], st["std"], cm, cs, out=False)
        z = torch.empty_like(x)
        say("snorm_apply", lib_ms(lambda: api.snorm_apply(ctx, x, st["mean"], st["std"], cm, cs, out=z, timing=True)))
        am, mx = torch.empty(N, dtype=torch.int64, device="cuda"), torch.empty(N, device="cuda")
        cden, rden = cs.clamp(min=1e-6), st["std"].clamp(min=1e-6)

        def torch_apply():
            for r0 in range(0, N, blk):
                xb = x[r0:r0 + blk]
                zb = 0.5 * ((xb - cm) / cden + (xb - st["mean"][r0:r0 + blk, None]) / rden[r0:r0 + blk, None])
                z[r0:r0 + blk] = zb
                torch.max(zb, dim=1, out=(mx[r0:r0 + blk], am[r0:r0 + blk]))
        say("torch_broadcast_max", torch_ms(torch_apply), argmax_agreement=float((am.int() == want["argmax"]).float().mean()))
    elif a.step == "det":
        say("enrolled_sweep", lib_ms(lambda: enrolled.score(T, llr=True, timing=True)))
        x = enrolled.score(T, llr=True)["llr"]
        tgt = spk.int()
        r = api.det_counts(ctx, x, tgt)["range"]
        th = np.linspace(float(min(r[0], r[2])), float(max(r[1], r[3])), 1024).astype(np.float32)
        say("det_counts", lib_ms(lambda: api.det_counts(ctx, x, tgt, th, timing=True)), M=1024)
        mine = api.det_counts(ctx, x, tgt, th)
        tht = torch.from_numpy(th).cuda()
        hist = torch.zeros(2 * 1025, dtype=torch.int64, device="cuda")
        cols = torch.arange(S, device="cuda")

        def torch_det():
            hist.zero_()
            for r0 in range(0, N, blk):
                xb = x[r0:r0 + blk]
                b = torch.bucketize(xb, tht, right=True)
                b += (cols[None, :] != spk[r0:r0 + blk, None]) * 1025
                hist.add_(torch.bincount(b.reshape(-1), minlength=2 * 1025))
        ms = torch_ms(torch_det)
        h = hist.cpu().numpy()
        say("torch_bucketize_bincount", ms, counts_equal=bool(np.array_equal(h[:1025], mine["tar_hist"]) and np.array_equal(h[1025:], mine["non_hist"])))


def table(a, res, notes):
    reg = compiled_resources()

    def regs(tag):
        k = [v for n_, v in reg.items() if tag in n_]
        return "%d registers per lane, %s" % (k[0][0], "no private segment" if k[0][1] == 0 else "%d B private segment" % k[0][1]) if k else "not compiled here"
    nk = 4 if a.cohort <= 256 else 16 if a.cohort <= 1024 else 32 if a.cohort <= 2048 else 64 if a.cohort <= 4096 else 0

    def ms(step, what):
        v = res.get((step, what))
        return "%.2f" % v["ms"] if v else "not measured yet"
    N, S, Cc = a.tests, a.speakers, a.cohort
    lines = ["# Score normalisation and detection-error counts (`tools/bench_snorm.py`)", "",
             "%d test vectors x %d enrolled speakers against a cohort of %d, top %d, q = %d, every matrix resident in HBM; median of %d calls after "
             "one untimed call, device milliseconds between events; each step in a process of its own, the torch composition in the same process "
             "on the same tensors." % (N, S, Cc, a.top, a.dim, a.reps), "",
             "| step | library | ms | the sweep that feeds it | ms | composed from torch | ms | compiled |", "|---|---|---|---|---|---|---|---|",
             "| top-%d statistics of %d x %d | `ssp_topn_stats` | %s | `ssp_plda_score` (cohort, matrix written) | %s | `topk` + mean / std | %s | %s |" % (
                 a.top, N, Cc, ms("topn", "topn_stats"), ms("topn", "cohort_sweep"), ms("topn", "torch_topk_mean_std"),
                 regs("snorm_topn_kernelILi%dELi1E" % nk)),
             "| normalise %d x %d in place + decision | `ssp_snorm_apply` | %s | `ssp_plda_score` (enrolled, matrix written) | %s | broadcasting + `max` | %s | %s |" % (
                 N, S, ms("apply", "snorm_apply"), ms("apply", "enrolled_sweep"), ms("apply", "torch_broadcast_max"), regs("snorm_apply_kernelILb1ELb1E")),
             "| miss / false-alarm histograms, 1024 thresholds | `ssp_det_counts` | %s | `ssp_plda_score` (enrolled, matrix written) | %s | `bucketize` + `bincount` | %s | %s, %d B of LDS |" % (
                 ms("det", "det_counts"), ms("det", "enrolled_sweep"), ms("det", "torch_bucketize_bincount"), regs("snorm_det_kernel"),
                 4 * (1024 + 2 * 1025 + 2)), ""]
    t, s = res.get(("topn", "topn_stats")), res.get(("topn", "cohort_sweep"))
    if t and s:
        lines += ["The selection is not fused into the sweep's epilogue.  The condition for leaving it so is that `ssp_topn_stats` takes less time than "
                  "the cohort sweep that produces its input: %.2f ms against %.2f ms, %.0f %% of the sweep — the condition %s.  The round trip of the "
                  "(tests x cohort) matrix through HBM that a fusion would save is 2 x %.1f GB by count."
                  % (t["ms"], s["ms"], 100.0 * t["ms"] / s["ms"], "HOLDS" if t["ms"] < s["ms"] else "FAILS: the design note on not fusing is wrong",
                     4e-9 * N * Cc), ""]
    for (step, what), v in sorted(res.items()):
        extra = {k: v[k] for k in v if k not in ("what", "ms", "N", "S", "C", "top", "q")}
        if extra:
            lines.append("- %s: %s" % (what, ", ".join("%s %s" % kv for kv in sorted(extra.items()))))
    for lib, tor in (("topn_stats", "torch_topk_mean_std"), ("snorm_apply", "torch_broadcast_max"), ("det_counts", "torch_bucketize_bincount")):
        step = {"topn_stats": "topn", "snorm_apply": "apply", "det_counts": "det"}[lib]
        l_, t_ = res.get((step, lib)), res.get((step, tor))
        if l_ and t_:
            lines.append("- `ssp_%s` %s the torch composition: %.2f ms against %.2f ms (%.2f x)." % (
                lib, "beats" if l_["ms"] < t_["ms"] else "LOSES to", l_["ms"], t_["ms"], t_["ms"] / l_["ms"]))
    lines += [""] + ["%s" % n for n in notes]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines).rstrip() + "\n")
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tests", type=int, default=1000000)
    ap.add_argument("--speakers", type=int, default=1251)
    ap.add_argument("--cohort", type=int, default=2048)
    ap.add_argument("--top", type=int, default=300)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step in this process (what the parent starts)")
    ap.add_argument("--step-timeout", type=float, default=240.0)
    ap.add_argument("--no-gpu", action="store_true", help="write the table from the compiled code alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snorm.md"))
    a = ap.parse_args()
    if a.step:
        run_step(a)
        return
    res, notes = {}, []
    for step in ([] if a.no_gpu else STEPS):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [x for k in ("tests", "speakers", "cohort", "top", "dim", "reps")
                                                                              for x in ("--" + k, str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            rc, out = r.returncode, r.stdout
        except subprocess.TimeoutExpired as e:
            rc, out = 124, (e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout) or ""
        for line in out.splitlines():
            if line.startswith("{"):
                v = json.loads(line)
                res[(step, v["what"])] = v
                print(line, flush=True)
        if rc != 0:
            notes.append("Step `%s` ended with status %d: what it had not printed by then was NOT measured." % (step, rc))
            print("step %s: exit status %d\n%s" % (step, rc, (r.stderr[-2000:] if rc != 124 else "time limit")), file=sys.stderr)
            if rc < 0 or rc in (124, 134, 137, 139):
                notes.append("No further step was started after it.")
                break
    if a.no_gpu:
        notes.append("No MI355X run has been made of this tool yet: the times are not measured; the last column is read from the compiled code.")
    table(a, res, notes)


if __name__ == "__main__":
    main()
