"""VB-HMM resegmentation beside the clustering it follows and against its float64 restatement, on one GPU (profiles/vbhmm.md).

    python tools/bench_vbhmm.py [--points design,small] [--reps 5] [--workers 16] [--numpy-recordings 8] [--out FILE.jsonl]

The diarization design points of tools/bench_diarize.py with S = 16 states, each in a child process of its own under its own time limit
(--step-timeout); the parent never opens the GPU, and after a child that ends on a signal or at its limit no further point is started:
  design  256 recordings x 800 windows x q = 256          small   4096 recordings x 150 windows x q = 256
Per point, in the same process: ssp_pairwise_scores and ssp_ahc_cluster (PLDA scores, threshold 0) on the batch, then ssp_vbhmm_resegment
on the same rows fed the AHC outputs on the device, at ten iterations run to the end (epsilon = -inf) and with the default early stop
(kernel_ms, device events; the median of --reps calls after one untimed call).  Then, in a process that never opens the GPU, the float64
numpy restatement (tests/vbhmm_oracle.resegment, ten iterations) on --numpy-recordings of the recordings with the labels the device's AHC
gave, in one process and in a pool of --workers processes, scaled to the batch.
The time of a recording-iteration is the call's time divided by the iterations and by the rounds of workgroups the launch needs
(recordings / (CUs x workgroups resident per CU), rounded up); the time of a time step is that divided by the windows of a recording.
One JSON line per measurement."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
POINTS = {"design": (256, 800, 256), "small": (4096, 150, 256)}
STATES, ITERS = 16, 10


def _numpy_one(args):
    import vbhmm_oracle as VO
    X, phi, lab, ni = args
    r = VO.resegment(X, phi, lab, ni, S=STATES, max_iters=ITERS, epsilon=-np.inf)
    return r["labels"]


def run_point(a):
    import torch
    from speech_signal_processing_amd import api, plda
    R, n, q = POINTS[a.point]
    ctx = api.default_context()
    g = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.RandomState(0)
    phi = (4.0 * np.sort(rng.gamma(2.0, 0.5, q))[::-1]).astype(np.float32)
    means = torch.randn((R, 4, q), generator=g, device="cuda") * torch.from_numpy(np.sqrt(phi)).cuda()[None, None, :]   # four speakers per recording
    who = torch.randint(0, 4, (R, n // 5 + 1), generator=g, device="cuda").repeat_interleave(5, dim=1)[:, :n]       # in runs of five windows
    X = (torch.gather(means, 1, who[:, :, None].expand(R, n, q)) + torch.randn((R, n, q), generator=g, device="cuda")).reshape(R * n, q).contiguous()
    seg = api.Segments.from_lengths(ctx, [n] * R)
    shape = {"point": a.point, "R": R, "n": n, "q": q, "S": STATES}

    def say(what, ms, **kw):
        print(json.dumps({"what": what, **shape, "ms": round(ms, 3), **kw}), flush=True)

    def med(fn):
        fn()
        return float(statistics.median(fn() for _ in range(a.reps)))
    gg, hh, c0 = plda.pairwise_coeffs(phi.astype(np.float64))
    scores = torch.empty(R * n * n, device="cuda")
    say("pairwise_scores", med(lambda: api.pairwise_scores(ctx, X, seg, g=gg, h=hh, c0=c0, out=scores, timing=True)[1]))
    say("ahc_threshold_0", med(lambda: api.ahc_cluster(ctx, scores, seg, threshold=0.0, timing=True)["kernel_ms"]))
    ahc = api.ahc_cluster(ctx, scores, seg, threshold=0.0)
    del scores
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sp = api.vbhmm_padded_states(STATES)
    lds = (sp * (q | 1) * 4 if api.vbhmm_alpha_in_lds(STATES, q) else 0) + (8 * n * sp if n <= api.vbhmm_n_lds(STATES, q) else 0) + 3088
    resident = max(1, min(4, (160 * 1024) // lds))
    rounds = -(-R // (cus * resident))
    for what, eps in (("vbhmm_10_iterations", float("-inf")), ("vbhmm_early_stop_1e-4", 1e-4)):
        def call():
            return api.vb_resegment(ctx, X, seg, phi, ahc["labels"], ahc["n_clusters"], n_states=STATES, max_iters=ITERS, epsilon=eps, want=(),
                                    timing=True)
        ms = med(lambda: call()["kernel_ms"])
        r = call()
        iters = float(r["n_iters"].float().mean())
        worst = int(r["n_iters"].max())
        say(what, ms, mean_iterations=round(iters, 2), max_iterations=worst, workgroup_rounds=rounds, workgroups_per_cu=resident,
            us_per_recording_iteration=round(1e3 * ms / worst / rounds, 2), us_per_time_step=round(1e3 * ms / worst / rounds / n, 4),
            amortised_us_per_recording_iteration=round(1e3 * ms / (R * iters), 3), mean_speakers=float(r["n_speakers"].float().mean()),
            mean_ahc_clusters=float(ahc["n_clusters"].float().mean()))
    k = min(R, a.numpy_recordings)
    full = api.vb_resegment(ctx, X, seg, phi, ahc["labels"], ahc["n_clusters"], n_states=STATES, max_iters=ITERS, epsilon=float("-inf"), want=())
    np.savez(a.host_file, X=X[:k * n].cpu().numpy().reshape(k, n, q), phi=phi, lab=ahc["labels"][:k * n].cpu().numpy().reshape(k, n),
             ni=ahc["n_clusters"][:k].cpu().numpy(), mine=full["labels"][:k * n].cpu().numpy().reshape(k, n), R=R)


def run_numpy(a):
    """the float64 restatement on the saved recordings: one process, then a pool of --workers processes; scaled to the batch"""
    with np.load(a.host_file) as z:
        X, phi, lab, ni, mine, R = z["X"], z["phi"], z["lab"], z["ni"], z["mine"], int(z["R"])
    k, n = X.shape[0], X.shape[1]
    shape = {"point": a.point, "R": R, "n": n, "S": STATES}
    jobs = [(X[i], phi, lab[i], int(ni[i])) for i in range(k)]
    t0 = time.perf_counter()
    ref = [_numpy_one(j) for j in jobs]
    one = (time.perf_counter() - t0) * 1e3
    agree = sum(bool(np.array_equal(m, r)) for m, r in zip(mine, ref))
    print(json.dumps({"what": "numpy_float64_one_process", **shape, "ms": round(one * R / k, 1), "measured_recordings": k,
                      "same_labels_as_device": agree, "us_per_recording_iteration": round(1e3 * one / k / ITERS, 1)}), flush=True)
    from multiprocessing import get_context
    many_jobs = jobs * max(1, -(-a.workers // k))
    with get_context("spawn").Pool(a.workers) as pool:
        pool.map(_numpy_one, many_jobs[:a.workers])
        t0 = time.perf_counter()
        pool.map(_numpy_one, many_jobs, chunksize=1)
        many = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"what": "numpy_float64_pool", **shape, "ms": round(many * R / len(many_jobs), 1), "measured_recordings": len(many_jobs),
                      "workers": a.workers}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="design,small")
    ap.add_argument("--point", default=None, help="(internal) run this point in this process")
    ap.add_argument("--host-file", default=None, help="(internal) where the device step leaves the recordings of the host step")
    ap.add_argument("--numpy-only", action="store_true", help="(internal) the host step")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--numpy-recordings", type=int, default=8)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.point:
        return run_numpy(a) if a.numpy_only else run_point(a)
    import tempfile
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        steps = [(point, host) for point in a.points.split(",") for host in (False, True)]
        for point, host in steps:
            cmd = [sys.executable, os.path.abspath(__file__), "--point", point, "--reps", str(a.reps), "--workers", str(a.workers),
                   "--numpy-recordings", str(a.numpy_recordings), "--host-file", os.path.join(tmp, point + ".npz")] + (["--numpy-only"] if host else [])
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                print("point %s ran into its time limit: no further step is started" % point, file=sys.stderr)
                break
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                print("point %s ended with status %d: no further step is started" % (point, r.returncode), file=sys.stderr)
                break
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
