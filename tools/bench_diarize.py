"""Pair scores and batched agglomerative clustering against their yardsticks on one GPU (profiles/diarize.md).

    python tools/bench_diarize.py [--points design,small] [--reps 5] [--workers 16] [--scipy-recordings 64] [--out FILE.jsonl]

Two points, each in a child process of its own under its own time limit (--step-timeout); the parent never opens the GPU, and after a
child that ends on a signal or at its limit no further point is started:
  design  256 recordings x 800 windows x q = 256 (ten-minute recordings at 1.5 s / 0.75 s windows): the workspace-resident clustering
  small   4096 recordings x 150 windows x q = 256: the LDS-resident clustering
Per point, in the same process:
  ssp_pairwise_scores (kernel_ms, device events) beside torch.bmm(X, X^T) on the batch (the recordings are of equal length: no padding),
  TF32 off; ssp_ahc_cluster at threshold 0.5 and run down to 4 clusters (threshold -inf: n - 4 merges in every recording) beside
  scipy.cluster.hierarchy.linkage + fcluster (average linkage, threshold 0.5) on the same matrices on the host, in one process and in a
  pool of --workers processes (on --scipy-recordings of the recordings, scaled to the batch; a step of its own, in a process that
  never opens the GPU).  Every device time is the median of --reps calls after one untimed call.
The time of a merge step is the clustering time divided by the merges of one recording and by the rounds of workgroups the launch needs
(recordings / (CUs x workgroups resident per CU), rounded up).  One JSON line per measurement."""
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
POINTS = {"design": (256, 800, 256), "small": (4096, 150, 256)}


def _scipy_one(args):
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    S, method, thr = args
    D = 1.0 - S.astype(np.float64)
    np.fill_diagonal(D, 0.0)
    return fcluster(linkage(squareform(D, checks=False), method=method), t=1.0 - thr, criterion="distance")


def run_point(a):
    import torch
    from speech_signal_processing_amd import api
    R, n, q = POINTS[a.point]
    torch.backends.cuda.matmul.allow_tf32 = False
    ctx = api.default_context()
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = torch.nn.functional.normalize(torch.randn((R, 4, q), generator=g, device="cuda"), dim=2)  # four speakers per recording
    who = torch.randint(0, 4, (R, n), generator=g, device="cuda")
    X = torch.gather(centres, 1, who[:, :, None].expand(R, n, q)) + 0.5 * torch.randn((R, n, q), generator=g, device="cuda") / q ** 0.5
    X = api.l2_normalize(ctx, X.reshape(R * n, q).contiguous())
    seg = api.Segments.from_lengths(ctx, [n] * R)
    shape = {"point": a.point, "R": R, "n": n, "q": q}

    def say(what, ms, **kw):
        print(json.dumps({"what": what, **shape, "ms": round(ms, 3), **kw}), flush=True)

    def med(fn):
        fn()
        return float(statistics.median(fn() for _ in range(a.reps)))
    out = torch.empty(R * n * n, device="cuda")
    say("pairwise_scores", med(lambda: api.pairwise_scores(ctx, X, seg, out=out, timing=True)[1]))
    Xb, ref = X.view(R, n, q), torch.empty((R, n, n), device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def bmm():
        e0.record()
        torch.bmm(Xb, Xb.transpose(1, 2), out=ref)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    say("torch_bmm_fp32", med(bmm), max_abs_diff=float((ref.reshape(-1) - out).abs().max()))
    del ref
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lds = (n * (n | 1) + 5 * n + 16) * 4 if n <= api.AHC_N_LDS else (5 * n + 16) * 4
    resident = max(1, min(8, (160 * 1024) // (lds + 64)))
    rounds = -(-R // (cus * resident))
    for linkage in ("average", "complete", "single"):
        for what, kw, merges in (("ahc_threshold_0.5", {"threshold": 0.5}, None), ("ahc_to_4_clusters", {"threshold": float("-inf"), "min_clusters": 4}, n - 4)):
            ms = med(lambda: api.ahc_cluster(ctx, out, seg, linkage=linkage, timing=True, **kw)["kernel_ms"])
            r = api.ahc_cluster(ctx, out, seg, linkage=linkage, **kw)
            if merges is None:
                merges = n - int(r["n_clusters"].min())
            say(what, ms, linkage=linkage, merges_per_recording=merges, workgroup_rounds=rounds,
                us_per_merge_step=round(1e3 * ms / max(merges, 1) / rounds, 3), mean_clusters=float(r["n_clusters"].float().mean()))
    # the matrices and labels of --scipy-recordings recordings, for the host step (run by the parent in a process that never opens the GPU)
    k = min(R, a.scipy_recordings)
    mine = api.ahc_cluster(ctx, out, seg, linkage="average", threshold=0.5)["labels"].cpu().numpy().reshape(R, n)[:k]
    np.savez(a.scipy_file, S=out[:k * n * n].cpu().numpy().reshape(k, n, n), labels=mine, R=R)


def run_scipy(a):
    """SciPy's linkage + fcluster on the saved matrices: one process, then a pool of --workers processes; scaled to the batch"""
    with np.load(a.scipy_file) as z:
        S, mine, R = z["S"], z["labels"], int(z["R"])
    k, n = S.shape[0], S.shape[1]
    shape = {"point": a.point, "R": R, "n": n}
    jobs = [(S[i], "average", 0.5) for i in range(k)]
    t0 = time.perf_counter()
    sp = [_scipy_one(j) for j in jobs]
    one = (time.perf_counter() - t0) * 1e3
    agree = sum(len(set(zip(m.tolist(), s.tolist()))) == len(set(s.tolist())) == len(set(m.tolist())) for m, s in zip(mine, sp))
    print(json.dumps({"what": "scipy_linkage_fcluster_one_process", **shape, "ms": round(one * R / k, 1), "measured_recordings": k,
                      "same_partition_as_device": agree}), flush=True)
    from multiprocessing import get_context
    with get_context("spawn").Pool(a.workers) as pool:
        pool.map(_scipy_one, jobs[:a.workers])
        t0 = time.perf_counter()
        pool.map(_scipy_one, jobs, chunksize=max(1, k // (4 * a.workers)))
        many = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"what": "scipy_linkage_fcluster_pool", **shape, "ms": round(many * R / k, 1), "measured_recordings": k,
                      "workers": a.workers}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="design,small")
    ap.add_argument("--point", default=None, help="(internal) run this point in this process")
    ap.add_argument("--scipy-file", default=None, help="(internal) where the device step leaves the matrices of the host step")
    ap.add_argument("--scipy-only", action="store_true", help="(internal) the host step")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--scipy-recordings", type=int, default=64)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.point:
        return run_scipy(a) if a.scipy_only else run_point(a)
    import tempfile
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        steps = [(point, host) for point in a.points.split(",") for host in (False, True)]
        for point, host in steps:
            cmd = [sys.executable, os.path.abspath(__file__), "--point", point, "--reps", str(a.reps), "--workers", str(a.workers),
                   "--scipy-recordings", str(a.scipy_recordings), "--scipy-file", os.path.join(tmp, point + ".npz")] + (["--scipy-only"] if host else [])
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
