"""List-fed host entry points against the concatenating recipes they replace (one process, GPU).

    python tools/list_feed_bench.py [--utts 2000] [--reps 7] [--out FILE]

Workload: --utts seeded int16 utterances of 3 s at 16 kHz, one pageable array each (as bench.py --full builds them for
extract_feature_shim).  Times, with alternating repeats after a warm-up, medians reported:
  old_recipe      flatten_signals + MfccPlan.run + astype(float64) + per-utterance views (what GMM_UBM.extract_feature did)
  run_list        api.mfcc_run_list(out_dtype=float64) + views
  extract_feature GMM_UBM.extract_feature as routed now
  score_old / score_list   the scoring of those float64 feature matrices: vstack + astype + GmmScorer.score against score_list
It also measures the pinned host-to-device rate over the same input bytes (frac_of_pcie_bound = that copy's time / run_list's median),
reads the pipeline's split from one SSP_HOST_TRACE=1 call, checks that old and new outputs are bit-equal, and prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stderr_of(fn):
    """runs fn() with file descriptor 2 sent to a temporary file; returns (fn's result, what was written)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            r = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return r, f.read().decode("utf-8", "replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from speech_signal_processing_amd import GMM_UBM, api

    n_samp = 48000
    rng = np.random.default_rng(2024)
    big = rng.integers(-8000, 8000, args.utts * n_samp).astype(np.int16)
    xs = [np.array(big[i * n_samp:(i + 1) * n_samp]) for i in range(args.utts)]   # pageable, one array per utterance
    y = [0] * args.utts
    plan = GMM_UBM._feature_plan('MFCC', 16000, 1)

    def old_recipe():
        flat, lens = api.flatten_signals(xs)
        seg = api.Segments.from_lengths(plan.ctx, lens)
        fseg = plan.frame_segments(seg)
        feats = np.asarray(plan.run(flat, seg, fseg), dtype=np.float64)
        return [feats[fseg.offsets[i]:fseg.offsets[i + 1]] for i in range(len(lens))]

    def run_list():
        feats, fseg = api.mfcc_run_list(plan, xs, out_dtype=np.float64)
        return [feats[fseg.offsets[i]:fseg.offsets[i + 1]] for i in range(fseg.n)]

    def extract():
        return GMM_UBM.extract_feature(xs, y)[0]

    mfcc_fns = {"old_recipe": old_recipe, "run_list": run_list, "extract_feature": extract}
    for fn in mfcc_fns.values():   # warm-up: plans, pinned slots, worker threads, allocator
        fn()
        fn()
    times = {k: [] for k in mfcc_fns}
    for _ in range(args.reps):
        for k, fn in mfcc_fns.items():
            t0 = time.perf_counter()
            r = fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
            del r
    med = {k: float(np.median(v)) for k, v in times.items()}

    a, b, c = old_recipe(), run_list(), extract()
    mfcc_equal = len(a) == len(b) == len(c) and all(np.array_equal(p, q) and np.array_equal(p, r) for p, q, r in zip(a, b, c))
    frames = int(sum(f.shape[0] for f in a))
    feats64 = c
    del a, b

    # pinned host -> device over the same input bytes
    pin = torch.from_numpy(big).pin_memory()
    dev = torch.empty_like(pin, device="cuda")
    for _ in range(3):
        dev.copy_(pin, non_blocking=True)
    torch.cuda.synchronize()
    h2d = []
    for _ in range(args.reps):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        dev.copy_(pin, non_blocking=True)
        ev1.record()
        ev1.synchronize()
        h2d.append(ev0.elapsed_time(ev1))
    h2d_ms = float(np.median(h2d))
    in_bytes = big.nbytes
    del pin, dev

    # the split of one list-fed call (SSP_HOST_TRACE=1: device events per slice, host time of the copying threads)
    os.environ["SSP_HOST_TRACE"] = "1"
    try:
        _, trace = _stderr_of(run_list)
    finally:
        del os.environ["SSP_HOST_TRACE"]
    split = {}
    rows = [tuple(float(v) for v in m.groups()) for m in re.finditer(r"slice +\d+: +([\d.]+) +([\d.]+) +([\d.]+)", trace)]
    if rows:
        split["slices"] = len(rows)
        split["device_ms_last_copy_in_done"] = rows[-1][0]
        split["device_ms_last_kernels_done"] = rows[-1][1]
        split["device_ms_last_copy_back_done"] = rows[-1][2]
        split["device_ms_per_slice"] = [list(r) for r in rows]
    m = re.search(r"list: (\d+) copying threads; host ms: gather ([\d.]+), copy-back waits ([\d.]+), features out ([\d.]+)", trace)
    if m:
        split.update(threads=int(m.group(1)), host_ms_gather=float(m.group(2)), host_ms_copy_back_waits=float(m.group(3)),
                     host_ms_features_out_f64=float(m.group(4)))
    m = re.search(r"one piece: (\d+) copying threads; host ms: gather ([\d.]+), features out ([\d.]+)", trace)
    if m:
        split.update(threads=int(m.group(1)), host_ms_gather=float(m.group(2)), host_ms_features_out_f64=float(m.group(3)), one_piece=True)

    # scoring of the float64 feature matrices: old recipe (vstack + astype + score) against score_list, as score_matrix now runs it
    S, K, D = 10, 64, feats64[0].shape[1]
    srng = np.random.default_rng(7)
    ctx = api.default_context()
    scorer = api.GmmScorer(ctx, srng.dirichlet(4 * np.ones(K), size=S + 1), 0.5 * srng.standard_normal((S + 1, K, D)),
                           srng.uniform(0.5, 2.0, (S + 1, K, D)), has_ubm=True)

    def score_old():
        fseg = api.Segments.from_lengths(ctx, [len(f) for f in feats64])
        flat = np.ascontiguousarray(np.vstack(feats64), dtype=np.float32)
        return scorer.score(flat, fseg, scores=True, argmax=True)

    def score_new():
        return scorer.score_list(feats64)

    sfns = {"score_old": score_old, "score_list": score_new}
    for fn in sfns.values():
        fn()
        fn()
    st = {k: [] for k in sfns}
    for _ in range(args.reps):
        for k, fn in sfns.items():
            t0 = time.perf_counter()
            fn()
            st[k].append((time.perf_counter() - t0) * 1e3)
    smed = {k: float(np.median(v)) for k, v in st.items()}
    ro, rn = score_old(), score_new()
    score_equal = np.array_equal(ro["scores"], rn["scores"]) and np.array_equal(ro["argmax"], rn["argmax"])
    os.environ["SSP_HOST_TRACE"] = "1"
    try:
        _, strace = _stderr_of(score_new)
    finally:
        del os.environ["SSP_HOST_TRACE"]
    m = re.search(r"gmm list: (\d+) copying threads; host ms: gather ([\d.]+)", strace)
    sgather = float(m.group(2)) if m else None

    res = {
        "what": "%d int16 utterances of 3 s at 16 kHz, one pageable array each; sidekit MFCC + delta + cmvn (26-d) -> float64" % args.utts,
        "utterances": args.utts, "frames": frames, "bytes_in": in_bytes, "reps": args.reps,
        "mfcc_ms_median": med, "mfcc_ms_all": times,
        "speedup_run_list_vs_old": med["old_recipe"] / med["run_list"],
        "speedup_extract_feature_vs_old": med["old_recipe"] / med["extract_feature"],
        "frames_per_s_extract_feature": frames / (med["extract_feature"] * 1e-3),
        "pinned_h2d_ms": h2d_ms, "pinned_h2d_gbs": in_bytes / (h2d_ms * 1e-3) / 1e9,
        "frac_of_pcie_bound": h2d_ms / med["run_list"],
        "split": split,
        "mfcc_bit_equal": bool(mfcc_equal),
        "score": {"models": S + 1, "K": K, "D": D, "ms_median": smed, "ms_all": st, "speedup": smed["score_old"] / smed["score_list"],
                  "host_ms_gather_narrow": sgather, "bit_equal": bool(score_equal)},
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
            f.write(trace)
            f.write(strace)
    return 0 if (mfcc_equal and score_equal) else 1


if __name__ == "__main__":
    sys.exit(main())
