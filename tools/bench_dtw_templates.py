"""Wall time of building every speaker's DTW template: the loop of MFCC_DTW.generate_template (one ssp_dtw_path call per (sample, template)
pair, strictly one after the other) against one MFCC_DTW.generate_templates call (round k of all speakers in one launch) in the same
process on the same arrays, after one warm-up of each.  Checks that the two results are bit-equal and prints one JSON line.

    python tools/bench_dtw_templates.py [--speakers 64] [--samples 8] [--length 1222] [--reps 3]

The default shape is 64 speakers x 8 samples of 1222 float values: the sequence length of bench.py's DTW stage.
"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speakers", type=int, default=64)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--length", type=int, default=1222)
    ap.add_argument("--reps", type=int, default=3, help="timed runs of each side (the minimum is reported)")
    a = ap.parse_args()
    from speech_signal_processing_amd import MFCC_DTW, api
    rng = np.random.default_rng(0)
    groups = [[rng.standard_normal(a.length).astype(np.float32).astype(np.float64) for _ in range(a.samples)] for _ in range(a.speakers)]
    loop_fn = lambda: [MFCC_DTW.generate_template(g) for g in groups]  # noqa: E731
    many_fn = lambda: MFCC_DTW.generate_templates(groups)  # noqa: E731
    ref = loop_fn()      # warm-up of each side at full size; also the results that are compared
    got = many_fn()
    equal = len(ref) == len(got) and all(r.dtype == g.dtype and r.shape == g.shape and np.array_equal(r, g) for r, g in zip(ref, got))
    t_loop = min(timed(loop_fn)[0] for _ in range(a.reps))
    t_many = min(timed(many_fn)[0] for _ in range(a.reps))
    t_prof, (_, kernel_ms) = timed(lambda: api.dtw_templates(api.default_context(), groups, timing=True))
    res = {"speakers": a.speakers, "samples": a.samples, "length": a.length, "pairs": a.speakers * (a.samples - 1), "reps": a.reps,
           "loop_s": round(t_loop, 4), "batched_s": round(t_many, 4), "speedup": round(t_loop / t_many, 2),
           "batched_kernel_ms": round(kernel_ms, 3), "timed_run_s": round(t_prof, 4), "bit_equal": bool(equal)}
    print(json.dumps(res), flush=True)
    if not equal:
        sys.exit("generate_templates differs from the loop of generate_template")
    if not t_many < t_loop:
        sys.exit("the batched call is not faster than the loop")


if __name__ == "__main__":
    main()
