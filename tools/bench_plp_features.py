#!/usr/bin/env python
"""The fused PLP tail (ssp_plp_features) next to the chain of kernels it replaces, measured in the same process on the same device arrays.

    python tools/bench_plp_features.py [--utt3s 100000] [--chunks 300000] [--e2e 2000] [--reps 5] [--inner 3]

Batches, resident in HBM: --utt3s utterances of 3 s (298 frames, the PLP row's batch) and --chunks chunks of 1 s (98 frames, the d-vector
row's batch), 16 kHz noise through the PLP front-end plan (21 Bark bands).  For delta_order 1, scale 1, float32 rows, with and without a
26-column left block, per batch:

  fused_ms / composed_ms   one ssp_plp_features call on its fused path and with SSP_PLP_FEATURES=composed (RASTA, cepstrum, delta, three
                           in-place CMVN launches, interleave: the stand-alone kernels chained on the stream): torch events around
                           --inner back-to-back calls, the two paths alternating, the minimum of --reps repetitions behind one warm-up each
  fused_ms_threads         the fused path with the workgroup widened (SSP_PLP_FEATURES_THREADS): the default is a lane per frame of the longest
                           utterance in whole waves (128 lanes for 98 frames, 320 for 298)
  bytes_per_frame          what the fused kernel moves through HBM per frame by count: 4 bands in + 4 left_dim in + 4 columns out
  fused_hbm_floor_ms       bytes_per_frame x frames over 8 TB/s
  max_abs_diff             fused against composed rows on the timed arrays

End to end: GMM_UBM.extract_feature(x, y, feature_type='PLP') on --e2e int16 utterances of 3 s in host memory, against the previous
host-glued recipe (plp_batch, api.delta_features per order, np.hstack, api.cmvn_features on numpy arrays), host clock, minimum of 3.
Clock state: ssp_calibrate's copy GB/s and FMA TFLOP/s before and after the runs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def old_extract_plp(x, fs, delta_order):
    """GMM_UBM._extract_plp as it was before the fused tail: four host round trips of the feature matrix"""
    from speech_signal_processing_amd import api
    from speech_signal_processing_amd.sidekit_features import plp_batch
    ctx = api.default_context()
    c, fseg = plp_batch(x, fs=fs)
    blocks = [c]
    for _ in range(delta_order):
        blocks.append(api.delta_features(ctx, blocks[-1], fseg, 2))
    feats = np.asarray(api.cmvn_features(ctx, np.ascontiguousarray(np.hstack(blocks)), fseg), dtype=np.float64)
    return [feats[fseg.offsets[i]:fseg.offsets[i + 1]] for i in range(len(x))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utt3s", type=int, default=100000)
    ap.add_argument("--chunks", type=int, default=300000)
    ap.add_argument("--e2e", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_plp_features.py needs an MI355X (no CPU fallback exists)")
    import speech_signal_processing_amd as pkg
    from speech_signal_processing_amd import GMM_UBM, api

    fs = 16000
    ctx = api.Context.for_torch(0)
    calib = [ctx.calibrate()]
    plan = api.MfccPlan(ctx, pkg.preset_sidekit_plp(fs=fs))
    rows = {}

    def set_env(key, val):
        if val is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = val

    def timed(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            call()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.inner

    for name, n_utt, n_samp in (("%d x 3 s" % args.utt3s, args.utt3s, 3 * fs), ("%d x 1 s" % args.chunks, args.chunks, fs)):
        if n_utt <= 0:
            continue
        g = torch.Generator(device="cuda")
        g.manual_seed(1)
        audio = (0.1 * torch.randn(n_utt * n_samp, generator=g, device="cuda")).float()
        seg = api.Segments.from_lengths(ctx, np.full(n_utt, n_samp, dtype=np.int64))
        fseg = plan.frame_segments(seg)
        logspec = plan.run(audio, seg, fseg)
        del audio
        F, T = int(fseg.total), int(fseg.total // n_utt)
        left26 = torch.randn((F, 26), generator=g, device="cuda")
        for lname, left in (("no left", None), ("left 26", left26)):
            D = (0 if left is None else 26) + 26
            out = torch.empty((F, D), device="cuda")

            def call():
                api.plp_features(ctx, logspec, fseg, fs / 2.0, left=left, delta_order=1, scale=True, out=out)
            variants = {"fused": (None, None), "composed": ("composed", None)}
            for th in (128, 256, 512):
                if th > 64 * -(-T // 64):
                    variants["fused %d lanes" % th] = (None, str(th))
            best = {k: float("inf") for k in variants}
            for k, (path, th) in variants.items():   # warm-up: code objects, scratch buffers
                set_env("SSP_PLP_FEATURES", path)
                set_env("SSP_PLP_FEATURES_THREADS", th)
                call()
            torch.cuda.synchronize()
            for _ in range(args.reps):
                for k, (path, th) in variants.items():
                    set_env("SSP_PLP_FEATURES", path)
                    set_env("SSP_PLP_FEATURES_THREADS", th)
                    best[k] = min(best[k], timed(call))
            set_env("SSP_PLP_FEATURES", "composed")
            set_env("SSP_PLP_FEATURES_THREADS", None)
            call()
            comp = out.clone()
            set_env("SSP_PLP_FEATURES", None)
            call()
            diff = float((out - comp).abs().max().item())
            del comp
            bpf = 4 * (21 + (0 if left is None else 26) + D)
            rows["%s, %s" % (name, lname)] = {
                "utterances": n_utt, "frames_per_utterance": T, "frames": F, "default_lanes": 64 * -(-T // 64),
                "fused_ms": best["fused"], "composed_ms": best["composed"], "composed_over_fused": best["composed"] / best["fused"],
                "fused_ms_threads": {k: v for k, v in best.items() if k.startswith("fused ")},
                "bytes_per_frame": bpf, "fused_hbm_floor_ms": bpf * F / 8e12 * 1e3, "fused_GBs": bpf * F / best["fused"] / 1e6,
                "max_abs_diff": diff}
            del out
        del logspec, left26
        torch.cuda.empty_cache()

    e2e = {}
    if args.e2e > 0:
        rng = np.random.RandomState(0)
        sigs = [(rng.randn(3 * fs) * 3000).astype(np.int16) for _ in range(args.e2e)]
        y = [0] * len(sigs)

        def wall(fn):
            fn()
            best = float("inf")
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                best = min(best, (time.perf_counter() - t0) * 1e3)
            return best
        new_ms = wall(lambda: GMM_UBM.extract_feature(sigs, y, feature_type='PLP'))
        old_ms = wall(lambda: old_extract_plp(sigs, fs, 1))
        new_ms = min(new_ms, wall(lambda: GMM_UBM.extract_feature(sigs, y, feature_type='PLP')))
        old_ms = min(old_ms, wall(lambda: old_extract_plp(sigs, fs, 1)))
        a = GMM_UBM.extract_feature(sigs[:50], y[:50], feature_type='PLP')[0]
        b = old_extract_plp(sigs[:50], fs, 1)
        e2e = {"utterances": len(sigs), "extract_feature_PLP_ms": new_ms, "previous_recipe_ms": old_ms, "previous_over_new": old_ms / new_ms,
               "max_abs_diff": float(max(np.abs(p - q).max() for p, q in zip(a, b)))}
    calib.append(ctx.calibrate())
    print(json.dumps({"metric": "fused PLP tail (ssp_plp_features) against the composed device chain, and extract_feature('PLP') end to end",
                      "config": {"reps": args.reps, "inner": args.inner, "device": torch.cuda.get_device_name(0), "delta_order": 1, "scale": 1},
                      "calibration_before_after": calib, "rows": rows, "end_to_end": e2e}))


if __name__ == "__main__":
    main()
