#!/usr/bin/env python
"""The VAD threshold sweep (ssp_vad_sweep) next to the loop it replaces, measured in the same process on the same device arrays.

    python tools/bench_vad_sweep.py [--steps 10] [--warmup 2] [--sample 256]

Shapes: ONE 60 s recording and a batch of 32 x 30 s synthetic 16 kHz recordings (bench.py's generator, each turned down for a third of
its length so that there is silence to find), features resident in HBM; labels = the detector's own mask at the reference's default
thresholds; grids of 16^3 and 32^3 threshold triples over the reference's box (VAD.py:197-201).

What the JSON line holds, per shape and grid:
  sweep_kernel_ms / sweep_wall_ms   the single ssp_vad_sweep call: hipEvent kernel milliseconds (median of --steps behind --warmup) and the
                                    whole device-pointer call on the host's clock (threshold upload and its host wait included)
  loop_wall_ms_sampled              the loop the call replaces — one ssp_vad_detect per triple, the counts of its mask by torch on the
                                    device, one read-back at the end — on a --sample of the triples (evenly spread over the grid)
  loop_wall_ms_scaled               that time times n_par / sample: SCALED, not measured, for the whole grid
  ratio                             loop_wall_ms_scaled / sweep_wall_ms
  counts_equal                      the sweep's counts at the sampled triples equal the loop's
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=256)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_vad_sweep.py needs an MI355X (no CPU fallback exists)")
    from speech_signal_processing_amd import VAD, api
    from bench import synth_audio_device

    fs = 16000
    device = torch.device("cuda", 0)
    ctx = api.Context.for_torch(0)
    rows = {}
    for name, n_utt, seconds in (("1x60s", 1, 60.0), ("32x30s", 32, 30.0)):
        n_samp = int(round(seconds * fs))
        audio = synth_audio_device(torch, n_utt, n_samp, fs, seed=1234, device=device)
        for u in range(n_utt):   # a quiet third, somewhere else in every recording
            at = (u * 7919) % (2 * n_samp // 3)
            audio[u, at:at + n_samp // 3] *= 1.0 / 128
        seg = api.Segments.from_lengths(ctx, np.full(n_utt, n_samp, dtype=np.int64))
        zcr, power, _, fseg = api.vad_features(ctx, audio.view(-1), seg)
        lab, _ = api.vad_detect(ctx, zcr, power, fseg, 0)
        y = lab.bool()
        for grid in (16, 32):
            axes = [np.linspace(lo, hi, grid).astype(np.float32) for lo, hi in (VAD.BOUNDS[k] for k in ("zcr_gate", "ampl", "amph"))]
            g, lo, hi = (m.reshape(-1) for m in np.meshgrid(*axes, indexing="ij"))
            n_par = g.shape[0]

            def sweep_ms():
                return api.vad_sweep(ctx, zcr, power, lab, fseg, g, lo, hi, timing=True)[1]

            def sweep_wall():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                api.vad_sweep(ctx, zcr, power, lab, fseg, g, lo, hi)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            for _ in range(args.warmup):
                sweep_ms()
            k_ms = float(np.median([sweep_ms() for _ in range(args.steps)]))
            w_ms = float(np.median([sweep_wall() for _ in range(args.steps)]))
            counts = api.vad_sweep(ctx, zcr, power, lab, fseg, g, lo, hi).sum(dim=1).cpu().numpy()

            pick = np.unique(np.linspace(0, n_par - 1, min(args.sample, n_par)).astype(np.int64))

            def loop():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = torch.empty((pick.shape[0], 3), dtype=torch.int64, device=device)
                for r, j in enumerate(pick):
                    mask, _ = api.vad_detect(ctx, zcr, power, fseg, 0, float(g[j]), float(lo[j]), float(hi[j]), 16)
                    m = mask.bool()
                    out[r, 0], out[r, 1], out[r, 2] = (m & y).sum(), (m & ~y).sum(), (~m & y).sum()
                res = out.cpu().numpy()
                return (time.perf_counter() - t0) * 1e3, res
            loop()
            times, res = zip(*[loop() for _ in range(max(3, args.steps // 3))])
            l_ms = float(np.median(times))
            scaled = l_ms * n_par / pick.shape[0]
            rows["%s grid %d^3" % (name, grid)] = {
                "utterances": n_utt, "frames": int(fseg.total), "n_par": int(n_par), "sweep_kernel_ms": k_ms, "sweep_wall_ms": w_ms,
                "loop_sample": int(pick.shape[0]), "loop_wall_ms_sampled": l_ms, "loop_wall_ms_scaled": scaled, "ratio": scaled / w_ms,
                "counts_equal": bool(np.array_equal(res[0], counts[pick])), "distinct_outcomes": len({tuple(c) for c in counts.tolist()}),
                "speech_share_of_labels": float(y.float().mean().item())}
    print(json.dumps({"metric": "VAD threshold sweep: one ssp_vad_sweep call against one ssp_vad_detect per triple plus counting (scaled from a sample)",
                      "config": {"steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}, "rows": rows}))


if __name__ == "__main__":
    main()
