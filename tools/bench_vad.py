#!/usr/bin/env python
"""Throughput of the voice activity detection kernels, next to the headline MFCC pass measured in the same process on the same box.

    python tools/bench_vad.py [--utts 100000] [--seconds 3] [--steps 20] [--warmup 3]

Shape: BASELINE.json configs[1]'s batch — 100 000 x 3 s synthetic 16 kHz utterances resident in HBM (375 VAD frames per utterance) — as
float32 and as int16; the detector on the result; remove_silence on 2 000 host utterances.  Times are hipEvent kernel milliseconds
(`kernel_ms` of the C-ABI), median of --steps launches behind --warmup untimed ones.  Prints one JSON line.

What the line holds:
  vad_f32 / vad_i16   frames/s, kernel_ms, fraction of the HBM bound (algorithmic bytes = every sample once + 12 B per frame, over 8 TB/s)
  mfcc_headline       the fused 39-d MFCC pass (bench.py's headline workload) on the same samples: frames/s, kernel_ms
  ratio_to_headline   vad_f32 frames/s over the headline's frames/s (required >= 0.85: `meets_0_85`)
  detect              VAD_detection / VAD_frequency kernel_ms and their share of the feature kernel's
  wall_ms_per_call    (vad_f32) the whole device-pointer call on the host's clock, host-side chunk table and its upload included
  remove_silence      wall seconds for 2 000 host utterances (copy in, both kernels, mask back, numpy slicing)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=100000)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-utts", type=int, default=2000, help="utterances of the remove_silence row (0: skip it)")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_vad.py needs an MI355X (no CPU fallback exists)")
    import speech_signal_processing_amd as pkg
    from speech_signal_processing_amd import VAD, api
    from bench import synth_audio_device

    fs = 16000
    n_samp, n_utt = int(round(args.seconds * fs)), args.utts
    device = torch.device("cuda", 0)
    ctx = api.Context.for_torch(0)
    audio = synth_audio_device(torch, n_utt, n_samp, fs, seed=1234, device=device)
    flat = audio.view(-1)
    seg = api.Segments.from_lengths(ctx, np.full(n_utt, n_samp, dtype=np.int64))

    def median_ms(fn):
        for _ in range(args.warmup):
            fn()
        ms = [fn() for _ in range(args.steps)]
        return float(np.median(ms)), [float(min(ms)), float(max(ms))]

    # ---- the headline MFCC pass on the same samples (set-up call first: chunk table, first touch of the output)
    plan = api.MfccPlan(ctx, pkg.preset_sidekit(fs=fs, delta_order=2, cmvn=0))
    mseg = plan.frame_segments(seg)
    feats = torch.empty((mseg.total, plan.d_out), dtype=torch.float32, device=device)
    plan.run(flat, seg, mseg, out=feats)
    torch.cuda.synchronize()
    mfcc_ms, mfcc_rng = median_ms(lambda: plan.run(flat, seg, mseg, out=feats, timing=True)[1])
    mfcc_fps = mseg.total / (mfcc_ms * 1e-3)
    del feats

    # ---- VAD features, float32 and int16
    fseg = api.vad_frame_segments(ctx, seg)
    rows = {}
    keep = None
    for name, x in (("vad_f32", flat), ("vad_i16", None)):
        if x is None:
            x = (flat * 32767.0).round_().to(torch.int16)
        api.vad_features(ctx, x, seg, fseg)
        torch.cuda.synchronize()
        last = {}

        def run(x=x, last=last):
            out = api.vad_features(ctx, x, seg, fseg, timing=True)
            last["out"] = out
            return out[4]
        ms, rng = median_ms(run)
        algo = n_utt * n_samp * x.element_size() + fseg.total * 12
        rows[name] = {"frames_per_s": fseg.total / (ms * 1e-3), "kernel_ms": ms, "kernel_ms_min_max": rng, "frames": int(fseg.total),
                      "algorithmic_bytes": int(algo), "achieved_gbs": algo / (ms * 1e-3) / 1e9,
                      "hbm_bound_ms": algo / (HBM_PEAK_GBS * 1e9) * 1e3, "frac_of_hbm_bound": algo / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
        if name == "vad_f32":
            keep = last["out"]
            ms0, _ = median_ms(lambda: api.vad_features(ctx, x, seg, fseg, normalize=False, timing=True)[4])
            rows[name]["kernel_ms_without_peak_pass"] = ms0

            def wall(x=x):   # the whole call as a caller sees it: chunk table built and uploaded (one host wait), kernels, final wait
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                api.vad_features(ctx, x, seg, fseg)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            rows[name]["wall_ms_per_call"] = median_ms(wall)[0]
        del x
    zcr, power, ent = keep[0], keep[1], keep[2]

    # ---- the detectors on the float32 result
    det_ms, _ = median_ms(lambda: api.vad_detect(ctx, zcr, power, fseg, 0, timing=True)[2])
    frq_ms, _ = median_ms(lambda: api.vad_detect(ctx, None, ent, fseg, 1, ampl=0.4, timing=True)[2])
    mask, count = api.vad_detect(ctx, zcr, power, fseg, 0)
    speech_share = float(count.sum().item()) / fseg.total

    # ---- remove_silence on host utterances
    host = [(audio[i] * 32767.0).round().to(torch.int16).cpu().numpy() for i in range(min(args.host_utts, n_utt))]
    # (the synthetic utterances are voiced throughout: one second is turned down so that there is silence to remove.  It starts in a trough
    #  of the 3 Hz envelope, where the run before it has been flushed: a short run cut off by the silence would stay open and take the gap in)
    lo, hi = min(n_samp, int(round(0.9167 * fs))), min(n_samp, int(round(1.9167 * fs)))
    for x in host:
        x[lo:hi] //= 128
    rs = None
    if host:
        VAD.remove_silence(host[:8])
        t0 = time.perf_counter()
        out = VAD.remove_silence(host)
        rs_s = time.perf_counter() - t0
        rs = {"utterances": len(host), "wall_s": rs_s, "utterances_per_s": len(host) / rs_s,
              "samples_kept_share": float(sum(y.shape[0] for y in out)) / float(sum(x.shape[0] for x in host))}

    ratio = rows["vad_f32"]["frames_per_s"] / mfcc_fps
    line = {"metric": "VAD frames/s (features of 256-sample frames every 128, per-utterance peak normalisation included)",
            "config": {"workload": "configs[1] batch: %d x %.0f s synthetic 16 kHz utterances resident in HBM" % (n_utt, args.seconds),
                       "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)},
            **rows,
            "mfcc_headline": {"frames_per_s": mfcc_fps, "kernel_ms": mfcc_ms, "kernel_ms_min_max": mfcc_rng, "frames": int(mseg.total)},
            "ratio_to_headline": ratio, "meets_0_85": bool(ratio >= 0.85),
            "detect": {"time_kernel_ms": det_ms, "frequency_kernel_ms": frq_ms, "share_of_feature_kernel": det_ms / rows["vad_f32"]["kernel_ms"],
                       "speech_frame_share": speech_share},
            "remove_silence": rs}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
