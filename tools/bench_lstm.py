#!/usr/bin/env python
"""Throughput of the LSTM d-vector forward pass (ssp_lstm_forward) at the reference's shape, next to per-step torch.matmul on the same
device in the same process.

    python tools/bench_lstm.py [--chunks 300000] [--T 98] [--D 13] [--H 128] [--steps 10] [--warmup 2] [--torch-steps 3]

Shape: --chunks 1-second chunks x (98, 13) MFCC frames resident in HBM -> 128-d embeddings (d_vector.py:271-294), both recurrent
activations.  Times are hipEvent kernel milliseconds (`kernel_ms` of the C-ABI), median of --steps launches behind --warmup untimed ones.
Prints one JSON line.

What the line holds, per activation:
  kernel_ms, embeddings_per_s
  algorithmic_tflops   2 (D + H) 4H T FLOP per sequence (14.15 MFLOP at the reference shape) over the time
  frac_of_fp32_mfma_peak   that over 157.3 TFLOP/s (the fp32-input MFMA peak); issued_frac counts the zero padding of D to 16 too
  torch_matmul_ms      for context only: the same batch as T steps of x_t @ W + h @ U and element-wise gates in torch (hipEvents)
  max_abs_diff_vs_torch    the two results on the same data (float32 both; no assertion)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP32_MFMA_PEAK_TFLOPS = 157.3


def keras_init(rng, D, H):
    """Keras' initialisation of an LSTM layer: Glorot-uniform kernel, one orthogonal block per gate, forget bias one"""
    lim = np.sqrt(6.0 / (D + 4 * H))
    W = rng.uniform(-lim, lim, (D, 4 * H)).astype(np.float32)
    U = np.concatenate([np.linalg.qr(rng.standard_normal((H, H)))[0] for _ in range(4)], axis=1).astype(np.float32)
    b = np.zeros(4 * H, np.float32)
    b[H:2 * H] = 1.0
    return W, U, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=300000)
    ap.add_argument("--T", type=int, default=98)
    ap.add_argument("--D", type=int, default=13)
    ap.add_argument("--H", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-steps", type=int, default=3, help="timed runs of the torch.matmul context row (0: skip it)")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lstm.py needs an MI355X (no CPU fallback exists)")
    from speech_signal_processing_amd import api

    N, T, D, H = args.chunks, args.T, args.D, args.H
    device = torch.device("cuda", 0)
    ctx = api.Context.for_torch(0)
    gen = torch.Generator(device=device)
    gen.manual_seed(1234)
    X = 3.0 * torch.randn((N, T, D), dtype=torch.float32, device=device, generator=gen)
    feats = X.view(N * T, D)
    fseg = api.Segments.from_lengths(ctx, np.full(N, T, dtype=np.int64))
    W, U, b = keras_init(np.random.default_rng(0), D, H)
    Wd, Ud, bd = (torch.from_numpy(v).to(device) for v in (W, U, b))

    def median_ms(fn, warmup, steps):
        for _ in range(warmup):
            fn()
        ms = [fn() for _ in range(steps)]
        return float(np.median(ms)), [float(min(ms)), float(max(ms))]

    def torch_forward(act):
        h = torch.zeros((N, H), dtype=torch.float32, device=device)
        c = torch.zeros_like(h)
        for t in range(T):
            z = torch.addmm(bd, X[:, t], Wd).addmm_(h, Ud)
            if act == "sigmoid":
                i, f, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.sigmoid(z[:, 3 * H:])
            else:
                i, f, o = (torch.clamp(0.2 * z[:, a:a + H] + 0.5, 0.0, 1.0) for a in (0, H, 3 * H))
            c = f * c + i * torch.tanh(z[:, 2 * H:3 * H])
            h = o * torch.tanh(c)
        return h

    def torch_ms(act):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch_forward(act)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    flop_alg = 2.0 * (D + H) * 4 * H * T * N
    flop_issued = 2.0 * (16 * ((D + 15) // 16) + H) * 4 * H * T * N
    rows = {}
    for act in ("hard_sigmoid", "sigmoid"):
        net = api.LstmForward(ctx, W, U, b, act)
        out = net.forward(feats, fseg)
        torch.cuda.synchronize()
        ms, rng = median_ms(lambda: net.forward(feats, fseg, timing=True)[1], args.warmup, args.steps)
        row = {"kernel_ms": ms, "kernel_ms_min_max": rng, "embeddings_per_s": N / (ms * 1e-3),
               "algorithmic_tflops": flop_alg / (ms * 1e-3) / 1e12,
               "frac_of_fp32_mfma_peak": flop_alg / (ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
               "issued_frac_of_fp32_mfma_peak": flop_issued / (ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
               "floor_ms_at_peak": flop_alg / (FP32_MFMA_PEAK_TFLOPS * 1e12) * 1e3}
        if args.torch_steps > 0:
            tms, trng = median_ms(lambda: torch_ms(act), 1, args.torch_steps)
            row["torch_matmul_ms"] = tms
            row["torch_matmul_ms_min_max"] = trng
            row["speedup_over_torch_matmul"] = tms / ms
            row["max_abs_diff_vs_torch"] = float((torch_forward(act) - out).abs().max().item())
        rows[act] = row
        del net, out
    line = {"metric": "LSTM d-vector embeddings/s (last hidden state of one LSTM layer, exact-fp32 MFMA)",
            "config": {"workload": "%d chunks x (%d, %d) -> %d resident in HBM" % (N, T, D, H), "steps": args.steps, "warmup": args.warmup,
                       "mflop_per_sequence": flop_alg / N / 1e6, "device": torch.cuda.get_device_name(0)},
            **rows}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
