#!/usr/bin/env python
"""Training throughput of the dense d-vector network (ssp_dnn_trainer_epoch) at the reference's shape, next to the same network built
from torch on the same device in the same process.

    python tools/bench_dnn_train.py [--rows 60000] [--d-in 1274] [--batch 128] [--classes 40,1251] [--epochs 5] [--warmup 1] [--torch-epochs 3]

Shape: --rows x 1274 feature rows resident in HBM, Dense(256) x 4 + Dense(n_class), dropout 0 / 0 / 0.5 / 0.5, batch 128, a fresh
permutation per epoch, Adam (d_vector.py:168-206).  An epoch is timed on the host clock around the call, which ends in a device
synchronise (the read-back of the per-step sums); `kernel_ms` of the C-ABI (hipEvents around the queued steps) is given beside it.
--warmup untimed epochs, then the median of --epochs.  Prints one JSON line.

What the line holds, per n_class:
  epoch_ms, steps_per_s, kernel_ms
  gflop_per_step       2 B sum(d_in units) forward, the same for dW, the same less the first layer for dX
  frac_of_fp32_mfma_peak   counted flop over epoch_ms over 157.3 TFLOP/s (a whole-epoch rate, launches and gaps included)
  torch_epoch_ms       Linear / relu / dropout / cross_entropy, autograd, torch.optim.Adam(eps=1e-7), TF32 off, rows gathered with the
                       same permutation, the loss kept on the device (one synchronise per epoch)
  calibration          ssp_calibrate's copy GB/s and FMA TFLOP/s of the box, before the runs (its clock, indirectly)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP32_MFMA_PEAK_TFLOPS = 157.3
RATES = (0.0, 0.0, 0.5, 0.5, 0.0)


def glorot(rng, dims):
    out = []
    for d_in, units in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (d_in + units))
        out.append((rng.uniform(-lim, lim, (d_in, units)).astype(np.float32), np.zeros(units, np.float32)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--d-in", type=int, default=1274)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--classes", default="40,1251")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-epochs", type=int, default=3, help="timed epochs of the torch network (0: skip it)")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dnn_train.py needs an MI355X (no CPU fallback exists)")
    from speech_signal_processing_amd import api
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False

    N, d0, B = args.rows, args.d_in, args.batch
    device = torch.device("cuda", 0)
    ctx = api.Context.for_torch(0)
    calibration = ctx.calibrate()
    gen = torch.Generator(device=device)
    gen.manual_seed(1234)
    X = torch.randn((N, d0), dtype=torch.float32, device=device, generator=gen)
    steps = (N + B - 1) // B
    rows = {}
    for C in (int(c) for c in args.classes.split(",")):
        dims = [d0, 256, 256, 256, 256, C]
        y = torch.randint(0, C, (N,), device=device, generator=gen).to(torch.int32)
        init = glorot(np.random.default_rng(0), dims)
        L = len(init)
        net = api.DnnTrainer(ctx, [(W, b, l < L - 1, RATES[l]) for l, (W, b) in enumerate(init)], max_batch=B)
        rng = np.random.default_rng(1)

        def epoch():
            order = rng.permutation(N)
            t0 = time.perf_counter()
            loss, corr, kms = net.epoch(X, y, order, batch_size=B, lr=1e-4, seed=0, timing=True)   # (returns after the read-back)
            return (time.perf_counter() - t0) * 1e3, kms, loss / N

        for _ in range(args.warmup):
            epoch()
        runs = [epoch() for _ in range(args.epochs)]
        ms = float(np.median([r[0] for r in runs]))
        mac = sum(a * b for a, b in zip(dims[:-1], dims[1:]))
        flop_step = 2.0 * B * (3 * mac - dims[0] * dims[1])
        row = {"epoch_ms": ms, "epoch_ms_min_max": [float(min(r[0] for r in runs)), float(max(r[0] for r in runs))],
               "kernel_ms": float(np.median([r[1] for r in runs])), "steps_per_epoch": steps, "steps_per_s": steps / (ms * 1e-3),
               "launches_per_step": 2 * L + (L - 1) + 2, "gflop_per_step": flop_step / 1e9,
               "algorithmic_tflops": flop_step * steps / (ms * 1e-3) / 1e12,
               "frac_of_fp32_mfma_peak": flop_step * steps / (ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
               "mean_loss_by_epoch": [r[2] for r in runs]}
        if args.torch_epochs > 0:
            lin = [torch.nn.Linear(a, b, device=device) for a, b in zip(dims[:-1], dims[1:])]
            with torch.no_grad():
                for m, (W, b) in zip(lin, init):
                    m.weight.copy_(torch.from_numpy(W.T))
                    m.bias.zero_()
            params = [p for m in lin for p in m.parameters()]
            opt = torch.optim.Adam(params, lr=1e-4, eps=1e-7)
            y64 = y.long()
            trng = np.random.default_rng(1)

            def torch_epoch():
                order = torch.from_numpy(trng.permutation(N)).to(device)
                total = torch.zeros((), device=device)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for r0 in range(0, N, B):
                    idx = order[r0:r0 + B]
                    h = X[idx]
                    for l, m in enumerate(lin):
                        h = m(h)
                        if l < L - 1:
                            h = torch.relu(h)
                        if RATES[l] > 0:
                            h = torch.nn.functional.dropout(h, RATES[l], training=True)
                    loss = torch.nn.functional.cross_entropy(h, y64[idx])
                    opt.zero_grad(set_to_none=True)
                    loss.backward()
                    opt.step()
                    total += loss.detach() * idx.shape[0]
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, float(total.item()) / N

            torch_epoch()
            truns = [torch_epoch() for _ in range(args.torch_epochs)]
            tms = float(np.median([r[0] for r in truns]))
            row["torch_epoch_ms"] = tms
            row["torch_epoch_ms_min_max"] = [float(min(r[0] for r in truns)), float(max(r[0] for r in truns))]
            row["torch_mean_loss_by_epoch"] = [r[1] for r in truns]
            row["library_over_torch_time"] = ms / tms
        rows["n_class=%d" % C] = row
        net.close()
    line = {"metric": "dense d-vector network training, ms per epoch (forward with dropout, softmax cross-entropy, backward, Adam; exact-fp32 MFMA)",
            "config": {"workload": "%d x %d rows resident in HBM, batch %d, Dense(256) x 4 + softmax" % (N, d0, B), "epochs": args.epochs,
                       "warmup": args.warmup, "device": torch.cuda.get_device_name(0)},
            "calibration": calibration, **rows}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
