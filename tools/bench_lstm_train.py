#!/usr/bin/env python
"""Training throughput of the recurrent d-vector network (ssp_lstm_trainer_epoch) at the reference's shape, next to the same network built
from torch on the same device in the same process, and next to the inference kernel on one batch.

    python tools/bench_lstm_train.py [--rows 60000] [--T 98] [--d-in 13] [--batch 128] [--classes 40,1251] [--activations hard_sigmoid,sigmoid]
                                     [--epochs 3] [--warmup 1] [--torch-epochs 2]

Shape: --rows x (98, 13) chunks resident in HBM, LSTM(128) + Dense(n_class) softmax, batch 128, a fresh permutation per epoch, Adam
(d_vector.py:271-294).  An epoch is timed on the host clock around the call, which ends in a device synchronise (the read-back of the
per-step sums); `kernel_ms` of the C-ABI (hipEvents around the queued steps) is given beside it.  --warmup untimed epochs, then the median
of --epochs.  Prints one JSON line.

What the line holds, per (n_class, activation):
  epoch_ms, step_ms, kernel_ms
  launch_ms            the nine launches of ONE step, a hipEvent between each (ssp_lstm_trainer_step_times; the median of 20 steps): events
                       between back-to-back launches add their own few microseconds, so the parts sum to a little more than step_ms
  torch_epoch_ms       nn.LSTM(batch_first) + Linear, cross_entropy, autograd, torch.optim.Adam(eps=1e-7), TF32 off, rows gathered with the
                       same permutation, the loss kept on the device (one synchronise per epoch).  torch's LSTM has sigmoid gates only:
                       the figure stands beside both activations
and once:
  forward_batch_ms     ssp_lstm_forward (lstm.hip: one wave = 16 sequences x all hidden tiles, weights streamed per step) on one batch of
                       128 chunks, kernel milliseconds, median of 20 — the decomposition the trainer does not reuse — beside
                       train_forward_ms, the trainer's own forward launch from launch_ms
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


def keras_init(rng, d_in, units, n_class):
    lim = np.sqrt(6.0 / (d_in + 4 * units))
    W = rng.uniform(-lim, lim, (d_in, 4 * units)).astype(np.float32)
    U = np.linalg.svd(rng.standard_normal((units, 4 * units)), full_matrices=False)[2].astype(np.float32)
    b = np.zeros(4 * units, np.float32)
    b[units:2 * units] = 1.0
    lim = np.sqrt(6.0 / (units + n_class))
    return W, U, b, rng.uniform(-lim, lim, (units, n_class)).astype(np.float32), np.zeros(n_class, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--T", type=int, default=98)
    ap.add_argument("--d-in", type=int, default=13)
    ap.add_argument("--units", type=int, default=128)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--classes", default="40,1251")
    ap.add_argument("--activations", default="hard_sigmoid,sigmoid")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-epochs", type=int, default=2, help="timed epochs of the torch network (0: skip it)")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lstm_train.py needs an MI355X (no CPU fallback exists)")
    from speech_signal_processing_amd import api
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False

    N, T, D, H, B = args.rows, args.T, args.d_in, args.units, args.batch
    device = torch.device("cuda", 0)
    ctx = api.Context.for_torch(0)
    calibration = ctx.calibrate()
    gen = torch.Generator(device=device)
    gen.manual_seed(1234)
    X = torch.randn((N, T, D), dtype=torch.float32, device=device, generator=gen)
    steps = (N + B - 1) // B
    rows = {}
    fwd_train = []
    for C in (int(c) for c in args.classes.split(",")):
        y = torch.randint(0, C, (N,), device=device, generator=gen).to(torch.int32)
        init = keras_init(np.random.default_rng(0), D, H, C)
        for act in args.activations.split(","):
            net = api.LstmTrainer(ctx, *init, T=T, recurrent_activation=act, max_batch=B)
            rng = np.random.default_rng(1)

            def epoch():
                order = rng.permutation(N)
                t0 = time.perf_counter()
                loss, corr, kms = net.epoch(X, y, order, batch_size=B, lr=1e-4, timing=True)   # (returns after the read-back)
                return (time.perf_counter() - t0) * 1e3, kms, loss / N

            for _ in range(args.warmup):
                epoch()
            runs = [epoch() for _ in range(args.epochs)]
            ms = float(np.median([r[0] for r in runs]))
            parts = [net.step_times(X, y, batch_size=B, lr=1e-4) for _ in range(20)]
            launch_ms = {k: float(np.median([p[k] for p in parts])) for k in parts[0]}
            fwd_train.append(launch_ms["forward+stash"])
            rows["n_class=%d %s" % (C, act)] = {
                "epoch_ms": ms, "epoch_ms_min_max": [float(min(r[0] for r in runs)), float(max(r[0] for r in runs))],
                "kernel_ms": float(np.median([r[1] for r in runs])), "steps_per_epoch": steps, "step_ms": ms / steps,
                "launch_ms": launch_ms, "launch_ms_sum": float(sum(launch_ms.values())), "mean_loss_by_epoch": [r[2] for r in runs]}
            net.close()
        if args.torch_epochs > 0:
            W, U, b, Wd, bd = init
            lstm = torch.nn.LSTM(D, H, batch_first=True, device=device)
            lin = torch.nn.Linear(H, C, device=device)
            with torch.no_grad():   # torch's gate order is i | f | g | o as well; its two bias vectors add up
                lstm.weight_ih_l0.copy_(torch.from_numpy(W.T))
                lstm.weight_hh_l0.copy_(torch.from_numpy(U.T))
                lstm.bias_ih_l0.copy_(torch.from_numpy(b))
                lstm.bias_hh_l0.zero_()
                lin.weight.copy_(torch.from_numpy(Wd.T))
                lin.bias.zero_()
            opt = torch.optim.Adam(list(lstm.parameters()) + list(lin.parameters()), lr=1e-4, eps=1e-7)
            y64 = y.long()
            trng = np.random.default_rng(1)

            def torch_epoch():
                order = torch.from_numpy(trng.permutation(N)).to(device)
                total = torch.zeros((), device=device)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for r0 in range(0, N, B):
                    idx = order[r0:r0 + B]
                    out, _ = lstm(X[idx])
                    loss = torch.nn.functional.cross_entropy(lin(out[:, -1]), y64[idx])
                    opt.zero_grad(set_to_none=True)
                    loss.backward()
                    opt.step()
                    total += loss.detach() * idx.shape[0]
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, float(total.item()) / N

            torch_epoch()
            truns = [torch_epoch() for _ in range(args.torch_epochs)]
            tms = float(np.median([r[0] for r in truns]))
            for act in args.activations.split(","):
                row = rows["n_class=%d %s" % (C, act)]
                row["torch_epoch_ms"] = tms
                row["torch_step_ms"] = tms / steps
                row["torch_epoch_ms_min_max"] = [float(min(r[0] for r in truns)), float(max(r[0] for r in truns))]
                row["torch_mean_loss_by_epoch"] = [r[1] for r in truns]
                row["library_over_torch_time"] = row["epoch_ms"] / tms
    # the inference kernel on one batch: the decomposition the trainer does not reuse
    W, U, b, _, _ = keras_init(np.random.default_rng(0), D, H, 2)
    fwd = api.LstmForward(ctx, W, U, b, "sigmoid")
    xb = X[:B].contiguous()
    fwd.forward(xb, timing=True)
    forward_batch_ms = float(np.median([fwd.forward(xb, timing=True)[1] for _ in range(20)]))
    line = {"metric": "recurrent d-vector network training, ms per epoch (forward with stash, softmax cross-entropy, backward through time, Adam; exact-fp32 MFMA)",
            "config": {"workload": "%d x (%d, %d) chunks resident in HBM, batch %d, LSTM(%d) + softmax" % (N, T, D, B, H), "epochs": args.epochs,
                       "warmup": args.warmup, "device": torch.cuda.get_device_name(0)},
            "calibration": calibration, "forward_batch_ms": forward_batch_ms, "train_forward_ms": float(np.median(fwd_train)), **rows}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
