#!/usr/bin/env python
"""Training throughput of the conv + GRU d-vector network (ssp_gru_trainer_epoch) at the reference's shape, next to the same network
composed from torch ops on the same device in the same process.

    python tools/bench_gru_train.py [--rows 6000] [--T 98] [--D 13] [--batch 128] [--classes 40,1251] [--activations hard_sigmoid,sigmoid]
                                    [--epochs 2] [--warmup 1] [--torch-epochs 1]

Shape: --rows x (98, 13) chunks resident in HBM, Conv2D(64, 5 x 5, strides 2) -> 3 x GRU(1024) -> mean -> Dense(512) -> l2_normalize ->
Dense(n_class) softmax, batch 128, a fresh permutation per epoch, Adam (d_vector.py:213-269).  An epoch is timed on the host clock around
the call, which ends in a device synchronise (the read-back of the per-step sums); `kernel_ms` of the C-ABI (hipEvents around the queued
steps) is given beside it.  --warmup untimed epochs, then the median of --epochs.  Prints one JSON line.

What the line holds, per (n_class, activation):
  epoch_ms, step_ms, kernel_ms
  launch_ms            the launch kinds of ONE step, a hipEvent between each (ssp_gru_trainer_step_times; the median of 5 steps); the 2 x 49
                       step launches of a layer and direction are one figure
  gflop_per_step, tflops   COUNTED multiply-adds x 2 of one step (forward + backward, the conv, the GEMMs and the recurrence; the
                       element-wise work is not counted) and that count over step_ms, beside the 157.3 TFLOP/s fp32 MFMA peak
  torch_epoch_ms       the same network from torch ops with autograd and torch.optim.Adam(eps=1e-7), TF32 off: F.conv2d, one input
                       projection per layer, per step torch.addmm for h U_zr and (r h) U_h, rows gathered with the same permutation, the
                       loss kept on the device (one synchronise per epoch)
and once:
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

PEAK_TFLOPS = 157.3


def keras_init(rng, D, F, H, n_gru, E, C, kernel=(5, 5), strides=(2, 2)):
    def glorot(shape, fan_in, fan_out):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        return rng.uniform(-lim, lim, shape).astype(np.float32)
    kh, kw = kernel
    K = glorot((kh, kw, 1, F), kh * kw, kh * kw * F)
    grus, d_in = [], -(-D // strides[1]) * F
    for _ in range(n_gru):
        W = glorot((d_in, 3 * H), d_in, 3 * H)
        U = np.linalg.svd(rng.standard_normal((H, 3 * H)), full_matrices=False)[2].astype(np.float32)
        grus.append((W, U, np.zeros(3 * H, np.float32)))
        d_in = H
    return (K, np.zeros(F, np.float32), strides), grus, (glorot((H, E), H, E), np.zeros(E, np.float32)), (glorot((E, C), E, C), np.zeros(C, np.float32))


def step_gflop(B, T, D, F, H, n_gru, E, C, kernel=(5, 5), strides=(2, 2)):
    """counted multiply-adds x 2 of one training step -> (forward, backward) GFLOP"""
    To, Do = -(-T // strides[0]), -(-D // strides[1])
    conv = B * To * Do * F * kernel[0] * kernel[1]
    fwd, bwd, d_in = conv, conv, Do * F                    # conv backward: dK only
    for _ in range(n_gru):
        proj, rec = B * To * d_in * 3 * H, B * To * 3 * H * H
        fwd += proj + rec
        bwd += 2 * proj + 2 * rec                          # dW and dx; the step products and dU
        d_in = H
    tail = B * (H * E + E * C)
    return 2e-9 * (fwd + tail), 2e-9 * (bwd + 2 * tail)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--T", type=int, default=98)
    ap.add_argument("--D", type=int, default=13)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--units", type=int, default=1024)
    ap.add_argument("--n-gru", type=int, default=3)
    ap.add_argument("--embedding", type=int, default=512)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--classes", default="40,1251")
    ap.add_argument("--activations", default="hard_sigmoid,sigmoid")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-epochs", type=int, default=1, help="timed epochs of the torch network (0: skip it)")
    args = ap.parse_args()

    import torch
    import torch.nn.functional as Fn
    if not torch.cuda.is_available():
        raise SystemExit("bench_gru_train.py needs an MI355X (no CPU fallback exists)")
    from speech_signal_processing_amd import api
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False

    N, T, D, F, H, L, E, B = args.rows, args.T, args.D, args.filters, args.units, args.n_gru, args.embedding, args.batch
    device = torch.device("cuda", 0)
    ctx = api.Context.for_torch(0)
    calibration = ctx.calibrate()
    gen = torch.Generator(device=device)
    gen.manual_seed(1234)
    X = torch.randn((N, T, D), dtype=torch.float32, device=device, generator=gen)
    steps = (N + B - 1) // B
    rows = {}
    for C in (int(c) for c in args.classes.split(",")):
        y = torch.randint(0, C, (N,), device=device, generator=gen).to(torch.int32)
        conv, grus, dense, head = keras_init(np.random.default_rng(0), D, F, H, L, E, C)
        gf, gb = step_gflop(B, T, D, F, H, L, E, C)
        for act in args.activations.split(","):
            net = api.GruTrainer(ctx, conv, grus, dense, head, T=T, D=D, recurrent_activation=act, reset_after=False, max_batch=B)
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
            parts = [net.step_times(X, y, batch_size=B, lr=1e-4) for _ in range(5)]
            launch_ms = {k: float(np.median([p[k] for p in parts])) for k in parts[0]}
            # (the last step of an epoch is the tail batch: the figure per step is over the rows, in full batches)
            step_ms = ms / (N / B)
            rows["n_class=%d %s" % (C, act)] = {
                "epoch_ms": ms, "epoch_ms_min_max": [float(min(r[0] for r in runs)), float(max(r[0] for r in runs))],
                "kernel_ms": float(np.median([r[1] for r in runs])), "steps_per_epoch": steps, "step_ms": step_ms,
                "launch_ms": launch_ms, "launch_ms_sum": float(sum(launch_ms.values())), "mean_loss_by_epoch": [r[2] for r in runs],
                "gflop_per_step": {"forward": gf, "backward": gb}, "tflops": (gf + gb) / step_ms, "share_of_fp32_mfma_peak": (gf + gb) / step_ms / PEAK_TFLOPS}
            net.close()
        if args.torch_epochs > 0:
            K, _, strides = conv
            params = {"K": torch.from_numpy(np.ascontiguousarray(K.transpose(3, 2, 0, 1))), "bc": torch.zeros(F)}
            for i, (W, U, b) in enumerate(grus):
                params["W%d" % i], params["U%d" % i], params["b%d" % i] = torch.from_numpy(W), torch.from_numpy(U), torch.from_numpy(b)
            params["Wd"], params["bd"] = torch.from_numpy(dense[0]), torch.zeros(E)
            params["Wh"], params["bh"] = torch.from_numpy(head[0]), torch.zeros(C)
            params = {k: v.to(device).requires_grad_(True) for k, v in params.items()}
            opt = torch.optim.Adam(list(params.values()), lr=1e-4, eps=1e-7)
            kh, kw = K.shape[:2]
            To, Do = -(-T // strides[0]), -(-D // strides[1])
            ph, pw = max((To - 1) * strides[0] + kh - T, 0), max((Do - 1) * strides[1] + kw - D, 0)
            pad = (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2)
            y64 = y.long()
            trng = np.random.default_rng(1)

            def forward(xb):
                h = Fn.conv2d(Fn.pad(xb[:, None], pad), params["K"], params["bc"], stride=strides).permute(0, 2, 3, 1).reshape(xb.shape[0], To, Do * F)
                for i in range(L):
                    W, U, b = params["W%d" % i], params["U%d" % i], params["b%d" % i]
                    P = torch.addmm(b, h.reshape(-1, h.shape[2]), W).reshape(xb.shape[0], To, 3 * H)
                    st = torch.zeros((xb.shape[0], H), device=device)
                    outs = []
                    for t in range(To):
                        zr = torch.sigmoid(torch.addmm(P[:, t, :2 * H], st, U[:, :2 * H]))   # (sigmoid gates: the figure stands beside both)
                        z, r = zr[:, :H], zr[:, H:]
                        hh = torch.tanh(torch.addmm(P[:, t, 2 * H:], r * st, U[:, 2 * H:]))
                        st = z * st + (1 - z) * hh
                        outs.append(st)
                    h = torch.stack(outs, dim=1)
                e = torch.addmm(params["bd"], h.mean(dim=1), params["Wd"])
                yv = e / torch.sqrt(torch.clamp((e * e).sum(dim=1, keepdim=True), min=1e-12))
                return torch.addmm(params["bh"], yv, params["Wh"])

            def torch_epoch():
                order = torch.from_numpy(trng.permutation(N)).to(device)
                total = torch.zeros((), device=device)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for r0 in range(0, N, B):
                    idx = order[r0:r0 + B]
                    loss = Fn.cross_entropy(forward(X[idx]), y64[idx]) + 0.01 * (params["K"] * params["K"]).sum()
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
                row["torch_step_ms"] = tms / (N / B)
                row["torch_epoch_ms_min_max"] = [float(min(r[0] for r in truns)), float(max(r[0] for r in truns))]
                row["torch_mean_loss_by_epoch"] = [r[1] for r in truns]
                row["library_over_torch_time"] = row["epoch_ms"] / tms
            del params, opt
    line = {"metric": "conv + GRU d-vector network training, ms per epoch (forward with stash, softmax cross-entropy + l2, backward through time, Adam; exact-fp32 MFMA)",
            "config": {"workload": "%d x (%d, %d) chunks resident in HBM, batch %d, conv %d + %d x GRU(%d) + Dense(%d) + softmax" % (N, T, D, B, F, L, H, E),
                       "epochs": args.epochs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)},
            "calibration": calibration, **rows}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
