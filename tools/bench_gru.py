#!/usr/bin/env python
"""Throughput of the conv + GRU d-vector forward pass (d_vector.ConvGruNet) at the reference's shape, next to the same network composed
from torch on the same device in the same process.

    python tools/bench_gru.py [--chunks 20000] [--steps 5] [--warmup 1] [--torch-steps 2] [--workspace-gib 4] [--variants all]

Shape: --chunks 1-second chunks x (98, 13) MFCC frames resident in HBM -> Conv2D(64, 5x5, stride 2, same) -> 3 x GRU(1024) -> mean over
time -> Dense(512) -> L2 normalisation (d_vector.py:213-269), all four (recurrent_activation, reset_after) variants.  A pass is timed
with HIP events on the stream around the whole predict() call (median of --steps behind --warmup untimed ones); the split comes from one
further pass that reads the C-ABI's kernel_ms stage by stage (it synchronises after every stage, so its sum is not the headline), with
the projections timed on their own as the same GEMMs (ssp_dense_forward) on a slab.
The yardstick is the same network composed from torch in slabs of the same size, TF32 off: conv2d, one matmul per projection, per-step
matmul plus element-wise gates.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP32_MFMA_PEAK_TFLOPS = 157.3
T, D, F, H, E, KH, KW, STRIDES = 98, 13, 64, 1024, 512, 5, 5, (2, 2)


def glorot(rng, shape, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, shape).astype(np.float32)


def init(rng, reset_after):
    """Keras' initialisation: Glorot-uniform kernels, one orthogonal block per gate, small biases"""
    K = glorot(rng, (KH, KW, 1, F), KH * KW, KH * KW * F)
    bc = (0.1 * rng.standard_normal(F)).astype(np.float32)
    grus, d_in = [], 7 * F
    for _ in range(3):
        W = glorot(rng, (d_in, 3 * H), d_in, 3 * H)
        U = np.concatenate([np.linalg.qr(rng.standard_normal((H, H)))[0] for _ in range(3)], axis=1).astype(np.float32)
        b = (0.1 * rng.standard_normal((2, 3 * H) if reset_after else (3 * H,))).astype(np.float32)
        grus.append((W, U, b))
        d_in = H
    return (K, bc, STRIDES), grus, (glorot(rng, (H, E), H, E), (0.1 * rng.standard_normal(E)).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-steps", type=int, default=2, help="timed passes of the torch composition (0: skip it)")
    ap.add_argument("--workspace-gib", type=float, default=4.0)
    ap.add_argument("--variants", default="all", help="all, or a comma list of e.g. sigmoid:1,hard_sigmoid:0 (activation:reset_after)")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_gru.py needs an MI355X (no CPU fallback exists)")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    from speech_signal_processing_amd import api, d_vector

    N = args.chunks
    device = torch.device("cuda", 0)
    gen = torch.Generator(device=device)
    gen.manual_seed(1234)
    X = 3.0 * torch.randn((N, T, D), dtype=torch.float32, device=device, generator=gen)
    To, Do = 49, 7
    flop_chunk = 2.0 * To * Do * F * KH * KW + sum(2.0 * To * (d + H) * 3 * H for d in (Do * F, H, H)) + 2.0 * H * E
    variants = [(a, r) for a in ("hard_sigmoid", "sigmoid") for r in (False, True)]
    if args.variants != "all":
        variants = [(v.split(":")[0], bool(int(v.split(":")[1]))) for v in args.variants.split(",")]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def median_ms(fn, warmup, steps):
        for _ in range(warmup):
            fn()
        ms = [timed(fn) for _ in range(steps)]
        return float(np.median(ms)), [float(min(ms)), float(max(ms))]

    rows = {}
    for act, reset_after in variants:
        conv, grus, dense = init(np.random.default_rng(0), reset_after)
        net = d_vector.ConvGruNet(conv, grus, dense, recurrent_activation=act, reset_after=reset_after,
                                  workspace_bytes=int(args.workspace_gib * (1 << 30)))
        out = net.predict(X)
        torch.cuda.synchronize()
        slab = net.last_slab
        ms, rng_ms = median_ms(lambda: net.predict(X), args.warmup, args.steps)
        parts = {"ms": None}
        net.predict(X, parts=parts)
        st = parts["ms"]
        # the projections on their own: the same GEMM on one slab's rows, scaled to the batch
        ctx = api.default_context(0, torch_stream=True)
        proj = []
        n1 = min(slab, N)
        for W, _, b in grus:
            xin = torch.randn((n1 * To, W.shape[0]), dtype=torch.float32, device=device, generator=gen)
            Wt = torch.from_numpy(np.ascontiguousarray(W.T)).to(device)
            bi = torch.from_numpy(np.ascontiguousarray(b.reshape(-1)[:3 * H])).to(device)
            api.dense_forward(ctx, xin, Wt, bi)
            proj.append(float(np.median([api.dense_forward(ctx, xin, Wt, bi, timing=True)[1] for _ in range(3)])) * N / n1)
            del xin
        row = {"pass_ms": ms, "pass_ms_min_max": rng_ms, "embeddings_per_s": N / (ms * 1e-3),
               "algorithmic_tflops": flop_chunk * N / (ms * 1e-3) / 1e12,
               "frac_of_fp32_mfma_peak": flop_chunk * N / (ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
               "slab_chunks": slab,
               "split_ms": {"conv": st["conv"], "projections": proj, "recurrent_steps": [g - p for g, p in zip(st["gru"], proj)],
                            "gru_layers_total": st["gru"], "tail": st["tail"]}}
        if args.torch_steps > 0:
            Kt = torch.from_numpy(np.ascontiguousarray(conv[0].transpose(3, 2, 0, 1))).to(device)
            bct = torch.from_numpy(conv[1]).to(device)
            gt = [tuple(torch.from_numpy(np.ascontiguousarray(v)).to(device) for v in g) for g in grus]
            Wdt, bdt = (torch.from_numpy(v).to(device) for v in dense)
            sig = torch.sigmoid if act == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0.0, 1.0))

            def torch_slab(x):
                n = x.shape[0]
                y = torch.nn.functional.conv2d(torch.nn.functional.pad(x[:, None], (2, 2, 1, 2)), Kt, bct, stride=STRIDES)
                h_seq = y.permute(0, 2, 3, 1).reshape(n, To, Do * F)
                for W, U, b in gt:
                    bi, br = (b[0], b[1]) if reset_after else (b, None)
                    P = torch.addmm(bi, h_seq.reshape(n * To, -1), W).view(n, To, 3 * H)
                    seq = torch.empty((n, To, H), dtype=torch.float32, device=device)
                    h = torch.zeros((n, H), dtype=torch.float32, device=device)
                    for t in range(To):
                        p = P[:, t]
                        if reset_after:
                            hu = torch.addmm(br, h, U)
                            z = sig(p[:, :H] + hu[:, :H])
                            r = sig(p[:, H:2 * H] + hu[:, H:2 * H])
                            hh = torch.tanh(p[:, 2 * H:] + r * hu[:, 2 * H:])
                        else:
                            zr = sig(p[:, :2 * H] + h @ U[:, :2 * H])
                            z, r = zr[:, :H], zr[:, H:]
                            hh = torch.tanh(p[:, 2 * H:] + (r * h) @ U[:, 2 * H:])
                        h = z * h + (1 - z) * hh
                        seq[:, t] = h
                    h_seq = seq
                yv = torch.addmm(bdt, h_seq.mean(dim=1), Wdt)
                return yv / torch.sqrt(torch.clamp((yv * yv).sum(dim=1, keepdim=True), min=1e-12))

            def torch_pass():
                return torch.cat([torch_slab(X[c0:c0 + slab]) for c0 in range(0, N, slab)])

            tms, trng = median_ms(torch_pass, 1, args.torch_steps)
            row["torch_composition_ms"] = tms
            row["torch_composition_ms_min_max"] = trng
            row["speedup_over_torch_composition"] = tms / ms
            row["max_abs_diff_vs_torch"] = float((torch_pass() - out).abs().max().item())
            del Kt, gt
        rows["%s,reset_after=%d" % (act, reset_after)] = row
        del net, out
        torch.cuda.empty_cache()
    line = {"metric": "conv + GRU d-vector embeddings/s (Conv2D -> 3 x GRU(1024) -> mean -> Dense(512) -> L2, exact-fp32 MFMA)",
            "config": {"workload": "%d chunks x (%d, %d) resident in HBM" % (N, T, D), "steps": args.steps, "warmup": args.warmup,
                       "gflop_per_chunk": flop_chunk / 1e9, "workspace_gib": args.workspace_gib, "device": torch.cuda.get_device_name(0)},
            **rows}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
