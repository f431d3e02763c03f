"""Measure the x-vector extractor on one MI355X and write profiles/xvector.md (bench.py is the flagship's yardstick, not this).

    python tools/bench_xvector.py [--utts 12000] [--recs 256] [--reps 3] [--out profiles/xvector.md]

(a) --utts utterances x 298 frames x 39 columns through the standard network (counted work: 5.41 MFLOP per pooled frame);
(b) --recs recordings x 60000 frames with the 799 windows of 150 frames every 75 that lie inside a recording: one windowed call against per-chunk extraction.
In the same process: every frame layer beside ssp_dense_forward on the explicitly unfolded matrix of the same GEMM shape, and the
network composed from torch (conv1d with dilation, var, linear; TF32 off) on the same tensors.  Times are hipEvent milliseconds around
the whole call on resident device tensors, the median of --reps after one warm-up call."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3     # fp32 MFMA, MI355X
SNYDER = ((5, 1), (3, 2), (3, 3), (1, 1), (1, 1))


def median_ms(fn, reps):
    fn()
    return float(np.median([fn() for _ in range(reps)]))


def torch_ms(torch, fn, reps):
    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    return median_ms(once, reps)


def flops_per_pooled_frame(net):
    return sum(2.0 * L["W"].size for L in net.frame_layers)


def torch_network(torch, net, dev):
    import torch.nn.functional as F
    fl = [{k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in L.items()} for L in net.frame_layers]
    sl = [{k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in L.items()} for L in net.segment_layers]
    for L in fl:
        L["Wc"] = L["W"].permute(0, 2, 1).contiguous()      # (units, d_in, taps)

    def run(x):     # x (N, T, d_in), equal lengths
        h = x.transpose(1, 2)
        for L in fl:
            h = F.conv1d(h, L["Wc"], L["b"], dilation=L["dilation"])
            if L["relu"]:
                h = torch.relu(h)
            if L["scale"] is not None:
                h = h * L["scale"][None, :, None] + L["offset"][None, :, None]
        p = torch.cat([h.mean(2), torch.sqrt(torch.clamp(h.var(2, unbiased=False), min=net.var_floor))], dim=1)
        for L in sl:
            p = F.linear(p, L["W"], L["b"])
            if L["relu"]:
                p = torch.relu(p)
        return p
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=12000)
    ap.add_argument("--recs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xvector.md"))
    args = ap.parse_args()
    import torch
    from speech_signal_processing_amd import api, xvector
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    dev = "cuda:0"
    ctx = api.default_context(torch_stream=True)
    rng = np.random.RandomState(0)
    net = xvector.XVectorNet.snyder(39, rng)
    fwd = api.XVectorForward(ctx, net.frame_layers, net.segment_layers, net.var_floor)
    R = fwd.receptive_field
    per_frame = flops_per_pooled_frame(net)
    lines = ["# x-vector extractor on one MI355X (`tools/bench_xvector.py`)", "",
             "Standard network (Snyder et al. 2018), 39 columns in, R = %d, %.2f MFLOP per pooled frame in the frame layers; fp32 MFMA peak %.1f TFLOP/s."
             % (R, per_frame / 1e6, PEAK_TFLOPS), "Medians of %d calls after a warm-up, hipEvents around the whole call, tensors resident in HBM, TF32 off in torch." % args.reps, ""]

    shown = [0]

    def show():     # (what is measured so far, should a later block fail)
        print("\n".join(lines[shown[0]:]), flush=True)
        shown[0] = len(lines)
    # ---------------------------------------------------------------------------------------------------------------- (a)
    N, T = args.utts, 298
    feats = torch.randn(N * T, 39, device=dev)
    seg = api.Segments.from_lengths(ctx, [T] * N)
    ms_a = median_ms(lambda: fwd.forward(feats, seg, timing=True)[1], args.reps)
    work_a = per_frame * N * (T - R + 1)
    tnet = torch_network(torch, net, dev)
    chunk = 500

    def torch_a():
        x = feats.view(N, T, 39)
        return torch.cat([tnet(x[i:i + chunk]) for i in range(0, N, chunk)])
    ms_ta = torch_ms(torch, torch_a, args.reps)
    got, ref = fwd.forward(feats, seg), torch_a()
    err_a = float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))
    lines += ["## (a) %d utterances x %d frames" % (N, T), "",
              "| what | ms | TFLOP/s | of the fp32 MFMA peak |", "|---|---|---|---|",
              "| `ssp_xvector_forward` (slabs of %d utterances under the 2 GiB workspace cap) | %.1f | %.1f | %.2f |" % (fwd.last_slab, ms_a, work_a / ms_a / 1e9, work_a / ms_a / 1e9 / PEAK_TFLOPS),
              "| torch: conv1d (dilation), var, linear, %d utterances at a time | %.1f | %.1f | %.2f |" % (chunk, ms_ta, work_a / ms_ta / 1e9, work_a / ms_ta / 1e9 / PEAK_TFLOPS), "",
              "Counted work %.2f TFLOP (%.0f ms at the peak); library / torch = %.2f%s; largest difference between the two %.2e of the largest embedding entry."
              % (work_a / 1e12, work_a / PEAK_TFLOPS / 1e9, ms_a / ms_ta, " — **the library is %.2f x slower than torch**" % (ms_a / ms_ta) if ms_a > ms_ta else "", err_a), ""]

    show()
    # ------------------------------------------------------------------------------------------- layers beside the dense kernel
    rows = 128 * 1024
    lines += ["## Frame layers beside `ssp_dense_forward` on the unfolded matrix (%d rows)" % rows, "",
              "| layer (taps, dilation, d_in -> units) | `ssp_tdnn_forward` ms | TFLOP/s | `ssp_dense_forward` on [rows x taps d_in] ms | TFLOP/s | tdnn / dense |", "|---|---|---|---|---|---|"]
    d = 39
    seg1 = api.Segments.from_lengths(ctx, [rows])
    slower = []
    for L in net.frame_layers:
        taps, dil, units = L["W"].shape[1], L["dilation"], L["W"].shape[0]
        x = torch.randn(rows, d, device=dev)
        W = torch.from_numpy(L["W"]).to(dev)
        b, sc, of = (torch.from_numpy(L[k]).to(dev) for k in ("b", "scale", "offset"))
        ms_t = median_ms(lambda: api.tdnn_forward(ctx, x, seg1, W, b, dilation=dil, relu=True, scale=sc, offset=of, timing=True)[2], args.reps)
        n_out = rows - (taps - 1) * dil
        unf = torch.cat([x[j * dil:j * dil + n_out] for j in range(taps)], dim=1).contiguous()
        unf = torch.cat([unf, torch.zeros(rows - n_out, taps * d, device=dev)])      # the same number of rows
        Wt = W.reshape(units, taps * d).contiguous()
        ms_d = median_ms(lambda: api.dense_forward(ctx, unf, Wt, b, relu=True, timing=True)[1], args.reps)
        fl = 2.0 * rows * taps * d * units
        lines.append("| (%d, %d, %d -> %d) | %.3f | %.1f | %.3f | %.1f | %.2f |" % (taps, dil, d, units, ms_t, fl / ms_t / 1e9, ms_d, fl / ms_d / 1e9, ms_t / ms_d))
        if ms_t > 1.02 * ms_d:
            slower.append("(%d, %d, %d -> %d): %.2f x" % (taps, dil, d, units, ms_t / ms_d))
        del x, unf
        d = units
    lines += ["", ("**Slower than the dense kernel on the unfolded matrix:** " + "; ".join(slower) + ".") if slower else
              "No frame layer is slower than the dense kernel on the unfolded matrix (2 % margin).", ""]

    show()
    # ---------------------------------------------------------------------------------------------------------------- (b)
    Rn, Tn, wl, wh = args.recs, 60000, 150, 75
    nw = (Tn - wl) // wh + 1      # 799: every window of 150 frames every 75 that lies inside the recording
    feats_b = torch.randn(Rn * Tn, 39, device=dev)
    segb = api.Segments.from_lengths(ctx, [Tn] * Rn)
    wins = np.stack([np.repeat(np.arange(Rn), nw), np.tile(np.arange(nw) * wh, Rn), np.tile(np.arange(nw) * wh + wl, Rn)], axis=1).astype(np.int64)
    t0 = time.time()
    ms_w = median_ms(lambda: fwd.forward(feats_b, segb, wins, timing=True)[1], args.reps)
    slab_w = fwd.last_slab
    idx = (torch.from_numpy(wins[:, 0] * Tn + wins[:, 1]).to(dev)[:, None] + torch.arange(wl, device=dev)[None, :]).reshape(-1)
    chunks = feats_b[idx].contiguous()      # every window's frames as a sequence of its own
    segc = api.Segments.from_lengths(ctx, [wl] * (Rn * nw))
    ms_c = median_ms(lambda: fwd.forward(chunks, segc, timing=True)[1], args.reps)
    same = bool(torch.equal(fwd.forward(feats_b, segb, wins).view(torch.int32), fwd.forward(chunks, segc).view(torch.int32)))
    work_w, work_c = per_frame * Rn * Tn, per_frame * Rn * nw * wl
    lines += ["## (b) %d recordings x %d frames, %d windows of %d frames every %d" % (Rn, Tn, nw, wl, wh), "",
              "| what | ms | frame-layer rows | TFLOP/s |", "|---|---|---|---|",
              "| one windowed `ssp_xvector_forward` (frame layers once per recording; slabs of %d recordings) | %.1f | %d | %.1f |" % (slab_w, ms_w, Rn * Tn, work_w / ms_w / 1e9),
              "| per-chunk extraction of the same %d windows | %.1f | %d | %.1f |" % (Rn * nw, ms_c, Rn * nw * wl, work_c / ms_c / 1e9), "",
              "Per-chunk / windowed = %.2f (by count %.2f); the two give the same bits on every window: %s.  (Wall time of this block: %.0f s.)"
              % (ms_c / ms_w, work_c / work_w, same, time.time() - t0), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines[shown[0]:]), flush=True)


if __name__ == "__main__":
    main()
