"""Times sliding-window normalisation (modes 0, 1, 2) and speech-frame selection at three shapes, beside two yardsticks in the same
process and on the same tensors: ssp_cmvn (one mean and deviation per utterance: the least such a pass can cost) and the same step
composed from torch (unfold, then mean / std, or compare-and-sum; boolean indexing for the selection).

    python tools/bench_featnorm.py [--shapes 100000x298x39,10000x3000x39,256x60000x39] [--window 300] [--reps 5] [--md FILE]

Device milliseconds between events (the library's own timing), median of --reps calls after one untimed call.  The torch compositions
hold a (frames, dim, window) view or mask, so they run on a slice of the batch that fits --torch-elems elements and are reported per
million frames; the library's and ssp_cmvn's times are of the whole batch and are also given per million frames.  The error against
float64 is measured on a sample batch of 8 utterances of at most 2000 frames of the same distribution (tests/featnorm_oracle.py).
Prints one JSON line per measurement; --md writes the table of profiles/featnorm.md."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, reps):
    fn()
    return float(np.median([fn() for _ in range(reps)]))


def torch_ms(fn, reps):
    import torch
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def torch_sliding(x3, W, mode):
    """x3 (N, T, D) -> the step composed from torch ops; every utterance has T frames"""
    import torch
    N, T, D = x3.shape
    Wn = min(W, T)
    win = x3.unfold(1, Wn, 1)                                      # (N, T - Wn + 1, D, Wn), a view
    idx = (torch.arange(T, device=x3.device) - W // 2).clamp_(0, T - Wn)
    if mode < 2:
        mean = win.mean(-1)
        y = x3 - mean[:, idx]
        if mode == 1:
            sd = win.std(-1, unbiased=False)
            y = y / torch.where(sd < 10 * 2.0 ** -23, torch.ones_like(sd), sd)[:, idx]
        return y
    w = win[:, idx]                                                # (N, T, D, Wn)
    xe = x3.unsqueeze(-1)
    k = 2 * (w < xe).sum(-1) + (w == xe).sum(-1)
    return torch.special.ndtri(k.to(torch.float32) / (2.0 * Wn))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x298x39,10000x3000x39,256x60000x39")
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-elems", type=float, default=1.5e9, help="largest (frames x dim x window) intermediate of a torch composition")
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import torch
    from speech_signal_processing_amd import api
    import featnorm_oracle as FO
    if not torch.cuda.is_available():
        raise SystemExit("bench_featnorm: no GPU (nothing is measured without one)")
    ctx = api.default_context()
    W = args.window
    rows = []

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        rows.append(kw)

    # ---- error against float64, on a sample batch
    rng = np.random.default_rng(1)
    for T in sorted({min(int(s.split("x")[1]), 2000) for s in args.shapes.split(",")}):
        lens = [T] * 8
        x = (rng.standard_normal((8 * T, 39)) * rng.uniform(0.5, 2.0, 39) + rng.uniform(-3, 3, 39)).astype(np.float32)
        seg = api.Segments.from_lengths(ctx, lens)
        for mode in (0, 1, 2):
            got = api.featnorm_sliding(ctx, torch.from_numpy(x).cuda(), seg, window=W, mode=mode).cpu().numpy()
            want, band = FO.sliding_batch(x, seg.offsets, W, mode)
            err = np.abs(got - want)
            assert (err[band == 0] == 0).all()                       # (mode 2 at k = n: exactly 0)
            share = np.where(band > 0, err / np.where(band > 0, band, 1.0), 0.0)
            emit(what="error", frames_per_utt=T, mode=mode, max_abs_err=float(err.max()), max_share_of_band=float(share.max()))

    for shape in args.shapes.split(","):
        N, T, D = (int(v) for v in shape.split("x"))
        frames = N * T
        g = torch.Generator(device="cuda").manual_seed(2)
        x = torch.randn((frames, D), device="cuda", generator=g) * 1.5 + 0.5
        mask = (torch.rand(frames, device="cuda", generator=g) < 0.6).to(torch.uint8)
        seg = api.Segments.from_lengths(ctx, [T] * N)
        per_m = 1e6 / frames
        ms = median_ms(lambda: api.cmvn_features(ctx, x, seg, timing=True)[1], args.reps)
        emit(what="ssp_cmvn", shape=shape, ms=ms, ms_per_mframe=ms * per_m)
        for mode in (0, 1, 2):
            ms = median_ms(lambda: api.featnorm_sliding(ctx, x, seg, window=W, mode=mode, timing=True)[1], args.reps)
            extra = {}
            if mode == 2:
                extra["compares"] = float(frames) * D * min(W, T)
                extra["gcompares_per_s"] = extra["compares"] / ms / 1e6
            else:
                extra["gb_per_s_in_plus_out"] = 2.0 * frames * D * 4 / ms / 1e6
            emit(what="ssp_featnorm_sliding", shape=shape, mode=mode, window=W, ms=ms, ms_per_mframe=ms * per_m, **extra)
            n_t = int(max(1, min(N, args.torch_elems // (T * D * min(W, T)))))
            x3 = x[:n_t * T].view(n_t, T, D)
            tms = torch_ms(lambda: torch_sliding(x3, W, mode), args.reps)
            emit(what="torch composition", shape=shape, mode=mode, window=W, utterances=n_t, ms=tms, ms_per_mframe=tms * 1e6 / (n_t * T))
        ms = median_ms(lambda: api.select_frames(ctx, x, seg, mask, timing=True)[3], args.reps)
        emit(what="ssp_select_frames", shape=shape, ms=ms, ms_per_mframe=ms * per_m, gb_per_s_in_plus_out=(1.0 + 0.6) * frames * D * 4 / ms / 1e6)
        tms = torch_ms(lambda: x[mask.bool()], args.reps)
        emit(what="torch boolean indexing", shape=shape, ms=tms, ms_per_mframe=tms * per_m)
        del x, mask, x3
        torch.cuda.empty_cache()

    if args.md:
        with open(args.md, "w") as f:
            f.write("| shape (utterances x frames x dim) | step | ms, whole batch | ms per million frames | torch composition, ms per million frames (utterances timed) | `ssp_cmvn`, ms per million frames |\n|---|---|---|---|---|---|\n")
            for shape in args.shapes.split(","):
                cm = next(r for r in rows if r["what"] == "ssp_cmvn" and r["shape"] == shape)
                for mode in (0, 1, 2):
                    a = next(r for r in rows if r["what"] == "ssp_featnorm_sliding" and r["shape"] == shape and r["mode"] == mode)
                    t = next(r for r in rows if r["what"] == "torch composition" and r["shape"] == shape and r["mode"] == mode)
                    f.write("| %s | `ssp_featnorm_sliding` mode %d, window %d | %.3f | %.4f | %.4f (%d) | %.4f |\n" % (
                        shape, mode, W, a["ms"], a["ms_per_mframe"], t["ms_per_mframe"], t["utterances"], cm["ms_per_mframe"]))
                a = next(r for r in rows if r["what"] == "ssp_select_frames" and r["shape"] == shape)
                t = next(r for r in rows if r["what"] == "torch boolean indexing" and r["shape"] == shape)
                f.write("| %s | `ssp_select_frames`, 60 %% kept | %.3f | %.4f | %.4f (all) | %.4f |\n" % (
                    shape, a["ms"], a["ms_per_mframe"], t["ms_per_mframe"], cm["ms_per_mframe"]))
            f.write("\n| frames per utterance (sample batch of 8) | mode | max abs error against float64 | largest share of the band |\n|---|---|---|---|\n")
            for r in rows:
                if r["what"] == "error":
                    f.write("| %d | %d | %.3e | %.3f |\n" % (r["frames_per_utt"], r["mode"], r["max_abs_err"], r["max_share_of_band"]))


if __name__ == "__main__":
    main()
