"""Speaker diarization — "who spoke when" in recordings whose speakers are not enrolled — after Kaldi's diarization/ recipe: cut the speech
into short windows, embed every window, score all window pairs of a recording (cosine or PLDA; api.pairwise_scores), cluster them
agglomeratively (api.ahc_cluster, one workgroup per recording) down to a threshold or a known speaker count.  An extension and UNPINNED:
the reference has no diarization; tests/diarize_oracle.py restates the two kernels.

    from speech_signal_processing_amd import diarize
    d = diarize.Diarizer("cosine", linkage="average", threshold=0.5)
    labels, n_clusters = d.cluster(embeddings, counts)                 # embeddings (total, q), counts: windows per recording
    frames = d.run(signals, embed, win=24000, hop=12000)               # per signal: one label per VAD frame, -1 = no speech

    d = diarize.Diarizer(plda_model, threshold=0.0, resegment=True)    # pair scores -> AHC -> VB-HMM resegmentation, all on the device

``VbHmm`` is the resegmentation pass on its own (api.vb_resegment: a Bayesian HMM over the projected vectors, started from the AHC labels).
``windows`` and ``frame_labels`` are host helpers; ``metrics.diarization_error`` scores the frame labels against a reference."""
from __future__ import annotations

import numpy as np

from . import api

_is_torch = api._is_torch


def windows(segments, win, hop, min_len=None):
    """Sliding windows over speech segments: ``segments`` is a list of (start, end) sample pairs (end exclusive; what
    ``VAD.speech_segments`` returns); every segment is cut into windows of ``win`` samples every ``hop`` samples from its start; where the
    next window would run past the segment's end, what it covers of the segment — the whole of a segment shorter than ``win`` — is
    kept as a last, shorter window if that is at least ``min_len`` samples (default: ``win // 2``).  -> int64 (n_windows, 2) of (start, end)."""
    win, hop = int(win), int(hop)
    min_len = win // 2 if min_len is None else int(min_len)
    if win < 1 or hop < 1 or min_len < 1:
        raise ValueError("win, hop and min_len must be >= 1")
    out = []
    for a, b in segments:
        a, b = int(a), int(b)
        s = a
        while s + win <= b:
            out.append((s, s + win))
            s += hop
        if b - s >= min_len:   # the tail: what the next window would have covered of the segment
            out.append((s, b))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def frame_labels(wins, labels, n_frames, frame_hop):
    """One label per frame: frame t stands at sample ``t * frame_hop``; a frame inside at least one window (start <= sample < end) takes
    the label of the window whose centre is nearest, ties to the earlier window; a frame outside every window gets -1.
    -> int32 (n_frames,)."""
    wins = np.asarray(wins, dtype=np.int64).reshape(-1, 2)
    labels = np.asarray(labels).reshape(-1)
    if labels.shape[0] != wins.shape[0]:
        raise ValueError("one label per window")
    out = np.full(int(n_frames), -1, dtype=np.int32)
    if wins.shape[0] == 0 or n_frames == 0:
        return out
    pos = np.arange(int(n_frames), dtype=np.int64) * int(frame_hop)
    inside = (pos[:, None] >= wins[None, :, 0]) & (pos[:, None] < wins[None, :, 1])
    dist = np.abs(2 * pos[:, None] - (wins[None, :, 0] + wins[None, :, 1]))   # twice the distance to the centre: exact in integers
    dist = np.where(inside, dist, np.iinfo(np.int64).max)
    best = np.argmin(dist, axis=1)   # (the first minimum: the earlier window)
    hit = inside.any(axis=1)
    out[hit] = labels[best[hit]].astype(np.int32)
    return out


class VbHmm:
    """VB-HMM resegmentation (VBx) of diarization labels: ``phi_or_plda`` is the between-speaker variance of the projected space — a
    vector of q entries, or a fitted plda.Plda, whose ``psi_`` it is and whose ``project`` then maps raw embeddings into that space.  The
    parameters are api.vb_resegment's; n_states None: 64 for device inputs, max(label) + 1 for host inputs."""

    def __init__(self, phi_or_plda, loop_prob=0.99, Fa=0.3, Fb=17.0, init_smoothing=5.0, max_iters=10, epsilon=1e-4, n_states=None,
                 ctx=None):
        self.plda = phi_or_plda if hasattr(phi_or_plda, "psi_") else None
        phi = self.plda.psi_ if self.plda is not None else phi_or_plda
        self.phi = np.ascontiguousarray(phi.cpu().numpy() if _is_torch(phi) else phi, dtype=np.float32).reshape(-1)
        if self.phi.size < 1 or not np.isfinite(self.phi).all() or (self.phi < 0).any():
            raise ValueError("phi must be a vector of finite, non-negative entries")
        self.params = dict(loop_prob=float(loop_prob), Fa=float(Fa), Fb=float(Fb), init_smoothing=float(init_smoothing),
                           max_iters=int(max_iters), epsilon=float(epsilon))
        self.n_states, self.ctx = n_states, ctx

    def resegment(self, projected, counts, labels, n_init=None, want=()):
        """projected (total, q): the PROJECTED vectors in time order, numpy or torch CUDA tensor; counts: windows per recording (or an
        api.Segments); labels (total,), n_init (R,) or None: the initial labels and cluster counts, of projected's kind.  -> the dict
        of api.vb_resegment ("labels", "states", "n_speakers", "n_iters" and what ``want`` names)"""
        self.ctx = self.ctx or api.default_context()
        return api.vb_resegment(self.ctx, projected, counts, self.phi, labels, n_init, n_states=self.n_states, want=want, **self.params)


class Diarizer:
    """backend: "cosine" (rows are L2-normalised, the score is their cosine) or a fitted plda.Plda (rows are projected, the score is the
    log-likelihood ratio of the pair); linkage "average" / "complete" / "single"; merging stops below ``threshold`` or at
    ``min_clusters`` clusters.  resegment: None, or a VbHmm (True: VbHmm(backend)) that runs on the AHC labels; with it ``cluster``
    returns the VB-HMM labels and speaker counts.  It needs the projected space of a PLDA back end; with the cosine back end True
    raises ValueError (there is no phi) and a VbHmm built from an explicit phi takes the rows as they are given."""

    def __init__(self, backend="cosine", linkage="average", threshold=0.0, min_clusters=1, ctx=None, resegment=None):
        if backend != "cosine" and not hasattr(backend, "pairwise_coeffs"):
            raise ValueError('backend must be "cosine" or a fitted plda.Plda')
        if linkage not in api.AHC_LINKAGES:
            raise ValueError("linkage must be one of %s" % sorted(api.AHC_LINKAGES))
        self.backend, self.linkage, self.threshold, self.min_clusters = backend, linkage, float(threshold), int(min_clusters)
        self.ctx = ctx
        if resegment is True:
            if backend == "cosine":
                raise ValueError("resegment=True needs a PLDA back end: the cosine back end has no between-speaker variance (pass a VbHmm built from phi)")
            resegment = VbHmm(backend)
        if resegment is not None and resegment is not False and not isinstance(resegment, VbHmm):
            raise ValueError("resegment must be None, True or a VbHmm")
        self.resegment = resegment or None

    def scores(self, embeddings, counts):
        """-> (packed score blocks, the api.Segments of the recordings)"""
        self.ctx = self.ctx or api.default_context()
        seg = api._as_recordings(self.ctx, counts)
        if self.backend == "cosine":
            return api.pairwise_scores(self.ctx, api.l2_normalize(self.ctx, embeddings), seg), seg
        g, h, c0 = self.backend.pairwise_coeffs()
        return api.pairwise_scores(self.ctx, self.backend.project(embeddings), seg, g=g, h=h, c0=c0), seg

    def cluster(self, embeddings, counts, n_speakers=None):
        """embeddings (total, q) numpy or torch CUDA tensor, counts: windows per recording (or an api.Segments).  -> (labels (total,)
        int32, n_clusters (R,) int32) of embeddings' kind"""
        if self.resegment is None:
            s, seg = self.scores(embeddings, counts)
            r = api.ahc_cluster(self.ctx, s, seg, linkage=self.linkage, threshold=self.threshold, min_clusters=self.min_clusters,
                                n_speakers=n_speakers)
            return r["labels"], r["n_clusters"]
        # pair scores, AHC and the VB-HMM on the same rows: projected once, the AHC outputs stay where they are
        self.ctx = self.ctx or api.default_context()
        seg = api._as_recordings(self.ctx, counts)
        if self.backend == "cosine":
            rows = embeddings
            s = api.pairwise_scores(self.ctx, api.l2_normalize(self.ctx, embeddings), seg)
        else:
            rows = self.backend.project(embeddings)
            g, h, c0 = self.backend.pairwise_coeffs()
            s = api.pairwise_scores(self.ctx, rows, seg, g=g, h=h, c0=c0)
        r = api.ahc_cluster(self.ctx, s, seg, linkage=self.linkage, threshold=self.threshold, min_clusters=self.min_clusters,
                            n_speakers=n_speakers)
        self.resegment.ctx = self.resegment.ctx or self.ctx
        v = self.resegment.resegment(rows, seg, r["labels"], r["n_clusters"])
        return v["labels"], v["n_speakers"]

    def run(self, signals, embed, win, hop, min_len=None, n_speakers=None, **vad):
        """signals: a list of raw signals (int16 PCM or float arrays); embed: a callable that takes the list of window chunks (1-D arrays)
        and returns one embedding row per chunk (numpy or torch CUDA); when it has an ``embed_windows(signals, wins)`` method that is
        called instead, with the per-signal (n, 2) sample windows.  VAD.detect_batch (keywords ``vad``) -> VAD.speech_segments ->
        windows(win, hop, min_len) -> embed -> cluster -> frame_labels on the VAD's frames.  -> a list of int32 arrays, one label per
        VAD frame of each signal, -1 where there is no speech (or no window)."""
        from . import VAD
        masks = VAD.detect_batch(signals, **vad)
        wins = [windows(VAD.speech_segments(m, len(x)), win, hop, min_len) for m, x in zip(masks, signals)]
        counts = [w.shape[0] for w in wins]
        chunks = [np.asarray(x).reshape(-1)[a:b] for x, w in zip(signals, wins) for a, b in w]
        step = VAD.frameSize - VAD.overlap
        if not chunks:
            return [np.full(len(m), -1, dtype=np.int32) for m in masks]
        # an embedder that can pool windows of a recording it has run once (xvector.Extractor) is handed the recordings and the windows
        emb = embed.embed_windows(signals, wins) if hasattr(embed, "embed_windows") else embed(chunks)
        if int(emb.shape[0]) != len(chunks):
            raise ValueError("embed returned %d rows for %d chunks" % (int(emb.shape[0]), len(chunks)))
        labels, _ = self.cluster(emb, counts, n_speakers=n_speakers)
        labels = labels.cpu().numpy() if _is_torch(labels) else labels
        off = np.concatenate([[0], np.cumsum(counts)])
        return [frame_labels(w, labels[off[i]:off[i + 1]], len(m), step) for i, (w, m) in enumerate(zip(wins, masks))]
