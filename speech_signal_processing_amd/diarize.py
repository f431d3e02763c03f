"""Speaker diarization — "who spoke when" in recordings whose speakers are not enrolled — after Kaldi's diarization/ recipe: cut the speech
into short windows, embed every window, score all window pairs of a recording (cosine or PLDA; api.pairwise_scores), cluster them
agglomeratively (api.ahc_cluster, one workgroup per recording) down to a threshold or a known speaker count.  An extension and UNPINNED:
the reference has no diarization; tests/diarize_oracle.py restates the two kernels.

    from speech_signal_processing_amd import diarize
    d = diarize.Diarizer("cosine", linkage="average", threshold=0.5)
    labels, n_clusters = d.cluster(embeddings, counts)                 # embeddings (total, q), counts: windows per recording
    frames = d.run(signals, embed, win=24000, hop=12000)               # per signal: one label per VAD frame, -1 = no speech

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


class Diarizer:
    """backend: "cosine" (rows are L2-normalised, the score is their cosine) or a fitted plda.Plda (rows are projected, the score is the
    log-likelihood ratio of the pair); linkage "average" / "complete" / "single"; merging stops below ``threshold`` or at
    ``min_clusters`` clusters."""

    def __init__(self, backend="cosine", linkage="average", threshold=0.0, min_clusters=1, ctx=None):
        if backend != "cosine" and not hasattr(backend, "pairwise_coeffs"):
            raise ValueError('backend must be "cosine" or a fitted plda.Plda')
        if linkage not in api.AHC_LINKAGES:
            raise ValueError("linkage must be one of %s" % sorted(api.AHC_LINKAGES))
        self.backend, self.linkage, self.threshold, self.min_clusters = backend, linkage, float(threshold), int(min_clusters)
        self.ctx = ctx

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
        s, seg = self.scores(embeddings, counts)
        r = api.ahc_cluster(self.ctx, s, seg, linkage=self.linkage, threshold=self.threshold, min_clusters=self.min_clusters,
                            n_speakers=n_speakers)
        return r["labels"], r["n_clusters"]

    def run(self, signals, embed, win, hop, min_len=None, n_speakers=None, **vad):
        """signals: a list of raw signals (int16 PCM or float arrays); embed: a callable that takes the list of window chunks (1-D arrays)
        and returns one embedding row per chunk (numpy or torch CUDA).  VAD.detect_batch (keywords ``vad``) -> VAD.speech_segments ->
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
        emb = embed(chunks)
        if int(emb.shape[0]) != len(chunks):
            raise ValueError("embed returned %d rows for %d chunks" % (int(emb.shape[0]), len(chunks)))
        labels, _ = self.cluster(emb, counts, n_speakers=n_speakers)
        labels = labels.cpu().numpy() if _is_torch(labels) else labels
        off = np.concatenate([[0], np.cumsum(counts)])
        return [frame_labels(w, labels[off[i]:off[i + 1]], len(m), step) for i, (w, m) in enumerate(zip(wins, masks))]
