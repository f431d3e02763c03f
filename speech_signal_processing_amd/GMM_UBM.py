"""GPU-backed mirror of the hot-path functions of the reference's ``GMM_UBM.py``.

* ``delta``            GMM_UBM.py:53-69
* ``extract_feature``  GMM_UBM.py:72-118  (sidekit mfcc -> [c, delta c] -> per-utterance scale; one fused kernel; 'PLP' and 'MFCC_PLP':
                       the fused PLP tail, api.plp_features)
* ``chunk_features`` / ``identify_language``  the language mode's read-out, UI/tmp.py:303-360
* ``score_matrix``     the scoring loops GMM_UBM.py:181-197 as a function that returns what the reference prints
* ``GMM``              GMM_UBM.py:134-199: trains one GMM per speaker + the UBM (EM on the GPU, gmm_train.GaussianMixture)
                       or takes pre-trained models, then scores
"""
from __future__ import annotations

import functools
import os
import pickle as pkl

import numpy as np

from . import api, frontend
from .gmm_train import GaussianMixture, fit_many, map_adapt
from .sidekit_features import mfcc, mfcc_batch, plp, plp_batch, plp_features_batch  # noqa: F401  (GMM_UBM.py:20 imports both names)


def delta(feat, N=2):
    """GMM_UBM.py:53-69 — regression delta over +-N frames with edge padding; returns an array like ``feat``."""
    if N < 1:
        raise ValueError('N must be an integer >= 1')
    feat = np.asarray(feat)
    if feat.ndim != 2:
        raise ValueError("feat must be (NUMFRAMES, features)")
    ctx = api.default_context()
    seg = api.Segments.from_lengths(ctx, [feat.shape[0]])
    out = api.delta_features(ctx, feat, seg, N)
    return out.astype(feat.dtype if feat.dtype.kind == "f" else np.float64)


@functools.lru_cache(maxsize=8)
def _feature_plan(feature_type, fs, delta_order):
    if feature_type != 'MFCC':
        raise NameError  # GMM_UBM.py:100-101
    return api.MfccPlan(api.default_context(), frontend.preset_sidekit(fs=fs, delta_order=delta_order, cmvn=1))


_SLIDING_MODES = {'sliding': 1, 'warp': 2}


@functools.lru_cache(maxsize=8)
def _feature_plan_raw(fs, delta_order):
    return api.MfccPlan(api.default_context(), frontend.preset_sidekit(fs=fs, delta_order=delta_order, cmvn=0))


def _extract_sliding(x, fs, delta_order, mode, window):
    """[c, delta c (, delta delta c)] without the per-utterance scale, normalised over a sliding window on the device: one upload, the
    MFCC plan and api.featnorm_sliding there, one download."""
    import torch
    plan = _feature_plan_raw(fs, delta_order)
    flat, lens = api.flatten_signals(x)
    seg = api.Segments.from_lengths(plan.ctx, lens)
    fseg = plan.frame_segments(seg)
    if fseg.total == 0:
        return [np.zeros((0, plan.d_out), dtype=np.float64) for _ in lens]
    dev = torch.from_numpy(np.ascontiguousarray(flat)).to("cuda:%d" % plan.ctx.device)
    feats = api.featnorm_sliding(plan.ctx, plan.run(dev, seg, fseg), fseg, window=window, mode=mode)
    feats = feats.cpu().numpy().astype(np.float64)
    return [feats[fseg.offsets[i]:fseg.offsets[i + 1]] for i in range(fseg.n)]


def extract_feature(x, y, is_train=False, feature_type='MFCC', fs=16000, delta_order=1, norm='utterance', window=300):
    """GMM_UBM.py:72-118.  x: list of 1-D audio arrays, y: list of labels.
    Returns (feature, y) or (train_data, feature, y); every feature is (T_i, 26) float64 = scale([c, delta c]).
    ``delta_order=2`` appends delta-delta (39-d) — an extension used by the benchmark configs.
    ``norm`` (an extension; 'utterance': the reference's per-utterance scale, unchanged): 'sliding' normalises mean and variance over
    the ``window`` frames around each frame instead, 'warp' warps the features over them (featnorm.cmvn_sliding / feature_warp; MFCC only)."""
    if norm not in ('utterance', 'sliding', 'warp'):
        raise ValueError("norm must be 'utterance', 'sliding' or 'warp'")
    if norm != 'utterance':
        if feature_type != 'MFCC':
            raise NotImplementedError("norm=%r is provided for feature_type='MFCC'" % norm)
        feature = _extract_sliding(x, int(fs), int(delta_order), _SLIDING_MODES[norm], int(window))
        if not is_train:
            return feature, y
        train_data = {}
        for f, lab in zip(feature, y):
            train_data[lab] = np.vstack((train_data[lab], f)) if lab in train_data else f
        return train_data, feature, y
    if feature_type in ('PLP', 'MFCC_PLP'):  # GMM_UBM.py:94-99: plp -> hstack(c, delta c) -> scale; UI/tmp.py:319-324: hstack(mfcc, plp)
        feature = _extract_plp(x, int(fs), int(delta_order), with_mfcc=feature_type == 'MFCC_PLP')
        if not is_train:
            return feature, y
        train_data = {}
        for f, lab in zip(feature, y):
            train_data[lab] = np.vstack((train_data[lab], f)) if lab in train_data else f
        return train_data, feature, y
    plan = _feature_plan(feature_type, int(fs), int(delta_order))
    # the utterances are read from their own arrays (int16 PCM — what load_data reads, GMM_UBM.py:24-50 — goes to the device as int16)
    # and the float64 features are written by the library: no concatenation or widening pass here
    feats, fseg = api.mfcc_run_list(plan, x, out_dtype=np.float64)
    feature = [feats[fseg.offsets[i]:fseg.offsets[i + 1]] for i in range(fseg.n)]
    if not is_train:
        return feature, y
    train_data = {}
    for f, lab in zip(feature, y):
        train_data[lab] = np.vstack((train_data[lab], f)) if lab in train_data else f
    return train_data, feature, y


def _extract_plp(x, fs, delta_order, with_mfcc=False):
    """[c, delta c (, delta delta c)] of the PLP cepstra, per-utterance scaled (with_mfcc: [mfcc | plp | d mfcc | d plp ...], 'MFCC_PLP');
    one upload, the front end(s) and the fused tail on the device, one download."""
    feats, fseg = plp_features_batch(x, fs=fs, with_mfcc=with_mfcc, delta_order=delta_order, scale=True, out_dtype=np.float64)
    return [feats[fseg.offsets[i]:fseg.offsets[i + 1]] for i in range(len(x))]


def chunk_features(audio, feature_type='MFCC', fs=16000):
    """UI/tmp.py:303-326: the audio cut into whole 1 s chunks, every chunk's scaled features without deltas — 'MFCC' scale(mfcc(x)[0]),
    'PLP' scale(plp(x)[0]), 'MFCC_PLP' scale(hstack(mfcc(x)[0], plp(x)[0])) — all chunks in one batch.  Returns a list of
    (98, 13 or 26) float64 arrays (at 16 kHz)."""
    if feature_type not in ('MFCC', 'PLP', 'MFCC_PLP'):
        raise NameError  # UI/tmp.py:325-326
    audio = np.asarray(audio).reshape(-1)
    fs = int(fs)
    chunks = [audio[j * fs:(j + 1) * fs] for j in range(audio.shape[0] // fs)]
    if not chunks:
        return []
    if feature_type == 'MFCC':
        feats, fseg = mfcc_batch(chunks, fs=fs, scale=True, out_dtype=np.float64)
    else:
        feats, fseg = plp_features_batch(chunks, fs=fs, with_mfcc=feature_type == 'MFCC_PLP', scale=True, out_dtype=np.float64)
    return [feats[fseg.offsets[i]:fseg.offsets[i + 1]] for i in range(len(chunks))]


def language_readout(pred, names=('Chinese', 'English', 'Japanese')):
    """The arithmetic of UI/tmp.py:345-360 on a (chunks, languages) matrix of score differences: per chunk the arg-max, its name (index 0,
    index 1, anything else: the reference's if / elif / else) and exp(max) / sum exp of its row.  -> (names, probabilities)."""
    pred = np.asarray(pred, dtype=np.float64)
    if pred.ndim != 2 or pred.shape[1] < 1:
        raise ValueError("pred must be (chunks, languages)")
    am = pred.argmax(axis=1)
    out = [names[0] if i == 0 else (names[1] if i == 1 else names[2]) for i in am]
    prob = np.exp(pred.max(axis=1)) / np.exp(pred).sum(axis=1)
    return out, prob


def identify_language(models, ubm, features, names=('Chinese', 'English', 'Japanese')):
    """UI/tmp.py:337-360: pred[j, i] = models[i].score(features[j]) - ubm.score(features[j]) for every chunk j (``score_matrix``), the
    language of every chunk and its probability exp(max) / sum exp.  Returns (names, probabilities, pred)."""
    pred, _ = score_matrix(models, ubm, features)
    out, prob = language_readout(pred, names)
    return out, prob, pred


def _cov_kind(g):
    """'full' for a model whose precisions_cholesky_ is (K, D, D) (sklearn's default covariance_type), else what it says ('diag')"""
    kind = getattr(g, "covariance_type", None)
    if kind is None:
        kind = "full" if np.ndim(getattr(g, "precisions_cholesky_", 0)) == 3 else "diag"
    return kind


def score_matrix(models, ubm, feats, top_c=None):
    """GMM_UBM.py:181-187 as a function: pred[j, i] = models[i].score(feats[j]) - ubm.score(feats[j]).
    ``top_c`` (an extension; None: the dense path below, unchanged): an int evaluates the same difference over the UBM's best top_c
    mixtures of every frame (api.MapScorer; the models must be mean-adapted from ``ubm``, gmm_train.map_adapt(adapt='m')) — same shapes,
    same ValueError; with top_c = n_components it is the dense difference.

    models / ubm: fitted sklearn GaussianMixture(covariance_type='diag') objects (or anything with weights_,
    means_, covariances_).  When every model and the UBM are covariance_type='full' (weights_, means_, precisions_cholesky_) they are scored
    through api.GmmFullScorer, same shapes and errors; a mixed set, or top_c with full models, raises ValueError.
    feats: list of (T_j, D) arrays.  Returns (pred (U, S) float64, argmax (U,) int64).
    ValueError when an utterance with frames holds a NaN or infinite entry, as sklearn's score raises (the scorer answers such an
    utterance with a NaN row — include/ssp.h, ssp_gmm_score — so this is read off the scores: no pass over the host arrays).  An empty
    utterance keeps its NaN row."""
    kinds = {_cov_kind(g) for g in list(models) + [ubm]}  # (looked at before a context is made: the refusals need no device)
    if len(kinds) > 1:
        raise ValueError("score_matrix: the models and the UBM mix covariance types %s; score 'diag' and 'full' sets apart" % sorted(kinds))
    if kinds == {"full"} and top_c is not None:
        raise ValueError("score_matrix: top_c scoring needs mean-adapted 'diag' models; full-covariance models are scored densely")
    ctx = api.default_context()
    if kinds == {"full"}:
        scorer = api.GmmFullScorer.from_sklearn(ctx, models, ubm)
        r = scorer.score_list(feats)
        scorer.close()
        sc = np.asarray(r["scores"], dtype=np.float64)
        lens = np.array([np.shape(f)[0] for f in feats], dtype=np.int64)
        bad = np.flatnonzero(~np.isfinite(sc).all(axis=1) & (lens > 0))
        if bad.size:
            raise ValueError("Input contains NaN, infinity or a value too large for float32: utterance %d%s"
                             % (int(bad[0]), "" if bad.size == 1 else " (and %d more)" % (bad.size - 1)))
        return sc[:, 1:] - sc[:, :1], np.asarray(r["argmax"]).astype(np.int64)
    if top_c is not None:
        scorer = api.MapScorer.from_sklearn(ctx, models, ubm)
        r = scorer.score_list(feats, top_c=int(top_c))
        scorer.close()
        pred = np.asarray(r["diff"], dtype=np.float64)
        lens = np.array([np.shape(f)[0] for f in feats], dtype=np.int64)
        bad = np.flatnonzero(~np.isfinite(pred).all(axis=1) & (lens > 0))
        if bad.size:
            raise ValueError("Input contains NaN, infinity or a value too large for float32: utterance %d%s"
                             % (int(bad[0]), "" if bad.size == 1 else " (and %d more)" % (bad.size - 1)))
        return pred, np.asarray(r["argmax"]).astype(np.int64)
    scorer = api.GmmScorer.from_sklearn(ctx, models, ubm)
    r = scorer.score_list(feats)   # (the rows are gathered and narrowed by the library: no vstack + astype here)
    sc = np.asarray(r["scores"], dtype=np.float64)
    lens = np.array([np.shape(f)[0] for f in feats], dtype=np.int64)
    bad = np.flatnonzero(~np.isfinite(sc).all(axis=1) & (lens > 0))
    if bad.size:
        raise ValueError("Input contains NaN, infinity or a value too large for float32: utterance %d%s"
                         % (int(bad[0]), "" if bad.size == 1 else " (and %d more)" % (bad.size - 1)))
    return sc[:, 1:] - sc[:, :1], np.asarray(r["argmax"]).astype(np.int64)


def identify_with_confidence(models, ubm, feature):
    """The GUI's read-out of one utterance (UI/GMM_UBM_GUI.py:102-113): prob[0, i] = models[i].score(feature) - ubm.score(feature),
    res = argmax, then the softmax of the score differences, exp(prob) / sum exp(prob).  Returns (index, softmax probability of that
    index, the (1, S) softmax row)."""
    pred, am = score_matrix(models, ubm, [feature])
    e = np.exp(pred)
    prob = e / e.sum(axis=1)
    return int(am[0]), float(prob[0, am[0]]), prob


def save_models(gmms, ubm, model_dir="Model"):
    """The two pickles the reference writes after training (GMM_UBM.py:173-179): Model/GMM_MFCC_model.pkl (list of the
    per-speaker models) and Model/UBM_MFCC_model.pkl."""
    if not os.path.exists(model_dir):
        os.mkdir(model_dir)
    with open(os.path.join(model_dir, "GMM_MFCC_model.pkl"), "wb") as f:
        pkl.dump(gmms, f)
    with open(os.path.join(model_dir, "UBM_MFCC_model.pkl"), "wb") as f:
        pkl.dump(ubm, f)


def load_models(model_dir="Model"):
    """GMM_UBM.py:141-146: the pickled speaker models and UBM (sklearn GaussianMixture objects written by the reference,
    or gmm_train.GaussianMixture objects written by save_models)."""
    with open(os.path.join(model_dir, "GMM_MFCC_model.pkl"), "rb") as f:
        gmms = pkl.load(f)
    with open(os.path.join(model_dir, "UBM_MFCC_model.pkl"), "rb") as f:
        ubm = pkl.load(f)
    return gmms, ubm


def GMM(train, x_train, y_train, x_test, y_test, n_components=16, model=None, random_state=None, model_dir=None, seeding='host',
        adapt=None, relevance_factor=16.0, top_c=None, covariance_type='diag'):
    """GMM_UBM.py:134-199.  ``model`` falsy (the reference's default): one ``GaussianMixture(n_components, 'diag')`` per
    speaker is fitted on ``train[speaker]`` (speakers in ascending label order, like label_encoder.values()) and the UBM
    on the stacked training data (GMM_UBM.py:154-170), EM on the GPU (the speaker models together through gmm_train.fit_many for
    n_components <= 64 and D <= 47, bit for bit the loop's models); with ``model_dir`` (the reference always uses
    "Model") the two pickles of GMM_UBM.py:173-179 are written.  ``model=True``: load those pickles from ``model_dir``
    (default "Model", GMM_UBM.py:141-146).  ``model`` = (list_of_speaker_GMMs, UBM): use them as given.
    ``seeding``: where the k-means++ seeds of the speaker fits and the UBM fit are computed, 'host' or 'device' (gmm_train.GaussianMixture).
    ``adapt`` (an extension; None: the reference's independent fits, unchanged): 'map' trains the UBM on the pooled data exactly as
    above and derives every speaker model from it by MAP adaptation of the means (gmm_train.map_adapt, ``relevance_factor``) instead of
    the per-speaker fits.  ``top_c`` (None: dense scoring, unchanged): an int scores through the top-C scorer (score_matrix; needs
    mean-adapted models).  ``covariance_type``: 'diag' (the reference's) or 'full' — passed to every fit; 'full' speaker models are
    fitted one after the other and cannot be combined with adapt='map' or top_c.
    Prints and returns the train/test accuracies the reference prints; the models are left in ``GMM.last_model``."""
    if model is True:
        model = load_models(model_dir or "Model")
    elif not model:
        speakers = sorted(train.keys())
        D = np.asarray(train[speakers[0]]).shape[1] if speakers else 0
        if adapt not in (None, 'map'):
            raise ValueError("adapt must be None or 'map'")
        if covariance_type != 'diag' and (adapt is not None or top_c is not None):
            raise ValueError("adapt and top_c need covariance_type='diag'")
        if adapt == 'map':
            gmms = None  # (from the UBM, below)
        elif covariance_type != 'diag':
            gmms = fit_many([train[s] for s in speakers], n_components=n_components, covariance_type=covariance_type, random_state=random_state,
                            seeding=seeding)
        elif n_components <= 64 and D <= 47:  # one EM launch per iteration for all speakers; the same bits as the loop below
            gmms = fit_many([train[s] for s in speakers], n_components=n_components, covariance_type='diag', random_state=random_state, seeding=seeding)
        else:
            gmms = [GaussianMixture(n_components=n_components, covariance_type='diag', random_state=random_state, seeding=seeding).fit(train[s])
                    for s in speakers]
        ubm_train = np.vstack([train[s] for s in speakers])
        ubm = GaussianMixture(n_components=n_components, covariance_type=covariance_type, random_state=random_state, seeding=seeding).fit(ubm_train)
        if adapt == 'map':
            gmms = map_adapt(ubm, [train[s] for s in speakers], relevance_factor=relevance_factor, adapt='m')
        model = (gmms, ubm)
        if model_dir:
            save_models(gmms, ubm, model_dir)
    gmms, ubm = model
    GMM.last_model = model
    kw = {} if top_c is None else {"top_c": top_c}
    valid = score_matrix(gmms, ubm, x_train, **kw)[1]
    acc_train = (valid == np.array(y_train)).sum() / len(x_train)
    pred = score_matrix(gmms, ubm, x_test, **kw)[1]
    acc = (pred == np.array(y_test)).sum() / len(x_test)
    print("train acc {:.2%}, test acc {:.2%}".format(acc_train, acc))
    return acc_train, acc
