"""GPU-backed stand-ins for the two sidekit feature functions the reference imports into GMM_UBM.py / d_vector.py / the GUIs
(``from sidekit.frontend.features import plp, mfcc``, GMM_UBM.py:20, d_vector.py:18).  Same call shape, same return value: a list
whose first item is the (frames, 13) cepstra - the only item the reference uses.  sidekit's source is absent from the reference
tree; both follow its published algorithms (parity unpinned, see oracle/ref_cpu.py)."""
from __future__ import annotations

import functools

import numpy as np

from . import api, frontend


@functools.lru_cache(maxsize=8)
def _mfcc_plan(fs, nwin, shift, nceps, prefac):
    return api.MfccPlan(api.default_context(), frontend.preset_sidekit(fs=fs, nwin=nwin, shift=shift, nceps=nceps, prefac=prefac))


@functools.lru_cache(maxsize=8)
def _plp_plan(fs, nwin, shift, prefac):
    return api.MfccPlan(api.default_context(), frontend.preset_sidekit_plp(fs=fs, nwin=nwin, shift=shift, prefac=prefac))


def mfcc(input_sig, fs=16000, nwin=0.025, shift=0.01, nceps=13, prefac=0.97):
    """sidekit mfcc at the reference's call sites (GMM_UBM.py:89, d_vector.py:91): [cepstra (T, nceps), None, None, None]."""
    plan = _mfcc_plan(int(fs), float(nwin), float(shift), int(nceps), float(prefac))
    x, lens = api.flatten_signals([input_sig])
    seg = api.Segments.from_lengths(plan.ctx, lens)
    return [np.asarray(plan.run(x, seg), dtype=np.float64), None, None, None]


def plp_batch(signals, fs=16000, nwin=0.025, shift=0.01, plp_order=13, prefac=0.97, rasta=True):
    """PLP cepstra of a list of utterances in two launches: -> (feats (sum T_i, plp_order) float32 array, frame Segments)."""
    plan = _plp_plan(int(fs), float(nwin), float(shift), float(prefac))
    flat, lens = api.flatten_signals(signals)
    seg = api.Segments.from_lengths(plan.ctx, lens)
    fseg = plan.frame_segments(seg)
    logspec = plan.run(flat, seg, fseg)
    return api.plp_post(plan.ctx, logspec, fseg, fs / 2.0, plp_order, rasta), fseg


@functools.lru_cache(maxsize=8)
def _mfcc_recipe_plan(fs, nwin, shift, nceps, prefac, delta_order, cmvn):
    return api.MfccPlan(api.default_context(), frontend.preset_sidekit(fs=fs, nwin=nwin, shift=shift, nceps=nceps, prefac=prefac,
                                                                       delta_order=delta_order, cmvn=cmvn))


def _upload(flat):
    """the flat sample array on the default context's device, in one copy (int16 PCM stays int16)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(flat)).to("cuda:%d" % api.default_context().device)


def mfcc_batch(signals, fs=16000, nwin=0.025, shift=0.01, nceps=13, prefac=0.97, delta_order=0, scale=False, out_dtype=np.float64):
    """sidekit MFCC cepstra of a list of utterances in one launch (the chunk loop of UI/tmp.py:309-313 as a batch), with the recipe's
    delta blocks and per-utterance scale when asked for: -> (feats (sum T_i, (1 + delta_order) nceps) array, frame Segments)."""
    plan = _mfcc_recipe_plan(int(fs), float(nwin), float(shift), int(nceps), float(prefac), int(delta_order), int(bool(scale)))
    flat, lens = api.flatten_signals(signals)
    seg = api.Segments.from_lengths(plan.ctx, lens)
    fseg = plan.frame_segments(seg)
    return np.asarray(plan.run(flat, seg, fseg), dtype=out_dtype), fseg


def plp_features_batch(signals, fs=16000, nwin=0.025, shift=0.01, plp_order=13, prefac=0.97, rasta=True, with_mfcc=False, nceps=13,
                       delta_order=0, scale=False, out_dtype=np.float64):
    """The PLP and MFCC+PLP feature recipes of a list of utterances (GMM_UBM.py:94-99, UI/tmp.py:314-324): the samples go to the device
    once, the PLP front end (and, ``with_mfcc``, the sidekit MFCC plan with cmvn = scale and the same delta_order) runs on them there,
    api.plp_features makes the final rows on the device and one copy brings them back.  Rows are [plp | d plp ...], with_mfcc
    [mfcc | plp | d mfcc | d plp ...].  -> (feats (sum T_i, D) array of out_dtype, frame Segments)."""
    out_dtype = np.dtype(out_dtype)
    plan = _plp_plan(int(fs), float(nwin), float(shift), float(prefac))
    flat, lens = api.flatten_signals(signals)
    seg = api.Segments.from_lengths(plan.ctx, lens)
    fseg = plan.frame_segments(seg)
    D = (1 + int(delta_order)) * (int(plp_order) + (int(nceps) if with_mfcc else 0))
    if fseg.total == 0:
        return np.zeros((0, D), dtype=out_dtype), fseg
    dev = _upload(flat)
    logspec = plan.run(dev, seg, fseg)
    left = None
    if with_mfcc:
        mplan = _mfcc_recipe_plan(int(fs), float(nwin), float(shift), int(nceps), float(prefac), int(delta_order), int(bool(scale)))
        mfseg = mplan.frame_segments(seg)
        assert np.array_equal(mfseg.offsets, fseg.offsets), "the MFCC and PLP plans cut different frames"
        left = mplan.run(dev, seg, mfseg)
    feats = api.plp_features(plan.ctx, logspec, fseg, fs / 2.0, plp_order, rasta, left=left, delta_order=delta_order, scale=scale,
                             out_dtype=out_dtype)
    return feats.cpu().numpy(), fseg


def cep_sliding_norm(features, win=301, center=True, reduce=False):
    """sidekit's cep_sliding_norm by name: mean (``reduce``: and variance) normalisation of a (T, D) array over a window of ``win``
    frames centred on each frame — featnorm.cmvn_sliding (recalled, parity unpinned).  The causal form (center=False) is not provided."""
    if not center:
        raise NotImplementedError("cep_sliding_norm: center=False (the causal window) is not provided")
    from . import featnorm
    return featnorm.cmvn_sliding(features, window=int(win), norm_vars=bool(reduce))


def stg(features, win=301):
    """sidekit's stg (short-term gaussianisation) by name: feature warping of a (T, D) array over a window of ``win`` frames —
    featnorm.feature_warp (recalled, parity unpinned)."""
    from . import featnorm
    return featnorm.feature_warp(features, window=int(win))


def plp(input_sig, nwin=0.025, fs=16000, plp_order=13, shift=0.01, get_spec=False, get_mspec=False, prefac=0.97, rasta=True):
    """sidekit plp (call sites GMM_UBM.py:95, d_vector.py:93, UI/GMM_UBM_GUI.py:93): [cepstra (T, plp_order), None, None, None].
    (log-energy / spectra, items 1-3 of sidekit's list, are not used by the reference and not computed.)"""
    if get_spec or get_mspec:
        raise NotImplementedError("plp: get_spec / get_mspec are not used by the reference and not provided")
    feats, _ = plp_batch([input_sig], fs, nwin, shift, plp_order, prefac, rasta)
    return [np.asarray(feats, dtype=np.float64), None, None, None]
