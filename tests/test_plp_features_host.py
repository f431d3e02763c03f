"""Host-side tests of the PLP feature recipes (no GPU): the C-ABI surface of ssp_plp_features, the column layout, the language read-out's
arithmetic (UI/tmp.py:344-357) and the NameError of an unknown feature type."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plp_features_is_declared_and_bound():
    from speech_signal_processing_amd import _lib
    header = open(os.path.join(ROOT, "include", "ssp.h")).read()
    m = re.search(r"^int\s+ssp_plp_features\s*\(([^;]*)\)\s*;", header, flags=re.M)
    assert m, "ssp_plp_features is not declared in include/ssp.h"
    params = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
    res, args = _lib.SIGNATURES["ssp_plp_features"]
    assert len(params) == len(args) == 16, (params, len(args))
    assert hasattr(_lib.load(), "ssp_plp_features")
    for cite in ("GMM_UBM.py:94-99", "UI/tmp.py:309-324", "UI/GMM_UBM_GUI.py:85-100"):
        assert cite in header, cite


@pytest.mark.parametrize("order,left_dim,delta_order", [(13, 0, 0), (13, 26, 1), (13, 13, 0), (9, 6, 2), (13, 39, 2)])
def test_column_layout_is_a_plain_interleave(order, left_dim, delta_order):
    from speech_signal_processing_amd import api
    nblk = 1 + delta_order
    lw = left_dim // nblk
    left = np.arange(5 * left_dim, dtype=np.float64).reshape(5, left_dim) + 1000.0
    plp = -np.arange(5 * nblk * order, dtype=np.float64).reshape(5, nblk * order) - 1.0
    rows = np.hstack([np.hstack((left[:, b * lw:(b + 1) * lw], plp[:, b * order:(b + 1) * order])) for b in range(nblk)])
    lc, pc = api.plp_feature_columns(order, left_dim, delta_order)
    assert sorted(np.concatenate((lc, pc))) == list(range(rows.shape[1]))
    assert np.array_equal(rows[:, lc], left) and np.array_equal(rows[:, pc], plp)


def test_column_layout_rejects_an_indivisible_left_block():
    from speech_signal_processing_amd import api
    with pytest.raises(ValueError):
        api.plp_feature_columns(13, 25, 1)


def test_language_readout_on_a_hand_made_matrix():
    from speech_signal_processing_amd import GMM_UBM
    pred = np.array([[0.0, -1.0, -2.0], [-3.0, 0.5, 0.25], [-1.0, -1.0, 4.0], [2.0, 2.0, 2.0]])
    names, prob = GMM_UBM.language_readout(pred)
    assert names == ['Chinese', 'English', 'Japanese', 'Chinese']   # (a tie goes to the first index, as argmax has it)
    e = np.exp(pred)
    np.testing.assert_allclose(prob, e.max(axis=1) / e.sum(axis=1), rtol=1e-15)
    assert abs(prob[3] - 1.0 / 3.0) < 1e-15
    # four models: every index past 1 reads as the third name (the reference's if / elif / else)
    names, prob = GMM_UBM.language_readout(np.array([[0.0, 0.0, 0.0, 1.0]]), names=('a', 'b', 'c'))
    assert names == ['c'] and abs(prob[0] - np.e / (3.0 + np.e)) < 1e-15
    with pytest.raises(ValueError):
        GMM_UBM.language_readout(np.zeros(3))


def test_unknown_feature_type_raises_before_any_gpu_work():
    from speech_signal_processing_amd import GMM_UBM
    with pytest.raises(NameError):
        GMM_UBM.extract_feature([np.zeros(16000, dtype=np.int16)], [0], feature_type='nope')
    with pytest.raises(NameError):
        GMM_UBM.chunk_features(np.zeros(16000, dtype=np.int16), 'nope')
