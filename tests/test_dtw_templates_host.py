"""Batched DTW templates without a GPU: the argument checks of api.dtw_templates / MFCC_DTW.generate_templates run before a context is
needed, a valid call fails loudly where there is no device, and the entry point is declared and bound."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("groups", [
    [[np.zeros(5), np.ones(7)], []],                      # an empty group
    [[np.zeros(5), np.zeros(0)]],                         # an empty sample
    [[np.zeros((5, 0))]],                                 # ... of rows without values
    [[np.zeros(5), np.ones((7, 1))]],                     # 1-D and 2-D samples mixed
    [[np.zeros((5, 3))], [np.ones((7, 3)), np.ones((4, 2))]],   # mixed dim, across groups
    [[np.zeros(5), np.array([0.0, np.nan, 1.0])]],        # a NaN
    [[np.zeros(5)], [np.array([np.inf])]],                # an infinity
], ids=["empty-group", "empty-sample", "zero-dim", "mixed-ndim", "mixed-dim", "nan", "inf"])
def test_argument_checks_need_no_gpu(groups):
    from speech_signal_processing_amd import MFCC_DTW, api
    with pytest.raises(ValueError):
        MFCC_DTW.generate_templates(groups)
    with pytest.raises(ValueError):
        api.dtw_templates(None, groups)


def test_no_groups_no_templates():
    from speech_signal_processing_amd import MFCC_DTW, api
    assert MFCC_DTW.generate_templates([]) == []
    assert api.dtw_templates(None, []) == []
    with pytest.raises(ValueError):
        MFCC_DTW.generate_templates([[np.zeros(3)]], workspace_bytes=-1)


def test_direction_bytes_pad_rows_to_dwords():
    from speech_signal_processing_amd import api
    assert [api._dtw_direction_bytes(r, c) for r, c in ((1, 1), (3, 4), (700, 1100), (2, 1222))] == [4, 12, 770000, 2448]


def test_valid_call_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from speech_signal_processing_amd import MFCC_DTW, _lib
    with pytest.raises(_lib.SspError):
        MFCC_DTW.generate_templates([[np.zeros(5), np.ones(7)], [np.ones(3)]])


def test_entry_point_is_declared_and_bound():
    from speech_signal_processing_amd import _lib
    header = open(os.path.join(ROOT, "include", "ssp.h")).read()
    assert re.search(r"^int\s+ssp_dtw_templates\s*\(", header, flags=re.M)
    assert "ssp_dtw_templates" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ssp_dtw_templates"][1]) == 11
    assert hasattr(_lib.load(), "ssp_dtw_templates")
    assert _lib.load().ssp_abi_version() == 4
