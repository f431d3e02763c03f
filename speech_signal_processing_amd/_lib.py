"""ctypes binding of include/ssp.h (libsspgpu.so).  Fails loudly when the library is absent."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SSP_LIB_PATH") or os.path.join(HERE, "libsspgpu.so")  # override: diagnostic builds only

SSP_OK, SSP_ERR_INVALID, SSP_ERR_UNSUPPORTED, SSP_ERR_HIP, SSP_ERR_NOMEM, SSP_ERR_NODEVICE = 0, -1, -2, -3, -4, -5
HOST, DEVICE = 0, 1
ABI_VERSION = 4
COMM_ID_BYTES = 128
VAD_ZCR_UNGATED = 1
PLDA_NO_CLASS_PATH = 1
FEATNORM_TILE = 256          # SSP_FEATNORM_TILE: frames of one utterance a workgroup of the sliding-normalisation kernel takes
FEATNORM_MAX_WINDOW = 1024
VBHMM_LDS_BYTES = 155648         # SSP_VBHMM_LDS_BYTES: LDS a workgroup of the VB-HMM kernel has for alpha and its two T x SP buffers
VBHMM_ALPHA_LDS_BYTES = 65536    # SSP_VBHMM_ALPHA_LDS_BYTES: alpha sits in LDS up to this many bytes


class SspError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libsspgpu error %d: %s" % (code, msg))
        self.code = code


class ssp_mfcc_cfg(C.Structure):
    _fields_ = [
        ("sample_rate", C.c_int32), ("win_len", C.c_int32), ("hop", C.c_int32), ("n_fft", C.c_int32),
        ("n_filt", C.c_int32), ("n_ceps", C.c_int32), ("frame_mode", C.c_int32), ("preemph_mode", C.c_int32),
        ("preemph", C.c_float), ("spec_power", C.c_int32), ("spec_scale", C.c_float), ("log_mode", C.c_int32),
        ("floor_mode", C.c_int32), ("eps", C.c_float), ("top_db", C.c_float), ("delta_order", C.c_int32),
        ("delta_N", C.c_int32), ("cmvn", C.c_int32),
    ]


_P = C.c_void_p
_I64P = C.POINTER(C.c_int64)
_F32P = C.c_void_p   # bulk arrays are passed as raw addresses (host or device)
_MSP = C.POINTER(C.c_float)

# name -> (restype, argtypes); every symbol declared in include/ssp.h
SIGNATURES = {
    "ssp_abi_version": (C.c_int, []),
    "ssp_last_error": (C.c_char_p, []),
    "ssp_ctx_create": (C.c_int, [C.c_int, _P, C.c_int, C.POINTER(_P)]),
    "ssp_ctx_destroy": (C.c_int, [_P]),
    "ssp_debug_poison_lds": (C.c_int, [_P, C.c_uint32]),
    "ssp_ctx_sync": (C.c_int, [_P]),
    "ssp_calibrate": (C.c_int, [_P, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ssp_ctx_wait_stream": (C.c_int, [_P, _P]),
    "ssp_ctx_signal_stream": (C.c_int, [_P, _P]),
    "ssp_comm_unique_id": (C.c_int, [_P]),
    "ssp_comm_init": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "ssp_comm_destroy": (C.c_int, [_P]),
    "ssp_comm_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ssp_allgather": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "ssp_allreduce_sum": (C.c_int, [_P, _P, C.c_size_t, C.c_int]),
    "ssp_segments_create": (C.c_int, [_P, _I64P, C.c_int64, C.POINTER(_P)]),
    "ssp_segments_destroy": (C.c_int, [_P]),
    "ssp_segments_count": (C.c_int, [_P, _I64P, _I64P]),
    "ssp_segments_read": (C.c_int, [_P, _I64P]),
    "ssp_mfcc_plan_create": (C.c_int, [_P, C.POINTER(ssp_mfcc_cfg), _F32P, _F32P, _F32P, C.POINTER(_P)]),
    "ssp_mfcc_plan_destroy": (C.c_int, [_P]),
    "ssp_mfcc_plan_set_flags": (C.c_int, [_P, C.c_uint32]),
    "ssp_mfcc_num_frames": (C.c_int, [C.POINTER(ssp_mfcc_cfg), C.c_int64, _I64P]),
    "ssp_mfcc_out_dim": (C.c_int, [C.POINTER(ssp_mfcc_cfg), C.POINTER(C.c_int32)]),
    "ssp_mfcc_frame_segments": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "ssp_mfcc_run": (C.c_int, [_P, _P, _P, _F32P, _F32P, C.c_int, C.c_int, _MSP]),
    "ssp_mfcc_run_i16": (C.c_int, [_P, _P, _P, _F32P, _F32P, C.c_int, C.c_int, _MSP]),
    "ssp_mfcc_run_list": (C.c_int, [_P, _P, _P, _P, C.c_int, _F32P, C.c_int, C.c_int, _MSP]),
    "ssp_vad_num_frames": (C.c_int, [C.c_int64, C.c_int32, _I64P]),
    "ssp_vad_frame_segments": (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P)]),
    "ssp_vad_features": (C.c_int, [_P, _F32P, C.c_int, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, _F32P, _F32P, _F32P, C.c_int, _MSP]),
    "ssp_vad_detect": (C.c_int, [_P, _F32P, _F32P, _P, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_int32, _P, _P, C.c_int, _MSP]),
    "ssp_vad_sweep": (C.c_int, [_P, _F32P, _F32P, _P, _P, C.c_int32, C.c_int32, _F32P, _F32P, _F32P, C.c_int32, _P, C.c_int, _MSP]),
    "ssp_enframe": (C.c_int, [_P, _F32P, C.c_int64, C.c_int32, C.c_int32, _F32P, _F32P, C.c_int, _MSP]),
    "ssp_cepstrum": (C.c_int, [_P, _F32P, C.c_int64, C.c_int32, _F32P, C.c_int32, _F32P, C.c_int32, C.c_int32, C.c_int32,
                               C.c_float, _F32P, C.c_int, _MSP]),
    "ssp_spectrum_abs": (C.c_int, [_P, _F32P, C.c_int64, C.c_int32, C.c_float, C.c_int32, _F32P, C.c_int, _MSP]),
    "ssp_delta": (C.c_int, [_P, _F32P, _P, C.c_int32, C.c_int32, _F32P, C.c_int, _MSP]),
    "ssp_cmvn": (C.c_int, [_P, _F32P, _P, C.c_int32, _F32P, C.c_int, _MSP]),
    "ssp_featnorm_sliding": (C.c_int, [_P, _F32P, _P, C.c_int32, C.c_int32, C.c_int32, _F32P, C.c_int, _MSP]),
    "ssp_select_frames": (C.c_int, [_P, _F32P, _P, C.c_int32, _P, _F32P, _I64P, C.c_int, _MSP]),
    "ssp_featnorm_table": (C.c_int, [C.c_int32, _F32P]),
    "ssp_plp_post": (C.c_int, [_P, _F32P, _P, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_float, _F32P, C.c_int, _MSP]),
    "ssp_plp_features": (C.c_int, [_P, _F32P, _P, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_float, _F32P, C.c_int32, C.c_int32, C.c_int32,
                                   _F32P, C.c_int, C.c_int, _MSP]),
    "ssp_gmm_pack": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.POINTER(_P)]),
    "ssp_gmm_destroy": (C.c_int, [_P]),
    "ssp_gmm_score": (C.c_int, [_P, _F32P, _P, _F32P, _F32P, _P, C.c_int, C.c_int, _MSP]),
    "ssp_gmm_score_list": (C.c_int, [_P, _P, C.c_int, C.c_int32, _P, _F32P, _P, C.c_int, _MSP]),
    "ssp_gmm_last_rescored": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "ssp_gmm_em_stats": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _F32P, C.c_int64, _P, _P, _P, _P, C.c_int, _MSP]),
    "ssp_gmm_em_stats_batch": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _F32P, C.c_int64, _P, _P, _P, _P, _P, _P,
                                         C.c_int, _MSP]),
    "ssp_gmm_em_stats_shared": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _F32P, C.c_int64, _P, _P, _P, _P, _P, _P,
                                          C.c_int, _MSP]),
    "ssp_gmm_full_em_stats": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, _F32P, C.c_int64, _P, _P, _P, _P, C.c_int, _MSP]),
    "ssp_gmm_full_pack": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.POINTER(_P)]),
    "ssp_gmm_full_destroy": (C.c_int, [_P]),
    "ssp_gmm_full_score": (C.c_int, [_P, _F32P, _P, _F32P, _F32P, _P, C.c_int, _MSP]),
    "ssp_gmm_map_pack": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, C.POINTER(_P)]),
    "ssp_gmm_map_destroy": (C.c_int, [_P]),
    "ssp_gmm_map_score": (C.c_int, [_P, _F32P, _P, C.c_int32, _F32P, _F32P, _P, _P, C.c_int, _MSP]),
    "ssp_gmm_map_score_list": (C.c_int, [_P, _P, C.c_int, C.c_int32, _P, C.c_int32, _F32P, _F32P, _P, _P, _MSP]),
    "ssp_ivector_create": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.POINTER(_P)]),
    "ssp_ivector_destroy": (C.c_int, [_P]),
    "ssp_ivector_set_t": (C.c_int, [_P, _P]),
    "ssp_ivector_set_workspace": (C.c_int, [_P, C.c_size_t]),
    "ssp_ivector_last_slab": (C.c_int, [_P, _I64P]),
    "ssp_ivector_last_stages": (C.c_int, [_P, _MSP]),
    "ssp_ivector_extract": (C.c_int, [_P, _P, _P, C.c_int64, _F32P, _F32P, _F32P, _MSP]),
    "ssp_ivector_estep": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, C.POINTER(C.c_double), _MSP]),
    "ssp_plda_stats": (C.c_int, [_P, _F32P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int, _MSP]),
    "ssp_plda_pack": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, C.POINTER(_P)]),
    "ssp_plda_destroy": (C.c_int, [_P]),
    "ssp_plda_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ssp_plda_score": (C.c_int, [_P, _F32P, C.c_int64, _F32P, _P, _F32P, C.c_int, _MSP]),
    "ssp_topn_stats": (C.c_int, [_P, _F32P, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _F32P, _F32P, _F32P, C.c_int, _MSP]),
    "ssp_snorm_apply": (C.c_int, [_P, _F32P, C.c_int64, C.c_int32, C.c_int64, _F32P, _F32P, _F32P, _F32P, C.c_float, _F32P, C.c_int64, _P, _F32P,
                                  C.c_int, _MSP]),
    "ssp_det_counts": (C.c_int, [_P, _F32P, C.c_int64, C.c_int32, C.c_int64, _P, _P, C.c_int32, _P, _P, _P, _P, C.c_int, _MSP]),
    "ssp_pairwise_size": (C.c_int, [_P, _I64P]),
    "ssp_pairwise_scores": (C.c_int, [_P, _F32P, _P, C.c_int32, _P, _P, C.c_float, _F32P, C.c_int, _MSP]),
    "ssp_ahc_cluster": (C.c_int, [_P, _F32P, _P, C.c_int32, C.c_float, C.c_int32, _P, _P, _P, _P, _F32P, C.c_int, _MSP]),
    "ssp_vbhmm_resegment": (C.c_int, [_P, _F32P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32,
                                      C.c_double, _P, _P, _P, _P, _P, _F32P, _F32P, _F32P, C.c_int, _MSP]),
    "ssp_kmeanspp_seed": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _F32P, C.c_int64, C.c_int, _P, _P, _P, _P, _P, _P, _P, _MSP]),
    "ssp_dense_forward": (C.c_int, [_P, _F32P, C.c_int64, C.c_int32, _F32P, _F32P, C.c_int32, C.c_int32, _F32P, C.c_int, _MSP]),
    "ssp_dnn_create": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(_P)]),
    "ssp_dnn_destroy": (C.c_int, [_P]),
    "ssp_dnn_forward": (C.c_int, [_P, _F32P, C.c_int64, _F32P, C.c_int, _MSP]),
    "ssp_lstm_create": (C.c_int, [_P, C.c_int32, C.c_int32, _F32P, _F32P, _F32P, C.c_int32, C.POINTER(_P)]),
    "ssp_lstm_destroy": (C.c_int, [_P]),
    "ssp_lstm_forward": (C.c_int, [_P, _F32P, _P, _F32P, C.c_int, _MSP]),
    "ssp_lstm_pack_weights": (C.c_int, [C.c_int32, C.c_int32, _F32P, _F32P, _F32P, _F32P, _I64P]),
    "ssp_gru_create": (C.c_int, [_P, C.c_int32, C.c_int32, _F32P, _F32P, _F32P, C.c_int32, C.c_int32, C.POINTER(_P)]),
    "ssp_gru_destroy": (C.c_int, [_P]),
    "ssp_gru_forward": (C.c_int, [_P, _F32P, C.c_int64, C.c_int32, _F32P, _F32P, C.c_int, _MSP]),
    "ssp_gru_set_workspace": (C.c_int, [_P, C.c_size_t]),
    "ssp_gru_last_slab": (C.c_int, [_P, _I64P]),
    "ssp_conv2d_same_forward": (C.c_int, [_P, _F32P, C.c_int64, C.c_int32, C.c_int32, _F32P, _F32P, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, _F32P, C.c_int, _MSP]),
    "ssp_l2_normalize": (C.c_int, [_P, _F32P, C.c_int64, C.c_int32, C.c_float, _F32P, C.c_int, _MSP]),
    "ssp_tdnn_forward": (C.c_int, [_P, _F32P, _P, C.c_int32, _F32P, _F32P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F32P, _F32P, _F32P, _I64P,
                                   C.c_int, _MSP]),
    "ssp_stats_pool": (C.c_int, [_P, _F32P, _P, C.c_int32, _I64P, C.c_int64, C.c_double, _F32P, C.c_int, _MSP]),
    "ssp_xvector_create": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                     C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_double, C.POINTER(_P)]),
    "ssp_xvector_destroy": (C.c_int, [_P]),
    "ssp_xvector_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ssp_xvector_set_workspace": (C.c_int, [_P, C.c_size_t]),
    "ssp_xvector_last_slab": (C.c_int, [_P, _I64P]),
    "ssp_xvector_forward": (C.c_int, [_P, _F32P, _P, _I64P, C.c_int64, _F32P, C.c_int, _MSP]),
    "ssp_dnn_trainer_create": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p), C.c_int32, C.POINTER(_P)]),
    "ssp_dnn_trainer_destroy": (C.c_int, [_P]),
    "ssp_dnn_trainer_epoch": (C.c_int, [_P, _F32P, _P, C.c_int64, _P, C.c_int32, C.c_float, C.c_uint64, C.POINTER(C.c_double), _I64P, C.c_int, _MSP]),
    "ssp_dnn_trainer_evaluate": (C.c_int, [_P, _F32P, _P, C.c_int64, C.POINTER(C.c_double), _I64P, C.c_int, _MSP]),
    "ssp_dnn_trainer_read": (C.c_int, [_P, C.c_int32, C.c_int32, _F32P]),
    "ssp_dnn_trainer_steps": (C.c_int, [_P, _I64P]),
    "ssp_lstm_trainer_create": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F32P, _F32P, _F32P, _F32P, _F32P, C.c_int32,
                                          C.POINTER(_P)]),
    "ssp_lstm_trainer_destroy": (C.c_int, [_P]),
    "ssp_lstm_trainer_epoch": (C.c_int, [_P, _F32P, _P, C.c_int64, _P, C.c_int32, C.c_float, C.POINTER(C.c_double), _I64P, C.c_int, _MSP]),
    "ssp_lstm_trainer_evaluate": (C.c_int, [_P, _F32P, _P, C.c_int64, C.POINTER(C.c_double), _I64P, C.c_int, _MSP]),
    "ssp_lstm_trainer_read": (C.c_int, [_P, C.c_int32, C.c_int32, _F32P]),
    "ssp_lstm_trainer_steps": (C.c_int, [_P, _I64P]),
    "ssp_lstm_trainer_step_times": (C.c_int, [_P, _F32P, _P, C.c_int32, C.c_float, _MSP]),
    "ssp_gru_trainer_create": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F32P, _F32P, C.c_int32,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int32, _F32P,
                                         _F32P, C.c_int32, _F32P, _F32P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    "ssp_gru_trainer_destroy": (C.c_int, [_P]),
    "ssp_gru_trainer_epoch": (C.c_int, [_P, _F32P, _P, C.c_int64, _P, C.c_int32, C.c_float, C.POINTER(C.c_double), _I64P, C.c_int, _MSP]),
    "ssp_gru_trainer_evaluate": (C.c_int, [_P, _F32P, _P, C.c_int64, C.POINTER(C.c_double), _I64P, C.c_int, _MSP]),
    "ssp_gru_trainer_read": (C.c_int, [_P, C.c_int32, C.c_int32, _F32P]),
    "ssp_gru_trainer_steps": (C.c_int, [_P, _I64P]),
    "ssp_gru_trainer_step_times": (C.c_int, [_P, _F32P, _P, C.c_int32, C.c_float, _MSP]),
    "ssp_dropout_keep": (C.c_int, [C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_float, _P]),
    "ssp_dtw_distances": (C.c_int, [_P, _F32P, _P, _F32P, _P, C.c_int32, C.c_int32, _F32P, C.c_int, _MSP]),
    "ssp_fastdtw_distances": (C.c_int, [_P, _F32P, _P, _F32P, _P, C.c_int32, C.c_void_p, _MSP]),
    "ssp_dtw_path": (C.c_int, [_P, _F32P, C.c_int64, _F32P, C.c_int64, C.c_int32, _P, _P, _P, _P]),
    "ssp_dtw_templates": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int64, _P, _P, _MSP]),
    "ssp_centroids": (C.c_int, [_P, _F32P, _P, C.c_int64, C.c_int32, C.c_int32, _F32P, C.c_int, _MSP]),
    "ssp_cosine_identify": (C.c_int, [_P, _F32P, C.c_int64, C.c_int32, _F32P, C.c_int32, _F32P, _P, _F32P, C.c_int, _MSP]),
    "ssp_cosine_identify2": (C.c_int, [_P, _F32P, C.c_int64, C.c_int32, _F32P, C.c_int32, _F32P, _P, _F32P, C.c_int, C.c_int, _MSP]),
    "ssp_cosine_last_auto": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ssp_gmm_last_auto": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "ssp_cosine_last_rescored": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "ssp_cosine_last_split_rows": (C.c_int, [_P, C.POINTER(C.c_int32)]),
}

_lib = None


def load():
    """Load libsspgpu.so and bind every symbol.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libsspgpu.so is missing (%s). Build it with `python -m speech_signal_processing_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    # ONE HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64 and whichever
    # copy initialises first owns the device, the other then reports "no ROCm-capable device".  Importing torch first
    # makes the dynamic loader resolve libsspgpu.so's NEEDED libamdhip64.so.7 (same SONAME) to torch's copy.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    # the ABI first: an older or variant library (SSP_LIB_PATH) gets the rebuild message, not a bare AttributeError on a newer symbol
    lib.ssp_abi_version.restype = C.c_int
    lib.ssp_abi_version.argtypes = []
    if lib.ssp_abi_version() != ABI_VERSION:
        raise ImportError("libsspgpu.so ABI version %d != %d (rebuild: python -m speech_signal_processing_amd.build)" % (lib.ssp_abi_version(), ABI_VERSION))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc == SSP_OK:
        return
    msg = load().ssp_last_error().decode("utf-8", "replace")
    if rc == SSP_ERR_INVALID:
        raise ValueError(msg)
    if rc == SSP_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise SspError(rc, msg)
