"""ctypes binding of libneuroir_hip.so (the C-ABI declared in include/neuroir_hip.h).

There is NO CPU fallback: if the shared library is missing or a tensor is not on a ROCm device the
call raises RuntimeError (mirrors how the reference surfaces torch errors).
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libneuroir_hip.so")

c_fp = C.c_void_p      # const float*   (device)
c_ip = C.c_void_p      # const int64_t* (device)
c_st = C.c_void_p      # hipStream_t


def _struct(name, float_fields, int_fields=()):
    fields = [(f, c_fp) for f in float_fields] + [(f, C.c_int) for f in int_fields]
    return type(name, (C.Structure,), {"_fields_": fields})


DrmmWeights = _struct("nir_drmm_weights",
                      ["gate_w", "gate_b", "ffnn0_w", "ffnn0_b", "ffnn1_w", "ffnn1_b", "out_w", "out_b"], ["snap_one"])
DrmmWeights = type("nir_drmm_weights", (C.Structure,), {"_fields_": list(DrmmWeights._fields_) + [("self_bin", C.c_void_p)]})
MatchTensorWeights = _struct(
    "nir_matchtensor_weights",
    ["proj_w", "proj_b", "q_wih", "q_whh", "q_bih", "q_bhh", "d_wih", "d_whh", "d_bih", "d_bhh",
     "qproj_w", "qproj_b", "dproj_w", "dproj_b", "alpha", "conv1_w", "conv1_b", "conv2_w", "conv2_b",
     "conv3_w", "conv3_b", "conv_w", "conv_b", "out_w", "out_b"],
    ["F", "Hq", "Hd", "C", "NF", "MF", "bounded"])
MatchTensorWeights = type("nir_matchtensor_weights", (C.Structure,), {"_fields_": list(MatchTensorWeights._fields_) + [("dproj_frag", C.c_void_p)]})
DuetWeights = _struct(
    "nir_duet_weights",
    ["l_conv_w", "l_conv_b", "l_fc1_w", "l_fc1_b", "l_fc2_w", "l_fc2_b", "l_fc3_w", "l_fc3_b",
     "convq_w", "convq_b", "convd1_w", "convd1_b", "convd2_w", "convd2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b",
     "fc3_w", "fc3_b", "fc4_w", "fc4_b"],
    ["NF", "pool", "bounded"])
DuetWeights = type("nir_duet_weights", (C.Structure,), {"_fields_": list(DuetWeights._fields_) + [
    (f, C.c_void_p) for f in ("table_h1", "table_h2", "convd1_h1", "convd1_h2", "convd2_h1", "convd2_h2")] + [("EP", C.c_int)] + [
    ("fw1", C.c_void_p), ("fw2", C.c_void_p), ("K1P", C.c_int), ("ftable", C.c_void_p), ("fw1c", C.c_void_p), ("EPT", C.c_int)]})
DssmWeights = _struct("nir_dssm_weights", ["q_w1t", "q_b1", "q_w2t", "q_b2", "d_w1t", "d_b1", "d_w2t", "d_b2"], ["NH", "NO"])
CdssmWeights = _struct("nir_cdssm_weights", ["q_w5t", "q_b", "q_semt", "q_semb", "d_w5t", "d_b", "d_semt", "d_semb"], ["NH", "NO"])
CONV1D_SPLIT, CONV1D_FP32, ARCI_MAX_LAYERS = 0, 1, 8


class Conv1dLayer(C.Structure):
    _fields_ = [("planes", C.c_void_p), ("wt", c_fp), ("bias", c_fp)] + [(f, C.c_int) for f in ("C_in", "F", "k", "p", "path")]


class ArciWeights(C.Structure):
    _fields_ = [("q", Conv1dLayer * ARCI_MAX_LAYERS), ("d", Conv1dLayer * ARCI_MAX_LAYERS), ("head_wq", c_fp), ("head_wd", c_fp), ("head_b", c_fp),
                ("n_layers", C.c_int), ("q_feats", C.c_int), ("d_feats", C.c_int)]


ARCII_MAX_LAYERS = 8


class Conv2dLayer(C.Structure):
    _fields_ = [("planes", C.c_void_p), ("wt", c_fp), ("bias", c_fp)] + [(f, C.c_int) for f in ("C_in", "F", "kh", "kw", "ph", "pw", "path")]


class ArciiWeights(C.Structure):
    _fields_ = [("q", Conv1dLayer), ("d", Conv1dLayer), ("l", Conv2dLayer * ARCII_MAX_LAYERS), ("head_w", c_fp), ("head_b", c_fp),
                ("n_layers", C.c_int), ("feats", C.c_int)]


CarsEncoderWeights = _struct(
    "nir_cars_encoder_weights",
    ["wih", "whh", "bih", "bhh", "attn0_w", "attn0_b", "attn3_w", "attn3_b"], ["H", "bounded"])
CarsEncoderWeights = type("nir_cars_encoder_weights", (C.Structure,), {"_fields_": list(CarsEncoderWeights._fields_) + [("attn_frag", C.c_void_p),
                                                                                                   ("whh_frag", C.c_void_p)]})
CarsSessionWeights = _struct(
    "nir_cars_session_weights",
    ["click0_w", "click0_b", "click3_w", "click3_b", "sq_attn_w", "sq_attn_b", "sd_attn_w", "sd_attn_b",
     "sq_wih", "sq_whh", "sq_bih", "sq_bhh", "sd_wih", "sd_whh", "sd_bih", "sd_bhh", "qproj_w", "qproj_b",
     "shared_w", "priv1_w", "mo0_w", "mo0_b", "mo1_w", "mo1_b", "mo2_w", "mo2_b", "wrank", "attn_ut",
     "sq_inner0_w", "sq_inner0_b", "sq_inner3_w", "sq_inner3_b", "sd_inner0_w", "sd_inner0_b", "sd_inner3_w", "sd_inner3_b",
     "th_w", "th_b", "tc_w", "tc_b"],
    ["D", "HS", "HDEC", "q_on", "d_on", "rank_on", "rank_bounded"])
CarsSessionWeights = type("nir_cars_session_weights", (C.Structure,), {"_fields_": list(CarsSessionWeights._fields_) + [("sq_whh_frag", C.c_void_p),
                                                                                                   ("sd_whh_frag", C.c_void_p)]})
class CarsDecoderWeights(C.Structure):
    _fields_ = [(f, c_fp) for f in ("rnn_wih", "rnn_whh", "rnn_bih", "rnn_bhh", "attn_in_w", "attn_out_w", "dec_attn_w", "pred1_w",
                                    "pred2_w", "sess_w")] + [(f, C.c_int) for f in ("HD", "DQ", "P", "KS")] + [("VT", C.c_int64), ("pred2_frag", C.c_void_p), ("rnn_gate_fold", C.c_void_p),
                                                                                                           ("rnn_whh_frag", C.c_void_p), ("attn_q_w", C.c_void_p)]


S2S_ATTN = {"general": 0, "dot": 1, "mlp": 2}


class Seq2seqDecoderWeights(C.Structure):
    _fields_ = [(f, c_fp) for f in ("rnn_wih", "rnn_whh", "rnn_bih", "rnn_bhh", "attn_in_wt", "attn_ctx_w", "attn_query_w", "attn_query_b", "attn_v",
                                    "attn_out_w", "attn_out_b", "gen_w", "gen_b")] + [("H", C.c_int), ("attn_type", C.c_int), ("VT", C.c_int64),
                                                                                     ("rnn_gate_fold", C.c_void_p), ("rnn_whh_frag", C.c_void_p),
                                                                                     ("gen_frag", C.c_void_p)]


class AcgCopyWeights(C.Structure):
    _fields_ = [("copy_w", c_fp), ("copy_b", c_fp), ("reuse_copy_attn", C.c_int)] + [(f, c_fp) for f in ("attn_in_wt", "attn_ctx_w", "attn_query_w",
                                                                                                    "attn_query_b", "attn_v")]


class HredqsDecoderWeights(C.Structure):
    _fields_ = [(f, c_fp) for f in ("rnn_wih", "rnn_whh", "rnn_bih", "rnn_bhh", "gen_w", "gen_b")] + [("H", C.c_int), ("VT", C.c_int64),
                                                                                                     ("rnn_gate_fold", C.c_void_p),
                                                                                                     ("rnn_whh_frag", C.c_void_p),
                                                                                                     ("gen_frag", C.c_void_p)]


CarsSessionOutputs = _struct("nir_cars_session_outputs", ["inner_q", "inner_d", "dec_h", "dec_c"])

MnsrfWeights = _struct(
    "nir_mnsrf_weights",
    ["q_wih", "q_whh", "q_bih", "q_bhh", "d_wih", "d_whh", "d_bih", "d_bhh", "s_wih", "s_whh", "s_bih", "s_bhh",
     "proj_w", "proj_b"], ["Hq", "Hd", "HS"])
MnsrfWeights = type("nir_mnsrf_weights", (C.Structure,), {"_fields_": list(MnsrfWeights._fields_) + [
    ("q_fold", C.c_void_p), ("d_fold", C.c_void_p), ("q_whh_frag", C.c_void_p), ("d_whh_frag", C.c_void_p), ("s_whh_frag", C.c_void_p), ("err", C.c_void_p)]})

_i, _l, _z = C.c_int, C.c_int64, C.c_size_t
# name -> (restype, argtypes); must list EVERY symbol include/neuroir_hip.h declares (tests check this)
SIGNATURES = {
    "nir_version": (_i, []),
    "nir_last_error_string": (C.c_char_p, []),
    "nir_debug_clock_probe": (_i, [C.c_void_p, _i, _i, C.c_void_p, c_st]),
    "nir_debug_set_buffer": (_i, [C.c_void_p]),
    "nir_set_stream_batches_in_flight": (_i, [c_st, _i]),
    "nir_debug_set_tunable": (_i, [C.c_char_p, _i]),
    "nir_profile_enable": (_i, [_i]),
    "nir_profile_report": (_i, [C.c_char_p, _z]),
    "nir_split_f16x2": (_i, [c_fp, _l, _i, _l, _i, C.c_void_p, C.c_void_p, c_st]),
    "nir_linear_planes_f32": (_i, [C.c_void_p, C.c_void_p, _l, c_ip, _l, _l, _i, _i, C.c_void_p, C.c_void_p, _l, c_fp, c_fp, _l, _l, _i, _i, _i, c_st]),
    "nir_sanitize_ids": (_i, [c_ip, _l, c_ip, _l, _l, c_ip, c_ip, C.c_void_p, c_st]),
    "nir_flag_publish": (_i, [C.c_void_p, C.c_void_p, c_st]),
    "nir_gather_fields": (_i, [C.c_void_p, _i, C.c_void_p, _l, c_st]),
    "nir_host_device_pointer": (_i, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "nir_softmax_rows_publish": (_i, [c_fp, c_fp, _l, _i, C.c_void_p, C.c_void_p, c_st]),
    "nir_host_rank_metric": (C.c_double, [_i, C.c_void_p, C.c_void_p, _i, _l, _i, _i]),
    "nir_widen_ids_i32": (_i, [C.c_void_p, C.c_void_p, _l, c_st]),
    "nir_linear_f32": (_i, [c_fp, _l, c_ip, c_fp, _i, _l, _l, c_fp, _l, c_fp, c_fp, c_fp, _l, _l, _i, _i, _i, c_st]),
    "nir_linear_ex_f32": (_i, [c_fp, _l, c_ip, c_fp, _i, _l, _l, c_fp, _l, c_fp, c_fp, c_fp, _l, _l, _i, _i, _i, c_fp, _l, c_st]),
    "nir_linear_feats_f32": (_i, [c_fp, c_fp, _l, _i, _i, c_fp, _l, c_fp, c_fp, _l, _l, _i, _i, c_st]),
    "nir_debug_gemm3_launches": (_i, [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "nir_rowdot_f32": (_i, [c_fp, _l, c_fp, c_fp, c_fp, _l, _i, _i, c_st]),
    "nir_attn_pool_workspace_bytes": (_z, [_l, _i, _i]),
    "nir_attn_pool_f32": (_i, [C.c_void_p, _i, C.POINTER(CarsEncoderWeights), c_ip, _l, _i, _i, _i, C.c_void_p, _z, c_fp, c_st]),
    "nir_bilstm_fwd": (_i, [c_fp, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, _l, _i, _i, _i, c_st]),
    "nir_bilstm_supported": (_i, [_i]),
    "nir_bilstm_fused_fwd": (_i, [c_fp, _i, c_fp, c_fp, c_fp, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, _l, _i, _i, _i, c_st]),
    "nir_bilstm_steps_workspace_bytes": (_z, [_l, _i]),
    "nir_bilstm_steps_fwd": (_i, [c_fp, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, _l, _i, _i, _i, C.c_void_p, _z, c_st]),
    "nir_birnn_steps_fwd": (_i, [_i, c_fp, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, _l, _i, _i, _i, C.c_void_p, _z, c_st]),
    "nir_maxpool_time_f32": (_i, [c_fp, _l, _i, _i, c_fp, c_st]),
    "nir_lstm256_whh_frag_bytes": (_z, [_i]),
    "nir_lstm256_pack_whh_frag": (_i, [c_fp, _i, C.c_void_p, C.c_void_p, c_st]),
    "nir_lstm256_workspace_bytes": (_z, [_l, _i]),
    "nir_lstm256_rows_fwd": (_i, [c_fp, c_ip, c_ip, C.c_void_p, c_fp, _i, C.c_void_p, _l, _l, _i, _i, C.c_void_p, _z, c_st]),
    "nir_lstm256_train_fwd": (_i, [c_fp, c_ip, C.c_void_p, c_fp, c_fp, c_fp, C.c_void_p, _l, _i, _i, C.c_void_p, C.c_size_t, c_st]),
    "nir_lstm256_bptt_workspace_bytes": (_z, [_l, _i]),
    "nir_lstm256_bptt": (_i, [c_fp, c_fp, c_fp, c_ip, c_fp, c_fp, _l, _i, _i, C.c_void_p, C.c_size_t, c_st]),
    "nir_decode_greedy_plain_workspace_bytes": (_z, [_l, _i, _l]),
    "nir_decode_greedy_plain": (_i, [c_fp, c_fp, _l, _i, c_fp, _l, _i, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, _l, c_ip, _l, _i, C.c_void_p, _z, c_ip,
                                     c_st]),
    "nir_decode_greedy_plain_folded": (_i, [c_fp, c_fp, _l, _i, c_fp, _l, _i, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, _l, c_ip, _l, _i, c_fp, C.c_void_p,
                                            C.c_void_p, _z, c_ip, c_st]),
    "nir_mnsrf_workspace_bytes": (_z, [_l, _i, _i, _i, _i, C.POINTER(MnsrfWeights)]),
    "nir_mnsrf_encode": (_i, [c_ip, c_ip, _l, _i, _i, c_fp, _l, _i, C.POINTER(MnsrfWeights), C.c_void_p, _z, c_fp, c_fp, c_st]),
    "nir_mnsrf_encode_states": (_i, [c_ip, c_ip, _l, _i, _i, c_fp, _l, _i, C.POINTER(MnsrfWeights), C.c_void_p, _z, c_fp, c_fp, c_fp, c_fp, c_st]),
    "nir_mnsrf_rank": (_i, [c_fp, c_fp, c_ip, c_ip, _l, _i, _i, _i, c_fp, _l, _i, C.POINTER(MnsrfWeights), C.c_void_p, _z, c_fp, c_st]),
    "nir_mnsrf_score": (_i, [c_ip, c_ip, c_ip, c_ip, _l, _i, _i, _i, _i, c_fp, _l, _i, C.POINTER(MnsrfWeights), C.c_void_p, _z,
                            c_fp, c_st]),
    "nir_softmax_rows": (_i, [c_fp, c_fp, _l, _i, c_st]),
    "nir_softmax_gathered": (_i, [c_fp, c_fp, c_fp, _i, _l, _i, _i, c_st]),
    "nir_rank_loss_bce": (_i, [c_fp, c_fp, _l, _i, c_fp, c_st]),
    "nir_rank_loss_softmax_nll": (_i, [c_fp, c_fp, _l, _i, c_fp, c_st]),
    "nir_esm_score": (_i, [c_ip, c_ip, _i, _i, _i, _i, c_fp, _l, _i, c_fp, c_st]),
    "nir_drmm_score": (_i, [c_ip, c_ip, _i, _i, _i, _i, c_fp, _l, _i, C.POINTER(DrmmWeights), c_fp, c_fp, c_st]),
    "nir_matchtensor_workspace_bytes": (_z, [_i, _i, _i, _i, C.POINTER(MatchTensorWeights)]),
    "nir_matchtensor_score": (_i, [c_ip, c_ip, c_ip, c_ip, _i, _i, _i, _i, c_fp, _l, _i,
                                   C.POINTER(MatchTensorWeights), C.c_void_p, _z, c_fp, c_fp, c_fp, c_fp, c_fp, c_st]),
    "nir_matchtensor_score_encoded": (_i, [c_ip, c_ip, c_fp, c_fp, _i, _i, _i, _i, C.POINTER(MatchTensorWeights), C.c_void_p, _z, c_fp, c_fp, c_fp,
                                           c_st]),
    "nir_matchtensor_score_folded": (_i, [c_ip, c_ip, c_ip, c_ip, _i, _i, _i, _i, C.c_void_p, C.c_void_p, _i, _l,
                                          C.POINTER(MatchTensorWeights), C.c_void_p, _z, c_fp, c_fp, c_fp, c_fp, c_fp, C.c_void_p, c_st]),
    "nir_duet_workspace_bytes": (_z, [_i, _i, _i, _i, _i, C.POINTER(DuetWeights)]),
    "nir_duet_score": (_i, [c_ip, c_ip, _i, _i, _i, _i, c_fp, _l, _i, C.POINTER(DuetWeights), C.c_void_p, _z,
                            c_fp, c_fp, c_fp, c_st]),
    "nir_duet_document_workspace_bytes": (_z, [_i, _i, _i, _i, C.POINTER(DuetWeights)]),
    "nir_duet_document_branch": (_i, [c_ip, _i, _i, _i, c_fp, _l, _i, C.POINTER(DuetWeights), c_fp, C.c_void_p, _z, c_fp, c_st]),
    "nir_dssm_workspace_bytes": (_z, [_i, _i, _i]),
    "nir_dssm_score": (_i, [c_ip, c_ip, _i, _i, _i, _i, c_fp, _l, _i, _l, C.POINTER(DssmWeights), C.c_void_p, _z, c_fp, c_fp, c_fp, c_st]),
    "nir_cdssm_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "nir_cdssm_score": (_i, [c_ip, c_ip, _i, _i, _i, _i, c_fp, _l, _i, _l, C.POINTER(CdssmWeights), C.c_void_p, _z, c_fp, c_fp, c_fp, c_st]),
    "nir_conv1d_planes_bytes": (_z, [_i, _i, _i]),
    "nir_conv1d_pack": (_i, [c_fp, _i, _i, _i, C.c_void_p, c_fp, C.c_void_p, c_st]),
    "nir_conv1d_pool_out_floats": (_z, [_l, _i, _i, _i, _i]),
    "nir_conv1d_pool_f32": (_i, [c_ip, c_fp, _l, _i, C.POINTER(Conv1dLayer), _i, c_fp, c_fp, c_st]),
    "nir_arci_workspace_bytes": (_z, [_i, _i, _i, _i, C.POINTER(ArciWeights)]),
    "nir_arci_score": (_i, [c_ip, c_ip, _i, _i, _i, _i, c_fp, _l, _i, C.POINTER(ArciWeights), C.c_void_p, _z, c_fp, c_st]),
    "nir_conv2d_planes_bytes": (_z, [_i, _i, _i, _i]),
    "nir_conv2d_pack": (_i, [c_fp, _i, _i, _i, _i, C.c_void_p, c_fp, C.c_void_p, c_st]),
    "nir_conv2d_pool_out_floats": (_z, [_l, _i, _i, _i, _i, _i, _i]),
    "nir_conv2d_pool_f32": (_i, [c_fp, c_fp, c_fp, _l, _i, _i, _i, C.POINTER(Conv2dLayer), _i, c_fp, c_fp, c_st]),
    "nir_arcii_workspace_bytes": (_z, [_i, _i, _i, _i, C.POINTER(ArciiWeights)]),
    "nir_arcii_score": (_i, [c_ip, c_ip, _i, _i, _i, _i, c_fp, _l, _i, C.POINTER(ArciiWeights), C.c_void_p, _z, c_fp, c_st]),
    "nir_maxpool_arg_f32": (_i, [c_fp, _l, _i, _i, c_fp, C.c_void_p, c_st]),
    "nir_maxpool_arg_bwd_f32": (_i, [c_fp, C.c_void_p, _l, _i, _i, c_fp, c_st]),
    "nir_cosine_bcast_f32": (_i, [c_fp, c_fp, _l, _i, _i, c_fp, c_st]),
    "nir_cosine_bcast_bwd_f32": (_i, [c_fp, c_fp, c_fp, _l, _i, _i, c_fp, c_fp, c_st]),
    "nir_rank_loss_softmax_nll_bwd": (_i, [c_fp, c_fp, c_fp, _l, _i, c_fp, c_st]),
    "nir_cars_encode_workspace_bytes": (_z, [_l, _i, _i, C.POINTER(CarsEncoderWeights)]),
    "nir_cars_encode": (_i, [c_ip, c_ip, _l, _i, c_fp, _l, _i, C.POINTER(CarsEncoderWeights), C.c_void_p, _z,
                             c_fp, c_fp, c_st]),
    "nir_lstm_whh_frag_bytes": (_z, [_i, _i]),
    "nir_lstm_pack_whh_frag": (_i, [c_fp, _i, _i, C.c_void_p, C.c_void_p, c_st]),
    "nir_lstm_fold_table_bytes": (_z, [_l, _i, _i, _i]),
    "nir_lstm_fold_table_workspace_bytes": (_z, [_l, _i, _i, _i, _i]),
    "nir_lstm_fold_table": (_i, [c_fp, _l, _i, c_fp, c_fp, c_fp, _i, _i, C.c_void_p, _i, C.c_void_p, _z, c_st]),
    "nir_bilstm_folded_fwd": (_i, [C.c_void_p, _i, c_ip, c_ip, c_fp, c_fp, C.c_void_p, _l, _l, _i, _i, _i, c_st]),
    "nir_cars_encode_folded_workspace_bytes": (_z, [_l, _i, C.POINTER(CarsEncoderWeights)]),
    "nir_cars_encode_folded": (_i, [c_ip, c_ip, _l, _i, C.c_void_p, _i, _l, C.POINTER(CarsEncoderWeights), C.c_void_p, _z,
                                    c_fp, c_fp, C.c_void_p, c_st]),
    "nir_cars_session_workspace_bytes": (_z, [_i, _i, _i, C.POINTER(CarsSessionWeights)]),
    "nir_linear_wgrad_f32": (_i, [c_fp, _l, c_fp, _l, c_ip, c_fp, _i, c_fp, _l, _l, _i, _i, c_st]),
    "nir_colsum_f32": (_i, [c_fp, _l, _l, _i, c_fp, c_st]),
    "nir_linear_wgrad_set_f32": (_i, [c_fp, _l, c_fp, _l, c_ip, c_fp, _i, c_fp, _l, _l, _i, _i, c_st]),
    "nir_linear_wgrad_bias_f32": (_i, [c_fp, _l, c_fp, _l, c_ip, c_fp, _i, c_fp, _l, c_fp, _l, _i, _i, c_st]),
    "nir_linear_wgrad_group_f32": (_i, [_i] + [C.c_void_p] * 10 + [c_st]),
    "nir_linear_wgrad_bias_set_f32": (_i, [c_fp, _l, c_fp, _l, c_ip, c_fp, _i, c_fp, _l, c_fp, _l, _i, _i, c_st]),
    "nir_colsum_set_f32": (_i, [c_fp, _l, _l, _i, c_fp, c_st]),
    "nir_colsum_det_floats": (C.c_size_t, [_l, _i]),
    "nir_colsum_det_f32": (_i, [c_fp, _l, _l, _i, c_fp, c_fp, c_st]),
    "nir_seq_rows": (_i, [c_ip, _l, _i, _i, C.c_void_p, C.c_void_p, c_st]),
    "nir_linear_wgrad_rows_set_f32": (_i, [c_fp, _l, _l, c_fp, _l, _l, C.c_void_p, C.c_void_p, _l, _i, _i, c_fp, _l, c_fp, _i, _i, c_st]),
    "nir_transpose_f32": (_i, [c_fp, _i, _i, c_fp, c_st]),
    "nir_transpose_group_f32": (_i, [_i, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_st]),
    "nir_lstm_train_fwd": (_i, [c_fp, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, _l, _i, _i, _i, c_st]),
    "nir_lstm_perm_weights": (_i, [c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, _i, _i, _i, c_fp, c_fp, c_st]),
    "nir_lstm_train_fwd_split": (_i, [c_fp, c_ip, c_ip, c_fp, c_fp, c_fp, c_fp, C.c_void_p, _l, _i, _i, _i, c_st]),
    "nir_lstm_train_bwd": (_i, [c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_ip, c_fp, c_fp, c_fp, c_fp, _l, _i, _i, _i, c_st]),
    "nir_lstm_cell_fwd": (_i, [c_fp, c_fp, c_fp, c_fp, c_fp, _l, _i, c_st]),
    "nir_lstm_cell_bwd": (_i, [c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, _l, _i, c_st]),
    "nir_lstm_cell_seq_fwd": (_i, [c_fp, _l, c_fp, c_fp, c_fp, _l, c_fp, _l, c_fp, _l, c_fp, _l, _l, _i, c_st]),
    "nir_lstm_cell_seq_bwd": (_i, [c_fp, _l, c_fp, c_fp, _l, c_fp, c_fp, _l, c_fp, _l, c_fp, _l, c_fp, _l, c_fp, _l, _i, c_st]),
    "nir_gru_train_mfma_supported": (_i, [_i]),
    "nir_gru_train_fwd": (_i, [c_fp, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, _l, _i, _i, _i, c_st]),
    "nir_gru_train_bwd": (_i, [c_fp, c_fp, c_fp, c_fp, c_ip, c_fp, c_fp, c_fp, _l, _i, _i, _i, _i, c_st]),
    "nir_gru_cell_seq_fwd": (_i, [c_fp, _l, c_fp, c_fp, c_fp, _l, c_fp, _l, c_fp, _l, _l, _i, c_st]),
    "nir_gru_cell_seq_bwd": (_i, [c_fp, _l, c_fp, c_fp, c_fp, _l, c_fp, _l, c_fp, _l, c_fp, _l, c_fp, _l, _i, c_st]),
    "nir_dropout_f32": (_i, [c_fp, c_fp, C.c_void_p, _l, C.c_float, C.c_uint64, c_st]),
    "nir_dropout_dev_f32": (_i, [c_fp, c_fp, C.c_void_p, _l, C.c_float, C.c_void_p, C.c_uint64, c_st]),
    "nir_mask_scale_f32": (_i, [c_fp, C.c_void_p, C.c_float, c_fp, _l, c_st]),
    "nir_act_bwd_f32": (_i, [c_fp, c_fp, c_fp, _l, _i, c_st]),
    "nir_im2col_rows_f32": (_i, [c_fp, _l, _i, _i, _i, _i, _i, _i, _i, c_fp, c_st]),
    "nir_mt_conv3_supported": (_i, [_i, _i, _i, _i]),
    "nir_mt_conv3_fwd": (_i, [c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, _l, _i, _i, _i, _i, c_fp, c_st]),
    "nir_mt_conv3_wt_floats": (C.c_size_t, [_i, _i]),
    "nir_mt_conv3_partial_floats": (C.c_size_t, [_l, _i, _i]),
    "nir_mt_conv3_bwd": (_i, [c_fp, c_fp, c_fp, c_fp, c_fp, _l, _i, _i, _i, _i, c_fp, c_fp, c_fp, c_st]),
    "nir_col2im_rows_f32": (_i, [c_fp, _l, _i, _i, _i, _i, _i, _i, _i, c_fp, c_st]),
    "nir_rank_loss_bce_bwd": (_i, [c_fp, c_fp, c_fp, c_fp, _l, c_st]),
    "nir_softmax_nll_ent_fwd": (_i, [c_fp, _l, c_ip, _l, _l, _i, c_fp, c_fp, c_fp, C.c_void_p, c_st]),
    "nir_softmax_nll_ent_bwd": (_i, [c_fp, _l, c_ip, _l, c_fp, c_fp, c_fp, c_fp, _l, _i, c_fp, c_st]),
    "nir_softmax_pool_fwd": (_i, [c_fp, C.c_void_p, _l, _l, c_fp, _l, _i, _i, _i, c_fp, c_fp, c_st]),
    "nir_softmax_pool_bwd": (_i, [c_fp, c_fp, c_fp, _l, _i, _i, _i, c_fp, c_fp, c_st]),
    "nir_embed_f32": (_i, [c_ip, c_fp, _l, _i, _l, c_fp, C.c_void_p, c_st]),
    "nir_embed_bwd_f32": (_i, [c_ip, c_fp, _l, _i, _l, c_fp, _l, c_st]),
    "nir_add_f32": (_i, [c_fp, c_fp, c_fp, _l, c_st]),
    "nir_cars_decode_workspace_bytes": (_z, [_l, _l, _i, C.POINTER(CarsDecoderWeights)]),
    "nir_cars_decode_greedy": (_i, [c_fp, c_fp, c_fp, c_ip, _l, _i, c_ip, _l, c_fp, c_fp, _l, _i, c_ip, _l, _i,
                                    C.POINTER(CarsDecoderWeights), C.c_void_p, _z, c_ip, c_st]),
    "nir_cars_session_pack_floats": (_z, [C.POINTER(CarsSessionWeights), C.POINTER(_z), C.POINTER(_z)]),
    "nir_cars_session_pack": (_i, [C.POINTER(CarsSessionWeights), c_fp, c_fp, c_st]),
    "nir_cars_rank_session": (_i, [c_fp, c_fp, c_fp, _i, _i, _i, C.POINTER(CarsSessionWeights), C.c_void_p, _z,
                                   c_fp, c_fp, C.POINTER(CarsSessionOutputs), c_st]),
    "nir_cars_rank_session_shard": (_i, [c_fp, c_fp, c_fp, _i, _i, _i, C.POINTER(CarsSessionWeights), C.c_void_p, _z,
                                         c_fp, c_fp, C.POINTER(CarsSessionOutputs), c_fp, _i, c_st]),
    "nir_cars_rank_session_rows": (_i, [c_fp, c_fp, c_fp, _i, _i, _i, C.POINTER(CarsSessionWeights), C.c_void_p, _z,
                                        c_fp, c_fp, C.POINTER(CarsSessionOutputs), c_fp, _i, c_fp, _l, C.c_void_p, _i, c_st]),
    "nir_cars_session_query_side": (_i, [c_fp, _i, _i, C.POINTER(CarsSessionWeights), c_fp, c_fp, c_st]),
    "nir_cars_rank_session_pre": (_i, [c_fp, c_fp, c_fp, _i, _i, _i, C.POINTER(CarsSessionWeights), C.c_void_p, _z,
                                       c_fp, c_fp, C.POINTER(CarsSessionOutputs), c_fp, _i, c_fp, _l, C.c_void_p, _i, c_fp, c_fp, c_st]),
    "nir_cars_click_max": (_i, [c_fp, _i, _i, _i, C.c_void_p, c_st]),
    "nir_lstm_step_whh_frag_bytes": (_z, [_i]),
    "nir_lstm_step_pack_whh_frag": (_i, [c_fp, _i, C.c_void_p, C.c_void_p, c_st]),
    "nir_seq2seq_gen_frag_bytes": (_z, [_l, _i]),
    "nir_seq2seq_pack_gen_frag": (_i, [c_fp, _l, _i, C.c_void_p, C.c_void_p, c_st]),
    "nir_seq2seq_gen_argmax_workspace_bytes": (_z, [_l, _i, _l, _i]),
    "nir_seq2seq_gen_argmax": (_i, [c_fp, _l, _i, c_fp, c_fp, C.c_void_p, _l, c_ip, _l, C.c_void_p, _z, c_ip, _l, c_ip, c_st]),
    "nir_seq2seq_attend": (_i, [c_fp, c_fp, c_fp, c_fp, c_fp, c_ip, _l, _i, _i, _i, c_fp, c_fp, _l, c_st]),
    "nir_seq2seq_decode_workspace_bytes": (_z, [_l, _i, C.POINTER(Seq2seqDecoderWeights)]),
    "nir_seq2seq_decode_greedy": (_i, [c_fp, c_fp, c_fp, c_ip, _l, _i, c_fp, _l, _i, c_ip, _l, _i, C.POINTER(Seq2seqDecoderWeights), C.c_void_p, _z,
                                       c_ip, c_fp, c_st]),
    "nir_hredqs_gen_argmax_workspace_bytes": (_z, [_l]),
    "nir_hredqs_gen_argmax": (_i, [C.c_void_p, _l, _i, c_fp, C.c_void_p, _l, c_ip, _l, C.c_void_p, _z, c_ip, _l, c_ip, c_st]),
    "nir_hredqs_decode_workspace_bytes": (_z, [_l, _l, _i, C.POINTER(HredqsDecoderWeights)]),
    "nir_hredqs_decode_greedy": (_i, [c_fp, c_fp, _l, _l, c_fp, _l, _i, c_ip, _l, _i, C.POINTER(HredqsDecoderWeights), C.c_void_p, _z, c_ip, c_st]),
    "nir_acg_gen_select_workspace_bytes": (_z, [_l, _i, _l, _i]),
    "nir_acg_gen_select": (_i, [c_fp, _l, _i, c_fp, c_fp, C.c_void_p, _l, c_fp, c_fp, c_fp, _l, c_ip, _i, c_ip, c_ip, c_ip, _i, c_ip, _l, C.c_void_p, _z,
                                c_ip, _l, c_ip, c_fp, c_fp, c_ip, c_st]),
    "nir_acg_decode_workspace_bytes": (_z, [_l, _i, _i, C.POINTER(Seq2seqDecoderWeights), C.POINTER(AcgCopyWeights)]),
    "nir_acg_decode_greedy": (_i, [c_fp, c_fp, c_fp, c_ip, _l, _i, c_fp, _l, _i, c_ip, _l, _i, C.POINTER(Seq2seqDecoderWeights),
                                   C.POINTER(AcgCopyWeights), c_ip, c_ip, c_ip, _i, C.c_void_p, _z, c_ip, c_fp, c_st]),
    "nir_acg_copy_loss_fwd": (_i, [c_fp, _l, c_fp, c_fp, c_ip, c_ip, _i, _l, _i, c_fp, c_fp, C.c_void_p, c_st]),
    "nir_acg_copy_loss_bwd": (_i, [c_fp, _l, c_fp, c_fp, c_ip, c_ip, _i, c_fp, c_fp, _l, _i, c_fp, c_fp, c_fp, c_st]),
}

# The GRU decoders of Seq2seq and ACG, declared in include/neuroir_gru_decode.h (csrc/gru_step.hip, csrc/seq2seq.hip, csrc/acg.hip).  A table of
# its own: SIGNATURES mirrors the declarations of neuroir_hip.h itself, whose per-family symbol lists are pinned by tests.
GRU_DECODE_SIGNATURES = {
    "nir_gru_step_whh_frag_bytes": (_z, [_i]),
    "nir_gru_step_pack_whh_frag": (_i, [c_fp, _i, C.c_void_p, C.c_void_p, c_st]),
    "nir_gru_step_workspace_bytes": (_z, [_l, _i]),
    "nir_gru_step": (_i, [c_ip, _l, c_fp, _l, _i, c_fp, c_fp, c_fp, c_fp, c_fp, C.c_void_p, _i, c_fp, C.c_void_p, c_fp, C.c_void_p, C.c_void_p, _z, c_st]),
    "nir_seq2seq_gru_decode_workspace_bytes": (_z, [_l, _i, C.POINTER(Seq2seqDecoderWeights)]),
    "nir_seq2seq_gru_decode_greedy": (_i, [c_fp, c_fp, c_ip, _l, _i, c_fp, _l, _i, c_ip, _l, _i, C.POINTER(Seq2seqDecoderWeights), C.c_void_p, _z,
                                           c_ip, c_fp, c_st]),
    "nir_acg_gru_decode_workspace_bytes": (_z, [_l, _i, _i, C.POINTER(Seq2seqDecoderWeights), C.POINTER(AcgCopyWeights)]),
    "nir_acg_gru_decode_greedy": (_i, [c_fp, c_fp, c_ip, _l, _i, c_fp, _l, _i, c_ip, _l, _i, C.POINTER(Seq2seqDecoderWeights),
                                       C.POINTER(AcgCopyWeights), c_ip, c_ip, c_ip, _i, C.c_void_p, _z, c_ip, c_fp, c_st]),
}

# Beam search for Seq2seq, declared in include/neuroir_beam.h (csrc/beam.hip): every symbol starts with nir_beam_.  A table of its own for the
# same reason.
BEAM_MAX_W, BEAM_EOS = 8, 3
_W = C.POINTER(Seq2seqDecoderWeights)
BEAM_SIGNATURES = {
    "nir_beam_gen_topk_workspace_bytes": (_z, [_l, _i, _l, _i, _i]),
    "nir_beam_gen_topk": (_i, [c_fp, _l, _i, c_fp, c_fp, C.c_void_p, _l, _i, C.c_void_p, _z, c_fp, C.c_void_p, c_fp, c_st]),
    "nir_beam_select": (_i, [c_fp, C.c_void_p, c_fp, _l, _i, _l, c_ip, _l, c_fp, C.c_void_p, C.c_void_p, C.c_void_p, c_ip, c_st]),
    "nir_beam_reorder": (_i, [C.c_void_p, _l, _i, _i, c_fp, c_fp, c_fp, c_fp, C.c_void_p, C.c_void_p, c_st]),
    "nir_beam_seq2seq_decode_workspace_bytes": (_z, [_l, _i, _i, _i, _W]),
    "nir_beam_seq2seq_decode": (_i, [c_fp, c_fp, c_fp, c_ip, _l, _i, _i, c_fp, _l, _i, c_ip, _l, _i, _W, C.c_void_p, _z, c_ip, c_fp, c_ip, c_fp,
                                     C.c_void_p, c_st]),
    "nir_beam_seq2seq_gru_decode_workspace_bytes": (_z, [_l, _i, _i, _i, _W]),
    "nir_beam_seq2seq_gru_decode": (_i, [c_fp, c_fp, c_ip, _l, _i, _i, c_fp, _l, _i, c_ip, _l, _i, _W, C.c_void_p, _z, c_ip, c_fp, c_ip, c_fp,
                                         C.c_void_p, c_st]),
}

# Beam search for the session models (CARS, M_MATCH_TENSOR, MNSRF), declared in include/neuroir_session_beam.h (csrc/beam.hip).  BEAM_SIGNATURES
# mirrors neuroir_beam.h exactly (pinned by a test), so these have a table of their own too.
_CW = C.POINTER(CarsDecoderWeights)
SESSION_BEAM_SIGNATURES = {
    "nir_beam_cars_decode_workspace_bytes": (_z, [_l, _l, _i, _i, _i, _CW, _i]),
    "nir_beam_cars_decode": (_i, [c_fp, c_fp, c_fp, c_ip, _l, _i, c_ip, _l, c_fp, c_fp, _l, _i, c_ip, _l, _i, _CW, C.c_void_p, _i, C.c_void_p, _z, c_ip,
                                  c_fp, c_ip, C.c_void_p, c_st]),
    "nir_beam_plain_decode_workspace_bytes": (_z, [_l, _i, _l, _i, _i, _i, _i]),
    "nir_beam_plain_decode": (_i, [c_fp, c_fp, _l, _i, c_fp, _l, _i, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, _l, c_ip, _l, _i, c_fp, C.c_void_p, C.c_void_p, _i,
                                   C.c_void_p, _z, c_ip, c_fp, c_ip, C.c_void_p, c_st]),
}

# Beam search for ACG (the copy generator's collapsed extended distribution), declared in include/neuroir_acg_beam.h (csrc/beam.hip).  The
# tables above mirror their headers exactly (pinned by tests), so these have one of their own as well.
_AW = C.POINTER(AcgCopyWeights)
ACG_BEAM_SIGNATURES = {
    "nir_acg_beam_gen_select_workspace_bytes": (_z, [_l, _i, _l, _i, _i]),
    "nir_acg_beam_gen_select": (_i, [c_fp, _l, _l, _i, c_fp, c_fp, C.c_void_p, _l, _i, c_fp, c_fp, c_fp, _l, c_ip, _i, c_ip, c_ip, c_ip, _i, C.c_void_p, _z,
                                     c_fp, C.c_void_p, c_st]),
    "nir_acg_beam_select": (_i, [c_fp, C.c_void_p, c_fp, _l, _i, _l, _i, c_ip, c_ip, _l, c_fp, C.c_void_p, C.c_void_p, C.c_void_p, c_ip, c_st]),
    "nir_acg_beam_decode_workspace_bytes": (_z, [_l, _i, _i, _i, _i, _W, _AW]),
    "nir_acg_beam_decode": (_i, [c_fp, c_fp, c_fp, c_ip, _l, _i, c_fp, _l, _i, c_ip, _l, _i, _W, _AW, c_ip, c_ip, c_ip, _i, _i, C.c_void_p, _z, c_ip, c_fp,
                                 c_ip, c_fp, C.c_void_p, c_st]),
    "nir_acg_beam_gru_decode_workspace_bytes": (_z, [_l, _i, _i, _i, _i, _W, _AW]),
    "nir_acg_beam_gru_decode": (_i, [c_fp, c_fp, c_ip, _l, _i, c_fp, _l, _i, c_ip, _l, _i, _W, _AW, c_ip, c_ip, c_ip, _i, _i, C.c_void_p, _z, c_ip, c_fp,
                                     c_ip, c_fp, C.c_void_p, c_st]),
}

# Beam search for HredQS, declared in include/neuroir_hredqs_beam.h (csrc/beam.hip): top-W on the split state of the folded step.  A table of
# its own, like the ones above.
_HW = C.POINTER(HredqsDecoderWeights)
HREDQS_BEAM_SIGNATURES = {
    "nir_beam_hredqs_gen_topk_workspace_bytes": (_z, [_l, _i, _l, _i]),
    "nir_beam_hredqs_gen_topk": (_i, [C.c_void_p, _l, _i, c_fp, C.c_void_p, _l, _i, C.c_void_p, _z, c_fp, C.c_void_p, c_fp, c_st]),
    "nir_beam_hredqs_decode_workspace_bytes": (_z, [_l, _l, _i, _i, _HW]),
    "nir_beam_hredqs_decode": (_i, [c_fp, c_fp, _l, _l, c_fp, _l, _i, c_ip, _l, _i, _HW, _i, C.c_void_p, _z, c_ip, c_fp, c_ip, C.c_void_p, c_st]),
}

# Teacher-forced scoring of candidate queries, declared in include/neuroir_score.h (csrc/score.hip): every symbol starts with nir_score_.  A
# table of its own, like the ones above.
SCORE_SIGNATURES = {
    "nir_score_gen_target_workspace_bytes": (_z, [_l, _i, _l, _i]),
    "nir_score_gen_target": (_i, [c_fp, _l, _i, c_fp, c_fp, C.c_void_p, _l, c_ip, _l, C.c_void_p, _z, c_fp, c_fp, C.c_void_p, c_st]),
    "nir_score_sequences": (_i, [c_fp, c_ip, _l, _i, _l, _l, c_fp, c_ip, c_st]),
}

# The teacher-forced decoder pass of the session models, declared in include/neuroir_teacher.h (csrc/tf_attend.hip): grouped attention for many
# decoder rows that share one memory bank.  A table of its own, like the ones above.
TEACHER_SIGNATURES = {
    "nir_tf_attend_fusable": (_i, [_i, _i, _i]),
    "nir_tf_attend_workspace_bytes": (_z, [_l, _l, _i, _i]),
    "nir_tf_attend": (_i, [c_fp, c_fp, c_fp, c_ip, c_ip, _l, _l, _l, _i, _i, c_fp, c_fp, _l, C.c_void_p, _z, c_st]),
}

# Sampling decode for Seq2seq, declared in include/neuroir_sample.h (csrc/sample.hip): every symbol starts with nir_sample_.  A table of its
# own, like the ones above.  (the seed is a uint64, the inverse temperature a float)
_u64, _f = C.c_uint64, C.c_float
SAMPLE_SIGNATURES = {
    "nir_sample_noise": (_i, [_u64, _l, _l, _l, _l, c_fp, C.c_void_p, c_st]),
    "nir_sample_gen_workspace_bytes": (_z, [_l, _i, _l, _i]),
    "nir_sample_gen": (_i, [c_fp, _l, _l, _i, c_fp, c_fp, C.c_void_p, _l, _f, _u64, _l, C.c_void_p, _z, C.c_void_p, c_fp, c_fp, c_st]),
    "nir_sample_topk_select": (_i, [c_fp, C.c_void_p, c_fp, _l, _l, _i, _f, _u64, _l, C.c_void_p, c_fp, c_st]),
    "nir_sample_seq2seq_decode_workspace_bytes": (_z, [_l, _i, _i, _i, _i, _W]),
    "nir_sample_seq2seq_decode": (_i, [c_fp, c_fp, c_fp, c_ip, _l, _i, _i, _i, _f, _u64, c_fp, _l, _i, c_ip, _l, _i, _W, C.c_void_p, _z, c_ip, c_fp,
                                       c_fp, c_ip, c_fp, c_st]),
    "nir_sample_seq2seq_gru_decode_workspace_bytes": (_z, [_l, _i, _i, _i, _i, _W]),
    "nir_sample_seq2seq_gru_decode": (_i, [c_fp, c_fp, c_ip, _l, _i, _i, _i, _f, _u64, c_fp, _l, _i, c_ip, _l, _i, _W, C.c_void_p, _z, c_ip, c_fp, c_fp,
                                           c_ip, c_fp, c_st]),
}

# Sampling decode for HredQS and the session models, declared in include/neuroir_session_sample.h (csrc/session_sample.hip).  SAMPLE_SIGNATURES
# mirrors neuroir_sample.h exactly (pinned by a test), so these have a table of their own.
SESSION_SAMPLE_SIGNATURES = {
    "nir_sample_hredqs_gen_workspace_bytes": (_z, [_l, _i, _l]),
    "nir_sample_hredqs_gen": (_i, [C.c_void_p, _l, _l, _i, c_fp, C.c_void_p, _l, _f, _u64, _l, C.c_void_p, _z, C.c_void_p, c_fp, c_fp, c_st]),
    "nir_sample_hredqs_decode_workspace_bytes": (_z, [_l, _l, _i, _i, _i, _HW]),
    "nir_sample_hredqs_decode": (_i, [c_fp, c_fp, _l, _l, c_fp, _l, _i, c_ip, _l, _i, _HW, _i, _i, _f, _u64, C.c_void_p, _z, c_ip, c_fp, c_fp, c_ip, c_st]),
    "nir_sample_plain_decode_workspace_bytes": (_z, [_l, _i, _l, _i, _i, _i, _i, _i]),
    "nir_sample_plain_decode": (_i, [c_fp, c_fp, _l, _i, c_fp, _l, _i, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, _l, c_ip, _l, _i, c_fp, C.c_void_p, C.c_void_p, _i,
                                     _i, _f, _u64, C.c_void_p, _z, c_ip, c_fp, c_fp, c_ip, c_st]),
    "nir_sample_cars_decode_workspace_bytes": (_z, [_l, _l, _i, _i, _i, _i, _CW, _i]),
    "nir_sample_cars_decode": (_i, [c_fp, c_fp, c_fp, c_ip, _l, _i, c_ip, _l, c_fp, c_fp, _l, _i, c_ip, _l, _i, _CW, C.c_void_p, _i, _i, _f, _u64, C.c_void_p,
                                    _z, c_ip, c_fp, c_fp, c_ip, c_st]),
}

# Teacher-forced scoring under ACG's collapsed extended distribution, declared in include/neuroir_acg_score.h (csrc/score.hip).  A table of its
# own, like the ones above.
ACG_SCORE_SIGNATURES = {
    "nir_acg_score_gen_target_workspace_bytes": (_z, [_l, _i, _l, _i]),
    "nir_acg_score_gen_target": (_i, [c_fp, _l, _l, _i, c_fp, c_fp, C.c_void_p, _l, c_fp, c_fp, c_fp, _l, c_ip, _i, c_ip, c_ip, _i, c_ip, _l, C.c_void_p, _z,
                                      c_fp, C.c_void_p, c_st]),
}

# Sampling decode for ACG (draws from the collapsed extended distribution), declared in include/neuroir_acg_sample.h (csrc/sample.hip): every
# symbol starts with nir_acg_sample_.  A table of its own, like the ones above.
ACG_SAMPLE_SIGNATURES = {
    "nir_acg_sample_gen_select_workspace_bytes": (_z, [_l, _i, _l, _i, _i]),
    "nir_acg_sample_gen_select": (_i, [c_fp, _l, _l, _i, c_fp, c_fp, C.c_void_p, _l, _i, _f, _u64, _l, c_fp, c_fp, c_fp, _l, c_ip, _i, c_ip, c_ip, c_ip, _i,
                                       C.c_void_p, _z, C.c_void_p, c_fp, c_fp, c_fp, c_st]),
    "nir_acg_sample_decode_workspace_bytes": (_z, [_l, _i, _i, _i, _i, _i, _W, _AW]),
    "nir_acg_sample_decode": (_i, [c_fp, c_fp, c_fp, c_ip, _l, _i, c_fp, _l, _i, c_ip, _l, _i, _W, _AW, c_ip, c_ip, c_ip, _i, _i, _i, _f, _u64, C.c_void_p, _z,
                                   c_ip, c_fp, c_fp, c_ip, c_fp, c_st]),
    "nir_acg_sample_gru_decode_workspace_bytes": (_z, [_l, _i, _i, _i, _i, _i, _W, _AW]),
    "nir_acg_sample_gru_decode": (_i, [c_fp, c_fp, c_ip, _l, _i, c_fp, _l, _i, c_ip, _l, _i, _W, _AW, c_ip, c_ip, c_ip, _i, _i, _i, _f, _u64, C.c_void_p, _z,
                                       c_ip, c_fp, c_fp, c_ip, c_fp, c_st]),
}

# Corpus retrieval for DSSM / CDSSM (the document index and the fused cosine top-k), declared in include/neuroir_retrieve.h (csrc/retrieve.hip):
# every symbol starts with nir_retrieve_.  A table of its own, like the ones above; neuroir_hip.h does not include that header.
RETRIEVE_MAX_K, RETRIEVE_MAX_D = 128, 256
RETRIEVE_AUTO, RETRIEVE_FUSED, RETRIEVE_PLAIN = 0, 1, 2
RETRIEVE_SIGNATURES = {
    "nir_retrieve_index_bytes": (_z, [_l, _i]),
    "nir_retrieve_add": (_i, [c_fp, _l, _i, C.c_void_p, _l, _l, C.c_void_p, c_st]),
    "nir_retrieve_export": (_i, [C.c_void_p, _l, _i, _l, _l, c_fp, c_st]),
    "nir_retrieve_import": (_i, [c_fp, _l, _i, C.c_void_p, _l, _l, c_st]),
    "nir_retrieve_topk_workspace_bytes": (_z, [_l, _l, _i, _i, _i]),
    "nir_retrieve_topk": (_i, [c_fp, _l, C.c_void_p, _l, _i, _i, _i, C.c_void_p, _z, C.c_void_p, c_fp, C.c_void_p, c_st]),
    "nir_retrieve_merge": (_i, [c_fp, C.c_void_p, _i, _l, _i, c_fp, C.c_void_p, c_st]),
    "nir_retrieve_chunk_docs": (_i, []),
}

DTYPE_F32, DTYPE_BF16, DTYPE_F32_SPLIT2 = 0, 1, 2
DTYPES = {"f32": DTYPE_F32, "fp32": DTYPE_F32, "bf16": DTYPE_BF16, "f32_split2": DTYPE_F32_SPLIT2}

_lib = None


def load():
    """dlopen the in-tree library (never builds implicitly; run `python -m context_attentive_ir_amd.build`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libneuroir_hip.so not found at %s -- build it with `python -m context_attentive_ir_amd.build` "
                "(hipcc, gfx950). The HIP path has no CPU fallback." % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in (list(SIGNATURES.items()) + list(GRU_DECODE_SIGNATURES.items()) + list(BEAM_SIGNATURES.items()) + list(SESSION_BEAM_SIGNATURES.items())
                                  + list(ACG_BEAM_SIGNATURES.items()) + list(HREDQS_BEAM_SIGNATURES.items()) + list(SCORE_SIGNATURES.items())
                                  + list(TEACHER_SIGNATURES.items()) + list(SAMPLE_SIGNATURES.items()) + list(SESSION_SAMPLE_SIGNATURES.items())
                                  + list(ACG_SCORE_SIGNATURES.items()) + list(ACG_SAMPLE_SIGNATURES.items())
                                  + list(RETRIEVE_SIGNATURES.items())):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        msg = load().nir_last_error_string().decode("utf-8", "replace")
        kind = "argument error" if rc < 0 else "hipError_t"
        raise RuntimeError("%s failed (%s %d): %s" % (what, kind, rc, msg))


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("context_attentive_ir_amd runs on a ROCm device only (got a %s tensor); "
                               "there is no CPU fallback -- move the model and inputs to cuda" % t.device)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def set_batches_in_flight(n, streams=None):
    """the library's scheduling hint (nir_set_stream_batches_in_flight) for `streams` (torch streams; default: the current one): n independent
    batches are kept in flight next to the calls enqueued there; n < 1 removes the entry (= 1)."""
    L = load()
    for s in ([torch.cuda.current_stream()] if streams is None else streams):
        L.nir_set_stream_batches_in_flight(C.c_void_p(s.cuda_stream), int(n))
        if int(n) < 1:
            _BIF.pop(s.cuda_stream, None)
        else:
            _BIF[s.cuda_stream] = int(n)


_BIF = {}


def batches_in_flight():
    """the hint of the current stream (1 without one): the host-side mirror of the library's per-stream table"""
    return _BIF.get(torch.cuda.current_stream().cuda_stream, 1) if _BIF else 1


def ids64(t):
    """int64 contiguous view of an id / length tensor (the reference feeds torch.LongTensor)."""
    if t.dtype != torch.int64:
        t = t.long()
    return t.contiguous()


class Packed(object):
    """A ctypes weight struct + the tensors that back its pointers (kept alive together)."""

    def __init__(self, struct_cls, tensors, ints=None):
        self.keep = {k: v.detach().to(torch.float32).contiguous() for k, v in tensors.items()}
        for k, v in self.keep.items():
            if v.data_ptr() % 16:
                self.keep[k] = v.clone()
        self.struct = struct_cls()
        for k, v in self.keep.items():
            setattr(self.struct, k, v.data_ptr())
        for k, v in (ints or {}).items():
            setattr(self.struct, k, int(v))

    def ref(self):
        return C.byref(self.struct)

    def without(self, *fields):
        """a copy of the struct with those pointer fields null -- the same pack in an entry's plain form; the entry takes C.byref() of it, and
        the caller holds the copy until the call is enqueued (the tensors behind the other pointers stay with this pack)"""
        plain = type(self.struct).from_buffer_copy(self.struct)
        for f in fields:
            setattr(plain, f, None)
        return plain


# bumped whenever any PackCache rebuilds (= the only moment a superseded pack can be FREED): a hipGraph captured at epoch e references live packs
# for as long as the epoch is still e, whatever happened to the parameters meanwhile (graph_runner.PredictGraphCache's optimistic replay)
PACK_EPOCH = [0]


class PackCache(object):
    """Re-pack weights only when a parameter was modified (tensor._version) or moved.

    Keys may mix tensors and plain hashables (e.g. a dtype name).  `tensor._version` is bumped by every in-place op
    (optimizer steps, load_state_dict, `with torch.no_grad(): p.copy_()`), but NOT by writes through `p.data`; code that
    writes that way must call invalidate().  Superseded packs are kept alive (the last RETAIN of them): a hipGraph
    captured earlier still holds their device pointers, so freeing them on a repack would let the graph read freed memory.
    """
    RETAIN = 8

    def __init__(self, retain=None):
        """retain: superseded packs kept alive (default RETAIN); the folded [V, 8H] tables pass 1 -- alternating train and eval would
        otherwise pin eight dead multi-hundred-MB tables; a graph captured over an older table must be re-captured after training anyway."""
        self.key, self.val, self.retired = None, None, []
        if retain is not None:
            self.RETAIN = int(retain)

    def invalidate(self):
        self.key = None

    def get(self, params, builder):
        key = tuple((p.data_ptr(), p._version, str(p.device)) if torch.is_tensor(p) else p for p in params)
        if key != self.key:
            if self.val is not None:
                self.retired = (self.retired + [self.val])[-self.RETAIN:] if self.RETAIN > 0 else []
            self.val, self.key = builder(), key
            PACK_EPOCH[0] += 1
        return self.val


_WS = {}
_WS_RETIRED = []
_WS_OWNER = [None]


class workspace_owner(object):
    """Context manager: scratch requested inside the block belongs to `owner` (any object; buffers are stored on it as
    `_nir_ws`) instead of the shared per-(device, stream) pool.  graph_runner.GraphedPredictor captures under it, so the
    pointers baked into its hipGraph stay valid for the predictor's whole life no matter what other callers do."""

    def __init__(self, owner):
        self.owner = owner

    def __enter__(self):
        self.prev = _WS_OWNER[0]
        _WS_OWNER[0] = self.owner
        if not hasattr(self.owner, "_nir_ws"):
            self.owner._nir_ws = {}
        return self

    def __exit__(self, *exc):
        _WS_OWNER[0] = self.prev
        return False


def workspace(nbytes, device):
    """Scratch buffer per (device, stream) -- or per workspace_owner; the C library never allocates device memory.
    Buffers only grow (geometrically); a superseded buffer is retired, never freed, because a captured hipGraph may still
    hold its address."""
    owner = _WS_OWNER[0]
    pool = _WS if owner is None else owner._nir_ws
    k = (str(device), torch.cuda.current_stream().cuda_stream)
    buf = pool.get(k)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:      # (an owner's superseded buffers live as long as the owner -- its graphs -- does; the shared pool's for the process)
            (_WS_RETIRED if owner is None else owner.__dict__.setdefault("_nir_ws_retired", [])).append(buf)
        grow = 0 if buf is None else 2 * buf.numel()
        buf = torch.empty(max(int(nbytes), grow, 1 << 20), dtype=torch.uint8, device=device)
        pool[k] = buf
    return buf


def fold_lstm_table(table, wih, bih, bhh, H, ndir, dtype):
    """nir_lstm_fold_table: [V, ndir*4H] folded gate table (fp32, or bf16 stored as int16) -- weight packing, run once
    per parameter version (PackCache)."""
    L = load()
    V, E = table.shape
    dt = DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    out = torch.empty(V, ndir * 4 * H, device=table.device, dtype=torch.float32 if dt == DTYPE_F32 else torch.int16)
    ws = torch.empty(max(1, L.nir_lstm_fold_table_workspace_bytes(V, E, H, ndir, dt)), dtype=torch.uint8, device=table.device)
    t = table.detach().float().contiguous()
    check(L.nir_lstm_fold_table(ptr(t), V, E, ptr(wih), ptr(bih), ptr(bhh), H, ndir, ptr(out), dt, ptr(ws), ws.numel(), stream()),
          "nir_lstm_fold_table")
    return out


def fold_gru_table(table, wih, bih, bhh, H):
    """the GRU decoders' folded gate table [V, 3H] (fp32) = table W_ih^T + b_ih + (b_hr, b_hz, 0): b_hn stays outside, it belongs inside the
    reset product (csrc/gru_step.hip) -- weight packing, run once per parameter version (PackCache)."""
    t = table.detach().float().contiguous()
    bias = bih.clone()
    bias[:2 * H] += bhh[:2 * H]
    out = torch.empty(t.shape[0], 3 * H, device=t.device, dtype=torch.float32)
    check(load().nir_linear_f32(ptr(t), t.shape[1], None, None, 0, 0, 0, ptr(wih), t.shape[1], ptr(bias), None, ptr(out), 3 * H, t.shape[0], 3 * H,
                                t.shape[1], 0, stream()), "nir_linear_f32")
    return out


# bumped by anything that changes which kernels an entry point launches without touching a weight (debug tunables): part of the key of
# graph_runner.PredictGraphCache, so a graph captured before the change is not replayed after it
GRAPH_EPOCH = [0]


class tunable(object):
    """Context manager: `with lib.tunable("lstm_mfma16", 1): ...` (nir_debug_set_tunable; restores `restore` on exit)."""

    def __init__(self, name, value, restore):
        self.name, self.value, self.restore = name.encode(), int(value), int(restore)

    def __enter__(self):
        check(load().nir_debug_set_tunable(self.name, self.value), "nir_debug_set_tunable")
        GRAPH_EPOCH[0] += 1
        return self

    def __exit__(self, *exc):
        load().nir_debug_set_tunable(self.name, self.restore)
        GRAPH_EPOCH[0] += 1
        return False


class Flags(object):
    """The error word of one device + its pinned, device-mapped host mirror (round 6).

    Every kernel that can detect an error ORs into `dev` (bit 0: token id outside the vocabulary; bit 1: recurrent weights outside the fp16
    range of a split recurrence; bit 2: a recurrence cluster timed out) and never synchronises.  `publish()` enqueues nir_flag_publish at the
    end of a predict() / update(): a non-zero word lands in `host` (pinned memory the device writes directly).  `poll()` reads the host word --
    no device round trip -- and raises what it finds: called at the entry of the next wrapper call and from the `.cpu()` of the returned
    scores, i.e. right after the caller's own synchronisation in the reference's drivers (main/ranker.py:255, main/multitask.py:284).
    `check()` is the blocking form (reads the device word)."""

    def __init__(self, device):
        self.device = device
        self.dev = torch.zeros(1, dtype=torch.int32, device=device)
        self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.host_np = self.host.numpy()
        self.mapped = True
        self.cluster_handlers = []                          # weak references to callables run when bit 2 (cluster time-out) is found

    def on_cluster_timeout(self, method):
        """register a bound method (kept weakly) that makes its owner safe after a recurrence cluster timed out (MNSRF: switch to the streaming
        recurrence) -- run BEFORE the RuntimeError of the failed call is raised, so the caller's retry already takes the safe path"""
        import weakref
        self.cluster_handlers.append(weakref.WeakMethod(method))

    def publish(self):
        """capturable; -> False when the host word cannot be written by the device (then only check() sees errors)"""
        if self.mapped:
            rc = load().nir_flag_publish(ptr(self.dev), C.c_void_p(self.host.data_ptr()), stream())
            if rc != 0:
                self.mapped = False
        return self.mapped

    def _raise(self, v):
        if v & 4:
            live = []
            for ref in self.cluster_handlers:
                fn = ref()
                if fn is not None:
                    fn()
                    live.append(ref)
            self.cluster_handlers = live
            raise RuntimeError("a recurrence cluster (csrc/lstm_cluster.hip) waited for a partner workgroup that never became resident; the results of "
                               "that call are invalid -- the models on this device have been switched to the streaming recurrence: re-issue the batch")
        if v & 2:
            raise RuntimeError("recurrent weights outside the fp16 range of the split-fp16 MFMA recurrence (|w_hh| >= 2^15); "
                               "results of that call are invalid -- the exact fp32 recurrence handles such weights")
        raise IndexError("index out of range in self (token id outside [0, src_vocab_size))")

    def take(self):
        """blocking read-and-clear of the device word -> its value"""
        v = int(self.dev.item())
        if v != 0:
            self.dev.zero_()
        self.host_np[0] = 0
        return v

    def poll(self):
        if self.host_np[0] != 0:
            torch.cuda.synchronize(self.device)         # error path only: later publishes of the same sticky word have landed
            self._raise(self.take())

    def check(self):
        v = self.take()
        if v != 0:
            self._raise(v)


_FLAGS = {}


def flags(device):
    """the Flags of `device` (a torch.device with an index, e.g. tensor.device)"""
    key = (device.type, device.index)
    f = _FLAGS.get(key)
    if f is None:
        f = _FLAGS[key] = Flags(device)
    return f


class IdCheck(object):
    """Mixin of the network mirrors: `q, d = self._clean_ids(q, d, V)` validates token ids on the device (nir_sanitize_ids, one
    launch, no sync) and `check_ids()` raises the IndexError the reference's nn.Embedding would have raised at the lookup.
    `validate_ids = False` skips the launch for callers that guarantee 0 <= id < V themselves.  The flag every kernel of a device
    writes is ONE word (lib.flags(device).dev): `_flag_word(device)` hands out its tensor."""
    validate_ids = True
    _flag_dev = None

    def _flag_word(self, device):
        f = flags(device)
        self._flag_dev = device
        return f.dev

    def _clean_ids(self, a, b, V):
        a = ids64(a)
        b = ids64(b) if b is not None else None
        if not self.validate_ids:
            return a, b
        flag = self._flag_word(a.device)
        oa = torch.empty_like(a)
        ob = torch.empty_like(b) if b is not None else None
        check(load().nir_sanitize_ids(ptr(a), a.numel(), ptr(b), b.numel() if b is not None else 0, int(V), ptr(oa), ptr(ob), ptr(flag),
                                      stream()), "nir_sanitize_ids")
        return oa, ob

    def check_ids(self):
        """Synchronising: raise IndexError / RuntimeError if any forward on this network's device since the last check set an error bit."""
        if self._flag_dev is not None:
            flags(self._flag_dev).check()


def split_f16x2(x, cols_pad=None):
    """nir_split_f16x2: fp32 [rows, cols] -> two fp16 term planes [rows, cols_pad] (stored as int16 tensors)."""
    x = x.detach().float().contiguous()
    rows, cols = x.shape
    cp = (cols + 7) // 8 * 8 if cols_pad is None else int(cols_pad)
    p1 = torch.empty(rows, cp, dtype=torch.int16, device=x.device)
    p2 = torch.empty_like(p1)
    check(load().nir_split_f16x2(ptr(x), rows, cols, cols, cp, ptr(p1), ptr(p2), stream()), "nir_split_f16x2")
    return p1, p2
