"""ctypes bridge to ``libe2hip.so`` (the C ABI of ``include/e2hip.h``).

PyTorch-ROCm is used here for device memory and streams only: every tensor
handed to the library is a ``torch.float32`` CUDA(=HIP) tensor whose
``data_ptr()`` and element strides are passed through ``e2_tensor5``.

There is NO fallback: if the shared library is missing or does not load, the
import of this module raises, and so does every op.  (The CPU oracle under
``oracle/`` is test infrastructure and is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import tiling

_HERE =os.path.dirname(os.path.abspath(__file__))
# E2HIP_LIB: explicit path of another build of the library (debug-switch / ablation builds
# made by `make BUILD=... OUT=...`; the product build is never overwritten by experiments)
LIB_PATH = os.environ.get("E2HIP_LIB") or os.path.join(_HERE, "libe2hip.so")

# computations.py:57-134 apply_activation (E2_ACT_* of include/e2hip.h).  'lin' and 'relu' are
# taken by every entry point with an `act`; the others by act_fwd / act_bwd alone.
ACT = {"lin": 0, "linear": 0, "relu": 1, "tanh": 2, "sigmoid": 3, "sig": 3, "logistic": 3,
       "abs": 4, "elu": 5, "selu": 6, "soft+": 7}


class E2Error(RuntimeError):
    pass


# E2_POOL_* of include/e2hip.h (0 stays free for max)
POOL_MODE = {'avg': 1, 'sum': 2}
# E2_LRN_* of include/e2hip.h
LRN_MODE = {'spatial': 0, 'channel': 1}


class Tensor5(C.Structure):
    _fields_ = [("ptr", C.c_void_p),
                ("n", C.c_int32), ("c", C.c_int32), ("d", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32),
                ("sn", C.c_int64), ("sc", C.c_int64), ("sd", C.c_int64),
                ("sh", C.c_int64)]


class Bf16Dst(C.Structure):
    """e2_bf16_dst (include/e2hip.h): where a producer kernel puts the bf16 copies of its output"""
    _fields_ = [("cl", C.c_void_p), ("cl_kg", C.c_int32), ("cl_d", C.c_int32), ("cl_h", C.c_int32),
                ("cl_w", C.c_int32), ("cl_oz", C.c_int32), ("cl_oy", C.c_int32), ("cl_ox", C.c_int32),
                ("pl", C.c_void_p), ("pl_plane", C.c_int64), ("pl_pitch", C.c_int32)]


def bf16_dst(cl=None, cl_dims=None, cl_off=(0, 0, 0), pl=None, pl_plane=0, pl_pitch=0):
    """cl: uint8 device tensor holding [n][d][kg][h][w][8] bf16 (cl_dims = (kg, d, h, w)); pl: uint8
    device tensor holding [n][c][d][pl_plane] bf16"""
    d = Bf16Dst()
    d.cl = cl.data_ptr() if cl is not None else None
    if cl is not None:
        d.cl_kg, d.cl_d, d.cl_h, d.cl_w = (int(v) for v in cl_dims)
        d.cl_oz, d.cl_oy, d.cl_ox = (int(v) for v in cl_off)
    d.pl = pl.data_ptr() if pl is not None else None
    d.pl_plane, d.pl_pitch = int(pl_plane), int(pl_pitch)
    return d


class NllWeights(C.Structure):
    """e2_nll_weights (include/e2hip.h): class / example weights and the lazy-labelling masks of
    the weighted MultinoulliNLL; null members take their default"""
    _fields_ = [("class_w", C.c_void_p), ("example_w", C.POINTER(Tensor5)),
                ("labelled", C.c_void_p), ("not_present", C.c_void_p)]


class LossTerm(C.Structure):
    """e2_loss_term (include/e2hip.h): one element-wise loss of a mix; kind = LOSS[...]"""
    _fields_ = [("kind", C.c_int), ("margin", C.c_void_p), ("scale_correction", C.c_void_p),
                ("subtract_label_entropy", C.c_int), ("sig_is_log", C.c_int)]


# E2_LOSS_* of include/e2hip.h
LOSS = {"squared": 0, "abs": 1, "binary_nll": 2, "gauss_nll": 3}
MAX_LOSS_TERMS = 8


def t5_shape(shape):
    """a Tensor5 that carries extents only (null pointer): the shape argument of the entry points
    whose operand was made ahead of the call"""
    n, c, d, h, w = (int(v) for v in shape)
    return Tensor5(None, n, c, d, h, w, c * d * h * w, d * h * w, h * w, w)


def _load():
    if not os.path.exists(LIB_PATH):
        raise E2Error(
            "libe2hip.so not found at %s -- build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C elektronn2_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    P5 = C.POINTER(Tensor5)
    PP5 = C.POINTER(P5)
    PV = C.POINTER(C.c_void_p)
    PW = C.POINTER(NllWeights)
    PL = C.POINTER(LossTerm)
    vp, i, sz, fp = C.c_void_p, C.c_int, C.c_size_t, C.c_void_p
    sig = {
        "e2_ctx_create": (C.c_int, [i, C.POINTER(vp)]),
        "e2_ctx_destroy": (C.c_int, [vp]),
        "e2_ctx_set_stream": (C.c_int, [vp, vp]),
        "e2_last_error": (C.c_char_p, []),
        "e2_version": (C.c_int, []),
        "e2_conv3d_workspace_bytes": (sz, [i, i, i, i, i]),
        "e2_conv3d_fwd": (C.c_int, [vp, P5, fp, i, i, i, i, P5, vp, sz]),
        "e2_conv3d_dgrad": (C.c_int, [vp, P5, fp, i, i, i, i, P5, vp, sz]),
        "e2_conv3d_pack": (C.c_int, [vp, fp, i, i, i, i, i, i, vp, sz]),
        "e2_conv3d_fwd_packed": (C.c_int, [vp, P5, vp, i, i, i, i, P5]),
        "e2_conv3d_dgrad_packed": (C.c_int, [vp, P5, vp, i, i, i, i, P5]),
        "e2_conv3d_fwd_packed_act": (C.c_int, [vp, P5, vp, i, i, i, i, fp, i, P5]),
        "e2_bias_act_bwd_out": (C.c_int, [vp, P5, P5, i, P5, fp]),
        "e2_conv3d_dgrad_packed_actbwd": (C.c_int, [vp, P5, vp, i, i, i, i, P5, i, fp, P5, i, i, i, fp]),
        "e2_conv3d_wgrad": (C.c_int, [vp, P5, P5, fp, i, i, i]),
        "e2_conv3d_wgrad_acc": (C.c_int, [vp, P5, P5, fp, i, i, i]),
        "e2_conv3d_wgrad_pad": (C.c_int, [vp, P5, P5, fp, i, i, i, i]),
        "e2_pack_job_bytes": (sz, []),
        "e2_pack_job_fill": (C.c_int, [vp, fp, vp, i, i, i, i, i, i]),
        "e2_pack_job_set_rows": (C.c_int, [vp, i]),
        "e2_pack_job_set_stride": (C.c_int, [vp, i]),
        "e2_set_image_rows": (C.c_int, [vp, i]),
        "e2_conv3d_pack_multi": (C.c_int, [vp, vp, i]),
        "e2_conv3d_pack_multi_ex": (C.c_int, [vp, vp, i, i]),
        "e2_head_supported": (C.c_int, [i, i]),
        "e2_head_fwd": (C.c_int, [vp, P5, fp, fp, i, P5, P5, fp]),
        "e2_head_bwd_workspace_bytes": (C.c_size_t, [i, i, i, i, i, i]),
        "e2_tail_supported": (C.c_int, [i, i, i]),
        "e2_tail_workspace_bytes": (C.c_size_t, [i, i, i, i, i, i, i]),
        "e2_tail_fwd_bwd": (C.c_int, [vp, P5, fp, fp, fp, i, fp, fp, i, P5, P5, P5, P5, i, P5, fp, fp,
                                      C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]),
        "e2_tail_reduce": (C.c_int, [vp, C.c_void_p, i, i, i, fp, fp, fp, fp, fp, i, fp]),
        "e2_head_bwd": (C.c_int, [vp, P5, fp, P5, P5, fp, P5, i, fp, fp, fp, C.c_void_p,
                                  C.c_size_t]),
        "e2_malis_loss_weights": (C.c_int, [i, C.c_void_p, i, C.c_void_p, C.c_void_p,
                                            C.c_void_p, i, C.c_void_p]),
        "e2_malis_connected_components": (C.c_int, [i, i, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    i, C.c_void_p]),
        "e2_warp_slice": (C.c_int, [vp, P5, C.POINTER(C.c_float), i, C.c_uint,
                                    C.POINTER(C.c_int), C.POINTER(C.c_float), P5]),
        "e2_grey_augment": (C.c_int, [vp, fp, C.c_size_t, C.c_float, C.c_float, C.c_float]),
        "e2_target_stride": (C.c_int, [vp, P5, C.POINTER(C.c_int), P5]),
        "e2_target_nhood": (C.c_int, [vp, P5, C.POINTER(C.c_int), i, C.POINTER(C.c_int), P5]),
        "e2_target_affinity": (C.c_int, [vp, P5, C.POINTER(C.c_int), i, C.POINTER(C.c_int), P5]),
        "e2_count_negative": (C.c_int, [vp, P5, C.c_void_p]),
        "e2_ids2barriers": (C.c_int, [vp, P5, C.POINTER(C.c_int), C.POINTER(C.c_int), i, P5]),
        "e2_stream_fork": (C.c_int, [vp, C.c_void_p]),
        "e2_stream_join": (C.c_int, [vp, C.c_void_p]),
        "e2_conv1_supported": (C.c_int, [i, i, i, i, i, i, i]),
        "e2_conv1_pool_act_fwd": (C.c_int, [vp, P5, fp, fp, i, i, i, i, i, i, P5]),
        "e2_conv1_bwd_workspace_bytes": (C.c_size_t, [i, i, i, i, i, i, i]),
        "e2_conv1_pool_act_bwd": (C.c_int, [vp, P5, fp, fp, P5, i, i, i, i, i, fp, fp,
                                            C.c_void_p, C.c_size_t]),
        "e2_pool_bias_act_fwd": (C.c_int, [vp, P5, fp, i, i, i, i, P5]),
        "e2_conv3d_fwd_packed_parts": (C.c_int, [vp, P5, vp, i, i, i, i, P5, C.c_int64, i,
                                                 C.POINTER(C.c_int)]),
        "e2_conv3d_dgrad_packed_parts": (C.c_int, [vp, P5, vp, i, i, i, i, P5, C.c_int64, i,
                                                   C.POINTER(C.c_int)]),
        "e2_pool_bias_act_fwd_parts": (C.c_int, [vp, P5, C.c_int64, i, fp, i, i, i, i, P5]),
        "e2_pool_bias_act_bwd_parts": (C.c_int, [vp, P5, C.c_int64, i, P5, fp, i, i, i, i, P5, fp]),
        "e2_bias_act_bwd_out_parts": (C.c_int, [vp, P5, C.c_int64, i, P5, i, P5, fp]),
        "e2_pool_bias_act_bwd": (C.c_int, [vp, P5, P5, fp, i, i, i, i, P5, fp]),
        "e2_maxpool3d_fwd": (C.c_int, [vp, P5, i, i, i, P5]),
        "e2_maxpool3d_bwd": (C.c_int, [vp, P5, P5, i, i, i, P5, i]),
        "e2_pool3d_lin_fwd": (C.c_int, [vp, P5, i, i, i, i, i, i, i, P5]),
        "e2_pool3d_lin_bwd": (C.c_int, [vp, P5, i, i, i, i, i, i, i, P5, i]),
        "e2_lrn_fwd": (C.c_int, [vp, P5, i, i, i, i, fp, fp, fp, P5, P5]),
        "e2_lrn_bwd": (C.c_int, [vp, P5, P5, P5, i, i, i, i, fp, fp, P5, P5, i]),
        "e2_upconv3d_workspace_bytes": (sz, [i, i, i, i, i, i, i, i, i]),
        "e2_upconv3d_fwd": (C.c_int, [vp, P5, fp, fp, i, i, i, i, i, P5, vp, sz]),
        "e2_upconv3d_bwd": (C.c_int, [vp, P5, fp, P5, P5, i, i, i, i, P5, fp, fp, vp, sz]),
        "e2_upconv3d_image_bytes": (sz, [i, i, i, i, i]),
        "e2_upconv3d_fwd_packed": (C.c_int, [vp, P5, fp, fp, i, i, i, i, i, P5]),
        "e2_upconv3d_bwd_packed": (C.c_int, [vp, P5, fp, P5, P5, i, i, i, i, P5, fp, fp, vp, sz, i]),
        "e2_transpose_ncdhw_to_ndhwc": (C.c_int, [vp, P5, fp]),
        "e2_transpose_ndhwc_to_ncdhw": (C.c_int, [vp, fp, P5]),
        "e2_copy5": (C.c_int, [vp, P5, P5, i]),
        "e2_set_dgrad_zinset": (C.c_int, [vp, i]),
        "e2_pad5": (C.c_int, [vp, P5, P5, i, i, i, C.c_float, i]),
        "e2_fill": (C.c_int, [vp, fp, sz, C.c_float]),
        "e2_softmax_nll_fwd": (C.c_int, [vp, P5, P5, P5, fp]),
        "e2_softmax_nll_bwd": (C.c_int, [vp, P5, P5, fp, P5, fp]),
        "e2_softmax_nll_fwd_w": (C.c_int, [vp, P5, P5, P5, fp, PW]),
        "e2_softmax_nll_bwd_w": (C.c_int, [vp, P5, P5, fp, P5, fp, PW]),
        "e2_softmax_nll_grouped_fwd": (C.c_int, [vp, P5, P5, P5, i, fp]),
        "e2_softmax_nll_grouped_bwd": (C.c_int, [vp, P5, P5, i, fp, P5, fp]),
        "e2_nll_multi_fwd": (C.c_int, [vp, i, PP5, PP5, PP5, fp]),
        "e2_nll_mix": (C.c_int, [vp, i, fp, fp, fp, fp, fp, fp]),
        "e2_nll_multi_bwd": (C.c_int, [vp, i, PP5, PP5, fp, PP5]),
        "e2_multihead_supported": (C.c_int, [i, i, C.POINTER(C.c_int)]),
        "e2_multihead_fwd": (C.c_int, [vp, P5, i, PV, PV, C.POINTER(C.c_int), PP5, PP5, fp]),
        "e2_multihead_bwd_workspace_bytes": (sz, [i, i, i, i, i, i]),
        "e2_multihead_bwd": (C.c_int, [vp, P5, i, PV, PP5, PP5, fp, P5, i, PV, PV, C.c_void_p, sz]),
        "e2_head_fwd_w": (C.c_int, [vp, P5, fp, fp, i, P5, P5, fp, PW]),
        "e2_head_bwd_w": (C.c_int, [vp, P5, fp, P5, P5, fp, P5, i, fp, fp, fp, C.c_void_p,
                                    sz, PW]),
        "e2_tail_fwd_bwd_w": (C.c_int, [vp, P5, fp, fp, fp, i, fp, fp, i, P5, P5, P5, P5, i, P5,
                                        fp, fp, C.c_void_p, sz, C.POINTER(C.c_int), PW]),
        "e2_malis_nll": (C.c_int, [vp, P5, fp, fp, fp, P5, fp]),
        "e2_fill_multi": (C.c_int, [vp, vp, vp, C.c_int, C.c_float]),
        "e2_set_skip_zero_fill": (C.c_int, [vp, C.c_int]),
        "e2_set_input_slack": (C.c_int, [vp, C.c_int]),
        "e2_conv_last_zero_fill": (C.c_int, [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
        "e2_set_mfma_dtype": (C.c_int, [vp, C.c_int]),
        "e2_set_tiling": (C.c_int, [vp, C.c_int, C.c_char_p]),
        "e2_last_launch": (C.c_int, [vp, C.c_char_p, C.c_int]),
        "e2_tiling_fallbacks": (C.c_uint, [vp]),
        "e2_conv3d_bf16_workspace_bytes": (sz, [i, i, i, i, i, i, i, i, i]),
        "e2_conv3d_fwd_bf16": (C.c_int, [vp, P5, fp, i, i, i, i, fp, i, P5, vp, sz]),
        "e2_conv3d_dgrad_bf16": (C.c_int, [vp, P5, fp, i, i, i, i, P5, vp, sz]),
        "e2_conv3d_wgrad_bf16_workspace_bytes": (sz, [i, i, i, i, i, i, i, i, i]),
        "e2_conv3d_wgrad_bf16": (C.c_int, [vp, P5, P5, fp, i, i, i, i, vp, sz]),
        "e2_conv3d_bf16_xkeep_bytes": (sz, [i, i, i, i, i, i, i]),
        "e2_conv3d_fwd_bf16_keep": (C.c_int, [vp, P5, fp, i, i, i, i, fp, i, P5, vp, sz, vp, sz]),
        "e2_conv3d_wgrad_bf16_xcl": (C.c_int, [vp, P5, vp, i, P5, fp, i, i, i, i, vp, sz]),
        "e2_pool_bias_act_bwd_bf16": (C.c_int, [vp, P5, C.c_int64, i, P5, fp, i, i, i, i, P5, fp, C.POINTER(Bf16Dst)]),
        "e2_pool_bias_act_fwd_bf16": (C.c_int, [vp, P5, C.c_int64, i, fp, i, i, i, i, P5, C.POINTER(Bf16Dst)]),
        "e2_conv1_pool_act_fwd_bf16": (C.c_int, [vp, P5, fp, fp, i, i, i, i, i, i, P5, vp, i]),
        "e2_conv3d_bf16_wb_bytes": (sz, [i, i, i, i, i, i, i, i, i]),
        "e2_bf16_wjob_bytes": (sz, []),
        "e2_bf16_wjob_fill": (C.c_int, [vp, fp, i, i, i, i, i, i, i, i, i, i, vp, sz]),
        "e2_conv3d_bf16_pack_w_multi": (C.c_int, [vp, vp, i]),
        "e2_conv3d_fwd_bf16_ex": (C.c_int, [vp, P5, fp, i, i, i, i, fp, i, P5, vp, sz, vp, sz, i, vp, vp, i]),
        "e2_conv3d_dgrad_bf16_ex": (C.c_int, [vp, P5, fp, i, i, i, i, P5, vp, sz, vp, vp]),
        "e2_conv3d_wgrad_bf16_geometry": (C.c_int, [i, i, i, i, i, i, i, i, i, C.POINTER(C.c_int64),
                                                    C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "e2_conv3d_wgrad_bf16_ex": (C.c_int, [vp, P5, vp, i, P5, vp, fp, fp, i, i, i, i, vp, sz]),
        "e2_dense_fwd": (C.c_int, [vp, fp, fp, fp, i, i, i]),
        "e2_dense_dgrad": (C.c_int, [vp, fp, fp, fp, i, i, i, i]),
        "e2_dense_wgrad": (C.c_int, [vp, fp, fp, fp, i, i, i, i]),
        "e2_batchnorm_act_fwd": (C.c_int, [vp, P5, fp, fp, fp, fp, i, i, i, P5, fp]),
        "e2_batchnorm_act_bwd": (C.c_int, [vp, P5, P5, fp, fp, fp, i, i, P5, fp, fp]),
        "e2_get_mfma_dtype": (C.c_int, [vp]),
        "e2_dropout_fwd": (C.c_int, [vp, P5, P5, i, fp, vp, C.c_uint32]),
        "e2_dropout_bwd": (C.c_int, [vp, P5, P5, i, fp, vp, C.c_uint32]),
        "e2_dropout_tick": (C.c_int, [vp, vp]),
        "e2_act_fwd": (C.c_int, [vp, P5, fp, i, P5]),
        "e2_act_bwd": (C.c_int, [vp, P5, P5, fp, i, P5, fp]),
        "e2_loss_partials": (sz, [vp, P5]),
        "e2_loss_fwd": (C.c_int, [vp, PL, P5, P5, P5, fp]),
        "e2_loss_mix": (C.c_int, [vp, i, PL, C.POINTER(C.c_void_p), C.POINTER(sz),
                                  C.POINTER(C.c_int64), fp, fp, fp, fp, fp]),
        "e2_loss_bwd": (C.c_int, [vp, PL, P5, P5, P5, fp, P5, P5, i]),
        "e2_fdist_fwd": (C.c_int, [vp, P5, P5, P5]),
        "e2_fdist_bwd": (C.c_int, [vp, P5, P5, P5, P5, P5, P5, i, i]),
        "e2_ramp_fwd": (C.c_int, [vp, P5, P5, fp, P5]),
        "e2_ramp_bwd": (C.c_int, [vp, P5, P5, fp, P5, P5, P5, i, i]),
        "e2_mean_fwd": (C.c_int, [vp, P5, fp]),
        "e2_mean_bwd": (C.c_int, [vp, fp, P5, i]),
        "e2_onehot": (C.c_int, [vp, P5, i, P5]),
        "e2_beta_nll_fwd": (C.c_int, [vp, P5, P5, P5, fp]),
        "e2_beta_nll_bwd": (C.c_int, [vp, P5, P5, P5, fp, P5, P5, i]),
        "e2_adam_step": (C.c_int, [vp, fp, fp, fp, fp, sz, vp, fp, i, fp]),
        "e2_sgd_step": (C.c_int, [vp, fp, fp, fp, sz, vp, fp, i, fp]),
        "e2_set_loss_grad_mode": (C.c_int, [vp, i, fp]),
        "e2_upd_job_bytes": (sz, []),
        "e2_upd_rest_bytes": (sz, []),
        "e2_upd_job_fill": (C.c_int, [vp, C.c_long, vp, vp, i, i, i, i, i, C.c_float, i,
                                      C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
        "e2_upd_rest_fill": (C.c_int, [vp, C.c_long, C.c_long, C.c_float]),
        "e2_adam_pack_step": (C.c_int, [vp, fp, fp, fp, fp, vp, i, i, vp, i, fp, fp, C.c_float, i, sz]),
        "e2_adam_step_ex": (C.c_int, [vp, fp, fp, fp, fp, sz, vp, fp, i, fp, fp, C.c_float, i]),
        "e2_sgd_step_ex": (C.c_int, [vp, fp, fp, fp, sz, vp, fp, i, fp, fp, C.c_float, i]),
        "e2_adagrad_step_ex": (C.c_int, [vp, fp, fp, fp, sz, vp, fp, i, fp, fp, C.c_float, i]),
        "e2_adadelta_step_ex": (C.c_int, [vp, fp, fp, fp, fp, sz, vp, fp, i, fp, fp, C.c_float, i]),
        "e2_step_prologue": (C.c_int, [vp, fp, i, C.c_size_t, fp, fp, i, fp, i, vp]),
        "e2_graph_begin": (C.c_int, [vp]),
        "e2_graph_end": (C.c_int, [vp, C.POINTER(vp)]),
        "e2_graph_launch": (C.c_int, [vp, vp]),
        "e2_graph_destroy": (C.c_int, [vp]),
        "e2_graph_debug_dot": (C.c_int, [vp, C.c_char_p, i]),
        "e2_event_create": (C.c_int, [C.POINTER(vp)]),
        "e2_event_record": (C.c_int, [vp, vp]),
        "e2_event_elapsed_ms": (C.c_int, [vp, vp, C.POINTER(C.c_float)]),
        "e2_event_destroy": (C.c_int, [vp]),
        "e2_stream_synchronize": (C.c_int, [vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)          # AttributeError if a symbol is missing
        fn.restype = res
        fn.argtypes = args
    return lib, sorted(sig)


_lib, EXPORTED_SYMBOLS = _load()


def lib():
    return _lib


def _chk(rc: int, what: str):
    if rc != 0:
        msg = _lib.e2_last_error()
        raise E2Error("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else "?"))


def t5(t: torch.Tensor) -> Tensor5:
    """Describe a 5-D float32 device tensor (any view with unit W stride)."""
    if t.dim() != 5:
        raise TypeError("expected a 5-D (b,f,z,x,y) tensor, got %s" % (tuple(t.shape),))
    if t.dtype != torch.float32:
        raise TypeError("expected float32, got %s" % t.dtype)
    if not t.is_cuda:
        raise E2Error("tensor is on %s; the HIP path needs a GPU tensor (no CPU fallback)"
                      % t.device)
    s = t.stride()
    if t.shape[4] > 1 and s[4] != 1:
        raise TypeError("innermost stride must be 1, got %s" % (s,))
    return Tensor5(t.data_ptr(), t.shape[0], t.shape[1], t.shape[2], t.shape[3],
                   t.shape[4], s[0], s[1], s[2], s[3])


def nll_weights(class_w=None, example_w=None, labelled=None, not_present=None):
    """an e2_nll_weights descriptor of device tensors: ``class_w`` (ncls,), ``example_w``
    (n, 1, d, h, w), ``labelled`` / ``not_present`` (n, ncls); None = the default.  The kernels
    read the tensors when they RUN: a captured launch follows later changes of their contents."""
    w = NllWeights()
    w._keep = (class_w, example_w, labelled, not_present)       # (the tensors outlive the descriptor)
    w.class_w = _fp(class_w)
    if example_w is not None:
        w._ew = t5(example_w)
        w.example_w = C.pointer(w._ew)
    w.labelled = _fp(labelled)
    w.not_present = _fp(not_present)
    return w


def loss_term(kind, margin=None, scale_correction=None, subtract_label_entropy=False,
              sig_is_log=False):
    """an e2_loss_term descriptor: ``kind`` a key of LOSS; ``margin`` / ``scale_correction`` one-
    element device tensors (None: absent) that the kernels read when they RUN."""
    if kind not in LOSS:
        raise ValueError("loss_term: unknown kind %r (one of %s)" % (kind, sorted(LOSS)))
    t = LossTerm()
    t._keep = (margin, scale_correction)                      # (the tensors outlive the descriptor)
    t.kind = LOSS[kind]
    t.margin = _fp(margin)
    t.scale_correction = _fp(scale_correction)
    t.subtract_label_entropy = int(bool(subtract_label_entropy))
    t.sig_is_log = int(bool(sig_is_log))
    return t


def _fp(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise TypeError("expected a contiguous float32 GPU tensor")
    return C.c_void_p(t.data_ptr())


class Context:
    """One HIP stream + the library handle (one per process / device)."""

    def __init__(self, device: int = 0, stream: Optional[torch.cuda.Stream] = None):
        if not torch.cuda.is_available():
            raise E2Error("no GPU visible: the elektronn2_amd hot path is HIP-only")
        torch.cuda.set_device(device)
        h = C.c_void_p()
        _chk(_lib.e2_ctx_create(device, C.byref(h)), "e2_ctx_create")
        self.h = h
        self.device = torch.device("cuda", device)
        self.stream = None
        self.set_stream(stream if stream is not None else torch.cuda.current_stream(device))
        self._ws = {}

    def set_stream(self, stream: torch.cuda.Stream):
        self.stream = stream
        _chk(_lib.e2_ctx_set_stream(self.h, C.c_void_p(stream.cuda_stream)),
             "e2_ctx_set_stream")

    def stream_fork(self, side: torch.cuda.Stream):
        _chk(_lib.e2_stream_fork(self.h, C.c_void_p(side.cuda_stream)), "e2_stream_fork")

    def stream_join(self, side: torch.cuda.Stream):
        _chk(_lib.e2_stream_join(self.h, C.c_void_p(side.cuda_stream)), "e2_stream_join")

    def synchronize(self):
        _chk(_lib.e2_stream_synchronize(self.h), "e2_stream_synchronize")

    # ---- workspace -----------------------------------------------------
    def workspace(self, key, nbytes: int) -> torch.Tensor:
        w = self._ws.get(key)
        if w is None or w.numel() * 4 < nbytes:
            w = torch.empty((nbytes + 3) // 4 + 64, dtype=torch.float32, device=self.device)
            self._ws[key] = w
        return w

    # ---- conv ------------------------------------------------------------
    def conv_ws_bytes(self, cout, cin, k):
        return int(_lib.e2_conv3d_workspace_bytes(cout, cin, k[0], k[1], k[2]))

    def conv3d_fwd(self, x, w, y, ws=None):
        cout, cin, kd, kh, kw = w.shape
        nb = self.conv_ws_bytes(cout, cin, (kd, kh, kw))
        ws = ws if ws is not None else self.workspace("conv", nb)
        _chk(_lib.e2_conv3d_fwd(self.h, C.byref(t5(x)), _fp(w), cout, kd, kh, kw,
                                C.byref(t5(y)), C.c_void_p(ws.data_ptr()), ws.numel() * 4),
             "e2_conv3d_fwd")

    def conv3d_dgrad(self, dy_pad, w, dx, ws=None):
        cout, cin, kd, kh, kw = w.shape
        nb = self.conv_ws_bytes(cout, cin, (kd, kh, kw))
        ws = ws if ws is not None else self.workspace("conv", nb)
        _chk(_lib.e2_conv3d_dgrad(self.h, C.byref(t5(dy_pad)), _fp(w), cin, kd, kh, kw,
                                  C.byref(t5(dx)), C.c_void_p(ws.data_ptr()),
                                  ws.numel() * 4), "e2_conv3d_dgrad")

    def conv3d_pack(self, w, mode, ws):
        cout, cin, kd, kh, kw = w.shape
        _chk(_lib.e2_conv3d_pack(self.h, _fp(w), cout, cin, kd, kh, kw, mode,
                                 C.c_void_p(ws.data_ptr()), ws.numel() * 4),
             "e2_conv3d_pack")

    def conv3d_fwd_packed(self, x, wp, cout, k, y):
        _chk(_lib.e2_conv3d_fwd_packed(self.h, C.byref(t5(x)), C.c_void_p(wp.data_ptr()),
                                       cout, k[0], k[1], k[2], C.byref(t5(y))),
             "e2_conv3d_fwd_packed")

    def conv3d_dgrad_packed(self, dy_pad, wp, cin, k, dx):
        _chk(_lib.e2_conv3d_dgrad_packed(self.h, C.byref(t5(dy_pad)),
                                         C.c_void_p(wp.data_ptr()), cin, k[0], k[1], k[2],
                                         C.byref(t5(dx))), "e2_conv3d_dgrad_packed")

    # ---- split-K with partial-sum stores (e2hip.h "split-K without atomics") ----------------
    def conv3d_fwd_packed_parts(self, x, wp, cout, k, y_parts):
        """y_parts: (P, n, cout, d, h, w) dense slabs; returns the number of parts written
        (1: y_parts[0] is the complete result)"""
        n = C.c_int(0)
        _chk(_lib.e2_conv3d_fwd_packed_parts(self.h, C.byref(t5(x)), C.c_void_p(wp.data_ptr()),
                                             cout, k[0], k[1], k[2], C.byref(t5(y_parts[0])),
                                             y_parts.stride(0), y_parts.shape[0], C.byref(n)),
             "e2_conv3d_fwd_packed_parts")
        return n.value

    def conv3d_dgrad_packed_parts(self, dy_pad, wp, cin, k, dx_parts):
        n = C.c_int(0)
        _chk(_lib.e2_conv3d_dgrad_packed_parts(self.h, C.byref(t5(dy_pad)),
                                               C.c_void_p(wp.data_ptr()), cin, k[0], k[1], k[2],
                                               C.byref(t5(dx_parts[0])), dx_parts.stride(0),
                                               dx_parts.shape[0], C.byref(n)),
             "e2_conv3d_dgrad_packed_parts")
        return n.value

    def pool_bias_act_fwd_parts(self, y_parts, nparts, bias, pool, act, out):
        _chk(_lib.e2_pool_bias_act_fwd_parts(self.h, C.byref(t5(y_parts[0])), y_parts.stride(0),
                                             nparts, _fp(bias), pool[0], pool[1], pool[2],
                                             ACT[act], C.byref(t5(out))),
             "e2_pool_bias_act_fwd_parts")

    def pool_bias_act_bwd_parts(self, dout_parts, nparts, y, bias, pool, act, dy, dbias):
        _chk(_lib.e2_pool_bias_act_bwd_parts(self.h, C.byref(t5(dout_parts[0])),
                                             dout_parts.stride(0), nparts, C.byref(t5(y)),
                                             _fp(bias), pool[0], pool[1], pool[2], ACT[act],
                                             C.byref(t5(dy)), _fp(dbias)),
             "e2_pool_bias_act_bwd_parts")

    def bias_act_bwd_out_parts(self, dout_parts, nparts, out, act, dy, dbias):
        _chk(_lib.e2_bias_act_bwd_out_parts(self.h, C.byref(t5(dout_parts[0])),
                                            dout_parts.stride(0), nparts, C.byref(t5(out)),
                                            ACT[act], C.byref(t5(dy)), _fp(dbias)),
             "e2_bias_act_bwd_out_parts")

    def conv3d_fwd_packed_act(self, x, wp, cout, k, bias, act, out):
        """conv + bias + activation in one launch (layers that do not pool)"""
        _chk(_lib.e2_conv3d_fwd_packed_act(self.h, C.byref(t5(x)), C.c_void_p(wp.data_ptr()),
                                           cout, k[0], k[1], k[2], _fp(bias), ACT[act],
                                           C.byref(t5(out))), "e2_conv3d_fwd_packed_act")

    def conv3d_dgrad_packed_actbwd(self, dy_pad, wp, cin, k, out_prev, act_prev, dy_pad_prev,
                                   pad_prev, dbias_prev, bias_prev=None):
        """data gradient + activation backward of the producing layer, written into the
        interior of that layer's zero-padded gradient buffer (e2hip.h)"""
        _chk(_lib.e2_conv3d_dgrad_packed_actbwd(
            self.h, C.byref(t5(dy_pad)), C.c_void_p(wp.data_ptr()), int(cin), int(k[0]),
            int(k[1]), int(k[2]), C.byref(t5(out_prev)), ACT[act_prev],
            _fp(bias_prev) if bias_prev is not None else None, C.byref(t5(dy_pad_prev)),
            int(pad_prev[0]), int(pad_prev[1]), int(pad_prev[2]),
            _fp(dbias_prev) if dbias_prev is not None else None),
            "e2_conv3d_dgrad_packed_actbwd")

    def bias_act_bwd_out(self, dout, out, act, dy, dbias):
        _chk(_lib.e2_bias_act_bwd_out(self.h, C.byref(t5(dout)), C.byref(t5(out)), ACT[act],
                                      C.byref(t5(dy)), _fp(dbias)), "e2_bias_act_bwd_out")

    # ---- patch extraction / augmentation ---------------------------------------
    def warp_slice(self, src, minv, perspective, nearest_mask, dest_off, src_off, dst):
        """src (F,Z,X,Y) view, dst (F,pz,px,py) dense device tensors; minv 4x4 host array"""
        m = (C.c_float * 16)(*[float(v) for v in np.asarray(minv, np.float32).ravel()])
        do = (C.c_int * 3)(*[int(v) for v in dest_off])
        so = (C.c_float * 3)(*[float(v) for v in src_off])
        _chk(_lib.e2_warp_slice(self.h, C.byref(t5(src[None])), m, 1 if perspective else 0,
                                int(nearest_mask), do, so, C.byref(t5(dst[None]))),
             "e2_warp_slice")

    def grey_augment(self, chan, alpha, c, gamma):
        """in place on one dense channel tensor"""
        if not chan.is_contiguous():
            raise TypeError("grey_augment needs a dense channel")
        _chk(_lib.e2_grey_augment(self.h, _fp(chan), chan.numel(), float(alpha), float(c),
                                  float(gamma)), "e2_grey_augment")

    # ---- target forms of the batch creator (targets.hip) --------------------------
    @staticmethod
    def _ints3(v):
        v = [int(x) for x in v]
        if len(v) != 3:
            raise ValueError("expected three values, got %r" % (v,))
        return (C.c_int * 3)(*v)

    @staticmethod
    def _nhood(nhood):
        nh = np.ascontiguousarray(nhood, np.int32)
        if nh.ndim != 2 or nh.shape[1] != 3:
            raise ValueError("nhood must be (E, 3), got %s" % (nh.shape,))
        return (C.c_int * nh.size)(*[int(v) for v in nh.ravel()]), int(nh.shape[0])

    def target_stride(self, t, stride, dst):
        """dst (n, C, d, h, w) = t[..., ::sz, ::sx, ::sy] with NaN -> -666"""
        _chk(_lib.e2_target_stride(self.h, C.byref(t5(t)), self._ints3(stride), C.byref(t5(dst))),
             "e2_target_stride")

    def target_nhood(self, t, nhood, stride, dst):
        """dst (n, E + C - 1, d, h, w): channel 0 of t shifted by every row of ``nhood`` (-1 where
        the shift leaves the patch), then the stride; the other channels strided; NaN -> -666"""
        nh, E = self._nhood(nhood)
        _chk(_lib.e2_target_nhood(self.h, C.byref(t5(t)), nh, E, self._ints3(stride),
                                  C.byref(t5(dst))), "e2_target_nhood")

    def target_affinity(self, t, nhood, stride, dst):
        """dst (n, E, d, h, w) = the affinity graph (0 / 1) of the rounded, strided channel 0 of t"""
        nh, E = self._nhood(nhood)
        _chk(_lib.e2_target_affinity(self.h, C.byref(t5(t)), nh, E, self._ints3(stride),
                                     C.byref(t5(dst))), "e2_target_affinity")

    def count_negative(self, t, count):
        """count[0] += #{t < 0}; ``count``: a one-element int32 device tensor the caller zeroes"""
        if count.dtype != torch.int32 or not count.is_cuda or count.numel() < 1:
            raise TypeError("count_negative: count must be an int32 GPU tensor")
        _chk(_lib.e2_count_negative(self.h, C.byref(t5(t)), C.c_void_p(count.data_ptr())),
             "e2_count_negative")

    def ids2barriers(self, ids, dilute, connectivity, ecs_mode, dst):
        """ids, dst (1, 1, D, H, W); ecs_mode 0 none, 1 ECS (id 0) is barrier, 2 ECS a class of its own"""
        _chk(_lib.e2_ids2barriers(self.h, C.byref(t5(ids)),
                                  self._ints3([bool(v) for v in dilute]),
                                  self._ints3([bool(v) for v in connectivity]), int(ecs_mode),
                                  C.byref(t5(dst))), "e2_ids2barriers")

    # ---- fused classifier head -------------------------------------------------
    @staticmethod
    def head_supported(cin, ncls):
        return bool(_lib.e2_head_supported(int(cin), int(ncls)))

    def head_fwd(self, x, w, bias, target, probs, stats, weights=None):
        """``weights``: an ``nll_weights`` descriptor -> the weighted loss (e2_head_fwd_w)"""
        args = (self.h, C.byref(t5(x)), _fp(w), _fp(bias), probs.shape[1],
                C.byref(t5(target)) if target is not None else None,
                C.byref(t5(probs)), _fp(stats) if stats is not None else None)
        if weights is None:
            _chk(_lib.e2_head_fwd(*args), "e2_head_fwd")
        else:
            _chk(_lib.e2_head_fwd_w(*(args + (C.byref(weights),))), "e2_head_fwd_w")

    @staticmethod
    def head_bwd_ws_bytes(x_shape, ncls):
        n, cin, d, h, w = (int(v) for v in x_shape)
        return int(_lib.e2_head_bwd_workspace_bytes(n, cin, int(ncls), d, h, w))

    def head_bwd(self, x, w, probs, target, stats, dx, accumulate_dx, dw, dbias, loss_out,
                 ws=None, weights=None):
        if ws is None:
            ws = torch.empty(self.head_bwd_ws_bytes(x.shape, probs.shape[1]) // 4 + 16,
                             dtype=torch.float32, device=self.device)
        args = (self.h, C.byref(t5(x)), _fp(w), C.byref(t5(probs)),
                C.byref(t5(target)), _fp(stats),
                C.byref(t5(dx)) if dx is not None else None,
                1 if accumulate_dx else 0, _fp(dw), _fp(dbias),
                _fp(loss_out) if loss_out is not None else None,
                C.c_void_p(ws.data_ptr()), ws.numel() * 4)
        if weights is None:
            _chk(_lib.e2_head_bwd(*args), "e2_head_bwd")
        else:
            _chk(_lib.e2_head_bwd_w(*(args + (C.byref(weights),))), "e2_head_bwd_w")

    # ---- the tail of the neuro3d nets: 1x1x1 conv + head, forward and backward --------
    @staticmethod
    def tail_supported(c1, c2, ncls):
        return bool(_lib.e2_tail_supported(int(c1), int(c2), int(ncls)))

    @staticmethod
    def tail_ws_bytes(x_shape, c2, ncls):
        n, c1, d, h, w = (int(v) for v in x_shape)
        return int(_lib.e2_tail_workspace_bytes(n, c1, int(c2), int(ncls), d, h, w))

    def tail_fwd_bwd(self, x, wp_fwd, wp_dgrad, bias1, w_head, b_head, target, probs, dpre, dx,
                     stats, ws, gm_mode=0, gm_src=None, gm_bias=None, weights=None):
        """csrc/tail.hip: forward and backward of [1x1x1 conv + bias + relu] -> [classifier
        head] in one launch; returns the number of partial-sum slots written to ``ws``.
        ``gm_mode``: dx goes through the activation backward of the layer that produced x
        (1: slope from ``gm_src`` = its activated output, 2: from ``gm_src`` = its
        pre-activation + ``gm_bias``, 3: linear) and that layer's bias gradient joins the slots.
        ``weights``: an ``nll_weights`` descriptor -> the weighted loss (e2_tail_fwd_bwd_w)"""
        n_slots = C.c_int(0)
        args = (self.h, C.byref(t5(x)), _fp(wp_fwd), _fp(wp_dgrad), _fp(bias1),
                dpre.shape[1], _fp(w_head), _fp(b_head), probs.shape[1],
                C.byref(t5(target)), C.byref(t5(probs)), C.byref(t5(dpre)),
                C.byref(t5(dx)) if dx is not None else None, int(gm_mode),
                C.byref(t5(gm_src)) if gm_src is not None else None,
                _fp(gm_bias), _fp(stats),
                C.c_void_p(ws.data_ptr()), ws.numel() * 4, C.byref(n_slots))
        if weights is None:
            _chk(_lib.e2_tail_fwd_bwd(*args), "e2_tail_fwd_bwd")
        else:
            _chk(_lib.e2_tail_fwd_bwd_w(*(args + (C.byref(weights),))), "e2_tail_fwd_bwd_w")
        return int(n_slots.value)

    def tail_reduce(self, ws, n_slots, c2, ncls, dw_head, db_head, db1, stats, loss_out,
                    db_parent=None):
        _chk(_lib.e2_tail_reduce(self.h, C.c_void_p(ws.data_ptr()), int(n_slots), int(c2),
                                 int(ncls), _fp(dw_head), _fp(db_head), _fp(db1), _fp(stats),
                                 _fp(loss_out) if loss_out is not None else None,
                                 0 if db_parent is None else int(db_parent.numel()),
                                 _fp(db_parent)), "e2_tail_reduce")

    def conv3d_wgrad(self, x, dy, dw, accumulate=False):
        kd, kh, kw = dw.shape[2:]
        fn = _lib.e2_conv3d_wgrad_acc if accumulate else _lib.e2_conv3d_wgrad
        _chk(fn(self.h, C.byref(t5(x)), C.byref(t5(dy)), _fp(dw), kd, kh, kw),
             "e2_conv3d_wgrad")

    def conv3d_wgrad_pad(self, x, dy_pad, dw, accumulate=False):
        """wgrad from the zero-padded gradient buffer (borders zero, >= 128 readable
        bytes after its last element): the direct kernel."""
        kd, kh, kw = dw.shape[2:]
        _chk(_lib.e2_conv3d_wgrad_pad(self.h, C.byref(t5(x)), C.byref(t5(dy_pad)), _fp(dw),
                                      kd, kh, kw, 1 if accumulate else 0),
             "e2_conv3d_wgrad_pad")

    def set_image_rows(self, rows):
        """floats per k-row of the packed conv weight images the next conv3d_pack /
        conv3d_{fwd,dgrad}_packed* calls read (0 / None = the library's formula)"""
        _chk(_lib.e2_set_image_rows(self.h, int(rows or 0)), "e2_set_image_rows")

    def make_pack_jobs(self, jobs, rows=None, strides=None):
        """jobs: list of (w tensor, wp tensor, mode).  Returns a device byte tensor
        of job records for conv3d_pack_multi.  ``rows`` (optional, one entry per job, None / 0 =
        default): how far the reading launch's M tiles reach (e2_pack_job_set_rows).  ``strides``
        (optional, likewise): row length of the image (e2_pack_job_set_stride; the launches that
        read it need set_image_rows with the same value)."""
        rec = int(_lib.e2_pack_job_bytes())
        buf = (C.c_char * (rec * len(jobs)))()
        for n, (w, wp, mode) in enumerate(jobs):
            cout, cin, kd, kh, kw = w.shape
            _chk(_lib.e2_pack_job_fill(C.byref(buf, n * rec), _fp(w), C.c_void_p(wp.data_ptr()),
                                       cout, cin, kd, kh, kw, mode), "e2_pack_job_fill")
            if strides is not None and strides[n]:
                _chk(_lib.e2_pack_job_set_stride(C.byref(buf, n * rec), int(strides[n])), "e2_pack_job_set_stride")
            if rows is not None and rows[n]:
                _chk(_lib.e2_pack_job_set_rows(C.byref(buf, n * rec), int(rows[n])), "e2_pack_job_set_rows")
        host = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
        dev = host.to(self.device)
        dev.max_taps = max(int(w.shape[2] * w.shape[3] * w.shape[4]) for w, _, _ in jobs)
        dev.keep = [(w, wp) for w, wp, _ in jobs]
        return dev, len(jobs)

    def conv3d_pack_multi(self, jobs_dev, njobs):
        _chk(_lib.e2_conv3d_pack_multi_ex(self.h, C.c_void_p(jobs_dev.data_ptr()), njobs,
                                          int(getattr(jobs_dev, 'max_taps', 248))),
             "e2_conv3d_pack_multi_ex")

    # ---- fused first layer ----------------------------------------------------
    @staticmethod
    def conv1_supported(cin, k, pool):
        return bool(_lib.e2_conv1_supported(cin, k[0], k[1], k[2], pool[0], pool[1], pool[2]))

    def conv1_pool_act_fwd(self, x, w, bias, pool, act, out):
        _chk(_lib.e2_conv1_pool_act_fwd(self.h, C.byref(t5(x)), _fp(w), _fp(bias), w.shape[0],
                                        w.shape[3], w.shape[4], pool[1], pool[2], ACT[act],
                                        C.byref(t5(out))), "e2_conv1_pool_act_fwd")

    def conv1_pool_act_fwd_bf16(self, x, w, bias, pool, act, out, next_xb, next_kg):
        """conv1_pool_act_fwd + the next conv layer's channels-last bf16 input image"""
        _chk(_lib.e2_conv1_pool_act_fwd_bf16(self.h, C.byref(t5(x)), _fp(w), _fp(bias), w.shape[0],
                                             w.shape[3], w.shape[4], pool[1], pool[2], ACT[act],
                                             C.byref(t5(out)), C.c_void_p(next_xb.data_ptr()),
                                             int(next_kg)), "e2_conv1_pool_act_fwd_bf16")

    @staticmethod
    def conv1_bwd_ws_bytes(dout_shape, k):
        n, cout, d, ho, wo = (int(v) for v in dout_shape)
        return int(_lib.e2_conv1_bwd_workspace_bytes(n, cout, d, ho, wo, k[1], k[2]))

    def conv1_pool_act_bwd(self, x, w, bias, dout, pool, act, dw, dbias, ws=None):
        if ws is None:
            ws = torch.empty(self.conv1_bwd_ws_bytes(dout.shape, w.shape[2:]) // 4 + 16,
                             dtype=torch.float32, device=self.device)
        _chk(_lib.e2_conv1_pool_act_bwd(self.h, C.byref(t5(x)), _fp(w), _fp(bias),
                                        C.byref(t5(dout)), w.shape[3], w.shape[4], pool[1],
                                        pool[2], ACT[act], _fp(dw), _fp(dbias),
                                        C.c_void_p(ws.data_ptr()), ws.numel() * 4),
             "e2_conv1_pool_act_bwd")

    # ---- pool / bias / act ---------------------------------------------------
    def pool_bias_act_fwd(self, y, bias, pool, act, out):
        _chk(_lib.e2_pool_bias_act_fwd(self.h, C.byref(t5(y)), _fp(bias), pool[0], pool[1],
                                       pool[2], ACT[act], C.byref(t5(out))),
             "e2_pool_bias_act_fwd")

    def pool_bias_act_bwd(self, dout, y, bias, pool, act, dy, dbias):
        _chk(_lib.e2_pool_bias_act_bwd(self.h, C.byref(t5(dout)), C.byref(t5(y)), _fp(bias),
                                       pool[0], pool[1], pool[2], ACT[act], C.byref(t5(dy)),
                                       _fp(dbias)), "e2_pool_bias_act_bwd")

    def act_fwd(self, pre, bias, act, out):
        """out = f(pre + bias[c]) for every name of ACT; bias may be None, out may be pre"""
        _chk(_lib.e2_act_fwd(self.h, C.byref(t5(pre)), _fp(bias), ACT[act], C.byref(t5(out))),
             "e2_act_fwd")

    # ---- element-wise losses and their mix (csrc/loss_elem.hip) ---------------------------------
    def loss_partials(self, pred):
        """rows of 4 floats that loss_fwd writes for this prediction"""
        n = int(_lib.e2_loss_partials(self.h, C.byref(t5(pred))))
        if n <= 0:
            raise E2Error("e2_loss_partials: empty prediction %s" % (tuple(pred.shape),))
        return n

    def loss_fwd(self, term, pred, sig, target, partials):
        """per-work-group sums (S1, n_lab, S2, 0) of one loss term into ``partials`` (rows, 4)"""
        if partials.numel() < 4 * self.loss_partials(pred):
            raise E2Error("loss_fwd: the partials slab is too small for this prediction")
        _chk(_lib.e2_loss_fwd(self.h, C.byref(term), C.byref(t5(pred)),
                              None if sig is None else C.byref(t5(sig)), C.byref(t5(target)),
                              _fp(partials)), "e2_loss_fwd")

    def loss_mix(self, terms, partials, n_tot, mix, coef, term_loss, count, loss_out):
        """slabs of the k terms -> term_loss[k], count[k], coef[k] and the total loss_out[0]"""
        k = len(terms)
        if not (len(partials) == len(n_tot) == k):
            raise E2Error("loss_mix: %d terms, %d slabs, %d sizes" % (k, len(partials), len(n_tot)))
        if k > MAX_LOSS_TERMS:
            raise E2Error("loss_mix: %d terms, at most %d are supported" % (k, MAX_LOSS_TERMS))
        for t in (mix, coef, term_loss, count):
            if t.numel() < k:
                raise E2Error("loss_mix: mix / coef / term_loss / count need %d floats" % k)
        if loss_out.numel() < 1:
            raise E2Error("loss_mix: loss_out needs one float")
        ta = (LossTerm * max(k, 1))(*terms)
        pa = (C.c_void_p * max(k, 1))(*[_fp(p) for p in partials])
        ra = (C.c_size_t * max(k, 1))(*[int(p.numel()) // 4 for p in partials])
        na = (C.c_int64 * max(k, 1))(*[int(n) for n in n_tot])
        _chk(_lib.e2_loss_mix(self.h, k, ta, pa, ra, na, _fp(mix), _fp(coef), _fp(term_loss),
                              _fp(count), _fp(loss_out)), "e2_loss_mix")

    def loss_bwd(self, term, pred, sig, target, coef, dpred, dsig=None, accumulate=False):
        """dpred (=|+=) coef * d(term sum)/d(pred) (GAUSS_NLL: also dsig); ``coef`` the one-element
        device tensor loss_mix wrote for the term"""
        opt = lambda t: None if t is None else C.byref(t5(t))
        _chk(_lib.e2_loss_bwd(self.h, C.byref(term), C.byref(t5(pred)), opt(sig),
                              C.byref(t5(target)), _fp(coef), opt(dpred), opt(dsig),
                              int(bool(accumulate))), "e2_loss_bwd")

    # ---- losses over the feature axis, the mean of a loss map (csrc/loss_map.hip) ---------------
    def fdist_fwd(self, pred, target, out):
        """out[n,0,...] = sqrt(sum_f (target - pred)^2), NaN stored as 0"""
        _chk(_lib.e2_fdist_fwd(self.h, C.byref(t5(pred)), C.byref(t5(target)), C.byref(t5(out))),
             "e2_fdist_fwd")

    def fdist_bwd(self, pred, target, out, dout, dpred, dtarget=None, acc_pred=False,
                  acc_target=False):
        """dpred (=|+=) -(target - pred) / out * dout, dtarget the negative; either may be None"""
        opt = lambda t: None if t is None else C.byref(t5(t))
        _chk(_lib.e2_fdist_bwd(self.h, C.byref(t5(pred)), C.byref(t5(target)), C.byref(t5(out)),
                               C.byref(t5(dout)), opt(dpred), opt(dtarget), int(bool(acc_pred)),
                               int(bool(acc_target))), "e2_fdist_bwd")

    def ramp_fwd(self, d_low, d_big, margin, out):
        """out[n,0,...] = mean_f max(d_low - d_big + margin, 0), NaN as 0; ``margin``: a one-
        element device tensor read when the kernel runs"""
        _chk(_lib.e2_ramp_fwd(self.h, C.byref(t5(d_low)), C.byref(t5(d_big)), _fp(margin),
                              C.byref(t5(out))), "e2_ramp_fwd")

    def ramp_bwd(self, d_low, d_big, margin, dout, dd_low, dd_big=None, acc_low=False,
                 acc_big=False):
        opt = lambda t: None if t is None else C.byref(t5(t))
        _chk(_lib.e2_ramp_bwd(self.h, C.byref(t5(d_low)), C.byref(t5(d_big)), _fp(margin),
                              C.byref(t5(dout)), opt(dd_low), opt(dd_big), int(bool(acc_low)),
                              int(bool(acc_big))), "e2_ramp_bwd")

    def mean_fwd(self, x, partials):
        """slab rows (sum x, elements, 0, 0): a term of loss_mix under a 'gauss_nll' descriptor"""
        if partials.numel() < 4 * self.loss_partials(x):
            raise E2Error("mean_fwd: the partials slab is too small for this tensor")
        _chk(_lib.e2_mean_fwd(self.h, C.byref(t5(x)), _fp(partials)), "e2_mean_fwd")

    def onehot(self, target, out):
        """out[n,k,...] = (target[n,0,...] == k) as float, k < out.shape[1]; exact equality"""
        _chk(_lib.e2_onehot(self.h, C.byref(t5(target)), int(out.shape[1]), C.byref(t5(out))),
             "e2_onehot")

    def beta_nll_fwd(self, mode, conc, target, partials):
        """slab rows of the BetaNLL sums: a term of loss_mix under a 'gauss_nll' descriptor"""
        if partials.numel() < 4 * self.loss_partials(mode):
            raise E2Error("beta_nll_fwd: the partials slab is too small for this prediction")
        _chk(_lib.e2_beta_nll_fwd(self.h, C.byref(t5(mode)), C.byref(t5(conc)),
                                  C.byref(t5(target)), _fp(partials)), "e2_beta_nll_fwd")

    def beta_nll_bwd(self, mode, conc, target, coef, dmode, dconc=None, accumulate=False):
        opt = lambda t: None if t is None else C.byref(t5(t))
        _chk(_lib.e2_beta_nll_bwd(self.h, C.byref(t5(mode)), C.byref(t5(conc)),
                                  C.byref(t5(target)), _fp(coef), opt(dmode), opt(dconc),
                                  int(bool(accumulate))), "e2_beta_nll_bwd")

    def mean_bwd(self, coef, dx, accumulate=False):
        """dx (=|+=) coef[0]; ``coef``: the one-element device tensor loss_mix wrote"""
        _chk(_lib.e2_mean_bwd(self.h, _fp(coef), C.byref(t5(dx)), int(bool(accumulate))),
             "e2_mean_bwd")

    def act_bwd(self, dout, pre, bias, act, dpre, dbias):
        """dpre = dout * f'(pre + bias[c]), dbias[c] += sum(dpre) (None: not wanted); dpre may
        be dout"""
        _chk(_lib.e2_act_bwd(self.h, C.byref(t5(dout)), C.byref(t5(pre)), _fp(bias), ACT[act],
                             C.byref(t5(dpre)), _fp(dbias)), "e2_act_bwd")

    def maxpool3d_fwd(self, x, pool, out):
        _chk(_lib.e2_maxpool3d_fwd(self.h, C.byref(t5(x)), pool[0], pool[1], pool[2],
                                   C.byref(t5(out))), "e2_maxpool3d_fwd")

    def maxpool3d_bwd(self, dout, x, pool, dx, accumulate=False):
        _chk(_lib.e2_maxpool3d_bwd(self.h, C.byref(t5(dout)), C.byref(t5(x)), pool[0],
                                   pool[1], pool[2], C.byref(t5(dx)), int(accumulate)),
             "e2_maxpool3d_bwd")

    def pool_lin_fwd(self, x, pool, stride, mode, out):
        """out = average ('avg') / sum ('sum') of x over windows ``pool`` placed every ``stride``
        (pad 0, extent floor((in - p) / s) + 1); any strided views"""
        _chk(_lib.e2_pool3d_lin_fwd(self.h, C.byref(t5(x)), int(pool[0]), int(pool[1]),
                                    int(pool[2]), int(stride[0]), int(stride[1]), int(stride[2]),
                                    POOL_MODE.get(mode, mode), C.byref(t5(out))),
             "e2_pool3d_lin_fwd")

    def pool_lin_bwd(self, dout, pool, stride, mode, dx, accumulate=False):
        """dx (+)= the gradient of pool_lin_fwd: a gather over the windows that hold each element;
        elements no window holds become +0 (are left alone with ``accumulate``)"""
        _chk(_lib.e2_pool3d_lin_bwd(self.h, C.byref(t5(dout)), int(pool[0]), int(pool[1]),
                                    int(pool[2]), int(stride[0]), int(stride[1]), int(stride[2]),
                                    POOL_MODE.get(mode, mode), C.byref(t5(dx)),
                                    int(bool(accumulate))), "e2_pool3d_lin_bwd")

    def lrn_fwd(self, x, mode, window, alpha, k, beta, out, q=None):
        """out = x * (k + alpha * m)^(-beta), m the mean square over ``window`` = (fz, fx, fy)
        around each element ('spatial', zeros outside) or over window[0] features ('channel', the
        edge feature replicated); ``alpha`` / ``k`` / ``beta`` one-element device tensors the
        kernel reads when it RUNS; ``q`` (None: not kept) receives k + alpha * m for lrn_bwd"""
        _chk(_lib.e2_lrn_fwd(self.h, C.byref(t5(x)), LRN_MODE.get(mode, mode), int(window[0]),
                             int(window[1]), int(window[2]), _fp(alpha), _fp(k), _fp(beta),
                             C.byref(t5(q)) if q is not None else None, C.byref(t5(out))),
             "e2_lrn_fwd")

    def lrn_bwd(self, dout, x, q, mode, window, alpha, beta, tmp, dx, accumulate=False):
        """dx (+)= the gradient of lrn_fwd: t = dout * x * q^(-beta-1) into ``tmp``, then a
        gather over the window of t (two launches, no atomics)"""
        _chk(_lib.e2_lrn_bwd(self.h, C.byref(t5(dout)), C.byref(t5(x)), C.byref(t5(q)),
                             LRN_MODE.get(mode, mode), int(window[0]), int(window[1]),
                             int(window[2]), _fp(alpha), _fp(beta), C.byref(t5(tmp)),
                             C.byref(t5(dx)), int(bool(accumulate))), "e2_lrn_bwd")

    # ---- upconv ------------------------------------------------------------------
    def upconv_ws_bytes(self, cout, cin, pool, x_shape):
        return int(_lib.e2_upconv3d_workspace_bytes(cout, cin, pool[0], pool[1], pool[2],
                                                    x_shape[0], x_shape[2], x_shape[3],
                                                    x_shape[4]))

    def upconv3d_fwd(self, x, w, bias, pool, act, y, ws=None):
        cout, cin = w.shape[:2]
        nb = self.upconv_ws_bytes(cout, cin, pool, x.shape)
        ws = ws if ws is not None else self.workspace("upconv", nb)
        _chk(_lib.e2_upconv3d_fwd(self.h, C.byref(t5(x)), _fp(w), _fp(bias), cout, pool[0],
                                  pool[1], pool[2], ACT[act], C.byref(t5(y)),
                                  C.c_void_p(ws.data_ptr()), ws.numel() * 4),
             "e2_upconv3d_fwd")

    def upconv3d_bwd(self, x, w, y, dout, pool, act, dx, dw, dbias, ws=None):
        cout, cin = w.shape[:2]
        nb = self.upconv_ws_bytes(cout, cin, pool, x.shape)
        ws = ws if ws is not None else self.workspace("upconv", nb)
        _chk(_lib.e2_upconv3d_bwd(self.h, C.byref(t5(x)), _fp(w), C.byref(t5(y)),
                                  C.byref(t5(dout)), pool[0], pool[1], pool[2], ACT[act],
                                  C.byref(t5(dx)) if dx is not None else None,
                                  _fp(dw), _fp(dbias), C.c_void_p(ws.data_ptr()),
                                  ws.numel() * 4), "e2_upconv3d_bwd")

    @staticmethod
    def upconv_image_bytes(cout, cin, pool):
        return int(_lib.e2_upconv3d_image_bytes(int(cout), int(cin), pool[0], pool[1], pool[2]))

    def upconv3d_fwd_packed(self, x, wp_fwd, bias, cout, pool, act, y):
        """the forward with the image a mode-2 pack job keeps current (make_pack_jobs)"""
        _chk(_lib.e2_upconv3d_fwd_packed(self.h, C.byref(t5(x)), _fp(wp_fwd), _fp(bias), int(cout),
                                         pool[0], pool[1], pool[2], ACT[act], C.byref(t5(y))),
             "e2_upconv3d_fwd_packed")

    def upconv3d_bwd_packed(self, x, wp_dgrad, y, dout, pool, act, dx, dw, dbias, ws,
                            accumulate=False):
        """the backward with the data gradient's image of a mode-3 pack job; accumulate: dw
        and dbias are added to (the caller zeroed them)"""
        _chk(_lib.e2_upconv3d_bwd_packed(self.h, C.byref(t5(x)), _fp(wp_dgrad), C.byref(t5(y)),
                                         C.byref(t5(dout)), pool[0], pool[1], pool[2], ACT[act],
                                         C.byref(t5(dx)) if dx is not None else None,
                                         _fp(dw), _fp(dbias), C.c_void_p(ws.data_ptr()),
                                         ws.numel() * 4, int(bool(accumulate))),
             "e2_upconv3d_bwd_packed")

    # ---- layout ------------------------------------------------------------------
    def to_ndhwc(self, src, dst):
        _chk(_lib.e2_transpose_ncdhw_to_ndhwc(self.h, C.byref(t5(src)), _fp(dst)),
             "e2_transpose_ncdhw_to_ndhwc")

    def to_ncdhw(self, src, dst):
        _chk(_lib.e2_transpose_ndhwc_to_ncdhw(self.h, _fp(src), C.byref(t5(dst))),
             "e2_transpose_ndhwc_to_ncdhw")

    def copy5(self, src, dst, accumulate=False):
        _chk(_lib.e2_copy5(self.h, C.byref(t5(src)), C.byref(t5(dst)), int(accumulate)),
             "e2_copy5")

    def set_dgrad_zinset(self, planes):
        """the dgrad launches that follow read a padded gradient inset by ``planes`` z planes on
        either side (e2_set_dgrad_zinset); 0 withdraws it"""
        _chk(_lib.e2_set_dgrad_zinset(self.h, int(planes)), "e2_set_dgrad_zinset")

    def pad5(self, src, dst, pad, value=0.0, frame_only=False):
        """dst = src inside a frame of ``value`` of widths ``pad`` = (pz, px, py) on the three
        spatial axes (e2_pad5); ``frame_only``: the interior of dst is left alone (src may be None)"""
        _chk(_lib.e2_pad5(self.h, C.byref(t5(src)) if src is not None else None, C.byref(t5(dst)),
                          int(pad[0]), int(pad[1]), int(pad[2]), float(value), int(bool(frame_only))),
             "e2_pad5")

    def fill(self, t, value=0.0):
        if not t.is_contiguous():
            raise TypeError("fill needs a contiguous tensor")
        _chk(_lib.e2_fill(self.h, C.c_void_p(t.data_ptr()), t.numel(), float(value)),
             "e2_fill")

    # ---- dropout (e2hip.h: the gate contract) ------------------------------------------
    @staticmethod
    def _drop_state(state):
        if not (isinstance(state, torch.Tensor) and state.is_cuda and state.dtype == torch.int32
                and state.numel() >= 4 and state.is_contiguous() and state.data_ptr() % 16 == 0):
            raise TypeError("dropout state: four int32 words in device memory, 16-byte aligned")
        return C.c_void_p(state.data_ptr())

    def dropout_fwd(self, x, out, rate, state, stream, feature_mode=False):
        """out = gate(x) (``out`` may be ``x``); ``rate``: a one-element float32 device tensor,
        ``state``: int32[4] device tensor (seed lo, seed hi, counter, -) -- both read when the
        kernel RUNS"""
        _chk(_lib.e2_dropout_fwd(self.h, C.byref(t5(x)), C.byref(t5(out)), int(bool(feature_mode)),
                                 _fp(rate), self._drop_state(state), int(stream) & 0xffffffff),
             "e2_dropout_fwd")

    def dropout_bwd(self, dout, dx, rate, state, stream, feature_mode=False):
        """dx = gate(dout), the gate of dropout_fwd for the same state and stream"""
        _chk(_lib.e2_dropout_bwd(self.h, C.byref(t5(dout)), C.byref(t5(dx)), int(bool(feature_mode)),
                                 _fp(rate), self._drop_state(state), int(stream) & 0xffffffff),
             "e2_dropout_bwd")

    def dropout_tick(self, state):
        """state's counter += 1: the launch in front of a step's dropout launches"""
        _chk(_lib.e2_dropout_tick(self.h, self._drop_state(state)), "e2_dropout_tick")

    # ---- loss / optimiser ----------------------------------------------------------
    def softmax_nll_fwd(self, logits, target, probs, stats, weights=None):
        """``weights``: an ``nll_weights`` descriptor -> the weighted loss (the _w entry points)"""
        args = (self.h, C.byref(t5(logits)), C.byref(t5(target)), C.byref(t5(probs)), _fp(stats))
        if weights is None:
            _chk(_lib.e2_softmax_nll_fwd(*args), "e2_softmax_nll_fwd")
        else:
            _chk(_lib.e2_softmax_nll_fwd_w(*(args + (C.byref(weights),))), "e2_softmax_nll_fwd_w")

    def softmax_nll_bwd(self, probs, target, stats, dlogits, loss_out, weights=None):
        args = (self.h, C.byref(t5(probs)), C.byref(t5(target)), _fp(stats),
                C.byref(t5(dlogits)), _fp(loss_out))
        if weights is None:
            _chk(_lib.e2_softmax_nll_bwd(*args), "e2_softmax_nll_bwd")
        else:
            _chk(_lib.e2_softmax_nll_bwd_w(*(args + (C.byref(weights),))), "e2_softmax_nll_bwd_w")

    def softmax_nll_grouped_fwd(self, logits, target, probs, n_indep, stats):
        """``n_indep`` softmaxes over consecutive feature groups and their NLL in one launch;
        ``target`` (n, n_indep, d, h, w) or None: probabilities only, ``stats`` is not touched"""
        _chk(_lib.e2_softmax_nll_grouped_fwd(
            self.h, C.byref(t5(logits)), C.byref(t5(target)) if target is not None else None,
            C.byref(t5(probs)), int(n_indep), _fp(stats)), "e2_softmax_nll_grouped_fwd")

    def softmax_nll_grouped_bwd(self, probs, target, n_indep, stats, dlogits, loss_out):
        _chk(_lib.e2_softmax_nll_grouped_bwd(
            self.h, C.byref(t5(probs)), C.byref(t5(target)), int(n_indep), _fp(stats),
            C.byref(t5(dlogits)), _fp(loss_out)), "e2_softmax_nll_grouped_bwd")

    # ---- K MultinoulliNLL terms under one AggregateLoss (csrc/softmax_nll.hip) ----
    @staticmethod
    def _views(tensors, k):
        """a host array of k view pointers (None entries: NULL) and the descriptors it points to;
        ``tensors`` None: a NULL array"""
        if tensors is None:
            return None, None
        keep = [None if t is None else t5(t) for t in tensors]
        arr = (C.POINTER(Tensor5) * max(len(keep), k, 1))()
        for j, d in enumerate(keep):
            if d is not None:
                arr[j] = C.pointer(d)
        return arr, keep

    def nll_multi_fwd(self, logits, targets, probs, stats, k=None):
        """one launch: probs[j] = softmax(logits[j]) and, with targets, stats[2j] += S_j,
        stats[2j + 1] += N_j for every term j.  ``targets`` None (or all entries None):
        probabilities only.  ``k`` defaults to len(logits)."""
        k = len(logits) if k is None else int(k)
        la, lk = self._views(logits, k)
        ta, tk = self._views(targets, k)
        pa, pk = self._views(probs, k)
        _chk(_lib.e2_nll_multi_fwd(self.h, k, la, ta, pa, _fp(stats)), "e2_nll_multi_fwd")

    def nll_mix(self, k, stats, mix, coef, term_loss, count, loss_out):
        """one small launch: coef[j] = mix[j] / (k (N_j + 1e-5)), term_loss[j] = L_j, count[j] = N_j,
        loss_out[0] = (1/k) sum_j mix[j] L_j; ``mix`` is read on the device"""
        _chk(_lib.e2_nll_mix(self.h, int(k), _fp(stats), _fp(mix), _fp(coef), _fp(term_loss),
                             _fp(count), _fp(loss_out)), "e2_nll_mix")

    def nll_multi_bwd(self, probs, targets, coef, dlogits, k=None):
        """one launch: dlogits[j] = d total / d logits[j]; dlogits[j] may alias probs[j]"""
        k = len(probs) if k is None else int(k)
        pa, pk = self._views(probs, k)
        ta, tk = self._views(targets, k)
        da, dk = self._views(dlogits, k)
        _chk(_lib.e2_nll_multi_bwd(self.h, k, pa, ta, _fp(coef), da), "e2_nll_multi_bwd")

    # ---- K classifier heads on one trunk, fused (csrc/multihead.hip) ----
    @staticmethod
    def _ptrs(tensors, k):
        """a host array of k device pointers (contiguous float32 tensors; None: NULL)"""
        if tensors is None:
            return None
        arr = (C.c_void_p * max(len(tensors), k, 1))()
        for j, t in enumerate(tensors):
            v = _fp(t)
            arr[j] = None if v is None else v.value
        return arr

    @staticmethod
    def multihead_supported(cin, ncls):
        ncls = [int(c) for c in ncls]
        return bool(_lib.e2_multihead_supported(int(cin), len(ncls),
                                                (C.c_int * max(len(ncls), 1))(*ncls)))

    def multihead_fwd(self, x, w, bias, targets, probs, stats, k=None):
        """one launch: probs[j] = softmax(w[j] x + bias[j]) for every head j of the trunk ``x``
        and, with targets, stats[2j] += S_j, stats[2j + 1] += N_j.  ``w[j]``: (ncls_j, cin) dense"""
        k = len(probs) if k is None else int(k)
        ncls = (C.c_int * max(len(probs), k, 1))(*[int(p.shape[1]) for p in probs])
        ta, tk = self._views(targets, k)
        pa, pk = self._views(probs, k)
        xd = t5(x)
        _chk(_lib.e2_multihead_fwd(self.h, C.byref(xd), k, self._ptrs(w, k), self._ptrs(bias, k),
                                   ncls, ta, pa, _fp(stats)), "e2_multihead_fwd")

    @staticmethod
    def multihead_bwd_ws_bytes(x_shape, sum_ncls):
        n, cin, d, h, w = (int(v) for v in x_shape)
        return int(_lib.e2_multihead_bwd_workspace_bytes(n, cin, int(sum_ncls), d, h, w))

    def multihead_bwd(self, x, w, probs, targets, coef, dx, accumulate_dx, dw, dbias, ws, k=None,
                      ws_bytes=None):
        """one launch (+ the reduce): dx (=|+=) sum_j w[j]^T dlogits_j, dw[j] / dbias[j] += their
        gradients; ``ws``: multihead_bwd_ws_bytes(x.shape, sum ncls) bytes"""
        k = len(probs) if k is None else int(k)
        pa, pk = self._views(probs, k)
        ta, tk = self._views(targets, k)
        xd = t5(x)
        dxd = t5(dx) if dx is not None else None
        _chk(_lib.e2_multihead_bwd(
            self.h, C.byref(xd), k, self._ptrs(w, k), pa, ta, _fp(coef),
            C.byref(dxd) if dxd is not None else None, 1 if accumulate_dx else 0,
            self._ptrs(dw, k), self._ptrs(dbias, k),
            C.c_void_p(ws.data_ptr()) if ws is not None else None,
            ws.numel() * ws.element_size() if ws_bytes is None else int(ws_bytes)),
            "e2_multihead_bwd")

    def fill_multi(self, ptrs_dev, counts_dev, n, value=0.0):
        """one launch that fills n flat regions (int64 device tensors of pointers / counts)"""
        _chk(_lib.e2_fill_multi(self.h, C.c_void_p(ptrs_dev.data_ptr()),
                                C.c_void_p(counts_dev.data_ptr()), int(n), float(value)),
             "e2_fill_multi")

    def set_skip_zero_fill(self, on):
        _chk(_lib.e2_set_skip_zero_fill(self.h, 1 if on else 0), "e2_set_skip_zero_fill")

    def conv_last_zero_fill(self):
        """(pointer, count) of the flat region the last conv launch zero-filled, or (0, 0)"""
        p, n = C.c_void_p(), C.c_size_t()
        _chk(_lib.e2_conv_last_zero_fill(self.h, C.byref(p), C.byref(n)), "e2_conv_last_zero_fill")
        return (p.value or 0), int(n.value)

    # ---- bf16 operands in memory (32x32x16 MFMA kernel, csrc/conv_bf16.hip) ---------------
    @staticmethod
    def conv_bf16_ws_bytes(x_shape, cout, k):
        n, cin, d, h, w = (int(v) for v in x_shape)
        return int(_lib.e2_conv3d_bf16_workspace_bytes(n, cin, d, h, w, int(cout), k[0], k[1], k[2]))

    @staticmethod
    def conv_bf16_xkeep_bytes(x_shape, k):
        """bytes of the forward's kept bf16 copy of x (zero-fill it once)"""
        n, cin, d, h, w = (int(v) for v in x_shape)
        return int(_lib.e2_conv3d_bf16_xkeep_bytes(n, cin, d, h, w, k[1], k[2]))

    def conv3d_fwd_bf16(self, x, w, y, bias=None, act='lin', ws=None, xkeep=None):
        """xkeep: a zero-initialised uint8 buffer of conv_bf16_xkeep_bytes that receives the
        channels-last bf16 copy of x (read again by conv3d_wgrad_bf16(xcl=...))"""
        cout, cin, kd, kh, kw = w.shape
        if ws is None:
            ws = self.workspace("conv_bf16", self.conv_bf16_ws_bytes(x.shape, cout, (kd, kh, kw)))
        if xkeep is not None:
            _chk(_lib.e2_conv3d_fwd_bf16_keep(self.h, C.byref(t5(x)), _fp(w), cout, kd, kh, kw,
                                              _fp(bias), ACT[act], C.byref(t5(y)),
                                              C.c_void_p(ws.data_ptr()), ws.numel() * ws.element_size(),
                                              C.c_void_p(xkeep.data_ptr()),
                                              xkeep.numel() * xkeep.element_size()),
                 "e2_conv3d_fwd_bf16_keep")
            return
        _chk(_lib.e2_conv3d_fwd_bf16(self.h, C.byref(t5(x)), _fp(w), cout, kd, kh, kw,
                                     _fp(bias), ACT[act], C.byref(t5(y)),
                                     C.c_void_p(ws.data_ptr()), ws.numel() * ws.element_size()),
             "e2_conv3d_fwd_bf16")

    def conv3d_dgrad_bf16(self, dy_pad, w, dx, ws=None):
        cout, cin, kd, kh, kw = w.shape
        if ws is None:
            ws = self.workspace("conv_bf16", self.conv_bf16_ws_bytes(dx.shape, cout, (kd, kh, kw)))
        _chk(_lib.e2_conv3d_dgrad_bf16(self.h, C.byref(t5(dy_pad)), _fp(w), cin, kd, kh, kw,
                                       C.byref(t5(dx)), C.c_void_p(ws.data_ptr()),
                                       ws.numel() * ws.element_size()), "e2_conv3d_dgrad_bf16")

    @staticmethod
    def wgrad_bf16_ws_bytes(x_shape, cout, k):
        n, cin, d, h, w = (int(v) for v in x_shape)
        return int(_lib.e2_conv3d_wgrad_bf16_workspace_bytes(n, cin, d, h, w, int(cout), k[0], k[1], k[2]))

    def conv3d_wgrad_bf16(self, x, dy, dw, accumulate=False, ws=None, xcl=None):
        """dw (n_f, n_in, kd, kh, kw) from x and the UNPADDED gradient view dy; xcl: the
        forward's kept bf16 copy of x (conv3d_fwd_bf16(xkeep=...)) -- x is not converted again"""
        cout, cin, kd, kh, kw = dw.shape
        if ws is None:
            ws = self.workspace("wgrad_bf16", self.wgrad_bf16_ws_bytes(x.shape, cout, (kd, kh, kw)))
        if xcl is not None:
            _chk(_lib.e2_conv3d_wgrad_bf16_xcl(self.h, C.byref(t5(x)), C.c_void_p(xcl.data_ptr()),
                                               (cin + 15) // 16 * 2, C.byref(t5(dy)), _fp(dw),
                                               kd, kh, kw, int(accumulate), C.c_void_p(ws.data_ptr()),
                                               ws.numel() * ws.element_size()),
                 "e2_conv3d_wgrad_bf16_xcl")
            return
        _chk(_lib.e2_conv3d_wgrad_bf16(self.h, C.byref(t5(x)), C.byref(t5(dy)), _fp(dw), kd, kh, kw,
                                       int(accumulate), C.c_void_p(ws.data_ptr()),
                                       ws.numel() * ws.element_size()), "e2_conv3d_wgrad_bf16")

    def bf16_memory_wgrad(self):
        return tiling.is_memory_form('wgrad', self.current_tiling('wgrad'))

    def set_input_slack(self, nbytes):
        """promise (or, 0, withdraw the promise) that the x of the conv launches that follow has
        nbytes readable finite bytes behind its last element (e2_set_input_slack)"""
        _chk(_lib.e2_set_input_slack(self.h, int(nbytes)), "e2_set_input_slack")

    def current_tiling(self, kind):
        """the tiling string in force for kind ('igemm' | 'wgrad'), '' when none is pinned"""
        return getattr(self, '_tiling', {}).get(kind, '')

    # ---- the producers' epilogues: operands made ahead of the GEMM launches ------------------
    @staticmethod
    def bf16_tile(s):
        """(MB, NB) of a "32,MB,NB" tiling string, else None"""
        return tiling.bf16_tile(s)

    @staticmethod
    def conv_bf16_wb_bytes(rows, kk, k, in_w, out_w, tile):
        return int(_lib.e2_conv3d_bf16_wb_bytes(int(rows), int(kk), k[0], k[1], k[2], int(in_w),
                                                int(out_w), tile[0], tile[1]))

    def make_bf16_wjobs(self, jobs):
        """jobs: list of (w5 tensor (nf, nin, kd, kh, kw), mode, in_w, out_w, (MB, NB), wb uint8
        tensor).  Returns (device records, count) for conv3d_bf16_pack_w_multi."""
        rec = int(_lib.e2_bf16_wjob_bytes())
        buf = (C.c_char * (rec * len(jobs)))()
        for n, (w, mode, in_w, out_w, tile, wb) in enumerate(jobs):
            nf, nin, kd, kh, kw = w.shape
            _chk(_lib.e2_bf16_wjob_fill(C.byref(buf, n * rec), _fp(w), nf, nin, kd, kh, kw, int(mode),
                                        int(in_w), int(out_w), tile[0], tile[1],
                                        C.c_void_p(wb.data_ptr()), wb.numel()), "e2_bf16_wjob_fill")
        host = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
        return host.to(self.device), len(jobs)

    def conv3d_bf16_pack_w_multi(self, jobs_dev, njobs):
        _chk(_lib.e2_conv3d_bf16_pack_w_multi(self.h, C.c_void_p(jobs_dev.data_ptr()), njobs),
             "e2_conv3d_bf16_pack_w_multi")

    def conv3d_fwd_bf16_ex(self, x, w, y, bias=None, act='lin', ws=None, xkeep=None, x_ready=False,
                           wb=None, next_xb=None, next_kg=0):
        """conv3d_fwd_bf16 with ready-made operands (include/e2hip.h): x_ready: xkeep holds this
        step's copy of x; wb: the packed filter rows; next_xb: receives the channels-last bf16
        copy of y for the next layer"""
        cout, cin, kd, kh, kw = w.shape
        if ws is None and not (x_ready and wb is not None):
            ws = self.workspace("conv_bf16", self.conv_bf16_ws_bytes(x.shape, cout, (kd, kh, kw)))
        _chk(_lib.e2_conv3d_fwd_bf16_ex(
            self.h, C.byref(t5(x)), _fp(w), cout, kd, kh, kw, _fp(bias), ACT[act], C.byref(t5(y)),
            C.c_void_p(ws.data_ptr()) if ws is not None else None,
            ws.numel() * ws.element_size() if ws is not None else 0,
            C.c_void_p(xkeep.data_ptr()) if xkeep is not None else None,
            xkeep.numel() * xkeep.element_size() if xkeep is not None else 0, int(bool(x_ready)),
            C.c_void_p(wb.data_ptr()) if wb is not None else None,
            C.c_void_p(next_xb.data_ptr()) if next_xb is not None else None, int(next_kg)),
            "e2_conv3d_fwd_bf16_ex")

    def conv3d_dgrad_bf16_ex(self, dy_pad, w, dx, ws=None, dy_cl=None, wb=None):
        cout, cin, kd, kh, kw = w.shape
        if ws is None and not (dy_cl is not None and wb is not None):
            ws = self.workspace("conv_bf16", self.conv_bf16_ws_bytes(dx.shape, cout, (kd, kh, kw)))
        _chk(_lib.e2_conv3d_dgrad_bf16_ex(
            self.h, C.byref(t5(dy_pad)), _fp(w), cin, kd, kh, kw, C.byref(t5(dx)),
            C.c_void_p(ws.data_ptr()) if ws is not None else None,
            ws.numel() * ws.element_size() if ws is not None else 0,
            C.c_void_p(dy_cl.data_ptr()) if dy_cl is not None else None,
            C.c_void_p(wb.data_ptr()) if wb is not None else None), "e2_conv3d_dgrad_bf16_ex")

    @staticmethod
    def wgrad_bf16_geometry(x_shape, cout, k):
        """(elements per dy plane, bytes of the dy planes, bytes of the f32 sums) of
        conv3d_wgrad_bf16_ex's ready-made operands"""
        n, cin, d, h, w = (int(v) for v in x_shape)
        pd, db, sb = C.c_int64(), C.c_size_t(), C.c_size_t()
        _chk(_lib.e2_conv3d_wgrad_bf16_geometry(n, cin, d, h, w, int(cout), k[0], k[1], k[2],
                                                C.byref(pd), C.byref(db), C.byref(sb)),
             "e2_conv3d_wgrad_bf16_geometry")
        return int(pd.value), int(db.value), int(sb.value)

    def conv3d_wgrad_bf16_ex(self, x, dy, dw, accumulate=False, ws=None, xcl=None, dyc=None, sums=None):
        """conv3d_wgrad_bf16 with ready-made operands: xcl (the forward's kept copy of x), dyc
        (the bf16 planes of dy written by its producer), sums (a zeroed f32 buffer of the
        caller's, left zero)"""
        cout, cin, kd, kh, kw = dw.shape
        if ws is None and not (xcl is not None and dyc is not None and sums is not None):
            ws = self.workspace("wgrad_bf16", self.wgrad_bf16_ws_bytes(x.shape, cout, (kd, kh, kw)))
        _chk(_lib.e2_conv3d_wgrad_bf16_ex(
            self.h, C.byref(t5(x)), C.c_void_p(xcl.data_ptr()) if xcl is not None else None,
            (cin + 15) // 16 * 2, C.byref(t5(dy)),
            C.c_void_p(dyc.data_ptr()) if dyc is not None else None, _fp(sums), _fp(dw),
            kd, kh, kw, int(accumulate),
            C.c_void_p(ws.data_ptr()) if ws is not None else None,
            ws.numel() * ws.element_size() if ws is not None else 0), "e2_conv3d_wgrad_bf16_ex")

    def pool_bias_act_bwd_bf16(self, dout, src, bias, pool, act, dy, dbias, dst, parts=1, part_stride=0):
        """pool_bias_act_bwd (bias given: src = conv output) / bias_act_bwd_out (bias None: src =
        activated output) writing dy (f32, or None) and the bf16 copies named by dst (bf16_dst)"""
        dyv = t5(dy) if dy is not None else Tensor5(None, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        _chk(_lib.e2_pool_bias_act_bwd_bf16(self.h, C.byref(t5(dout)), int(part_stride), int(parts),
                                            C.byref(t5(src)), _fp(bias), pool[0], pool[1], pool[2],
                                            ACT[act], C.byref(dyv), _fp(dbias), C.byref(dst)),
             "e2_pool_bias_act_bwd_bf16")

    def pool_bias_act_fwd_bf16(self, y, bias, pool, act, out, dst, parts=1, part_stride=0):
        _chk(_lib.e2_pool_bias_act_fwd_bf16(self.h, C.byref(t5(y)), int(part_stride), int(parts),
                                            _fp(bias), pool[0], pool[1], pool[2], ACT[act],
                                            C.byref(t5(out)), C.byref(dst)),
             "e2_pool_bias_act_fwd_bf16")

    # ---- config 1 (mnist): Perceptron dot product, batch normalisation ------------------
    def dense_fwd(self, x, w, y):
        """y (n, m) = x (n, k) . w (k, m); contiguous 2-D views of device tensors"""
        n, k = x.shape
        _chk(_lib.e2_dense_fwd(self.h, _fp(x), _fp(w), _fp(y), n, k, w.shape[1]), "e2_dense_fwd")

    def dense_dgrad(self, dy, w, dx, accumulate=False):
        n, m = dy.shape
        _chk(_lib.e2_dense_dgrad(self.h, _fp(dy), _fp(w), _fp(dx), n, w.shape[0], m,
                                 int(accumulate)), "e2_dense_dgrad")

    def dense_wgrad(self, x, dy, dw, accumulate=False):
        n, k = x.shape
        _chk(_lib.e2_dense_wgrad(self.h, _fp(x), _fp(dy), _fp(dw), n, k, dy.shape[1],
                                 int(accumulate)), "e2_dense_wgrad")

    def batchnorm_act_fwd(self, x, gamma, bias, run_mean, run_std, train, update_running, act,
                          out, save=None):
        _chk(_lib.e2_batchnorm_act_fwd(self.h, C.byref(t5(x)), _fp(gamma), _fp(bias),
                                       _fp(run_mean), _fp(run_std), int(bool(train)),
                                       int(bool(update_running)), ACT[act], C.byref(t5(out)),
                                       _fp(save)), "e2_batchnorm_act_fwd")

    def batchnorm_act_bwd(self, dout, x, gamma, bias, save, train, act, dx, dgamma, dbias):
        _chk(_lib.e2_batchnorm_act_bwd(self.h, C.byref(t5(dout)), C.byref(t5(x)), _fp(gamma),
                                       _fp(bias), _fp(save), int(bool(train)), ACT[act],
                                       C.byref(t5(dx)) if dx is not None else None,
                                       _fp(dgamma), _fp(dbias)), "e2_batchnorm_act_bwd")

    def set_tiling(self, kind, cfg):
        """force the tiling of the following 'igemm' ("MT,NT,CC,SK": conv fwd / dgrad /
        UpConv) or 'wgrad' ("MT,NT,WK,BP,PS") launches of this context; None / '' returns
        the choice to the library's cost model (e2_set_tiling)"""
        code = {'igemm': 0, 'wgrad': 1}[kind]
        _chk(_lib.e2_set_tiling(self.h, code, (cfg or "").encode()), "e2_set_tiling")
        self._tiling = getattr(self, '_tiling', {})
        self._tiling[kind] = cfg or ""

    def last_launch(self):
        """(kernel family, tiling that ran, 'forced' | 'model' | 'fallback') of the last conv GEMM
        launch of this context (e2_last_launch), or None before the first one"""
        buf = C.create_string_buffer(160)
        _chk(_lib.e2_last_launch(self.h, buf, 160), "e2_last_launch")
        parts = buf.value.decode().split(" ")
        return tuple(parts) if len(parts) == 3 else None

    def tiling_fallbacks(self):
        """launches of this context whose forced tiling was not the one that ran"""
        return int(_lib.e2_tiling_fallbacks(self.h))

    def bf16_memory_form(self):
        """True while the forced igemm tiling selects the kernel with bf16 operands in memory
        ("32,MB,NB", csrc/conv_bf16.hip): the callers that hold the canonical weights then
        call conv3d_fwd_bf16 / conv3d_dgrad_bf16 instead of the packed entry points"""
        return tiling.is_memory_form('igemm', self.current_tiling('igemm'))

    def set_mfma_dtype(self, dtype):
        """'f32' (default) or 'bf16': operand rounding of the conv GEMMs (f32 sums)"""
        code = {'f32': 0, 'float32': 0, 'bf16': 1, 'bfloat16': 1}.get(dtype)
        if code is None:
            raise ValueError("mfma dtype must be 'f32' or 'bf16', got %r" % (dtype,))
        _chk(_lib.e2_set_mfma_dtype(self.h, code), "e2_set_mfma_dtype")
        self._mfma = 'bf16' if code else 'f32'

    @property
    def mfma_dtype(self):
        m = getattr(self, '_mfma', None)
        if m is None:
            m = self._mfma = 'bf16' if _lib.e2_get_mfma_dtype(self.h) == 1 else 'f32'
        return m

    def malis_nll(self, probs, pos, neg, norm, dlogits, loss_sum):
        """MALIS NLL of a (1, 2E, z, x, y) pair-softmax; dlogits None = loss only"""
        _chk(_lib.e2_malis_nll(self.h, C.byref(t5(probs)), _fp(pos), _fp(neg), _fp(norm),
                               C.byref(t5(dlogits)) if dlogits is not None else None,
                               _fp(loss_sum)), "e2_malis_nll")

    def set_loss_grad_mode(self, sum_mode, count_out=None):
        """sum_mode: the NLL backward launches that follow leave the gradient unnormalised and
        write this rank's labelled count to ``count_out`` (one-element device tensor)"""
        _chk(_lib.e2_set_loss_grad_mode(self.h, int(bool(sum_mode)), _fp(count_out)),
             "e2_set_loss_grad_mode")

    def _opt_step(self, entry_name, p, g, states, seg_off, seg_reg, hyper, gdiv, gmul, zero_g):
        """one optimiser update over the arena p: ``states`` are the rule's state arenas in the
        order of the entry point's arguments"""
        _chk(getattr(_lib, entry_name)(self.h, _fp(p), _fp(g), *[_fp(s) for s in states], p.numel(),
                                       C.c_void_p(seg_off.data_ptr()), _fp(seg_reg),
                                       seg_reg.numel(), _fp(hyper), _fp(gdiv), float(gmul),
                                       int(bool(zero_g))), entry_name)

    def adam_step(self, p, g, m, s, seg_off, seg_reg, hyper, gdiv=None, gmul=1.0, zero_g=False):
        """gdiv / gmul: the update sees g * gmul / (gdiv[0] + 1e-5) (gdiv: device scalar, or
        None); zero_g: g is left zero for the next backward pass"""
        self._opt_step("e2_adam_step_ex", p, g, (m, s), seg_off, seg_reg, hyper, gdiv, gmul, zero_g)

    def make_upd_jobs(self, jobs, rests):
        """records of adam_pack_step.  jobs: (arena offset, forward image | None, data-gradient
        image | None, (cout, cin, kd, kh, kw), weight-decay multiplier) per conv weight tensor;
        rests: (arena offset, elements, multiplier) for every other trainable run.  Returns the
        handle adam_pack_step takes."""
        rj, rr = int(_lib.e2_upd_job_bytes()), int(_lib.e2_upd_rest_bytes())
        bj = (C.c_char * max(rj * len(jobs), 1))()
        br = (C.c_char * max(rr * len(rests), 1))()
        tile0, lds = 0, 16
        keep = []
        for n, (off, wf, wd_, shape, reg) in enumerate(jobs):
            nt, lb = C.c_int(), C.c_size_t()
            cout, cin, kd, kh, kw = (int(v) for v in shape)
            _chk(_lib.e2_upd_job_fill(C.byref(bj, n * rj), int(off),
                                      C.c_void_p(wf.data_ptr()) if wf is not None else None,
                                      C.c_void_p(wd_.data_ptr()) if wd_ is not None else None,
                                      cout, cin, kd, kh, kw, float(reg), tile0, C.byref(nt), C.byref(lb)),
                 "e2_upd_job_fill")
            tile0 += nt.value
            lds = max(lds, int(lb.value))
            keep += [wf, wd_]
        for n, (off, cnt, reg) in enumerate(rests):
            _chk(_lib.e2_upd_rest_fill(C.byref(br, n * rr), int(off), int(cnt), float(reg)), "e2_upd_rest_fill")
        return dict(jobs=torch.frombuffer(bytearray(bj), dtype=torch.uint8).to(self.device), njobs=len(jobs),
                    ntiles=tile0, rest=torch.frombuffer(bytearray(br), dtype=torch.uint8).to(self.device),
                    nrest=len(rests), lds=lds, keep=keep)

    def adam_pack_step(self, p, g, m, s, upd, hyper, gdiv=None, gmul=1.0, zero_g=False):
        """adam_step + the repack of every conv's weight images in one launch (make_upd_jobs)"""
        _chk(_lib.e2_adam_pack_step(self.h, _fp(p), _fp(g), _fp(m), _fp(s),
                                    C.c_void_p(upd['jobs'].data_ptr()), upd['njobs'], upd['ntiles'],
                                    C.c_void_p(upd['rest'].data_ptr()), upd['nrest'], _fp(hyper),
                                    _fp(gdiv), float(gmul), int(bool(zero_g)), upd['lds']),
             "e2_adam_pack_step")

    def sgd_step(self, p, g, d, seg_off, seg_reg, hyper, gdiv=None, gmul=1.0, zero_g=False):
        self._opt_step("e2_sgd_step_ex", p, g, (d,), seg_off, seg_reg, hyper, gdiv, gmul, zero_g)

    def adagrad_step(self, p, g, h, seg_off, seg_reg, hyper, gdiv=None, gmul=1.0, zero_g=False):
        """h' = h + c g^2 (c = 2 at t = 0, else 1), p' = p - lr / sqrt(h') (g + wd r p); an element
        whose h' is 0 is left unchanged; t in hyper[4] advances (e2hip.h: e2_adagrad_step_ex)"""
        self._opt_step("e2_adagrad_step_ex", p, g, (h,), seg_off, seg_reg, hyper, gdiv, gmul, zero_g)

    def adadelta_step(self, p, g, s, d, seg_off, seg_reg, hyper, gdiv=None, gmul=1.0, zero_g=False):
        """s' = mom s + (1 - mom) g^2, dir = g sqrt(d + eps) / sqrt(s + eps) on the old s and d,
        d' = mom d + (1 - mom) dir^2, p' = p - lr (dir + wd mult p) (e2hip.h: e2_adadelta_step_ex)"""
        self._opt_step("e2_adadelta_step_ex", p, g, (s, d), seg_off, seg_reg, hyper, gdiv, gmul, zero_g)

    # ---- first launch of a step that may stand k times in one graph (e2hip.h: e2_step_prologue) ----
    def step_prologue(self, state, ring=None, dst=None, src=None, hist=None):
        """with L = launches on ``state`` (zeroed int64[2]) so far: dst = ring[L % n_slots] (ring:
        (n_slots, slot_floats) f32) and hist[(L - 1) % hist_slots] = src[:hist.shape[1]]"""
        assert state.dtype == torch.int64 and state.numel() >= 2 and state.is_contiguous()
        if ring is not None:
            assert ring.dim() == 2 and ring.is_contiguous() and ring.dtype == torch.float32
            assert dst is not None and dst.is_contiguous() and dst.numel() >= ring.shape[1]
        if hist is not None:
            assert hist.dim() == 2 and hist.is_contiguous() and src is not None and src.numel() >= hist.shape[1]
        _chk(_lib.e2_step_prologue(self.h, _fp(ring), int(ring.shape[0]) if ring is not None else 0,
                                   int(ring.shape[1]) if ring is not None else 0, _fp(dst), _fp(src),
                                   int(hist.shape[1]) if hist is not None else 0, _fp(hist),
                                   int(hist.shape[0]) if hist is not None else 0,
                                   C.c_void_p(state.data_ptr())), "e2_step_prologue")

    # ---- graph capture / events --------------------------------------------------------
    def graph_begin(self):
        _chk(_lib.e2_graph_begin(self.h), "e2_graph_begin")

    def graph_end(self):
        g = C.c_void_p()
        _chk(_lib.e2_graph_end(self.h, C.byref(g)), "e2_graph_end")
        return g

    def graph_launch(self, g):
        _chk(_lib.e2_graph_launch(self.h, g), "e2_graph_launch")

    def graph_destroy(self, g):
        _chk(_lib.e2_graph_destroy(g), "e2_graph_destroy")

    def graph_debug_dot(self, g, path, verbose=True):
        _chk(_lib.e2_graph_debug_dot(g, str(path).encode(), 1 if verbose else 0), "e2_graph_debug_dot")

    def event(self):
        e = C.c_void_p()
        _chk(_lib.e2_event_create(C.byref(e)), "e2_event_create")
        return e

    def record(self, e):
        _chk(_lib.e2_event_record(self.h, e), "e2_event_record")

    def elapsed_ms(self, e0, e1) -> float:
        ms = C.c_float()
        _chk(_lib.e2_event_elapsed_ms(e0, e1, C.byref(ms)), "e2_event_elapsed_ms")
        return float(ms.value)
