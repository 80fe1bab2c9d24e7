"""ctypes binding of librohm_hip.so (the C ABI in include/rohm_hip.h and the headers that include it: `HEADERS`).

There is no CPU fallback: if the library is missing, or a tensor is not on a HIP device,
the call raises.  Build the library with `python -m rohm_amd.build`.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('ROHM_HIP_LIB') or os.path.join(_HERE, 'librohm_hip.so')

c_float_p = C.POINTER(C.c_float)
c_int64_p = C.POINTER(C.c_int64)
c_double_p = C.POINTER(C.c_double)


class RohmHipError(RuntimeError):
    pass


ROHM_ERR_EXCHANGE = -5      # include/rohm_hip.h


class LayerWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        'in_proj_w', 'in_proj_b', 'out_proj_w', 'out_proj_b', 'lin1_w', 'lin1_b', 'lin2_w', 'lin2_b',
        'norm1_w', 'norm1_b', 'norm2_w', 'norm2_b')]


class PoseNetWeights(C.Structure):
    _fields_ = [('in_x_w', C.c_void_p), ('in_x_b', C.c_void_p), ('in_c_w', C.c_void_p), ('in_c_b', C.c_void_p),
                ('pe', C.c_void_p), ('pe_len', C.c_int),
                ('t_w0', C.c_void_p), ('t_b0', C.c_void_p), ('t_w2', C.c_void_p), ('t_b2', C.c_void_p),
                ('out_w', C.c_void_p), ('out_b', C.c_void_p),
                ('layers', C.POINTER(LayerWeights))]


class LayerGrads(C.Structure):
    _fields_ = LayerWeights._fields_


class PoseNetGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('in_x_w', 'in_x_b', 'in_c_w', 'in_c_b', 't_w0', 't_b0', 't_w2', 't_b2', 'out_w',
                                          'out_b')] + [('layers', C.POINTER(LayerGrads))]


class TensorRef(C.Structure):
    _fields_ = [('data', C.c_void_p), ('numel', C.c_size_t)]


class TrajNetWeights(C.Structure):
    _fields_ = [('tensors', C.POINTER(TensorRef)), ('n_tensors', C.c_int)]


class ResultRowsItem(C.Structure):
    _fields_ = [('src', C.c_void_p), ('stride_b', C.c_longlong), ('stride_t', C.c_longlong), ('stride_c', C.c_longlong),
                ('mean', C.c_void_p), ('std', C.c_void_p), ('traj', C.c_void_p), ('traj_rows', C.c_longlong), ('out', C.c_void_p)]


class ProfileRow(C.Structure):
    _fields_ = [('name', C.c_char * 48), ('launches', C.c_uint64), ('total_ms', C.c_double),
                ('flops', C.c_double), ('bytes', C.c_double)]


_lib = None

# the public headers under include/; together they declare every symbol of the library, each in one header
HEADERS = ('rohm_hip.h', 'rohm_multiview.h', 'rohm_fit_views.h', 'rohm_rig.h')

# name -> (restype, argtypes); must list every symbol the HEADERS declare (rohm_hip.h's first, then header by header)
SIGNATURES = {
    'rohm_last_error': (C.c_char_p, []),
    'rohm_version': (C.c_int, []),
    'rohm_profile_start': (C.c_int, [C.c_int]),
    'rohm_profile_stop': (C.c_int, [C.POINTER(ProfileRow), C.c_int, C.POINTER(C.c_int)]),
    'rohm_profile_detail': (C.c_int, [C.c_int]),
    'rohm_gemm_f32': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'rohm_exchange_probe': (C.c_int, [C.c_int, C.POINTER(C.c_char_p)]),
    'rohm_gemm_res_layernorm_scratch_bytes': (C.c_size_t, [C.c_int, C.c_int]),
    'rohm_gemm_res_layernorm_f32': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                              C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_layernorm_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'rohm_attention_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'rohm_planes_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'rohm_planes_split': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    'rohm_gemm_planes': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p]),
    'rohm_gemm_planes_ln': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                      C.c_void_p]),
    'rohm_layernorm_planes_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p]),
    'rohm_attention_planes_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'rohm_posenet_precision': (C.c_int, [C.c_void_p]),
    'rohm_ddpm_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                 C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_ddpm_step_table': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                       C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                       C.c_size_t, C.c_void_p]),
    'rohm_posenet_create': (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(PoseNetWeights), C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'rohm_posenet_destroy': (None, [C.c_void_p]),
    'rohm_posenet_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    'rohm_posenet_exchange_status': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_posenet_status_offset': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    'rohm_posenet_exchange_mode': (C.c_int, [C.c_void_p]),
    'rohm_posenet_exchange_guard': (C.c_char_p, [C.c_void_p]),
    'rohm_posenet_set_exchange': (C.c_int, [C.c_void_p, C.c_int]),
    'rohm_posenet_inject_exchange_fault': (C.c_int, [C.c_void_p, C.c_int]),
    'rohm_posenet_stack_addressable': (C.c_int, [C.c_longlong, C.c_int, C.c_int, C.c_int]),
    'rohm_posenet_stack_timeline_bytes': (C.c_size_t, [C.c_int]),
    'rohm_posenet_set_stack_timeline': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    'rohm_output_process_scratch_bytes': (C.c_size_t, []),
    'rohm_output_process_plan': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'rohm_output_process_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_posenet_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_posenet_sample_loop': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_int64_p, c_float_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                           C.c_void_p]),
    'rohm_posenet_train_saved_bytes': (C.c_size_t, [C.c_int] * 8),
    'rohm_posenet_train_scratch_bytes': (C.c_size_t, [C.c_int] * 8),
    'rohm_posenet_train_forward': (C.c_int, [C.POINTER(PoseNetWeights)] + [C.c_int] * 7 + [C.c_void_p] * 3 +
                                   [C.c_int, C.c_int, C.c_float, C.c_ulonglong, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_posenet_train_backward': (C.c_int, [C.POINTER(PoseNetWeights)] + [C.c_int] * 7 + [C.c_void_p] * 2 +
                                    [C.c_int, C.c_int, C.c_float, C.c_ulonglong, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.POINTER(PoseNetGrads), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_posenet_dropout_mask': (C.c_int, [C.c_ulonglong, C.c_int, C.c_int, C.c_float, C.c_longlong, C.c_void_p, C.c_void_p]),
    'rohm_q_sample': (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]),
    'rohm_trajnet_create': (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(TrajNetWeights), C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int]),
    'rohm_trajnet_destroy': (None, [C.c_void_p]),
    'rohm_trajnet_tune': (C.c_int, [C.c_int, C.c_int, C.c_int]),
    'rohm_trajnet_loop_mode': (C.c_int, []),
    'rohm_trajnet_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    'rohm_trajnet_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_trajnet_sample_loop': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_int64_p, c_float_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_size_t, C.c_void_p]),
    'rohm_trajnet_train_saved_bytes': (C.c_size_t, [C.c_int] * 7),
    'rohm_trajnet_train_scratch_bytes': (C.c_size_t, [C.c_int] * 7),
    'rohm_trajnet_train_forward': (C.c_int, [C.POINTER(TrajNetWeights)] + [C.c_int] * 5 + [C.c_void_p] * 4 +
                                   [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_trajnet_train_backward': (C.c_int, [C.POINTER(TrajNetWeights)] + [C.c_int] * 7 +
                                    [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_trajnet_train_last_gemms': (C.c_int, []),
    'rohm_smplx_create': (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_int, C.c_int]),
    'rohm_smplx_destroy': (None, [C.c_void_p]),
    'rohm_smplx_frames_to_world': (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rohm_smplx_joints': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_int, C.c_void_p]),
    'rohm_guidance_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int]),
    'rohm_guidance_skating_grad': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_guidance_skating_prepare': (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                                C.c_void_p]),
    'rohm_guidance_skating_apply': (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_size_t, C.c_void_p]),
    'rohm_guidance_proj2d_grad': (C.c_int, [C.c_void_p] * 10 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_size_t, C.c_void_p]),
    'rohm_smplx_set_skinning': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    'rohm_smplx_skinning_mode': (C.c_int, [C.c_void_p]),
    'rohm_smplx_lbs_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int]),
    'rohm_smplx_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_repr_joints': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p,
                                   C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'rohm_repr_joints_vjp': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong,
                                       C.c_longlong, C.c_longlong, C.c_void_p]),
    'rohm_amass_metrics': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_uint,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'rohm_scene_metrics': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'rohm_traj_rederive': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong] +
                           [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong,
                                               C.c_void_p]),
    'rohm_clips_scratch_bytes': (C.c_size_t, [C.c_int, C.c_int]),
    'rohm_clips_build': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_double] +
                         [C.c_void_p] * 8 + [C.c_size_t, C.c_void_p]),
    'rohm_clips_build_f64': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_double] +
                             [C.c_void_p] * 9 + [C.c_size_t, C.c_void_p]),
    'rohm_clips_repr': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 +
                        [C.c_size_t, C.c_void_p]),
    'rohm_smplx_param_noise': (C.c_int, [C.c_void_p] * 5 + [C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]),
    'rohm_repr_stats_scratch_bytes': (C.c_size_t, [C.c_longlong]),
    'rohm_repr_stats': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_amass_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5),
    'rohm_amass_preprocess': (C.c_int, [C.c_void_p] * 9 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rohm_keypoints_undistort': (C.c_int, [C.c_void_p, C.c_longlong, c_double_p, c_double_p, C.c_double, C.c_void_p,
                                           C.c_void_p]),
    'rohm_visibility_masks': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    'rohm_depth_workspace_bytes': (C.c_size_t, [C.c_int] * 4),
    'rohm_depth_render': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, c_float_p] + [C.c_double] * 4 +
                          [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_depth_probe': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, c_float_p] + [C.c_double] * 4 +
                         [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'rohm_project_pixels': (C.c_int, [C.c_void_p, c_double_p, c_double_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'rohm_joint_occlusion_mask': (C.c_int, [C.c_void_p, c_double_p, c_double_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                            C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'rohm_vertex_normals': (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p]),
    'rohm_color_workspace_bytes': (C.c_size_t, [C.c_int] * 4),
    'rohm_color_render': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, c_float_p] + [C.c_double] * 4 +
                          [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                           C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rohm_skeleton_mesh': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rohm_image_requantize': (C.c_int, [C.c_void_p, C.c_float, C.c_longlong, C.c_void_p, C.c_void_p]),
    'rohm_image_paste': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    'rohm_image_overlay': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    'rohm_image_flip_lr': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'rohm_train_cond': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                  C.c_void_p, c_int64_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rohm_train_traj_window': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'rohm_adamw_limits': (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'rohm_adamw_step': (C.c_int, [C.POINTER(C.c_void_p)] * 4 + [C.POINTER(C.c_longlong), C.c_int] + [C.c_double] * 5 +
                        [C.c_longlong, C.c_void_p, C.c_void_p]),
    'rohm_grad_norm_scratch_bytes': (C.c_size_t, [C.c_longlong, C.c_int]),
    'rohm_grad_norm': (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p]),
    'rohm_result_rows': (C.c_int, [C.POINTER(ResultRowsItem), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'rohm_traj_report': (C.c_int, [C.c_void_p] * 6 + [C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p,
                                                       C.c_void_p, C.c_void_p]),
    'rohm_export_smplx': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong] + [C.c_void_p] * 6 +
                          [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rohm_export_smplx_blend': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong] + [C.c_void_p] * 9 +
                                [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rohm_track_resample': (C.c_int, [C.c_void_p] * 6 + [C.c_double] + [C.c_int] * 5 + [C.c_void_p] * 6),
    'rohm_track_quality': (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_float, C.c_void_p] + [C.c_double] * 4 +
                           [C.c_void_p, C.c_float] + [C.c_void_p] * 6),
    'rohm_floor_clearance': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    'rohm_floor_candidates': (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_float, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    'rohm_floor_hypotheses': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double] +
                              [C.c_void_p] * 4),
    'rohm_floor_moments': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    'rohm_fit_pose': (C.c_int, [C.c_void_p] * 7 + [C.c_double, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4),
    'rohm_fit_shape_moments': (C.c_int, [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 3),
    # include/rohm_multiview.h
    'rohm_mv_limits': (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'rohm_mv_triangulate': (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_double] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 6),
    'rohm_mv_residuals': (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_double, C.c_void_p, C.c_void_p]),
    # include/rohm_fit_views.h
    'rohm_fit_views_pose': (C.c_int, [C.c_void_p] * 7 + [C.c_double] * 4 + [C.c_int] * 4 + [C.c_void_p] * 5),
    # include/rohm_rig.h
    'rohm_rig_pair_ws_bytes': (C.c_longlong, [C.c_int, C.c_longlong]),
    'rohm_rig_ba_ws_bytes': (C.c_longlong, [C.c_int, C.c_longlong]),
    'rohm_rig_pair_hypotheses': (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_double] * 2 + [C.c_void_p] * 5),
    'rohm_rig_pair_moments': (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_double] * 2 + [C.c_void_p] * 3),
    'rohm_rig_ba_moments': (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_double] * 3 + [C.c_void_p] * 5),
    'rohm_rig_ba_update': (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_double] * 3 + [C.c_void_p] * 3),
}

# include/provisional/: headers written to the standard of HEADERS whose declarations have no case in the contract registries of
# tests/ yet (tests/header_cases.py); their own tests hold them to the contracts until they move up.  lib() applies these rows after
# SIGNATURES under the same strict rule.
PROVISIONAL_HEADERS = ('rohm_sync.h',)

PROVISIONAL_SIGNATURES = {
    # include/provisional/rohm_sync.h
    'rohm_sync_ws_bytes': (C.c_longlong, [C.c_int, C.c_longlong]),
    'rohm_sync_pair_sweep': (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_double] * 3 + [C.c_void_p] * 3),
    'rohm_sync_resample': (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_void_p] * 2),
}


def lib():
    """Load (once) and return the ctypes library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RohmHipError(
                f'{LIB_PATH} not found: the HIP extension is required (no CPU fallback). '
                f'Build it with `python -m rohm_amd.build` (needs hipcc, --offload-arch=gfx950).')
        handle = C.CDLL(LIB_PATH)
        # the shipped library must export every declared symbol; an experiment library selected through ROHM_HIP_LIB (same-box A/B
        # runs against an older tree, scripts/build_variant.py) may lack the newest ones -- they then fail where they are used
        strict = not os.environ.get('ROHM_HIP_LIB')
        for name, (res, args) in list(SIGNATURES.items()) + list(PROVISIONAL_SIGNATURES.items()):
            if not strict and not hasattr(handle, name):
                continue
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what=''):
    if rc != 0:
        msg = lib().rohm_last_error()
        raise RohmHipError(f'{what} failed (code {rc}): {msg.decode() if msg else "?"}')


def ptr(t):
    """Device pointer of a contiguous fp32/int64 HIP tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RohmHipError('rohm_amd kernels need tensors on a HIP device (got CPU tensor); '
                           'there is no CPU fallback')
    if not t.is_contiguous():
        raise RohmHipError('rohm_amd kernels need contiguous tensors')
    return C.c_void_p(t.data_ptr())


def ptr_rows(t):
    """Device pointer of a row-major 2-D HIP tensor whose rows are dense but whose row stride may exceed the row length (a view into
    a larger matrix: the entry points that take a leading dimension); None -> NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RohmHipError('rohm_amd kernels need tensors on a HIP device (got CPU tensor); '
                           'there is no CPU fallback')
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RohmHipError('rohm_amd kernels need row-major matrices with dense rows')      # the row stride is the library's to judge
    return C.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_hip(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RohmHipError('this operator only runs on an AMD GPU through librohm_hip.so; '
                               'got a CPU tensor and there is deliberately no CPU fallback')


def hip_tensor(x, name, kernels):
    """x, if it is a torch tensor on a HIP device; `kernels` is the caller's phrase for who asks ('the fit kernels take')."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f'{name}: {kernels} torch tensors on a HIP device, got {type(x).__name__}')
    require_hip(x)
    return x


def hip_rows(x, name, shape, kernels):
    """x (None stays None) as a contiguous float64 HIP tensor of exactly `shape`."""
    if x is None:
        return None
    x = hip_tensor(x, name, kernels).detach().double().contiguous()
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f'{name} must be {list(shape)}, got {list(x.shape)}')
    return x


UP_AXIS = {'z': 2, 'y': 1}


def up_index(up_axis):
    """'z' or 'y' -> the coordinate index the floor and quality kernels take as up_axis."""
    if up_axis not in UP_AXIS:
        raise ValueError(f"up_axis must be 'z' or 'y', got {up_axis!r}")
    return UP_AXIS[up_axis]


def npz_dict(source):
    """The arrays of an .npz path (no pickles), or a copy of a mapping."""
    if isinstance(source, (str, os.PathLike)):
        import numpy as np
        with np.load(source, allow_pickle=False) as f:
            return {k: f[k] for k in f.files}
    return dict(source)


def profile_start(step_stride=1):
    check(lib().rohm_profile_start(step_stride), 'rohm_profile_start')


def profile_stop():
    """-> {label: dict(launches, total_ms, flops, bytes)} measured with HIP events on the launch stream."""
    rows = (ProfileRow * 256)()
    n = C.c_int(0)
    check(lib().rohm_profile_stop(rows, 256, C.byref(n)), 'rohm_profile_stop')
    return {rows[i].name.decode(): dict(launches=int(rows[i].launches), total_ms=rows[i].total_ms,
                                        flops=rows[i].flops, bytes=rows[i].bytes) for i in range(n.value)}
