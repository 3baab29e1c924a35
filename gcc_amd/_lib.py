"""ctypes binding of libgcc_hip.so (include/gcc_hip.h).  There is NO fallback: if the library is
missing or a call fails, this raises -- the product never routes through PyTorch eager or the
CPU oracle."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('GCC_HIP_LIB') or os.path.join(_HERE, 'libgcc_hip.so')     # GCC_HIP_LIB: another build of the same ABI (A/B runs)

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH = 0, 1, 2, 3
GCC_HIP_ABI = 605       # include/gcc_hip.h GCC_HIP_ABI: the generation of struct layouts / option ids these bindings were written for
WGRAD_GROUP_MAX = 32     # include/gcc_hip.h GCC_WGRAD_GROUP_MAX
CHANSUM_GROUP_MAX = 24   # include/gcc_hip.h GCC_CHANSUM_GROUP_MAX
SPECTRAL_GROUP_MAX = 8    # include/gcc_hip.h GCC_SPECTRAL_GROUP_MAX
CHANSUM_SMALL_MAX_PIXELS = 16384     # include/gcc_hip.h GCC_CHANSUM_SMALL_MAX_PIXELS


class GccError(RuntimeError):
    pass


class conv_plan_t(C.Structure):
    """include/gcc_hip.h gcc_conv_plan_t: the tile plan of a convolution call (every field 0 = the library's default)"""
    _fields_ = [(n, C.c_int) for n in ('tile_families', 'big_min', 'big_nk', 'pair', 'halo_hc', 'wgrad_wgs_big', 'wgrad_wgs')]


PLAN_FIELDS = tuple(n for n, _ in conv_plan_t._fields_)


class conv_t(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('N', 'H', 'W', 'Ci', 'Co', 'KH', 'KW', 'stride', 'pad',
                                       'ldx', 'xoff', 'ldy', 'yoff')] + [('plan', conv_plan_t)]


class wgrad_item_t(C.Structure):
    """include/gcc_hip.h gcc_wgrad_item_t: one entry of a grouped weight gradient"""
    _fields_ = [('c', conv_t), ('x', C.c_void_p), ('dy', C.c_void_p), ('dw', C.c_void_p), ('accumulate', C.c_int)]


class chansum_item_t(C.Structure):
    """include/gcc_hip.h gcc_chansum_item_t"""
    _fields_ = [('x', C.c_void_p), ('ld', C.c_int), ('off', C.c_int), ('C', C.c_int), ('pixels', C.c_size_t), ('out', C.c_void_p),
                ('accumulate', C.c_int)]


class sn_item_t(C.Structure):
    """include/gcc_hip.h gcc_sn_item_t: one layer of a grouped spectral-norm power iteration"""
    _fields_ = [('w_bar', C.c_void_p), ('u', C.c_void_p), ('v', C.c_void_p), ('R', C.c_int), ('C', C.c_int), ('T', C.c_int),
                ('t_out', C.c_void_p), ('sigma_out', C.c_void_p), ('w', C.c_void_p), ('wt', C.c_void_p)]


class sn_eval_item_t(C.Structure):
    """include/gcc_hip.h gcc_sn_eval_item_t: one layer of gcc_spectral_eval_coeffs_group"""
    _fields_ = [('w_bar', C.c_void_p), ('u', C.c_void_p), ('v', C.c_void_p), ('R', C.c_int), ('C', C.c_int), ('T', C.c_int),
                ('t_out', C.c_void_p), ('sigma_out', C.c_void_p), ('gamma', C.c_void_p), ('beta', C.c_void_p),
                ('running_mean', C.c_void_p), ('running_var', C.c_void_p), ('bias', C.c_void_p), ('eps', C.c_float),
                ('pad_', C.c_int), ('scale', C.c_void_p), ('shift', C.c_void_p)]


class epilogue_t(C.Structure):
    _fields_ = [('bias', C.c_void_p), ('act', C.c_int), ('slope', C.c_float), ('stats_partial', C.c_void_p),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('bn', C.c_void_p),
                ('y2', C.c_void_p), ('ldy2', C.c_int), ('y2off', C.c_int), ('y2_mode', C.c_int), ('y2_gate', C.c_void_p)]


class eval_epilogue_t(C.Structure):
    """include/gcc_hip.h gcc_eval_epilogue_t: the eval-mode epilogue of gcc_conv_fprop_eval"""
    _fields_ = [('scale', C.c_void_p), ('shift', C.c_void_p), ('slope', C.c_void_p), ('residual', C.c_void_p),
                ('ld_residual', C.c_int), ('residual_off', C.c_int), ('act', C.c_int), ('pad_', C.c_int),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t)]


EVAL_ACT_NONE, EVAL_ACT_PRELU, EVAL_ACT_TANH = 0, 1, 2     # include/gcc_hip.h GCC_EVAL_ACT_*
EVAL_ACT_RELU, EVAL_ACT_LRELU = 3, 4                       # gcc_conv_eval_ex only


class eval_ex_epilogue_t(C.Structure):
    """include/gcc_hip.h gcc_eval_ex_epilogue_t: the epilogue of gcc_conv_eval_ex (forward / transposed, second output)"""
    _fields_ = [('scale', C.c_void_p), ('shift', C.c_void_p), ('y2', C.c_void_p), ('ldy2', C.c_int), ('y2off', C.c_int),
                ('act', C.c_int), ('act2', C.c_int), ('slope', C.c_float), ('pad_', C.c_int),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t)]


class eval_f32_epilogue_t(C.Structure):
    """include/gcc_hip.h gcc_eval_f32_epilogue_t: the epilogue of gcc_conv_eval_f32 (fp32 in, fp32 out; residual before the act)"""
    _fields_ = [('scale', C.c_void_p), ('shift', C.c_void_p), ('residual', C.c_void_p), ('ld_residual', C.c_int),
                ('residual_off', C.c_int), ('act', C.c_int), ('dilation', C.c_int)]


class eval_f32_act_epilogue_t(C.Structure):
    """include/gcc_hip.h gcc_eval_f32_act_epilogue_t: the epilogue of gcc_conv_eval_f32_act (PReLU by a device slope, tanh, shuffle)"""
    _fields_ = [('scale', C.c_void_p), ('shift', C.c_void_p), ('residual', C.c_void_p), ('ld_residual', C.c_int),
                ('residual_off', C.c_int), ('act', C.c_int), ('shuffle', C.c_int), ('slope', C.c_void_p), ('dilation', C.c_int),
                ('pad_', C.c_int)]


class eval_f32_unet_epilogue_t(C.Structure):
    """include/gcc_hip.h gcc_eval_f32_unet_epilogue_t: the epilogue of gcc_conv_eval_f32_unet (two activated fp32 outputs)"""
    _fields_ = [('scale', C.c_void_p), ('shift', C.c_void_p), ('y2', C.c_void_p), ('ldy2', C.c_int), ('y2off', C.c_int),
                ('act', C.c_int), ('act2', C.c_int), ('slope', C.c_float), ('pad_', C.c_int)]


class eval_f32_resnet_epilogue_t(C.Structure):
    """include/gcc_hip.h gcc_eval_f32_resnet_epilogue_t: the epilogue of gcc_conv_eval_f32_resnet (none / ReLU / tanh)"""
    _fields_ = [('scale', C.c_void_p), ('shift', C.c_void_p), ('act', C.c_int), ('pad_', C.c_int)]


F32_RESNET_REFLECT, F32_RESNET_TRANSPOSED3 = 0, 1           # include/gcc_hip.h GCC_F32_RESNET_*
FID_IN_BF16, FID_IN_U8, FID_IN_F32 = 0, 1, 2               # include/gcc_hip.h GCC_FID_IN_*
POOL3_MAX_S2, POOL3_MAX_S1P1, POOL3_AVG_S1P1 = 0, 1, 2     # include/gcc_hip.h GCC_POOL3_*
DWIN_PLAIN, DWIN_NORM_RELU, DWIN_RESIDUAL = 0, 1, 2        # include/gcc_hip.h GCC_DWIN_*
DW_INORM_WORKSPACE_BYTES = 4096 + (3 << 20)                # include/gcc_hip.h GCC_DW_INORM_WORKSPACE_BYTES
DWIN_PLAN = dict(S=0, S1=1, G=2, rows=3, CG=4, CHg=5, PL=6, tile=7)      # include/gcc_hip.h GCC_DWIN_PLAN_*
# include/gcc_hip.h GCC_CONVBN_PLAN_* (gcc_conv_bn_act_plan); the names from S on exist on route 2 only
CONVBN_PLAN = dict(route=0, ksplit=1, launches=2, S=3, S1=4, G=5, rows=6, CG=7, CHg=8, PL=9, PPT=10)
CONVBN_PLAN_GRID = ('S', 'S1', 'G', 'rows', 'CG', 'CHg', 'PL', 'PPT')
# include/gcc_hip.h GCC_DISTILL_PLAN_* (gcc_distill_plan), in the enum's order
DISTILL_PLAN = ('off_scal', 'off_gf', 'off_gt', 'off_s', 'off_dfg', 'ws_bytes', 'gram_splits', 'gram_kper', 'gram_col_tiles',
                'gram_co_tiles', 'gram_fold', 'bwd_route', 'bwd_bp', 'bwd_bc', 'bwd_ntiles', 'bwd_mtiles', 'fwd_launches',
                'bwd_launches')
KID_TILE, KID_KSTEP = 128, 16                                # include/gcc_hip.h GCC_KID_TILE, GCC_KID_KSTEP (gcc_kid_poly_sum)
# include/gcc_hip.h GCC_PRDC_* (gcc_prdc_kth_dist, gcc_prdc_ball_count)
PRDC_TILE, PRDC_COL_TILE, PRDC_SMALL_TILE, PRDC_SMALL_BELOW, PRDC_KSTEP = 128, 128, 64, 256, 16
PRDC_MAX_K, PRDC_MAX_CHUNKS, PRDC_FILL_WORKGROUPS = 8, 16, 512
IS_TILE, IS_KSTEP, IS_CHUNK = 64, 16, 4096                   # include/gcc_hip.h GCC_IS_* (gcc_is_logits, gcc_is_split_scores)
MAP_MEAN_MAX_SEGMENTS, MAP_MEAN_PIXELS_PER_THREAD = 64, 64   # include/gcc_hip.h GCC_MAP_MEAN_* (gcc_map_mean)


class dw_inorm_t(C.Structure):
    """include/gcc_hip.h gcc_dw_inorm_t: depthwise 3x3 + InstanceNorm in one launch (gcc_dw_inorm_fwd)"""
    _fields_ = [('mode', C.c_int), ('x', C.c_void_p), ('ldx', C.c_int), ('r', C.c_void_p), ('ldr', C.c_int),
                ('u_out', C.c_void_p), ('ldu', C.c_int), ('w', C.c_void_p), ('bias', C.c_void_p), ('y', C.c_void_p),
                ('ldy', C.c_int), ('N', C.c_int), ('H', C.c_int), ('W', C.c_int), ('C', C.c_int), ('eps', C.c_float),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t)]


class bn_eval_item_t(C.Structure):
    """include/gcc_hip.h gcc_bn_eval_item_t: one entry of gcc_bn_eval_coeffs_group"""
    _fields_ = [('gamma', C.c_void_p), ('beta', C.c_void_p), ('running_mean', C.c_void_p), ('running_var', C.c_void_p),
                ('bias', C.c_void_p), ('scale', C.c_void_p), ('shift', C.c_void_p), ('C', C.c_int), ('eps', C.c_float)]


class bnact_t(C.Structure):
    _fields_ = [('scale', C.c_void_p), ('shift', C.c_void_p), ('gate', C.c_void_p), ('gate_after_act', C.c_int),
                ('act', C.c_int), ('slope', C.c_float), ('act2', C.c_int), ('drop_p', C.c_float),
                ('seed', C.c_uint64), ('groups', C.c_int), ('ld_residual', C.c_int), ('residual', C.c_void_p)]


class bn_t(C.Structure):
    _fields_ = [('gamma', C.c_void_p), ('beta', C.c_void_p), ('eps', C.c_float), ('momentum', C.c_float), ('count', C.c_double),
                ('running_mean', C.c_void_p), ('running_var', C.c_void_p), ('mean', C.c_void_p), ('rstd', C.c_void_p),
                ('scale', C.c_void_p), ('shift', C.c_void_p), ('tail_ws', C.c_void_p), ('tail_ws_bytes', C.c_size_t),
                ('finalize_in_launch', C.c_int), ('pad_', C.c_int)]


class bnact_bwd_t(C.Structure):
    _fields_ = [('bn', C.c_int), ('bn_eval', C.c_int), ('mean', C.c_void_p), ('rstd', C.c_void_p),
                ('gamma', C.c_void_p), ('beta', C.c_void_p), ('gate', C.c_void_p), ('gate_after_act', C.c_int),
                ('act', C.c_int), ('slope', C.c_float), ('act2', C.c_int), ('drop_p', C.c_float),
                ('seed', C.c_uint64), ('dgamma', C.c_void_p), ('dbeta', C.c_void_p), ('dalpha', C.c_void_p),
                ('groups', C.c_int), ('flags', C.c_int)]


class adam_tensor_t(C.Structure):
    _fields_ = [('p', C.c_void_p), ('g', C.c_void_p), ('m', C.c_void_p), ('v', C.c_void_p),
                ('numel', C.c_int64), ('l1', C.c_float), ('grad_scale', C.c_float)]


class pack_desc_t(C.Structure):
    _fields_ = [('master', C.c_void_p), ('w', C.c_void_p), ('wt', C.c_void_p), ('rows', C.c_int), ('taps', C.c_int),
                ('cols', C.c_int), ('colsp', C.c_int), ('rowsp', C.c_int), ('row_split', C.c_int),
                ('col_split', C.c_int), ('pad_', C.c_int)]


class pack_item_t(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('tensor', 'kind', 'a', 'b', 'c', 'pad_')]


class adam_chunk_t(C.Structure):
    _fields_ = [('tensor', C.c_int), ('pad_', C.c_int), ('offset', C.c_int64)]


# gcc_set_option ids (enum in include/gcc_hip.h)
(OPT_IGEMM_THIN, OPT_FUSE_BN, OPT_BN_BWD_SMALL, OPT_IGEMM_HALO, OPT_INORM_GRID, OPT_WGRAD_TS, OPT_HALO_XCD_COLS) = range(7)
OPT_COUNT = 7
OPT_NAMES = ('IGEMM_THIN', 'FUSE_BN', 'BN_BWD_SMALL', 'IGEMM_HALO', 'INORM_GRID', 'WGRAD_TS', 'HALO_XCD_COLS')

_P = C.c_void_p
_I = C.c_int
_F = C.c_float
_Z = C.c_size_t

# name -> (restype, argtypes): every symbol include/gcc_hip.h declares
PROTOTYPES = {
    'gcc_strerror': (C.c_char_p, [_I]),
    'gcc_version': (_I, []),
    'gcc_launch_count': (C.c_longlong, [_I]),
    'gcc_device_error': (_I, [_I]),
    'gcc_set_option': (_I, [_I, _I]),
    'gcc_get_option': (_I, [_I]),
    'gcc_options_default': (_I, []),
    'gcc_conv_tile': (_I, [C.POINTER(conv_t), _I]),
    'gcc_conv_stat_tiles': (_I, [C.POINTER(conv_t), _I]),
    'gcc_conv_halo_mode': (_I, [C.POINTER(conv_t), _I, _I]),
    'gcc_conv_route': (_I, [C.POINTER(conv_t), _I, C.POINTER(epilogue_t)]),
    'gcc_conv_y2_supported': (_I, [C.POINTER(conv_t), _I, C.POINTER(epilogue_t)]),
    'gcc_conv_workspace': (_Z, [C.POINTER(conv_t), _I]),
    'gcc_conv_fprop': (_I, [C.POINTER(conv_t), _P, _P, _P, C.POINTER(epilogue_t), _P]),
    'gcc_conv_dgrad': (_I, [C.POINTER(conv_t), _P, _P, _P, C.POINTER(epilogue_t), _P]),
    'gcc_conv_wgrad_workspace': (_Z, [C.POINTER(conv_t)]),
    'gcc_conv_wgrad': (_I, [C.POINTER(conv_t), _P, _P, _P, _I, _P, _Z, _P]),
    'gcc_conv_wgrad_seg': (_I, [C.POINTER(conv_t), _P, _P, _P, _I, _I, _I, _I, _I, _P, _Z, _P]),
    'gcc_conv_wgrad_group_table_bytes': (_Z, []),
    'gcc_conv_wgrad_group_workspace': (_Z, [C.POINTER(wgrad_item_t), _I]),
    'gcc_conv_wgrad_group_prepare': (_I, [C.POINTER(wgrad_item_t), _I, _P, _Z, _P]),
    'gcc_conv_wgrad_group_run': (_I, [_P, _P, _P]),
    'gcc_pack_weights': (_I, [_P, _I, _I, _I, _P, _P, _P]),
    'gcc_pack_weights_multi': (_I, [_P, _P, _I, _P]),
    'gcc_nchw_f32_to_nhwc_bf16': (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    'gcc_nhwc_bf16_to_nchw_f32': (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'gcc_nhwc_copy': (_I, [_P, _I, _I, _P, _I, _I, _I, _I, _Z, _P]),
    'gcc_nhwc_pack_pair': (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _I, _Z, _P]),
    'gcc_nhwc_copy_route': (_I, [_I, _I, _I, _I, _I, _I]),
    'gcc_nhwc_add': (_I, [_P, _I, _I, _P, _I, _I, _I, _Z, _P]),
    'gcc_bn_finalize': (_I, [_P, _I, _I, C.c_double, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P, _P]),
    'gcc_in_finalize': (_I, [_P, _I, _I, _I, C.c_double, _F, _P, _P, _P, _P, _P]),
    'gcc_write_i32': (_I, [_P, _P, _I, _P]),
    'gcc_image_pool_query': (_I, [_P, _P, _P, _P, _I, _Z, _I, _P]),
    'gcc_replay_begin': (_I, [_P]),
    'gcc_replay_end': (_I, [_P, _I]),
    'gcc_replay_run': (_I, [_P]),
    'gcc_replay_tag_next': (_I, [_I]),
    'gcc_replay_patch': (_I, [_P, _I, _I, _P, _Z]),
    'gcc_replay_info': (C.c_longlong, [_P, _I]),
    'gcc_replay_destroy': (_I, [_P]),
    'gcc_event_create': (_I, [_P]),
    'gcc_event_destroy': (_I, [_P]),
    'gcc_event_record': (_I, [_P, _P]),
    'gcc_stream_wait_event': (_I, [_P, _P]),
    'gcc_adam_factors': (_I, [_F, _F, _I, _P]),
    'gcc_inorm_fwd': (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _F, _F, _P, _P, _P, _P, _P, _Z, _P]),
    'gcc_inorm_bwd': (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P, _Z, _P]),
    'gcc_bn_bwd_one_launch': (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _I, _Z, _I, _F, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'gcc_bn_bwd_one_launch_ex': (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _Z, _I, _I, _F, _F, C.c_uint64, _P, _P, _P, _P, _P, _P, _P,
                                      _P, _Z, _P]),
    'gcc_channel_stats_tiles': (_I, [_Z, _I]),
    'gcc_channel_stats': (_I, [_P, _I, _I, _I, _Z, _I, _P, _P]),
    'gcc_reflect_pad': (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    'gcc_dwconv3x3_reflect': (_I, [_I, _P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P]),
    'gcc_dwconv3x3_wgrad_workspace': (_Z, [_I, _I, _I, _I]),
    'gcc_dwconv3x3_reflect_wgrad': (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    'gcc_bn_eval_coeffs': (_I, [_P, _P, _P, _P, _F, _I, _P, _P, _P]),
    'gcc_bn_eval_state': (_I, [_P, _P, _P, _P, _F, _I, _P, _P, _P, _P, _P]),
    'gcc_bnact_fwd': (_I, [C.POINTER(bnact_t), _P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _Z, _P]),
    'gcc_conv_bn_act_workspace': (_Z, [C.POINTER(conv_t), _I]),
    'gcc_conv_fprop_eval': (_I, [C.POINTER(conv_t), _P, _P, _P, C.POINTER(eval_epilogue_t), _P]),
    'gcc_conv_eval_route': (_I, [C.POINTER(conv_t), _Z]),
    'gcc_conv_eval_workspace': (_Z, [C.POINTER(conv_t)]),
    'gcc_bn_eval_coeffs_group': (_I, [_P, _I, _P]),
    'gcc_conv_eval_ex': (_I, [C.POINTER(conv_t), _I, _P, _P, _P, C.POINTER(eval_ex_epilogue_t), _P]),
    'gcc_conv_eval_ex_workspace': (_Z, [C.POINTER(conv_t), _I]),
    'gcc_conv_eval_ex_route': (_I, [C.POINTER(conv_t), _I, _Z]),
    'gcc_conv_eval_f32': (_I, [C.POINTER(conv_t), _P, _P, _P, C.POINTER(eval_f32_epilogue_t), _P]),
    'gcc_conv_eval_f32_route': (_I, [C.POINTER(conv_t), _I]),
    'gcc_conv_eval_f32_kp': (_I, [_I, _I, _I]),
    'gcc_conv_eval_f32_ex': (_I, [C.POINTER(conv_t), _I, _I, _P, _P, _P, C.POINTER(eval_f32_epilogue_t), _P]),
    'gcc_conv_eval_f32_ex_route': (_I, [C.POINTER(conv_t), _I, _I, _I]),
    'gcc_conv_eval_f32_act': (_I, [C.POINTER(conv_t), _I, _I, _P, _P, _P, C.POINTER(eval_f32_act_epilogue_t), _P]),
    'gcc_conv_eval_f32_act_route': (_I, [C.POINTER(conv_t), _I, _I, _I, _I]),
    'gcc_conv_eval_f32_unet': (_I, [C.POINTER(conv_t), _I, _P, _P, _P, C.POINTER(eval_f32_unet_epilogue_t), _P]),
    'gcc_conv_eval_f32_unet_route': (_I, [C.POINTER(conv_t), _I]),
    'gcc_conv_eval_f32_unet_kp': (_I, [_I, _I]),
    'gcc_conv_eval_f32_resnet': (_I, [C.POINTER(conv_t), _I, _P, _P, _P, C.POINTER(eval_f32_resnet_epilogue_t), _P]),
    'gcc_conv_eval_f32_resnet_route': (_I, [C.POINTER(conv_t), _I]),
    'gcc_conv_eval_f32_resnet_kp': (_I, [_I, _I, _I]),
    'gcc_dwconv3x3_reflect_f32': (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    'gcc_inorm_f32_workspace': (_Z, [_I, _I, C.c_longlong]),
    'gcc_inorm_stats_f32': (_I, [_P, _I, _I, _I, _I, _I, _P, _Z, _P]),
    'gcc_inorm_apply_f32': (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _F, _P, _Z, _P]),
    'gcc_nhwc_f32_to_nchw_f32': (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'gcc_nchw_f32_to_nhwc_f32': (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    'gcc_image_to_u8': (_I, [_P, _I, _I, _Z, _P, _P]),
    'gcc_image_to_u8_f32': (_I, [_P, _I, _I, _Z, _P, _P]),
    'gcc_dw_inorm_fwd': (_I, [C.POINTER(dw_inorm_t), _P]),
    'gcc_dw_inorm_route': (_I, [C.POINTER(dw_inorm_t)]),
    'gcc_dw_inorm_plan': (_I, [C.POINTER(dw_inorm_t), _I]),
    'gcc_conv_bn_act': (_I, [C.POINTER(conv_t), _I, _P, _P, _P, C.POINTER(bn_t), C.POINTER(bnact_t), _P, _I, _I, _P, _I, _I, _P, _Z, _P]),
    'gcc_conv_bn_act_plan': (_I, [C.POINTER(conv_t), _I, C.POINTER(bn_t), _I]),
    'gcc_bnact_bwd_workspace': (_Z, [_I, _Z]),
    'gcc_bnact_bwd': (_I, [C.POINTER(bnact_bwd_t), _P, _I, _I, _P, _I, _I, _P, _I, _I, _P, _I, _I, _P, _I, _I,
                           _I, _Z, _P, _Z, _P]),
    'gcc_bnact_bwd_ex': (_I, [C.POINTER(bnact_bwd_t), _I, _F, _P, _I, _I, _P, _I, _I, _P, _I, _I, _P, _I, _I, _P,
                              _I, _I, _I, _Z, _P, _Z, _P]),
    'gcc_channel_sum': (_I, [_P, _I, _I, _I, _Z, _P, _I, _P, _Z, _P]),
    'gcc_channel_sum_workspace': (_Z, [_I, _Z]),
    'gcc_channel_sum_group': (_I, [C.POINTER(chansum_item_t), _I, _P]),
    'gcc_gate_mask': (_I, [_P, _F, _P, _I, _P]),
    'gcc_gan_loss': (_I, [_I, _I, _I, _P, _I, _I, _Z, _F, _P, _I, _P, _P, _Z, _P]),
    'gcc_gan_loss_ex': (_I, [_I, _I, _I, _P, _I, _I, _Z, _P, _P, _F, _P, _I, _P]),
    'gcc_arch_coeffs': (_I, [_P, _P, _P, _P, _F, _P, _P, _P, _P]),
    'gcc_spectral_workspace': (_Z, [_I, _I, _I]),
    'gcc_spectral_power_iteration': (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _Z, _P]),
    'gcc_spectral_power_iteration_pack': (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _Z, _P]),
    'gcc_spectral_group_workspace': (_Z, [C.POINTER(sn_item_t), _I]),
    'gcc_spectral_power_iteration_pack_group': (_I, [C.POINTER(sn_item_t), _I, _P, _Z, _P]),
    'gcc_spectral_eval_coeffs_workspace': (_Z, [C.POINTER(sn_eval_item_t), _I]),
    'gcc_spectral_eval_coeffs_group': (_I, [C.POINTER(sn_eval_item_t), _I, _P, _Z, _P]),
    'gcc_spectral_grad': (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _Z, _P]),
    'gcc_resample_u8': (_I, [_P, _I, _I, _Z, _P, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P]),
    'gcc_crop_flip_normalize': (_I, [_P, _I, _I, _Z, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    'gcc_crop_convert': (_I, [_P, _I, _I, _Z, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P]),
    'gcc_seg_input': (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    'gcc_miou_score': (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P, _P]),
    'gcc_phase_regroup': (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    'gcc_relu_bf16': (_I, [_P, _I, _I, _I, _Z, _P]),
    'gcc_seg_head': (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P]),
    'gcc_seg_head_f32': (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P]),
    'gcc_fid_resize': (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _I, _P]),
    'gcc_pool3x3': (_I, [_I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    'gcc_border_copy': (_I, [_P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    'gcc_global_avgpool': (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P]),
    'gcc_fid_resize_f32': (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _I, _P]),
    'gcc_pool3x3_f32': (_I, [_I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    'gcc_global_avgpool_f32': (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P]),
    'gcc_map_mean_segments': (_I, [_I, _I, _I]),
    'gcc_map_mean_workspace': (_Z, [_I, _I, _I, _I]),
    'gcc_map_mean': (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _Z, _P]),
    'gcc_map_mean_f32': (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _Z, _P]),
    'gcc_argmax_channels': (_I, [_P, _I, _I, _Z, _P, _P]),
    'gcc_confusion_hist': (_I, [_P, _P, _Z, _I, _P, _P]),
    'gcc_psnr_workspace': (_Z, []),
    'gcc_psnr_y_sse': (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _Z, _P]),
    'gcc_ssim_y_sum': (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _Z, _P]),
    'gcc_activation_stats_workspace': (_Z, [_I, _I]),
    'gcc_activation_stats': (_I, [_P, _I, _I, _I, _P, _P, _P, _Z, _P]),
    'gcc_activation_stats_stream_workspace': (_Z, [_I, _I]),
    'gcc_activation_stats_update': (_I, [_P, _I, _I, _I, _I, C.c_longlong, _P, _P, _P, _Z, _P]),
    'gcc_activation_stats_finish': (_I, [_P, C.c_longlong, _I, _P, _P]),
    'gcc_fid_input': (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P]),
    'gcc_frechet_workspace': (_Z, [_I]),
    'gcc_frechet_distance': (_I, [_P, _P, _P, _P, _I, _I, C.c_double, _P, _P, _Z, _P]),
    'gcc_kid_workspace': (_Z, [_I, _I, _I]),
    'gcc_kid_poly_sum': (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _I, _I, _P, _P, _Z, _P]),
    'gcc_prdc_workspace': (_Z, [_I, _I, _I]),
    'gcc_prdc_tile': (_I, [_I, _I]),
    'gcc_prdc_chunks': (_I, [_I, _I]),
    'gcc_prdc_kth_dist': (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _Z, _P]),
    'gcc_prdc_ball_count': (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _I, _P, _I, _I, _P, _P, _Z, _P]),
    'gcc_is_workspace': (_Z, [_I, _I, _I]),
    'gcc_is_logits': (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P]),
    'gcc_is_split_scores': (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _Z, _P]),
    'gcc_attention_fwd': (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _I, _I, _P, _I, _P, _I, _P, _P, _P]),
    'gcc_attention_bwd': (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P]),
    'gcc_attention_infer': (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _I, _I, _P, _I, _P, _Z, _P]),
    'gcc_attention_infer_workspace': (_Z, [_I, _I, _I, _I]),
    'gcc_attention_infer_route': (_I, [_I, _I, _I, _I, _Z]),
    'gcc_attention_infer_f32': (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _I, _I, _P, _I, _P]),
    'gcc_attention_infer_f32_route': (_I, [_I, _I, _I, _I]),
    'gcc_conv_eval_f32_z4': (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P]),
    'gcc_conv_eval_f32_z4_route': (_I, [_I, _I, _I]),
    'gcc_conv_eval_f32_z4_kp': (_I, [_I]),
    'gcc_l1_loss': (_I, [_P, _I, _I, _P, _I, _I, _I, _Z, _F, _P, _I, _P, _I, _I, _P, _Z, _P]),
    'gcc_mse_loss': (_I, [_P, _I, _I, _P, _I, _I, _I, _Z, _F, _P, _I, _P, _I, _I, _P, _Z, _P]),
    'gcc_loss_workspace': (_Z, [_Z, _I]),
    'gcc_prelu': (_I, [_I, _P, _I, _P, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _P, _Z, _P]),
    'gcc_maxpool2x2': (_I, [_I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    'gcc_pool_linear_fwd': (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P]),
    'gcc_pool_linear_bwd': (_I, [_P, _I, _P, _P, _I, _I, _I, _P, _I, _P, _P, _P]),
    'gcc_distill_workspace': (_Z, [_I, _I, _I]),
    'gcc_distill_plan': (_I, [_I, _I, _I, C.POINTER(C.c_longlong)]),
    'gcc_distill_fwd': (_I, [_P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _Z, _P]),
    'gcc_distill_bwd': (_I, [_P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _F, _F, _P, _I, _I, _P, _Z, _P]),
    'gcc_adam_step': (_I, [_P, _P, _I, _I, _F, _F, _F, _F, _I, _P]),
    'gcc_fill_f32': (_I, [_P, _F, _Z, _P]),
    'gcc_add_f32': (_I, [_P, _P, _Z, _P]),
    'gcc_clamp_f32': (_I, [_P, _F, _F, _Z, _P]),
    'gcc_scalar_op': (_I, [_I, _P, _P, _P, _F, _F, _P, _P]),
    'gcc_comm_unique_id': (_I, [_P]),
    'gcc_comm_init': (_I, [C.POINTER(C.c_void_p), _I, _I, _P]),
    'gcc_comm_allreduce_sum_f32': (_I, [_P, _P, _Z, _P]),
    'gcc_comm_allreduce_sum_bf16': (_I, [_P, _P, _Z, _P]),
    'gcc_cast_f32_bf16': (_I, [_P, _P, _Z, _P]),
    'gcc_cast_bf16_f32': (_I, [_P, _P, _Z, _P]),
    'gcc_comm_rank': (_I, [_P]),
    'gcc_comm_world': (_I, [_P]),
    'gcc_comm_count': (_I, [_P]),
    'gcc_comm_destroy': (_I, [_P]),
    'gcc_comm_last_error': (C.c_char_p, []),
}

_lib = None


def load():
    """Load the in-tree library; raises GccError when it has not been built (run
    ``python -c 'import __graft_entry__ as g; g.build()'`` or gcc_amd/csrc/build.sh)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GccError('libgcc_hip.so is not built (%s missing): the HIP kernels are the only '
                       'implementation of this path -- build them with gcc_amd/csrc/build.sh' % LIB_PATH)
    # PyTorch-ROCm ships its own HIP runtime: it must be resident first so that this library binds to
    # the same libamdhip64 (and the same device/stream state) instead of initialising a second one
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)      # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    got = lib.gcc_version()
    if got != GCC_HIP_ABI:
        raise GccError('%s was built from another generation of include/gcc_hip.h (gcc_version() = %d, these bindings are '
                       'for GCC_HIP_ABI %d): struct layouts and option ids differ -- rebuild with gcc_amd/csrc/build.sh'
                       % (LIB_PATH, got, GCC_HIP_ABI))
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != 0:
        msg = load().gcc_strerror(rc).decode()
        raise GccError('%s failed: %s (%d)' % (what or 'gcc call', msg, rc))
