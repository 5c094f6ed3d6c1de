"""ctypes binding of libmagbert_hip.so (include/magbert_hip.h).  The HIP library IS the product: importing the
package without it (or calling any operator without a GPU) raises -- there is no CPU fallback."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MB_LIB_DIR: another build of the same library (scripts/build_variant.py -> gpurun_ab/<name>/) for same-box A/B measurements
LIB_PATH = os.path.join(os.environ.get("MB_LIB_DIR") or os.path.join(_HERE, "lib"), "libmagbert_hip.so")

DT_F32, DT_BF16 = 0, 1
GEMM_NT, GEMM_NN, GEMM_TN = 0, 1, 2
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_DROP_RES, EPI_ADD_RES, EPI_DGELU, EPI_ACCUM_F32, EPI_BIAS_F32 = range(7)
# epilogue 1 with another activation in the place of erf-GELU (layout 0 only): C = act'(u), C2 = act(u)
EPI_BIAS_RELU, EPI_BIAS_SWISH, EPI_BIAS_GELU_NEW, EPI_BIAS_MISH = 7, 8, 9, 10
# feed-forward activation of an engine config (hidden_act / ff_activation), by transformers' ACT2FN names; silu is swish
ACT_GELU, ACT_RELU, ACT_SWISH, ACT_GELU_NEW, ACT_MISH = range(5)
ACTIVATIONS = {"gelu": ACT_GELU, "relu": ACT_RELU, "swish": ACT_SWISH, "silu": ACT_SWISH, "gelu_new": ACT_GELU_NEW, "mish": ACT_MISH}
ACT_EPILOGUE = {ACT_GELU: EPI_BIAS_GELU, ACT_RELU: EPI_BIAS_RELU, ACT_SWISH: EPI_BIAS_SWISH, ACT_GELU_NEW: EPI_BIAS_GELU_NEW,
                ACT_MISH: EPI_BIAS_MISH}


def activation_code(name, field):
    """ACT_* of a config's activation name; anything else (a callable included) is not built"""
    if isinstance(name, str) and name in ACTIVATIONS:
        return ACTIVATIONS[name]
    raise NotImplementedError("%s=%r: the feed-forward activations built are %s (and silu = swish)"
                              % (field, name, ", ".join(n for n in ACTIVATIONS if n != "silu")))


class DropKey(C.Structure):
    _fields_ = [("k0", C.c_uint32), ("k1", C.c_uint32), ("thresh", C.c_uint32), ("scale", C.c_float)]


class BertEngineConfig(C.Structure):
    _fields_ = [("vocab_size", C.c_int), ("hidden_size", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int),
                ("intermediate_size", C.c_int), ("max_position", C.c_int), ("type_vocab", C.c_int),
                ("num_labels", C.c_int), ("visual_dim", C.c_int), ("acoustic_dim", C.c_int), ("pad_token_id", C.c_int),
                ("layer_norm_eps", C.c_float), ("mag_layer_norm_eps", C.c_float), ("beta_shift", C.c_float),
                ("hidden_dropout", C.c_float), ("attn_dropout", C.c_float), ("mag_dropout", C.c_float),
                ("dtype", C.c_int), ("max_batch", C.c_int), ("max_seq", C.c_int), ("injection_index", C.c_int),
                ("hidden_act", C.c_int)]
    # mb_bert_config keeps hidden_act as its last field (include/magbert_hip.h), so injection_index lies in front of it in memory;
    # POSITIONAL arguments keep the order in which the fields were added -- hidden_act the 21st, injection_index the 22nd -- so every
    # caller written before the field existed builds the config it always built
    POSITIONAL = tuple(n for n, _ in _fields_ if n != "injection_index") + ("injection_index",)

    def __init__(self, *args, **kw):
        if len(args) > len(self.POSITIONAL):
            raise TypeError("too many initializers")
        super().__init__()
        for name, value in zip(self.POSITIONAL, args):
            setattr(self, name, value)
        for name, value in kw.items():
            if name not in self.POSITIONAL:
                raise TypeError("BertEngineConfig has no field %r" % name)
            setattr(self, name, value)


class XlnetEngineConfig(C.Structure):
    _fields_ = [("vocab_size", C.c_int), ("d_model", C.c_int), ("n_layer", C.c_int), ("n_head", C.c_int), ("d_inner", C.c_int),
                ("num_labels", C.c_int), ("visual_dim", C.c_int), ("acoustic_dim", C.c_int), ("injection_index", C.c_int),
                ("layer_norm_eps", C.c_float), ("mag_layer_norm_eps", C.c_float), ("beta_shift", C.c_float),
                ("dropout", C.c_float), ("summary_last_dropout", C.c_float), ("mag_dropout", C.c_float),
                ("dtype", C.c_int), ("max_batch", C.c_int), ("max_seq", C.c_int), ("ff_activation", C.c_int)]


class HeadLossStruct(C.Structure):
    """mb_head_loss (include/magbert_hip.h): the head's objective with its options; vec a device pointer for the operator entries
    (mb_head_forward_ex / mb_head_backward_ex), a host pointer for the engines' setters"""
    _fields_ = [("kind", C.c_int), ("param", C.c_float), ("vec", C.c_void_p), ("label_smoothing", C.c_float), ("focal_gamma", C.c_float),
                ("has_ignore_index", C.c_int), ("ignore_index", C.c_int)]


def head_loss_struct(kind, param=0.0, vec=None, label_smoothing=None, focal_gamma=None, ignore_index=None):
    """vec: an address (int / c_void_p) or None; None options are neutral"""
    return HeadLossStruct(int(kind), float(param or 0.0), vec, float(label_smoothing or 0.0), float(focal_gamma or 0.0),
                          0 if ignore_index is None else 1, 0 if ignore_index is None else int(ignore_index))


_vp, _i, _f, _sz, _u64, _u32 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_uint64, C.c_uint32
_dk = C.POINTER(DropKey)

# name -> (restype, argtypes): every symbol include/magbert_hip.h declares
PROTOTYPES = {
    "mb_error_string": (C.c_char_p, [_i]),
    "mb_version": (_i, []),
    "mb_make_dropkey": (None, [_u64, _u64, _u32, _f, _dk]),
    "mb_gemm": (_i, [_i, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _f, _dk, _i, _i, _vp]),
    "mb_gemm_grouped_wgrad": (_i, [_i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mb_narrow": (_i, [_i, _vp, _vp, _sz, _vp]),
    "mb_widen": (_i, [_i, _vp, _vp, _sz, _vp]),
    "mb_layernorm_forward": (_i, [_i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _i, _i, _dk, _vp]),
    "mb_layernorm_backward": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _dk, _dk, _vp]),
    "mb_embed_forward": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _i, _i, _i, _dk, _vp]),
    "mb_embed_backward": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i,
                               _i, _dk, _vp]),
    "mb_attention_forward": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _dk, _vp]),
    "mb_attention_backward": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _dk, _vp]),
    "mb_attention_resident_forward": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _dk, _vp, _vp, _vp]),
    "mb_attention_resident_backward": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _dk, _vp, _vp]),
    "mb_head_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _dk, _i, _f, _vp, _vp]),
    "mb_head_backward": (_i, [_i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _dk, _i, _f, _vp, _vp]),
    "mb_head_forward_ex": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _dk, C.POINTER(HeadLossStruct), _vp]),
    "mb_head_backward_ex": (_i, [_i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _dk, C.POINTER(HeadLossStruct), _vp]),
    "mb_bert_set_head_loss_ex": (_i, [_vp, C.POINTER(HeadLossStruct)]),
    "mb_bert_get_head_loss_ex": (_i, [_vp, C.POINTER(HeadLossStruct), _vp, C.POINTER(_i)]),
    "mb_xlnet_set_head_loss_ex": (_i, [_vp, C.POINTER(HeadLossStruct)]),
    "mb_xlnet_get_head_loss_ex": (_i, [_vp, C.POINTER(HeadLossStruct), _vp, C.POINTER(_i)]),
    "mb_bert_set_head_loss": (_i, [_vp, _i, _f, _vp]),
    "mb_bert_get_head_loss": (_i, [_vp, C.POINTER(_i), C.POINTER(_f), _vp, C.POINTER(_i)]),
    "mb_xlnet_set_head_loss": (_i, [_vp, _i, _f, _vp]),
    "mb_xlnet_get_head_loss": (_i, [_vp, C.POINTER(_i), C.POINTER(_f), _vp, C.POINTER(_i)]),
    "mb_attention_tiled_stats_bytes": (_sz, [_i, _i, _i]),
    "mb_attention_tiled_forward": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _dk, _vp, _vp, _vp]),
    "mb_attention_tiled_backward": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _dk, _vp, _vp]),
    "mb_mag_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "mb_mag_forward": (_i, [_i] + [_vp] * 13 + [_f, _dk, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mb_mag_backward": (_i, [_i] + [_vp] * 11 + [_f, _dk] + [_vp] * 14 + [_i, _i, _i, _i, _vp]),
    # test hooks (tests/mag_op_helpers.py): MAG as the engines call it (padded text, caller-kept pad rows, slabs, stored weight gradients)
    "mb_debug_mag_forward_ex": (_i, [_i] + [_vp] * 13 + [_f, _dk, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "mb_debug_mag_slab_bytes": (_sz, [_i, _i]),
    "mb_debug_mag_backward_ex": (_i, [_i] + [_vp] * 7 + [_f, _dk] + [_vp] * 14 + [_i, _i, _i, _i, _i, _i, _i, _vp, _sz, _i,
                                      C.POINTER(_i), _vp]),
    "mb_adamw_step": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _sz, _f, _f, _f, _f, _f, _i, _i, _f, _i, _vp]),
    "mb_bert_create": (_i, [C.POINTER(BertEngineConfig), C.POINTER(_vp)]),
    "mb_bert_destroy": (None, [_vp]),
    "mb_bert_num_tensors": (_i, [_vp]),
    "mb_bert_tensor_info": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_i),
                                 C.POINTER(C.c_int64), C.POINTER(_i)]),
    "mb_bert_param_count": (_sz, [_vp]),
    "mb_bert_decay_count": (_sz, [_vp]),
    "mb_bert_shadow_range": (None, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "mb_bert_workspace_bytes": (_sz, [_vp]),
    "mb_bert_bind": (_i, [_vp, _vp, _vp, _vp, _vp, _sz]),
    "mb_bert_sync_weights": (_i, [_vp, _vp]),
    "mb_bert_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _u64, _u64, _vp, _vp, _vp, _vp]),
    "mb_bert_backward": (_i, [_vp, _vp, _vp, _f, _i, _i, _vp]),
    "mb_bert_sequence_output": (_vp, [_vp]),
    "mb_bert_pooled_output": (_vp, [_vp]),
    "mb_bert_hidden_state": (_vp, [_vp, _i]),
    "mb_bert_set_attention_output": (_i, [_vp, _vp]),
    # test hooks (tests/gemm_op_helpers.py): what mb_gemm / mb_gemm_grouped_wgrad cannot set, and which kernel the last launch used
    "mb_debug_gemm_ex": (_i, [_i, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _f, _dk, _i, _i,
                              _i, _sz, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _f, _f, _f, _f, _f, _i, _i, _f, _vp,
                              C.POINTER(_i), _vp]),
    "mb_debug_gemm_grouped_ex": (_i, [_i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp,
                                      _sz, _i, _i, _f, _f, _f, _f, _f, _i, _i, _f, _vp, _vp]),
    "mb_debug_gemm_last_kernel": (_i, [C.c_char_p, _i]),
    "mb_debug_gemm_grouped_rows": (_i, [_i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "mb_debug_live_rows": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "mb_bert_debug_live_wgrad_launches": (_i, [_vp]),
    "mb_bert_debug_wgrad_dy": (_vp, [_vp, _i, _i, C.POINTER(_i)]),
    "mb_debug_gemm_trace": (_i, [_vp, _i]),
    "mb_debug_attention_trace": (_i, [_vp, _i]),
    "mb_xlnet_attention_probs": (_vp, [_vp, _i, C.POINTER(_i)]),
    "mb_xlnet_attention_probs_into": (_i, [_vp, _i, _vp, _vp]),
    "mb_xlnet_attention_tiled_stats_bytes": (_sz, [_i, _i, _i]),
    "mb_xlnet_attention_tiled_scratch_bytes": (_sz, [_i, _i, _i, _i]),
    "mb_xlnet_attention_tiled_forward": (_i, [_i] + [_vp] * 10 + [_i, _i, _i, _dk, _vp, _vp, _i, _vp, _vp]),
    "mb_xlnet_attention_tiled_backward": (_i, [_i] + [_vp] * 19 + [_i, _i, _i, _dk, _vp, _vp, _vp]),
    "mb_xlnet_attention_forward": (_i, [_i] + [_vp] * 11 + [_i, _i, _i, _dk, _vp, _vp, _i, _vp]),
    "mb_xlnet_attention_backward": (_i, [_i] + [_vp] * 20 + [_i, _i, _i, _dk, _vp, _vp, _vp]),
    "mb_xlnet_set_head_mask": (_i, [_vp, _vp]),
    "mb_xlnet_set_perm_mask": (_i, [_vp, _vp]),
    "mb_xlnet_set_mems": (_i, [_vp, _vp, _i]),
    "mb_xlnet_query_stream_scratch_bytes": (_sz, [_vp, _i, _i, _i]),
    "mb_xlnet_query_stream_state_bytes": (_sz, [_vp, _i, _i]),
    "mb_xlnet_query_stream": (_i, [_vp, _vp, _i, _vp, _sz, _vp, _vp]),
    "mb_bert_mark_grads_zero": (_i, [_vp, _i]),
    "mb_xlnet_mark_grads_zero": (_i, [_vp, _i]),
    "mb_bert_distrust_word_stamps": (_i, [_vp]),
    "mb_bert_word_skip_updates": (_sz, [_vp]),
    "mb_bert_distrust_word_moments": (_i, [_vp]),
    "mb_bert_word_moment_skip_updates": (_sz, [_vp]),
    "mb_bert_word_moment_scans": (_sz, [_vp]),
    "mb_debug_adamw_sweep": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp, _vp, _vp, _sz, _sz, C.c_uint32, _vp]),
    "mb_debug_word_moments_scan": (_i, [_vp, _vp, _vp, _sz, _sz, C.c_uint32, C.c_uint32, _vp]),
    "mb_bert_materialize_grads": (_i, [_vp, _vp]),
    "mb_xlnet_materialize_grads": (_i, [_vp, _vp]),
    "mb_bert_grads_stale": (_i, [_vp]),
    "mb_xlnet_grads_stale": (_i, [_vp]),
    "mb_bert_set_head_mask": (_i, [_vp, _vp]),
    "mb_bert_set_inputs_embeds": (_i, [_vp, _vp]),
    "mb_bert_set_position_ids": (_i, [_vp, _vp]),
    "mb_bert_inputs_embeds_grad": (_vp, [_vp]),
    "mb_bert_backward_outputs": (_i, [_vp, _vp, _vp, _vp]),
    "mb_bert_stage_grad_ranges": (_i, [_vp, _i, C.POINTER(_sz), C.POINTER(_sz), _i]),
    "mb_bert_train_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f,
                                _i, _i, _f, _f, _i, _vp]),
    "mb_bert_stage_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _u64, _u64, _vp, _vp, _vp, _i, _vp]),
    "mb_bert_stage_backward": (_i, [_vp, _f, _i, _i, _vp]),
    "mb_bert_staged_input_ids": (_vp, [_vp]),
    "mb_bert_load_batch": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(_vp), _vp]),
    "mb_bert_graph_stats": (_i, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "mb_bert_set_profiling": (_i, [_vp, _i]),
    "mb_bert_profile_wgrad_us": (_i, [_vp, C.POINTER(_f)]),
    "mb_bert_profile_adamw_us": (_i, [_vp, C.POINTER(_f)]),
    "mb_xlnet_set_inputs_embeds": (_i, [_vp, _vp]),
    "mb_xlnet_inputs_embeds_grad": (_vp, [_vp]),
    "mb_xlnet_model_output": (_vp, [_vp, _vp]),
    "mb_xlnet_backward_outputs": (_i, [_vp, _vp, _vp]),
    "mb_xlnet_set_profiling": (_i, [_vp, _i]),
    "mb_xlnet_profile_wgrad_us": (_i, [_vp, C.POINTER(_f)]),
    "mb_xlnet_profile_adamw_us": (_i, [_vp, C.POINTER(_f)]),
    "mb_xlnet_create": (_i, [C.POINTER(XlnetEngineConfig), C.POINTER(_vp)]),
    "mb_xlnet_destroy": (None, [_vp]),
    "mb_xlnet_num_tensors": (_i, [_vp]),
    "mb_xlnet_tensor_info": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_i),
                                  C.POINTER(C.c_int64), C.POINTER(_i)]),
    "mb_xlnet_param_count": (_sz, [_vp]),
    "mb_xlnet_decay_count": (_sz, [_vp]),
    "mb_xlnet_shadow_range": (None, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "mb_xlnet_workspace_bytes": (_sz, [_vp]),
    "mb_xlnet_bind": (_i, [_vp, _vp, _vp, _vp, _vp, _sz]),
    "mb_xlnet_sync_weights": (_i, [_vp, _vp]),
    "mb_xlnet_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _u64, _u64, _vp, _vp, _vp, _vp]),
    "mb_xlnet_backward": (_i, [_vp, _vp, _vp, _f, _i, _i, _vp]),
    "mb_xlnet_sequence_output": (_vp, [_vp]),
    "mb_xlnet_hidden_state": (_vp, [_vp, _i]),
    "mb_xlnet_train_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f,
                                 _i, _i, _f, _f, _i, _vp]),
    "mb_xlnet_load_batch": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(_vp), _vp]),
    "mb_xlnet_graph_stats": (_i, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "mb_xlnet_trainable_count": (_sz, [_vp]),
    "mb_bert_set_update_map": (_i, [_vp, _i, _i, _vp, _vp]),
    "mb_bert_set_update_decay": (_i, [_vp, _i, _vp]),
    "mb_bert_set_update_values": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mb_bert_update_stats": (_i, [_vp, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_i)]),
    "mb_bert_set_update_frozen": (_i, [_vp, _i, _vp]),
    "mb_bert_freeze_stats": (_i, [_vp, C.POINTER(_sz), C.POINTER(_i), C.POINTER(_i)]),
    "mb_xlnet_set_update_frozen": (_i, [_vp, _i, _vp]),
    "mb_xlnet_freeze_stats": (_i, [_vp, C.POINTER(_sz), C.POINTER(_i), C.POINTER(_i)]),
    "mb_xlnet_set_update_map": (_i, [_vp, _i, _i, _vp, _vp]),
    "mb_xlnet_set_update_decay": (_i, [_vp, _i, _vp]),
    "mb_xlnet_set_update_values": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mb_xlnet_update_stats": (_i, [_vp, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_i)]),
    "mb_grad_clip_scratch_bytes": (_sz, [_sz]),
    "mb_grad_clip_coef": (_i, [_vp, _sz, _f, _f, _vp, _vp, _vp]),
    "mb_bert_set_grad_clip": (_i, [_vp, _f]),
    "mb_bert_grad_clip_stats": (_i, [_vp, C.POINTER(_f), C.POINTER(_f), _vp]),
    "mb_xlnet_set_grad_clip": (_i, [_vp, _f]),
    "mb_xlnet_grad_clip_stats": (_i, [_vp, C.POINTER(_f), C.POINTER(_f), _vp]),
    "mb_xlnet_stage_grad_ranges": (_i, [_vp, _i, C.POINTER(_sz), C.POINTER(_sz), _i]),
    # data parallel (csrc/comm.hip)
    "mb_comm_unique_id": (_i, [_vp]),
    "mb_comm_create_rccl": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "mb_comm_create_callbacks": (_i, [_i, _i, _vp, _vp, _vp, C.POINTER(_vp)]),
    "mb_comm_destroy": (None, [_vp]),
    "mb_comm_rank": (_i, [_vp]),
    "mb_comm_world": (_i, [_vp]),
    "mb_comm_stream": (_vp, [_vp]),
    "mb_comm_scratch_bytes": (_sz, [_i, _i, _sz, _i, _i, _i]),
    "mb_comm_bind_scratch": (_i, [_vp, _vp, _sz, _i, _sz, _i, _i, _i]),
    "mb_comm_all_reduce": (_i, [_vp, _vp, _sz, _vp]),
    "mb_comm_exchange_rows": (_i, [_vp, _vp, _vp, _i, _vp]),
    "mb_comm_set_row_exchange": (_i, [_vp, _i]),
    "mb_comm_set_sharding": (_i, [_vp, _i]),
    "mb_comm_sharding": (_i, [_vp]),
    "mb_comm_join": (_i, [_vp, _vp]),
    "mb_comm_gather_shards": (_i, [_vp, _vp, _i, _vp]),
    "mb_comm_shard_slices": (_i, [_vp, C.POINTER(_sz), _i]),
    "mb_comm_set_timing": (_i, [_vp, _i]),
    "mb_comm_exposed_ms": (_i, [_vp, C.POINTER(_f)]),
    "mb_comm_stats": (_i, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "mb_comm_last_error": (C.c_char_p, []),
    "mb_bert_train_step_dp": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f,
                                   _i, _i, _f, _f, _i, _vp, _vp]),
    "mb_xlnet_train_step_dp": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f,
                                    _i, _i, _f, _f, _i, _vp, _vp]),
}

ALL_REDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
ALL_GATHER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

_lib = None


class MagbertError(RuntimeError):
    pass


def lib():
    """The loaded library.  Raises (never falls back) when the .so is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MagbertError(
                "libmagbert_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(h, name)        # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def check(code):
    if code != 0:
        msg = lib().mb_error_string(code).decode()
        if code == 1005 or 2000 <= code < 2100:
            msg += ": " + (lib().mb_comm_last_error() or b"").decode()
        raise MagbertError("%s (code %d)" % (msg, code))


def ptr(t):
    """device pointer of a tensor (None -> NULL)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def make_dropkey(seed, step, site, p):
    k = DropKey()
    lib().mb_make_dropkey(int(seed) & (2**64 - 1), int(step), int(site), float(p), C.byref(k))
    return k


def no_drop():
    return DropKey(0, 0, 0, 1.0)
