"""ctypes mirror of include/adafortitran_amd.h (structs + state_dict -> pointer table).

Kept free of any library loading so that both the product loader (_lib.py) and the
test-side oracle wrapper (oracle/oracle.py) can share the struct definitions.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Optional

AFT_ABI_VERSION = 10
AFT_ENGINE_PACKED, AFT_ENGINE_GENERAL = 0, 1
AFT_OK, AFT_ERR_ARG, AFT_ERR_SHAPE, AFT_ERR_HIP = 0, 1, 2, 3
AFT_ACT_RELU, AFT_ACT_GELU = 0, 1
AFT_ENCODER_AUTO, AFT_ENCODER_LAUNCHES, AFT_ENCODER_PLANE = 0, 1, 2
AFT_PRECISION_F32, AFT_PRECISION_BF16X3 = 0, 1

_fp = C.c_void_p  # const float* -- kept untyped so torch data_ptr() ints and numpy ptrs both fit


class AftConfig(C.Structure):
    _fields_ = [
        ("num_scs", C.c_int32), ("num_symbols", C.c_int32),
        ("pilot_scs", C.c_int32), ("pilot_symbols", C.c_int32),
        ("patch_scs", C.c_int32), ("patch_symbols", C.c_int32),
        ("num_layers", C.c_int32), ("model_dim", C.c_int32), ("num_head", C.c_int32),
        ("activation", C.c_int32), ("adaptive", C.c_int32),
        ("hidden", C.c_int32 * 3), ("encoder_path", C.c_int32), ("precision", C.c_int32),
    ]

    @property
    def tokens(self) -> int:
        return (self.num_scs // self.patch_scs) * (self.num_symbols // self.patch_symbols)


LAYER_FIELDS = ("in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "lin1_w", "lin1_b",
                "lin2_w", "lin2_b", "norm1_w", "norm1_b", "norm2_w", "norm2_b")
#: nn.TransformerEncoderLayer parameter names in LAYER_FIELDS order
LAYER_PARAM_NAMES = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
                     "self_attn.out_proj.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
                     "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")


class AftLayerWeights(C.Structure):
    _fields_ = [(n, _fp) for n in LAYER_FIELDS]


class AftLayerGrads(C.Structure):
    _fields_ = [(n, _fp) for n in LAYER_FIELDS]


class AftStepControl(C.Structure):
    """aft_step_control: 32 bytes of device memory between the preparation launch and the Adam launch (optim.py keeps it as
    eight int32 words and views the float fields)."""
    _fields_ = [("skip", C.c_int32), ("step", C.c_int32), ("grad_scale", C.c_float), ("inv_bc1", C.c_float),
                ("inv_sqrt_bc2", C.c_float), ("grad_norm", C.c_float), ("clip_coef", C.c_float), ("reserved", C.c_int32)]


AFT_CHANSIM_MAX_TAPS, AFT_CHANSIM_MAX_RAYS, AFT_CHANSIM_MAX_VALUES = 32, 16, 16
AFT_CHANSIM_MAX_PILOT_SCS, AFT_CHANSIM_MAX_PILOT_SYMBOLS = 64, 16
AFT_CHANSIM_MAX_GROUP = 16
AFT_CHANSIM_MAX_SLOTS = 4096
AFT_LMMSE_MAX_WINDOW_PILOTS = 32
AFT_LINK_RATE_1_2, AFT_LINK_RATE_2_3, AFT_LINK_RATE_3_4 = 0, 1, 2
AFT_LINK_CODE_MAX_INFO_BITS = 4090
AFT_LINK_LDPC_Z, AFT_LINK_LDPC_MAX_EDGES = 64, 160
AFT_LINK_MAX_BRANCHES = 8
AFT_LINK_MAX_STREAMS = 2
AFT_LINK_PAIR_TIME, AFT_LINK_PAIR_FREQUENCY = 0, 1
AFT_LINK_MAX_SUBBANDS = 1024
AFT_LINK_OBSERVE_DECIDED, AFT_LINK_OBSERVE_SENT = 0, 1
AFT_LINK_HARQ_MAX_ROUNDS, AFT_LINK_HARQ_COUNTS = 4, 7


class AftChanSim(C.Structure):
    """aft_chansim: the channel simulator's configuration, by value (chansim.ChannelSimConfig.tables() fills it)."""
    _fields_ = [
        ("num_scs", C.c_int32), ("num_symbols", C.c_int32), ("pilot_scs", C.c_int32), ("pilot_symbols", C.c_int32),
        ("taps", C.c_int32), ("rays", C.c_int32), ("n_snr", C.c_int32), ("n_ds", C.c_int32), ("n_dop", C.c_int32),
        ("reserved", C.c_int32),
        ("subcarrier_spacing_hz", C.c_double), ("symbol_period_s", C.c_double),
        ("tap_delay", C.c_float * AFT_CHANSIM_MAX_TAPS), ("tap_amp", C.c_float * AFT_CHANSIM_MAX_TAPS),
        ("snr_db", C.c_float * AFT_CHANSIM_MAX_VALUES), ("noise_sigma", C.c_float * AFT_CHANSIM_MAX_VALUES),
        ("delay_spread_ns", C.c_float * AFT_CHANSIM_MAX_VALUES), ("doppler_hz", C.c_float * AFT_CHANSIM_MAX_VALUES),
        ("pilot_sc_index", C.c_int32 * AFT_CHANSIM_MAX_PILOT_SCS), ("pilot_symbol_index", C.c_int32 * AFT_CHANSIM_MAX_PILOT_SYMBOLS),
    ]


class AftLmmse(C.Structure):
    """aft_lmmse: the LMMSE baseline's plan, by value (lmmse.LmmseTables.to_struct() fills it)."""
    _fields_ = [
        ("num_scs", C.c_int32), ("num_symbols", C.c_int32), ("pilot_scs", C.c_int32), ("pilot_symbols", C.c_int32),
        ("n_snr", C.c_int32), ("n_ds", C.c_int32), ("n_dop", C.c_int32),
        ("fixed_snr", C.c_int32), ("fixed_ds", C.c_int32), ("fixed_dop", C.c_int32),
        ("snr_db", C.c_float * AFT_CHANSIM_MAX_VALUES), ("delay_spread_ns", C.c_float * AFT_CHANSIM_MAX_VALUES),
        ("doppler_hz", C.c_float * AFT_CHANSIM_MAX_VALUES), ("noise_var", C.c_float * AFT_CHANSIM_MAX_VALUES),
    ]


class AftLink(C.Structure):
    """aft_link: the link-level error count's configuration, by value (linksim.LinkConfig.to_struct() fills it)."""
    _fields_ = [
        ("num_scs", C.c_int32), ("num_symbols", C.c_int32), ("pilot_scs", C.c_int32), ("pilot_symbols", C.c_int32),
        ("bits_per_symbol", C.c_int32), ("reserved", C.c_int32),
        ("pilot_sc_index", C.c_int32 * AFT_CHANSIM_MAX_PILOT_SCS), ("pilot_symbol_index", C.c_int32 * AFT_CHANSIM_MAX_PILOT_SYMBOLS),
    ]


class AftWeights(C.Structure):
    _fields_ = [
        ("up_w", _fp), ("up_b", _fp),
        ("enh_w", _fp * 4), ("enh_b", _fp * 4),
        ("ref_w", _fp * 4), ("ref_b", _fp * 4),
        ("ada_w", (_fp * 3) * 3), ("ada_b", (_fp * 3) * 3),
        ("lin1_w", _fp), ("lin1_b", _fp),
        ("pos", _fp),
        ("lin2_w", _fp), ("lin2_b", _fp),
        ("layers", C.POINTER(AftLayerWeights)),     # host array of num_layers entries (any layer count)
    ]


def make_config(*, ofdm, pilot, patch, num_layers: int, model_dim: int, num_head: int,
                activation: str = "gelu", adaptive_hidden=None) -> AftConfig:
    cfg = AftConfig()
    cfg.num_scs, cfg.num_symbols = int(ofdm[0]), int(ofdm[1])
    cfg.pilot_scs, cfg.pilot_symbols = int(pilot[0]), int(pilot[1])
    cfg.patch_scs, cfg.patch_symbols = int(patch[0]), int(patch[1])
    cfg.num_layers, cfg.model_dim, cfg.num_head = int(num_layers), int(model_dim), int(num_head)
    cfg.activation = AFT_ACT_GELU if activation == "gelu" else AFT_ACT_RELU
    cfg.adaptive = 1 if adaptive_hidden is not None else 0
    for i in range(3):
        cfg.hidden[i] = int(adaptive_hidden[i]) if adaptive_hidden is not None else 0
    return cfg


def config_from_pydantic(system_config, model_config, adaptive: bool) -> AftConfig:
    return make_config(
        ofdm=(system_config.ofdm.num_scs, system_config.ofdm.num_symbols),
        pilot=(system_config.pilot.num_scs, system_config.pilot.num_symbols),
        patch=tuple(model_config.patch_size), num_layers=model_config.num_layers,
        model_dim=model_config.model_dim, num_head=model_config.num_head,
        activation=model_config.activation,
        adaptive_hidden=tuple(model_config.channel_adaptivity_hidden_sizes) if adaptive else None)


_ENC = ("snr_encoder", "ds_encoder", "dop_encoder")
_TE = "transformer_encoder"


def make_weights(cfg: AftConfig, ptr: Callable[[str], int], pos_key: Optional[str] = None) -> AftWeights:
    """Fill the pointer table from reference ``state_dict`` key names
    (SURVEY.md Appendix A).  ``ptr(key)`` returns the address of that tensor's
    contiguous float32 storage (device address for the HIP library, host address
    for the oracle)."""
    w = AftWeights()
    w.up_w, w.up_b = ptr("pilot_upsampler.weight"), ptr("pilot_upsampler.bias")
    for i, slot in enumerate((0, 2, 4, 6)):
        w.enh_w[i] = ptr(f"initial_enhancer.conv_block.{slot}.weight")
        w.enh_b[i] = ptr(f"initial_enhancer.conv_block.{slot}.bias")
        w.ref_w[i] = ptr(f"final_refiner.conv_block.{slot}.weight")
        w.ref_b[i] = ptr(f"final_refiner.conv_block.{slot}.bias")
    if cfg.adaptive:
        for e, enc in enumerate(_ENC):
            for j, slot in enumerate((0, 2, 4)):
                w.ada_w[e][j] = ptr(f"channel_adapter.{enc}.{slot}.weight")
                w.ada_b[e][j] = ptr(f"channel_adapter.{enc}.{slot}.bias")
    w.lin1_w, w.lin1_b = ptr(f"{_TE}.linear_1.weight"), ptr(f"{_TE}.linear_1.bias")
    w.lin2_w, w.lin2_b = ptr(f"{_TE}.linear_2.weight"), ptr(f"{_TE}.linear_2.bias")
    w.pos = ptr(pos_key or f"{_TE}.positional_encoding.position_embeddings")
    table = (AftLayerWeights * cfg.num_layers)()
    w.layers = C.cast(table, C.POINTER(AftLayerWeights))
    w._layer_table = table          # the struct holds a bare pointer: keep the host array alive with it
    for i in range(cfg.num_layers):
        lp = f"{_TE}.transformer.layers.{i}"
        lw = table[i]
        lw.in_proj_w, lw.in_proj_b = ptr(lp + ".self_attn.in_proj_weight"), ptr(lp + ".self_attn.in_proj_bias")
        lw.out_proj_w, lw.out_proj_b = ptr(lp + ".self_attn.out_proj.weight"), ptr(lp + ".self_attn.out_proj.bias")
        lw.lin1_w, lw.lin1_b = ptr(lp + ".linear1.weight"), ptr(lp + ".linear1.bias")
        lw.lin2_w, lw.lin2_b = ptr(lp + ".linear2.weight"), ptr(lp + ".linear2.bias")
        lw.norm1_w, lw.norm1_b = ptr(lp + ".norm1.weight"), ptr(lp + ".norm1.bias")
        lw.norm2_w, lw.norm2_b = ptr(lp + ".norm2.weight"), ptr(lp + ".norm2.bias")
    return w


def pos_key_of(state: Dict[str, object]) -> str:
    k = f"{_TE}.positional_encoding.position_embeddings"
    return k if k in state else f"{_TE}.positional_encoding.pe"


# ---- the entry points: name -> (restype, argtypes), one line each, in the header's order.  _lib.load_path types the library from this
# table and tests/test_abi.py checks every line of it against the header's prototype (count, kind and order of the arguments, the
# return type, the struct a pointer names).  A new entry point: the header first, then ONE line here; the test says where they disagree.
vp = C.c_void_p
cfgp, wp, lwp, lgp = C.POINTER(AftConfig), C.POINTER(AftWeights), C.POINTER(AftLayerWeights), C.POINTER(AftLayerGrads)
p3, p4, p9, i3 = C.POINTER(vp * 3), C.POINTER(vp * 4), C.POINTER(vp * 9), C.POINTER(C.c_int32 * 3)
i6 = [C.c_int] * 6   # planes, num_scs, num_symbols, patch_scs, patch_symbols, model_dim
SIGNATURES = {
    "aft_version": (C.c_int, []),
    "aft_last_error": (C.c_char_p, []),
    "aft_check_config": (C.c_int, [cfgp]),
    "aft_engine_of": (C.c_int, [cfgp]),
    "aft_set_switch": (C.c_int, [C.c_char_p, C.c_char_p]),
    "aft_get_switch": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t]),
    "aft_max_batch": (C.c_int, [cfgp]),
    "aft_workspace_bytes": (C.c_size_t, [cfgp, C.c_int]),
    "aft_workspace_bytes_layer_fused": (C.c_size_t, [cfgp, C.c_int]),
    "aft_layer_fused_of": (C.c_int, [cfgp, C.c_int]),
    "aft_workspace_lanes": (C.c_int, [cfgp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "aft_workspace_region": (C.c_int, [cfgp, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "aft_forward_f32": (C.c_int, [cfgp, wp, vp, vp, vp, vp, vp, vp, C.c_size_t, C.c_int, vp]),
    "aft_packed_weights_bytes": (C.c_size_t, [cfgp]),
    "aft_pack_weights_f32": (C.c_int, [cfgp, wp, vp, C.c_size_t, vp]),
    "aft_forward_prepacked_f32": (C.c_int, [cfgp, wp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, C.c_int, vp]),
    "aft_linear_forward_f32": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "aft_mse_partial_f32": (C.c_int, [vp, vp, vp, C.c_longlong, vp]),
    # the data formats either side of the path, the channel simulator, the LMMSE baseline, the link-level error count
    "aft_pilot_gather_f32": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "aft_ls_mse_db_f32": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp]),
    "aft_frame_gather_f32": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_longlong, C.c_int, C.c_int, vp]),
    "aft_channel_sim_f32": (C.c_int, [C.POINTER(AftChanSim), C.c_ulonglong] + [C.c_longlong] * 4 + [C.c_int, vp, vp, vp, vp]),
    "aft_channel_sim_group_f32": (C.c_int, [C.POINTER(AftChanSim), C.c_int, C.c_int, vp, C.c_ulonglong] + [C.c_longlong] * 4 +
                                  [C.c_int, vp, vp, vp, vp]),
    "aft_channel_sim_seq_f32": (C.c_int, [C.POINTER(AftChanSim), C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_ulonglong] +
                                [C.c_longlong] * 4 + [C.c_int, vp, vp, vp, vp]),
    "aft_lmmse_table_floats": (C.c_size_t, [C.POINTER(AftLmmse)]),
    "aft_lmmse_f32": (C.c_int, [C.POINTER(AftLmmse), vp, vp, vp, vp, vp, vp, C.c_int, vp]),
    "aft_lmmse_seq_table_floats": (C.c_size_t, [C.POINTER(AftLmmse), C.c_int]),
    "aft_lmmse_seq_f32": (C.c_int, [C.POINTER(AftLmmse)] + [C.c_int] * 4 + [vp, vp, vp, vp, vp, vp, C.c_int, vp]),
    "aft_lmmse_grid_f32": (C.c_int, [C.POINTER(AftLmmse), C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp]),
    "aft_lmmse_classify_table_floats": (C.c_size_t, [C.POINTER(AftLmmse), C.c_int]),
    "aft_lmmse_classify_f32": (C.c_int, [C.POINTER(AftLmmse)] + [C.c_int] * 5 + [vp] * 8 + [C.c_int, vp]),
    "aft_link_errors_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, vp, vp, vp, C.c_int, vp]),
    "aft_link_soft_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp]),
    "aft_link_decode_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_float, vp, vp,
                                      C.c_int, vp]),
    "aft_link_ldpc_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, C.c_int, C.c_int, vp, C.c_ulonglong, C.c_ulonglong, C.c_float, C.c_int,
                                    C.c_int, vp, vp, C.c_int, vp]),
    "aft_link_mrc_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]),
    "aft_link_harq_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_ulonglong, C.c_ulonglong,
                                    C.c_float, C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "aft_link_sm_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]),
    "aft_link_joint_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]),
    "aft_link_alamouti_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]),
    "aft_link_precoded_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp]),
    "aft_link_precoded_delayed_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                vp, vp, vp, vp, C.c_int, vp]),
    "aft_link_sic_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp]),
    "aft_link_cancel_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp,
                                      C.c_int, vp]),
    "aft_link_ldpc_masked_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, C.c_int, C.c_int, vp, C.c_ulonglong, C.c_ulonglong, C.c_float, C.c_int,
                                           C.c_int, vp, C.c_int, vp, vp, C.c_int, vp]),
    "aft_link_observe_f32": (C.c_int, [C.POINTER(AftLink), vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]),
    # training path
    "aft_encoder_tape_bytes": (C.c_size_t, [cfgp, C.c_int]),
    "aft_encoder_train_scratch_bytes": (C.c_size_t, [cfgp, C.c_int]),
    "aft_encoder_layer_fwd_train_f32": (C.c_int, [cfgp, lwp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_float, C.c_uint64, vp]),
    "aft_encoder_layer_fwd_train_chained_f32": (C.c_int, [cfgp, lwp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_float, C.c_uint64,
                                                          C.c_int, lwp, vp, C.c_size_t, C.POINTER(C.c_int), vp]),
    "aft_encoder_layer_bwd_f32": (C.c_int, [cfgp, lwp, vp, vp, C.c_size_t, vp, vp, lgp, C.c_int, vp, C.c_size_t, C.c_int, C.c_float,
                                            C.c_uint64, vp]),
    "aft_dense_fwd_f32": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "aft_dense_bwd_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "aft_dense_bwd_f32": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp]),
    "aft_conv_enhancer_fwd_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "aft_conv_enhancer_fwd_train_f32": (C.c_int, [p4, p4, vp, vp, vp, vp, vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp]),
    "aft_conv_enhancer_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "aft_conv_enhancer_bwd_f32": (C.c_int, [p4, vp, vp, vp, vp, vp, vp, p4, p4, C.c_int, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp]),
    "aft_adapter_fwd_train_f32": (C.c_int, [p3, p9, p9, i3, C.c_int, C.c_int, vp, vp, vp, vp]),
    "aft_adapter_bwd_f32": (C.c_int, [p3, p9, p9, i3, C.c_int, C.c_int, vp, vp, vp, vp, vp, p9, p9, C.c_int, vp]),
    "aft_embed_bwd_scratch_bytes": (C.c_size_t, i6 + [C.c_int]),
    "aft_embed_fwd_train_f32": (C.c_int, [vp] * 6 + i6 + [vp]),
    "aft_embed_bwd_f32": (C.c_int, [vp] * 9 + [C.c_int, vp, C.c_size_t] + i6 + [vp]),
    "aft_tail_bwd_scratch_bytes": (C.c_size_t, i6),
    "aft_tail_fwd_train_f32": (C.c_int, [vp] * 5 + i6 + [vp]),
    "aft_tail_bwd_f32": (C.c_int, [vp] * 6 + [C.c_int, vp, C.c_size_t] + i6 + [vp]),
    # the optimizer step; aft_step_control * stays untyped: optim.py passes the address of a tensor
    "aft_adam_step_f32": (C.c_int, [vp, vp, vp, vp, C.c_size_t] + [C.c_float] * 6 + [C.c_int, vp]),
    "aft_grad_sumsq_scratch_bytes": (C.c_size_t, [C.c_size_t]),
    "aft_grad_sumsq_f32": (C.c_int, [vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp]),
    "aft_adam_prepare_f32": (C.c_int, [vp, vp, vp, vp, C.c_double, C.c_double, C.c_float, C.c_float, vp]),
    "aft_adam_step_ctrl_f32": (C.c_int, [vp, vp, vp, vp, C.c_size_t] + [C.c_float] * 5 + [vp, vp]),
    "aft_grad_clip_f32": (C.c_int, [vp, C.c_size_t, vp, C.c_double, C.c_double, vp, vp]),
    # per-stage entry points, measurement and test hooks
    "aft_stage_upsample_f32": (C.c_int, [cfgp, wp, vp, vp, C.c_int, vp]),
    "aft_stage_adapter_f32": (C.c_int, [cfgp, wp, vp, vp, vp, vp, C.c_int, vp]),
    "aft_stage_embed_f32": (C.c_int, [cfgp, wp, vp, vp, vp, C.c_int, vp]),
    "aft_stage_encoder_layer_f32": (C.c_int, [cfgp, wp, C.c_int, vp, vp, C.c_size_t, C.c_int, vp]),
    "aft_stage_tail_f32": (C.c_int, [cfgp, wp, vp, vp, vp, C.c_int, vp]),
    "aft_profile_kernel_f32": (C.c_int, [cfgp, wp, C.c_int, vp, vp, C.c_size_t, C.c_int, C.c_int, vp]),
    "aft_debug_fill_lds_f32": (C.c_int, [C.c_float, vp]),
    "aft_debug_peek_lds_f32": (C.c_int, [vp, C.c_int, C.c_int, vp]),
}
#: every symbol include/adafortitran_amd.h declares (tests check the .so exports them all)
EXPORTED_SYMBOLS = tuple(SIGNATURES)
REGION_IDS = {"conv_enhanced": 0, "tokens6": 1, "enc_out": 2}   # aft_workspace_region
KERNEL_IDS = {"upsample": 0, "embed": 1, "qkv": 2, "attention": 3, "chain": 4, "tail": 5, "chain_last": 6, "prologue": 8}
