// switches.h -- every run-time switch of the library, declared once.  A switch is an "AFT_*" name that selects a kernel variant, a
// split or a fallback path for measurements and A/B comparisons; none changes results beyond summation order -- but AFT_L0_FOLD, which
// also changes rounding: it selects between two algebraically equal forms of layer 0's keys and values -- and the product never sets one.  The library fills the table from the environment ONCE, when it is loaded (names not listed here are ignored: the tools'
// own AFT_BATCH, AFT_REPS, AFT_LIB_PATH ... are not switches); afterwards a switch changes only through aft_set_switch, and an unknown
// name is refused there.  Set to anything = on; switch_int reads the value as atoi() does.
//
// X(id, name, purpose).  The last five are read by the Python module only (through aft_get_switch): the library is the one store.
#pragma once

#define AFT_SWITCHES(X) \
    X(LANES, "AFT_LANES", "1 = never split a forward into lanes; 2 .. 4 = always that many shares (header section \"Lanes\")") \
    X(L0_FOLD, "AFT_L0_FOLD", "0 = layer 0's keys and values by the model_dim-deep product over x0, not from the input features on the prologue's tables (DESIGN.md 4.1)") \
    X(LAYER_FUSED, "AFT_LAYER_FUSED", "0 = never the one-launch-per-layer sequence (k_layer.hip), 1 = wherever its shape is covered (default: where plane-aligned tiles add no round)") \
    X(PROLOGUE_NO_UP, "AFT_PROLOGUE_NO_UP", "measurement: the profiled prologue launch without the pilot upsampler product") \
    X(CONV_NSPLIT, "AFT_CONV_NSPLIT", "1 | 2 | 4 column ranges per plane in the streaming conv kernels (default: by the batch)") \
    X(CONV_BANDED, "AFT_CONV_BANDED", "the banded conv kernel instead of the column- / row-streaming ones") \
    X(CONV_COLUMN_TILES, "AFT_CONV_COLUMN_TILES", "the column-tiled conv path even where a band plan fits; n > 2 = at least n tiles per plane") \
    X(GEMM_BM, "AFT_GEMM_BM", "64 | 96: row tile of the training GEMM (default: by the shape)") \
    X(EMBED_ANY_OLD, "AFT_EMBED_ANY_OLD", "the general engine's own embedding kernel instead of the training path's") \
    X(EMBED_BWD_GENERIC, "AFT_EMBED_BWD_GENERIC", "the vector embedding backward instead of the MFMA one (model_dim 128)") \
    X(TRAIN_UNFUSED_FWD, "AFT_TRAIN_UNFUSED_FWD", "the launch sequence the fused forward chain of a training layer replaced") \
    X(TRAIN_UNFUSED_BWD, "AFT_TRAIN_UNFUSED_BWD", "the launch sequence the fused backward chain of a training layer replaced") \
    X(TRAIN_ATTN_BWD_SPLIT, "AFT_TRAIN_ATTN_BWD_SPLIT", "the two-pass attention backward instead of the one-pass kernel") \
    X(ATTN_BWD_GROUPS, "AFT_ATTN_BWD_GROUPS", "1 | 4 problems per workgroup of the one-pass attention backward (default: by shape)") \
    X(STAMPS, "AFT_STAMPS", "phase stamps printed on the host: the diag variant only (libaft_hip_diag.so, build.build_diag(): -DAFT_DIAG_STAMPS)") \
    X(ALLOW_COMPOSITE, "AFT_ALLOW_COMPOSITE", "1 = run a configuration the kernels do not cover on the PyTorch-ROCm composite") \
    X(TRAIN_NO_FUSED_ENDS, "AFT_TRAIN_NO_FUSED_ENDS", "training: PyTorch's unfold / cat / add around the dense ends, not fused") \
    X(TRAIN_NO_QKV_CHAIN, "AFT_TRAIN_NO_QKV_CHAIN", "training: every layer runs its own in-projection GEMM (no chained tapes)") \
    X(PRECISION, "AFT_PRECISION", "f32 | bf16x3: the estimators' default hip_precision") \
    X(ENCODER_PATH, "AFT_ENCODER_PATH", "auto | launches | plane: aft_config.encoder_path of every HipEngine (`plane`: retired, runs the launches)")

namespace aft {

enum Switch : int {
#define AFT_SWITCH_ID(id, name, purpose) SW_##id,
    AFT_SWITCHES(AFT_SWITCH_ID)
#undef AFT_SWITCH_ID
    kNumSwitches
};

// The read path: atomic loads indexed by the id -- no lock, no allocation.
bool switch_on(Switch s);                 // set (to anything)
int switch_int(Switch s, int dflt);       // atoi of the value, dflt when unset

}  // namespace aft
