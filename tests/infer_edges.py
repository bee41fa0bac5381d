"""The inference encoder layer at token counts on and around the edges of its attention and chain kernels (helper module: no tests
here; tests/test_infer_token_edges.py and tools/debug/infer_edges_vs_fp64.py run it).

One layer through ``HipEngine.stage_encoder_layer`` -- the launch sequence chain(qkv), attention, chain(mlp) on the packed engine,
``general_layer`` off it -- against ``dropout_reference.reference_layer`` in float64 on the CPU, with the same formulas in float32 on
the GPU as the rounding yardstick.  x and the layer's twelve tensors come from ``dropout_reference.make_case`` (non-trivial biases and
LayerNorm parameters, the seed fixed by the shape) and overwrite layer 0 of a ``synth.make_state_dict`` model, so the kernels and
the reference read the same float32 bits.

Where the inference attention (csrc/attn_device.h, attn16_device.h) treats token counts differently:

  tokens % 8 == 0      padded keys masked in whole 8-key groups by a wave-uniform test; otherwise lane by lane
  ragged last tile     whole 16-key and 8-key MFMA sub-steps past the last key are skipped; V^T columns zeroed apart from the scores
  tokens % 4 != 0      the chain epilogue stores the last V^T group one token at a time
  280, 1120            the token count is a compile-time constant (attn_kernel<32, 280>, <32, 1120>, attn16_kernel<280>, <280, 8>);
                       every other count, their neighbours included, takes the run-time instantiation

The matrix.  Token count N is the grid (3 N, 2) at patch 3 x 2; 1120 tokens is (240, 28).  gelu and 2 planes unless noted.

  (d, heads)   engine    what the row reaches                                  tokens
  (128, 4)     packed    head dim 32: attn_kernel<32, *>, chain at D = 128     TOKENS_128_4; relu at 33, 280, 1120; 6 planes at 33, 97
                                                                               (global row tiles straddle three plane boundaries)
  (128, 2)     packed    head dim 64                                           TOKENS_FAMILY
  (128, 8)     packed    head dim 16: attn16_kernel                            TOKENS_FAMILY
  (128, 16)    packed    head dim 8                                            TOKENS_FAMILY
  (96, 4)      packed    head dim 24                                           TOKENS_FAMILY
  (160, 4)     packed    head dim 40                                           TOKENS_FAMILY
  (192, 4)     packed    head dim 48                                           TOKENS_FAMILY
  (256, 8)     packed    chain at D = 256                                      TOKENS_FAMILY; relu at 33, 280
  (64, 2)      packed    two-wave chain                                        TOKENS_FAMILY
  (32, 1)      packed    one-wave chain                                        TOKENS_FAMILY
  (384, 4)     general   general_layer through the same entry point            TOKENS_GENERAL
  (200, 8)     general   the same, head dim 25                                 TOKENS_GENERAL
"""
import functools

import torch

import dropout_reference as R
from adafortitran_amd import _abi, synth

# on and around the 8-key groups, the 16-key halves, tokens % 4 and the two compile-time counts
TOKENS_128_4 = [31, 32, 33, 39, 40, 41, 47, 48, 49, 63, 64, 65, 96, 97, 210, 279, 280, 281, 288, 289, 1119, 1120, 1121]
TOKENS_FAMILY = [32, 33, 40, 41, 48, 49, 64, 65, 97, 280, 281]
TOKENS_GENERAL = [32, 33, 97, 281]
PACKED_FAMILIES = [(128, 2), (128, 8), (128, 16), (96, 4), (160, 4), (192, 4), (256, 8), (64, 2), (32, 1)]
GENERAL_FAMILIES = [(384, 4), (200, 8)]
ENGINE_OF = {**{f: "packed" for f in [(128, 4)] + PACKED_FAMILIES}, **{f: "general" for f in GENERAL_FAMILIES}}

# a case: (d, heads, tokens, planes, act)
CASES = (
    [(128, 4, n, 2, "gelu") for n in TOKENS_128_4]
    + [(128, 4, n, 2, "relu") for n in (33, 280, 1120)]
    + [(128, 4, n, 6, "gelu") for n in (33, 97)]
    + [(d, h, n, 2, "gelu") for d, h in PACKED_FAMILIES for n in TOKENS_FAMILY]
    + [(256, 8, n, 2, "relu") for n in (33, 280)]
    + [(d, h, n, 2, "gelu") for d, h in GENERAL_FAMILIES for n in TOKENS_GENERAL])

# what a kernel can get wrong at the last key of a plane (dropout_reference.attention): the inference matrix's own list
DEFECTS = ("last_key_left_out", "phantom_key", "last_value_zeroed")

# The factor over the float32 composite's own error, as on the training path (dropout_reference.EDGE_FACTOR).  The CPU separation
# test caps it: every planted defect has to move the layer's output by at least SEPARATION x the bound at every family and count.
FACTOR = R.EDGE_FACTOR
SEPARATION = 10.0


def grid_of(tokens):
    return (240, 28) if tokens == 1120 else R.edge_grid(tokens)


def seed_of(case):
    """Fixed by the shape, as dropout_reference.edge_case does."""
    d, heads, tokens, planes, act = case
    return 7000 + 8 * d + heads + 100003 * tokens + 1009 * planes + (17 if act == "relu" else 0)


def case_id(case):
    d, heads, tokens, planes, act = case
    return f"d{d}h{heads}_{tokens}tok_{planes}pl_{act}"


def spec_of(case):
    d, heads, tokens, planes, act = case
    return dict(ofdm=grid_of(tokens), pilot=(12, 2), patch=(3, 2), num_layers=1, model_dim=d, num_head=heads)


def config_of(case):
    return _abi.make_config(**spec_of(case), activation=case[4])


@functools.lru_cache(maxsize=None)
def inputs(case):
    """x [planes, tokens, d] and the layer's twelve tensors (ABI order), float32 on the CPU: shared, never modified."""
    d, heads, tokens, planes, act = case
    x, _, params = R.make_case(d, heads, tokens, planes, seed_of(case))
    return x, params


def reference(case, dtype=torch.float64, device="cpu", defect=None):
    """The layer in plain torch ops with all-ones masks and keep scale 1: float64 on the CPU is the reference, float32 the
    yardstick.  Returns a float64 CPU tensor [planes, tokens, d]."""
    d, heads, tokens, planes, act = case
    x, params = inputs(case)
    with torch.no_grad():
        y = R.reference_layer(x, params, R.ones_masks(planes, heads, tokens, d), 1.0, heads, act, dtype, device, defect=defect)
    return y.double().cpu()


def limits(e_torch32):
    """(project bound, edge bound), both relative to the float64 output's max; a result has to satisfy both.  The HIP result never
    enters either."""
    return R.bound(R.TOL_FWD, e_torch32), FACTOR * e_torch32 + 1e-6


def hip_layer(case, device="cuda:0"):
    """stage_encoder_layer(0, x) on a one-layer model whose layer 0 holds the case's tensors; float64 CPU tensor."""
    from adafortitran_amd.hip_ops import engine_from_numpy
    d, heads, tokens, planes, act = case
    x, params = inputs(case)
    sd = synth.make_state_dict(**spec_of(case), max_seq_len=max(512, tokens), seed=seed_of(case))
    for name, t in zip(_abi.LAYER_PARAM_NAMES, params):
        key = f"transformer_encoder.transformer.layers.0.{name}"
        assert sd[key].shape == tuple(t.shape), key
        sd[key] = t.numpy()
    eng = engine_from_numpy(config_of(case), sd, device)
    assert eng.tokens == tokens
    y = eng.stage_encoder_layer(0, x.to(device))
    return y.double().cpu()


def figures(case, y, ref, e_torch32):
    """What the test asserts on and the tool records: errors, both bounds and where the largest error sits."""
    err = (y - ref).abs().amax(dim=-1).reshape(-1)            # per global row = plane * tokens + token
    row = int(err.argmax())
    project, edge = limits(e_torch32)
    return dict(e_hip=R.rel_err(y, ref), e_torch32=e_torch32, ratio=R.rel_err(y, ref) / max(e_torch32, 1e-30), project_bound=project,
                edge_bound=edge, worst_row=row, worst_token=row % case[2], worst_plane=row // case[2])


def worst_row_share_in_last_tile(y, ref, tokens):
    """Largest error among the rows of every plane's last 32-token tile over the largest error anywhere else (inf at one tile)."""
    err = (y - ref).abs().amax(dim=-1)                        # [planes, tokens]
    first = (tokens - 1) // 32 * 32
    if first == 0:
        return float("inf")
    return float(err[:, first:].max()) / max(float(err[:, :first].max()), 1e-300)
