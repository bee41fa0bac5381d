"""The encoder layer's training path at token counts on and around its 32-row tiles (dropout_reference.EDGE_CASES: full last tile,
a tail of one token, whole three-wave rounds, the twelve-wave workgroup's fit at 320 / 321 tokens, one-pass / two-pass attention
backward at 2368 / 2369), against the float64 reference with the kernels' own masks.

GPU: (a) the tape -- log-sum-exp and attention output recomputed in float64 from the float32 qkv block the attention kernel read;
(b) layer output and all thirteen gradients, the A/B variants, two-layer stacks (the chained in-projection on a ragged last tile).
CPU: (c) the bounds of (a) and (b) separate defects planted at the last key / last query from rounding; (d) the library takes
every grid of the matrix.

Bounds.  (a) attention output, relative to max |O|: 4 e_torch32 + 1e-6; LSE, absolute: 4 e_torch32 + 4 float32 spacings at
max |lse|.  (b) per tensor, relative to the float64 tensor's max, BOTH the project bound max(5e-5 | 2e-4 | 3e-4, 2 e_torch32 + 1e-6)
and edge_bound = 4 e_torch32 + 1e-6: one phantom key moves the layer's tensors by about 1 x the project bound at 2400 tokens, so the
project bound alone cannot see it.  e_torch32 = the error of the same formulas in float32 (PyTorch on the GPU); the HIP result never
enters a bound.  tools/debug/token_edges_vs_fp64.py prints every figure; profiles/token_edges_vs_fp64.json holds them."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import dropout_reference as R
from adafortitran_amd import _abi
from train_tape import forward_tape

gpu = pytest.mark.gpu


def _cfg(d, heads, ofdm, act="gelu"):
    return _abi.make_config(ofdm=ofdm, pilot=(12, 2), patch=(3, 2), num_layers=1, model_dim=d, num_head=heads, activation=act)


# ---------------------------------------------------------------- CPU: (d) the grids, (c) the bounds themselves

def test_every_grid_of_the_matrix_passes_the_config_check_cpu():
    """aft_encoder_tape_bytes is host-only and returns 0 for a config check_config refuses."""
    from adafortitran_amd import _lib
    lib = _lib.load()
    shapes = {(c[0], c[1], c[2]) for c in R.EDGE_CASES + R.EDGE_VARIANT_CASES}
    shapes |= {(d, heads, R.edge_grid(tokens)) for d, heads, tokens in R.EDGE_STACKS}
    for d, heads, ofdm in sorted(shapes):
        cfg = _cfg(d, heads, ofdm)
        assert lib.aft_encoder_tape_bytes(C.byref(cfg), 1) != 0, (d, heads, ofdm)


def test_the_matrix_is_the_stated_one_cpu():
    """Token lists, families and probabilities as dropout_reference's table states them; gelu and 2 planes everywhere."""
    E, E4 = [31, 32, 33, 64, 65, 96, 97, 160, 193, 320, 321], [32, 33, 96, 97]
    assert (R.EDGE_TOKENS, R.EDGE_TOKENS_4, R.EDGE_VARIANT_TOKENS, R.EDGE_LDS_TOKENS) == (E, E4, [32, 33, 96, 97, 320], [2368, 2369])
    got = {(c[0], c[1], R.tokens_of(c[2]), c[5]) for c in R.EDGE_CASES}
    want = {(128, 4, n, p) for n in E for p in (0.0, 0.1)}
    want |= {(d, h, n, 0.1) for d, h in ((128, 2), (256, 8)) for n in E}
    want |= {(d, h, n, 0.0) for d, h in ((128, 2), (256, 8)) for n in (32, 33, 97)}
    want |= {(d, h, n, 0.1) for d, h in ((384, 4), (512, 4), (128, 8), (96, 3), (200, 8)) for n in E4}
    want |= {(32, 1, n, p) for n in (2368, 2369) for p in (0.0, 0.1)}
    assert got == want and len(R.EDGE_CASES) == len(want)
    assert all(c[3] == 2 and c[4] == "gelu" for c in R.EDGE_CASES + R.EDGE_VARIANT_CASES)
    assert [(c[0], c[1], R.tokens_of(c[2]), c[5]) for c in R.EDGE_VARIANT_CASES] == [(128, 4, n, 0.1) for n in (32, 33, 96, 97, 320)]
    assert R.EDGE_STACKS == [(128, 4, 33), (128, 4, 97), (256, 8, 33)]


def _tile_local_key_masks(seed, p, planes, heads, tokens, d):
    """Planted defect 4: the keys of the last 32-key tile hash their tile-local index k % 32 where the kernel hashes the key's
    index within the call, problem * tokens + k."""
    first = (tokens - 1) // 32 * 32

    def key_of(ph, keys):
        return np.where(keys >= first, keys % np.uint64(32), keys + np.uint64(ph * tokens))
    return R.layer_masks(seed, p, planes, heads, tokens, d, key_of=key_of)


@pytest.mark.parametrize("d,heads,tokens", [(128, 4, n) for n in R.EDGE_TOKENS] + [(32, 1, 2369)], ids=lambda v: str(v))
def test_bounds_separate_planted_token_edge_defects_from_rounding_cpu(d, heads, tokens):
    """Four defects of the last key / last query, planted one at a time into the float64 reference at p = 0.1: each moves at least
    one tensor that (a) or (b) compares by more than 10 x the bound the GPU test applies to that tensor (the float32 yardstick is
    evaluated on the CPU here).  The last key left out and the last query's detached k / v must be caught by (b), the layer's
    tensors; the phantom key -- about 1 x the project bound at 2400 tokens -- by (a), the tape, at the long count."""
    d_, heads_, ofdm, planes, act, p, in_seed = R.edge_case(d, heads, tokens, 0.1)
    x, gout, ps = R.make_case(d, heads, tokens, planes, in_seed)
    masks, ks = R.layer_masks(R.DROP_SEED, p, planes, heads, tokens, d), float(R.keep_scale(p))
    probe = {}
    out64, g64 = R.reference_grads(x, gout, [ps], [masks], ks, heads, act, probe=probe)
    out32, g32 = R.reference_grads(x, gout, [ps], [masks], ks, heads, act, dtype=torch.float32)
    limits = R.layer_limits(out64, g64, out32, g32)
    assert max(e for e, _, _ in limits) <= 2e-6, "the float32 composite itself is not within rounding of the reference"
    qkv = probe["qkv"].float().numpy().reshape(planes * tokens, 3 * d)          # the bits a tape would hold
    lse64, o64, lim_lse, lim_o, _, _ = R.tape_figures(qkv, masks[0], ks, planes, heads, "cpu")

    def tape_moves(defect, m0):
        lse, o = R.attention_tape(qkv, m0, ks, planes, heads, torch.float64, "cpu", defect=defect)
        return max(float((lse - lse64).abs().max()) / lim_lse, R.rel_err(o, o64) / lim_o)

    def layer_moves(defect, bad_masks):
        out, grads = R.reference_grads(x, gout, [ps], [bad_masks], ks, heads, act, defect=defect)
        errs = [R.rel_err(out, out64)] + [R.rel_err(g, r) for g, r in zip(grads, g64)]
        return max(e / min(project, edge) for e, (_, project, edge) in zip(errs, limits))

    bad4 = _tile_local_key_masks(R.DROP_SEED, p, planes, heads, tokens, d)
    assert not np.array_equal(bad4[0], masks[0])
    moved = {"last_key_left_out": layer_moves("last_key_left_out", masks),
             "last_query_detached_kv": layer_moves("last_query_detached_kv", masks),
             "phantom_key": tape_moves("phantom_key", masks[0]),
             "tile_local_key_word": tape_moves(None, bad4[0])}
    if tokens < 1000:                        # at the short counts (b) sees the phantom key and the wrong mask words as well
        moved["phantom_key, layer"] = layer_moves("phantom_key", masks)
        moved["tile_local_key_word, layer"] = layer_moves(None, bad4)
    print({k: round(v, 1) for k, v in moved.items()})
    assert all(v > 10 for v in moved.values()), moved


# ---------------------------------------------------------------- GPU

@functools.lru_cache(maxsize=None)
def _reference(case):
    """Inputs, masks, float64 reference and float32-on-the-GPU yardstick of one case: computed once, shared, never modified."""
    d, heads, ofdm, planes, act, p, in_seed = case
    tokens = R.tokens_of(ofdm)
    x, gout, ps = R.make_case(d, heads, tokens, planes, in_seed)
    masks, ks = R.case_masks(case)
    out64, g64 = R.reference_grads(x, gout, [ps], [masks], ks, heads, act)
    out32, g32 = R.reference_grads(x, gout, [ps], [masks], ks, heads, act, dtype=torch.float32, device="cuda")
    return x, gout, ps, masks[0], ks, out64, g64, out32, g32


def _compare(label, out, grads, out64, g64, out32, g32, names, tol_grad=R.TOL_GRAD):
    """Print every figure, then hold each tensor to the project bound and to edge_bound."""
    bad = []
    for n, h, r, (e_t32, project, edge) in zip(("out",) + tuple(names), [out] + list(grads), [out64] + list(g64),
                                               R.layer_limits(out64, g64, out32, g32, tol_grad)):
        e_hip = R.rel_err(h, r)
        print(f"{label} {n}: hip {e_hip:.2e} torch32 {e_t32:.2e} project bound {project:.2e} edge bound {edge:.2e}")
        if not (e_hip <= project and e_hip <= edge):
            bad.append(f"{n}: hip {e_hip:.2e} > min({project:.2e}, {edge:.2e}) (torch32 {e_t32:.2e})")
    assert not bad, label + "\n" + "\n".join(bad)


def _check_layer(case, label):
    from adafortitran_amd.training import HipEncoderLayerFunction
    d, heads, ofdm, planes, act, p, in_seed = case
    x, gout, ps, _, _, out64, g64, out32, g32 = _reference(case)
    xs = x.cuda().requires_grad_(True)
    leaves = [q.cuda().requires_grad_(True) for q in ps]
    out = HipEncoderLayerFunction.apply(xs, _cfg(d, heads, ofdm, act), p, R.DROP_SEED, *leaves)
    out.backward(gout.cuda())
    _compare(label, out.detach(), [xs.grad] + [q.grad for q in leaves], out64, g64, out32, g32, R.GRAD_NAMES)


@gpu
@pytest.mark.parametrize("case", R.EDGE_CASES, ids=R.case_id)
def test_tape_lse_and_attention_output_match_float64(case):
    """(a) From the tape of a direct forward call: the qkv block is what the attention kernel read; its base-2 LSE
    ([planes][heads][tokens]) and its output against float64 from the same bits, with the restated site-0 mask -- which this check
    therefore reads at every multi-tile token count."""
    d, heads, ofdm, planes, act, p, in_seed = case
    tokens = R.tokens_of(ofdm)
    x, _, ps, m0, ks = _reference(case)[:5]
    t = forward_tape(_cfg(d, heads, ofdm, act), ps, x, p, R.DROP_SEED)
    lse64, o64, lim_lse, lim_o, e_lse, e_o = R.tape_figures(t["qkv"], m0, ks, planes, heads, "cuda")
    lse = torch.from_numpy(t["lse"].reshape(planes, heads, tokens)).double() * math.log(2.0)
    hip_lse = float((lse - lse64).abs().max())
    hip_o = R.rel_err(torch.from_numpy(t["attn"].reshape(planes, tokens, d)), o64)
    print(f"tape lse: hip {hip_lse:.2e} torch32 {e_lse:.2e} bound {lim_lse:.2e} (max |lse| {float(lse64.abs().max()):.2f}); "
          f"attn: hip {hip_o:.2e} torch32 {e_o:.2e} bound {lim_o:.2e}")
    assert hip_lse <= lim_lse and hip_o <= lim_o


@gpu
@pytest.mark.parametrize("case", R.EDGE_CASES, ids=R.case_id)
def test_layer_matches_float64_at_token_edges(case):
    """(b) HipEncoderLayerFunction: output and all thirteen gradients against the float64 reference with the kernels' own masks."""
    _check_layer(case, "layer")


@gpu
@pytest.mark.parametrize("case", R.EDGE_VARIANT_CASES, ids=R.case_id)
@pytest.mark.parametrize("variant", [{"AFT_TRAIN_UNFUSED_FWD": "1", "AFT_TRAIN_UNFUSED_BWD": "1"}, {"AFT_TRAIN_ATTN_BWD_SPLIT": "1"},
                                     {"AFT_ATTN_BWD_GROUPS": "4"}], ids=["unfused", "attn_bwd_split", "attn_bwd_groups4"])
def test_layer_variants_match_float64_at_token_edges(case, variant, switches):
    """(b) on the kernels behind the A/B switches: the unfused launch sequences, the two-pass attention backward, twelve-wave
    attention-backward workgroups (8 problems; 320 tokens is the largest count that shape takes)."""
    for name, value in variant.items():
        switches.set(name, value)
    _check_layer(case, "+".join(variant))


@gpu
@pytest.mark.parametrize("d,heads,tokens", R.EDGE_STACKS, ids=lambda v: str(v))
def test_stack_matches_float64_at_token_edges(d, heads, tokens):
    """(b) through encoder_stack_train over two layers at p = 0.1 with 2 planes: layer 1's q/k/v come from layer 0's row-local
    kernel, whose last tile is ragged at these token counts (d = 256: the link's GEMM fallback)."""
    from adafortitran_amd.training import encoder_stack_train, layer_params
    ofdm, planes, p, n = R.edge_grid(tokens), 2, 0.1, 2
    ks = float(R.keep_scale(p))
    x, gout, sets = R.make_case(d, heads, tokens, planes, seed=61 + tokens, layers=n)
    torch.manual_seed(99)
    seeds = torch.randint(0, 2 ** 62, (n,), dtype=torch.int64).tolist()
    masks = [R.layer_masks(s, p, planes, heads, tokens, d) for s in seeds]
    out64, g64 = R.reference_grads(x, gout, sets, masks, ks, heads, "gelu")
    out32, g32 = R.reference_grads(x, gout, sets, masks, ks, heads, "gelu", dtype=torch.float32, device="cuda")
    layers = [torch.nn.TransformerEncoderLayer(d_model=d, nhead=heads, dim_feedforward=2 * d, dropout=p, activation="gelu",
                                               batch_first=True).cuda().train() for _ in range(n)]
    with torch.no_grad():
        for layer, ps in zip(layers, sets):
            for q, v in zip(layer_params(layer), ps):
                q.copy_(v)
    xs = x.cuda().requires_grad_(True)
    torch.manual_seed(99)
    out = encoder_stack_train(xs, layers, _cfg(d, heads, ofdm), p)
    out.backward(gout.cuda())
    grads = [xs.grad] + [q.grad for layer in layers for q in layer_params(layer)]
    names = ["dx"] + [f"layers.{i}.{nm}" for i in range(n) for nm in R.GRAD_NAMES[1:]]
    _compare("stack", out.detach(), grads, out64, g64, out32, g32, names, tol_grad=R.TOL_STACK_GRAD)
