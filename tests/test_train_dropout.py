"""The encoder layer's dropout path (the `threshold != 0` branch of every training kernel: the model configs set dropout 0.1)
against a float64 reference that uses the kernels' OWN masks (tests/dropout_reference.py).

CPU: the reference is nn.TransformerEncoderLayer when the masks are all ones; the bounds of the GPU tests separate planted
dropout defects from rounding; the relu cases' inputs keep every pre-activation away from zero.
GPU: (a) the kernels' masks are the restated masks bit for bit, read out of the tape; (b) layer output and all thirteen gradients
per kernel family; (c) the A/B variants; (d) two backward passes accumulated into the same .grad; (e) a three-layer stack.

Bounds of (b) .. (e), per tensor, relative to the float64 tensor's max: max(project bound, 2 * e_torch32 + 1e-6), project bound =
5e-5 forward, 2e-4 gradients (3e-4 through a stack), e_torch32 = the error of the same composite in float32 on the GPU.  The HIP
result never enters a bound.  tools/debug/dropout_vs_fp64.py prints every figure; profiles/dropout_vs_fp64.json holds them."""
import functools

import numpy as np
import pytest
import torch

import dropout_reference as R
from adafortitran_amd import _abi
from train_tape import forward_tape

gpu = pytest.mark.gpu


def _cfg(d, heads, ofdm, act="gelu"):
    return _abi.make_config(ofdm=ofdm, pilot=(12, 2), patch=(3, 2), num_layers=1, model_dim=d, num_head=heads, activation=act)


# ---------------------------------------------------------------- CPU: the reference and the bounds themselves

@pytest.mark.parametrize("d,heads,tokens,act", [(128, 4, 56, "gelu"), (128, 4, 56, "relu"), (96, 3, 28, "gelu"), (96, 3, 28, "relu")])
def test_reference_with_all_ones_masks_is_the_torch_layer_cpu(d, heads, tokens, act):
    """All-ones masks and ks = 1: reference_layer in float64 is nn.TransformerEncoderLayer(dropout=0).double().train() -- output
    and all thirteen gradients to 1e-12 of each tensor's max."""
    from adafortitran_amd.training import layer_params
    planes = 2
    x, gout, ps = R.make_case(d, heads, tokens, planes, seed=41)
    out, grads = R.reference_grads(x, gout, [ps], [R.ones_masks(planes, heads, tokens, d)], 1.0, heads, act)
    layer = torch.nn.TransformerEncoderLayer(d_model=d, nhead=heads, dim_feedforward=2 * d, dropout=0.0, activation=act,
                                             batch_first=True).double().train()
    with torch.no_grad():
        for q, v in zip(layer_params(layer), ps):
            q.copy_(v.double())
    xl = x.double().requires_grad_(True)
    ref = layer(xl)
    ref.backward(gout.double())
    assert R.rel_err(out, ref.detach()) <= 1e-12
    for name, g, r in zip(R.GRAD_NAMES, grads, [xl.grad] + [q.grad for q in layer_params(layer)]):
        assert R.rel_err(g, r) <= 1e-12, name


def _planted(seed, p, planes, heads, tokens, d):
    """(label, tensor it must move, kwargs of reference_grads' layer, masks, keep scales) per planted defect."""
    ks = float(R.keep_scale(p))
    good = R.layer_masks(seed, p, planes, heads, tokens, d)
    transposed = [np.ascontiguousarray(good[0].transpose(0, 1, 3, 2))] + good[1:]
    return [("out_proj bias added outside the dropout", "self_attn.out_proj.bias", dict(bias_outside=(1,)), good, ks),
            ("linear2 bias added outside the dropout", "linear2.bias", dict(bias_outside=(3,)), good, ks),
            ("attention mask transposed (row and column words swapped)", "self_attn.in_proj_weight", {}, transposed, ks),
            ("1/(1-p) omitted at the attention site", "self_attn.in_proj_weight", {}, good, (1.0, ks, ks, ks)),
            ("seeds of sites 1 and 3 exchanged", "self_attn.out_proj.bias", {},
             R.layer_masks(seed, p, planes, heads, tokens, d, sites=(0, 3, 2, 1)), ks),
            ("plane-local row index (row modulo tokens)", "linear1.bias", {},
             R.layer_masks(seed, p, planes, heads, tokens, d, row_of=lambda r: r % np.uint64(tokens)), ks)]


@pytest.mark.parametrize("case", [R.LAYER_CASES[-1], R.LAYER_CASES[0]], ids=["smallest", "default"])
def test_bounds_separate_planted_dropout_defects_from_rounding_cpu(case):
    """Defects the p = 0 tests and the finite-difference check of dx cannot see, planted one at a time into the float64
    reference at the GPU test's smallest and default shapes: each moves the tensor named with it by more than 10 x the bound the
    GPU test applies to that tensor (the float32 yardstick is evaluated on the CPU here)."""
    d, heads, ofdm, planes, act, p, in_seed = case
    tokens = R.tokens_of(ofdm)
    x, gout, ps = R.make_case(d, heads, tokens, planes, in_seed)
    masks, ks = R.layer_masks(R.DROP_SEED, p, planes, heads, tokens, d), float(R.keep_scale(p))
    out, grads = R.reference_grads(x, gout, [ps], [masks], ks, heads, act)
    _, g32 = R.reference_grads(x, gout, [ps], [masks], ks, heads, act, dtype=torch.float32)
    for label, tensor, kw, bad_masks, bad_ks in _planted(R.DROP_SEED, p, planes, heads, tokens, d):
        _, bad = R.reference_grads(x, gout, [ps], [bad_masks], bad_ks, heads, act, **kw)
        i = R.GRAD_NAMES.index(tensor)
        limit = R.bound(R.TOL_GRAD, R.rel_err(g32[i], grads[i]))
        moved = R.rel_err(bad[i], grads[i])
        assert moved > 10 * limit, f"{label}: {tensor} moves by {moved:.2e}, bound {limit:.2e}"


@pytest.mark.parametrize("case", [c for c in R.LAYER_CASES if c[4] == "relu"], ids=lambda c: f"d{c[0]}h{c[1]}")
def test_relu_cases_have_a_margin_cpu(case):
    """A relu decision that two evaluations take differently moves a whole row of dW1: not an accuracy statement.  The input
    seeds of the relu cases keep every linear1 pre-activation of the float64 forward at least 1e-5 |a|max away from zero."""
    d, heads, ofdm, planes, act, p, in_seed = case
    tokens = R.tokens_of(ofdm)
    x, _, ps = R.make_case(d, heads, tokens, planes, in_seed)
    probe = {}
    with torch.no_grad():
        R.reference_layer(x, ps, R.layer_masks(R.DROP_SEED, p, planes, heads, tokens, d), float(R.keep_scale(p)), heads, act,
                          torch.float64, "cpu", probe=probe)
    a = probe["a"].abs()
    assert float(a.min()) >= 1e-5 * float(a.max()), float(a.min() / a.max())


# ---------------------------------------------------------------- GPU

def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("ofdm", [(12, 14), (24, 14)], ids=["28tok", "56tok"])
@pytest.mark.parametrize("d,heads", [(128, 4), (256, 8)], ids=["fused_chain", "add_ln_gemm_act"])
def test_kernel_masks_are_the_restated_masks(d, heads, ofdm, p):
    """The masks the kernels apply, read out of the tape of a direct forward call, are dropout_reference's masks element for
    element (seed above 2^32).  Site 2: hd != 0 is M2 wherever the activation is not zero, kept values are gelu(a) * ks.  Sites 1
    and 3: every dropped element leaves the residual's bits (s1 == x_in, s2 == x1), every kept element changes them (but for at
    most 0.1 % where the projection is under half an ulp of the residual).  Site 0 (28 tokens): with Wq = Wk = 0 the
    probabilities are uniform, x[plane, k] = e_k and Wv[h * 32 + f, f] = 1 make V an identity per head, so the attention output
    IS ks / 28 * M0[plane, head, q, f].
    The kept values of site 2: the library's GELU is 0.5 a (1 + erf), erf to 1e-7 absolute (aft_internal.h::activate2), so its
    own fp32 evaluation is uncertain by (1e-7 + 2 ulp) * |a| / 2 whatever the mask does -- for a < 0 far more than 2 ulp of the
    cancelled result.  The check is |hd - fl32(gelu64(a) * ks)| <= 2 ulp(hd) + (1e-7 + 2^-23) * |a| ks / 2: four orders of
    magnitude below what a wrong or twice-applied keep scale moves."""
    planes, tokens = 2, R.tokens_of(ofdm)
    seed = R.DROP_SEED + d + tokens
    cfg = _cfg(d, heads, ofdm)
    ks = R.keep_scale(p)
    x, _, ps = R.make_case(d, heads, tokens, planes, seed=17)
    m0, m1, m2, m3 = R.layer_masks(seed, p, planes, heads, tokens, d)
    t = forward_tape(cfg, ps, x, p, seed)

    a64 = torch.from_numpy(t["a"]).double()
    g64 = torch.nn.functional.gelu(a64).numpy()
    live = torch.nn.functional.gelu(torch.from_numpy(t["a"])).numpy() != 0          # fp32 GELU saturates to 0 below a ~ -5.6
    assert (~live).mean() <= 1e-3
    assert np.array_equal((t["hd"] != 0)[live], m2[live]), f"site 2: {int(((t['hd'] != 0) != m2)[live].sum())} elements differ"
    want = (g64 * float(ks)).astype(np.float32)
    slack = 2 * np.spacing(np.abs(want)) + (1e-7 + 2.0 ** -23) * np.abs(t["a"]) * float(ks) / 2
    sel = live & m2
    over = np.abs(t["hd"].astype(np.float64) - want)[sel] / slack[sel]
    print(f"site 2 kept values: worst |hd - gelu(a) ks| / allowance = {over.max():.3f}")
    assert over.max() <= 1.0

    for site, m, s, resid in ((1, m1, t["s1"], t["x"]), (3, m3, t["s2"], t["x1"])):
        same = _bits(s) == _bits(resid)
        assert same[~m].all(), f"site {site}: {int((~same[~m]).sum())} restated-dropped elements were changed"
        assert same[m].mean() <= 1e-3, f"site {site}: {same[m].mean():.2%} of the restated-kept elements are unchanged"

    if tokens == 28:
        xs = torch.zeros(planes, tokens, d)
        xs[:, torch.arange(tokens), torch.arange(tokens)] = 1.0
        crafted = [q.clone() for q in ps]
        crafted[0].zero_()
        crafted[1].zero_()
        for h in range(heads):
            for f in range(tokens):
                crafted[0][2 * d + h * 32 + f, f] = 1.0
        attn = forward_tape(cfg, crafted, xs, p, seed)["attn"].reshape(planes, tokens, heads, 32)
        got = attn[..., :tokens].transpose(0, 2, 1, 3)                       # [plane, head, q, k]
        assert np.array_equal(got != 0, m0), f"site 0: {int(((got != 0) != m0).sum())} elements differ"
        assert not attn[..., tokens:].any()
        assert np.abs(got[m0] / (float(ks) / tokens) - 1).max() <= 1e-5


@functools.lru_cache(maxsize=None)
def _reference(d, heads, ofdm, planes, act, p, in_seed, drop_seeds=(R.DROP_SEED,)):
    """Inputs, float64 reference and float32-on-the-GPU yardstick of one case: computed once, shared, never modified.  More than
    one drop seed: the references are summed (two backward passes into the same .grad)."""
    tokens = R.tokens_of(ofdm)
    x, gout, ps = R.make_case(d, heads, tokens, planes, in_seed)
    ks = float(R.keep_scale(p))
    out64 = out32 = None
    g64 = g32 = None
    for s in drop_seeds:
        masks = R.layer_masks(s, p, planes, heads, tokens, d)
        o64, a = R.reference_grads(x, gout, [ps], [masks], ks, heads, act)
        o32, b = R.reference_grads(x, gout, [ps], [masks], ks, heads, act, dtype=torch.float32, device="cuda")
        out64, out32 = o64, o32
        g64 = a if g64 is None else [u + v for u, v in zip(g64, a)]
        g32 = b if g32 is None else [u + v for u, v in zip(g32, b)]
    return x, gout, ps, out64, g64, out32, g32


def _compare(label, out, grads, out64, g64, out32, g32, names, tol_grad=R.TOL_GRAD):
    """Print every figure, then hold each tensor to max(project bound, 2 e_torch32 + 1e-6)."""
    rows = [("out", R.rel_err(out, out64), R.rel_err(out32, out64), R.TOL_FWD)] if out is not None else []
    rows += [(n, R.rel_err(g, r), R.rel_err(t, r), tol_grad) for n, g, r, t in zip(names, grads, g64, g32)]
    bad = []
    for n, e_hip, e_t32, tol in rows:
        limit = R.bound(tol, e_t32)
        print(f"{label} {n}: hip {e_hip:.2e} torch32 {e_t32:.2e} bound {limit:.2e}" + (" (from e_torch32)" if limit > tol else ""))
        if not e_hip <= limit:
            bad.append(f"{n}: hip {e_hip:.2e} > {limit:.2e} (torch32 {e_t32:.2e})")
    assert not bad, label + "\n" + "\n".join(bad)


def _hip_layer(x, gout, ps, cfg, p, seed):
    from adafortitran_amd.training import HipEncoderLayerFunction
    xs = x.cuda().requires_grad_(True)
    leaves = [q.cuda().requires_grad_(True) for q in ps]
    out = HipEncoderLayerFunction.apply(xs, cfg, p, seed, *leaves)
    out.backward(gout.cuda())
    return out.detach(), [xs.grad] + [q.grad for q in leaves]


def _check_layer(case, label):
    d, heads, ofdm, planes, act, p, in_seed = case
    x, gout, ps, out64, g64, out32, g32 = _reference(*case)
    out, grads = _hip_layer(x, gout, ps, _cfg(d, heads, ofdm, act), p, R.DROP_SEED)
    _compare(label, out, grads, out64, g64, out32, g32, R.GRAD_NAMES)


@gpu
@pytest.mark.parametrize("case", R.LAYER_CASES, ids=lambda c: f"d{c[0]}h{c[1]}_{c[2][0]}x{c[2][1]}_{c[4]}_p{c[5]}")
def test_layer_with_dropout_matches_float64_with_the_same_masks(case):
    """HipEncoderLayerFunction with dropout on: output and all thirteen gradients against the float64 reference that applies the
    kernels' own masks.  One case per kernel family (dropout_reference.LAYER_CASES)."""
    _check_layer(case, "layer")


VARIANT_CASES = [(128, 4, (24, 14), 2, "gelu", 0.1, 21), R.LAYER_CASES[0]]


@gpu
@pytest.mark.parametrize("case", VARIANT_CASES, ids=["24x14", "120x14"])
@pytest.mark.parametrize("variant", [{"AFT_TRAIN_UNFUSED_FWD": "1", "AFT_TRAIN_UNFUSED_BWD": "1"}, {"AFT_TRAIN_ATTN_BWD_SPLIT": "1"},
                                     {"AFT_ATTN_BWD_GROUPS": "4"}], ids=["unfused", "attn_bwd_split", "attn_bwd_groups4"])
def test_layer_variants_with_dropout_match_float64(case, variant, switches):
    """The same check on the kernels behind the A/B switches: the launch sequences the fused chains replaced, the two-pass
    attention backward, twelve-wave attention-backward workgroups."""
    for name, value in variant.items():
        switches.set(name, value)
    _check_layer(case, "+".join(variant))


@gpu
@pytest.mark.parametrize("d,heads", [(128, 4), (256, 8)])
def test_accumulated_backward_passes_with_dropout_match_float64(d, heads):
    """Two backward passes with different dropout seeds added by the kernels into the same flat .grad views (the
    direct-accumulation path): the sum of the two float64 references, each with its own masks."""
    from adafortitran_amd import training
    from adafortitran_amd.optim import FlatParameters
    ofdm, planes, p = (24, 14), 2, 0.1
    seeds = (R.DROP_SEED, R.DROP_SEED + (1 << 33))
    x, gout, ps, _, g64, _, g32 = _reference(d, heads, ofdm, planes, "gelu", p, 31, seeds)
    cfg = _cfg(d, heads, ofdm)
    params = [torch.nn.Parameter(q.cuda()) for q in ps]
    flat = FlatParameters(params, direct_accumulation=True)
    flat.zero_grad()
    assert training.direct_grad_ok(params)
    xs = x.cuda().requires_grad_(True)
    for s in seeds:
        training.HipEncoderLayerFunction.apply(xs, cfg, p, s, *params).backward(gout.cuda())
    _compare("accumulated", None, [xs.grad] + [q.grad for q in params], None, g64, None, g32, R.GRAD_NAMES)


@gpu
@pytest.mark.parametrize("d,heads", [(128, 4), (256, 8)], ids=["chained_in_proj", "d256"])
def test_stack_with_dropout_matches_float64_with_the_same_masks(d, heads):
    """encoder_stack_train over three layers at p = 0.1: the stack draws its per-layer seeds from torch's generator, the test
    draws the same three after the same torch.manual_seed and builds the float64 three-layer reference with their masks."""
    from adafortitran_amd.training import encoder_stack_train, layer_params
    ofdm, planes, p, n = (24, 14), 4, 0.1, 3
    tokens, ks = R.tokens_of(ofdm), float(R.keep_scale(p))
    x, gout, sets = R.make_case(d, heads, tokens, planes, seed=51, layers=n)
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
