"""The training layer at token counts on and around its 32-row tiles (tests/dropout_reference.py: EDGE_CASES, EDGE_VARIANT_CASES,
EDGE_STACKS): errors of the HIP kernels and of the same formulas in float32 (PyTorch on the GPU), both against float64 with the
kernels' own masks -- the tape's log-sum-exp and attention output, the layer's output and thirteen gradients, the A/B variants, the
two-layer stacks.  Prints one line per case and tensor and writes profiles/token_edges_vs_fp64.json -- the record behind the bounds
of tests/test_train_token_edges.py.  Nothing is asserted here.

    python tools/debug/token_edges_vs_fp64.py [--out profiles/token_edges_vs_fp64.json]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import dropout_reference as R  # noqa: E402
from adafortitran_amd import _abi, _lib  # noqa: E402
from adafortitran_amd.training import HipEncoderLayerFunction, encoder_stack_train, layer_params  # noqa: E402
from train_tape import forward_tape  # noqa: E402

VARIANTS = {"unfused": {"AFT_TRAIN_UNFUSED_FWD": "1", "AFT_TRAIN_UNFUSED_BWD": "1"}, "attn_bwd_split": {"AFT_TRAIN_ATTN_BWD_SPLIT": "1"},
            "attn_bwd_groups4": {"AFT_ATTN_BWD_GROUPS": "4"}}


def cfg_of(d, heads, ofdm, act="gelu"):
    return _abi.make_config(ofdm=ofdm, pilot=(12, 2), patch=(3, 2), num_layers=1, model_dim=d, num_head=heads, activation=act)


def table(names, hip, ref, limits):
    rows = []
    for n, h, r, (e_t32, project, edge) in zip(names, hip, ref, limits):
        e_hip = R.rel_err(h, r)
        rows.append(dict(tensor=n, e_hip=e_hip, e_torch32=e_t32, project_bound=project, edge_bound=edge))
        print(f"    {n:34s} hip {e_hip:.2e}  torch32 {e_t32:.2e}  ratio {e_hip / max(e_t32, 1e-30):6.2f}  project {project:.2e}  "
              f"edge {edge:.2e}" + ("  OVER" if e_hip > min(project, edge) else ""), flush=True)
    return rows


def reference(case):
    d, heads, ofdm, planes, act, p, in_seed = case
    x, gout, ps = R.make_case(d, heads, R.tokens_of(ofdm), planes, in_seed)
    masks, ks = R.case_masks(case)
    out64, g64 = R.reference_grads(x, gout, [ps], [masks], ks, heads, act)
    out32, g32 = R.reference_grads(x, gout, [ps], [masks], ks, heads, act, dtype=torch.float32, device="cuda")
    return x, gout, ps, masks, ks, [out64] + g64, R.layer_limits(out64, g64, out32, g32)


def hip_layer(case, x, gout, ps):
    d, heads, ofdm, planes, act, p, in_seed = case
    xs = x.cuda().requires_grad_(True)
    leaves = [q.cuda().requires_grad_(True) for q in ps]
    out = HipEncoderLayerFunction.apply(xs, cfg_of(d, heads, ofdm, act), p, R.DROP_SEED, *leaves)
    out.backward(gout.cuda())
    return [out.detach(), xs.grad] + [q.grad for q in leaves]


def tape_case(case, x, ps, m0, ks):
    d, heads, ofdm, planes, act, p, in_seed = case
    tokens = R.tokens_of(ofdm)
    t = forward_tape(cfg_of(d, heads, ofdm, act), ps, x, p, R.DROP_SEED)
    lse64, o64, lim_lse, lim_o, e_lse, e_o = R.tape_figures(t["qkv"], m0, ks, planes, heads, "cuda")
    lse = torch.from_numpy(t["lse"].reshape(planes, heads, tokens)).double() * math.log(2.0)
    fig = dict(lse_e_hip=float((lse - lse64).abs().max()), lse_e_torch32=e_lse, lse_bound=lim_lse, lse_max=float(lse64.abs().max()),
               attn_e_hip=R.rel_err(torch.from_numpy(t["attn"].reshape(planes, tokens, d)), o64), attn_e_torch32=e_o, attn_bound=lim_o)
    print(f"    tape lse (absolute)                hip {fig['lse_e_hip']:.2e}  torch32 {e_lse:.2e}  bound {lim_lse:.2e}  max |lse| "
          f"{fig['lse_max']:.2f}" + ("  OVER" if fig["lse_e_hip"] > lim_lse else ""))
    print(f"    tape attn                          hip {fig['attn_e_hip']:.2e}  torch32 {e_o:.2e}  bound {lim_o:.2e}"
          + ("  OVER" if fig["attn_e_hip"] > lim_o else ""), flush=True)
    return fig


def stack_case(d, heads, tokens, planes=2, p=0.1, n=2):
    ofdm, ks = R.edge_grid(tokens), float(R.keep_scale(p))
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
    out = encoder_stack_train(xs, layers, cfg_of(d, heads, ofdm), p)
    out.backward(gout.cuda())
    names = ["out", "dx"] + [f"layers.{i}.{nm}" for i in range(n) for nm in R.GRAD_NAMES[1:]]
    return table(names, [out.detach(), xs.grad] + [q.grad for layer in layers for q in layer_params(layer)], [out64] + g64,
                 R.layer_limits(out64, g64, out32, g32, R.TOL_STACK_GRAD))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_edges_vs_fp64.json"))
    args = ap.parse_args()
    result = dict(device=torch.cuda.get_device_name(0), drop_seed=R.DROP_SEED, edge_factor=R.EDGE_FACTOR, lse_spacings=R.LSE_SPACINGS,
                  cases=[])
    names = ("out",) + R.GRAD_NAMES
    for case in R.EDGE_CASES:
        d, heads, ofdm, planes, act, p, in_seed = case
        print(f"layer d {d} heads {heads} tokens {R.tokens_of(ofdm)} planes {planes} {act} p {p}", flush=True)
        x, gout, ps, masks, ks, ref, limits = reference(case)
        entry = dict(kind="layer", d=d, heads=heads, tokens=R.tokens_of(ofdm), ofdm=list(ofdm), planes=planes, act=act, p=p,
                     input_seed=in_seed, tape=tape_case(case, x, ps, masks[0], ks),
                     tensors=table(names, hip_layer(case, x, gout, ps), ref, limits))
        result["cases"].append(entry)
        if case in R.EDGE_VARIANT_CASES:
            for label, switches in VARIANTS.items():
                print(f"  variant {label}", flush=True)
                old = {k: _lib.get_switch(k) for k in switches}
                for k, v in switches.items():
                    _lib.set_switch(k, v)
                try:
                    rows = table(names, hip_layer(case, x, gout, ps), ref, limits)
                finally:
                    for k, v in old.items():
                        _lib.set_switch(k, v)
                result["cases"].append(dict(entry, kind="variant:" + label, tape=None, tensors=rows))
    for d, heads, tokens in R.EDGE_STACKS:
        print(f"stack of 2, d {d} heads {heads} tokens {tokens} planes 2 gelu p 0.1", flush=True)
        result["cases"].append(dict(kind="stack2", d=d, heads=heads, tokens=tokens, ofdm=list(R.edge_grid(tokens)), planes=2, act="gelu",
                                    p=0.1, tape=None, tensors=stack_case(d, heads, tokens)))
    every = [(c, t) for c in result["cases"] for t in c["tensors"]]
    c, worst = max((ct for ct in every if ct[1]["e_torch32"] > 0), key=lambda ct: ct[1]["e_hip"] / ct[1]["e_torch32"])
    tapes = [c["tape"] for c in result["cases"] if c["tape"]]
    over = [dict(kind=c["kind"], d=c["d"], heads=c["heads"], tokens=c["tokens"], p=c["p"], **t) for c, t in every
            if t["e_hip"] > R.EDGE_FACTOR * t["e_torch32"]]
    result.update(
        worst_ratio_e_hip_over_e_torch32=worst["e_hip"] / worst["e_torch32"],
        worst_ratio_at=dict(kind=c["kind"], d=c["d"], heads=c["heads"], tokens=c["tokens"], p=c["p"], tensor=worst["tensor"]),
        worst_e_hip=max(t["e_hip"] for _, t in every),
        tensors_over_factor_times_e_torch32=over,
        tensors_over_a_bound=sum(t["e_hip"] > min(t["project_bound"], t["edge_bound"]) for _, t in every),
        worst_tape_lse_e_hip=max(t["lse_e_hip"] for t in tapes), worst_tape_lse_e_torch32=max(t["lse_e_torch32"] for t in tapes),
        worst_tape_lse_e_hip_over_bound=max(t["lse_e_hip"] / t["lse_bound"] for t in tapes),
        worst_tape_attn_e_hip=max(t["attn_e_hip"] for t in tapes), worst_tape_attn_e_torch32=max(t["attn_e_torch32"] for t in tapes),
        worst_tape_attn_e_hip_over_bound=max(t["attn_e_hip"] / t["attn_bound"] for t in tapes))
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}, indent=1))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
