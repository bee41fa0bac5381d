"""Dropout on: errors of the HIP encoder layer / stack and of the same composite in float32 (PyTorch on the GPU), both against
the float64 reference that applies the kernels' own masks (tests/dropout_reference.py).  Prints one line per case and tensor and
writes profiles/dropout_vs_fp64.json -- the record behind the bounds of tests/test_train_dropout.py.

    python tools/debug/dropout_vs_fp64.py [--out profiles/dropout_vs_fp64.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import dropout_reference as R  # noqa: E402
from adafortitran_amd import _abi  # noqa: E402
from adafortitran_amd.training import HipEncoderLayerFunction, encoder_stack_train, layer_params  # noqa: E402


def cfg_of(d, heads, ofdm, act):
    return _abi.make_config(ofdm=ofdm, pilot=(12, 2), patch=(3, 2), num_layers=1, model_dim=d, num_head=heads, activation=act)


def table(names, hip, g64, g32, tols):
    rows = []
    for n, h, r, t, tol in zip(names, hip, g64, g32, tols):
        e_hip, e_t32 = R.rel_err(h, r), R.rel_err(t, r)
        rows.append(dict(tensor=n, e_hip=e_hip, e_torch32=e_t32, bound=R.bound(tol, e_t32), bound_from_e_torch32=R.bound(tol, e_t32) > tol))
        print(f"    {n:34s} hip {e_hip:.2e}  torch32 {e_t32:.2e}  ratio {e_hip / max(e_t32, 1e-30):6.2f}  bound {rows[-1]['bound']:.2e}")
    return rows


def layer_case(case):
    d, heads, ofdm, planes, act, p, in_seed = case
    tokens, ks = R.tokens_of(ofdm), float(R.keep_scale(p))
    x, gout, ps = R.make_case(d, heads, tokens, planes, in_seed)
    masks = R.layer_masks(R.DROP_SEED, p, planes, heads, tokens, d)
    out64, g64 = R.reference_grads(x, gout, [ps], [masks], ks, heads, act)
    out32, g32 = R.reference_grads(x, gout, [ps], [masks], ks, heads, act, dtype=torch.float32, device="cuda")
    xs = x.cuda().requires_grad_(True)
    leaves = [q.cuda().requires_grad_(True) for q in ps]
    out = HipEncoderLayerFunction.apply(xs, cfg_of(d, heads, ofdm, act), p, R.DROP_SEED, *leaves)
    out.backward(gout.cuda())
    return table(("out",) + R.GRAD_NAMES, [out.detach(), xs.grad] + [q.grad for q in leaves], [out64] + g64, [out32] + g32,
                 [R.TOL_FWD] + [R.TOL_GRAD] * 13)


def stack_case(d, heads, ofdm=(24, 14), planes=4, p=0.1, n=3):
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
    out = encoder_stack_train(xs, layers, cfg_of(d, heads, ofdm, "gelu"), p)
    out.backward(gout.cuda())
    names = ["out", "dx"] + [f"layers.{i}.{nm}" for i in range(n) for nm in R.GRAD_NAMES[1:]]
    return table(names, [out.detach(), xs.grad] + [q.grad for layer in layers for q in layer_params(layer)], [out64] + g64,
                 [out32] + g32, [R.TOL_FWD] + [R.TOL_STACK_GRAD] * (1 + 12 * n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_vs_fp64.json"))
    args = ap.parse_args()
    result = dict(device=torch.cuda.get_device_name(0), drop_seed=R.DROP_SEED, cases=[])
    for case in R.LAYER_CASES:
        d, heads, ofdm, planes, act, p, in_seed = case
        print(f"layer d {d} heads {heads} grid {ofdm} planes {planes} {act} p {p}")
        result["cases"].append(dict(kind="layer", d=d, heads=heads, ofdm=list(ofdm), planes=planes, act=act, p=p, input_seed=in_seed,
                                    tensors=layer_case(case)))
    for d, heads in ((128, 4), (256, 8)):
        print(f"stack of 3, d {d} heads {heads} grid (24, 14) planes 4 gelu p 0.1")
        result["cases"].append(dict(kind="stack3", d=d, heads=heads, ofdm=[24, 14], planes=4, act="gelu", p=0.1, tensors=stack_case(d, heads)))
    every = [t for c in result["cases"] for t in c["tensors"]]
    meaningful = [t for t in every if t["e_torch32"] > 0]
    worst = max(meaningful, key=lambda t: t["e_hip"] / t["e_torch32"])
    result["worst_ratio_e_hip_over_e_torch32"] = worst["e_hip"] / worst["e_torch32"]
    result["worst_e_hip"] = max(t["e_hip"] for t in every)
    result["tensors_with_bound_from_e_torch32"] = sum(t["bound_from_e_torch32"] for t in every)
    result["tensors_over_their_bound"] = sum(t["e_hip"] > t["bound"] for t in every)
    print(f"worst e_hip / e_torch32 = {result['worst_ratio_e_hip_over_e_torch32']:.2f} ({worst['tensor']}), worst e_hip = "
          f"{result['worst_e_hip']:.2e}, bounds from e_torch32: {result['tensors_with_bound_from_e_torch32']}, over their bound: "
          f"{result['tensors_over_their_bound']}")
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
