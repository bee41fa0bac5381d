"""The inference encoder layer at token counts on and around the edges of its attention and chain kernels (tests/infer_edges.py:
CASES): the error of HipEngine.stage_encoder_layer and of the same formulas in float32 (PyTorch on the GPU), both against float64 on
the CPU, their ratio, both bounds, the row of the largest error and how it compares with the rows before every plane's last 32-token
tile.  Prints one line per case and writes profiles/infer_edges_vs_fp64.json -- the record behind the bounds of
tests/test_infer_token_edges.py.  Nothing is asserted here.

    python tools/debug/infer_edges_vs_fp64.py [--out profiles/infer_edges_vs_fp64.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import dropout_reference as R  # noqa: E402
import infer_edges as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infer_edges_vs_fp64.json"))
    args = ap.parse_args()
    result = dict(device=torch.cuda.get_device_name(0), factor=E.FACTOR, project_tolerance=R.TOL_FWD, cases=[])
    for case in E.CASES:
        d, heads, tokens, planes, act = case
        ref = E.reference(case)
        e32 = R.rel_err(E.reference(case, torch.float32, "cuda"), ref)
        y = E.hip_layer(case)
        f = E.figures(case, y, ref, e32)
        f["last_tile_over_rest"] = E.worst_row_share_in_last_tile(y, ref, tokens)
        over = f["e_hip"] > min(f["project_bound"], f["edge_bound"])
        print(f"{E.case_id(case):28s} hip {f['e_hip']:.2e}  torch32 {e32:.2e}  ratio {f['ratio']:5.2f}  project {f['project_bound']:.2e}  "
              f"edge {f['edge_bound']:.2e}  worst row {f['worst_row']} (plane {f['worst_plane']} token {f['worst_token']})  last tile / rest "
              f"{f['last_tile_over_rest']:.2f}" + ("  OVER" if over else ""), flush=True)
        if f["last_tile_over_rest"] == float("inf"):
            f["last_tile_over_rest"] = None      # a single tile per plane: nothing to compare with
        result["cases"].append(dict(d=d, heads=heads, tokens=tokens, planes=planes, act=act, engine=E.ENGINE_OF[(d, heads)],
                                    ofdm=list(E.grid_of(tokens)), input_seed=E.seed_of(case), over=over, **f))
    worst = max(result["cases"], key=lambda c: c["ratio"])
    by_family = {}
    for c in result["cases"]:
        key = f"d{c['d']}h{c['heads']}"
        by_family[key] = max(by_family.get(key, 0.0), c["ratio"])
    result.update(worst_ratio_e_hip_over_e_torch32=worst["ratio"],
                  worst_ratio_at={k: worst[k] for k in ("d", "heads", "tokens", "planes", "act", "worst_plane", "worst_token")},
                  worst_ratio_by_family=by_family, worst_e_hip=max(c["e_hip"] for c in result["cases"]),
                  worst_e_torch32=max(c["e_torch32"] for c in result["cases"]),
                  worst_e_hip_over_bound=max(c["e_hip"] / min(c["project_bound"], c["edge_bound"]) for c in result["cases"]),
                  cases_over_a_bound=sum(c["over"] for c in result["cases"]))
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}, indent=1))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
