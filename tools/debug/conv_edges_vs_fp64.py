"""The ConvEnhancer training kernels at their plan edges (tests/conv_edges.py: CASES): errors of the HIP kernels and of the same
formulas in float32 (PyTorch on the GPU), both against float64 -- the forward call's y, c1..c3, and the backward call's dx, g1..g3 and
eight parameter gradients against the float64 backward run on the c1..c3 the forward kernel wrote.  Prints one line per case and tensor
and writes profiles/conv_edges_vs_fp64.json -- the record behind the bounds of tests/test_conv_train_edges.py.  Nothing is asserted.

    python tools/debug/conv_edges_vs_fp64.py [--out profiles/conv_edges_vs_fp64.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import conv_edges as E  # noqa: E402
from adafortitran_amd import _lib  # noqa: E402


class Switches:
    """What the tests' ``switches`` fixture does, for one case."""

    def __init__(self):
        self.old = {}

    def set(self, name, value):
        self.old.setdefault(name, _lib.get_switch(name))
        _lib.set_switch(name, value)

    def restore(self):
        for name, value in self.old.items():
            _lib.set_switch(name, value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_edges_vs_fp64.json"))
    args = ap.parse_args()
    result = dict(device=torch.cuda.get_device_name(0), edge_factor=E.EDGE_FACTOR, sum_floor=E.SUM_FLOOR, raised_factors=E.FACTOR,
                  note="elementwise tensors: hip, e32, bound relative to the float64 tensor's max; parameter gradients: per element "
                       "relative to A_i = sum |terms| (hip_max, e32_max: relative to the tensor's max, held to `project`)", cases=[])
    for case in E.CASES:
        S, T, n, sw, scratch = case
        plan = E.plan(S, T, int(dict(sw)["AFT_CONV_COLUMN_TILES"]) if "AFT_CONV_COLUMN_TILES" in dict(sw) else None)
        print(f"{E.case_id(case)}  plan {plan}", flush=True)
        s = Switches()
        try:
            rows_f, rows_b = E.gpu_case(case, s)
        finally:
            s.restore()
        over = E.show("   ", rows_f + rows_b)
        for line in over:
            print("    OVER " + line, flush=True)
        result["cases"].append(dict(id=E.case_id(case), S=S, T=T, planes=n, switches=dict(sw), forward_scratch=scratch, plan=plan,
                                    wgrad_chunks=E.wgrad_chunks(n, S, T)[0], tensors=rows_f + rows_b))
    every = [(c["id"], t) for c in result["cases"] for t in c["tensors"]]
    cid, worst = max((ct for ct in every if ct[1]["e32"] > 0), key=lambda ct: ct[1]["hip"] / ct[1]["e32"])
    cid_b, worst_b = max(every, key=lambda ct: ct[1]["ratio"])
    result.update(worst_hip_over_e32=worst["hip"] / worst["e32"], worst_hip_over_e32_at=dict(case=cid, tensor=worst["name"]),
                  worst_error_over_bound=worst_b["ratio"], worst_error_over_bound_at=dict(case=cid_b, tensor=worst_b["name"]),
                  tensors_over_a_bound=[dict(case=c, **t) for c, t in every if not t["ok"]])
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}, indent=1))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
