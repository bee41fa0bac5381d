"""The training step's ends, dense layers and channel adapter at their plan edges (tests/ends_edges.py: ENDS_CASES, DENSE_CASES,
ADAPTER_CASES): errors of the HIP kernels and of the same formulas in float32 (PyTorch on the GPU), both against float64.  Prints one
line per case and tensor and writes profiles/ends_edges_vs_fp64.json -- the record behind the bounds of
tests/test_ends_dense_edges.py: per case and tensor the HIP error, the float32 yardstick, the bound and the ratio.  Nothing is asserted
but that every output element was written.

    python tools/debug/ends_edges_vs_fp64.py [--out profiles/ends_edges_vs_fp64.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ends_edges as E  # noqa: E402
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ends_edges_vs_fp64.json"))
    args = ap.parse_args()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    result = dict(device=torch.cuda.get_device_name(0), cus=cus, edge_factor=E.EDGE_FACTOR, sum_floor=E.SUM_FLOOR,
                  raised_factors={f"{k[0]}.{k[1]}": v for k, v in E.FACTOR.items()},
                  note="elementwise tensors: hip, e32, bound relative to the float64 tensor's max; summed gradients: per element "
                       "relative to A_i = sum |terms| (hip_max, e32_max: relative to the tensor's max, held to `project`)", cases=[])

    def record(cid, family, plan, rows):
        for line in E.show("   ", rows):
            print("    OVER " + line, flush=True)
        result["cases"].append(dict(id=cid, family=family, plan=plan, tensors=rows))

    def plan_of(q):
        return {k: v for k, v in vars(q).items() if isinstance(v, (int, str, bool, list, tuple))}

    for case in E.ENDS_CASES:
        print(E.ends_id(case), flush=True)
        s = Switches()
        try:
            rows_e, rows_t = E.gpu_ends(case, s)
        finally:
            s.restore()
        record(E.ends_id(case), "ends", plan_of(E.ends_props(case, cus)), rows_e + rows_t)
    for case in E.DENSE_CASES:
        print(E.dense_id(case), flush=True)
        s = Switches()
        try:
            rows = E.gpu_dense(case, s)
        finally:
            s.restore()
        record(E.dense_id(case), "dense", plan_of(E.dense_props(case, cus)), rows)
    for case in E.EMPTY_SLICES:
        print(E.dense_id(case) + " scratch 1e30", flush=True)
        record(E.dense_id(case) + "_scratch1e30", "dense", plan_of(E.dense_props(case, cus)), E.gpu_dense(case, Switches(), fill=1e30))
    for case in E.ADAPTER_CASES:
        print(E.adapter_id(case), flush=True)
        rows_f, rows_b = E.gpu_adapter(case)
        record(E.adapter_id(case), "adapter", dict(hidden=list(case[0]), frames=case[1]), rows_f + rows_b)
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
