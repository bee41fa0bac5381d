"""The inference encoder layer at token counts on and around the edges of its attention and chain kernels (infer_edges.CASES: the
8-key groups, the 16-key halves, tokens % 4, the compile-time counts 280 and 1120 and their neighbours; every packed-engine family
and the general engine), one layer through HipEngine.stage_encoder_layer against float64.

GPU: the layer's output, relative to the float64 output's max, within BOTH the project bound max(5e-5, 2 e_torch32 + 1e-6) and
4 e_torch32 + 1e-6: one phantom key moves ONE layer's output by 7.5e-5 of its max at 1120 tokens and a whole forward by less, so
the project bound alone cannot see it.  e_torch32 = the error of the same formulas in float32 (PyTorch on the GPU); the HIP result
never enters a bound.  CPU: the library takes every grid of the matrix on the engine the table names; the matrix is the stated one;
the bound separates three defects planted at the last key from rounding, by at least 10 x, at every family and token count.
tools/debug/infer_edges_vs_fp64.py prints every figure; profiles/infer_edges_vs_fp64.json holds them."""
import ctypes as C
import functools

import pytest
import torch

import dropout_reference as R
import infer_edges as E
from adafortitran_amd import _abi

gpu = pytest.mark.gpu


# ---------------------------------------------------------------- CPU

def test_the_matrix_is_the_stated_one_cpu():
    T = [31, 32, 33, 39, 40, 41, 47, 48, 49, 63, 64, 65, 96, 97, 210, 279, 280, 281, 288, 289, 1119, 1120, 1121]
    F = [32, 33, 40, 41, 48, 49, 64, 65, 97, 280, 281]
    G = [32, 33, 97, 281]
    assert (E.TOKENS_128_4, E.TOKENS_FAMILY, E.TOKENS_GENERAL) == (T, F, G)
    packed = [(128, 2), (128, 8), (128, 16), (96, 4), (160, 4), (192, 4), (256, 8), (64, 2), (32, 1)]
    want = {(128, 4, n, 2, "gelu") for n in T}
    want |= {(128, 4, n, 2, "relu") for n in (33, 280, 1120)}
    want |= {(128, 4, n, 6, "gelu") for n in (33, 97)}
    want |= {(d, h, n, 2, "gelu") for d, h in packed for n in F}
    want |= {(256, 8, n, 2, "relu") for n in (33, 280)}
    want |= {(d, h, n, 2, "gelu") for d, h in ((384, 4), (200, 8)) for n in G}
    assert set(E.CASES) == want and len(E.CASES) == len(want) == 137
    assert E.DEFECTS == ("last_key_left_out", "phantom_key", "last_value_zeroed")
    assert R.DEFECTS == ("last_key_left_out", "phantom_key", "last_query_detached_kv")      # the training tests' list is untouched
    assert E.FACTOR == R.EDGE_FACTOR == 4.0 and E.SEPARATION == 10.0
    assert all(E.grid_of(n) == (3 * n, 2) for n in T + F + G if n != 1120) and E.grid_of(1120) == (240, 28)
    assert all(R.tokens_of(E.grid_of(c[2])) == c[2] for c in E.CASES)
    assert len({E.seed_of(c) for c in E.CASES}) == len(E.CASES)
    assert E.ENGINE_OF == {**{f: "packed" for f in [(128, 4)] + packed}, (384, 4): "general", (200, 8): "general"}


def test_every_grid_of_the_matrix_runs_on_the_engine_the_table_names_cpu():
    """aft_workspace_bytes and aft_engine_of are host-only; the first returns 0 for a configuration check_config refuses."""
    from adafortitran_amd import _lib
    lib = _lib.load()
    engine = {"packed": _abi.AFT_ENGINE_PACKED, "general": _abi.AFT_ENGINE_GENERAL}
    for case in E.CASES:
        cfg = E.config_of(case)
        assert cfg.tokens == case[2], case
        assert lib.aft_workspace_bytes(C.byref(cfg), case[3] // 2) > 0, case
        assert lib.aft_engine_of(C.byref(cfg)) == engine[E.ENGINE_OF[case[:2]]], case


FAMILY_TOKENS = ([((128, 4), E.TOKENS_128_4)] + [(f, E.TOKENS_FAMILY) for f in E.PACKED_FAMILIES]
                 + [(f, E.TOKENS_GENERAL) for f in E.GENERAL_FAMILIES])


@pytest.mark.parametrize("family,tokens", FAMILY_TOKENS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_bound_separates_planted_last_key_defects_from_rounding_cpu(family, tokens):
    """Three defects of the last key, planted one at a time into the float64 reference: each moves the layer's output by at least
    10 x the bound the GPU test applies (the float32 yardstick is evaluated on the CPU here)."""
    d, heads = family
    weakest = {}
    for n in tokens:
        case = (d, heads, n, 2, "gelu")
        ref = E.reference(case)
        e32 = R.rel_err(E.reference(case, torch.float32), ref)
        assert e32 <= 2e-6, "the float32 composite itself is not within rounding of the reference"
        limit = min(E.limits(e32))
        for defect in E.DEFECTS:
            moved = R.rel_err(E.reference(case, defect=defect), ref) / limit
            weakest[defect] = min(weakest.get(defect, (moved, n)), (moved, n))
            assert moved >= E.SEPARATION, (case, defect, moved, e32, limit)
    print(family, {k: (round(v, 1), n) for k, (v, n) in weakest.items()})


# ---------------------------------------------------------------- GPU

@functools.lru_cache(maxsize=None)
def _reference(case):
    """Float64 reference and the float32-on-the-GPU yardstick's error of one case: computed once, shared, never modified."""
    ref = E.reference(case)
    return ref, R.rel_err(E.reference(case, torch.float32, "cuda"), ref)


@gpu
@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_inference_layer_matches_float64_at_token_edges(case):
    ref, e32 = _reference(case)
    y = E.hip_layer(case)
    assert torch.isfinite(y).all()
    f = E.figures(case, y, ref, e32)
    print(f"{E.case_id(case)}: hip {f['e_hip']:.2e} torch32 {e32:.2e} ratio {f['ratio']:.2f} project bound {f['project_bound']:.2e} "
          f"edge bound {f['edge_bound']:.2e} worst at plane {f['worst_plane']} token {f['worst_token']}")
    assert f["e_hip"] <= f["project_bound"] and f["e_hip"] <= f["edge_bound"], f
