"""The ConvEnhancer stack's training kernels (training forward with its three saved activations, the masked data-gradient run,
k_conv_train.hip's weight and bias gradients) at the grids where their geometry changes -- conv_edges.py: one row tile / one more row,
one-row and two-row bands, the last band plan and the first column-tile plan, the weight-gradient kernel's 64-row chunks, its grid
stride past 2048 chunks, the 8-plane groups and 256-pixel blocks of wgrad8x1_kernel -- against float64.

GPU: (a) y, c1, c2, c3 of a direct forward call against the float64 stack; (b) dx, g1..g3 (read from the call's scratch) and the eight
parameter gradients of a direct backward call against the float64 backward run on the float32 c1..c3 the forward kernel wrote (no ReLU
decision crosses a precision boundary); (c) accumulate = 1; (d) HipConvEnhancerFunction against float64 autograd, the project's bounds.
CPU: (e) the planners restated in conv_edges.py give every grid the property it is in the matrix for, and the library takes it;
(f) the matrix is the stated one; (g) the bounds of (a) and (b) separate seven planted edge defects from rounding.

Bounds.  e32 = the error of the same formulas in float32 (PyTorch on the GPU); the HIP result never enters a bound.  Elementwise
tensors, relative to the float64 tensor's max: BOTH the project bound (2e-5 for y, c*; 1e-4 for g*, dx) and 4 e32 + 1e-6.  Parameter
gradients are sums of planes * S * T products in tensors as small as one element, where one float32 run's error can be zero by luck:
per element, against A_i = sum |terms| (the float64 routine on |g| and |a|): err_i / A_i <= 4 e32' + 2^-22, e32' = the same ratio for
torch float32; and 2e-4 of the tensor's max.  tools/debug/conv_edges_vs_fp64.py prints every figure; profiles/conv_edges_vs_fp64.json
holds them."""
import functools

import pytest
import torch

import conv_edges as E

gpu = pytest.mark.gpu


# ---------------------------------------------------------------- CPU: (e) plans, (f) the matrix, (g) the bounds themselves

def test_every_grid_reaches_its_plan_edge_cpu():
    """The restated planners (TRAIN = true, no extra LDS floats) give each grid what the matrix names it for, and
    aft_conv_enhancer_scratch_bytes (host-only; 0 for a grid without a plan) takes every grid."""
    from adafortitran_amd import _lib
    lib = _lib.load()
    for n, S, T in E.all_grids():
        assert lib.aft_conv_enhancer_scratch_bytes(n, S, T) > 0, (n, S, T)
    P = E.plan
    for S, T in E.ONE_BAND:
        p = P(S, T)
        assert (p["kind"], p["nbands"], p["band_rows"], p["nctiles"]) == ("bands", 1, S, 1), (S, T)
        assert p["ntiles"] == -(-S // 30) and p["nseg"] == (2 if T >= 8 else 1), (S, T)
    assert P(3, 8)["nseg"] == 2 and P(29, 7)["nseg"] == 1
    assert [P(S, T)["ntiles"] for S, T in ((30, 8), (31, 9), (60, 14), (61, 14))] == [1, 2, 2, 3]     # 31 = 30 + 1, 61 = 60 + 1
    assert P(120, 16)["lds"] == 157120 and E.plan_bands(120, 17)["nbands"] > 1                       # the largest one-band plan
    assert P(120, 14) == dict(kind="bands", nbands=1, band_rows=120, ntiles=4, nseg=2, sp=128, lds=139712, nctiles=1, tcols=14)
    for (S, T), (nb, br) in E.SEVERAL_BANDS.items():
        p = P(S, T)
        assert (p["kind"], p["nbands"], p["band_rows"]) == ("bands", nb, br) and nb * br == S, (S, T)
    assert P(118, 20)["ntiles"] == 3 and (59 + 2) % 30 == 1           # the band's 61 rows leave one row in the third tile
    assert P(232, 33)["lds"] == 157536
    assert P(30, 64)["lds"] == 162016 and P(62, 64)["lds"] == 162016 and 163840 - 162016 < 17 * 36 * 4   # not one more column
    assert E.plan_bands(30, 65) is None and E.plan_bands(62, 65) is None
    for (S, T), want in E.COLUMN_TILES.items():
        p = P(S, T)
        assert E.plan_bands(S, T) is None and p["kind"] == "tiles" and p["nctiles"] >= 2, (S, T)
        if want is not None:
            assert (p["nbands"], E.tile_widths(p, T)) == want, (S, T)
    assert (P(37, 66)["nbands"], P(37, 66)["ntiles"]) == (1, 2)
    for (S, T), v in E.FORCED_TILES:
        p = P(S, T, v)
        assert p["kind"] == "tiles" and p["nctiles"] >= min(max(2, v), -(-T // p["tcols"])) and p["nctiles"] >= 2, (S, T, v)
    # weight gradients: 64-row chunks and their two-value tail, the grid stride, plane groups, 256-pixel blocks
    assert [-(-S // 64) for S in (63, 64, 65, 128, 129)] == [1, 1, 2, 2, 3]
    assert [S * 4 for S in (63, 64, 65)] == [252, 256, 260]
    assert E.wgrad_chunks(600, 8, 8) == (4800, 512) and E.wgrad_chunks(350, 65, 3) == (2100, 512)     # past 4 x 512 chunks
    assert all(E.wgrad_chunks(n, S, T)[0] <= 2048 for n, S, T in E.all_grids() if n < 300)
    assert [-(-n // 8) for n in (9, 17)] == [2, 3]


def test_the_matrix_is_the_stated_one_cpu():
    two = {(1, 1), (2, 3), (3, 8), (29, 7), (30, 8), (31, 9), (60, 14), (61, 14), (63, 4), (64, 4), (65, 4), (128, 2), (129, 2),
           (120, 16), (120, 14), (118, 20), (122, 15), (122, 28), (59, 40), (232, 33), (30, 64), (62, 64), (30, 65), (62, 65), (16, 70),
           (37, 66)}
    want = {(S, T, 2, (), True) for S, T in two}
    want |= {(8, 8, 600, (), True), (65, 3, 350, (), True), (24, 4, 9, (), True), (24, 4, 17, (), True)}
    want |= {(120, 14, 2, (("AFT_CONV_NSPLIT", v),), True) for v in "124"} | {(120, 14, 2, (), False)}
    want |= {(S, T, 2, (("AFT_CONV_COLUMN_TILES", v),), True) for S, T in ((31, 9), (118, 20)) for v in "27"}
    assert set(E.CASES) == want and len(E.CASES) == len(want) == 38
    assert E.ACCUMULATE_GRID == (65, 4)
    assert E.END_TO_END + [g for g, _ in E.END_TO_END_PLANES] == [(61, 14), (118, 20), (62, 65), (120, 14), (65, 3), (24, 4)]
    assert (E.EDGE_FACTOR, E.SUM_FLOOR, E.TOL_FWD, E.TOL_DGRAD, E.TOL_WGRAD, E.FACTOR) == (4.0, 2.0 ** -22, 2e-5, 1e-4, 2e-4, {})


def test_shifted_products_are_torchs_convolutions_cpu():
    """The yardstick's nine shifted channel products against F.conv2d and torch.nn.grad.conv2d_input / conv2d_weight, in float64."""
    torch.manual_seed(3)
    x, w, b, g = [torch.randn(*s, dtype=torch.float64) for s in ((3, 8, 5, 7), (32, 8, 3, 3), (32,), (3, 32, 5, 7))]
    conv, dgrad, wgrad = E.conv_ops("cpu")
    for mine, ref in ((E.conv_taps(x, w, b), conv(x, w, b)), (E.dgrad_taps(g, w), dgrad(g, w)), (E.wgrad_taps(x, g), wgrad(x, g))):
        assert mine.shape == ref.shape and float((mine - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


# defect -> the grids it applies to (S, T, planes).  (g) needs more than 2048 chunks, which only the many-plane grids have.
PLANTED = [("seam_fwd3", (118, 20, 2)), ("seam_fwd3", (59, 40, 2)), ("seam_dgrad2", (118, 20, 2)), ("seam_dgrad2", (59, 40, 2)),
           ("halo_mask", (118, 20, 2)), ("halo_mask", (59, 40, 2)), ("halo_mask", (62, 65, 2)), ("tile_seam_fwd3", (62, 65, 2)),
           ("tail_dropped", (65, 4, 2)), ("plane9_missing", (24, 4, 9)), ("second_chunk", (8, 8, 600)), ("second_chunk", (65, 3, 350))]


@functools.lru_cache(maxsize=None)
def _cpu_figures(grid):
    """Inputs, the float32 CPU forward's c1..c3 as the tape's bits, float64 references, float32 yardsticks (on the CPU here) and A."""
    S, T, n = grid
    params, x, dy = E.make_case(S, T, n)
    f64, f32 = E.forward(params, x), E.forward(params, x, torch.float32)
    cs = [c.float() for c in f32[1:]]
    b64, b32 = E.backward(params, x, dy, cs), E.backward(params, x, dy, cs, torch.float32)
    mag = {k: v for k, v in E.backward(params, x, dy, cs, magnitudes=True).items() if k in E.GRAD_NAMES}
    return params, x, dy, cs, dict(zip(E.FWD_NAMES, f64)), dict(zip(E.FWD_NAMES, f32)), b64, b32, mag


@pytest.mark.parametrize("defect,grid", PLANTED, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_bounds_separate_planted_edge_defects_from_rounding_cpu(defect, grid):
    """Each defect, planted alone into the float64 reference, moves at least one tensor that (a) or (b) compares by more than 10 x
    the bound the GPU test applies to it; the float32 yardstick itself stays inside every bound."""
    S, T, n = grid
    params, x, dy, cs, f64, f32, b64, b32, mag = _cpu_figures(grid)
    names_b = E.BWD_ELEMENT_NAMES + E.GRAD_NAMES
    own = E.judge(E.FWD_NAMES, f32, f64, f32) + E.judge(names_b, b32, b64, b32, mag)
    assert all(r["ok"] for r in own), [r for r in own if not r["ok"]]
    geo = E.plan(S, T)
    if defect in ("seam_fwd3", "tile_seam_fwd3"):
        assert (geo["nbands"] if defect == "seam_fwd3" else geo["nctiles"]) > 1
        seam = (2, geo["band_rows"]) if defect == "seam_fwd3" else (3, geo["tcols"])
        rows = E.judge(E.FWD_NAMES, dict(zip(E.FWD_NAMES, E.forward(params, x, seam3=seam))), f64, f32)
    else:
        if defect in ("seam_dgrad2", "halo_mask"):
            assert geo["nbands"] > 1
        rows = E.judge(names_b, E.backward(params, x, dy, cs, defect=defect, geo=geo), b64, b32, mag)
    moved = {r["name"]: round(r["ratio"], 1) for r in rows if r["ratio"] > 1}
    print(defect, grid, moved)
    assert moved and max(moved.values()) > 10, moved
    expected = {"seam_fwd3": {"c3", "y"}, "tile_seam_fwd3": {"c3", "y"}, "seam_dgrad2": {"g1", "dx", "dW1", "db1"},
                "halo_mask": {"g1", "dx", "dW1", "db1"}, "tail_dropped": {"dW2", "dW3"}, "plane9_missing": {"dW1", "dW4"},
                "second_chunk": {"dW2"}}[defect]
    assert set(moved) <= expected, "the planted defect reaches tensors it should not touch"


# ---------------------------------------------------------------- GPU

def _hold(label, rows):
    bad = E.show(label, rows)
    assert not bad, label + "\n" + "\n".join(bad)


@gpu
@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_conv_training_matches_float64_at_plan_edges(case, switches):
    """(a) and (b) on one case: the forward call's y, c1, c2, c3; then the backward call on the c1..c3 it just wrote: dx, g1..g3 and
    the eight parameter gradients."""
    rows_f, rows_b = E.gpu_case(case, switches)
    _hold(E.case_id(case) + " forward", rows_f)
    _hold(E.case_id(case) + " backward", rows_b)


@gpu
def test_accumulate_adds_the_gradient_onto_prefilled_tensors():
    """(c) accumulate = 1 at (65, 4): every parameter gradient is prefill + the gradient of the overwriting call to ONE float32
    addition (the reduction adds its fixed-order sum to what is there); dx is overwritten either way."""
    S, T = E.ACCUMULATE_GRID
    params, x, dy = E.make_case(S, T, 2)
    params, x, dy = [t.cuda() for t in params], x.cuda(), dy.cuda()
    cs = E.hip_forward(params, x)[1:]
    plain = E.hip_backward(params, x, dy, cs)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(77)
        prefill = [torch.randn(p.shape).cuda() for p in params]
    acc = E.hip_backward(params, x, dy, cs, prefill=prefill)
    assert torch.equal(acc["dx"], plain["dx"])
    for name, pre in zip(E.GRAD_NAMES, prefill):
        assert torch.equal(acc[name], pre + plain[name]), name
        assert not torch.equal(acc[name], plain[name]), name


@gpu
@pytest.mark.parametrize("S,T,n", [(S, T, 2) for S, T in E.END_TO_END] + [(S, T, n) for (S, T), n in E.END_TO_END_PLANES],
                         ids=lambda v: str(v))
def test_conv_enhancer_function_matches_float64_autograd(S, T, n):
    """(d) The wiring: HipConvEnhancerFunction.apply(...).backward(dy) against plain float64 autograd, the project's bounds."""
    from adafortitran_amd.training import HipConvEnhancerFunction
    params, x, dy = E.make_case(S, T, n)
    xs = x.cuda().requires_grad_(True)
    ps = [p.cuda().requires_grad_(True) for p in params]
    y = HipConvEnhancerFunction.apply(xs, *ps)
    y.backward(dy.cuda())
    x64 = x.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in params]
    h = x64
    for k in range(4):
        h = torch.nn.functional.conv2d(h, p64[2 * k], p64[2 * k + 1], padding=1)
        h = torch.relu(h) if k < 3 else h
    h.backward(dy.double())
    got, ref = [y.detach(), xs.grad] + [p.grad for p in ps], [h.detach(), x64.grad] + [p.grad for p in p64]
    for name, a, b, tol in zip(("y", "dx") + E.GRAD_NAMES, got, ref, [E.TOL_FWD, E.TOL_DGRAD] + [E.TOL_WGRAD] * 8):
        err = E.rel_err(a, b)
        print(f"{S}x{T}x{n} {name}: hip {err:.2e} bound {tol:.2e}")
        assert err <= tol, name
