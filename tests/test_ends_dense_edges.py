"""The rest of the training step -- the encoder's two thin ends (k_ends_train.hip), the dense layers behind HipLinear (k_gemm.hip:
launch_gemm NT / NN, launch_gemm_tn, launch_colsum, the slice reductions) and the channel adapter (k_train.hip: adapter_train_*) -- at
the sizes where their geometry changes (ends_edges.py: one partial 32-row tile / the tile boundary, tiles that straddle a plane, the
persistent loop's second trip, every row-group count, every instantiation of the embed and tail backward at its class boundary, plane
chunks with a partial last pass, the three GEMM paths of the three products, 64- and 96-row tile walks, split slices that stay
empty) against float64.

GPU: (a) every ends case: x0, d_conv, d_tok6, dW1, db1, dpos of direct embed calls and out, dx, dW2, db2 of direct tail calls;
(b) every dense case: y, dx, dW, db; (c) every adapter case: tokens, a0, a1, then da0, da1 and the 18 gradients from the float32 a0, a1
the forward kernel wrote; (d) the empty-slice cases again with the scratch poisoned by 1e30; (e) accumulate = 1 on one case of each
family; (f) the refusals; (g) every case reaches its edge with the device's CU count, and the scratch queries agree with the restated
planners.  Outputs and scratch are NaN before every call and every output element must be finite after it.
CPU: (h) the restated planners give every case the property it is in the matrix for (256 CUs), and the host-only dense scratch
query agrees; (i) the matrix is the stated one; (j) the formulas are torch's linear / PatchEmbedding / InversePatchEmbedding in
float64; (k) the bounds separate eight planted edge defects from rounding.

Bounds.  e32 = the error of the same formulas in float32 torch; the HIP result never enters a bound.  Elementwise tensors, relative to
the float64 tensor's max: BOTH the project bound (2e-6 x0 / out, 2e-5 the ends' gradients, 1e-5 dense and adapter) and 4 e32 + 1e-6.
Summed gradients, per element against A_i = sum |terms| (the float64 routine on absolute values): err_i / A_i <= 4 e32' + 2^-22, and
the project's whole-tensor bound (2e-5 ends, 1e-4 dense and adapter).  tools/debug/ends_edges_vs_fp64.py prints every figure;
profiles/ends_edges_vs_fp64.json holds them."""
import functools

import pytest
import torch

import ends_edges as E

gpu = pytest.mark.gpu


# ---------------------------------------------------------------- CPU: (h) plans, (i) the matrix, (j) the formulas, (k) the bounds

def _missed(cus):
    bad = [E.ends_id(c) for i, c in enumerate(E.ENDS_CASES) if not E.ENDS_EDGE[i](E.ends_props(c, cus))]
    return bad + [E.dense_id(c) for i, c in enumerate(E.DENSE_CASES) if not E.DENSE_EDGE[i](E.dense_props(c, cus))]


def test_every_case_reaches_its_edge_cpu():
    """The restated planners, at 256 CUs, give each case what the matrix names it for; aft_dense_bwd_scratch_bytes (host-only) agrees
    with the restated slice counts."""
    assert len(E.ENDS_EDGE) == len(E.ENDS_CASES) and len(E.DENSE_EDGE) == len(E.DENSE_CASES)
    assert _missed(256) == []
    P = lambda i: E.ends_props(E.ENDS_CASES[i])  # noqa: E731
    assert (P(8).grid, P(8).ntiles - P(8).grid) == (1024, 11)                             # 11 workgroups take a second tile
    assert [P(i).row_groups for i in (0, 1, 3, 5, 6, 7)] == [256, 128, 8, 5, 3, 2] and P(0).row_groups > E.ENDS_TILE
    assert (P(15).tb, P(15).ch, P(15).ppc, P(15).chunks, P(15).passes, P(15).last_chunk) == (256, 4, 5, 4, [4, 1], 3)
    assert (P(16).tb, P(16).ch, P(16).ppc, P(16).chunks, P(16).passes, P(16).last_chunk) == (35, 30, 9, 29, [4, 4, 1], 4)
    assert P(17).passes == [4, 4, 1] and P(17).chunks == 29
    assert [P(i).last_block for i in (0, 1, 6)] == [3, 8, 1]
    assert [E.make_dims(n, S, T, p0, p1, d, False) for n, S, T, p0, p1, d in E.REFUSALS] == [None] * 4
    assert E.make_dims(2, 4, 2, 1, 1, 512, True) is not None
    D = lambda i: E.dense_props(E.DENSE_CASES[i])  # noqa: E731
    assert (D(16).fwd_tiles, D(16).fwd_grid, D(16).dgrad_tiles, D(16).dgrad_grid) == (684, 684, 1025, 1024)
    assert (D(17).fwd_tiles, D(17).fwd_grid) == (1025, 1024) and (D(18).fwd_tiles, D(18).fwd_grid) == (769, 768)
    assert D(22).rows == 128 * 256 + 8 and D(22).used * D(22).chunk >= D(22).rows > (D(22).used - 1) * D(22).chunk
    assert D(26).rows == 65 * 1024 + 1
    from adafortitran_amd import _lib
    lib = _lib.load()
    for c in E.DENSE_CASES:
        assert lib.aft_dense_bwd_scratch_bytes(*c[:3]) == 4 * E.dense_scratch_floats(*c[:3]), c


def test_the_matrix_is_the_stated_one_cpu():
    G = (("AFT_EMBED_BWD_GENERIC", "1"),)
    ends = [(3, 1, 1, 1, 4, False, 2, (), True), (4, 2, 1, 1, 8, False, 4, (), True), (3, 1, 1, 1, 8, True, 11, (), True),
            (28, 4, 2, 2, 128, True, 3, (), True), (28, 4, 2, 2, 128, True, 3, (), False), (30, 3, 3, 1, 200, False, 3, (), True),
            (9, 2, 1, 2, 260, True, 5, (), True), (16, 16, 4, 8, 512, True, 3, (), True), (20, 6, 1, 1, 8, False, 276, (), True),
            (20, 6, 1, 1, 8, True, 276, (), True), (10, 6, 5, 2, 128, True, 5, (), True), (10, 6, 5, 2, 128, True, 5, G, True),
            (22, 3, 11, 1, 128, True, 5, (), True), (8, 12, 4, 6, 256, False, 9, (), True), (10, 10, 5, 5, 256, False, 9, (), True),
            (64, 32, 1, 1, 8, False, 18, (), True), (20, 14, 1, 1, 8, False, 256, G, True), (20, 14, 1, 1, 128, False, 256, (), True),
            (8, 4, 4, 2, 128, False, 9, (), True), (6, 6, 3, 3, 128, False, 9, (), True), (16, 8, 8, 4, 128, False, 9, (), True),
            (8, 10, 4, 5, 256, False, 9, (), True), (8, 12, 4, 6, 200, False, 9, (), True)]
    assert E.ENDS_CASES == ends and len(set(ends)) == 23
    plain = [(64, 16, 16), (63, 16, 128), (64, 16, 128), (65, 16, 128), (64, 16, 127), (64, 16, 129), (64, 16, 132), (65, 12, 132),
             (64, 1, 128), (64, 17, 128), (65, 17, 129), (64, 8, 1), (64, 8, 17), (1, 16, 4), (16, 16, 4), (17, 16, 4), (65600, 16, 4)]
    more = [(127, 16, 8), (255, 16, 8), (256, 16, 8), (32776, 16, 8), (32777, 16, 8), (32784, 16, 8), (32777, 15, 8), (66561, 4, 8),
            (128, 4, 63), (128, 4, 64), (128, 4, 65)]
    dense = ([(*s, True, True, ()) for s in plain]
             + [(65600, 16, 4, True, True, (("AFT_GEMM_BM", "64"),)), (73824, 16, 4, True, True, (("AFT_GEMM_BM", "96"),))]
             + [(*s, True, True, ()) for s in more] + [(65, 12, 132, True, False, ()), (65, 12, 132, False, True, ())])
    assert E.DENSE_CASES == dense and len(set(dense)) == 32
    assert [c[:3] for c in E.EMPTY_SLICES] == [(32776, 16, 8), (32777, 16, 8), (32784, 16, 8), (32777, 15, 8)]
    assert E.ADAPTER_CASES == [(h, f) for h in ((1, 1, 2), (256, 64, 560), (7, 42, 560), (5, 9, 82)) for f in (1, 13)]
    assert E.ADAPTER_REFUSED == (7, 65, 560)
    assert E.REFUSALS == [(2, 33, 2, 33, 1, 8), (2, 4, 2, 1, 1, 516), (2, 4, 2, 1, 1, 6), (2, 7, 2, 2, 1, 8)]
    assert E.ACCUMULATE == dict(ends=ends[5], dense=dense[7], adapter=((5, 9, 82), 13))
    assert (E.EDGE_FACTOR, E.SUM_FLOOR, E.FACTOR) == (4.0, 2.0 ** -22, {})
    assert E.ENDS_TOL == dict(x0=2e-6, out=2e-6, d_conv=2e-5, d_tok6=2e-5, dx=2e-5, dW1=2e-5, db1=2e-5, dpos=2e-5, dW2=2e-5, db2=2e-5)
    assert E.DENSE_TOL == dict(y=1e-5, dx=1e-5, dW=1e-4, db=1e-4) and (E.ADAPTER_ELEMENT_TOL, E.ADAPTER_SUM_TOL) == (1e-5, 1e-4)


def _close(a, b):
    return a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("case", [E.ENDS_CASES[3], E.ENDS_CASES[5], E.ENDS_CASES[7]], ids=E.ends_id)
def test_the_formulas_are_torchs_modules_in_float64_cpu(case):
    """embed / tail / dense of ends_edges.py against float64 autograd through torch.nn.functional.linear, PatchEmbedding and
    InversePatchEmbedding; the adapter's against blocks.ChannelAdapter."""
    from adafortitran_amd.blocks import ChannelAdapter, InversePatchEmbedding, PatchEmbedding
    S, T, p0, p1, d, adapter, planes = case[:7]
    inp = E.make_ends(case)
    leaf = {k: v.double().requires_grad_(True) for k, v in inp.items() if v is not None}
    tk = PatchEmbedding((p0, p1))(leaf["conv"])
    if adapter:
        tk = torch.cat((tk, leaf["tok6"]), dim=2)
    x0 = torch.nn.functional.linear(tk, leaf["w1"], leaf["b1"]) + leaf["pos"]
    x0.backward(leaf["dx0"].detach())
    mine = E.embed(case, inp)
    want = dict(x0=x0.detach(), d_conv=leaf["conv"].grad, dW1=leaf["w1"].grad, db1=leaf["b1"].grad, dpos=leaf["pos"].grad)
    if adapter:
        want["d_tok6"] = leaf["tok6"].grad
    assert set(mine) == set(want) and all(_close(mine[k], want[k]) for k in want)
    out = leaf["resid"] + InversePatchEmbedding((S, T), (p0, p1))(torch.nn.functional.linear(leaf["x"], leaf["w2"], leaf["b2"]))
    out.backward(leaf["d_out"].detach())
    mine = E.tail(case, inp)
    want = dict(out=out.detach(), dx=leaf["x"].grad, dW2=leaf["w2"].grad, db2=leaf["b2"].grad)
    assert set(mine) == set(want) and all(_close(mine[k], want[k]) for k in want)
    # dense
    dc = E.DENSE_CASES[10]
    di = E.make_dense(dc)
    lf = {k: v.double().requires_grad_(True) for k, v in di.items()}
    y = torch.nn.functional.linear(lf["x"], lf["w"], lf["b"])
    y.backward(lf["dy"].detach())
    mine = E.dense(dc, di)
    assert all(_close(mine[k], v) for k, v in dict(y=y.detach(), dx=lf["x"].grad, dW=lf["w"].grad, db=lf["b"].grad).items())
    # adapter: the tape is the float64 forward's own activations here
    ac = E.ADAPTER_CASES[7]
    ai = E.make_adapter(ac)
    ad = ChannelAdapter(ac[0]).double()
    with torch.no_grad():
        for p, v in zip(ad.parameters(), ai["params"]):
            p.copy_(v)
    tok = ad(*[c.double()[:, None] for c in ai["conds"]])
    tok.backward(ai["dtok"].double())
    fwd = E.adapter_forward(ai)
    assert _close(fwd["tok6"], tok.detach())
    bwd = E.adapter_backward(ai, fwd["a0"], fwd["a1"])
    for name, p in zip(E.ADAPTER_GRADS, ad.parameters()):
        assert _close(bwd[name].reshape(p.shape), p.grad), name


# defect -> (family, the case it applies to, the tensors it may move)
PLANTED = [("second_tile", "tail", E.PERSISTENT, {"dW2", "db2"}),
           ("stray_plane", "embed", E.STRADDLE, {"x0", "dW1"}), ("stray_plane", "tail", E.STRADDLE, {"dx", "dW2", "db2"}),
           ("last_block", "embed", E.ONE_TOKEN_BLOCK, {"dpos", "d_conv"}),
           ("fifth_plane", "embed", E.FIVE_PLANES, {"dW1", "db1", "dpos"}),
           ("fgn", "tail", E.NF_1_2, {"dW2"}),
           ("stale_slice", "dense", E.STALE_SLICE, {"dW"}), ("k17", "dense", E.K17, {"y"}), ("colsum_tail", "dense", E.COLSUM_TAIL, {"db"})]
_FAMILY = dict(embed=(E.embed, E.make_ends, E.EMBED_SUMS, E.ENDS_TOL, "ends"), tail=(E.tail, E.make_ends, E.TAIL_SUMS, E.ENDS_TOL, "ends"),
               dense=(E.dense, E.make_dense, E.DENSE_SUMS, E.DENSE_TOL, "dense"))


@functools.lru_cache(maxsize=None)
def _cpu_figures(family, case):
    fn, make, sums, _, _ = _FAMILY[family]
    inp = make(case)
    return inp, fn(case, inp), fn(case, inp, torch.float32), {k: v for k, v in fn(case, inp, magnitudes=True).items() if k in sums}


@pytest.mark.parametrize("defect,family,case,expected", PLANTED, ids=[f"{d}-{f}" for d, f, _, _ in PLANTED])
def test_bounds_separate_planted_edge_defects_from_rounding_cpu(defect, family, case, expected):
    """Each defect, planted alone into the float64 reference, moves at least one compared tensor by more than 10 x the bound the GPU
    test applies to it, and only the tensors it should; the float32 yardstick itself stays inside every bound."""
    fn, _, _, tol, fam = _FAMILY[family]
    inp, f64, f32, mag = _cpu_figures(family, case)
    own = E.judge(fam, list(f64), f32, f64, f32, mag, tol)
    assert all(r["ok"] for r in own), [r for r in own if not r["ok"]]
    rows = E.judge(fam, list(f64), fn(case, inp, defect=defect), f64, f32, mag, tol)
    moved = {r["name"]: round(r["ratio"], 1) for r in rows if r["ratio"] > 1}
    print(defect, family, moved)
    assert moved and max(moved.values()) > 10, moved
    assert set(moved) <= expected, "the planted defect reaches tensors it should not touch"


# ---------------------------------------------------------------- GPU

def _hold(label, rows):
    bad = E.show(label, rows)
    assert not bad, label + "\n" + "\n".join(bad)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@gpu
def test_every_case_reaches_its_edge_on_the_device():
    """(g) The named property of every case with the device's CU count (a case that misses its edge fails), and the scratch queries
    that need the CU count against the restated planners."""
    from adafortitran_amd import _lib
    lib, cus = _lib.load(), _cus()
    assert _missed(cus) == []
    for c in E.ENDS_CASES:
        S, T, p0, p1, d, adapter, planes = c[:7]
        dims = (planes, S, T, p0, p1, d)
        assert lib.aft_embed_bwd_scratch_bytes(*dims, int(adapter)) == 4 * E.embed_bwd_slice_floats(E.make_dims(*dims, adapter), cus), c
        assert lib.aft_tail_bwd_scratch_bytes(*dims) == 4 * E.tail_bwd_slice_floats(E.make_dims(*dims, False), cus), c
    for dims in E.REFUSALS:
        assert lib.aft_embed_bwd_scratch_bytes(*dims, 0) == 0 and lib.aft_tail_bwd_scratch_bytes(*dims) == 0


@gpu
@pytest.mark.parametrize("case", E.ENDS_CASES, ids=E.ends_id)
def test_ends_match_float64_at_plan_edges(case, switches):
    """(a) embed forward + backward and tail forward + backward of one case."""
    rows_e, rows_t = E.gpu_ends(case, switches)
    _hold(E.ends_id(case) + " embed", rows_e)
    _hold(E.ends_id(case) + " tail", rows_t)


@gpu
@pytest.mark.parametrize("case", E.DENSE_CASES, ids=E.dense_id)
def test_dense_matches_float64_at_plan_edges(case, switches):
    """(b) aft_dense_fwd_f32 + aft_dense_bwd_f32 of one case."""
    _hold(E.dense_id(case), E.gpu_dense(case, switches))


@gpu
@pytest.mark.parametrize("case", E.EMPTY_SLICES, ids=E.dense_id)
def test_empty_trailing_slices_do_not_leak_the_scratch(case, switches):
    """(d) launch_gemm_tn rounds the per-slice row chunk up to 16, so 28 of 256 slices start past the last row: they must be written
    as zeros.  The scratch holds 1e30 before the call."""
    _hold(E.dense_id(case) + " scratch 1e30", E.gpu_dense(case, switches, fill=1e30))


@gpu
@pytest.mark.parametrize("case", E.ADAPTER_CASES, ids=E.adapter_id)
def test_adapter_matches_float64(case):
    """(c) aft_adapter_fwd_train_f32, then aft_adapter_bwd_f32 on the activations it wrote."""
    rows_f, rows_b = E.gpu_adapter(case)
    _hold(E.adapter_id(case) + " forward", rows_f)
    _hold(E.adapter_id(case) + " backward", rows_b)


def _prefill(seed, like):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return {k: torch.randn(v.shape).cuda() for k, v in like.items()}


@gpu
def test_accumulate_adds_the_gradient_onto_prefilled_tensors():
    """(e) accumulate = 1: every summed gradient is prefill + the overwriting call's gradient to ONE float32 addition (the reduction
    adds its fixed-order sum to what is there); the data gradients are overwritten either way."""
    case = E.ACCUMULATE["ends"]
    dev = E._cuda(E.make_ends(case))
    for hip, sums, data in ((E.hip_embed, E.EMBED_SUMS, ("x0", "d_conv")), (E.hip_tail, E.TAIL_SUMS, ("out", "dx"))):
        plain = hip(case, dev)
        pre = _prefill(71, {k: plain[k] for k in sums})
        acc = hip(case, dev, prefill=pre)
        for k in data:
            assert torch.equal(acc[k], plain[k]), k
        for k in sums:
            assert torch.equal(acc[k], pre[k] + plain[k]) and not torch.equal(acc[k], plain[k]), k
    case = E.ACCUMULATE["dense"]
    dev = E._cuda(E.make_dense(case))
    plain = E.hip_dense(case, dev)
    pre = _prefill(72, {k: plain[k] for k in E.DENSE_SUMS})
    acc = E.hip_dense(case, dev, prefill=pre)
    assert torch.equal(acc["y"], plain["y"]) and torch.equal(acc["dx"], plain["dx"])
    for k in E.DENSE_SUMS:
        assert torch.equal(acc[k], pre[k] + plain[k]) and not torch.equal(acc[k], plain[k]), k
    case = E.ACCUMULATE["adapter"]
    inp = E.make_adapter(case)
    dev = dict(params=[p.cuda() for p in inp["params"]], conds=[c.cuda() for c in inp["conds"]], dtok=inp["dtok"].cuda())
    plain = E.hip_adapter(case, dev)
    pre = _prefill(73, {k: plain[k] for k in E.ADAPTER_GRADS})
    acc = E.hip_adapter(case, dev, prefill=[pre[k].view(p.shape) for k, p in zip(E.ADAPTER_GRADS, dev["params"])])
    for k in ("tok6", "da0", "da1"):
        assert torch.equal(acc[k], plain[k]), k
    for k in E.ADAPTER_GRADS:
        assert torch.equal(acc[k], pre[k] + plain[k]) and not torch.equal(acc[k], plain[k]), k


@gpu
@pytest.mark.parametrize("dims", E.REFUSALS, ids=lambda v: "x".join(map(str, v)))
def test_ends_refuse_what_they_do_not_cover(dims):
    """(f) A patch of 33 elements, d = 516, d = 6, S % p0 != 0: every entry point returns AFT_ERR_* and leaves the NaN-filled outputs
    untouched."""
    from adafortitran_amd import _abi
    planes, S, T, p0, p1, d = dims
    tokens, p = (S // p0) * (T // p1), p0 * p1
    names = ("conv", "w1", "b1", "pos", "dx0", "x", "w2", "b2", "resid", "d_out")
    shapes = ((planes, S, T), (d, p), (d,), (tokens, d), (planes, tokens, d), (planes, tokens, d), (p, d), (p,), (planes, S, T), (planes, S, T))
    dev = {n: torch.randn(*s, device="cuda") for n, s in zip(names, shapes)}
    dev["tok6"] = None
    case = (S, T, p0, p1, d, False, planes, (), True)
    for hip in (E.hip_embed, E.hip_tail):
        rc_f, rc_b, out = hip(case, dev, check=False)
        assert rc_f in (_abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE) and rc_b in (_abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE)
        for k, v in out.items():
            assert v is None or bool(torch.isnan(v).all()), k


@gpu
def test_adapter_backward_refuses_a_second_layer_wider_than_64():
    from adafortitran_amd import _abi
    case = (E.ADAPTER_REFUSED, 2)
    inp = E.make_adapter(case)
    dev = dict(params=[p.cuda() for p in inp["params"]], conds=[c.cuda() for c in inp["conds"]], dtok=inp["dtok"].cuda())
    rc_f, rc_b, out = E.hip_adapter(case, dev, check=False)
    assert rc_f == _abi.AFT_OK and rc_b == _abi.AFT_ERR_SHAPE
    for k in ("da0", "da1") + E.ADAPTER_GRADS:
        assert bool(torch.isnan(out[k]).all()), k
