"""OFDM grids longer than 64 symbols on the GPU: the conv stacks split a plane into column tiles whose halo columns
are recomputed.  Inference against the CPU oracle on grids the band plan cannot hold, the bits against the batch, a stale workspace
and the number of column tiles, AFT_CONV_COLUMN_TILES on the default grid against the existing kernels, and the training kernels of
the conv stack against float64 autograd."""
import numpy as np
import pytest
import torch

import adafortitran_amd as A
from adafortitran_amd import _abi, synth
from adafortitran_amd.hip_ops import engine_from_numpy
from helpers import DEFAULT_SPEC, TOL_HIP_OUT, max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _spec(ofdm, pilot, patch, d=64, heads=2, layers=1):
    return dict(ofdm=ofdm, pilot=pilot, patch=patch, num_layers=layers, model_dim=d, num_head=heads)


def _tokens(spec):
    return synth.token_count(*spec["ofdm"], spec["patch"])


def _setup(spec, adaptive, seed=3):
    tok = _tokens(spec)
    hid = (5, 9, 2 * tok) if adaptive else None
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, seed=seed, max_seq_len=max(512, tok))
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    return cfg, sd, hid


def _inputs(spec, batch, adaptive, seed=7):
    inp = synth.make_inputs(batch, ofdm=spec["ofdm"], pilot=spec["pilot"], seed=seed)
    meta = [(inp[k] if adaptive else None) for k in ("snr", "ds", "dop")]
    return inp["pilots"], meta


def _hip(eng, pilots, meta):
    return eng.forward(_t(pilots), *[None if m is None else _t(m) for m in meta])


# (ofdm, pilot, patch, model_dim, heads, adaptive, batch): T from 65 to 600, S from 3 to 300, both engines (model_dim 48 / 200 are
# the general engine's), planes of one row tile to planes > 240 rows (row bands x column tiles)
RANDOM_CASES = [
    ((24, 140), (4, 4), (3, 2), 64, 2, False, 3),
    ((24, 140), (4, 4), (4, 7), 64, 2, True, 2),
    ((120, 66), (12, 2), (3, 2), 128, 4, True, 2),
    ((120, 65), (12, 5), (3, 5), 128, 4, False, 1),
    ((12, 560), (4, 8), (3, 8), 64, 2, False, 2),
    ((3, 1000), (3, 8), (3, 10), 64, 2, True, 3),
    ((3, 600), (1, 8), (1, 6), 48, 2, False, 5),
    ((6, 600), (2, 12), (3, 4), 200, 8, False, 2),
    ((264, 72), (8, 4), (8, 2), 64, 2, False, 1),
    ((300, 100), (10, 4), (6, 5), 64, 4, True, 1),
    ((250, 80), (5, 4), (5, 4), 48, 2, False, 1),
    ((240, 70), (12, 2), (6, 5), 64, 2, True, 1),
    ((60, 130), (6, 2), (6, 5), 96, 3, False, 2),
    ((36, 201), (6, 3), (6, 3), 64, 2, False, 2),
    ((48, 96), (8, 4), (4, 4), 64, 1, True, 4),
    ((18, 333), (3, 3), (3, 9), 200, 8, True, 2),
    ((9, 450), (3, 6), (3, 9), 64, 2, False, 3),
    ((100, 65), (10, 5), (5, 5), 48, 2, True, 2),
    ((30, 256), (6, 4), (5, 4), 128, 4, False, 3),
    ((150, 90), (10, 6), (5, 6), 64, 2, False, 1),
]


@pytest.mark.parametrize("case", RANDOM_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}_d{c[3]}{'_ada' if c[5] else ''}_B{c[6]}")
def test_long_grids_match_oracle(oracle_lib, case):
    ofdm, pilot, patch, d, heads, adaptive, batch = case
    spec = _spec(ofdm, pilot, patch, d, heads)
    cfg, sd, _ = _setup(spec, adaptive)
    eng = engine_from_numpy(cfg, sd, DEV)
    pilots, meta = _inputs(spec, batch, adaptive)
    out = _hip(eng, pilots, meta).cpu().numpy()
    ref = oracle_lib.Oracle(cfg, sd).forward(pilots, *meta)
    assert np.isfinite(out.view(np.float32)).all()
    assert np.abs(out - ref).max() <= TOL_HIP_OUT * np.abs(ref).max(), (np.abs(out - ref).max(), np.abs(ref).max())


@pytest.mark.parametrize("ofdm,pilot,patch", [((24, 140), (4, 4), (3, 2)), ((264, 72), (8, 4), (3, 2))])
def test_long_grid_stages_match_oracle(oracle_lib, ofdm, pilot, patch):
    """The head of the forward (forward_region) and the two stage entry points that run the conv stacks on their own inputs (the
    upsampler streamed in the kernel, linear_2 applied from the LDS) against the oracle's intermediates."""
    spec = _spec(ofdm, pilot, patch)
    cfg, sd, _ = _setup(spec, False)
    eng = engine_from_numpy(cfg, sd, DEV)
    pilots, meta = _inputs(spec, 2, False)
    orc = oracle_lib.Oracle(cfg, sd)
    ref, dump = orc.forward(pilots, *meta, dump=True)
    out = _hip(eng, pilots, meta)
    assert max_rel(eng.forward_region("conv_enhanced", 2).cpu().numpy(), dump["conv_enhanced"]) <= TOL_HIP_OUT
    assert max_rel(eng.stage_upsample(_t(pilots)).cpu().numpy(), dump["conv_enhanced"]) <= TOL_HIP_OUT
    assert max_rel(out.cpu().numpy(), ref) <= TOL_HIP_OUT
    tail = eng.stage_tail(_t(dump["layer_out"][-1]), _t(dump["conv_enhanced"])).cpu().numpy()
    assert max_rel(tail, ref) <= TOL_HIP_OUT


def test_long_grid_estimators_construct_and_run_on_the_kernels(oracle_lib):
    """A GPU FortiTranEstimator / AdaFortiTranEstimator on a 140-symbol grid constructs without AFT_ALLOW_COMPOSITE, trains on the
    library's kernels (training_backends all None) and its eval() forward on CPU inputs matches the oracle."""
    from test_estimators_cpu import _configs
    for adaptive in (False, True):
        spec = _spec((24, 140), (4, 4), (3, 2))
        cfg, sd, hid = _setup(spec, adaptive)
        sc, mc = _configs(dict(spec, adaptive_hidden=hid, max_seq_len=max(512, _tokens(spec))), device="cuda")
        model = (A.AdaFortiTranEstimator if adaptive else A.FortiTranEstimator)(sc, mc)
        assert set(model.training_backends().values()) == {None}
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        model.eval()
        pilots, meta = _inputs(spec, 3, adaptive)
        with torch.no_grad():
            cond = (None, *(torch.from_numpy(m) for m in meta), None, None) if adaptive else None   # the reference dataset's tuple
            out = model(torch.from_numpy(pilots), cond).cpu().numpy()
        ref = oracle_lib.Oracle(cfg, sd).forward(pilots, *meta)
        assert np.abs(out - ref).max() <= TOL_HIP_OUT * np.abs(ref).max()


@pytest.mark.parametrize("ofdm,pilot,patch", [((24, 140), (4, 4), (3, 2)), ((120, 66), (12, 2), (3, 2)), ((264, 72), (8, 4), (3, 2))])
def test_long_grid_bits_do_not_depend_on_batch_workspace_or_tiles(switches, ofdm, pilot, patch):
    """Halo columns are recomputed, never exchanged: the same frames alone and inside a 130-frame batch, through a NaN-filled
    workspace, and with the column split forced to 3, 5 or 9 tiles (row-streaming and banded kernels) carry the same bits."""
    spec = _spec(ofdm, pilot, patch)
    cfg, sd, _ = _setup(spec, False)
    eng = engine_from_numpy(cfg, sd, DEV)
    pilots, meta = _inputs(spec, 130, False)
    pil = _t(pilots)
    big = torch.view_as_real(eng.forward(pil, None, None, None)).clone()
    small = torch.view_as_real(eng.forward(pil[:4].contiguous(), None, None, None)).clone()
    assert torch.isfinite(big).all()
    assert torch.equal(big[:4], small)
    eng.workspace(4).view(torch.float32).fill_(float("nan"))
    assert torch.equal(torch.view_as_real(eng.forward(pil[:4].contiguous(), None, None, None)), small)
    for banded in (False, True):
        if banded:
            switches.set("AFT_CONV_BANDED", "1")
        base = None
        for tiles in (None, "3", "5", "9"):
            if tiles is None:
                switches.unset("AFT_CONV_COLUMN_TILES")
            else:
                switches.set("AFT_CONV_COLUMN_TILES", tiles)
            out = torch.view_as_real(eng.forward(pil[:4].contiguous(), None, None, None)).clone()
            base = out if base is None else base
            assert torch.equal(out, base), (banded, tiles)
        switches.unset("AFT_CONV_COLUMN_TILES")
        switches.unset("AFT_CONV_BANDED")


def test_forced_column_tiles_on_the_default_grid_agree_with_the_existing_kernels(switches):
    """AFT_CONV_COLUMN_TILES=1 on 120 x 14 at 128 frames: the forward and the conv stack's gradients on the column-tiled path against
    the default grid's kernels, at the rounding level (conv4's summation order differs)."""
    from adafortitran_amd.training import HipConvEnhancerFunction
    hid = (7, 42, 560)
    sd = synth.make_state_dict(**DEFAULT_SPEC, adaptive_hidden=hid, seed=21)
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=hid)
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(128, seed=22)
    args = [_t(inp[k]) for k in ("pilots", "snr", "ds", "dop")]
    ref = torch.view_as_real(eng.forward(*args)).clone()
    switches.set("AFT_CONV_COLUMN_TILES", "1")
    out = torch.view_as_real(eng.forward(*args)).clone()
    switches.unset("AFT_CONV_COLUMN_TILES")
    assert (out - ref).abs().max() <= 2e-6 * ref.abs().max()

    import adafortitran_amd.blocks as blocks
    torch.manual_seed(4)
    enh = blocks.ConvEnhancer().to(DEV)
    params = [p.detach() for p in enh.parameters()]
    x0 = torch.randn(256, 1, 120, 14, device=DEV)
    gy = torch.randn(256, 1, 120, 14, device=DEV)

    def run():
        x = x0.clone().requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for p in params]
        y = HipConvEnhancerFunction.apply(x, *ps)
        y.backward(gy)
        return [y.detach(), x.grad] + [p.grad for p in ps]

    base = run()
    switches.set("AFT_CONV_COLUMN_TILES", "1")
    tiled = run()
    switches.unset("AFT_CONV_COLUMN_TILES")
    for i, (a, b) in enumerate(zip(tiled, base)):
        assert (a - b).abs().max() <= 2e-6 * b.abs().max(), i


def _conv_ref64(x, params):
    """ConvEnhancer (reference blocks/enhancers.py:12-20) in float64 on the CPU: y and the gradients of <y, gy>."""
    import torch.nn.functional as F
    w1, b1, w2, b2, w3, b3, w4, b4 = params
    h = F.relu(F.conv2d(x, w1, b1, padding=1))
    h = F.relu(F.conv2d(h, w2, b2, padding=1))
    h = F.relu(F.conv2d(h, w3, b3, padding=1))
    return F.conv2d(h, w4, b4, padding=1)


@pytest.mark.parametrize("S,T,n", [(24, 140, 3), (264, 72, 2), (3, 300, 2)])
def test_conv_enhancer_training_on_long_grids_matches_float64(switches, S, T, n):
    """HipConvEnhancerFunction (training forward with the saved activations, the dgrad run, the weight gradients) on grids without a
    band plan against float64 autograd; the bits do not depend on the number of column tiles."""
    import adafortitran_amd.blocks as blocks
    from adafortitran_amd.training import HipConvEnhancerFunction
    torch.manual_seed(S + T)
    enh = blocks.ConvEnhancer()
    params = [p.detach().to(DEV) for p in enh.parameters()]
    x0 = torch.randn(n, 1, S, T, device=DEV)
    gy = torch.randn(n, 1, S, T, device=DEV)

    def run():
        x = x0.clone().requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for p in params]
        y = HipConvEnhancerFunction.apply(x, *ps)
        y.backward(gy)
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in ps]

    hip = run()
    x64 = x0.double().cpu().requires_grad_(True)
    p64 = [p.double().cpu().requires_grad_(True) for p in params]
    y64 = _conv_ref64(x64, p64)
    y64.backward(gy.double().cpu())
    ref = [y64.detach(), x64.grad] + [p.grad for p in p64]
    tol = [2e-5, 1e-4] + [2e-4] * 8
    for i, (a, b, t) in enumerate(zip(hip, ref, tol)):
        assert float((a.double().cpu() - b).abs().max() / b.abs().max()) <= t, i
    switches.set("AFT_CONV_COLUMN_TILES", "7")
    again = run()
    switches.unset("AFT_CONV_COLUMN_TILES")
    assert torch.equal(again[0], hip[0]) and torch.equal(again[1], hip[1])


def test_conv_training_past_2_gib_of_activations_runs_in_chunks():
    """256 planes of 120 x 600: conv2's saved activations are 2.4 GB, past the kernels' 32-bit offsets, so the call runs as two
    launches.  Output and data gradient of the first and last planes equal those planes run alone; the weight gradients equal the
    sum over two halves of the batch."""
    import adafortitran_amd.blocks as blocks
    from adafortitran_amd.training import HipConvEnhancerFunction
    torch.manual_seed(9)
    params = [p.detach().to(DEV) for p in blocks.ConvEnhancer().parameters()]
    x0 = torch.randn(256, 1, 120, 600, device=DEV)
    gy = torch.randn(256, 1, 120, 600, device=DEV)

    def run(sl):
        x = x0[sl].clone().requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for p in params]
        y = HipConvEnhancerFunction.apply(x, *ps)
        y.backward(gy[sl])
        return [y.detach(), x.grad] + [p.grad for p in ps]

    full = run(slice(0, 256))
    for sl in (slice(0, 2), slice(254, 256)):
        part = run(sl)
        assert torch.equal(part[0], full[0][sl]) and torch.equal(part[1], full[1][sl]), sl
    a, b = run(slice(0, 128)), run(slice(128, 256))
    for i in range(2, 10):
        ref = a[i] + b[i]
        assert (full[i] - ref).abs().max() <= 1e-5 * ref.abs().max(), i
