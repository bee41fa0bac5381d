"""tests/test_lds_poison.py for the column-tiled conv paths of grids longer than 64 symbols: the row-streaming kernel
with column ranges sized by the LDS, the banded kernel with row bands x column tiles (inference, stage entry points, training forward
and dgrad).  Run clean, then behind a NaN / 1e30 / -inf fill of every CU's LDS: the same BITS."""
import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, synth
from adafortitran_amd.hip_ops import engine_from_numpy, fill_lds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISONS = [float("nan"), 1e30, float("-inf")]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


CASES = {
    "rows_120x66": (dict(ofdm=(120, 66), pilot=(12, 2), patch=(3, 2), num_layers=1, model_dim=64, num_head=2), False, 3, False),
    "rows_ada_3x600": (dict(ofdm=(3, 600), pilot=(3, 8), patch=(3, 10), num_layers=1, model_dim=64, num_head=2), True, 4, False),
    "tiles_24x140": (dict(ofdm=(24, 140), pilot=(4, 4), patch=(3, 2), num_layers=1, model_dim=64, num_head=2), False, 3, False),
    "banded_120x66": (dict(ofdm=(120, 66), pilot=(12, 2), patch=(3, 2), num_layers=1, model_dim=64, num_head=2), False, 3, True),
    "tiles2d_264x72": (dict(ofdm=(264, 72), pilot=(8, 4), patch=(8, 2), num_layers=1, model_dim=64, num_head=2), False, 2, False),
    "tiles2d_general_300x100": (dict(ofdm=(300, 100), pilot=(10, 4), patch=(6, 5), num_layers=1, model_dim=48, num_head=2), True, 1, False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_long_grid_forward_bits_do_not_depend_on_what_the_lds_held(switches, case):
    spec, adaptive, batch, banded = CASES[case]
    tokens = synth.token_count(*spec["ofdm"], spec["patch"])
    hid = (5, 11, 2 * tokens) if adaptive else None
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, seed=11, max_seq_len=max(512, tokens))
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    if banded:
        switches.set("AFT_CONV_BANDED", "1")
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(batch, ofdm=spec["ofdm"], pilot=spec["pilot"], seed=12)
    meta = [(_t(inp[k]) if adaptive else None) for k in ("snr", "ds", "dop")]
    pil = _t(inp["pilots"])
    ref = eng.forward(pil, *meta).clone()
    up = eng.stage_upsample(pil).clone()
    assert torch.isfinite(torch.view_as_real(ref)).all() and torch.isfinite(up).all()
    for value in POISONS:
        fill_lds(value, DEV)
        out = eng.forward(pil, *meta)
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(ref)), (case, value)
        fill_lds(value, DEV)
        assert torch.equal(eng.stage_upsample(pil), up), (case, value)


@pytest.mark.parametrize("S,T", [(24, 140), (264, 72)])
def test_long_grid_conv_training_bits_do_not_depend_on_what_the_lds_held(S, T):
    """HipConvEnhancerFunction (training forward with saved activations, dgrad, weight gradients) on column tiles behind an LDS fill."""
    import adafortitran_amd.blocks as blocks
    from adafortitran_amd.training import HipConvEnhancerFunction
    torch.manual_seed(3)
    params = [p.detach().to(DEV) for p in blocks.ConvEnhancer().parameters()]
    x0 = torch.randn(3, 1, S, T, device=DEV)
    gy = torch.randn(3, 1, S, T, device=DEV)

    def run():
        x = x0.clone().requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for p in params]
        y = HipConvEnhancerFunction.apply(x, *ps)
        y.backward(gy)
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in ps]

    ref = run()
    assert all(torch.isfinite(r).all() for r in ref)
    for value in POISONS:
        fill_lds(value, DEV)
        got = run()
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), (value, i)
