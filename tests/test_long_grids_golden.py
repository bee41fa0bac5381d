"""Grids longer than 64 symbols pinned on the reference itself (tests/golden/make_golden_long_grids.py): 24 x 140 (FortiTran, 560
tokens; AdaFortiTran with 4 x 7 patches, the general engine) and 264 x 72 (row bands x column tiles), and one training
step on 24 x 140 with its float64 twin.  CPU: the oracle and the PyTorch composite against the fixtures.  GPU: HipEngine, the module
surface and the HIP training step."""
import numpy as np
import pytest
import torch

import adafortitran_amd as A
from adafortitran_amd import synth
from helpers import TOL_HIP_MSE, TOL_HIP_OUT, TOL_ORACLE_OUT, TOL_ORACLE_STAGE, Golden, max_rel
from test_train_golden import COND_FACTOR, _check, _errors64, _row_view, _tokens

DEV = "cuda:0"
SETS = ["X140_forti_grid24x140", "X140_ada_grid24x140_p4x7", "X72_forti_grid264x72"]
GRAD = "G_grad_forti_t140"
# HIP vs float64 (element base, norm base) + COND_FACTOR x gcond, as tests/test_train_golden.py's BASE64: the PyTorch composite's
# fp32 step on the CPU is at most 9.5e-7 of |g|max from the float64 one (the reference's own fp32 step: 7.4e-7); base = ten times that,
# for sums over 67 200 pixels per plane in the kernels' order
BASE64_T140 = (1e-5, 1e-5)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("name", SETS)
def test_oracle_matches_long_grid_reference_cpu(oracle_lib, name):
    g = Golden(name)
    orc = oracle_lib.Oracle(g.abi_config(), g.state_dict())
    out, dump = orc.forward(g["pilots"], *g.meta_arrays(), dump=True)
    assert np.abs(out - g["out"]).max() <= TOL_ORACLE_OUT * max(1.0, np.abs(g["out"]).max())
    for st in ("conv_enhanced", "enc_out", "tokens6"):
        if st in g:
            assert max_rel(dump[st], g[st]) <= TOL_ORACLE_STAGE, (st, max_rel(dump[st], g[st]))


def _model(spec, device, dropout=None):
    sc = A.SystemConfig(ofdm=dict(num_scs=spec["ofdm"][0], num_symbols=spec["ofdm"][1]),
                        pilot=dict(num_scs=spec["pilot"][0], num_symbols=spec["pilot"][1]))
    kw = dict(model_type="adafortitran" if spec.get("adaptive_hidden") else "fortitran", patch_size=tuple(spec["patch"]),
              num_layers=spec["num_layers"], model_dim=spec["model_dim"], num_head=spec["num_head"],
              activation=spec.get("activation", "gelu"), max_seq_len=spec["max_seq_len"], pos_encoding_type="learnable", device=device)
    if dropout is not None:
        kw["dropout"] = dropout
    if spec.get("adaptive_hidden"):
        kw.update(channel_adaptivity_hidden_sizes=list(spec["adaptive_hidden"]), adaptive_token_length=6)
    return (A.AdaFortiTranEstimator if spec.get("adaptive_hidden") else A.FortiTranEstimator)(sc, A.ModelConfig(**kw))


def _train_step(device):
    """One training step of the fixture's model, as make_golden.py::run_grad runs it on the reference."""
    g = Golden(GRAD)
    model = _model(g.spec, device, dropout=g.spec["dropout"])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()}, strict=True)
    model.train()
    out = model(torch.from_numpy(g["pilots"]))
    tgt = torch.from_numpy(g["target"]).to(out.device)
    cat = lambda z: torch.cat((torch.real(z), torch.imag(z)), dim=1)  # noqa: E731
    loss = torch.nn.MSELoss()(cat(out), cat(tgt))
    loss.backward()
    return g, model, float(loss.detach())


def _failures64(model):
    g64 = Golden(GRAD.replace("G_grad_", "G_grad64_"))
    grads = {n: p.grad.detach().reshape(-1).cpu().numpy() for n, p in model.named_parameters()}
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters()}
    bad = []
    for n, (e, en, es, where) in _errors64(g64, grads, shapes).items():
        tol_e = BASE64_T140[0] + COND_FACTOR * float(g64[f"gcond__{n}"])
        tol_n = BASE64_T140[1] + COND_FACTOR * float(g64[f"gcondnorm__{n}"])
        if e > tol_e or en > tol_n or es > tol_e:
            bad.append(f"{n}: elem {e:.2e} spread {es:.2e} at {where} (tol {tol_e:.2e}) norm {en:.2e} (tol {tol_n:.2e})")
    pe = "transformer_encoder.positional_encoding.position_embeddings"
    rows = grads[pe].reshape(_row_view(shapes[pe]))
    if np.any(rows[_tokens(g64.spec):] != 0):
        bad.append(f"{pe}: rows past the grid's tokens not zero")
    return bad


def test_composite_long_grid_training_step_matches_reference_cpu():
    """The PyTorch composite on the CPU: the reference's own fp32 step at the existing fp32 tolerance, and the float64 rule."""
    g, model, loss = _train_step("cpu")
    _check(g, model, loss, 2e-5)
    assert not _failures64(model)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_hip_engine_matches_long_grid_reference(name):
    from adafortitran_amd.hip_ops import engine_from_numpy
    g = Golden(name)
    eng = engine_from_numpy(g.abi_config(), g.state_dict(), DEV)
    meta = [None if m is None else _t(m) for m in g.meta_arrays()]
    out = eng.forward(_t(g["pilots"]), *meta).cpu().numpy()
    assert np.abs(out - g["out"]).max() <= TOL_HIP_OUT * np.abs(g["out"]).max()
    mse = np.mean(np.abs(out - g["target"]) ** 2)
    assert abs(mse - g.meta["metric_2xmse"]) / g.meta["metric_2xmse"] <= TOL_HIP_MSE
    B = g["pilots"].shape[0]
    assert max_rel(eng.forward_region("conv_enhanced", B).cpu().numpy(), g["conv_enhanced"]) <= TOL_HIP_OUT
    if "tokens6" in g:
        assert max_rel(eng.forward_region("tokens6", B).cpu().numpy(), g["tokens6"]) <= TOL_HIP_OUT
    assert max_rel(eng.stage_upsample(_t(g["pilots"])).cpu().numpy(), g["conv_enhanced"]) <= TOL_HIP_OUT


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_module_surface_matches_long_grid_reference(name):
    """eval() forward of the estimator built on the HIP device (no AFT_ALLOW_COMPOSITE) on CPU inputs."""
    g = Golden(name)
    model = _model(g.spec, "cuda")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()})
    model.eval()
    with torch.no_grad():
        pil = torch.from_numpy(g["pilots"])
        meta = synth.meta_tuple({k: g[k] for k in ("snr", "ds", "dop")}) if g.adaptive else None
        out = (model(pil, meta) if meta is not None else model(pil)).cpu().numpy()
    assert np.abs(out - g["out"]).max() <= TOL_HIP_OUT * np.abs(g["out"]).max()


@pytest.mark.gpu
def test_hip_long_grid_training_step_matches_float64_reference():
    """A whole training step on the 140-symbol grid through the library's kernels (upsampler, conv stacks on column tiles, embedding
    and tail at 560 tokens, encoder layers, loss glue): the reference's fp32 step at test_train_golden.py's HIP tolerance and the
    float64 step under base + 2 x gcond, every row."""
    g, model, loss = _train_step("cuda")
    assert all(v is None for v in model.training_backends().values())
    assert model.transformer_encoder._hip_train_eligible(torch.empty(2, 560, 64, device="cuda"))
    _check(g, model, loss, 5e-4)
    bad = _failures64(model)
    assert not bad, "\n".join(bad)
