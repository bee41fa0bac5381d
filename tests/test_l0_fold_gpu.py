"""Layer 0's keys and values from the input features ("the fold"; AFT_L0_FOLD, default on).

With x0 = W1 in + b1 + pos[t] the first encoder launch forms K[t] = (Wk W1) in + Wk (b1 + pos[t]) and V[t] likewise (+ bv) on tables the
prologue launch rebuilds in every call, instead of a model_dim-deep product over x0.  That is a change of ROUNDING against AFT_L0_FOLD=0
(the parent's arithmetic), so both arms are held against the CPU oracle and the reference's goldens at the stated fp32 tolerance; between
the paths of one build (fused layers or launches, batch, lanes, stale workspaces, a caller-owned packed image) the bits are equal."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import adafortitran_amd as A
from adafortitran_amd import _abi, _lib, synth
from helpers import DEFAULT_SPEC, Golden, TOL_HIP_OUT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2 = dict(DEFAULT_SPEC, num_layers=2)

# name -> (spec, adaptive hidden sizes, max_seq_len).  Two layers unless the case is about the layer count.
CASES = {
    "280_ragged_ninth_tile": (L2, (7, 42, 560), 512),
    "224_whole_tiles_attn_is_two_tables": (dict(L2, ofdm=(96, 14)), (7, 42, 448), 512),
    "33_one_valid_row_in_last_tile": (dict(L2, ofdm=(99, 2), pilot=(11, 1)), (7, 42, 66), 512),
    "210_patch_4x2_K14": (dict(L2, patch=(4, 2)), (7, 42, 420), 512),
    "28_launch_path_tokpad_above_tokens": (dict(ofdm=(12, 14), pilot=(4, 2), patch=(3, 2), num_layers=2, model_dim=64, num_head=2), (7, 42, 56), 32),
    "d256_heads8": (dict(L2, model_dim=256, num_head=8), (7, 42, 560), 512),
    "one_layer": (dict(DEFAULT_SPEC, num_layers=1), (7, 42, 560), 512),
}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _setup(spec, hid, batch, seed, max_seq_len=512, **gains):
    from adafortitran_amd.hip_ops import engine_from_numpy
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, max_seq_len=max_seq_len, seed=seed, **gains)
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    inp = synth.make_inputs(batch, ofdm=spec["ofdm"], pilot=spec["pilot"], seed=seed + 1)
    meta = [_t(inp[k]) for k in ("snr", "ds", "dop")] if hid else []
    return engine_from_numpy(cfg, sd, DEV), _t(inp["pilots"]), meta, (cfg, sd, inp)


def _arms(switches, eng, pil, meta):
    """The forward with AFT_L0_FOLD at 1 and at 0, as complex numpy arrays."""
    out = {}
    for v in ("1", "0"):
        switches.set("AFT_L0_FOLD", v)
        out[v] = eng.forward(pil, *meta).cpu().numpy()
    return out["1"], out["0"]


def _rel_err(out, ref):
    return float(np.abs(out - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_both_arms_match_the_oracle(switches, oracle_lib, case, adaptive, batch):
    spec, hid, msl = CASES[case]
    hid = hid if adaptive else None
    eng, pil, meta, (cfg, sd, inp) = _setup(spec, hid, batch, seed=1100 + 7 * list(CASES).index(case) + batch, max_seq_len=msl)
    ref = oracle_lib.Oracle(cfg, sd).forward(inp["pilots"], *([inp["snr"], inp["ds"], inp["dop"]] if adaptive else [None] * 3))
    folded, deep = _arms(switches, eng, pil, meta)
    e1, e0 = _rel_err(folded, ref), _rel_err(deep, ref)
    print(f"{case} adaptive={adaptive} batch={batch}: max|out - oracle| / |y|max  folded {e1:.3e}  128-deep {e0:.3e}")
    assert np.isfinite(folded).all() and np.isfinite(deep).all()
    assert e1 <= TOL_HIP_OUT and e0 <= TOL_HIP_OUT, (e1, e0)


def test_hot_logits_keep_the_unfolded_arms_accuracy(switches, oracle_lib):
    """Logits of several hundred in layer 0 (attn_gain = 32 synthetic weights against the oracle; the reference's own A_ada and
    DH_forti_hot goldens): K's and V's rounding reaches the softmax amplified.  The unfolded arm is the parent's arithmetic; the folded
    one may exceed its error by at most a factor of 2 -- two fp32 roundings in place of one, nothing more -- and stays under the stated
    tolerance.  Both figures per set go to profiles/l0_fold_accuracy.json."""
    figures = {}
    # the synthetic hot set of test_hip_parity.py::test_ragged_batches_match_oracle (no adapter: with the adapter's features at this gain
    # the softmax of six layers is an argmax whose ties flip -- the parent's arithmetic is 0.26 |y|max off the oracle there, measured)
    eng, pil, meta, (cfg, sd, inp) = _setup(DEFAULT_SPEC, None, 3, seed=4242, attn_gain=32.0, head_gain=2.0)
    ref = oracle_lib.Oracle(cfg, sd).forward(inp["pilots"], None, None, None)
    folded, deep = _arms(switches, eng, pil, meta)
    figures["synth_attn_gain_32"] = {"folded": _rel_err(folded, ref), "unfolded": _rel_err(deep, ref)}
    from adafortitran_amd.hip_ops import engine_from_numpy
    for name in ("A_ada", "DH_forti_hot"):
        g = Golden(name)
        eng = engine_from_numpy(g.abi_config(), g.state_dict(), DEV)
        meta = [_t(g[k]) for k in ("snr", "ds", "dop")] if g.adaptive else []
        folded, deep = _arms(switches, eng, _t(g["pilots"]), meta)
        figures[name] = {"folded": _rel_err(folded, g["out"]), "unfolded": _rel_err(deep, g["out"])}
    for name, f in figures.items():
        print(f"{name}: max|out - reference| / |y|max  folded {f['folded']:.3e}  unfolded {f['unfolded']:.3e}")
    with open(os.path.join(ROOT, "profiles", "l0_fold_accuracy.json"), "w") as fh:
        json.dump({"what": "max|out - reference| / |y|max with AFT_L0_FOLD=1 (folded) and =0 (unfolded); tolerance 5e-5",
                   "sets": {k: {a: float(f"{v:.4e}") for a, v in f.items()} for k, f in figures.items()}}, fh, indent=1)
        fh.write("\n")
    for name, f in figures.items():
        assert f["folded"] <= TOL_HIP_OUT, (name, f)
        assert f["folded"] <= 2 * f["unfolded"], (name, f)


# ---- bit-equality between the paths of one build, the fold on ----
HID = (7, 42, 560)


def _real(eng, pil, meta, **kw):
    return torch.view_as_real(eng.forward(pil, *meta, **kw).clone())


def test_fused_layers_and_launches_give_the_same_bits(switches):
    """chain_plane_tiles_kernel (plane-aligned tiles, 16-byte table reads) and chain_kernel<false, true> (global tiles that straddle
    planes, table reads token by token) share the folded body; 280 and 210 tokens (210: no multiple of 4)."""
    switches.set("AFT_L0_FOLD", "1")
    for spec, hid, batch in ((L2, HID, 3), (dict(L2, patch=(4, 2)), (7, 42, 420), 2)):
        eng, pil, meta, _ = _setup(spec, hid, batch, seed=1400 + batch)
        out = {}
        for v in ("0", "1"):
            switches.set("AFT_LAYER_FUSED", v)
            assert _lib.load().aft_layer_fused_of(ctypes.byref(eng.cfg), batch) == int(v)
            out[v] = _real(eng, pil, meta)
        assert torch.isfinite(out["0"]).all()
        assert torch.equal(out["0"], out["1"])


def test_frames_do_not_depend_on_their_batch(switches):
    """Frames 3..7 of a 37-frame call equal a 5-frame call on those frames: the tables do not depend on the batch, the lane or the grid."""
    switches.set("AFT_L0_FOLD", "1")
    eng, pil, meta, _ = _setup(L2, HID, 37, seed=1500)
    big = _real(eng, pil, meta)
    small = _real(eng, pil[3:8], [m[3:8] for m in meta])
    assert torch.equal(big[3:8], small)


def test_two_lanes_and_one_give_the_same_bits(switches):
    """Every lane rebuilds the tables in its own slice of the workspace, in its own prologue launch."""
    switches.set("AFT_L0_FOLD", "1")
    eng, pil, meta, _ = _setup(L2, HID, 6, seed=1600)
    out = {}
    for lanes in ("1", "2"):
        switches.set("AFT_LANES", lanes)
        out[lanes] = _real(eng, pil, meta)
    assert torch.equal(out["1"], out["2"])


def test_bits_do_not_depend_on_the_workspace(switches):
    """The tables' pad tokens, the folded matrices' steps beyond K and everything else the first launch reads are written by the
    prologue of the same call: a NaN- and a 1e30-filled workspace give the bits of a zero-filled one (280 tokens: pad tokens 280..287;
    33 tokens on the fused path; 28 tokens of S28's grid on the launch path)."""
    switches.set("AFT_L0_FOLD", "1")
    s28, hid28, msl28 = CASES["28_launch_path_tokpad_above_tokens"]
    for spec, hid, msl in ((L2, HID, 512), (dict(L2, ofdm=(99, 2), pilot=(11, 1)), None, 512), (s28, hid28, msl28)):
        eng, pil, meta, _ = _setup(spec, hid, 3, seed=1700, max_seq_len=msl)
        outs = []
        for fill in (0.0, float("nan"), 1e30):
            eng.workspace(3).view(torch.float32).fill_(fill)
            outs.append(_real(eng, pil, meta))
        assert torch.isfinite(outs[0]).all()
        assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0]), spec


def test_caller_owned_packed_image_gives_the_stateless_bits(switches):
    """cache_packed=True: the caller's image is read-only (Q's fragments come from it), the fold is still computed per call from the raw
    weights, into the lane's own idle packed-weight slot."""
    switches.set("AFT_L0_FOLD", "1")
    eng, pil, meta, _ = _setup(L2, HID, 3, seed=1800)
    stateless = _real(eng, pil, meta)
    image_before = eng.packed_weights().clone()
    cached = _real(eng, pil, meta, cache_packed=True)
    assert torch.equal(cached, stateless)
    assert torch.equal(eng.packed_weights(), image_before)       # nothing wrote into the caller's image


def test_module_forward_sees_a_raw_write_to_linear_1():
    """The tables and the folded matrices are functions of linear_1's weights: a raw ``.data`` write between two module calls (no version
    counter moves) changes the second output, and restoring the weights restores the bits -- nothing of the fold survives a call."""
    from test_estimators_cpu import _configs
    g = Golden("D_forti")
    sc, mc = _configs(g.spec, device="cuda")
    model = A.FortiTranEstimator(sc, mc)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()})
    model.eval()
    pil = torch.from_numpy(g["pilots"])
    w = model.transformer_encoder.linear_1.weight
    with torch.no_grad():
        out0 = model(pil).clone()
        saved, v0 = w.data.clone(), w._version
        w.data.mul_(1.25)
        assert w._version == v0
        out1 = model(pil).clone()
        assert not torch.equal(torch.view_as_real(out1), torch.view_as_real(out0))
        w.data.copy_(saved)
        out2 = model(pil)
        assert torch.equal(torch.view_as_real(out2), torch.view_as_real(out0))
