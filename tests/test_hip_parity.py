"""GPU parity tests (run with -m gpu on an MI355X): the hand-written HIP path, called through
the C ABI, against (a) golden vectors produced by the reference itself and (b) the CPU oracle on
the same seeded inputs.  Tolerances are the stated fp32 ones of SURVEY.md 8(d)."""
import os

import numpy as np
import pytest
import torch

import adafortitran_amd as A
from adafortitran_amd import _abi, synth
from helpers import DEFAULT_SPEC, Golden, TOL_HIP_MSE, TOL_HIP_OUT, max_rel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DEFAULT_SETS = ["D_forti", "A_ada", "DH_forti_hot", "AH_ada_mid", "AS_ada_sin_relu"]


def _engine(g: Golden):
    from adafortitran_amd.hip_ops import engine_from_numpy
    return engine_from_numpy(g.abi_config(), g.state_dict(), DEV)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _meta(g: Golden):
    return [(_t(g[k]) if g.adaptive else None) for k in ("snr", "ds", "dop")]


def test_extension_is_loaded_in_tree():
    from adafortitran_amd import _lib
    lib = _lib.load()
    assert lib.aft_version() == _abi.AFT_ABI_VERSION
    assert "/adafortitran_amd/csrc/libaft_hip.so" in _lib.lib_path()
    maps = open("/proc/self/maps").read()
    assert "libaft_hip.so" in maps


OTHER_SHAPE_SETS = ["H16_ada_heads8", "H64_forti_heads2", "S28_ada_tokens28",   # head dim 16 / 64; 28 tokens (one masked key tile)
                    "H24_ada_d96_heads4", "H48_forti_d192_heads4",                # head dims 24 / 48: heads that start anywhere in a 32-feature block
                    # round 6, the general engine: model_dim 512, heads of 128 / 56 / 25 features, a 24-element patch;
                    # and 40 layers on the packed engine (more than one window of the layer table the kernels take by value)
                    "W512_ada_d512_heads8", "H128_forti_d256_heads2", "H56_ada_d224_heads4", "D200_forti_d200_heads8", "P24_ada_patch12x2",
                    "L40_forti_layers40"]


@pytest.mark.parametrize("name", DEFAULT_SETS + ["C5_ada_large"] + OTHER_SHAPE_SETS)
def test_forward_matches_reference_golden(name):
    g = Golden(name)
    eng = _engine(g)
    out = eng.forward(_t(g["pilots"]), *_meta(g)).cpu().numpy()
    ref = g["out"]
    err = np.abs(out - ref).max()
    assert err <= TOL_HIP_OUT * np.abs(ref).max(), (err, np.abs(ref).max())
    # metric parity: |dMSE|/MSE against the reference's own 2*MSELoss(cat(Re,Im))
    mse = np.mean(np.abs(out - g["target"]) ** 2)
    assert abs(mse - g.meta["metric_2xmse"]) / g.meta["metric_2xmse"] <= TOL_HIP_MSE


@pytest.mark.parametrize("name", ["D_forti", "A_ada", "DH_forti_hot", "AH_ada_mid"])
def test_stages_match_golden_and_oracle(oracle_lib, name):
    g = Golden(name)
    eng = _engine(g)
    orc = oracle_lib.Oracle(g.abi_config(), g.state_dict())
    _, dump = orc.forward(g["pilots"], *g.meta_arrays(), dump=True)
    ce = eng.stage_upsample(_t(g["pilots"]))
    assert max_rel(ce.cpu().numpy(), g["conv_enhanced"]) <= TOL_HIP_OUT
    tok6 = None
    if g.adaptive:
        tok6 = eng.stage_adapter(*_meta(g))
        assert max_rel(tok6.cpu().numpy(), dump["tokens6"]) <= TOL_HIP_OUT
    x0 = eng.stage_embed(_t(dump["conv_enhanced"]), None if tok6 is None else _t(dump["tokens6"]))
    assert max_rel(x0.cpu().numpy(), dump["x0"]) <= TOL_HIP_OUT
    if "x0_f0" in g:
        assert max_rel(x0[:2].cpu().numpy(), g["x0_f0"]) <= TOL_HIP_OUT
    # every encoder layer on the oracle's input of that layer (no error accumulation)
    xin = dump["x0"]
    for layer in range(g.spec["num_layers"]):
        y = eng.stage_encoder_layer(layer, _t(xin)).cpu().numpy()
        assert max_rel(y, dump["layer_out"][layer]) <= TOL_HIP_OUT, layer
        xin = dump["layer_out"][layer]
    if "layer_first_last_p0" in g:
        L = g.spec["num_layers"]
        y = eng.stage_encoder_layer(L - 1, _t(dump["layer_out"][L - 2])).cpu().numpy()
        assert max_rel(y[0], g["layer_first_last_p0"][1]) <= 4 * TOL_HIP_OUT
    out = eng.stage_tail(_t(dump["layer_out"][-1]), _t(dump["conv_enhanced"])).cpu().numpy()
    assert np.abs(out - g["out"]).max() <= TOL_HIP_OUT * np.abs(g["out"]).max()


@pytest.mark.parametrize("name", ["D_forti", "A_ada", "DH_forti_hot", "AH_ada_mid"])
def test_forward_intermediates_match_golden(name):
    """The kernels aft_forward_f32 itself launches, pinned stage by stage on the reference's own intermediates: on the default grid
    the forward runs the pilot_upsampler product in its prologue launch and the column-streaming conv kernels, which the per-stage
    entry points (no scratch of their own) do not -- so the regions the forward leaves in its workspace are compared directly:
    conv_enhanced (S1+S2, fortitran.py:203-209), the adapter tokens (channel_adaptivity.py:59-63) and linear_2's output
    (encoders.py:70); the tail's residual + refinement is then pinned by `out` given a pinned enc_out and conv_enhanced."""
    g = Golden(name)
    eng = _engine(g)
    B = g["pilots"].shape[0]
    out = eng.forward(_t(g["pilots"]), *_meta(g)).cpu().numpy()
    ce = eng.forward_region("conv_enhanced", B).cpu().numpy()
    assert max_rel(ce, g["conv_enhanced"]) <= TOL_HIP_OUT
    if g.adaptive and "tokens6" in g:
        assert max_rel(eng.forward_region("tokens6", B).cpu().numpy(), g["tokens6"]) <= TOL_HIP_OUT
    enc = eng.forward_region("enc_out", B).cpu().numpy()[:, :, :g["enc_out"].shape[2]]
    assert max_rel(enc, g["enc_out"]) <= 4 * TOL_HIP_OUT       # six layers deep: the stated bound of the layer-chain test above
    assert np.abs(out - g["out"]).max() <= TOL_HIP_OUT * np.abs(g["out"]).max()
    # and the conv kernels of the forward against the stage entry points' (banded) ones on the same inputs: same arithmetic
    ce_stage = eng.stage_upsample(_t(g["pilots"])).cpu().numpy()
    assert max_rel(ce, ce_stage) <= 2e-6


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("batch", [1, 3, 37])
def test_ragged_batches_match_oracle(oracle_lib, adaptive, batch):
    """batch sizes that leave partial 64-row tiles (2B*280 not a multiple of 64)."""
    hid = (7, 42, 560) if adaptive else None
    sd = synth.make_state_dict(**DEFAULT_SPEC, adaptive_hidden=hid, seed=4242, attn_gain=0.25 if adaptive else 32.0,
                               head_gain=2.0)
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(batch, seed=777 + batch)
    meta = [(_t(inp[k]) if adaptive else None) for k in ("snr", "ds", "dop")]
    out = eng.forward(_t(inp["pilots"]), *meta).cpu().numpy()
    orc = oracle_lib.Oracle(cfg, sd)
    ref = orc.forward(inp["pilots"], *([inp["snr"], inp["ds"], inp["dop"]] if adaptive else [None] * 3))
    assert np.abs(out - ref).max() <= TOL_HIP_OUT * np.abs(ref).max()


def test_full_size_batch128_properties(oracle_lib):
    """BASELINE config 3 at full size: frames are independent (fortitran.py:176-177), so the
    B=128 launch must reproduce (i) B=16 chunks bit-for-bit and (ii) the oracle on a sample."""
    hid = (7, 42, 560)
    sd = synth.make_state_dict(**DEFAULT_SPEC, adaptive_hidden=hid, seed=20251114)
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(128, seed=20251114)
    meta = [_t(inp[k]) for k in ("snr", "ds", "dop")]
    pil = _t(inp["pilots"])
    full = eng.forward(pil, *meta)
    assert torch.isfinite(torch.view_as_real(full)).all()
    for lo in (0, 48, 112):
        part = eng.forward(pil[lo:lo + 16], *[m[lo:lo + 16] for m in meta])
        assert torch.equal(torch.view_as_real(part), torch.view_as_real(full[lo:lo + 16]))
    again = eng.forward(pil, *meta)
    assert torch.equal(torch.view_as_real(again), torch.view_as_real(full))  # deterministic, no atomics
    orc = oracle_lib.Oracle(cfg, sd)
    idx = [0, 63, 127]
    ref = orc.forward(inp["pilots"][idx], inp["snr"][idx], inp["ds"][idx], inp["dop"][idx])
    got = full[idx].cpu().numpy()
    assert np.abs(got - ref).max() <= TOL_HIP_OUT * np.abs(ref).max()
    # metric on device == oracle metric
    from adafortitran_amd.hip_ops import mse_sum
    tgt = _t(inp["target"])
    dev_sum = mse_sum(full, tgt).item()
    host_sum = oracle_lib.mse_sum(full.cpu().numpy(), inp["target"])
    assert abs(dev_sum - host_sum) <= 1e-9 * host_sum


def _poison_allocator(value):
    """Leave the caching allocator's pool full of `value`: the next torch.empty (workspaces, outputs) gets that memory."""
    blocks = [torch.full((n,), value, device=DEV) for n in (1 << 26, 1 << 25, 1 << 24, 1 << 22, 1 << 20, 1 << 18) for _ in range(3)]
    del blocks


@pytest.mark.parametrize("batch", [3, 40, 64, 130, 170])
def test_conv_stream_column_ranges_reproduce_whole_planes(switches, batch):
    """Small batches split every plane of the default grid into 2 or 4 column ranges (k_conv_stream.hip, NSPLIT), and the planes
    beyond a whole number of one-plane-per-CU rounds (130 frames = 260 planes: 4; 170 frames: 84) run as a second launch of ranges:
    the ranges recompute what they need of their neighbours' columns and every output element goes through the same instruction
    sequence, so the forward's conv_enhanced and output carry the same BITS whatever the split."""
    hid = (7, 42, 560)
    sd = synth.make_state_dict(**DEFAULT_SPEC, adaptive_hidden=hid, seed=91, head_gain=2.0)
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(batch, seed=92)
    pil, meta = _t(inp["pilots"]), [_t(inp[k]) for k in ("snr", "ds", "dop")]
    outs = {}
    for ns in ("1", "2", "4"):
        switches.set("AFT_CONV_NSPLIT", ns)
        outs[ns] = (eng.forward(pil, *meta).clone(), eng.forward_region("conv_enhanced", batch))
    switches.unset("AFT_CONV_NSPLIT")
    auto = eng.forward(pil, *meta).clone()
    for ns in ("2", "4"):
        assert torch.equal(outs[ns][1], outs["1"][1]), f"conv_enhanced differs at NSPLIT={ns}"
        assert torch.equal(torch.view_as_real(outs[ns][0]), torch.view_as_real(outs["1"][0])), f"output differs at NSPLIT={ns}"
    assert torch.equal(torch.view_as_real(auto), torch.view_as_real(outs["1"][0]))
    assert torch.isfinite(torch.view_as_real(auto)).all()


@pytest.mark.parametrize("batch,reps", [(128, 600), (64, 300), (16, 300), (130, 200)])
def test_conv_stream_hand_over_soak(batch, reps):
    """The column-streaming conv kernel hands conv1 / conv3 columns between its waves through LDS flags (k_conv_stream.hip); a lost
    hand-over would be a one-in-many-launches event.  Hundreds of forwards of the benchmark batch -- and of batches that run two / four
    column ranges per plane and a remainder launch -- EVERY output compared on the device with the first one's bits (was
    tools/debug/soak_forward.py)."""
    hid = (7, 42, 560)
    sd = synth.make_state_dict(**DEFAULT_SPEC, adaptive_hidden=hid, seed=20251114)
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(batch, seed=3)
    pil, meta = _t(inp["pilots"]), [_t(inp[k]) for k in ("snr", "ds", "dop")]
    ref = eng.forward(pil, *meta).clone()
    out = torch.empty_like(ref)
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    for _ in range(reps):
        eng.forward(pil, *meta, out=out)
        bad += (torch.view_as_real(out) != torch.view_as_real(ref)).any().to(torch.int64)
    assert int(bad.item()) == 0


@pytest.mark.parametrize("value", [float("nan"), 1e30, -3e38, float("inf")])
def test_output_bits_do_not_depend_on_stale_workspace(value):
    """Workspace and pad regions nobody writes (q / k / vt rows 280..287 of every (plane, head), the tail of the out6
    rows, ...) hold whatever the allocator hands out.  None of it may reach the arithmetic of a stored value -- not even
    through a wave-wide branch: the output must be the same bits whatever the pool held.  (Round 2: a large stale value in
    a padded query lane switched the valid lanes of its wave onto attention's rescale path: 1e-7 differences between a
    B = 16 run and the same frames inside a B = 128 run, visible only when the training tests had run first.)"""
    from adafortitran_amd.hip_ops import engine_from_numpy
    cases = [(DEFAULT_SPEC, (7, 42, 560), 37),                                                     # 280 tokens: ragged key / query tiles
             (dict(ofdm=(30, 8), pilot=(6, 2), patch=(3, 2), num_layers=2, model_dim=128, num_head=4), (5, 9, 80), 5),   # 40 tokens
             (dict(ofdm=(66, 12), pilot=(11, 3), patch=(3, 3), num_layers=2, model_dim=128, num_head=4), None, 3),      # 88 tokens
             (dict(ofdm=(54, 14), pilot=(6, 2), patch=(3, 2), num_layers=2, model_dim=256, num_head=8), (4, 8, 252), 3),   # d = 256, 126 tokens
             (dict(ofdm=(54, 14), pilot=(6, 2), patch=(3, 2), num_layers=2, model_dim=64, num_head=2), None, 2),
             (dict(ofdm=(54, 14), pilot=(6, 2), patch=(3, 2), num_layers=2, model_dim=192, num_head=6), None, 2)]

    def run(spec, hid, B):
        sd = synth.make_state_dict(**spec, adaptive_hidden=hid, seed=7)
        cfg = _abi.make_config(**spec, adaptive_hidden=hid)
        eng = engine_from_numpy(cfg, sd, DEV)
        inp = synth.make_inputs(B, ofdm=spec["ofdm"], pilot=spec["pilot"], seed=8)
        meta = [_t(inp[k]) for k in ("snr", "ds", "dop")] if hid else []
        return eng.forward(_t(inp["pilots"]), *meta).clone()

    for spec, hid, B in cases:
        _poison_allocator(0.0)
        ref = run(spec, hid, B)
        _poison_allocator(value)
        out = run(spec, hid, B)
        assert torch.isfinite(torch.view_as_real(out)).all()
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(ref)), (spec["ofdm"], value)


@pytest.mark.parametrize("ofdm,pilot,patch,adaptive", [((30, 8), (6, 2), (3, 2), True), ((66, 12), (11, 3), (3, 3), False),
                                                        ((150, 8), (10, 2), (5, 2), True),
                                                        ((120, 14), (12, 2), (4, 2), True), ((120, 14), (12, 2), (2, 2), False),
                                                        ((54, 14), (6, 2), (3, 2), False),
                                                        ((48, 16), (8, 2), (3, 2), False), ((30, 50), (6, 5), (3, 2), True),
                                                        ((60, 18), (6, 3), (3, 2), False)])
def test_other_grid_geometries_match_oracle(oracle_lib, ofdm, pilot, patch, adaptive):
    """Grids whose row count is not a multiple of 4 / of the 30-row conv tiles, other patch shapes, a
    grid taller than the default (one band, five conv tiles): conv tiling, patch addressing, ragged
    attention tiles; token counts that are not a multiple of 8 or 4 (210, 420, 126).  The last three have bands of one or
    two conv row tiles and >= 16 symbols: FOUR column segments with three exact seams (exchange rows behind the arena for
    16 / 18 symbols, in the dead input plane for 50; segments of 4 / 5 columns for 18)."""
    tokens = (ofdm[0] // patch[0]) * (ofdm[1] // patch[1])
    spec = dict(ofdm=ofdm, pilot=pilot, patch=patch, num_layers=2, model_dim=128, num_head=4)
    hid = (5, 9, 2 * tokens) if adaptive else None
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, seed=99)
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(5, ofdm=ofdm, pilot=pilot, seed=31)
    meta = [(_t(inp[k]) if adaptive else None) for k in ("snr", "ds", "dop")]
    out = eng.forward(_t(inp["pilots"]), *meta).cpu().numpy()
    ref = oracle_lib.Oracle(cfg, sd).forward(inp["pilots"], *([inp["snr"], inp["ds"], inp["dop"]] if adaptive else [None] * 3))
    assert np.abs(out - ref).max() <= TOL_HIP_OUT * np.abs(ref).max()


@pytest.mark.parametrize("ofdm,pilot,patch,adaptive,batch", [((240, 28), (24, 4), (3, 2), True, 3), ((180, 20), (12, 4), (3, 2), False, 1),
                                                              ((96, 40), (8, 5), (3, 2), True, 2), ((100, 36), (10, 4), (2, 2), False, 5)])
def test_tall_planes_run_the_row_streaming_conv_kernel(oracle_lib, switches, ofdm, pilot, patch, adaptive, batch):
    """Planes that need several bands in the banded conv kernel (17 channel planes > 160 KB of LDS) run k_conv_rows.hip in the whole
    forward: all rows per workgroup, four-column rings, column ranges with recomputed halo columns (2 or 4 ranges at these batches;
    8 / 6 / 4 row tiles, the last tile of the 100-row grid partly outside the plane).  Against the oracle, and against the banded
    kernel on the same inputs (AFT_CONV_BANDED is read per launch): the two differ by conv4's summation order only."""
    tokens = (ofdm[0] // patch[0]) * (ofdm[1] // patch[1])
    spec = dict(ofdm=ofdm, pilot=pilot, patch=patch, num_layers=2, model_dim=128, num_head=4)
    hid = (5, 9, 2 * tokens) if adaptive else None
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, max_seq_len=max(512, tokens), seed=77)
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(batch, ofdm=ofdm, pilot=pilot, seed=33)
    meta = [(_t(inp[k]) if adaptive else None) for k in ("snr", "ds", "dop")]
    pil = _t(inp["pilots"])
    out = eng.forward(pil, *meta).clone()
    ref, dump = oracle_lib.Oracle(cfg, sd).forward(inp["pilots"], *([inp["snr"], inp["ds"], inp["dop"]] if adaptive else [None] * 3), dump=True)
    assert np.abs(out.cpu().numpy() - ref).max() <= TOL_HIP_OUT * np.abs(ref).max()
    # the head stage of the kernel the forward launched (conv_rows16_kernel), straight from the workspace
    assert max_rel(eng.forward_region("conv_enhanced", batch).cpu().numpy(), dump["conv_enhanced"]) <= TOL_HIP_OUT
    eng.workspace(batch).view(torch.float32).fill_(float("nan"))           # stale workspace: same bits
    assert torch.equal(torch.view_as_real(eng.forward(pil, *meta)), torch.view_as_real(out))
    switches.set("AFT_CONV_BANDED", "1")
    banded = eng.forward(pil, *meta).clone()
    switches.unset("AFT_CONV_BANDED")
    assert float((banded - out).abs().max()) <= 2e-6 * float(out.abs().max())


def test_row_streaming_conv_does_not_depend_on_the_column_split():
    """k_conv_rows.hip splits a plane into column ranges when there are fewer planes than CUs; every output element is computed by the
    same instruction sequence whatever the range (the halo columns are recomputed, not exchanged), so the first frames of a batch
    large enough for ONE range per plane (130 frames = 260 planes) carry the same bits as the same frames alone (two ranges)."""
    ofdm, pilot, patch = (180, 20), (12, 4), (3, 2)
    spec = dict(ofdm=ofdm, pilot=pilot, patch=patch, num_layers=1, model_dim=128, num_head=4)
    sd = synth.make_state_dict(**spec, adaptive_hidden=None, max_seq_len=600, seed=78)
    cfg = _abi.make_config(**spec, adaptive_hidden=None)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(130, ofdm=ofdm, pilot=pilot, seed=34)
    pil = _t(inp["pilots"])
    big = eng.forward(pil, None, None, None).clone()
    small = eng.forward(pil[:4].contiguous(), None, None, None).clone()
    assert torch.isfinite(torch.view_as_real(big)).all()
    assert torch.equal(torch.view_as_real(big[:4]), torch.view_as_real(small))


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("d,heads", [(64, 2), (192, 6),                    # head dim 32: two / six waves per chain workgroup
                                     (128, 8), (64, 4), (192, 12), (256, 16),   # head dim 16: two heads per 32-feature block
                                     (128, 2), (64, 1), (192, 3), (256, 4),     # head dim 64: a head spans two blocks
                                     (32, 1), (32, 2), (96, 3), (96, 6), (160, 5), (160, 10), (224, 7), (224, 14),   # round 5: every multiple of 32
                                     # late round 5: heads that start anywhere in a block -- head dims 8 / 24 / 40 / 48
                                     (128, 16), (32, 4), (256, 32), (96, 4), (192, 8), (160, 4), (96, 2), (192, 4)])
def test_other_model_dims_match_oracle(oracle_lib, adaptive, d, heads):
    """Every (model_dim, num_head) the kernels cover besides the default: nn.MultiheadAttention takes any num_head that divides
    model_dim (reference blocks/encoders.py:44-51).  Non-uniform softmax (attn_gain), 9 frames = ragged row tiles, run-to-run
    determinism, every encoder layer on the oracle's own layer input, the whole forward against the oracle."""
    spec = dict(ofdm=(120, 14), pilot=(12, 2), patch=(3, 2), num_layers=3, model_dim=d, num_head=heads)
    hid = (7, 42, 560) if adaptive else None
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, seed=64 + heads, attn_gain=0.25 if adaptive else 16.0, head_gain=2.0)
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(9, seed=65)
    meta = [(_t(inp[k]) if adaptive else None) for k in ("snr", "ds", "dop")]
    out = eng.forward(_t(inp["pilots"]), *meta)
    assert torch.equal(torch.view_as_real(eng.forward(_t(inp["pilots"]), *meta)), torch.view_as_real(out))
    orc = oracle_lib.Oracle(cfg, sd)
    ref, dump = orc.forward(inp["pilots"], *([inp["snr"], inp["ds"], inp["dop"]] if adaptive else [None] * 3), dump=True)
    assert np.abs(out.cpu().numpy() - ref).max() <= TOL_HIP_OUT * np.abs(ref).max()
    xin = dump["x0"]
    for layer in range(spec["num_layers"]):
        y = eng.stage_encoder_layer(layer, _t(xin)).cpu().numpy()
        assert max_rel(y, dump["layer_out"][layer]) <= TOL_HIP_OUT, layer
        xin = dump["layer_out"][layer]


@pytest.mark.parametrize("ofdm,pilot,patch,d,heads", [((12, 14), (4, 2), (3, 2), 64, 2),     # 28 tokens
                                                       ((12, 4), (4, 2), (3, 2), 128, 4),     # 8 tokens: four planes per row tile
                                                       ((6, 14), (2, 2), (3, 2), 128, 8),     # 14 tokens, head dim 16
                                                       ((24, 6), (4, 2), (3, 2), 64, 1),      # 24 tokens, head dim 64
                                                       ((30, 6), (6, 2), (3, 2), 192, 6),     # 30 tokens
                                                       ((3, 2), (1, 1), (3, 2), 64, 2)])      # ONE token per plane
@pytest.mark.parametrize("batch", [1, 7, 33])
def test_grids_with_fewer_than_32_tokens_match_oracle(oracle_lib, ofdm, pilot, patch, d, heads, batch):
    """Token counts below one MFMA tile (the reference accepts any grid divisible by the patch, fortitran.py:52-81): attention
    runs one masked key tile per (plane, head), a 32-row tile of the row-local chain holds several whole planes."""
    tokens = (ofdm[0] // patch[0]) * (ofdm[1] // patch[1])
    spec = dict(ofdm=ofdm, pilot=pilot, patch=patch, num_layers=2, model_dim=d, num_head=heads)
    hid = (7, 42, 2 * tokens)
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, max_seq_len=32, seed=500 + tokens, attn_gain=0.5, head_gain=2.0)
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(batch, ofdm=ofdm, pilot=pilot, seed=600 + batch)
    meta = [_t(inp[k]) for k in ("snr", "ds", "dop")]
    out = eng.forward(_t(inp["pilots"]), *meta)
    assert torch.equal(torch.view_as_real(eng.forward(_t(inp["pilots"]), *meta)), torch.view_as_real(out))
    ref = oracle_lib.Oracle(cfg, sd).forward(inp["pilots"], inp["snr"], inp["ds"], inp["dop"])
    assert np.abs(out.cpu().numpy() - ref).max() <= TOL_HIP_OUT * np.abs(ref).max()


def test_config5_persistent_tiles(oracle_lib):
    """BASELINE config 5 shapes (240x28 grid, 12 layers, d=256, 8 heads, 1120 tokens) at B=16:
    1120 row tiles over 256 resident workgroups, so every workgroup walks several tiles (the
    persistent loop of k_chain.hip / k_attn.hip) -- determinism, chunk independence, oracle sample."""
    g = Golden("C5_ada_large")
    cfg, sd = g.abi_config(), g.state_dict()
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    B = 16
    inp = synth.make_inputs(B, ofdm=(240, 28), pilot=(24, 4), seed=515)
    meta = [_t(inp[k]) for k in ("snr", "ds", "dop")]
    pil = _t(inp["pilots"])
    full = eng.forward(pil, *meta).clone()
    again = eng.forward(pil, *meta)
    assert torch.equal(torch.view_as_real(again), torch.view_as_real(full))
    part = eng.forward(pil[12:16], *[m[12:16] for m in meta])
    assert torch.equal(torch.view_as_real(part), torch.view_as_real(full[12:16]))
    idx = [0, 15]
    ref = oracle_lib.Oracle(cfg, sd).forward(inp["pilots"][idx], inp["snr"][idx], inp["ds"][idx], inp["dop"][idx])
    got = full[idx].cpu().numpy()
    assert np.abs(got - ref).max() <= TOL_HIP_OUT * np.abs(ref).max()


def test_config5_at_stated_size_per_gpu(oracle_lib):
    """BASELINE config 5 at its stated per-GPU size: 64 frames (512 over 8 GPUs) of the 240x28 grid
    = 143 360 token rows, 4480 row tiles, 9216 (plane, head) attention problems of 1120 keys.
    Size-independent properties (determinism, chunk independence bit for bit) + an oracle sample."""
    g = Golden("C5_ada_large")
    cfg, sd = g.abi_config(), g.state_dict()
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    B = 64
    inp = synth.make_inputs(B, ofdm=(240, 28), pilot=(24, 4), seed=516)
    meta = [_t(inp[k]) for k in ("snr", "ds", "dop")]
    pil = _t(inp["pilots"])
    full = eng.forward(pil, *meta).clone()
    again = eng.forward(pil, *meta)
    assert torch.equal(torch.view_as_real(again), torch.view_as_real(full))
    part = eng.forward(pil[40:43], *[m[40:43] for m in meta])
    assert torch.equal(torch.view_as_real(part), torch.view_as_real(full[40:43]))
    idx = [63]
    ref = oracle_lib.Oracle(cfg, sd).forward(inp["pilots"][idx], inp["snr"][idx], inp["ds"][idx], inp["dop"][idx])
    got = full[idx].cpu().numpy()
    assert np.abs(got - ref).max() <= TOL_HIP_OUT * np.abs(ref).max()


@pytest.mark.parametrize("name", ["D_forti", "A_ada"])
def test_module_surface_on_gpu(name):
    """The drop-in nn.Module: CPU inputs in, device output out, HIP path under eval+no_grad,
    autograd composite under train() -- both against the reference golden output."""
    from test_estimators_cpu import _configs, golden_meta
    g = Golden(name)
    sc, mc = _configs(g.spec, device="cuda")
    cls = A.AdaFortiTranEstimator if g.adaptive else A.FortiTranEstimator
    model = cls(sc, mc)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()})
    model.eval()
    pil, meta = torch.from_numpy(g["pilots"]), golden_meta(g)       # CPU tensors, as the DataLoader yields
    with torch.no_grad():
        out = model(pil, meta) if meta is not None else model(pil)
    assert out.device.type == "cuda" and out.dtype == torch.complex64
    assert model._engine is not None                                # the C-ABI path ran
    assert np.abs(out.cpu().numpy() - g["out"]).max() <= TOL_HIP_OUT * np.abs(g["out"]).max()
    with torch.enable_grad():                                        # autograd path (PyTorch-ROCm composite)
        out_g = model(pil, meta) if meta is not None else model(pil)
        assert out_g.requires_grad
    assert np.abs(out_g.detach().cpu().numpy() - g["out"]).max() <= 2 * TOL_HIP_OUT * np.abs(g["out"]).max()
    if g.adaptive:
        with pytest.raises(ValueError, match="meta_data is required"), torch.no_grad():
            model(pil)


def test_module_engine_cache_and_invalidation():
    """The module's per-call engine lookup is pointer/identity compares only: the same engine object
    serves consecutive forwards, in-place parameter updates are seen without a rebuild (the ABI reads
    the parameters' own storage), and a re-homed or replaced tensor rebuilds it."""
    from test_estimators_cpu import _configs
    g = Golden("D_forti")
    sc, mc = _configs(g.spec, device="cuda")
    model = A.FortiTranEstimator(sc, mc)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()})
    model.eval()
    pil = torch.from_numpy(g["pilots"])
    with torch.no_grad():
        out0 = model(pil).clone()
        eng = model._engine
        model(pil)
        assert model._engine is eng                                    # O(1) path: no rebuild
        w = model.final_refiner.conv_block[6].bias
        w.add_(0.25)                                                    # in-place update (what an optimizer does)
        out1 = model(pil)
        assert model._engine is eng
        assert np.allclose((out1 - out0).cpu().numpy(), 0.25 + 0.25j, atol=1e-6)
        w.data = w.data.clone() - 0.25                                 # re-homed storage -> new pointer
        out2 = model(pil)
        assert model._engine is not eng
        assert np.allclose((out2 - out0).cpu().numpy(), 0.0, atol=1e-6)
        eng2 = model._engine
        model.final_refiner.conv_block[6].bias = torch.nn.Parameter(w.data.clone() + 0.5)   # replaced object
        out3 = model(pil)
        assert model._engine is not eng2
        assert np.allclose((out3 - out0).cpu().numpy(), 0.5 + 0.5j, atol=1e-6)


def test_uncovered_configuration_is_refused_at_construction(switches):
    """One coverage predicate, asked at construction on the HIP device: a shape the reference accepts but
    the kernels do not cover raises a ValueError before any training, unless the caller opts
    into the PyTorch-ROCm composite."""
    # model_dim 100 (5 heads of 20): accepted by the reference's schema (> 0), not by the kernels (multiples of 8 up to 512; round 5's
    # example, model_dim 80, runs the general engine since round 6)
    sc = A.SystemConfig(ofdm=dict(num_scs=120, num_symbols=14), pilot=dict(num_scs=12, num_symbols=2))
    kw = dict(model_type="fortitran", patch_size=(3, 2), num_layers=2, model_dim=100, num_head=5)
    assert A.FortiTranEstimator(sc, A.ModelConfig(device="cpu", **kw)) is not None      # CPU: the reference's own path
    switches.unset("AFT_ALLOW_COMPOSITE")
    with pytest.raises(ValueError, match="not covered by the gfx950 kernels"):
        A.FortiTranEstimator(sc, A.ModelConfig(device="cuda", **kw))
    switches.set("AFT_ALLOW_COMPOSITE", "1")
    model = A.FortiTranEstimator(sc, A.ModelConfig(device="cuda", **kw)).eval()
    pil = torch.from_numpy(synth.make_inputs(2, seed=3)["pilots"])
    with torch.no_grad():
        out = model(pil)
    assert out.shape == (2, 120, 14) and model._engine is None          # composite ran, no C-ABI engine


@pytest.mark.parametrize("name", OTHER_SHAPE_SETS)
def test_module_surface_with_other_head_dims_and_small_grids(name):
    """`num_head: 8` at `model_dim: 128` (head dim 16), `num_head: 2` (head dim 64) and a 28-token grid through the MODULE, as the
    reference's YAML would configure them: eval() runs the HIP engine (golden parity, CPU inputs), train() differentiates through the
    library's training kernels (head dims 16 and 64 and the 28-token grid since round 5; training_backends() says what runs where)
    -- and the gradients agree with the CPU composite."""
    from test_estimators_cpu import _configs, golden_meta
    g = Golden(name)
    sc, mc = _configs(g.spec, device="cuda")
    cls = A.AdaFortiTranEstimator if g.adaptive else A.FortiTranEstimator
    model = cls(sc, mc)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()})
    model.eval()
    pil = torch.from_numpy(g["pilots"])
    meta = golden_meta(g) if g.adaptive else None
    with torch.no_grad():
        out = model(pil, meta) if g.adaptive else model(pil)
    assert model._engine is not None                                     # the C-ABI engine ran
    err = np.abs(out.cpu().numpy() - g["out"]).max()
    if err > TOL_HIP_OUT * np.abs(g["out"]).max():                       # say where it went wrong: intermediates, a second call, device inputs
        diag = {"err": float(err), "engine": model.hip_engine_name()}
        for reg in ("conv_enhanced", "enc_out"):
            r = model._engine.forward_region(reg, pil.shape[0]).cpu().numpy()
            diag[reg] = float(np.abs(r).max())
            if reg in g:
                diag[reg + "_err"] = float(np.abs(r[..., :g[reg].shape[-1]].reshape(-1) - g[reg].reshape(-1)).max())
        with torch.no_grad():
            diag["second_call_err"] = float(np.abs((model(pil, meta) if g.adaptive else model(pil)).cpu().numpy() - g["out"]).max())
            dev_meta = meta
            diag["device_input_err"] = float(np.abs((model(pil.cuda(), dev_meta) if g.adaptive else model(pil.cuda())).cpu().numpy() - g["out"]).max())
        raise AssertionError(diag)
    assert all(v is None for v in model.training_backends().values())    # head dims 16 / 64 and the 28-token grid train on the library's kernels
    # one training step on the GPU against the same step on the CPU composite
    sc_c, mc_c = _configs(dict(g.spec, dropout=0.0), device="cpu")
    sc_g, mc_g = _configs(dict(g.spec, dropout=0.0), device="cuda")
    grads = []
    for s_, m_, dev in ((sc_c, mc_c, "cpu"), (sc_g, mc_g, "cuda")):
        mdl = cls(s_, m_)
        mdl.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()})
        mdl.train()
        est = mdl(pil, meta) if g.adaptive else mdl(pil)
        tgt = torch.from_numpy(g["target"]).to(dev)
        torch.view_as_real(est - tgt).pow(2).mean().backward()
        grads.append({n: p.grad.detach().cpu().numpy() for n, p in mdl.named_parameters()})
    off = [n for n, ref in grads[0].items() if np.abs(grads[1][n] - ref).max() > 2e-3 * np.abs(ref).max() + 1e-12]
    if off:
        # A pre-activation of the first conv stack that is ~0 takes different sides of its ReLU in two fp32 summation orders; the
        # tensors upstream of it (pilot_upsampler, conv_block.0: |g|max ~ 1e-6) then differ by ~1e-2 although both are valid
        # (H24 set: the CPU composite and PyTorch-ROCm fp32 agree with each other, the library's kernels with float64 --
        # tools/debug/hd24_surface_repro.py).  Arbiter: the same module in float64 -- the library's gradients must sit on ITS side.
        mdl = cls(sc_g, mc_g)
        mdl.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()})
        mdl.train().double()
        m64 = tuple(x.double() if torch.is_tensor(x) and x.is_floating_point() else x for x in meta) if g.adaptive else None
        est = mdl(pil.to(torch.complex128), m64) if g.adaptive else mdl(pil.to(torch.complex128))
        torch.view_as_real(est - torch.from_numpy(g["target"]).cuda().to(torch.complex128)).pow(2).mean().backward()
        g64 = {n: p.grad.detach().cpu().numpy() for n, p in mdl.named_parameters()}
        for n in off:
            assert n.startswith(("pilot_upsampler", "initial_enhancer")), n
            assert np.abs(grads[1][n] - g64[n]).max() <= 1e-4 * np.abs(g64[n]).max(), n


def test_stream_and_graph_semantics():
    """The ABI is asynchronous on the caller's stream and allocation-free: it runs on a side
    stream and inside a captured hipGraph (test_graph_capture_as_first_call covers the cold start)."""
    g = Golden("A_ada")
    eng = _engine(g)
    pil, meta = _t(g["pilots"]), _meta(g)
    ref = eng.forward(pil, *meta).clone()                      # warm call on the default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out_side = eng.forward(pil, *meta).clone()
    side.synchronize()
    assert torch.equal(torch.view_as_real(out_side), torch.view_as_real(ref))
    static_out = torch.empty_like(ref)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.forward(pil, *meta, out=static_out)
    static_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(static_out), torch.view_as_real(ref))
    pil2 = _t(np.ascontiguousarray(g["pilots"][::-1]))         # new inputs through the same buffers
    pil.copy_(pil2)
    graph.replay()
    torch.cuda.synchronize()
    want = eng.forward(pil2, *meta)
    assert torch.equal(torch.view_as_real(static_out), torch.view_as_real(want))


@pytest.mark.parametrize("batch", [2, 5, 33, 64, 130])
def test_lanes_reproduce_the_unsplit_forward(batch, switches):
    """include/adafortitran_amd.h "Lanes": a forward of fewer than ~2.5 rounds of the persistent grids runs as two complete forwards
    over contiguous shares of the batch, share 1 on a library-owned side stream forked from / joined into the caller's.  Same bits
    as the unsplit forward (AFT_LANES=1) for every split the switch allows, the intermediates the forward leaves behind included;
    back-to-back calls on one stream and calls on two caller streams at once stay correct (each caller stream has its own side
    stream and events)."""
    g = Golden("A_ada")
    eng = _engine(g)
    inp = synth.make_inputs(batch, seed=77)
    pil, meta = _t(inp["pilots"]), [_t(inp[k]) for k in ("snr", "ds", "dop")]
    switches.set("AFT_LANES", "1")
    ref = eng.forward(pil, *meta).clone()
    regions = {n: eng.forward_region(n, batch) for n in ("conv_enhanced", "tokens6", "enc_out")}
    for want in (None, "2", "3", "4"):
        if want is None:
            switches.unset("AFT_LANES")
        else:
            switches.set("AFT_LANES", want)
        _poison_allocator(1e30)
        for _ in range(3):                                        # back to back: the next call's fork waits for this call's join
            out = eng.forward(pil, *meta)
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(ref)), want
        for n, r in regions.items():
            assert torch.equal(eng.forward_region(n, batch), r), (want, n)
    # inside a hipGraph capture the side stream joins the capture (fork / join are event nodes of the graph)
    switches.set("AFT_LANES", "2")
    static_out = torch.empty_like(ref)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.forward(pil, *meta, out=static_out)
    for _ in range(2):
        static_out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(static_out), torch.view_as_real(ref))
    switches.unset("AFT_LANES")
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = []
    for rep in range(4):
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                outs.append(eng.forward(pil, *meta))
    torch.cuda.synchronize()
    assert all(torch.equal(torch.view_as_real(o), torch.view_as_real(ref)) for o in outs)


def test_lanes_under_host_threads_and_many_caller_streams(switches):
    """The library keeps one side stream + events per (device, caller stream), behind a mutex, for at most 16 caller streams: four
    host threads forwarding at once on their own streams, then 24 caller streams in turn (the later ones run unsplit) -- the bits of
    the unsplit forward every time."""
    import threading
    g = Golden("A_ada")
    inp = synth.make_inputs(48, seed=78)
    pil, meta = _t(inp["pilots"]), [_t(inp[k]) for k in ("snr", "ds", "dop")]
    switches.set("AFT_LANES", "1")
    ref = _engine(g).forward(pil, *meta).clone()
    switches.unset("AFT_LANES")
    torch.cuda.synchronize()
    bad = []

    def worker(k):
        eng, st = _engine(g), torch.cuda.Stream()
        with torch.cuda.stream(st):
            for it in range(40):
                out = eng.forward(pil, *meta)
                if it % 10 == 9:
                    st.synchronize()
                    if not torch.equal(torch.view_as_real(out), torch.view_as_real(ref)):
                        bad.append((k, it))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, bad
    eng = _engine(g)
    for k in range(24):
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            out = eng.forward(pil, *meta)
        st.synchronize()
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(ref)), k


def test_graph_capture_as_first_call():
    """No call-describing state in the library: in a fresh process the FIRST call may already be a
    hipGraph capture (kernel attributes / CU count are set per device on demand, nothing needs a warm
    call).  Runs tests/graph_first_call.py as a child process."""
    import subprocess
    import sys
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "graph_first_call.py")
    res = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "graph-first-call" in res.stdout


def test_abi_error_codes():
    g = Golden("A_ada")
    eng = _engine(g)
    with pytest.raises(ValueError, match="meta_data is required"):
        eng.forward(_t(g["pilots"]))
    with pytest.raises(ValueError, match="Expected pilot shape"):
        eng.forward(_t(np.zeros((2, 5, 5), np.complex64)), *_meta(g))
    from adafortitran_amd import _lib
    import ctypes as C
    lib = _lib.load()
    ws = eng.workspace(8)
    pil = torch.view_as_real(_t(g["pilots"]))
    m = _meta(g)
    rc = lib.aft_forward_f32(C.byref(eng.cfg), C.byref(eng.weights), pil.data_ptr(), m[0].data_ptr(), m[1].data_ptr(),
                             m[2].data_ptr(), pil.data_ptr(), ws.data_ptr(), 1024, 8, None)
    assert rc == _abi.AFT_ERR_ARG and b"workspace too small" in lib.aft_last_error()


def test_linear_and_mse_kernels(oracle_lib):
    g = Golden("L_linear")
    seed = g.meta["seed"]
    w = synth.uniform_pm(seed, "linear.weight", (1680, 24), 1 / np.sqrt(24))
    b = synth.uniform_pm(seed, "linear.bias", (1680,), 1 / np.sqrt(24))
    from adafortitran_amd.hip_ops import linear_forward, mse_sum
    out = linear_forward(_t(w), _t(b), _t(g["pilots"]), (120, 14)).cpu().numpy()
    assert np.abs(out - g["out"]).max() <= 1e-5
    for n in (1, 7, 1680 * 5 + 3):
        rng = np.random.default_rng(n)
        e = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        r = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        got = mse_sum(_t(e), _t(r)).item()
        want = oracle_lib.mse_sum(e, r)
        assert abs(got - want) <= 1e-6 * want   # device subtracts in fp32 (as torch does), oracle in fp64


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("d,heads", [(512, 8), (512, 4), (384, 4), (448, 8),      # head dims 64 / 128 / 96 / 56 above model_dim 256
                                     (288, 9), (320, 5), (512, 16),                 # head dims 32 / 64 / 32: the one- and two-block attention kernels
                                     (224, 4), (128, 1), (96, 1), (256, 2),         # inside the packed engine's model dims: heads of 56 / 128 / 96 / 128
                                     (80, 5), (200, 8), (120, 8), (96, 8), (40, 2), (8, 1), (72, 2)])   # model dims off the multiples of 32; heads of 16 / 25 / 15 / 12 / 20 / 8 / 36
def test_general_engine_matches_oracle(oracle_lib, adaptive, d, heads):
    """Round 6: everything nn.TransformerEncoderLayer builds up to model_dim 512 / head dim 128 that the packed engine
    does not take runs the GENERAL engine (row-major GEMM / attention / LayerNorm launches, include/adafortitran_amd.h aft_engine_of).
    Non-uniform softmax, 9 frames (ragged tiles), run-to-run determinism, every encoder layer on the oracle's own layer input, the
    whole forward against the oracle, batch independence of the bits."""
    import ctypes
    from adafortitran_amd import _lib
    spec = dict(ofdm=(120, 14), pilot=(12, 2), patch=(3, 2), num_layers=2, model_dim=d, num_head=heads)
    hid = (7, 42, 560) if adaptive else None
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, seed=640 + heads, attn_gain=0.25 if adaptive else 16.0, head_gain=2.0)
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    assert _lib.load().aft_engine_of(ctypes.byref(cfg)) == _abi.AFT_ENGINE_GENERAL
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(9, seed=65)
    meta = [(_t(inp[k]) if adaptive else None) for k in ("snr", "ds", "dop")]
    out = eng.forward(_t(inp["pilots"]), *meta)
    assert torch.equal(torch.view_as_real(eng.forward(_t(inp["pilots"]), *meta)), torch.view_as_real(out))
    few = eng.forward(_t(inp["pilots"][:4]), *[(m[:4] if m is not None else None) for m in meta])
    assert torch.equal(torch.view_as_real(few), torch.view_as_real(out[:4]))            # a frame's bits do not depend on its batch
    orc = oracle_lib.Oracle(cfg, sd)
    ref, dump = orc.forward(inp["pilots"], *([inp["snr"], inp["ds"], inp["dop"]] if adaptive else [None] * 3), dump=True)
    assert np.abs(out.cpu().numpy() - ref).max() <= TOL_HIP_OUT * np.abs(ref).max()
    xin = dump["x0"]
    for layer in range(spec["num_layers"]):
        y = eng.stage_encoder_layer(layer, _t(xin)).cpu().numpy()
        assert max_rel(y, dump["layer_out"][layer]) <= TOL_HIP_OUT, layer
        xin = dump["layer_out"][layer]


@pytest.mark.parametrize("ofdm,pilot,patch,d,heads,adaptive", [((120, 14), (12, 2), (3, 2), 512, 8, True), ((96, 14), (12, 2), (12, 2), 200, 8, True),
                                                              ((64, 16), (8, 2), (8, 4), 256, 2, False), ((12, 14), (4, 2), (3, 2), 8, 1, True)])
def test_general_engine_embedding_kernels_give_the_same_bits(ofdm, pilot, patch, d, heads, adaptive, switches):
    """Late round 6: the general engine's embedding runs the training path's forward kernel (k_ends_train.hip: W1^T staged once per
    persistent workgroup; 326 -> ~30 us at d = 512) instead of embed_any_kernel (switch AFT_EMBED_ANY_OLD).  Both add bias + position
    first and then the input features in ascending order: the same bits, through the stage entry point and through a whole forward."""
    tokens = (ofdm[0] // patch[0]) * (ofdm[1] // patch[1])
    spec = dict(ofdm=ofdm, pilot=pilot, patch=patch, num_layers=1, model_dim=d, num_head=heads)
    hid = (5, 11, 2 * tokens) if adaptive else None
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, seed=31, head_gain=2.0, max_seq_len=max(64, tokens))
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    inp = synth.make_inputs(5, ofdm=ofdm, pilot=pilot, seed=32)
    meta = [(_t(inp[k]) if adaptive else None) for k in ("snr", "ds", "dop")]

    def run():
        eng = engine_from_numpy(cfg, sd, DEV)
        out = eng.forward(_t(inp["pilots"]), *meta).clone()
        x0 = eng.region("x").clone() if hasattr(eng, "region") else None
        return out, x0

    new, x_new = run()
    switches.set("AFT_EMBED_ANY_OLD", "1")
    old, x_old = run()
    assert torch.isfinite(torch.view_as_real(new)).all()
    assert torch.equal(torch.view_as_real(new), torch.view_as_real(old))
    if x_new is not None:
        assert torch.equal(x_new, x_old)


@pytest.mark.parametrize("ofdm,pilot,patch,d,heads,layers", [((96, 14), (12, 2), (12, 2), 128, 4, 2),     # 24-element patch, 56 tokens
                                                            ((64, 16), (8, 2), (8, 4), 64, 2, 1),         # 32-element patch, 32 tokens
                                                            ((60, 20), (6, 4), (5, 5), 512, 8, 1),        # 25 elements at model_dim 512
                                                            ((12, 14), (4, 2), (3, 2), 32, 1, 70),        # 70 layers, packed engine (three windows)
                                                            ((30, 8), (6, 2), (3, 2), 40, 5, 35)])        # 35 layers, general engine
def test_large_patches_and_any_layer_count_match_oracle(oracle_lib, ofdm, pilot, patch, d, heads, layers):
    """Patches of up to 32 elements (the packed engine's fused embedding takes 16) and any number of layers (ABI 7: aft_weights.layers is
    a host array; the kernels that take the table by value are launched per window of 32 layers)."""
    tokens = (ofdm[0] // patch[0]) * (ofdm[1] // patch[1])
    spec = dict(ofdm=ofdm, pilot=pilot, patch=patch, num_layers=layers, model_dim=d, num_head=heads)
    for adaptive in (False, True):
        hid = (5, 11, 2 * tokens) if adaptive else None
        sd = synth.make_state_dict(**spec, adaptive_hidden=hid, seed=77, head_gain=2.0, max_seq_len=max(64, tokens))
        cfg = _abi.make_config(**spec, adaptive_hidden=hid)
        from adafortitran_amd.hip_ops import engine_from_numpy
        eng = engine_from_numpy(cfg, sd, DEV)
        inp = synth.make_inputs(5, ofdm=ofdm, pilot=pilot, seed=78)
        meta = [(_t(inp[k]) if adaptive else None) for k in ("snr", "ds", "dop")]
        out = eng.forward(_t(inp["pilots"]), *meta).cpu().numpy()
        ref = oracle_lib.Oracle(cfg, sd).forward(inp["pilots"], *([inp["snr"], inp["ds"], inp["dop"]] if adaptive else [None] * 3))
        assert np.isfinite(out).all() and np.abs(out - ref).max() <= TOL_HIP_OUT * np.abs(ref).max(), adaptive


def test_general_engine_through_the_module_surface():
    """A model the packed engine does not take, built through the reference's module surface on the HIP device: eval() forwards run
    the general engine (one aft_forward_f32 call), match the same module's CPU composite -- what the reference itself computes -- and
    the state_dict moves both ways unchanged."""
    sc = A.SystemConfig(ofdm=dict(num_scs=120, num_symbols=14), pilot=dict(num_scs=12, num_symbols=2))
    kw = dict(model_type="adafortitran", patch_size=(3, 2), num_layers=2, model_dim=320, num_head=5, channel_adaptivity_hidden_sizes=[7, 42, 560],
              adaptive_token_length=6)
    torch.manual_seed(3)
    cpu = A.AdaFortiTranEstimator(sc, A.ModelConfig(device="cpu", **kw)).eval()
    gpu = A.AdaFortiTranEstimator(sc, A.ModelConfig(device="cuda", **kw)).eval()
    gpu.load_state_dict(cpu.state_dict())
    assert gpu.hip_engine_name() == "general" and all(v is None for v in gpu.training_backends().values())
    inp = synth.make_inputs(6, seed=4)
    pil, meta = torch.from_numpy(inp["pilots"]), synth.meta_tuple(inp)
    with torch.no_grad():
        want, got = cpu(pil, meta), gpu(pil, meta)
    assert gpu._engine is not None and got.device.type == "cuda"
    assert (got.cpu() - want).abs().max() <= TOL_HIP_OUT * want.abs().max()


def _random_specs_general(n, seed):
    """Random configurations from what round 6 added: model_dim any multiple of 8 up to 512, any head count that divides it with heads
    of at most 128 features, patches of up to 32 elements, 1-3 layers -- keeping only draws the packed engine does NOT take."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p0, p1 = int(rng.integers(1, 9)), int(rng.integers(1, 5))
        if p0 * p1 > 32:
            continue
        gs, gt = int(rng.integers(2, 24)), int(rng.integers(1, 8))
        if gs * gt > 300 or gs * p0 > 160 or gt * p1 > 28:
            continue
        d = 8 * int(rng.integers(1, 65))
        divs = [h for h in range(1, d + 1) if d % h == 0 and d // h <= 128]
        heads = int(rng.choice(divs))
        hd = d // heads
        packed = d % 32 == 0 and d <= 256 and hd % 8 == 0 and hd <= 64 and hd != 56 and p0 * p1 <= 16
        if packed:
            continue
        ps, pt = int(rng.integers(2, 13)), int(rng.integers(1, 4))
        out.append(dict(ofdm=(gs * p0, gt * p1), pilot=(ps, pt), patch=(p0, p1), num_layers=int(rng.integers(1, 4)),
                        model_dim=d, num_head=heads, activation=str(rng.choice(["gelu", "relu"])),
                        pos=str(rng.choice(["learnable", "sinusoidal"])), adaptive=bool(rng.integers(0, 2)),
                        batch=int(rng.integers(1, 6))))
    return out


def _random_specs(n, seed, head_dims=(16, 32, 64)):
    """Random valid configurations: any grid the patch divides (token counts from 1 to 512, below one MFMA tile included), patches of
    <= 16 elements, model_dim any multiple of 32 up to 256 with head dim 16 / 32 / 64 (64 where it divides), 1-3 layers, both activations /
    positional encodings."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p0, p1 = int(rng.integers(1, 6)), int(rng.integers(1, 5))
        if p0 * p1 > 16:
            continue
        small = rng.integers(0, 4) == 0                                   # a quarter of the draws: fewer than 32 tokens
        gs, gt = (int(rng.integers(1, 8)), int(rng.integers(1, 5))) if small else (int(rng.integers(4, 30)), int(rng.integers(2, 9)))
        if (not small and gs * gt < 32) or (small and gs * gt >= 32) or gs * gt > 512 or gs * p0 > 160 or gt * p1 > 28:
            continue
        d = int(rng.choice([32, 64, 96, 128, 160, 192, 224, 256]))
        fits = [x for x in head_dims if d % x == 0]
        if not fits:
            continue
        hd = int(rng.choice(fits))
        ps, pt = int(rng.integers(2, 13)), int(rng.integers(1, 4))
        out.append(dict(ofdm=(gs * p0, gt * p1), pilot=(ps, pt), patch=(p0, p1), num_layers=int(rng.integers(1, 4)),
                        model_dim=d, num_head=d // hd, activation=str(rng.choice(["gelu", "relu"])),
                        pos=str(rng.choice(["learnable", "sinusoidal"])), adaptive=bool(rng.integers(0, 2)),
                        batch=int(rng.integers(1, 6))))
    return out


@pytest.mark.parametrize("spec", _random_specs(40, 2027) + _random_specs(20, 2031, head_dims=(8, 24, 40, 48)) + _random_specs_general(30, 2039), ids=lambda s: f"{s['ofdm'][0]}x{s['ofdm'][1]}p{s['patch'][0]}x{s['patch'][1]}d{s['model_dim']}h{s['num_head']}{'a' if s['adaptive'] else 'f'}")
def test_random_configurations_match_oracle(oracle_lib, spec):
    tokens = (spec["ofdm"][0] // spec["patch"][0]) * (spec["ofdm"][1] // spec["patch"][1])
    base = dict(ofdm=spec["ofdm"], pilot=spec["pilot"], patch=spec["patch"], num_layers=spec["num_layers"],
                model_dim=spec["model_dim"], num_head=spec["num_head"])
    hid = (5, 11, 2 * tokens) if spec["adaptive"] else None
    sd = synth.make_state_dict(**base, adaptive_hidden=hid, pos_encoding_type=spec["pos"], max_seq_len=512, seed=7,
                               head_gain=2.0)
    cfg = _abi.make_config(**base, activation=spec["activation"], adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(spec["batch"], ofdm=spec["ofdm"], pilot=spec["pilot"], seed=8)
    meta = [(_t(inp[k]) if spec["adaptive"] else None) for k in ("snr", "ds", "dop")]
    out = eng.forward(_t(inp["pilots"]), *meta).cpu().numpy()
    ref = oracle_lib.Oracle(cfg, sd).forward(inp["pilots"], *([inp["snr"], inp["ds"], inp["dop"]] if spec["adaptive"] else [None] * 3))
    assert np.isfinite(out).all()
    assert np.abs(out - ref).max() <= TOL_HIP_OUT * np.abs(ref).max()
    # and the same bits from a fresh engine whose workspace comes out of a 1e30-poisoned pool
    del eng
    _poison_allocator(1e30)
    again = engine_from_numpy(cfg, sd, DEV).forward(_t(inp["pilots"]), *meta).cpu().numpy()
    assert np.array_equal(again, out)


# ---- aft_config.encoder_path: every value gives the same bits ----
def _with_path(eng, path):
    eng.cfg.encoder_path = {"auto": _abi.AFT_ENCODER_AUTO, "launches": _abi.AFT_ENCODER_LAUNCHES,
                            "plane": _abi.AFT_ENCODER_PLANE}[path]
    return eng


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("batch", [1, 37])
def test_encoder_path_plane_launches_and_auto_give_identical_bits(adaptive, batch):
    """AFT_ENCODER_PLANE (retired: it runs the launches), AFT_ENCODER_LAUNCHES and AFT_ENCODER_AUTO (which may run the fused layer
    sequence) must give IDENTICAL bits, and the library never reports the fused sequence for PLANE."""
    import ctypes
    spec = dict(DEFAULT_SPEC, num_layers=2)
    hid = (7, 42, 560) if adaptive else None
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, seed=4242, attn_gain=0.25 if adaptive else 32.0,
                               head_gain=2.0)
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    from adafortitran_amd import _lib
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(batch, seed=99 + batch)
    meta = [(_t(inp[k]) if adaptive else None) for k in ("snr", "ds", "dop")]
    pil = _t(inp["pilots"])
    a = _with_path(eng, "launches").forward(pil, *meta).clone()
    b = _with_path(eng, "plane").forward(pil, *meta).clone()
    assert _lib.load().aft_layer_fused_of(ctypes.byref(eng.cfg), batch) == 0
    assert torch.isfinite(torch.view_as_real(a)).all()
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    c = _with_path(eng, "auto").forward(pil, *meta)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(c))


# ---- robustness of the drop-in surface (round 3) ----
def test_batches_above_the_offset_limit_run_in_chunks():
    """The reference accepts any batch (fortitran.py:145-182); the ABI's limit (aft_max_batch: 32-bit offsets into the
    largest workspace region) is handled by chunking in HipEngine.forward, not surfaced as an error."""
    g = Golden("A_ada")
    eng = _engine(g)
    pil, meta = _t(g["pilots"]), _meta(g)
    ref = eng.forward(pil, *meta).clone()
    eng.max_batch = 3                                            # 8 frames -> chunks of 3, 3, 2
    out = eng.forward(pil, *meta)
    assert torch.equal(torch.view_as_real(out), torch.view_as_real(ref))
    out2 = eng.forward(pil, *meta, cache_packed=True)
    assert torch.equal(torch.view_as_real(out2), torch.view_as_real(ref))
    # ... and with the inputs in PINNED HOST memory, read by the kernels directly (the module surface's path): chunk offsets apply
    # to host pointers just the same
    pil_h = torch.from_numpy(np.ascontiguousarray(g["pilots"])).pin_memory()
    meta_h = [torch.from_numpy(np.ascontiguousarray(g[k]).reshape(-1)).pin_memory() for k in ("snr", "ds", "dop")]
    out3 = eng.forward(pil_h, *meta_h, pinned_inputs=True)
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(out3), torch.view_as_real(ref))
    with pytest.raises(ValueError, match="pinned"):
        eng.forward(pil_h, *meta_h)                              # CPU tensors without the promise that they are pinned


def test_general_engine_batches_above_the_offset_limit_run_in_chunks(oracle_lib):
    """The same for the general engine, with its real limit: at model_dim 512 its largest tensor is q | k | v (rows x 1536 floats), so
    aft_max_batch is 624 frames on the default grid; 650 frames run as 624 + 26, a frame's bits do not depend on the chunk it lands in
    (prepacked calls are accepted and ignore the token image), and an oracle sample pins the values."""
    spec = dict(ofdm=(120, 14), pilot=(12, 2), patch=(3, 2), num_layers=1, model_dim=512, num_head=8)
    sd = synth.make_state_dict(**spec, adaptive_hidden=None, seed=21, head_gain=2.0)
    cfg = _abi.make_config(**spec)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    assert eng.max_batch == (2 ** 31 - 1) // (2 * 280 * 3 * 512 * 4) == 624
    inp = synth.make_inputs(650, seed=22)
    pil = _t(inp["pilots"])
    out = eng.forward(pil)
    a, b = eng.forward(pil[:300]), eng.forward(pil[300:])
    assert torch.equal(torch.view_as_real(out[:300]), torch.view_as_real(a)) and torch.equal(torch.view_as_real(out[300:]), torch.view_as_real(b))
    assert torch.equal(torch.view_as_real(eng.forward(pil, cache_packed=True)), torch.view_as_real(out))
    ref = oracle_lib.Oracle(cfg, sd).forward(inp["pilots"][620:628], None, None, None)
    assert np.abs(out[620:628].cpu().numpy() - ref).max() <= TOL_HIP_OUT * np.abs(ref).max()
    del eng, out, a, b
    torch.cuda.empty_cache()


def test_largest_accepted_batch_has_no_offset_overflow():
    """B = aft_max_batch exactly (7281 frames for the default model: q / k / v^T blocks just under 2 GiB, 11 GB of
    workspace): frames at both ends of the batch must equal the same frames run as a small batch, bit for bit; one
    frame more is refused by the raw ABI (and chunked by the engine)."""
    import ctypes as C
    from adafortitran_amd import _lib
    hid = (7, 42, 560)
    sd = synth.make_state_dict(**DEFAULT_SPEC, adaptive_hidden=hid, seed=11)
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    B = eng.max_batch
    assert B == (2 ** 31 - 1) // (2 * 288 * 128 * 4)
    small = synth.make_inputs(64, seed=3)
    reps = (B + 63) // 64
    pil = _t(small["pilots"]).repeat(reps, 1, 1)[:B].contiguous()
    meta = [_t(small[k]).reshape(-1).repeat(reps)[:B].contiguous() for k in ("snr", "ds", "dop")]
    ref = eng.forward(pil[:64], *[m[:64] for m in meta]).clone()
    out = eng.forward(pil, *meta)
    assert torch.equal(torch.view_as_real(out[:64]), torch.view_as_real(ref))
    lo = (B - 64) // 64 * 64                                      # the last complete repetition of the 64 frames
    assert torch.equal(torch.view_as_real(out[lo:lo + 64]), torch.view_as_real(ref))
    tail = B - (B // 64) * 64
    if tail:
        assert torch.equal(torch.view_as_real(out[B - tail:]), torch.view_as_real(ref[:tail]))
    lib = _lib.load()
    ws = eng.workspace(B)
    rc = lib.aft_forward_f32(C.byref(eng.cfg), C.byref(eng.weights), torch.view_as_real(pil).data_ptr(), meta[0].data_ptr(),
                             meta[1].data_ptr(), meta[2].data_ptr(), torch.view_as_real(out).data_ptr(), ws.data_ptr(),
                             ws.numel(), B + 1, None)
    assert rc == _abi.AFT_ERR_ARG and b"aft_max_batch" in lib.aft_last_error()
    del out, pil, ws
    eng._ws.clear()
    torch.cuda.empty_cache()


def test_module_surface_from_alternating_streams():
    """CPU inputs through the module on two streams in turn: the kernels read each call's pinned ring slot directly (no
    H2D copy is enqueued), the slot is guarded by an event recorded behind the forward on ITS stream, and every stream
    has its own scratch buffer -- so forwards in flight on different streams do not disturb each other and the results
    equal the single-stream ones."""
    from test_estimators_cpu import _configs, golden_meta
    g = Golden("A_ada")
    sc, mc = _configs(g.spec, device="cuda")
    model = A.AdaFortiTranEstimator(sc, mc)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()})
    model.eval()
    pil, meta = torch.from_numpy(g["pilots"]), golden_meta(g)
    rev = torch.from_numpy(np.ascontiguousarray(g["pilots"][::-1]))
    with torch.no_grad():
        want_a, want_b = model(pil, meta).clone(), model(rev, meta).clone()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        got = []
        for i in range(24):                                         # more calls than ring slots, streams alternate
            with torch.cuda.stream(streams[i & 1]):
                got.append((i & 1, model(pil if i & 1 == 0 else rev, meta)))
        torch.cuda.synchronize()
    eng = model._engine
    assert len({eng._ws[int(st.cuda_stream)].data_ptr() for st in streams}) == 2    # one scratch buffer per stream
    for which, out in got:
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(want_a if which == 0 else want_b))


def test_concurrent_streams_do_not_share_scratch():
    """Two engines' worth of work on ONE engine: B = 64 forwards of different frames issued back to back on two streams
    (nothing orders them, the persistent grids of one leave CUs for the other) must each equal the serial result."""
    hid = (7, 42, 560)
    sd = synth.make_state_dict(**DEFAULT_SPEC, adaptive_hidden=hid, seed=5)
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(128, seed=6)
    halves = []
    for lo in (0, 64):
        halves.append((_t(inp["pilots"][lo:lo + 64]), [_t(inp[k][lo:lo + 64]) for k in ("snr", "ds", "dop")]))
    want = [eng.forward(p, *m).clone() for p, m in halves]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for _ in range(5):
        outs = []
        for st, (p, m) in zip(streams, halves):
            with torch.cuda.stream(st):
                outs.append(eng.forward(p, *m))
        torch.cuda.synchronize()
        for o, w in zip(outs, want):
            assert torch.equal(torch.view_as_real(o), torch.view_as_real(w))


def test_module_forward_never_runs_stale_weights():
    """The module's inference path is stateless (aft_forward_f32 re-lays the encoder weights inside every call, in the
    adapter's launch): an in-place torch update, a raw ``.data`` write in eval() (EMA swap, dist.broadcast(p.data), an
    optimizer that writes through device pointers) and a train()/eval() bracket are all seen by the next forward."""
    from test_estimators_cpu import _configs
    g = Golden("D_forti")
    sc, mc = _configs(g.spec, device="cuda")
    model = A.FortiTranEstimator(sc, mc)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()})
    model.eval()
    pil = torch.from_numpy(g["pilots"])
    w = model.transformer_encoder.transformer.layers[2].linear1.weight
    with torch.no_grad():
        out0 = model(pil).clone()
        eng = model._engine
        w.mul_(1.5)                                                  # torch op: version counter moves
        out1 = model(pil).clone()
        assert model._engine is eng and not torch.equal(torch.view_as_real(out1), torch.view_as_real(out0))
        v0 = w._version
        w.data.copy_(w.data / 1.5)                                   # raw write in eval(): the version counter does NOT move
        assert w._version == v0
        out2 = model(pil).clone()
        assert np.abs((out2 - out0).cpu().numpy()).max() <= 1e-6 * np.abs(g["out"]).max() + 1e-7
        saved = w.data.clone()
        w.data.mul_(2.0)
        out3 = model(pil).clone()
        assert not torch.equal(torch.view_as_real(out3), torch.view_as_real(out2))
        model.train()
        w.data.copy_(saved)
        model.eval()
        out4 = model(pil)
        assert torch.equal(torch.view_as_real(out4), torch.view_as_real(out2))
        # the engine-level cache is opt-in and documents the caller's duty
        c1 = eng.forward(_t(g["pilots"]), cache_packed=True).clone()
        assert torch.equal(torch.view_as_real(c1), torch.view_as_real(out4))
        w.data.mul_(2.0)                                             # raw write: the cached image is now stale ...
        eng.invalidate_packed()                                      # ... until the caller says so
        c2 = eng.forward(_t(g["pilots"]), cache_packed=True)
        assert torch.equal(torch.view_as_real(c2), torch.view_as_real(out3))


# ---- split-precision tier (AFT_PRECISION_BF16X3): opt-in, reported separately, its own stated tolerance ----
TOL_SPLIT_OUT = 1e-3       # stated: max|d| <= 1e-3 |y|max  (include/adafortitran_amd.h)
TOL_SPLIT_MSE = 1e-2       # stated: |dMSE| / MSE <= 1e-2   (SURVEY.md 8d ceiling for the bf16 tier)


def _split(eng):
    eng.cfg.precision = _abi.AFT_PRECISION_BF16X3
    return eng


@pytest.mark.parametrize("name", DEFAULT_SETS)
def test_split_precision_tier_matches_reference_golden(name):
    """The bf16 hi/lo tier on the reference-generated goldens -- including A_ada, whose layer-0 logits reach +-500 (bf16-split
    q / k carry 16 mantissa bits: the hardest case for this tier)."""
    g = Golden(name)
    eng = _split(_engine(g))
    out = eng.forward(_t(g["pilots"]), *_meta(g)).cpu().numpy()
    ref = g["out"]
    err = np.abs(out - ref).max() / np.abs(ref).max()
    mse = np.mean(np.abs(out - g["target"]) ** 2)
    rel = abs(mse - g.meta["metric_2xmse"]) / g.meta["metric_2xmse"]
    print(f"split tier {name}: max|d|/|y|max {err:.2e}, |dMSE|/MSE {rel:.2e}")
    assert err <= TOL_SPLIT_OUT and rel <= TOL_SPLIT_MSE, (err, rel)


@pytest.mark.parametrize("batch", [1, 3, 37, 128])
def test_split_precision_tier_ragged_batches_and_determinism(oracle_lib, batch):
    hid = (7, 42, 560)
    sd = synth.make_state_dict(**DEFAULT_SPEC, adaptive_hidden=hid, seed=4242, attn_gain=0.25, head_gain=2.0)
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = _split(engine_from_numpy(cfg, sd, DEV))
    inp = synth.make_inputs(batch, seed=777 + batch)
    meta = [_t(inp[k]) for k in ("snr", "ds", "dop")]
    pil = _t(inp["pilots"])
    out = eng.forward(pil, *meta).clone()
    n = min(batch, 8)
    ref = oracle_lib.Oracle(cfg, sd).forward(inp["pilots"][:n], inp["snr"][:n], inp["ds"][:n], inp["dop"][:n])
    assert np.abs(out[:n].cpu().numpy() - ref).max() <= TOL_SPLIT_OUT * np.abs(ref).max()
    # deterministic, independent of what the workspace held, and frames independent of their batch
    eng.workspace(batch).view(torch.float32).fill_(float("nan"))
    assert torch.equal(torch.view_as_real(eng.forward(pil, *meta)), torch.view_as_real(out))
    if batch >= 37:
        part = eng.forward(pil[16:32], *[m[16:32] for m in meta])
        assert torch.equal(torch.view_as_real(part), torch.view_as_real(out[16:32]))


def test_split_precision_is_opt_in_and_refused_where_not_instantiated():
    from test_estimators_cpu import _configs
    g = Golden("D_forti")
    assert g.abi_config().precision == _abi.AFT_PRECISION_F32            # the default is exact fp32
    sc, mc = _configs(g.spec, device="cuda")
    model = A.FortiTranEstimator(sc, mc)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()})
    model.eval()
    pil = torch.from_numpy(g["pilots"])
    with torch.no_grad():
        exact = model(pil).clone()
        assert model._engine.cfg.precision == _abi.AFT_PRECISION_F32
        model.hip_precision = "bf16x3"
        fast = model(pil)
        assert model._engine.cfg.precision == _abi.AFT_PRECISION_BF16X3
    d = (fast - exact).abs().max().item() / exact.abs().max().item()
    assert 0 < d <= TOL_SPLIT_OUT
    odd = _abi.make_config(**dict(DEFAULT_SPEC, model_dim=192, num_head=6))   # model_dim 192: not instantiated for the tier
    odd.precision = _abi.AFT_PRECISION_BF16X3
    from adafortitran_amd.hip_ops import config_coverage
    assert "split-precision" in config_coverage(odd)


def test_split_precision_tier_config5(oracle_lib):
    """BASELINE config 5 (240x28, 12 layers, d = 256, 8 heads, 1120 tokens) in the split tier against the reference-generated golden."""
    g = Golden("C5_ada_large")
    eng = _split(_engine(g))
    out = eng.forward(_t(g["pilots"]), *_meta(g)).cpu().numpy()
    err = np.abs(out - g["out"]).max() / np.abs(g["out"]).max()
    print(f"split tier C5: max|d|/|y|max {err:.2e}")
    assert err <= TOL_SPLIT_OUT


@pytest.mark.parametrize("ofdm,pilot,patch,adaptive", [((30, 8), (6, 2), (3, 2), True), ((66, 12), (11, 3), (3, 3), False),
                                                        ((150, 8), (10, 2), (5, 2), True),
                                                        ((120, 14), (12, 2), (4, 2), True), ((120, 14), (12, 2), (2, 2), False),
                                                        ((54, 14), (6, 2), (3, 2), False)])
def test_split_precision_tier_other_grid_geometries(oracle_lib, ofdm, pilot, patch, adaptive):
    """Token counts that are not a multiple of 8 or 4 (40, 88, 120, 210, 420, 126) in the split tier: the in-projection epilogue's
    element-wise bf16 v^T stores, row tiles that straddle planes, ragged last key tiles with their bf16 masks."""
    tokens = (ofdm[0] // patch[0]) * (ofdm[1] // patch[1])
    spec = dict(ofdm=ofdm, pilot=pilot, patch=patch, num_layers=2, model_dim=128, num_head=4)
    hid = (5, 9, 2 * tokens) if adaptive else None
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, seed=99)
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    from adafortitran_amd.hip_ops import engine_from_numpy
    eng = _split(engine_from_numpy(cfg, sd, DEV))
    inp = synth.make_inputs(5, ofdm=ofdm, pilot=pilot, seed=31)
    meta = [(_t(inp[k]) if adaptive else None) for k in ("snr", "ds", "dop")]
    pil = _t(inp["pilots"])
    out = eng.forward(pil, *meta).clone()
    ref = oracle_lib.Oracle(cfg, sd).forward(inp["pilots"], *([inp["snr"], inp["ds"], inp["dop"]] if adaptive else [None] * 3))
    err = np.abs(out.cpu().numpy() - ref).max() / np.abs(ref).max()
    print(f"split tier {ofdm} patch {patch} ({tokens} tokens): max|d|/|y|max {err:.2e}")
    assert err <= TOL_SPLIT_OUT
    eng.workspace(5).view(torch.float32).fill_(float("nan"))
    assert torch.equal(torch.view_as_real(eng.forward(pil, *meta)), torch.view_as_real(out))
