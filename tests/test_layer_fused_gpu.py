"""The fused layer sequence (k_layer.hip): one launch per encoder layer on plane-aligned row tiles.

Per row every product keeps its k order and every LayerNorm its merge order, so the estimate must carry the BITS of the
[attention, chain] launch sequence: every GPU test here runs the same seeded synthetic weights and inputs with AFT_LAYER_FUSED=1
and =0 and compares with torch.equal.  Host-only tests pin the selection rule, the opt-in workspace size and the register budget of the new kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib, synth
from helpers import DEFAULT_SPEC, TOL_HIP_OUT

DEV = "cuda:0"
L2 = dict(DEFAULT_SPEC, num_layers=2)
HID = (7, 42, 560)


def _t(a):
    return torch.from_numpy(a).to(DEV)


def _setup(spec, hid, batch, seed):
    from adafortitran_amd.hip_ops import engine_from_numpy
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, seed=seed)
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    inp = synth.make_inputs(batch, ofdm=spec["ofdm"], pilot=spec["pilot"], seed=seed + 1)
    meta = [_t(inp[k]) for k in ("snr", "ds", "dop")] if hid else []
    return engine_from_numpy(cfg, sd, DEV), _t(inp["pilots"]), meta, (cfg, sd, inp)


def _both(switches, eng, pil, meta, batch, eligible=True):
    """The forward with the switch at 0 and at 1; asserts which sequence the library says it runs."""
    out = {}
    for v in ("0", "1"):
        switches.set("AFT_LAYER_FUSED", v)
        assert _lib.load().aft_layer_fused_of(ctypes.byref(eng.cfg), batch) == (1 if v == "1" and eligible else 0)
        out[v] = torch.view_as_real(eng.forward(pil, *meta).clone())
    assert torch.isfinite(out["0"]).all()
    return out["0"], out["1"]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("adaptive", [False, True])
def test_ragged_ninth_tile_matches_launch_path(switches, adaptive, batch):
    """120 x 14 grid: 280 tokens, nine tiles per plane, the ninth with 24 valid rows; 2 and 6 planes: every plane boundary is a tile
    boundary, and the grid is smaller than the co-resident workgroup count."""
    eng, pil, meta, _ = _setup(L2, HID if adaptive else None, batch, seed=100 + batch)
    a, b = _both(switches, eng, pil, meta, batch)
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_whole_tiles_only_matches_launch_path(switches):
    """96 x 14 with 3 x 2 patches: 224 tokens = 7 whole tiles per plane -- the generic token-count instantiation, no ragged tile."""
    eng, pil, meta, _ = _setup(dict(L2, ofdm=(96, 14)), None, 2, seed=200)
    a, b = _both(switches, eng, pil, meta, 2)
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_last_tile_with_one_valid_row_matches_launch_path(switches):
    """99 x 2 with 3 x 2 patches: 33 tokens = 32 + 1 -- the second tile of every plane holds ONE valid row (and one valid key)."""
    eng, pil, meta, _ = _setup(dict(L2, ofdm=(99, 2), pilot=(11, 1)), None, 2, seed=300)
    assert eng.tokens == 33
    a, b = _both(switches, eng, pil, meta, 2)
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_token_count_not_a_multiple_of_four_matches_launch_path(switches):
    """120 x 14 with 4 x 2 patches: 210 tokens = 6 x 32 + 18 -- the last V^T group of four keys of a plane holds TWO valid tokens, stored
    one by one (every token its own value), and the attention masks padded keys lane by lane instead of in groups of eight."""
    eng, pil, meta, _ = _setup(dict(L2, patch=(4, 2)), (7, 42, 420), 2, seed=350)
    assert eng.tokens == 210
    a, b = _both(switches, eng, pil, meta, 2)
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_fused_bits_do_not_depend_on_the_workspace(switches):
    """B = 5, six layers: rows 280..287 of every plane's ninth tile (x, q / k / v^T, the second K / V^T buffers behind the planned workspace) are never written and
    never reach a stored value: a NaN- and a 1e30-filled workspace give the bits of a zero-filled one -- and of the launch path."""
    eng, pil, meta, _ = _setup(DEFAULT_SPEC, HID, 5, seed=400)
    ref, _ = _both(switches, eng, pil, meta, 5)
    outs = []
    for fill in (0.0, float("nan"), 1e30):
        eng.workspace(5).view(torch.float32).fill_(fill)
        outs.append(torch.view_as_real(eng.forward(pil, *meta).clone()))     # the switch is still at 1
    assert torch.isfinite(outs[0]).all()
    for fill, o in zip(("nan", "1e30"), outs[1:]):
        assert torch.equal(o, outs[0]), fill
    assert torch.equal(outs[0], ref)


@pytest.mark.gpu
def test_fused_frames_do_not_depend_on_their_batch(switches):
    """Frames 3..7 of a 37-frame call equal a 5-frame call on those frames (other tile walk, other workgroups, lanes or not)."""
    eng, pil, meta, _ = _setup(L2, HID, 37, seed=500)
    launches, big = _both(switches, eng, pil, meta, 37)
    small = torch.view_as_real(eng.forward(pil[3:8], *[m[3:8] for m in meta]).clone())
    assert torch.equal(big[3:8], small)
    assert torch.equal(big, launches)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["head_dim_16", "tokens_below_32", "split_precision"])
def test_ineligible_configurations_run_the_launch_path(switches, oracle_lib, case):
    """What the fused kernels are not instantiated for runs the launches whatever the switch says, and returns the right answer."""
    spec = {"head_dim_16": dict(L2, num_head=8), "tokens_below_32": dict(L2, ofdm=(30, 4), pilot=(6, 2)), "split_precision": L2}[case]
    eng, pil, meta, (cfg, sd, inp) = _setup(spec, None, 2, seed=600)
    if case == "split_precision":
        eng.cfg.precision = _abi.AFT_PRECISION_BF16X3
    a, b = _both(switches, eng, pil, meta, 2, eligible=False)
    assert torch.equal(a, b)
    if case != "split_precision":       # (the split tier has its own tolerance and its own tests; here: it still runs, finite, unfused)
        ref = oracle_lib.Oracle(cfg, sd).forward(inp["pilots"], None, None, None)
        out = torch.view_as_complex(b).cpu().numpy()
        assert np.abs(out - ref).max() <= TOL_HIP_OUT * np.abs(ref).max()


@pytest.mark.gpu
def test_a_workspace_without_room_runs_the_launches(switches):
    """The fused sequence's two extra blocks lie behind the planned workspace: a caller who passes exactly aft_workspace_bytes gets the
    launch path -- same bits, nothing written past the end of the buffer (a NaN guard behind it stays NaN)."""
    eng, pil, meta, _ = _setup(L2, HID, 3, seed=700)
    switches.set("AFT_LAYER_FUSED", "1")
    ref = torch.view_as_real(eng.forward(pil, *meta).clone())
    lib = _lib.load()
    small = lib.aft_workspace_bytes(ctypes.byref(eng.cfg), 3)
    assert lib.aft_workspace_bytes_layer_fused(ctypes.byref(eng.cfg), 3) > small
    buf = torch.full((small // 4 + 4096,), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.empty_like(ref)
    rc = lib.aft_forward_f32(ctypes.byref(eng.cfg), ctypes.byref(eng.weights), torch.view_as_real(pil).data_ptr(), *[m.reshape(-1).float().data_ptr() for m in meta],
                             out.data_ptr(), buf.data_ptr(), small, 3, eng._stream())
    assert rc == _abi.AFT_OK, lib.aft_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert torch.isnan(buf[small // 4:]).all()


# ---- every layer_kernel instantiation, walks of more than one tile per workgroup, lanes, stale workspaces ----
# d = 128, 4 heads.  Token count -> (grid, patch): N tokens are the grid (3 N, 2) at patch 3 x 2 except where noted.
GRIDS = {280: ((120, 14), (3, 2)), 210: ((120, 14), (4, 2)), 512: ((192, 16), (3, 2))}
INSTANTIATION_TOKENS = [32, 33, 40, 41, 64, 65, 210, 280]


def _spec(tokens, layers):
    ofdm, patch = GRIDS.get(tokens, ((3 * tokens, 2), (3, 2)))
    return dict(DEFAULT_SPEC, ofdm=ofdm, patch=patch, num_layers=layers)


def _setup_act(tokens, layers, act, adaptive, batch, seed):
    """_setup on the token count's grid; the activation is the configuration's alone (the synthetic weights do not know it)."""
    eng, pil, meta, rest = _setup(_spec(tokens, layers), (7, 42, 2 * tokens) if adaptive else None, batch, seed)
    eng.cfg.activation = _abi.AFT_ACT_GELU if act == "gelu" else _abi.AFT_ACT_RELU
    assert eng.tokens == tokens
    return eng, pil, meta, rest


@pytest.mark.gpu
@pytest.mark.parametrize("tokens", INSTANTIATION_TOKENS)
@pytest.mark.parametrize("layers", [1, 2, 3])
@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_every_instantiation_matches_launch_path(switches, act, layers, tokens):
    """layer_kernel<activation, last layer or not, 280 tokens or any count> at batch 2: 32 tokens are one tile and one key tile per
    plane; a single layer runs only the first launch and the last-layer kernel; three layers end on the other K / V^T buffer than two.
    Adaptive on for half of the cases."""
    adaptive = (INSTANTIATION_TOKENS.index(tokens) + layers + (act == "relu")) % 2 == 0
    eng, pil, meta, _ = _setup_act(tokens, layers, act, adaptive, 2, seed=800 + 10 * tokens + layers)
    a, b = _both(switches, eng, pil, meta, 2)
    assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_xcd_remap_below_the_resident_count_matches_launch_path(switches, act):
    """Batch 4 at 280 tokens: 8 planes x 9 tiles = 72 workgroups, a multiple of 8 -- the XCD remap is active on a grid smaller than the
    co-resident workgroup count."""
    eng, pil, meta, _ = _setup_act(280, 2, act, act == "relu", 4, seed=850)
    a, b = _both(switches, eng, pil, meta, 4)
    assert torch.equal(a, b)


def _slots():
    return 3 * torch.cuda.get_device_properties(0).multi_processor_count


def _ceil_div(a, b):
    return -(-a // b)


# (tokens, act, layers, frames as a function of slots = 3 x CUs).  At 256 CUs: 43 frames = 774 tiles, a few workgroups take a second tile
# and the remap is active; 64 frames = 1.5 rounds; 193 frames of 33 tokens = 772 tiles, a second-round tile may hold a single valid row;
# 25 frames of 512 tokens = 800 tiles of 16 per plane on the run-time count.
WALKS = {"280tok_a_few_second_tiles": (280, "gelu", 2, lambda s: _ceil_div(s + 1, 18)),
         "280tok_one_and_a_half_rounds": (280, "gelu", 2, lambda s: _ceil_div(3 * s, 2 * 18)),
         "33tok_relu_three_layers": (33, "relu", 3, lambda s: _ceil_div(s + 1, 4)),
         "512tok_relu_one_layer": (512, "relu", 1, lambda s: _ceil_div(s + 1, 32))}


@pytest.mark.gpu
@pytest.mark.parametrize("walk", list(WALKS))
def test_partial_second_round_matches_launch_path(switches, walk):
    """One lane, more plane-aligned tiles than the 3 x CUs workgroups of the persistent grid, a partial last round: the workgroups that
    take a second tile, and the ones that do not, carry the bits of the launches; the last three frames -- second-round tiles -- equal a
    3-frame call on those frames."""
    tokens, act, layers, frames_of = WALKS[walk]
    slots = _slots()
    batch = frames_of(slots)
    tiles = 2 * batch * _ceil_div(tokens, 32)
    assert slots < tiles < 2 * slots, (slots, tiles)
    switches.set("AFT_LANES", "1")
    eng, pil, meta, _ = _setup_act(tokens, layers, act, walk.startswith("280"), batch, seed=900 + tokens)
    launches, big = _both(switches, eng, pil, meta, batch)
    assert torch.equal(big, launches)
    k = batch - 3      # (a workgroup's second tile is its first + the grid size: the second round is the last tiles, so the last frames)
    small = torch.view_as_real(eng.forward(pil[k:k + 3], *[m[k:k + 3] for m in meta]).clone())      # the switch is still at 1
    assert torch.equal(big[k:k + 3], small)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [64, 100])
def test_default_lanes_match_launch_path(switches, batch):
    """AFT_LANES unset, 280 tokens: whatever split aft_workspace_lanes reports gives the bits of the launches."""
    switches.unset("AFT_LANES")
    eng, pil, meta, _ = _setup_act(280, 2, "gelu", True, batch, seed=950 + batch)
    lanes, frames, offs = ctypes.c_int(), (ctypes.c_int * 4)(), (ctypes.c_size_t * 4)()
    for v in ("0", "1"):
        switches.set("AFT_LAYER_FUSED", v)
        assert _lib.load().aft_workspace_lanes(ctypes.byref(eng.cfg), batch, ctypes.byref(lanes), frames, offs) == _abi.AFT_OK
        assert 1 <= lanes.value <= 4 and sum(frames[:lanes.value]) == batch
        print(f"batch {batch} AFT_LAYER_FUSED={v}: {lanes.value} lane(s) of {list(frames[:lanes.value])} frames")
    a, b = _both(switches, eng, pil, meta, batch)
    assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("tokens", [33, 210])
def test_stale_workspace_on_ragged_run_time_counts(switches, tokens):
    """33 and 210 tokens (a last tile of 1 and of 18 valid rows, the run-time token count), relu, three layers, batch 3: a NaN- and a
    1e30-filled workspace give the bits of a zero-filled one -- and of the launch path."""
    eng, pil, meta, _ = _setup_act(tokens, 3, "relu", tokens == 210, 3, seed=1000 + tokens)
    ref, _ = _both(switches, eng, pil, meta, 3)
    outs = []
    for fill in (0.0, float("nan"), 1e30):
        eng.workspace(3).view(torch.float32).fill_(fill)
        outs.append(torch.view_as_real(eng.forward(pil, *meta).clone()))     # the switch is still at 1
    assert torch.isfinite(outs[0]).all()
    for fill, o in zip(("nan", "1e30"), outs[1:]):
        assert torch.equal(o, outs[0]), fill
    assert torch.equal(outs[0], ref)


# ---- host only ----
def test_fused_workspace_size_is_the_plan_plus_two_blocks():
    """aft_workspace_bytes stays what it was; the opt-in size adds x on plane-aligned tiles and the second V^T buffer (each planes x
    tokpad x model_dim floats: a whole number of 256-byte units, so exactly that much), and nothing where the sequence is not
    instantiated."""
    lib = _lib.load()
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=HID)
    for b in (1, 5, 37, 128):
        base, big = lib.aft_workspace_bytes(ctypes.byref(cfg), b), lib.aft_workspace_bytes_layer_fused(ctypes.byref(cfg), b)
        block = 4 * 2 * b * 288 * 128
        assert big == base + 2 * block
    other = _abi.make_config(**dict(DEFAULT_SPEC, num_head=8), adaptive_hidden=None)
    assert lib.aft_workspace_bytes_layer_fused(ctypes.byref(other), 8) == lib.aft_workspace_bytes(ctypes.byref(other), 8) > 0


def test_selection_rule(switches):
    """The default: fused where plane-aligned tiles add no round to the persistent grid of 3 x CUs workgroups.  The benchmark's batch
    (256 planes x 9 = 2 304 = 3 x 768 tiles against 2 240 global ones: three rounds either way) runs fused; 129 frames (2 322
    plane-aligned tiles: a fourth round, 2 258 global ones: three) the launches.  The rule is written in CUs: the decisions are
    asserted for the MI355X's 256, the library's answer when no device is visible too."""
    lib = _lib.load()
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=HID)
    fused = lambda c, b: lib.aft_layer_fused_of(ctypes.byref(c), b)   # noqa: E731
    switches.unset("AFT_LAYER_FUSED")
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    if cus == 256:
        assert [fused(cfg, b) for b in (1, 64, 127, 128, 129, 130, 192)] == [1, 1, 1, 1, 0, 0, 1]
    for b in (1, 128, 129):
        slots = 3 * cus
        assert fused(cfg, b) == int(-(-(2 * b * 9) // slots) <= -(-(-(-(2 * b * 280) // 32)) // slots))
    switches.set("AFT_LAYER_FUSED", "0")
    assert fused(cfg, 128) == 0
    switches.set("AFT_LAYER_FUSED", "1")
    assert fused(cfg, 129) == 1
    # never what the kernels are not instantiated for, never against the caller's explicit path, whatever the switch says
    assert fused(_abi.make_config(**dict(DEFAULT_SPEC, num_head=8), adaptive_hidden=None), 128) == 0
    assert fused(_abi.make_config(**dict(DEFAULT_SPEC, model_dim=256, num_head=8), adaptive_hidden=None), 128) == 0
    assert fused(_abi.make_config(**dict(DEFAULT_SPEC, ofdm=(30, 4), pilot=(6, 2)), adaptive_hidden=None), 128) == 0
    forced = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=HID)
    forced.encoder_path = _abi.AFT_ENCODER_LAUNCHES
    assert fused(forced, 128) == 0
    split = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=HID)
    split.precision = _abi.AFT_PRECISION_BF16X3
    assert fused(split, 128) == 0
    assert fused(cfg, 0) == -1


def test_layer_kernels_have_no_register_spills():
    """hipcc's own resource report for k_layer.hip: every layer_kernel instantiation (activation x last layer or not x 280 tokens at
    compile time or any count) and the plane-tile form of the first launch stay inside the 168 registers three waves per SIMD allow --
    no vector register spilled, no scratch (a scratch reload is a VMEM load whose wait drains vmcnt)."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adafortitran_amd", "csrc")
    res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "k_layer.hip", "-o", "/dev/null",
                          "-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    report, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
        for key, pat in (("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgprs", r" VGPRs: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                report[name][key] = int(m.group(1))
    layer = {k: v for k, v in report.items() if "layer_kernel" in k}
    first = {k: v for k, v in report.items() if "chain_plane_tiles_kernel" in k}
    assert len(layer) == 8 and len(first) == 1, report
    for k, v in {**layer, **first}.items():
        assert v["spill"] == 0 and v["scratch"] == 0 and v["vgprs"] <= 168 and v["occupancy"] >= 3, (k, v)
