"""The DIAGNOSTIC build of the kernels against the product build ("the diagnostic build").

``libaft_hip_diag.so`` = the same sources with -DAFT_DIAG_STAMPS (``python -m adafortitran_amd.build --diag``, built by
``__graft_entry__.build()``): with AFT_STAMPS=1 the launchers hand a stamp table to the launch the product makes (csrc/stamps.h,
aft_stamps.hip) and print what came back (csrc/stamp_report.h).  What is tested, on small shapes: the stamped launches are the
product's -- every output has the product build's BITS, at every head dimension, with column tiles and through a training layer -- and
the reports appear (matched by their leading words; what they compute is pinned on the CPU, tests/test_stamp_report.py, and so is
the capacity rule: no launch here comes near it).

The library prints only the first few reports of a kind per process, so the cases that expect report lines come first in this file
and each expects kinds no earlier case has used up."""
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib, synth
from adafortitran_amd.hip_ops import engine_from_numpy
from helpers import DEFAULT_SPEC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIAG = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_diag.so")
HID = (7, 42, 560)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def diag_lib():
    if not os.path.exists(DIAG):
        from adafortitran_amd import build
        build.build_diag()             # hipcc is on the GPU box too; normally the file travels with the tree
    lib = _lib.load_path(DIAG)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION
    return lib


@pytest.fixture
def diag(diag_lib, switches):
    """The diagnostic library with AFT_STAMPS=1 and, on both libraries, AFT_LAYER_FUSED=0 (the chain and attention launches run);
    both are restored behind the test -- the diagnostic library's switches through ITS aft_set_switch."""
    import ctypes as C
    old = {}
    for name, value in (("AFT_STAMPS", b"1"), ("AFT_LAYER_FUSED", b"0")):
        buf = C.create_string_buffer(256)
        rc = diag_lib.aft_get_switch(name.encode(), buf, 256)
        assert rc >= 0
        old[name] = buf.value if rc else None
        assert diag_lib.aft_set_switch(name.encode(), value) == _abi.AFT_OK
    switches.set("AFT_LAYER_FUSED", "0")
    yield diag_lib
    for name, value in old.items():
        assert diag_lib.aft_set_switch(name.encode(), value) == _abi.AFT_OK


def _forward_pair(spec, hid, diag, batch=2, seed=5, max_seq_len=512):
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, seed=seed, max_seq_len=max_seq_len)
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    inp = synth.make_inputs(batch, ofdm=spec["ofdm"], pilot=spec["pilot"], seed=seed + 1)
    pil, meta = _t(inp["pilots"]), [(_t(inp[k]) if hid else None) for k in ("snr", "ds", "dop")]
    want = engine_from_numpy(cfg, sd, DEV).forward(pil, *meta)
    got = engine_from_numpy(cfg, sd, DEV, lib=diag).forward(pil, *meta)
    torch.cuda.synchronize()
    assert torch.isfinite(torch.view_as_real(want)).all()
    return torch.equal(torch.view_as_real(got), torch.view_as_real(want))


def test_default_model_reports_its_launches_and_keeps_the_bits(diag, capfd):
    """Two frames, two layers of the default model as separate launches: the streaming conv head and tail, the chain in its three
    variants (in-projection only, layer, last layer) and attention each report; the output is the product's."""
    assert _forward_pair(dict(DEFAULT_SPEC, num_layers=2), HID, diag)
    out = capfd.readouterr().out
    for lead in ("conv stream16: input plane in LDS", "conv stream mode 0 (mean cycles): matrix wave:", "conv stream mode 1 (mean cycles): matrix wave:",
                 "  stamped: launch 1 of 1,", "chain<128,mlp=0,qkv=1>", "chain<128,mlp=1,qkv=1>", "chain<128,mlp=1,qkv=0>",
                 "  round 0 (", "in-kernel shader clock:", "attn stamps: mean per task: prologue=", "  round 0: start"):
        assert any(line.startswith(lead) for line in out.splitlines()), (lead, out)
    assert "does not fit" not in out


def test_training_layer_reports_and_keeps_output_and_gradients(diag, capfd):
    """One encoder layer's training forward and backward at model_dim 128, 280 tokens, one frame: the output and all thirteen
    gradients are the product's bits, and the fused forward chain reports."""
    from test_checked_build import _layer_step
    cfg = _abi.make_config(**dict(DEFAULT_SPEC, num_layers=2), adaptive_hidden=HID)
    d, tokens = 128, 280
    gen = torch.Generator().manual_seed(23)
    shapes = [(3 * d, d), (3 * d,), (d, d), (d,), (2 * d, d), (2 * d,), (d, 2 * d), (d,), (d,), (d,), (d,), (d,)]   # _abi.LAYER_FIELDS order
    params = [(torch.randn(s, generator=gen) * 0.1 + (1.0 if i in (8, 10) else 0.0)).to(DEV)
              for i, s in enumerate(shapes)]
    x, gout = torch.randn(2, tokens, d, generator=gen).to(DEV), torch.randn(2, tokens, d, generator=gen).to(DEV)
    want = _layer_step(_lib.load(), cfg, params, x, gout)
    got = _layer_step(diag, cfg, params, x, gout)
    torch.cuda.synchronize()
    assert len(want) == 14                     # the output, dx and the twelve parameter gradients
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.isfinite(b).all() and torch.equal(a, b), i
    out = capfd.readouterr().out
    for lead in ("chain_fwd_train<QKV=", "  mean cycles per tile: outproj="):
        assert any(line.startswith(lead) for line in out.splitlines()), (lead, out)


def test_column_tiled_conv_reports_and_keeps_the_bits(diag, capfd):
    """A 24 x 140 grid (tests/test_long_grids_gpu.py's column-tile case): the banded kernel runs planes x bands x COLUMN TILES
    workgroups in the stamped launch too."""
    spec = dict(ofdm=(24, 140), pilot=(4, 4), patch=(3, 2), num_layers=1, model_dim=64, num_head=2)
    assert _forward_pair(spec, None, diag, seed=3, max_seq_len=max(512, synth.token_count(24, 140, (3, 2))))
    out = capfd.readouterr().out
    assert any(line.startswith("conv mode 0 stamps (mean cycles, thread 0): weights=") for line in out.splitlines()), out
    assert any(line.startswith("conv mode 1 stamps (mean cycles, thread 0): weights=") for line in out.splitlines()), out


@pytest.mark.parametrize("heads", [2, 8])
def test_other_head_dimensions_keep_the_bits(diag, heads):
    """Head dimension 64 (its own attn_kernel instantiation, stamped) and 16 (attn16_kernel: never stamped) of the default model."""
    assert _forward_pair(dict(DEFAULT_SPEC, num_layers=2, num_head=heads), HID, diag)
