"""OFDM grids longer than 64 symbols: the conv stacks' column tiles give every grid a plan, so the coverage predicates
accept them (CPU: no kernel runs here)."""
import ctypes

import pytest

from adafortitran_amd import _abi, _lib

P, G = _abi.AFT_ENGINE_PACKED, _abi.AFT_ENGINE_GENERAL


def _cfg(ofdm, pilot, patch, d=128, heads=4, adaptive=False):
    spec = dict(ofdm=ofdm, pilot=pilot, patch=patch, num_layers=2, model_dim=d, num_head=heads)
    tokens = (ofdm[0] // patch[0]) * (ofdm[1] // patch[1])
    return _abi.make_config(**spec, adaptive_hidden=(7, 42, 2 * tokens) if adaptive else None)


# (ofdm, pilot, patch, model_dim, heads, engine): 120 x 64 with the default model was refused (linear_2's weights beside the plane),
# 120 x 65 and longer had no band plan at all; 264 x 72 and 300 x 100 need row bands AND column tiles; 3 x 1000 has one-row planes
LONG_GRIDS = [
    ((120, 64), (12, 2), (3, 2), 128, 4, P),
    ((120, 65), (12, 5), (3, 5), 128, 4, P),
    ((120, 65), (12, 5), (3, 5), 512, 8, G),
    ((24, 140), (4, 4), (3, 2), 64, 2, P),
    ((24, 140), (4, 4), (3, 2), 200, 8, G),
    ((12, 560), (4, 8), (3, 2), 128, 4, P),
    ((12, 560), (4, 8), (3, 2), 512, 8, G),
    ((264, 72), (8, 4), (3, 2), 64, 2, P),
    ((264, 72), (8, 4), (3, 2), 200, 8, G),
    ((300, 100), (10, 4), (3, 2), 64, 2, P),
    ((300, 100), (10, 4), (3, 2), 512, 8, G),
    ((3, 1000), (3, 8), (3, 2), 128, 4, P),
    ((3, 1000), (3, 8), (3, 2), 48, 2, G),
]


@pytest.mark.parametrize("ofdm,pilot,patch,d,heads,engine", LONG_GRIDS)
@pytest.mark.parametrize("adaptive", [False, True])
def test_long_grids_are_covered(ofdm, pilot, patch, d, heads, engine, adaptive):
    lib = _lib.load()
    cfg = _cfg(ofdm, pilot, patch, d, heads, adaptive)
    assert lib.aft_check_config(ctypes.byref(cfg)) == _abi.AFT_OK, lib.aft_last_error()
    assert lib.aft_engine_of(ctypes.byref(cfg)) == engine
    assert lib.aft_workspace_bytes(ctypes.byref(cfg), 4) > 0
    assert lib.aft_max_batch(ctypes.byref(cfg)) > 0
    S, T = ofdm
    assert lib.aft_conv_enhancer_scratch_bytes(4, S, T) > 0
    assert lib.aft_conv_enhancer_fwd_scratch_bytes(4, S, T) > 0


@pytest.mark.parametrize("S,T", [(1, 65), (3, 1000), (24, 140), (240, 600), (264, 72), (300, 100), (2000, 2000)])
def test_every_grid_has_a_conv_stack_plan(S, T):
    """The training entry points ask for a plan without side data: any (S, T) gets one."""
    lib = _lib.load()
    assert lib.aft_conv_enhancer_scratch_bytes(2, S, T) > 0
    assert lib.aft_conv_enhancer_fwd_scratch_bytes(2, S, T) > 0


def test_training_backends_of_a_long_grid_are_the_kernels():
    """training_backends() hands neither conv stack to autograd on a grid the band plan cannot hold (the HIP device is not needed to
    ask: the predicate is the library's)."""
    from adafortitran_amd.hip_ops import conv_enhancer_covered
    for S, T in ((24, 140), (120, 65), (264, 72), (3, 1000)):
        assert conv_enhancer_covered(S, T)


def test_conv_training_refuses_planes_past_32_bit_offsets():
    """The training kernels address one launch's saved activations with 32-bit byte offsets: calls run in chunks of planes below
    2 GiB of conv2 activations, and a grid whose single plane passes that is refused rather than computed wrong."""
    lib = _lib.load()
    assert lib.aft_conv_enhancer_scratch_bytes(256, 120, 600) > 0          # 2.4 GB of conv2 activations: two launches
    assert lib.aft_conv_enhancer_scratch_bytes(1, 5000, 5000) == 0
    assert lib.aft_conv_enhancer_fwd_scratch_bytes(1, 5000, 5000) == 0
