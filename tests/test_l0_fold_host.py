"""The fold of layer 0's keys and values lives in regions the workspace plan already has: no byte of the plan moves.

PARENT holds what the commit before the fold answered (taken from a build of it): aft_workspace_bytes, aft_workspace_bytes_layer_fused
and the (offset, size) of the three regions aft_workspace_region names, at batches 1, 5 and 128.  No GPU needed."""
import ctypes

import pytest

from adafortitran_amd import _abi, _lib
from helpers import DEFAULT_SPEC

HID = (7, 42, 560)
CONFIGS = {"C3": (DEFAULT_SPEC, HID), "C2": (DEFAULT_SPEC, None), "d256": (dict(DEFAULT_SPEC, model_dim=256, num_head=8), HID)}
# (config, batch) -> (workspace bytes, with the fused layer sequence's blocks, [(offset, size) of conv_enhanced, tokens6, enc_out])
PARENT = {
    ("C3", 1): (4705024, 5294848, [(0, 13440), (13568, 6720), (4640768, 17920)]),
    ("C3", 5): (20316160, 23265280, [(0, 67200), (67328, 33600), (10586880, 89600)]),
    ("C3", 128): (205337600, 280835072, [(0, 1720320), (1720320, 860160), (193421312, 2293760)]),
    ("C2", 1): (4705024, 5294848, [(0, 13440), (13568, 0), (4640768, 17920)]),
    ("C2", 5): (20316160, 23265280, [(0, 67200), (67328, 0), (10586880, 89600)]),
    ("C2", 128): (205337600, 280835072, [(0, 1720320), (1720320, 0), (193421312, 2293760)]),
    ("d256", 1): (15616768, 15616768, [(0, 13440), (13568, 6720), (15552512, 17920)]),
    ("d256", 5): (65421312, 65421312, [(0, 67200), (67328, 33600), (27364096, 89600)]),
    ("d256", 128): (430781440, 430781440, [(0, 1720320), (1720320, 860160), (390553600, 2293760)]),
}


@pytest.mark.parametrize("fold", [None, "0", "1"])
def test_workspace_plan_is_the_parents(switches, fold):
    """... whatever the switch says: the plan does not read it."""
    lib = _lib.load()
    if fold is None:
        switches.unset("AFT_L0_FOLD")
    else:
        switches.set("AFT_L0_FOLD", fold)
    for (name, batch), (plain, fused, regions) in PARENT.items():
        spec, hid = CONFIGS[name]
        cfg = _abi.make_config(**spec, adaptive_hidden=hid)
        assert lib.aft_workspace_bytes(ctypes.byref(cfg), batch) == plain, (name, batch)
        assert lib.aft_workspace_bytes_layer_fused(ctypes.byref(cfg), batch) == fused, (name, batch)
        for region, want in zip(("conv_enhanced", "tokens6", "enc_out"), regions):
            off, size = ctypes.c_size_t(), ctypes.c_size_t()
            assert lib.aft_workspace_region(ctypes.byref(cfg), batch, _abi.REGION_IDS[region], ctypes.byref(off), ctypes.byref(size)) == _abi.AFT_OK
            assert (off.value, size.value) == want, (name, batch, region)


def test_the_tables_fit_the_attention_region_at_every_batch():
    """The two tables take 2 x tokpad x model_dim floats of `attn`, which is planes x tokpad x model_dim floats or more: the region
    between q's and attn's starts cannot be asked for, but the plan's total at batch 1 bounds it from above and the fused block (one
    planes x tokpad x model_dim block, test_layer_fused_gpu.py) is exactly the size the tables need at batch 1."""
    lib = _lib.load()
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=HID)
    block = (lib.aft_workspace_bytes_layer_fused(ctypes.byref(cfg), 1) - lib.aft_workspace_bytes(ctypes.byref(cfg), 1)) // 2
    assert block == 4 * 2 * 288 * 128       # planes x tokpad x model_dim floats at batch 1 = the two tables


def test_switch_is_declared_and_reads_back(switches):
    switches.set("AFT_L0_FOLD", "0")
    assert _lib.get_switch("AFT_L0_FOLD") == "0"
    switches.set("AFT_L0_FOLD", "1")
    assert _lib.get_switch("AFT_L0_FOLD") == "1"
    switches.unset("AFT_L0_FOLD")
    assert _lib.get_switch("AFT_L0_FOLD") is None
