"""tests/test_checked_build.py for grids longer than 64 symbols: the CHECKED build (-DAFT_CHECKED=1: the banded
kernel asserts that a column tile's window holds its owned columns and their halo inside the LDS arena; the row-streaming kernel's ring
tags) against the product build, on the row-streaming and the 2-D tiled paths: no assert fires, same bits."""
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHECK = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def checked():
    if not os.path.exists(CHECK):
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(CHECK)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION
    return lib


@pytest.mark.parametrize("ofdm,pilot,patch,batch,banded", [((24, 140), (4, 4), (3, 2), 3, False), ((120, 66), (12, 2), (3, 2), 70, False),
                                                           ((120, 66), (12, 2), (3, 2), 3, True),
                                                           ((264, 72), (8, 4), (8, 2), 2, False), ((3, 1000), (3, 8), (3, 10), 5, False),
                                                           ((12, 560), (4, 8), (3, 2), 2, True)])
def test_long_grids_on_the_checked_build(switches, checked, ofdm, pilot, patch, batch, banded):
    from adafortitran_amd.hip_ops import engine_from_numpy
    tokens = synth.token_count(*ofdm, patch)
    spec = dict(ofdm=ofdm, pilot=pilot, patch=patch, num_layers=1, model_dim=64, num_head=2)
    hid = (5, 11, 2 * tokens)
    sd = synth.make_state_dict(**spec, adaptive_hidden=hid, seed=12, max_seq_len=max(512, tokens))
    cfg = _abi.make_config(**spec, adaptive_hidden=hid)
    if banded:   # both libraries: each keeps its own switch table
        switches.set("AFT_CONV_BANDED", "1")
        assert checked.aft_set_switch(b"AFT_CONV_BANDED", b"1") == _abi.AFT_OK
    try:
        prod, chk = engine_from_numpy(cfg, sd, DEV), engine_from_numpy(cfg, sd, DEV, lib=checked)
        inp = synth.make_inputs(batch, ofdm=ofdm, pilot=pilot, seed=13)
        pil, meta = _t(inp["pilots"]), [_t(inp[k]) for k in ("snr", "ds", "dop")]
        want = prod.forward(pil, *meta)
        got = chk.forward(pil, *meta)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(got), torch.view_as_real(want))
        assert torch.equal(chk.stage_upsample(pil), prod.stage_upsample(pil))
    finally:
        checked.aft_set_switch(b"AFT_CONV_BANDED", None)
