"""Host-only parts of the sync-free optimizer step: argument checks and scratch sizes of the new entry points (no launch happens:
every call below is refused, or is pure host arithmetic), the control block's layout, and the CPU-tensor twins of the new
``ShardedFlatAdam`` surface (``clip_grad_norm_``, ``last_grad_norm``, the count of applied steps)."""
import ctypes
import os

import pytest
import torch

from adafortitran_amd import _abi, _lib
from adafortitran_amd.optim import ShardedFlatAdam


def test_control_block_is_32_bytes_with_the_header_field_order():
    assert ctypes.sizeof(_abi.AftStepControl) == 32
    assert [f[0] for f in _abi.AftStepControl._fields_] == ["skip", "step", "grad_scale", "inv_bc1", "inv_sqrt_bc2", "grad_norm",
                                                            "clip_coef", "reserved"]
    assert _abi.AftStepControl.step.offset == 4 and _abi.AftStepControl.grad_norm.offset == 20    # optim.py views these words


def test_sumsq_scratch_size_is_host_arithmetic_on_n_alone():
    """One float64 partial + one uint32 flag per 4096-element chunk, rounded to 16 bytes; n up to 2^28 (and the 2^40 the call
    accepts) without overflow; 0 for what the call refuses."""
    lib = _lib.load()
    size = lib.aft_grad_sumsq_scratch_bytes
    for n in (1, 7, 4095, 4096, 4097, 1 << 20, (1 << 20) + 64, 1 << 28, 1 << 40):
        chunks = (n + 4095) // 4096
        assert size(n) == (chunks * 12 + 15) // 16 * 16, n
    assert size(1 << 28) == 65536 * 12
    assert size(0) == 0 and size((1 << 40) + 1) == 0


def test_new_entry_points_refuse_null_pointers_and_empty_buffers():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()                     # 512 bytes of host memory, 16-byte aligned below: never dereferenced
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    n, sb = 16, 16
    E = _abi.AFT_ERR_ARG

    def refused(rc, word):
        assert rc == E
        assert word in lib.aft_last_error().decode(), lib.aft_last_error()

    for args in ((None, n, p, sb, p, p), (p, n, None, sb, p, p), (p, n, p, sb, None, p), (p, n, p, sb, p, None), (p, 0, p, sb, p, p)):
        refused(lib.aft_grad_sumsq_f32(*args, None), "squared-norm")
    refused(lib.aft_grad_sumsq_f32(p, n, p, 8, p, p, None), "scratch")             # scratch too small
    refused(lib.aft_grad_sumsq_f32(p + 4, n, p, sb, p, p, None), "16-byte")         # misaligned gradient buffer
    refused(lib.aft_grad_sumsq_f32(p, (1 << 40) + 1, p, 1 << 40, p, p, None), "squared-norm")
    refused(lib.aft_adam_prepare_f32(None, p, p, p, 1.0, 1.0, 0.9, 0.999, None), "control block")
    refused(lib.aft_adam_prepare_f32(p, p, None, None, 1.0, -1.0, 0.9, 0.999, None), "max_norm")
    refused(lib.aft_adam_prepare_f32(p, p, None, None, 1.0, float("nan"), 0.9, 0.999, None), "max_norm")
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    for args in ((None, p, p, p, n, *hp, p), (p, None, p, p, n, *hp, p), (p, p, None, p, n, *hp, p), (p, p, p, None, n, *hp, p),
                 (p, p, p, p, n, *hp, None), (p, p, p, p, 0, *hp, p)):
        refused(lib.aft_adam_step_ctrl_f32(*args, None), "Adam")
    for args in ((None, n, p, 1.0, 1.0, p), (p, n, None, 1.0, 1.0, p), (p, n, p, 1.0, 1.0, None), (p, 0, p, 1.0, 1.0, p),
                 (p, 6, p, 1.0, 1.0, p), (p + 4, n, p, 1.0, 1.0, p), (p, n, p, 1.0, -2.0, p)):
        refused(lib.aft_grad_clip_f32(*args, None), "clipping")


def test_checked_build_exports_the_new_entry_points():
    """``python -m adafortitran_amd.build --variant check -DAFT_CHECKED=1`` compiles every source, the new kernels included."""
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path):
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION == 10
    assert lib.aft_grad_sumsq_scratch_bytes(1 << 20) == 256 * 12


def _pair(seed=0):
    torch.manual_seed(seed)
    a = torch.nn.Sequential(torch.nn.Linear(20, 33), torch.nn.Tanh(), torch.nn.Linear(33, 5))
    b = torch.nn.Sequential(torch.nn.Linear(20, 33), torch.nn.Tanh(), torch.nn.Linear(33, 5))
    b.load_state_dict(a.state_dict())
    return a, b


def test_cpu_clip_grad_norm_matches_torch_and_reports_the_norm():
    a, b = _pair()
    opt = ShardedFlatAdam(b.parameters(), lr=1e-2)
    ref = torch.optim.Adam(a.parameters(), lr=1e-2)
    assert opt.last_grad_norm is None
    gen = torch.Generator().manual_seed(3)
    for it, amp in enumerate((5.0, 1e-3, 2.0)):            # above, below, above the clip value
        for p, q in zip(a.parameters(), b.parameters()):
            g = torch.randn(p.shape, generator=gen) * amp
            p.grad = g.clone()
            q.grad.copy_(g)
        want = torch.nn.utils.clip_grad_norm_(a.parameters(), 1.0)
        got = opt.clip_grad_norm_(1.0)
        assert got.dim() == 0 and got.dtype == torch.float32
        assert (want > 1.0) == (it != 1)
        assert abs(float(got) - float(want)) <= 1e-6 * float(want)
        assert float(opt.last_grad_norm) == float(got)
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.allclose(p.grad, q.grad, rtol=1e-6, atol=1e-12)
        ref.step()
        opt.step()
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.allclose(p, q, rtol=0, atol=1e-6)
    assert opt.steps == 3


def test_cpu_steps_counts_applied_steps_and_round_trips():
    _, b = _pair(1)
    opt = ShardedFlatAdam(b.parameters(), lr=1e-2, max_grad_norm=1.0)
    x = torch.randn(8, 20)
    for found in (0.0, 1.0, 0.0):
        opt.zero_grad()
        b(x).square().mean().backward()
        opt.found_inf, opt.grad_scale = torch.tensor([found]), None      # what GradScaler.step sets around the call
        try:
            opt.step()
        finally:
            del opt.found_inf, opt.grad_scale
    assert opt.steps == 2 and float(opt.state_dict()["state"][0]["step"]) == 2.0
    assert opt.last_grad_norm is not None and opt.last_grad_norm.dim() == 0 and opt.last_grad_nonfinite is None
    _, c = _pair(1)
    opt2 = ShardedFlatAdam(c.parameters(), lr=1e-2)
    opt2.load_state_dict(opt.state_dict())
    assert opt2.steps == 2 and torch.equal(opt2.exp_avg, opt.exp_avg)
    with pytest.raises(AttributeError):
        opt.last_grad_norm = None                                        # read-only
