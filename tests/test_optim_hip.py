"""The optimizer step on the HIP device without a host read: device-side gradient norm / clipping, GradScaler's skip, the count of
applied steps (``ShardedFlatAdam`` in ``adafortitran_amd/optim.py``; kernels in ``csrc/k_train.hip``).

Fixed synthetic gradients are written into ``p.grad`` (no forward): the amplitudes alternate so that the global norm is far above
the clip value 1.0 in some steps and far below it in others.  The references are the reference trainer's own calls
(``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.Adam``, src/main/trainer.py:211-224,407-413) in float64 on the CPU (a) and in
float32 on the device (b); what the new path (c) may differ from (a) by is bounded by what torch's own float32 run differs by."""
import numpy as np
import pytest
import torch

from adafortitran_amd import _lib
from adafortitran_amd.optim import ShardedFlatAdam

pytestmark = pytest.mark.gpu
LR, CLIP, STEPS = 1e-3, 1.0, 5
AMPS = (5e-3, 1e-5, 4e-3, 3e-5, 1e-3)      # x sqrt(#parameters ~ 3.5e5): norms ~ 3, 0.006, 2.4, 0.02, 0.6


def _model(name, dropout, pos="learnable"):
    import adafortitran_amd as A
    sc = A.SystemConfig(ofdm=dict(num_scs=120, num_symbols=14), pilot=dict(num_scs=12, num_symbols=2))
    kw = dict(model_type=name, patch_size=(3, 2), num_layers=2, model_dim=128, num_head=4, activation="gelu",
              max_seq_len=512, pos_encoding_type=pos, device="cuda", dropout=dropout)
    if name == "adafortitran":
        kw.update(channel_adaptivity_hidden_sizes=[7, 42, 560], adaptive_token_length=6)
    cls = A.AdaFortiTranEstimator if name == "adafortitran" else A.FortiTranEstimator
    return cls(sc, A.ModelConfig(**kw))


def _fresh_model():
    torch.manual_seed(5)
    return _model("fortitran", 0.0).train()


def _gradients(model, amps=AMPS, seed=1234):
    """One list of CPU float32 gradients per step, drawn once."""
    gen = torch.Generator().manual_seed(seed)
    return [[torch.randn(p.shape, generator=gen) * amp for p in model.parameters()] for amp in amps]


def _poke(tensors, value):
    """Element 17 of the largest tensor of a list of gradients (any fixed place does)."""
    max(tensors, key=lambda t: t.numel()).view(-1)[17] = value


def _vec(params):
    return torch.cat([p.detach().reshape(-1).double().cpu() for p in params])


def _torch_run(params0, grads, dtype, device):
    """clip_grad_norm_ + torch.optim.Adam on copies of the parameters; parameter vector and pre-clip norm after every step."""
    params = [torch.nn.Parameter(p.detach().to(device=device, dtype=dtype).clone()) for p in params0]
    opt = torch.optim.Adam(params, lr=LR)
    traj, norms = [], []
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.to(device=device, dtype=dtype).clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, CLIP)))
        opt.step()
        traj.append(_vec(params))
    return traj, norms


def _write_grads(model, gs, scale=1.0):
    for p, g in zip(model.parameters(), gs):
        p.grad.copy_(g.to(p.device) * scale)


def _within_torch_fp32_error(got, ref64, torch32, what):
    """The issue's criterion on the finite elements: max|got - a| <= 2 max|b - a| + lr 1e-6, and the same for the median."""
    fin = torch.isfinite(ref64)
    assert torch.equal(torch.isfinite(got), fin) and torch.equal(torch.isfinite(torch32), fin), what
    dc, db = (got - ref64)[fin].abs(), (torch32 - ref64)[fin].abs()
    print(f"{what}: max|c-a| {float(dc.max()):.3e} (torch fp32 {float(db.max()):.3e})  "
          f"median|c-a| {float(dc.median()):.3e} (torch fp32 {float(db.median()):.3e})")
    assert float(dc.max()) <= 2 * float(db.max()) + LR * 1e-6, what
    assert float(dc.median()) <= 2 * float(db.median()) + LR * 1e-6, what


class _no_sync:
    """torch.cuda.set_sync_debug_mode("error") around a block only."""

    def __enter__(self):
        self.old = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.old)
        return False


def test_step_never_synchronises_with_clipping_or_a_grad_scaler():
    """Form used: ``torch.cuda.set_sync_debug_mode("error")`` -- the ROCm build of torch honours it (the deliberate ``.item()``
    below raises under it, which this test asserts first, so a build that ignored the mode would fail here rather than pass
    vacuously).  Fails on the parent commit at ``float(sq.sqrt())`` / ``float(found_inf)``."""
    model = _fresh_model()
    grads = _gradients(model)
    probe = torch.ones((), device="cuda")
    with _no_sync():
        with pytest.raises(RuntimeError):
            probe.item()
    assert torch.cuda.get_sync_debug_mode() == 0
    opt = ShardedFlatAdam(model.parameters(), lr=LR, max_grad_norm=CLIP)
    _write_grads(model, grads[0])
    with _no_sync():
        opt.step()
    assert opt.last_grad_norm.is_cuda and opt.last_grad_norm.dim() == 0
    # the reference's mixed-precision order (trainer.py:207-217): unscale_ -> clip -> scaler.step
    opt.max_grad_norm = None
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    scaler.scale(torch.zeros((), device="cuda"))              # creates the scale tensor, as scaling a loss does
    _write_grads(model, grads[1], 1024.0)
    with _no_sync():
        scaler.unscale_(opt)
        norm = opt.clip_grad_norm_(CLIP)
        scaler.step(opt)
    scaler.update()
    assert norm.is_cuda and norm.dim() == 0
    # ... and without unscale_: grad_scale reaches the step as a device pointer
    opt.max_grad_norm = CLIP
    _write_grads(model, grads[2], 1024.0)
    with _no_sync():
        scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    assert opt.steps == 3 and all(bool(torch.isfinite(p).all()) for p in model.parameters())


@pytest.mark.parametrize("mode", ["max_grad_norm", "clip_grad_norm_"])
def test_clipped_steps_match_the_reference_optimizer(mode):
    model = _fresh_model()
    grads = _gradients(model)
    params0 = [p.detach().clone() for p in model.parameters()]
    a, norms = _torch_run(params0, grads, torch.float64, "cpu")
    b, _ = _torch_run(params0, grads, torch.float32, "cuda")
    assert sum(n > 1.3 * CLIP for n in norms) >= 2 and sum(n < 0.1 * CLIP for n in norms) >= 2, norms   # both branches of min(1, .)
    opt = ShardedFlatAdam(model.parameters(), lr=LR, max_grad_norm=CLIP if mode == "max_grad_norm" else None)
    assert opt.last_grad_norm is None
    for it, gs in enumerate(grads):
        _write_grads(model, gs)
        if mode == "clip_grad_norm_":
            ret = opt.clip_grad_norm_(CLIP)
            assert ret.is_cuda and ret.dim() == 0 and abs(float(ret) - norms[it]) <= 1e-6 * norms[it]
        opt.step()
        got = float(opt.last_grad_norm)
        print(f"step {it}: norm {norms[it]:.9e} device {got:.9e}")
        assert abs(got - norms[it]) <= 1e-6 * norms[it]
        _within_torch_fp32_error(_vec(model.parameters()), a[it], b[it], f"{mode} step {it}")
    assert opt.steps == STEPS and float(opt.last_grad_nonfinite) == 0.0


def test_hip_path_equals_the_cpu_path_of_the_class_inf_gradient_included():
    """Same gradients through ShardedFlatAdam on CPU tensors and on the device, max_grad_norm set; step 2 carries one ``inf`` and
    there is no scaler: the norm is inf, the coefficient 0, so the inf element turns its own parameter into nan (inf * 0) and every
    other element sees a zero gradient -- on both paths, element for element.  The two float32 paths may differ by what two
    float32 evaluations of the step differ by: twice torch's own float32 error against float64 (the bound of the test above)."""
    model = _fresh_model()
    grads = _gradients(model)
    _poke(grads[2], float("inf"))
    params0 = [p.detach().clone() for p in model.parameters()]
    a, _ = _torch_run(params0, grads, torch.float64, "cpu")
    b, _ = _torch_run(params0, grads, torch.float32, "cuda")
    twin = [torch.nn.Parameter(p.cpu().clone()) for p in params0]
    cpu = ShardedFlatAdam(twin, lr=LR, max_grad_norm=CLIP)
    hip = ShardedFlatAdam(model.parameters(), lr=LR, max_grad_norm=CLIP)
    for it, gs in enumerate(grads):
        _write_grads(model, gs)
        for p, g in zip(twin, gs):
            p.grad.copy_(g)
        cpu.step()
        hip.step()
        c, h = _vec(twin), _vec(model.parameters())
        fin = torch.isfinite(c)
        assert torch.equal(torch.isfinite(h), fin) and torch.equal(torch.isfinite(a[it]), fin)
        assert int((~fin).sum()) == (1 if it >= 2 else 0)
        d, db = (h - c)[fin].abs(), (b[it] - a[it])[fin].abs()
        print(f"step {it}: max|hip-cpu| {float(d.max()):.3e} median {float(d.median()):.3e}; torch fp32 vs fp64 "
              f"{float(db.max()):.3e} / {float(db.median()):.3e}")
        assert float(d.max()) <= 2 * float(db.max()) + LR * 1e-6 and float(d.median()) <= 2 * float(db.median()) + LR * 1e-6
        n_c, n_h = float(cpu.last_grad_norm), float(hip.last_grad_norm)
        assert (n_c == n_h == float("inf")) if it == 2 else abs(n_c - n_h) <= 1e-6 * n_c
    assert float(hip.last_grad_nonfinite) == 0.0 and cpu.steps == hip.steps == STEPS
    # moments too: finite where finite
    for x, y in ((cpu.exp_avg, hip.exp_avg), (cpu.exp_avg_sq, hip.exp_avg_sq)):
        assert torch.equal(torch.isfinite(x), torch.isfinite(y.cpu()))


def test_nan_norm_leaves_the_gradient_unclipped_as_the_cpu_path_does():
    """The pinned rule: Python's ``min(1.0, nan)`` is 1.0, so a nan gradient element (nan norm) means NO clipping -- the step is
    bit for bit the unclipped one, on the device as on CPU tensors."""
    grads = None
    out = {}
    for clip in (CLIP, None):
        model = _fresh_model()
        grads = grads or _gradients(model, amps=(3e-3,))
        _poke(grads[0], float("nan"))
        opt = ShardedFlatAdam(model.parameters(), lr=LR, max_grad_norm=clip)
        _write_grads(model, grads[0])
        opt.step()
        out[clip] = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()
        if clip is not None:
            assert bool(torch.isnan(opt.last_grad_norm)) and float(opt.last_grad_nonfinite) == 1.0
    assert torch.equal(out[CLIP].view(torch.int32), out[None].view(torch.int32))
    assert int(torch.isnan(out[CLIP]).sum()) == 1
    twin = [torch.nn.Parameter(p.detach().cpu().clone()) for p in _fresh_model().parameters()]
    cpu = ShardedFlatAdam(twin, lr=LR, max_grad_norm=CLIP)
    for p, g in zip(twin, grads[0]):
        p.grad.copy_(g)
    cpu.step()
    c = torch.cat([p.detach().reshape(-1) for p in twin])
    h = out[CLIP].cpu()
    assert torch.equal(torch.isnan(c), torch.isnan(h))
    assert float((c - h)[~torch.isnan(c)].abs().max()) <= LR * 1e-3       # an unclipped first Adam step moves every element by ~lr


def _state(opt):
    return [t.clone() for t in (opt.flat.data, opt.exp_avg, opt.exp_avg_sq)]


def test_skipped_steps_touch_nothing_and_do_not_count():
    model = _fresh_model()
    grads = _gradients(model)
    opt = ShardedFlatAdam(model.parameters(), lr=LR, max_grad_norm=CLIP)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    scaler.scale(torch.zeros((), device="cuda"))
    before = _state(opt)
    assert opt.steps == 0
    # found_inf = 1 the way GradScaler sets it: an inf in one gradient element, unscale_, step
    _write_grads(model, grads[0], 1024.0)
    _poke([p.grad for p in model.parameters()], float("inf"))
    scaler.unscale_(opt)
    scaler.step(opt)
    scaler.update()
    assert all(torch.equal(x, y) for x, y in zip(before, _state(opt))) and opt.steps == 0
    assert float(scaler.get_scale()) == 512.0
    # the next, clean step (through the scaler, gradients scaled by its power of two) = step 1 of a fresh optimizer, bit for bit
    _write_grads(model, grads[0], 512.0)
    scaler.step(opt)
    scaler.update()
    fresh_model = _fresh_model()
    fresh = ShardedFlatAdam(fresh_model.parameters(), lr=LR, max_grad_norm=CLIP)
    _write_grads(fresh_model, grads[0])
    fresh.step()
    assert all(torch.equal(x, y) for x, y in zip(_state(fresh), _state(opt))) and opt.steps == fresh.steps == 1
    _write_grads(model, grads[1])
    opt.step()
    # one skipped + two applied steps
    sd = opt.state_dict()
    assert all(float(s["step"]) == 2.0 for s in sd["state"].values()) and opt.steps == 2
    torch_params = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    ref = torch.optim.Adam(torch_params, lr=LR)
    ref.load_state_dict(sd)
    assert float(ref.state[torch_params[0]]["step"]) == 2.0
    assert torch.equal(ref.state[torch_params[1]]["exp_avg"], sd["state"][1]["exp_avg"])
    # a fresh ShardedFlatAdam over the same parameter values continues identically
    cont_model = _fresh_model()
    for p, q in zip(cont_model.parameters(), model.parameters()):
        p.data.copy_(q.data)
    cont = ShardedFlatAdam(cont_model.parameters(), lr=LR, max_grad_norm=CLIP)
    cont.load_state_dict(sd)
    assert cont.steps == 2
    for m, o in ((model, opt), (cont_model, cont)):
        _write_grads(m, grads[2])
        o.step()
    assert all(torch.equal(x, y) for x, y in zip(_state(cont), _state(opt))) and cont.steps == opt.steps == 3


def _host_sumsq(x):
    """The kernels' summation order in numpy float64: chunks of 4096; lane t adds the squares of the 16-byte pieces t, t + 256, ..
    element by element; xor butterfly 32..1 inside each wave of 64 lanes; the four waves in order; then the partials the same way
    (thread t adds partials t, t + 256, ..)."""
    def block(acc):                                   # acc [256] float64 -> the workgroup's sum
        v = acc.reshape(4, 64).copy()
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lanes ^ o]
        return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]

    n = x.size
    chunks = (n + 4095) // 4096
    pad = np.zeros(chunks * 4096, dtype=np.float64)
    pad[:n] = x.astype(np.float64)
    sq = (pad * pad).reshape(chunks, 4, 256, 4)       # [chunk][j][lane][c]
    partial = np.zeros((chunks + 255) // 256 * 256, dtype=np.float64)
    for b in range(chunks):
        acc = np.zeros(256, dtype=np.float64)
        for j in range(4):
            for c in range(4):
                acc = acc + sq[b, j, :, c]
        partial[b] = block(acc)
    acc = np.zeros(256, dtype=np.float64)
    for r in range(partial.size // 256):
        acc = acc + partial[r * 256:(r + 1) * 256]
    return block(acc)


def _device_sumsq(lib, x, scratch, out, flag):
    _lib.check(lib.aft_grad_sumsq_f32(x.data_ptr(), x.numel(), scratch.data_ptr(), scratch.numel(), out.data_ptr(), flag.data_ptr(),
                                      _lib.current_stream_ptr(x.device)))


def test_squared_norm_is_deterministic_and_follows_its_stated_order():
    lib = _lib.load()
    gen = torch.Generator().manual_seed(99)
    n = 1 << 20
    host = torch.randn(n, generator=gen) * torch.logspace(-4, 2, n)         # seven decades: the order of the additions matters
    x = host.cuda()
    scratch = torch.empty(lib.aft_grad_sumsq_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    outs = torch.zeros(21, dtype=torch.float64, device="cuda")
    flag = torch.zeros((), dtype=torch.float32, device="cuda")
    for i in range(20):
        _device_sumsq(lib, x, scratch, outs[i], flag)
    # once more while a large matmul on a second stream occupies the device
    a = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(8):
            a @ a
    _device_sumsq(lib, x, scratch, outs[20], flag)
    torch.cuda.synchronize()
    bits = outs.cpu().view(torch.int64)
    assert len(set(bits.tolist())) == 1, bits
    want = _host_sumsq(host.numpy())
    assert abs(float(outs[0]) - want) <= 1e-15 * want and float(flag) == 0.0
    # n not a multiple of the chunk (nor of 4), and n shorter than one chunk
    for m in (3 * 4096 + 1234 + 1, 1000, 3):
        out = torch.zeros((), dtype=torch.float64, device="cuda")
        _device_sumsq(lib, x[:m], scratch, out, flag)
        want = _host_sumsq(host.numpy()[:m])
        print(f"n {m}: device {float(out):.17e} host {want:.17e}")
        assert abs(float(out) - want) <= 1e-15 * want and float(flag) == 0.0
    # a non-finite element is ordinary data: the flag says so, whichever chunk holds it
    y = x[:3 * 4096 + 64].clone()
    y[2 * 4096 + 7] = float("inf")
    out = torch.zeros((), dtype=torch.float64, device="cuda")
    _device_sumsq(lib, y, scratch, out, flag)
    assert float(out) == float("inf") and float(flag) == 1.0


def test_world_size_one_process_group_places_the_collectives_on_the_device():
    """A world-size-1 RCCL group in a child process: reduce-scatter -> norm -> all-reduce of the device scalar -> preparation ->
    Adam -> all-gather gives the parameters of the same clipped step without a group."""
    import torch.multiprocessing as mp
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_pg_worker, args=(ret,), nprocs=1, join=True)
        err, norm_err, steps = ret[0]
    assert err == 0.0 and norm_err == 0.0 and steps == 2


def _pg_worker(rank, ret):
    import os
    import socket
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    def run():
        torch.manual_seed(0)
        lin = torch.nn.Linear(40, 24).to(dev)
        opt = ShardedFlatAdam(lin.parameters(), lr=1e-2, max_grad_norm=0.5)
        x = torch.randn(16, 40, device=dev)
        for amp in (30.0, 1e-2):
            opt.zero_grad()
            (lin(x).square().mean() * amp).backward()
            opt.step()
        torch.cuda.synchronize()
        return torch.cat([p.detach().reshape(-1) for p in lin.parameters()]).clone(), opt.last_grad_norm.clone(), opt.steps

    alone, norm_alone, _ = run()
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    grouped, norm_grouped, steps = run()
    ret[0] = (float((alone - grouped).abs().max()), float((norm_alone - norm_grouped).abs()), steps)
    dist.barrier()
    dist.destroy_process_group()
