"""ingest.ResidentLoader and ``aft_frame_gather_f32`` on the HIP device: the kernel against ``torch.index_select`` bit for bit, the
loader against its CPU twin, no synchronisation inside an epoch, evaluation and training fed by it, and the checked build."""
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib, ingest
from adafortitran_amd.hip_ops import frame_gather
from test_resident_loader import PS, make_pack

pytestmark = pytest.mark.gpu
DEV = "cuda"


class _no_sync:
    """torch.cuda.set_sync_debug_mode("error") around a block only (the helper form of tests/test_optim_hip.py)."""

    def __enter__(self):
        self.old = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.old)
        return False


def _arrays(n, grid, pilot, seed):
    g = torch.Generator().manual_seed(seed)
    ideal = torch.view_as_complex(torch.randn((n, *grid, 2), generator=g))
    pilots = torch.view_as_complex(torch.randn((n, *pilot, 2), generator=g))
    return ideal, pilots


def _poison(shapes):
    """Leave NaN-filled free blocks of exactly the sizes the gather's three outputs will ask for, and check that the caching allocator
    does hand those blocks to the next requests of these sizes: an output element the kernel leaves unwritten then shows."""
    def blocks(fill):
        out = [torch.empty(shape, dtype=dt, device=DEV) for shape, dt in shapes]
        if fill:
            for t in out:
                (torch.view_as_real(t) if t.is_complex() else t.view(torch.float32)).fill_(float("nan"))
        return out
    junk = blocks(True)
    del junk
    probe = blocks(False)
    assert all(torch.isnan(torch.view_as_real(t) if t.is_complex() else t.view(torch.float32)).all() for t in probe)
    del probe


def _check(ideal_src, pilots_src, ideal_h, pilots_h, index_h, lib=None):
    n = ideal_h.shape[0]
    index = index_h.to(DEV)
    b = index_h.numel()
    _poison([((b, *ideal_h.shape[1:]), torch.complex64), ((b, *pilots_h.shape[1:]), torch.complex64), ((b,), torch.int32)])
    ideal, pilots, flags = frame_gather(ideal_src, pilots_src, index, lib=lib)
    bad = (index_h < 0) | (index_h >= n)
    safe = torch.where(bad, torch.zeros_like(index_h), index_h)
    want_i, want_p = torch.index_select(ideal_h, 0, safe), torch.index_select(pilots_h, 0, safe)
    want_i[bad], want_p[bad] = 0, 0
    assert ideal.shape == want_i.shape and pilots.shape == want_p.shape and flags.dtype == torch.int32
    assert torch.equal(torch.view_as_real(ideal.cpu()).view(torch.int32), torch.view_as_real(want_i).view(torch.int32))
    assert torch.equal(torch.view_as_real(pilots.cpu()).view(torch.int32), torch.view_as_real(want_p).view(torch.int32))
    assert torch.equal(flags.cpu(), bad.to(torch.int32))


GRIDS = [((120, 14), (12, 2)), ((240, 28), (24, 4)), ((3, 5), (3, 1))]     # the last: odd element counts, the 8-byte form


@pytest.mark.parametrize("grid,pilot", GRIDS)
@pytest.mark.parametrize("where", ["hbm", "pinned"])
def test_frame_gather_is_index_select(grid, pilot, where):
    n = 257
    ideal_h, pilots_h = _arrays(n, grid, pilot, seed=grid[0])
    if where == "hbm":
        ideal_src, pilots_src = ideal_h.to(DEV), pilots_h.to(DEV)
    else:
        ideal_src, pilots_src = ideal_h.pin_memory(), pilots_h.pin_memory()
    g = torch.Generator().manual_seed(7)
    for batch in (1, 3, 37, 128, 512):
        index = torch.randint(0, n, (batch,), generator=g)                 # with repeats (certainly at 512 of 257)
        if batch >= 3:
            index[1] = index[0]
        _check(ideal_src, pilots_src, ideal_h, pilots_h, index)
    index = torch.randint(0, n, (37,), generator=g)
    index[0], index[5], index[36], index[17] = -1, n, 1 << 40, n - 1
    _check(ideal_src, pilots_src, ideal_h, pilots_h, index)
    _check(ideal_src, pilots_src, ideal_h, pilots_h, torch.tensor([-(1 << 62), n]))      # nothing but bad entries


def test_frame_gather_with_bases_that_are_only_8_byte_aligned():
    """Even element counts whose bases sit 8 bytes off a 16-byte boundary take the 8-byte form: same frames."""
    n, grid, pilot = 50, (120, 14), (12, 2)
    ideal_h, pilots_h = _arrays(n, grid, pilot, seed=3)
    flat_i = torch.empty(ideal_h.numel() + 1, dtype=torch.complex64, device=DEV)
    flat_p = torch.empty(pilots_h.numel() + 1, dtype=torch.complex64, device=DEV)
    ideal_src, pilots_src = flat_i[1:].view(ideal_h.shape), flat_p[1:].view(pilots_h.shape)
    ideal_src.copy_(ideal_h)
    pilots_src.copy_(pilots_h)
    assert ideal_src.data_ptr() % 16 == 8 and pilots_src.data_ptr() % 16 == 8
    _check(ideal_src, pilots_src, ideal_h, pilots_h, torch.randperm(n)[:33])
    _check(ideal_src, pilots_h.to(DEV), ideal_h, pilots_h, torch.randperm(n)[:33])        # one array of each form in one launch


def test_frame_gather_wrapper_refuses_what_the_kernel_cannot_read():
    ideal_h, pilots_h = _arrays(8, (120, 14), (12, 2), seed=1)
    index = torch.arange(4, device=DEV)
    with pytest.raises(ValueError, match="pinned"):
        frame_gather(ideal_h, pilots_h.to(DEV), index)                     # pageable host memory
    with pytest.raises(ValueError, match="index"):
        frame_gather(ideal_h.to(DEV), pilots_h.to(DEV), index.to(torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        frame_gather(ideal_h.to(DEV)[:, ::2], pilots_h.to(DEV), index)
    with pytest.raises(ValueError, match="frames"):
        frame_gather(ideal_h.to(DEV), pilots_h.to(DEV)[:4], index)


def _same(dev_batches, host_batches):
    assert len(dev_batches) == len(host_batches)
    for (pd, idv, md), (ph, ih, mh) in zip(dev_batches, host_batches):
        assert pd.is_cuda and idv.is_cuda and not md[0].is_cuda
        assert torch.equal(pd.cpu(), ph) and torch.equal(idv.cpu(), ih)
        assert all(torch.equal(a, b) for a, b in zip(md[:5], mh[:5])) and md[5] == mh[5]


@pytest.mark.parametrize("residency", ["device", "pinned"])
def test_loader_on_the_device_equals_its_cpu_twin(residency):
    packed = make_pack(37)
    cap = {} if residency == "device" else {"max_device_bytes": 0}
    for batch, world in ((8, 1), (4, 2)):
        for rank in range(world):
            kw = dict(batch_size=batch, seed=3, rank=rank, world_size=world)
            host = ingest.ResidentLoader(packed, PS, device="cpu", **kw)
            dev = ingest.ResidentLoader(packed, PS, device=DEV, **kw, **cap)
            assert dev.residency == residency and len(dev) == len(host)
            for _ in range(2):
                _same(list(dev), list(host))
            assert dev.epoch == host.epoch == 2
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                got = list(dev)
            side.synchronize()
            _same(got, list(host))
    # a consumer that changes streams inside an epoch: the index upload is ordered in front of the new stream's launches
    host, dev = (ingest.ResidentLoader(packed, PS, 8, device=d, seed=5, **(cap if d == DEV else {})) for d in ("cpu", DEV))
    side, got = torch.cuda.Stream(), []
    for k, batch in enumerate(dev):
        got.append(batch)
        if k == 1:
            torch.cuda.set_stream(side)
    torch.cuda.set_stream(torch.cuda.default_stream())
    torch.cuda.synchronize()
    _same(got, list(host))


def test_pilot_count_error_at_construction_on_the_device():
    packed = make_pack(9)
    packed["h_ls_sparse"][7, 1, 0] = 1.0
    with pytest.raises(ValueError, match=r"Expected 24 pilot values, got 25 \(frame 7\)"):
        ingest.ResidentLoader(packed, PS, 4, device=DEV)


@pytest.mark.parametrize("residency", ["device", "pinned"])
def test_an_epoch_never_synchronises(residency):
    packed = make_pack(37)
    probe = torch.ones((), device=DEV)
    with _no_sync():
        with pytest.raises(RuntimeError):
            probe.item()                                                   # the mode is honoured: the epoch below is not vacuous
    cap = {} if residency == "device" else {"max_device_bytes": 0}
    dev = ingest.ResidentLoader(packed, PS, 8, device=DEV, seed=1, **cap)
    host = ingest.ResidentLoader(packed, PS, 8, device="cpu", seed=1)
    assert dev.residency == residency
    with _no_sync():
        epochs = [list(dev) for _ in range(5)]                             # from the third on, the index slots are re-used
    for got in epochs:
        _same(got, list(host))


def test_evaluation_sweep_over_a_resident_loader(tmp_path):
    import adafortitran_amd as A
    from adafortitran_amd.evaluation import evaluate_dataloader
    from helpers import Golden
    from test_estimators_cpu import _configs
    from test_ingest_eval import _write_tree
    g = Golden("A_ada")
    _write_tree(str(tmp_path))
    ingest.pack_mat_folder(tmp_path / "SNR_10", tmp_path / "p.npz")
    sd = {k: torch.from_numpy(v) for k, v in g.state_dict().items()}
    res = {}
    for dev in ("cpu", "cuda"):
        sc, mc = _configs(g.spec, device=dev)
        model = A.AdaFortiTranEstimator(sc, mc)
        model.load_state_dict(sd)
        res[dev] = evaluate_dataloader(model, ingest.ResidentLoader(str(tmp_path / "p.npz"), PS, 2, device=dev, shuffle=False))
    print(f"MSE cpu {res['cpu']:.9e}  hip {res['cuda']:.9e}  |d|/MSE {abs(res['cuda'] - res['cpu']) / res['cpu']:.3e}")
    assert abs(res["cuda"] - res["cpu"]) <= 1e-4 * res["cpu"]


def test_three_training_steps_fed_by_the_loader_equal_the_host_fed_steps():
    """``tests/test_train_hip.py::test_training_step_soak_same_bits_every_time`` asserts that a training step is bit-reproducible run
    to run, so the parameters after three steps must be EQUAL: the loader hands the step the same bits as the CPU twin's batches moved
    with ``.to("cuda")``."""
    import adafortitran_amd as A
    from adafortitran_amd.optim import ShardedFlatAdam
    packed = make_pack(24, seed=9)
    packed["meta"][:, 1] = np.linspace(0, 30, 24)                          # snr, delay spread, doppler in the ranges the model sees
    packed["meta"][:, 2] = np.linspace(50, 350, 24)
    packed["meta"][:, 3] = np.linspace(200, 1400, 24)
    sc = A.SystemConfig(ofdm=dict(num_scs=120, num_symbols=14), pilot=dict(num_scs=12, num_symbols=2))
    mc = A.ModelConfig(model_type="adafortitran", patch_size=(3, 2), num_layers=2, model_dim=128, num_head=4, device="cuda", dropout=0.1,
                       channel_adaptivity_hidden_sizes=[7, 42, 560], adaptive_token_length=6)

    def train(loader, move):
        torch.manual_seed(4)
        model = A.AdaFortiTranEstimator(sc, mc).train()
        opt = ShardedFlatAdam(model.parameters(), lr=1e-3)
        losses = []
        for k, (pilots, ideal, meta) in enumerate(loader):
            if move:
                pilots, ideal = pilots.to("cuda"), ideal.to("cuda")
            assert pilots.is_cuda and ideal.is_cuda
            torch.manual_seed(100 + k)                                     # the dropout masks of step k
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(torch.view_as_real(model(pilots, meta)), torch.view_as_real(ideal))   # trainer.py:219-222
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        assert k == 2
        return [p.detach().clone() for p in model.parameters()], torch.stack(losses).cpu()

    kw = dict(batch_size=8, seed=6, shuffle=True)
    p_dev, l_dev = train(ingest.ResidentLoader(packed, PS, device="cuda", **kw), move=False)
    p_host, l_host = train(ingest.ResidentLoader(packed, PS, device="cpu", **kw), move=True)
    assert torch.isfinite(l_dev).all() and torch.equal(l_dev, l_host), (l_dev, l_host)
    for i, (a, b) in enumerate(zip(p_dev, p_host)):
        assert torch.equal(a, b), i


def test_checked_build_gathers_the_same_bits():
    import ctypes
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_frame_gather_f32"):   # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)                                             # raises unless every symbol of the table is exported
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_frame_gather_f32")
    ideal_h, pilots_h = _arrays(257, (120, 14), (12, 2), seed=2)
    index = torch.randint(0, 257, (37,), generator=torch.Generator().manual_seed(8))
    index[3] = -1
    _check(ideal_h.to(DEV), pilots_h.to(DEV), ideal_h, pilots_h, index, lib=lib)
    want = frame_gather(ideal_h.to(DEV), pilots_h.to(DEV), index.to(DEV))
    got = frame_gather(ideal_h.to(DEV), pilots_h.to(DEV), index.to(DEV), lib=lib)
    assert all(torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b)
               for a, b in zip(got, want))
