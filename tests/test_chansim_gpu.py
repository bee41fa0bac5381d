"""``aft_channel_sim_f32`` and ``chansim.SynthLoader`` on the HIP device: the kernel against the float64 definition within a bound
DERIVED here from the configuration, meta bit for bit, batch / shard independence bit for bit, no unwritten output, the checked build,
the entry point's refusals, and the loader feeding evaluation and training without a synchronisation.

The bound (``derived_bounds``).  u = 2^-24 is float32's unit roundoff; every float32 operation below errs by at most u times its
result; sincospi / cospi err by at most 4 ulp and log by 3 ulp (the OpenCL full-profile limits the device library is built to), an
ulp of a value below 1 being at most u; sqrt is correctly rounded.  A = max f_D T_sym (turns per symbol), X = the largest delay turn
count (S - 1) max(df DS) max(d_p), M rays, P taps, G = sum_{p,m} sqrt(pw_p / M) = M sum_p amp_p:

* angle turn a = (m + u20) / M: m + u20 is exact (24 bits), the division rounds once: |da| <= u.  cos(2 pi a): argument 2 pi u, function
  4 u.  rate = A' cos: d rate <= A ((2 pi + 4) u + u).
* phase in turns th = fma(rate, t, phi): |d th| <= t_max d rate + u (A t_max + 1); x - floor(x) and the doubling are exact; the sincospi
  of it errs by 2 pi |d th| from its argument and 4 sqrt(2) u of its own:  e_ray = 2 pi |d th| + 4 sqrt(2) u.
* tap gain: M such terms summed in sequence (partial sums at most M: sqrt(2) M (M - 1) u) and scaled by amp_p (sqrt(2) M u):
  |d h_p| <= amp_p M (e_ray + sqrt(2) M u).
* delay phasor: c_p = tau d_p and x = s c_p round once each, |dx| <= 2 u X:  e_del = 4 pi u X + 4 sqrt(2) u.
* the sum over taps: two fused multiply-adds per component and tap, each rounding a partial sum of at most G: 2 sqrt(2) P u G.
  |dH| <= G (e_ray + sqrt(2) M u + e_del + 2 sqrt(2) P u).
* pilots: the same with t_max the last pilot symbol, plus the noise r z, r = sigma sqrt(-ln u1) <= sigma sqrt(24 ln 2): -ln u1 to
  3 ulp = 6 u relative, its root halves that, the product with sigma adds u: 4 u relative; z to 4 sqrt(2) u; the final fused
  multiply-add rounds a value of at most G + r: sqrt(2) u (G + r).
The comparison is against the float64 definition itself (not rounded to float32).  Observed maxima are printed; DESIGN.md records them."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib, chansim, ingest
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, make_pack, simulate_frames_host
from adafortitran_amd.hip_ops import ChannelSimPlan

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def derived_bounds(cfg: ChannelSimConfig):
    """(bound on |ideal - definition|, bound on |pilots - definition|), absolute, per complex element; module docstring."""
    t = cfg.tables()
    S, T = cfg.ofdm
    M, P = cfg.rays, len(t["tap_delay"])
    A = float(t["doppler_turns"].max())
    X = (S - 1) * float(t["delay_turns"].max()) * float(t["tap_delay"].max())
    G = M * float(t["tap_amp"].astype(np.float64).sum())
    r2 = np.sqrt(2.0)

    def channel(t_max):
        d_rate = A * ((2 * np.pi + 4) * U + U)
        d_theta = t_max * d_rate + U * (A * t_max + 1)
        e_ray = 2 * np.pi * d_theta + 4 * r2 * U
        e_del = 4 * np.pi * U * X + 4 * r2 * U
        return G * (e_ray + r2 * M * U + e_del + 2 * r2 * P * U)

    r = float(t["noise_sigma"].max()) * np.sqrt(24 * np.log(2.0))
    noise = r * (4 * U + 4 * r2 * U) + r2 * U * (G + r)
    return channel(T - 1), channel(max(cfg.pilot_symbols)) + noise


class _no_sync:
    """torch.cuda.set_sync_debug_mode("error") around a block only (the helper form of tests/test_optim_hip.py)."""

    def __enter__(self):
        self.old = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.old)
        return False


def _shapes(cfg, b):
    return [((b, *cfg.ofdm), torch.complex64), ((b, *cfg.pilot), torch.complex64), ((b, 3), torch.float32)]


def _poison(shapes):
    """Leave NaN-filled free blocks of exactly the sizes the three outputs will ask for, and check that the caching allocator does hand
    those blocks to the next requests of these sizes: an output element the kernel leaves unwritten then shows."""
    def blocks(fill):
        out = [torch.empty(shape, dtype=dt, device=DEV) for shape, dt in shapes]
        if fill:
            for t in out:
                (torch.view_as_real(t) if t.is_complex() else t).fill_(float("nan"))
        return out
    junk = blocks(True)
    del junk
    probe = blocks(False)
    assert all(torch.isnan(torch.view_as_real(t) if t.is_complex() else t).all() for t in probe)
    del probe


def _bits(t: torch.Tensor) -> torch.Tensor:
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32).cpu()


def _same_bits(a, b):
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


_DENSE = ChannelSimConfig(ofdm=(64, 10), pilot=(8, 2), profile=np.stack([0.25 * np.arange(32), -0.4 * np.arange(32)], axis=1), rays=16,
                          snr_db=np.linspace(-5, 40, 16), delay_spread_ns=np.linspace(10, 1000, 16), doppler_hz=np.linspace(0, 3000, 16))
CONFIGS = {
    "default_120x14": ChannelSimConfig(),
    "240x28": ChannelSimConfig(ofdm=(240, 28), pilot=(24, 4)),
    "long_72x80": ChannelSimConfig(ofdm=(72, 80), pilot=(6, 4)),
    "pilot_lists": ChannelSimConfig(pilot=(4, 3), pilot_scs=(0, 7, 118, 119), pilot_symbols=(0, 1, 13)),
    "odd_30x7": ChannelSimConfig(ofdm=(30, 7), pilot=(3, 1)),               # odd T: the 8-byte store form
    "tables_at_their_bounds": _DENSE,
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_kernel_against_the_float64_definition(name):
    cfg = CONFIGS[name]
    plan = ChannelSimPlan(cfg, DEV)
    b_ideal, b_pilots = derived_bounds(cfg)
    worst = [0.0, 0.0]
    for seed, base, batch in ((1, 0, 1), (1, 5, 37), (2, 1 << 33, 128)):
        _poison(_shapes(cfg, batch))
        ideal, pilots, meta = plan(seed, base, 0, 1, 1 << 40, batch)
        frames = base + np.arange(batch)
        want_i, want_p, want_m = simulate_frames_host(cfg, seed, frames)
        assert ideal.shape == want_i.shape and pilots.shape == want_p.shape and ideal.dtype == pilots.dtype == torch.complex64
        assert torch.equal(_bits(meta), _bits(torch.from_numpy(want_m)))
        got_i, got_p = ideal.cpu().numpy().astype(np.complex128), pilots.cpu().numpy().astype(np.complex128)
        assert np.isfinite(got_i).all() and np.isfinite(got_p).all()         # nothing left unwritten
        worst = [max(worst[0], float(np.abs(got_i - want_i).max())), max(worst[1], float(np.abs(got_p - want_p).max()))]
    print(f"{name}: max|ideal - def| {worst[0]:.3e} (derived bound {b_ideal:.3e})   max|pilots - def| {worst[1]:.3e} (derived bound "
          f"{b_pilots:.3e})")
    assert worst[0] <= b_ideal and worst[1] <= b_pilots


def test_the_8_byte_store_form_on_a_base_off_16_bytes():
    """The caching allocator only hands out 512-byte aligned blocks; a base 8 bytes off goes through the entry point directly."""
    cfg = ChannelSimConfig()
    lib, sim, b = _lib.load(), cfg.to_struct(), 5
    want = ChannelSimPlan(cfg, DEV)(3, 0, 0, 1, 100, b)
    flat = torch.full((b * 120 * 14 + 1,), float("nan"), dtype=torch.complex64, device=DEV)
    pilots, meta = torch.empty((b, 12, 2), dtype=torch.complex64, device=DEV), torch.empty((b, 3), device=DEV)
    assert (flat.data_ptr() + 8) % 16 == 8
    _lib.check(lib.aft_channel_sim_f32(sim, 3, 0, 0, 1, 100, b, flat.data_ptr() + 8, pilots.data_ptr(), meta.data_ptr(),
                                       _lib.current_stream_ptr(flat.device)))
    _same_bits((flat[1:].view(b, 120, 14), pilots, meta), want)


@pytest.mark.parametrize("name", ["default_120x14", "long_72x80", "odd_30x7"])
def test_a_frame_does_not_depend_on_its_batch_or_its_rank(name):
    cfg = CONFIGS[name]
    plan = ChannelSimPlan(cfg, DEV)
    far = 1 << 40
    whole = plan(5, 0, 0, 1, far, 128)
    for cuts in ((0, 37, 128), (0, 1, 2, 66, 127, 128)):
        parts = [plan(5, 0, lo, 1, far, hi - lo) for lo, hi in zip(cuts, cuts[1:])]
        _same_bits([torch.cat([p[k] for p in parts]) for k in range(3)], whole)
    _same_bits(plan(5, 100, 0, 1, far, 28), [w[100:] for w in whole])            # base
    for world in (2, 8):
        for rank in range(world):
            share = plan(5, 0, rank, world, 128, 128 // world)
            _same_bits(share, [w[rank::world] for w in whole])
    wrapped = plan(5, 0, 120, 3, 128, 6)                                         # positions 120, 123, 126, 129 -> 1, 4, 7
    _same_bits(wrapped, [w[[120, 123, 126, 1, 4, 7]] for w in whole])


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_channel_sim_f32"):   # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_channel_sim_f32")
    for name in ("default_120x14", "long_72x80", "pilot_lists", "odd_30x7", "tables_at_their_bounds"):
        plan = ChannelSimPlan(CONFIGS[name], DEV)
        _same_bits(plan(9, 3, 1, 2, 77, 41, lib=lib), plan(9, 3, 1, 2, 77, 41))


def test_every_refusal_of_the_entry_point_launches_nothing():
    lib, cfg, b = _lib.load(), ChannelSimConfig(), 4
    outs = [torch.empty(s, dtype=dt, device=DEV) for s, dt in _shapes(cfg, b)]
    for t in outs:
        (torch.view_as_real(t) if t.is_complex() else t).fill_(float("nan"))
    ptr = [t.data_ptr() for t in outs]

    def refused(code, word, sim=None, seed=1, base=0, start=0, stride=1, modulo=10, batch=b, ideal=ptr[0], pilots=ptr[1], meta=ptr[2]):
        rc = lib.aft_channel_sim_f32(sim if sim is not None else cfg.to_struct(), seed, base, start, stride, modulo, batch, ideal, pilots,
                                     meta, None)
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    rc = lib.aft_channel_sim_f32(None, 1, 0, 0, 1, 10, b, *ptr, None)
    assert rc == E and "NULL" in lib.aft_last_error().decode()
    for k in ("ideal", "pilots", "meta"):
        refused(E, "NULL", **{k: None})
    refused(E, "8-byte", ideal=ptr[0] + 4)
    refused(E, "8-byte", pilots=ptr[1] + 4)
    refused(E, "4-byte", meta=ptr[2] + 2)
    for batch in (0, -3):
        refused(E, "batch must be at least 1", batch=batch)
    for kw in (dict(base=-1), dict(start=-1), dict(stride=0), dict(modulo=0), dict(base=1 << 62), dict(start=1 << 61, stride=1 << 61)):
        refused(E, "bad frame numbers", **kw)
    for field, value, word in (("taps", 33, "taps = 33 is outside 1..32"), ("taps", 0, "taps = 0"), ("rays", 17, "rays = 17 is outside 1..16"),
                               ("n_snr", 17, "n_snr = 17"), ("n_ds", 0, "n_ds = 0"), ("n_dop", 17, "n_dop = 17"),
                               ("pilot_scs", 65, "pilot_scs = 65 is outside 1..64"), ("pilot_symbols", 17, "pilot_symbols = 17"),
                               ("num_scs", 0, "num_scs = 0"), ("num_symbols", -1, "num_symbols = -1")):
        sim = cfg.to_struct()
        setattr(sim, field, value)
        refused(SH, word, sim=sim)
    sim = cfg.to_struct()
    sim.pilot_sc_index[11] = 120
    refused(SH, "pilot_sc_index[11] = 120 is outside the grid's 120 subcarriers", sim=sim)
    sim = cfg.to_struct()
    sim.pilot_symbol_index[0] = -1
    refused(SH, "pilot_symbol_index[0] = -1", sim=sim)
    torch.cuda.synchronize()
    assert all(torch.isnan(torch.view_as_real(t) if t.is_complex() else t).all() for t in outs)      # nothing was launched
    assert lib.aft_channel_sim_f32(cfg.to_struct(), 1, 0, 0, 1, 10, b, *ptr, None) == _abi.AFT_OK
    torch.cuda.synchronize()
    assert all(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all() for t in outs)   # ... and the good call writes it all
    with pytest.raises(ValueError, match="HIP device"):
        ChannelSimPlan(cfg, "cpu")


@pytest.mark.parametrize("world,fresh,drop_last", [(1, True, False), (2, False, False), (8, True, True)])
def test_loader_on_the_device_matches_its_cpu_twin_without_a_synchronisation(world, fresh, drop_last):
    cfg = ChannelSimConfig()
    b_ideal, b_pilots = derived_bounds(cfg)
    probe = torch.ones((), device=DEV)
    with _no_sync():
        with pytest.raises(RuntimeError):
            probe.item()                                                         # the mode is honoured: the epochs below are not vacuous
    for rank in {0, world - 1}:
        kw = dict(batch_size=8, frames_per_epoch=37, seed=4, rank=rank, world_size=world, drop_last=drop_last, fresh_each_epoch=fresh)
        dev, host = SynthLoader(cfg, device=DEV, **kw), SynthLoader(cfg, device="cpu", **kw)
        assert len(dev) == len(host)
        with _no_sync():
            epochs = [list(dev) for _ in range(3)]
        assert dev.epoch == 3
        for got in epochs:
            want = list(host)
            assert len(got) == len(want) == len(dev)
            for (pd, idv, md), (ph, ih, mh) in zip(got, want):
                assert pd.is_cuda and idv.is_cuda and not md[0].is_cuda and pd.dtype == idv.dtype == torch.complex64
                assert pd.shape == ph.shape and idv.shape == ih.shape
                assert all(torch.equal(x, y) for x, y in zip(md[:5], mh[:5])) and md[5] == mh[5]
                # the twin's batch is the definition ROUNDED to complex64: u per component of a value of at most G (G + r for a pilot)
                G = cfg.rays * float(cfg.tables()["tap_amp"].astype(np.float64).sum())
                r = float(cfg.tables()["noise_sigma"].max()) * np.sqrt(24 * np.log(2.0))
                assert float((idv.cpu() - ih).abs().max()) <= b_ideal + np.sqrt(2.0) * U * G
                assert float((pd.cpu() - ph).abs().max()) <= b_pilots + np.sqrt(2.0) * U * (G + r)


def test_training_steps_fed_by_the_loader_never_synchronise():
    import adafortitran_amd as A
    from adafortitran_amd.optim import ShardedFlatAdam
    sc = A.SystemConfig(ofdm=dict(num_scs=120, num_symbols=14), pilot=dict(num_scs=12, num_symbols=2))
    mc = A.ModelConfig(model_type="adafortitran", patch_size=(3, 2), num_layers=2, model_dim=128, num_head=4, device="cuda", dropout=0.1,
                       channel_adaptivity_hidden_sizes=[7, 42, 560], adaptive_token_length=6)
    torch.manual_seed(4)
    model = A.AdaFortiTranEstimator(sc, mc).train()
    opt = ShardedFlatAdam(model.parameters(), lr=1e-3)
    loader = SynthLoader(ChannelSimConfig(), 16, 16 * 7, device=DEV, seed=1)

    def step(pilots, ideal, meta):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(torch.view_as_real(model(pilots, meta)), torch.view_as_real(ideal))   # trainer.py:219-222
        loss.backward()
        opt.step()
        return loss.detach()

    it = iter(loader)
    losses = [step(*next(it))]                                                   # the first step allocates workspaces: outside the guard
    torch.cuda.synchronize()
    with _no_sync():
        for batch in it:
            losses.append(step(*batch))
    losses = torch.stack(losses).cpu()
    print("losses", [round(float(v), 5) for v in losses])
    assert len(losses) == 7 and torch.isfinite(losses).all()


def test_evaluation_sweep_over_a_simulated_pack():
    import adafortitran_amd as A
    from adafortitran_amd.evaluation import evaluate_dataloader
    from helpers import Golden
    from test_estimators_cpu import _configs
    g = Golden("A_ada")
    cfg = ChannelSimConfig()
    pack = make_pack(cfg, 10, seed=3, snr_db=10)
    sd = {k: torch.from_numpy(v) for k, v in g.state_dict().items()}
    res = {}
    for dev in ("cpu", "cuda"):
        sc, mc = _configs(g.spec, device=dev)
        model = A.AdaFortiTranEstimator(sc, mc)
        model.load_state_dict(sd)
        res[dev] = evaluate_dataloader(model, ingest.ResidentLoader(pack, cfg.pilot, 4, device=dev, shuffle=False))
        res[dev + "_packed"] = evaluate_dataloader(model, ingest.PackedLoader(pack, cfg.pilot, 4, device=dev))
    print(f"MSE cpu {res['cpu']:.9e}  hip {res['cuda']:.9e}  |d|/MSE {abs(res['cuda'] - res['cpu']) / res['cpu']:.3e}")
    assert abs(res["cuda"] - res["cpu"]) <= 1e-4 * res["cpu"]                    # the bound of the existing ingest test
    assert abs(res["cuda_packed"] - res["cpu"]) <= 1e-4 * res["cpu"] and abs(res["cpu_packed"] - res["cpu"]) <= 1e-4 * res["cpu"]
    ls = ingest.ls_mse_db_per_frame(torch.from_numpy(pack["h_ls_full"]).to(DEV), torch.from_numpy(pack["h_ideal"]).to(DEV)).cpu()
    ls_host = ingest.ls_mse_db_per_frame(torch.from_numpy(pack["h_ls_full"]), torch.from_numpy(pack["h_ideal"]))
    assert torch.allclose(ls, ls_host, atol=1e-3) and torch.isfinite(ls).all()
